"""Golden vectors for the normals of render_set, produced by RUNNING the reference's own two functions.

    python tests/golden/make_reference_vectors7.py        # needs /root/reference; runs on the CPU

train.py cannot be imported (it pulls wandb, lpips, cv2, the dataset readers and parses arguments), so only the two FunctionDef
nodes `depth2pcd_fromplane` (:252-267) and `least_square_normal_regress_fast01` (:270-298) are taken out of its syntax tree and
compiled in place, into a namespace that holds `torch` and `F`; nothing of the reference is copied, only inputs and the tensors it
returned are stored (ref_normals.npz).  One redirection: `.cuda()` stays on the CPU, as in make_reference_vectors5.

Per case, prefix "<case>/": depth [h,w], K [3,3], c2w [3,4] (fp32); points = the fp32 point map the reference produced [3,h,w];
normals_ref32 = the reference on it in fp32; normals_ref64 = the reference, unmodified, called with that fp32 point map cast to
fp64 and an fp64 eye / ones (both [1,3,w,h], the reference's return layout).

  benign      40x48, focal 38: a smooth slanted surface at depth 3 .. 5, a x1.4 depth step along a diagonal (the gamma mask fires
              on a few percent of the window points) and a block of depth 0 (constant points: rank-1 A, det = 0)
  near        37x53, focal 800, depth ~ 0.25 on a steep slant whose plane passes 0.6 from the origin: det < eps for about half the pixels
  real_focal  24x31, focal 800, depth ~ 1: the regime in which normals_ref32 is rounding noise -- stored to document that, never
              used as an expected value
  tiny        5x7: the window is larger than the image

The inputs are checked here with the tests' own oracle (tests/normals_helpers.py): no window point has ||dz/zc| - gamma| < 1e-5 and
no pixel has |det/eps - 1| < 1e-6, so that the reference's fp32 and fp64 runs and the kernel take the same decisions and no test
excludes a pixel.  The figures printed at the end (fp32 against fp64, oracle against fp64) are the ones INTEGRATION Q quotes.
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF_TRAIN = "/root/reference/train.py"
NAMES = ("depth2pcd_fromplane", "least_square_normal_regress_fast01")
SIZE, GAMMA, EPS = 9, 0.15, 1e-5


def load_reference_functions():
    tree = ast.parse(open(REF_TRAIN).read(), REF_TRAIN)
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert [n.name for n in tree.body] == list(NAMES)
    ns = {"torch": torch, "F": F}
    exec(compile(tree, REF_TRAIN, "exec"), ns)
    return ns[NAMES[0]], ns[NAMES[1]]


def case_inputs(name):
    from normals_helpers import rotation
    if name == "benign":
        h, w, f = 40, 48, 38.0
        i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        depth = 4.0 + 0.018 * (j - 24) + 0.014 * (i - 20) + 0.12 * np.sin(0.21 * i + 0.4) * np.cos(0.17 * j)
        depth = np.where(i * 1.3 + j > 62.5, depth * 1.4, depth)
        depth[6:19, 4:18] = 0.0
        R, t = rotation(0.12, -0.18, 0.07), [0.05, -0.03, 0.04]
    elif name == "near":
        h, w, f = 37, 53, 800.0
        i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        depth = 0.25 + 0.0036 * (j - 26) + 0.0006 * (i - 18) + 0.002 * np.sin(0.3 * i) * np.cos(0.23 * j)
        R, t = rotation(0.1, 0.25, -0.05), [-0.572, 0.068, 0.255]
    elif name == "real_focal":
        h, w, f = 24, 31, 800.0
        i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        depth = 1.0 + 0.003 * (j - 15) - 0.002 * (i - 12) + 0.004 * np.sin(0.5 * i + 0.3 * j)
        R, t = rotation(-0.2, 0.15, 0.3), [2.0, 0.5, -1.5]
    elif name == "tiny":
        h, w, f = 5, 7, 9.0
        i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        depth = 2.0 + 0.11 * j - 0.07 * i + 0.05 * i * j / 7.0
        R, t = rotation(0.2, 0.1, -0.1), [0.2, 0.3, 0.1]
    else:
        raise ValueError(name)
    K = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1]], np.float32)
    c2w = np.concatenate([R, np.asarray(t, np.float64)[:, None]], 1).astype(np.float32)
    return depth.astype(np.float32), K, c2w


def angle(a, b):
    return np.arccos(np.clip((a * b).sum(-1), -1.0, 1.0))


def run_case(fns, name):
    from normals_helpers import from_reference_layout, normal_tol, normals_oracle
    depth2pcd, regress = fns
    depth, K, c2w = case_inputs(name)
    h, w = depth.shape
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with torch.no_grad():
            pts = depth2pcd(depth2d=torch.from_numpy(depth)[None], c2w=torch.from_numpy(c2w), K=torch.from_numpy(K), h=h, w=w)
            assert pts.dtype == torch.float32 and tuple(pts.shape) == (1, 3, h, w)
            ref32 = regress(pts.clone(), torch.eye(3), torch.ones([h * w, SIZE ** 2, 1]))
            ref64 = regress(pts.double(), torch.eye(3, dtype=torch.float64), torch.ones([h * w, SIZE ** 2, 1], dtype=torch.float64))
    finally:
        torch.Tensor.cuda = real_cuda
    assert tuple(ref32.shape) == tuple(ref64.shape) == (1, 3, w, h) and ref64.dtype == torch.float64
    points = pts[0].numpy()
    o = normals_oracle(points, SIZE, GAMMA, EPS)
    assert o["margin"].min() >= 1e-5, (name, "a window point sits on the gamma threshold", o["margin"].min())
    assert np.abs(o["det"] / EPS - 1.0).min() >= 1e-6, (name, "a determinant sits on eps")
    n32, n64 = from_reference_layout(ref32.numpy()).astype(np.float64), from_reference_layout(ref64.numpy())
    a = angle(n32, n64)
    dev = np.abs(o["normals"] - n64)
    print(f"{name}: {h}x{w}  det<eps on {np.mean(o['det'] < EPS):.3f} of the pixels, mask zeroes {o['dropped'].sum() / (h * w * SIZE ** 2):.3f} "
          f"of the window points, cond median {np.median(o['cond']):.3g} max {o['cond'].max():.3g}; "
          f"closest |dz/zc| to gamma {o['margin'].min():.3g}, closest det/eps to 1 {np.abs(o['det'] / EPS - 1.0).min():.3g}, |p| max {np.abs(points).max():.3g}")
    print(f"    reference fp32 against fp64: angle median {np.median(a):.3g} p99 {np.percentile(a, 99):.3g} max {a.max():.3g} rad; "
          f"component max {np.abs(n32 - n64).max():.3g}")
    print(f"    oracle against reference fp64: component max {dev.max():.3g}, largest share of the tolerance {(dev / normal_tol(o['cond'], SIZE)).max():.3g}")
    return {f"{name}/depth": depth, f"{name}/K": K, f"{name}/c2w": c2w, f"{name}/points": points,
            f"{name}/normals_ref32": ref32.numpy().copy(), f"{name}/normals_ref64": ref64.numpy().copy()}


def main():
    fns = load_reference_functions()
    cases = ("benign", "near", "real_focal", "tiny")
    out = {}
    for name in cases:
        out.update(run_case(fns, name))
    out["cases"] = np.array(cases)
    out["settings"] = np.array([SIZE, GAMMA, EPS])
    path = os.path.join(HERE, "ref_normals.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
