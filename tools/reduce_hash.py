#!/usr/bin/env python
"""sha256 over the raw bytes of every output of the entry points whose reductions come from gsr_reduce.h, on the smallest cases that
reach each path (one wave group, ragged sizes, more partials than the finisher has threads, NaN and signed zeros where a join could
tell) -- to show that two builds (GSR_LIB) give the same BITS.  Inputs come from numpy generators with fixed seeds.
usage: GSR_LIB=... python tools/reduce_hash.py [--json FILE]"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd import frames, loss_utils, lpips, metrics, scene_init, simple_knn  # noqa: E402

DEV = "cuda"
PICTURES = ((16, 32), (40, 70), (160, 288))  # one 32x16 tile per channel; partial tiles; 270 partials > the finisher's 256 threads


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def cases():
    for H, W in PICTURES:
        r = np.random.default_rng(H * 1000 + W)
        img, gt, wgt = (r.random((3, H, W), dtype=np.float32) for _ in range(3))
        x = dev(img).requires_grad_(True)
        loss, l1, ss = loss_utils.rgb_loss(x, dev(gt), dev(wgt[:1]), return_parts=True)
        loss.backward()
        yield f"rgb_loss 3x{H}x{W}", digest(loss, l1, ss, x.grad)

    # the launcher takes ceil(H W / 256) workgroups, 512 at the most: 1, 8 (ragged), 257 > the finisher's 256 threads
    for H, W in ((16, 16), (37, 53), (257, 256)):
        r = np.random.default_rng(H * 1000 + W + 1)
        d, y = r.random((H, W), dtype=np.float32) + 0.5, r.random((H, W), dtype=np.float32) + 0.5
        m, g = (r.random((H, W)) < 0.8).astype(np.float32), (r.random((H, W)) < 0.9).astype(np.float32)
        x = dev(d).requires_grad_(True)
        loss, parts = loss_utils.depth_loss(x, dev(y), dev(m), dev(m), dev(g), 0.7, 0.3, return_parts=True)
        loss.backward()
        yield f"depth_loss {H}x{W}", digest(loss, parts, x.grad)

    for H, W in PICTURES:
        r = np.random.default_rng(H * 1000 + W + 2)
        pred, gt = r.random((2, 3, H, W), dtype=np.float32), r.random((2, 3, H, W), dtype=np.float32)
        mask = r.random((2, 1, H, W)) < 0.6
        nan = pred.copy()
        nan[0, 1, H // 2, W // 3] = np.nan
        for name, p, m in (("plain", pred, None), ("mask", pred, mask), ("nan", nan, None)):
            out = metrics.image_metrics(dev(p), dev(gt), None if m is None else dev(m))
            yield f"image_metrics 2x3x{H}x{W} {name}", digest(*out)

    for H, W in ((25, 40), (1, 3 * 4096 + 5), (1025, 1025)):  # HW = 1000; three chunks and five; 257 chunks
        r = np.random.default_rng(H * 1000 + W + 3)
        d, y = r.standard_normal((2, H, W)).astype(np.float32), r.standard_normal((2, H, W)).astype(np.float32)
        m = (r.random((2, H, W)) < 0.7).astype(np.float32)
        d.reshape(2, -1)[:, 5::97] = 0.0
        d.reshape(2, -1)[:, 9::101] = -0.0
        y.reshape(2, -1)[:, 7::89] = -0.0
        d[1].reshape(-1)[H * W // 2] = np.nan
        yield f"frame_stats 2x{H}x{W}", digest(*frames.frame_stats(dev(d), dev(y), dev(m)))

    model = lpips.LPIPS.random(seed=3, device=DEV)
    for H, W in ((lpips.MIN_SIZE, lpips.MIN_SIZE), (264, 256)):  # the smallest the entry point takes; 264 spatial partials > 256
        r = np.random.default_rng(H * 1000 + W + 4)
        a, b = r.random((2, 3, H, W), dtype=np.float32), r.random((2, 3, H, W), dtype=np.float32)
        mask = r.random((2, H, W)) < 0.5
        for name, m in (("plain", None), ("mask", dev(mask))):
            out = lpips._run(model, dev(a), dev(b), m, True, spatial=True, core="hip")
            yield f"lpips 2x3x{H}x{W} {name}", digest(out["plain"], out["layers"], out["masked"], out["spatial"])

    for P in (65, 257, 4097):
        pts = np.random.default_rng(P).standard_normal((P, 3)).astype(np.float32)
        pts[3] = (0.0, -0.0, 0.0)
        yield f"distCUDA2 {P}", digest(simple_knn.distCUDA2(dev(pts)))

    for N in (65, 257, 1000):
        pts = np.random.default_rng(N + 5).random((N, 3), dtype=np.float32)
        s = scene_init.create_from_pcd(dev(pts), voxel_size=0.05)
        yield f"create_from_pcd {N}", digest(s._anchor, s._offset, s._anchor_feat, s._scaling, s._rotation, s._opacity, s._uncertainty,
                                             s.max_radii2D, s.xyz_max, s.dist2)
        bad = pts.copy()
        bad[N // 2, 1] = np.inf  # the flags join across the waves; the entry point still fills `info`
        out, info = scene_init._voxelize_hip(dev(bad), 0.05)
        yield f"voxelize_sample {N} one point non-finite", digest(info[:2])
        try:
            scene_init.create_from_pcd(dev(bad), voxel_size=0.05)
            said = "no error"
        except ValueError as e:
            said = str(e)
        yield f"create_from_pcd {N} one point non-finite", hashlib.sha256(said.encode()).hexdigest()
        out, info = scene_init._voxelize_hip(dev(pts), 0.05)
        yield f"voxelize_sample {N}", digest(out[:int(info[0])], info[:2])


def main():
    got = {}
    for name, h in cases():
        got[name] = h
        print(f"{name:48s} {h}", flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(got, f, indent=1)


if __name__ == "__main__":
    main()
