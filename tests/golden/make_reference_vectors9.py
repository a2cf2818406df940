"""Golden vectors for render_set's output frames, produced by RUNNING the reference's compute_scale_and_shift and matplotlib's imsave.

    python tests/golden/make_reference_vectors9.py        # needs /root/reference and matplotlib; runs on the CPU

train.py cannot be imported (it pulls wandb, lpips, cv2, the dataset readers and parses arguments), so only the FunctionDef node
`compute_scale_and_shift` (:198-218) is taken out of its syntax tree and compiled in place, into a namespace that holds `torch`, as
make_reference_vectors7 does; nothing of the reference is copied, only inputs and returned values are stored (ref_frames.npz).

Per fit case, prefix "<case>/": depth, target, mask [1,h,w] fp32; scale32 / shift32 = the reference in fp32 (scale before render_set's
abs), scale64 / shift64 = the reference, unmodified, on the same values cast to fp64; panel [h,2w] fp32 = render_set's :784-788 on the
fp32 run, torch.cat((depth * |scale| + shift, target)) laid out as make_grid(padding=0) lays it out; imsave [h,2w,4] uint8 = the bytes
plt.imsave(cmap="viridis") writes for that panel (written to a BytesIO as PNG, decoded with PIL).

  slanted   12x16: a slanted depth with a ripple, an affine target with noise, a 0 / 1 mask that drops ~30 %
  inverse   9x11: the target falls where the depth rises (the fit's scale is negative: render_set's abs matters), a full mask
  empty     5x7: an all-zero mask: det = 0, scale = shift = 0, so the aligned half is constant 0

and two panels alone, "constant/..." (every value 0.75: vmin == vmax) and "nan/..." (one NaN: matplotlib colours the whole picture
(0, 0, 0, 0)).  "versions" records matplotlib's and numpy's versions.  The oracle of tests/frames_helpers.py is checked against the
stored bytes here, before the file is written.
"""
import ast
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF_TRAIN = "/root/reference/train.py"
NAME = "compute_scale_and_shift"


def load_reference_function():
    tree = ast.parse(open(REF_TRAIN).read(), REF_TRAIN)
    tree.body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == NAME]
    assert [n.name for n in tree.body] == [NAME]
    ns = {"torch": torch}
    exec(compile(tree, REF_TRAIN, "exec"), ns)
    return ns[NAME]


def case_inputs(name):
    rng = np.random.default_rng({"slanted": 1, "inverse": 2, "empty": 3}[name])
    h, w = {"slanted": (12, 16), "inverse": (9, 11), "empty": (5, 7)}[name]
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    depth = 3.0 + 0.11 * j - 0.07 * i + 0.3 * np.sin(0.5 * i + 0.3 * j)
    if name == "slanted":
        target, mask = 0.41 * depth + 0.6 + 0.05 * rng.standard_normal((h, w)), (rng.random((h, w)) > 0.3)
    elif name == "inverse":
        target, mask = -0.8 * depth + 6.0 + 0.05 * rng.standard_normal((h, w)), np.ones((h, w), bool)
    else:
        target, mask = 0.5 * depth + 0.1 * rng.standard_normal((h, w)), np.zeros((h, w), bool)
    return depth.astype(np.float32)[None], target.astype(np.float32)[None], mask.astype(np.float32)[None]


def imsave_bytes(panel):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from PIL import Image
    buf = io.BytesIO()
    plt.imsave(buf, panel, cmap="viridis", format="png")
    buf.seek(0)
    out = np.array(Image.open(buf))
    assert out.dtype == np.uint8 and out.shape == panel.shape + (4,), (out.dtype, out.shape)
    return out


def main():
    import matplotlib
    from frames_helpers import aligned, cmap_mpl, extrema
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from gscream_amd.frames import colormap_lut
    fit = load_reference_function()
    lut = colormap_lut("viridis").numpy()
    out, cases = {}, ("slanted", "inverse", "empty")
    for name in cases:
        depth, target, mask = case_inputs(name)
        d, y, m = (torch.from_numpy(v) for v in (depth, target, mask))
        with torch.no_grad():
            s32, t32 = fit(d, y, m)
            s64, t64 = fit(d.double(), y.double(), m.double())
            assert s32.dtype == torch.float32 and s64.dtype == torch.float64 and tuple(s32.shape) == (1,)
            scale = torch.abs(s32)
            a = d * scale + t32                                  # train.py:784-785
            panel = torch.cat((a, y), dim=0).unsqueeze(1)        # :787; make_grid(padding=0) of [2,1,h,w] lays the two side by side
            panel = torch.cat(list(panel[:, 0]), dim=1).numpy()  # [h, 2w]: its channel 0, which is what :789 saves
        assert np.array_equal(panel[:, :depth.shape[2]], aligned(depth[0], scale.item(), t32.item())), name
        picture = imsave_bytes(panel)
        assert np.array_equal(cmap_mpl(panel, *extrema(panel), lut), picture), (name, "the oracle does not give imsave's bytes")
        print(f"{name}: {depth.shape[1]}x{depth.shape[2]}  fp32 scale {s32.item():.9g} shift {t32.item():.9g}; fp64 scale {s64.item():.17g} shift {t64.item():.17g}; "
              f"fp32 off by {abs(s32.item() - s64.item()):.3g} / {abs(t32.item() - t64.item()):.3g}")
        out.update({f"{name}/depth": depth, f"{name}/target": target, f"{name}/mask": mask, f"{name}/scale32": s32.numpy(), f"{name}/shift32": t32.numpy(),
                    f"{name}/scale64": s64.numpy(), f"{name}/shift64": t64.numpy(), f"{name}/panel": panel, f"{name}/imsave": picture})
    constant = np.full((4, 6), 0.75, np.float32)
    bad = np.linspace(0, 1, 35, dtype=np.float32).reshape(5, 7).copy()
    bad[2, 3] = np.nan
    for name, panel in (("constant", constant), ("nan", bad)):
        picture = imsave_bytes(panel)
        assert np.array_equal(cmap_mpl(panel, *extrema(panel), lut), picture), name
        out.update({f"{name}/panel": panel, f"{name}/imsave": picture})
    assert (out["nan/imsave"] == 0).all() and (out["constant/imsave"] == np.append(lut[0], 255)).all()
    rng = np.random.default_rng(9)  # the rule on random fp32 arrays of several ranges, not stored
    for k in range(5):
        panel = (rng.standard_normal((37, 53)) * 10.0 ** (k - 2) + k).astype(np.float32)
        assert np.array_equal(cmap_mpl(panel, *extrema(panel), lut), imsave_bytes(panel)), k
    out["cases"] = np.array(cases)
    out["versions"] = np.array([f"matplotlib {matplotlib.__version__}", f"numpy {np.__version__}"])
    path = os.path.join(HERE, "ref_frames.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", ", ".join(out["versions"]))


if __name__ == "__main__":
    main()
