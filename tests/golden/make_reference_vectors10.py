"""Golden vectors for the voxel dedupe, produced by RUNNING the reference's GaussianModel.voxelize_sample on the CPU.

    python tests/golden/make_reference_vectors10.py <path of the reference checkout>     # or GSCREAM_REFERENCE=<path>; numpy only

scene/gaussian_model.py cannot be imported (it pulls simple_knn, torch_scatter, plyfile and the CUDA rasterizer), so only the
FunctionDef node `voxelize_sample` (:295-299) is taken out of the class body in its syntax tree and compiled in place, into a namespace
that holds `np`, as make_reference_vectors7 / 9 do; nothing of the reference is copied, only inputs and returned arrays are stored
(ref_voxelize.npz).  The method shuffles its argument in place, so it is handed a copy.

Cases (tests/scene_init_helpers.py draws the inputs; the seeds of numpy.random.default_rng are recorded as "<case>/seed"):

  dense    5000 points, sigma 0.02, voxel 0.01: several points per voxel, hundreds of components that round to +0 and to -0
  wide     70 000 fp32 points over a 40 x 3 x 0 box at z = 1.5 (negative coordinates, one constant axis), voxel 0.001
  wide64   70 000 fp64 points over 40 x 3 x 8, voxel 0.001
  same     300 copies of one point, voxel 0.001: one row
  ties     (0.125, 0.375, -0.125), (0.625, -0.375, 0.875), (0.124, 0.376, -0.126) at voxel 0.25: every component of the first two is a
           half-way case; rows (0, 0.5, -0.25), (0, 0.5, -0), (0.5, -0.5, 1)
  one      a single point

Per case and dtype, prefix "<case>/<dtype>/": points (not for wide / wide64, whose inputs are drawn again from the seed and checked
against points_digest), out = the returned array (not for wide64: 1.7 MB), M, out_digest (scene_init_helpers.digest: SHA-256 of the
values with -0.0 folded onto +0.0), sample_index / sample_rows = every 64th row.  "versions" records numpy's version.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from scene_init_helpers import CASES, DIGEST_ONLY, FIXTURE, REGENERATED, SEEDS, case_points, digest  # noqa: E402

NAME = "voxelize_sample"


def load_reference_function(root):
    path = os.path.join(root, "scene", "gaussian_model.py")
    tree = ast.parse(open(path).read(), path)
    found = [n for c in tree.body if isinstance(c, ast.ClassDef) and c.name == "GaussianModel"
             for n in c.body if isinstance(n, ast.FunctionDef) and n.name == NAME]
    assert len(found) == 1
    tree.body = found
    ns = {"np": np}
    exec(compile(tree, path, "exec"), ns)
    return ns[NAME]


def main():
    root = os.environ.get("GSCREAM_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not root:
        sys.exit(__doc__)
    voxelize = load_reference_function(root)
    out = {}
    for name, (voxel_size, dtypes) in CASES.items():
        out[f"{name}/voxel_size"] = np.float64(voxel_size)
        if name in SEEDS:
            out[f"{name}/seed"] = np.int64(SEEDS[name])
        for dtype in dtypes:
            points = case_points(name, dtype)
            rows = voxelize(None, data=points.copy(), voxel_size=voxel_size)
            assert rows.dtype == points.dtype and rows.ndim == 2 and rows.shape[1] == 3, (name, rows.dtype, rows.shape)
            key = f"{name}/{dtype}"
            idx = np.arange(0, rows.shape[0], 64)
            out.update({f"{key}/M": np.int64(rows.shape[0]), f"{key}/out_digest": np.array(digest(rows)), f"{key}/sample_index": idx,
                        f"{key}/sample_rows": rows[idx]})
            if name in REGENERATED:
                out[f"{key}/points_digest"] = np.array(digest(points))
            else:
                out[f"{key}/points"] = points
            if name not in DIGEST_ONLY:
                out[f"{key}/out"] = rows
            zeros = rows[rows == 0]
            print(f"{name} {dtype}: {points.shape[0]} points -> {rows.shape[0]} rows at voxel {voxel_size}; zero components: "
                  f"{int((~np.signbit(zeros)).sum())} positive, {int(np.signbit(zeros).sum())} negative")
            if name == "ties":
                assert (rows == np.array([[0, 0.5, -0.25], [0, 0.5, -0.0], [0.5, -0.5, 1.0]])).all(), rows
    out["cases"] = np.array(list(CASES))
    out["versions"] = np.array([f"numpy {np.__version__}"])
    np.savez_compressed(FIXTURE, **out)
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes;", ", ".join(out["versions"]))
    assert os.path.getsize(FIXTURE) < (1 << 20)


if __name__ == "__main__":
    main()
