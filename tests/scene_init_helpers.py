"""Shared by tests/golden/make_reference_vectors10.py and the scene_init tests: the inputs of the fixture's cases, the fixture's
reader, and the comparison the issue of this stage sets (same M, same row order, values equal under ==; the sign of a zero is not
compared)."""
import hashlib
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ref_voxelize.npz")
# case -> (voxel size, dtypes it is recorded in)
CASES = {
    "dense": (0.01, ("float32", "float64")),
    "wide": (0.001, ("float32",)),
    "wide64": (0.001, ("float64",)),
    "same": (0.001, ("float32", "float64")),
    "ties": (0.25, ("float32", "float64")),
    "one": (0.001, ("float32", "float64")),
}
SEEDS = {"dense": 101, "wide": 102, "wide64": 103, "same": 104, "one": 105}  # numpy.random.default_rng(seed); recorded in the file too
REGENERATED = ("wide", "wide64")  # inputs too large to store: drawn again from the recorded seed and checked against the recorded digest
DIGEST_ONLY = ("wide64",)         # outputs too large to store: M, a SHA-256 of the rows and every 64th row are recorded


def case_points(name, dtype, seed=None):
    """The input cloud of a case in `dtype` (the wide cases exist in one dtype each)."""
    rng = np.random.default_rng(SEEDS[name] if seed is None and name in SEEDS else seed)
    if name == "dense":    # 5000 points, sigma 0.02: ~6 points per occupied 0.01 voxel, hundreds of components that round to +-0
        p = rng.standard_normal((5000, 3)) * 0.02
    elif name == "wide":   # 40 x 3 x 0 box at z = 1.5: negative coordinates, one constant axis
        p = np.stack([rng.uniform(-20.0, 20.0, 70000), rng.uniform(-1.5, 1.5, 70000), np.full(70000, 1.5)], axis=1)
    elif name == "wide64":  # 40 x 3 x 8
        p = np.stack([rng.uniform(-20.0, 20.0, 70000), rng.uniform(-1.5, 1.5, 70000), rng.uniform(-4.0, 4.0, 70000)], axis=1)
    elif name == "same":
        p = np.repeat(rng.uniform(-1.0, 1.0, (1, 3)), 300, axis=0)
    elif name == "ties":   # every component of the first two rows is a half-way case at voxel size 0.25
        p = np.array([[0.125, 0.375, -0.125], [0.625, -0.375, 0.875], [0.124, 0.376, -0.126]])
    elif name == "one":
        p = rng.uniform(-1.0, 1.0, (1, 3))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(p.astype(dtype))


def digest(a):
    """SHA-256 of an array's values with -0.0 folded onto +0.0 (shape and dtype included)."""
    a = np.ascontiguousarray(np.asarray(a) + 0.0)
    return hashlib.sha256(repr((a.shape, str(a.dtype))).encode() + a.tobytes()).hexdigest()


def load_case(z, name, dtype):
    """-> (points, voxel size, expected) with expected = {"M", "rows" (or None), "digest", "sample_index", "sample_rows"}."""
    key = f"{name}/{dtype}"
    if name in REGENERATED:
        points = case_points(name, dtype, int(z[f"{name}/seed"]))
        assert digest(points) == str(z[f"{key}/points_digest"]), f"{name}: this numpy does not redraw the recorded input"
    else:
        points = z[f"{key}/points"]
    want = {"M": int(z[f"{key}/M"]), "digest": str(z[f"{key}/out_digest"]), "rows": None if name in DIGEST_ONLY else z[f"{key}/out"],
            "sample_index": z[f"{key}/sample_index"], "sample_rows": z[f"{key}/sample_rows"]}
    return points, float(z[f"{name}/voxel_size"]), want


def assert_rows_equal(got, want, what):
    """got [M,3] against load_case's expected: same M, same order, == on every value (so -0.0 == +0.0), the same dtype."""
    got = np.asarray(got)
    assert got.ndim == 2 and got.shape == (want["M"], 3), f"{what}: {got.shape} rows, the reference has {want['M']}"
    idx = want["sample_index"]
    assert (got[idx] == want["sample_rows"]).all(), f"{what}: the sampled rows differ, first at row {idx[np.nonzero((got[idx] != want['sample_rows']).any(1))[0][0]]}"
    if want["rows"] is not None:
        assert got.dtype == want["rows"].dtype, (what, got.dtype)
        bad = np.nonzero((got != want["rows"]).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[0]}: {got[bad[0]]} vs {want['rows'][bad[0]]}"
    assert digest(got) == want["digest"], f"{what}: the rows' digest differs from the reference's"
