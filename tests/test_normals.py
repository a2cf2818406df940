"""gscream_amd.normals without a GPU: the fp64 oracle the GPU tests measure against (pinned to the reference's own fp64 run), the
module's torch path, the reference's return layout, the point map, and the argument checks of gsr_depth_points / gsr_point_normals.
Bounds: tests/normals_helpers.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.normals_helpers import (POINTS_K, U32, from_reference_layout, normal_tol, normals_oracle, points_oracle,  # noqa: E402
                                   reference_layout, synthetic_frame)

GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_normals.npz")
CASES = ("benign", "near", "real_focal", "tiny")
SHAPES = {"benign": (40, 48), "near": (37, 53), "real_focal": (24, 31), "tiny": (5, 7)}
_cache = {}


def stored(case):
    """The stored case with its oracle run (computed once, shared, never written to)."""
    if case not in _cache:
        z = np.load(GOLDEN)
        d = {k: z[f"{case}/{k}"] for k in ("depth", "K", "c2w", "points", "normals_ref32", "normals_ref64")}
        size, gamma, eps = z["settings"]
        d["settings"] = (int(size), float(gamma), float(eps))
        d["oracle"] = normals_oracle(d["points"], *d["settings"])
        for v in list(d.values()) + list(d["oracle"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[case] = d
    return _cache[case]


def test_the_file_holds_the_four_cases_and_the_settings():
    z = np.load(GOLDEN)
    assert tuple(z["cases"]) == CASES and tuple(z["settings"]) == (9.0, 0.15, 1e-5)
    for case, (h, w) in SHAPES.items():
        d = stored(case)
        assert d["depth"].shape == (h, w) and d["points"].shape == (3, h, w) and d["points"].dtype == np.float32
        assert d["normals_ref32"].shape == d["normals_ref64"].shape == (1, 3, w, h) and d["normals_ref64"].dtype == np.float64
        assert h != w


@pytest.mark.parametrize("case", CASES)
def test_the_inputs_sit_on_no_threshold(case):
    """What the generator checked: no window point within 1e-5 of gamma, no determinant within 1e-6 (relative) of eps."""
    d = stored(case)
    o, eps = d["oracle"], d["settings"][2]
    assert o["margin"].min() >= 1e-5 and np.abs(o["det"] / eps - 1.0).min() >= 1e-6


def test_the_cases_cover_what_they_are_there_for():
    b, n, t = stored("benign"), stored("near"), stored("tiny")
    eps = b["settings"][2]
    share = b["oracle"]["dropped"].sum() / (40 * 48 * 81)
    assert 0.02 <= share <= 0.15                                          # the gamma mask fires
    block = b["oracle"]["det"].reshape(40, 48)[10:15, 8:14]
    assert (b["depth"][6:19, 4:18] == 0).all() and (np.abs(block) < 1e-9).all()   # constant points: rank 1
    below = np.mean(n["oracle"]["det"] < eps)
    assert 0.3 <= below <= 0.7                                             # both branches of det < eps
    assert (t["depth"] != 0).all() and min(SHAPES["tiny"]) < 9


@pytest.mark.parametrize("case", CASES)
def test_the_oracle_reproduces_the_references_fp64_run(case):
    d = stored(case)
    want = from_reference_layout(d["normals_ref64"])
    dev = np.abs(d["oracle"]["normals"] - want)
    assert (dev <= normal_tol(d["oracle"]["cond"], 9)).all(), dev.max()


@pytest.mark.parametrize("case", CASES)
def test_the_torch_path_on_cpu_tensors(case):
    from gscream_amd import normals as N
    d = stored(case)
    h, w = SHAPES[case]
    x = torch.from_numpy(d["points"].copy())[None]
    r = N.least_square_normal_regress_fast01(x)
    assert N.last_path == "torch" and tuple(r.shape) == (1, 3, w, h) and r.dtype == torch.float32
    tol = normal_tol(d["oracle"]["cond"], 9)
    got = from_reference_layout(r.numpy()).astype(np.float64)
    assert (np.abs(got - d["oracle"]["normals"]) <= tol).all()
    # the caller's reshape(3, h, w)[c, i, j] is pixel (i, j): the stored picture
    pic = r.reshape(3, h, w).numpy().astype(np.float64)
    assert (np.abs(pic - d["oracle"]["normals"].reshape(h, w, 3).transpose(2, 0, 1)) <= tol.reshape(h, w, 1).transpose(2, 0, 1)).all()
    assert (np.abs(pic - d["normals_ref64"].reshape(3, h, w)) <= 2 * tol.reshape(h, w, 1).transpose(2, 0, 1)).all()
    # the reference's eye / ones, given, change nothing; the same arguments in the same order
    r2 = N.least_square_normal_regress_fast01(x, torch.eye(3), torch.ones(h * w, 81, 1), 9, 0.15, 1, 1e-5)
    assert torch.equal(r, r2)


def test_the_return_layout_is_the_references():
    """r[0, c, a, b] = n[a*h + b, c] on a non-square frame."""
    from gscream_amd import normals as N
    d = stored("tiny")
    h, w = SHAPES["tiny"]
    r = N.least_square_normal_regress_fast01(torch.from_numpy(d["points"].copy())[None]).numpy()
    n = N._normals_torch(torch.from_numpy(d["points"].copy()), 9, 0.15, 1e-5, torch.float64).numpy().astype(np.float32)
    for c in range(3):
        for a in range(w):
            for b in range(h):
                assert r[0, c, a, b] == n[a * h + b, c]
    assert np.array_equal(reference_layout(n, h, w), r) and np.array_equal(from_reference_layout(r), n)


@pytest.mark.parametrize("case", CASES)
def test_the_point_map(case):
    """Against fp64 within POINTS_K roundings, against the stored fp32 map (another summation order) within twice that."""
    from gscream_amd import normals as N
    d = stored(case)
    h, w = SHAPES[case]
    P64, mag = points_oracle(d["depth"], d["K"], d["c2w"])
    assert (np.abs(d["points"].astype(np.float64) - P64) <= POINTS_K * U32 * mag).all()  # the stored map itself
    for depth in (torch.from_numpy(d["depth"].copy())[None], torch.from_numpy(d["depth"].copy())):
        got = N.depth2pcd_fromplane(depth, torch.from_numpy(d["c2w"].copy()), torch.from_numpy(d["K"].copy()), h, w)
        assert N.last_path == "torch" and tuple(got.shape) == (1, 3, h, w) and got.dtype == torch.float32
        g = got[0].numpy().astype(np.float64)
        assert (np.abs(g - P64) <= POINTS_K * U32 * mag).all()
        assert (np.abs(g - d["points"].astype(np.float64)) <= 2 * POINTS_K * U32 * mag).all()


def test_fp32_is_the_references_arithmetic_on_the_benign_case():
    """_normals_torch(dtype=float32) against normals_ref32: the same arithmetic, not necessarily the same bmm order, so to the
    difference the file itself shows between the reference's fp32 and fp64 runs on this case, times 4."""
    from gscream_amd import normals as N
    d = stored("benign")
    ref32, ref64 = from_reference_layout(d["normals_ref32"]).astype(np.float64), from_reference_layout(d["normals_ref64"])
    shown = np.abs(ref32 - ref64).max()
    got = N._normals_torch(torch.from_numpy(d["points"].copy()), 9, 0.15, 1e-5, torch.float32)
    assert got.dtype == torch.float32
    dev = np.abs(got.numpy().astype(np.float64) - ref32).max()
    print(f"fp32 torch statement against normals_ref32: {dev:.3g}; the file's ref32 against ref64: {shown:.3g}")
    assert 0 < shown < 1e-3 and dev <= 4 * shown


def test_normal_map_is_the_composition():
    from gscream_amd import normals as N
    depth, K, c2w = (torch.from_numpy(a) for a in synthetic_frame(11, 14, 3))
    got = N.normal_map(depth[None], c2w, K)
    pts = N.depth2pcd_fromplane(depth[None], c2w, K, 11, 14)
    n = N.least_square_normal_regress_fast01(pts).reshape(3, 11, 14).permute(1, 2, 0)
    want = (torch.nn.functional.normalize(n, p=2, dim=-1).permute(2, 0, 1) + 1) / 2
    assert tuple(got.shape) == (3, 11, 14) and torch.equal(got, want) and float(got.min()) >= 0 and float(got.max()) <= 1


def test_other_sizes_and_bad_arguments_on_the_torch_path():
    from gscream_amd import normals as N
    d = stored("tiny")
    x = torch.from_numpy(d["points"].copy())[None]
    for size in (1, 3, 17):  # 17: beyond the kernel's range, the torch statement takes any odd size
        o = normals_oracle(d["points"], size, 0.15, 1e-5)
        r = N.least_square_normal_regress_fast01(x, size=size)
        assert (np.abs(from_reference_layout(r.numpy()) - o["normals"]) <= normal_tol(o["cond"], size)).all(), size
    with pytest.raises(ValueError):
        N.least_square_normal_regress_fast01(x, size=4)
    with pytest.raises(ValueError):
        N.least_square_normal_regress_fast01(x[0])
    with pytest.raises(ValueError):
        N.depth2pcd_fromplane(torch.zeros(1, 5, 7), torch.zeros(3, 4), torch.eye(3), 5, 8)
    x64 = x.double()
    r = N.least_square_normal_regress_fast01(x64)
    assert r.dtype == torch.float64 and N.last_path == "torch"


def test_header_binding_and_library_have_the_two_calls(native_lib):
    from gscream_amd import _abi, _native
    hdr = _abi.header()
    assert hdr.constants["GSR_ABI_VERSION"] == 9 and _native.ABI_VERSION == 9 and native_lib.gsr_abi_version() == 9
    for name in ("gsr_depth_points", "gsr_point_normals"):
        assert hdr.functions[name][0] == "int" and name in _native.EXPORTED_SYMBOLS and hasattr(native_lib, name)
    assert len(native_lib.gsr_depth_points.argtypes) == 7 and len(native_lib.gsr_point_normals.argtypes) == 8
    for lib in ("libgsraster_precise.so", "libgsraster_replayall.so"):  # the two test builds link the same objects
        import ctypes
        path = os.path.join(os.path.dirname(_native.LIB_PATH), lib)
        if os.path.exists(path):
            assert hasattr(ctypes.CDLL(path), "gsr_point_normals")


def test_argument_checks_without_a_gpu(native_lib):
    """Everything the two calls reject, they reject before launching (there is no device here to launch on)."""
    points, normals, err = native_lib.gsr_depth_points, native_lib.gsr_point_normals, native_lib.gsr_last_error
    a, b, c, d = 256, 512, 768, 1024  # never dereferenced on the host
    for hw in ((0, 5), (5, 0), (-1, 5), (5, -3)):
        assert points(*hw, a, b, c, d, None) == -1 and b"need both > 0" in err(), hw
        assert normals(*hw, a, 9, 0.15, 1e-5, b, None) == -1 and b"need both > 0" in err(), hw
    for hw in ((1 << 16, 1 << 15), (46341, 46341), (2 ** 31 - 256, 1), (1, 2 ** 31 - 1)):
        assert points(*hw, a, b, c, d, None) == -1 and b"too many pixels" in err(), hw
        assert normals(*hw, a, 9, 0.15, 1e-5, b, None) == -1 and b"too many pixels" in err(), hw
    for k in range(4):
        args = [a, b, c, d]
        args[k] = None
        assert points(5, 7, *args, None) == -1 and b"NULL" in err(), k
    assert normals(5, 7, None, 9, 0.15, 1e-5, b, None) == -1 and b"NULL" in err()
    assert normals(5, 7, a, 9, 0.15, 1e-5, None, None) == -1 and b"NULL" in err()
    for size in (0, -1, 2, 8, 16, 17, 255):
        assert normals(5, 7, a, size, 0.15, 1e-5, b, None) == -1 and b"odd size" in err() and str(size).encode() in err(), size
