"""CPU tests of gscream_amd.scene_init: the numpy / torch statement of the voxel rule against tests/golden/ref_voxelize.npz (the
reference's own voxelize_sample, recorded on the CPU), kth_smallest's fallback against torch.kthvalue, argument errors, and the
constants the binding mirrors."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.scene_init_helpers import CASES, FIXTURE, assert_rows_equal, load_case  # noqa: E402

from gscream_amd import scene_init as SI  # noqa: E402

CASE_DTYPES = [(name, dtype) for name, (_, dtypes) in CASES.items() for dtype in dtypes]


@pytest.fixture(scope="module")
def fixture_file():
    return np.load(FIXTURE)


@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_the_fallback_statement_equals_the_reference(fixture_file, name, dtype):
    points, voxel_size, want = load_case(fixture_file, name, dtype)
    before = points.copy()
    got = SI.voxelize_sample(points, voxel_size)
    assert SI.last_path == "torch" and isinstance(got, np.ndarray) and got.dtype == points.dtype
    assert_rows_equal(got, want, f"{name} {dtype} (numpy in)")
    assert np.array_equal(points, before)  # the caller's array is not shuffled
    t = torch.from_numpy(points)
    got_t = SI.voxelize_sample(t, voxel_size)
    assert isinstance(got_t, torch.Tensor) and got_t.dtype == t.dtype
    assert_rows_equal(got_t.numpy(), want, f"{name} {dtype} (tensor in)")


def test_the_fixture_holds_what_the_issue_lists(fixture_file):
    z = fixture_file
    assert list(z["cases"]) == list(CASES)
    assert int(z["same/float32/M"]) == 1 and int(z["one/float64/M"]) == 1 and int(z["wide/float32/M"]) < 70000
    ties = z["ties/float32/out"]
    assert (ties == np.array([[0, 0.5, -0.25], [0, 0.5, 0], [0.5, -0.5, 1]], np.float32)).all()
    dense = z["dense/float32/out"]
    zeros = dense[dense == 0]
    assert np.signbit(zeros).sum() > 100 and (~np.signbit(zeros)).sum() > 100  # zero components of both signs
    wide = z["wide/float32/out"]
    assert (wide[:, 0] < 0).any() and (wide[:, 2] == wide[0, 2]).all()       # negative coordinates, one constant axis


def test_fp32_and_fp64_are_different_rules():
    """The division and the precision are part of the rule: a product by 1 / v, or the other precision, moves cells."""
    rng = np.random.default_rng(7)
    p = rng.uniform(-300.0, 300.0, 600_000).astype(np.float32)
    own = np.round(p / 0.001)
    assert (own != np.round(p * np.float32(1000.0))).sum() > 0
    assert (own != np.round(p.astype(np.float64) / 0.001)).sum() > 0


@pytest.mark.parametrize("n", [1, 2, 257, 10_001])
def test_kth_smallest_fallback_equals_kthvalue(n):
    g = torch.Generator().manual_seed(n)
    v = (torch.randint(0, max(2, n // 8), (n,), generator=g).float() * 0.37)  # many repeated values
    for k in sorted({1, max(1, int(n * 0.5)), n}):
        got = SI.kth_smallest(v, k)
        assert SI.last_path == "torch" and got.dim() == 0
        assert got.item() == torch.kthvalue(v, k).values.item() == torch.sort(v).values[k - 1].item()


def test_argument_errors():
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        SI.voxelize_sample(np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        SI.voxelize_sample(torch.zeros(6))
    for bad in (np.nan, np.inf):
        p = np.zeros((3, 3), np.float32)
        p[1, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            SI.voxelize_sample(p, 0.01)
    with pytest.raises(ValueError, match="not finite"):
        SI.voxelize_sample(np.ones((3, 3), np.float32), 0.0)
    with pytest.raises(ValueError, match=r"2\^31"):
        SI.voxelize_sample(np.array([[0.0, 0.0, 3.0e6]], np.float32), 0.001)
    with pytest.raises(ValueError, match="64"):  # 32 + 32 + 1 bits
        SI.voxelize_sample(np.array([[-2.0e6, -2.0e6, 0.0], [2.0e6, 2.0e6, 0.001]], np.float64), 0.001)
    v = torch.rand(5)
    for k in (0, 6, -1):
        with pytest.raises(RuntimeError, match="out of range"):
            SI.kth_smallest(v, k)
        with pytest.raises(RuntimeError, match="out of range"):
            torch.kthvalue(v, k)  # the error torch raises
    with pytest.raises(IndexError):
        SI.kth_smallest(torch.rand(0), 0)
    with pytest.raises(ValueError):
        SI.kth_smallest(torch.rand(2, 2), 1)
    with pytest.raises(RuntimeError, match="HIP device"):
        SI.create_from_pcd(torch.zeros(10, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        SI.sort_keys(torch.zeros(10, dtype=torch.int64))
    with pytest.raises(ValueError):
        SI.sort_keys(torch.zeros(10, dtype=torch.int32))


def test_the_binding_mirrors_the_library(native_lib):
    assert native_lib.gsr_sort_block_keys() == SI.SORT_BLOCK_KEYS
    from gscream_amd import _abi
    for name, value in (("GSR_SORT_BLOCK_KEYS", SI.SORT_BLOCK_KEYS), ("GSR_VOXELIZE_NONFINITE", SI.NONFINITE),
                        ("GSR_VOXELIZE_CELL_RANGE", SI.CELL_RANGE), ("GSR_VOXELIZE_KEY_WIDTH", SI.KEY_WIDTH)):
        assert _abi.header().constants[name] == value
    assert native_lib.gsr_sort_keys_workspace_bytes(-1) == 0 and native_lib.gsr_voxelize_workspace_bytes(1000) > 3 * 8 * 1000
    assert native_lib.gsr_sort_keys_u64(-1, None, None, None, None) != 0  # rejected before anything is launched
    assert native_lib.gsr_kth_smallest_f32(4, 5, None, None, None, None) != 0
    assert abs(SI.opacity_init() - np.log(0.1 / 0.9)) < 1e-6
