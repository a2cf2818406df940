"""Scene initialisation on the HIP path (gscream_amd.scene_init: gsr_voxelize, gsr_kth_smallest_f32, gsr_scene_init_fill).

* every case of tests/golden/ref_voxelize.npz (the reference's voxelize_sample, recorded on the CPU) through the kernels: same M,
  same row order, == on every value; fresh random clouds against the numpy line evaluated here;
* the key's limits: 21 bits on every axis at once and 64 bits in all pass, one bit more raises, and so do |r| >= 2^31 and a NaN;
* kth_smallest exact against torch.kthvalue; create_from_pcd's tensors; the voxel_size <= 0 branch; host stops; repeatability; one
  training iteration on the model it makes.

The bound on `_scaling` is not a constant: it is the error torch's own device evaluation of log(sqrt(clamp_min(d, 1e-7))) has
against fp64 on the same values, plus one fp32 ulp of the value (another correct rounding of logf is not a fault)."""
import os
import sys
import traceback

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.scene_init_helpers import CASES, FIXTURE, assert_rows_equal, load_case  # noqa: E402

from gscream_amd import scene_init as SI  # noqa: E402
from gscream_amd.simple_knn import distCUDA2  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_DTYPES = [(name, dtype) for name, (_, dtypes) in CASES.items() for dtype in dtypes]


@pytest.fixture(scope="module")
def fixture_file():
    return np.load(FIXTURE)


def numpy_line(points, voxel_size):
    return np.unique(np.round(points / voxel_size), axis=0) * voxel_size


def hip_voxelize(points, voxel_size):
    got = SI.voxelize_sample(torch.from_numpy(points).to(DEV), voxel_size)
    assert SI.last_path == "hip" and got.is_cuda and got.dtype == torch.from_numpy(points).dtype
    return got


def assert_same_rows(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


# ---- the fixture and the numpy rule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype", CASE_DTYPES)
def test_the_kernels_equal_the_reference(fixture_file, name, dtype):
    points, voxel_size, want = load_case(fixture_file, name, dtype)
    dev_points = torch.from_numpy(points).to(DEV)
    got = SI.voxelize_sample(dev_points, voxel_size)
    assert SI.last_path == "hip" and got.dtype == dev_points.dtype
    assert_rows_equal(got.cpu().numpy(), want, f"{name} {dtype}")
    assert torch.equal(dev_points.cpu(), torch.from_numpy(points))  # the caller's tensor is as it was
    again = SI.voxelize_sample(dev_points, voxel_size)
    assert torch.equal(got.view(torch.uint8), again.view(torch.uint8))  # identical bits the second time


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fresh_random_points_against_the_numpy_line(dtype):
    rng = np.random.default_rng(2024)
    points = (rng.standard_normal((70_000, 3)) * np.array([0.5, 0.1, 0.2])).astype(dtype)  # many rows share a voxel
    for voxel_size in (0.01, 0.0037):
        want = numpy_line(points, voxel_size)
        assert want.shape[0] < points.shape[0]
        assert_same_rows(hip_voxelize(points, voxel_size), want, f"{np.dtype(dtype).name} voxel {voxel_size}")


def test_an_empty_cloud_and_a_strided_one():
    assert SI.voxelize_sample(torch.zeros((0, 3), device=DEV), 0.01).shape == (0, 3)
    rng = np.random.default_rng(5)
    wide = torch.from_numpy(rng.standard_normal((3000, 6)).astype(np.float32)).to(DEV)
    view = wide[:, ::2]  # not contiguous
    assert_same_rows(SI.voxelize_sample(view, 0.05), numpy_line(view.cpu().numpy(), 0.05), "strided")


# ---- key width ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("lo,hi", [(-(1 << 20), (1 << 20) - 1), (0, 1 << 20), (-(1 << 20) + 1, 1)])
def test_twenty_one_bits_on_every_axis_at_once(dtype, lo, hi):
    """Two points whose cells span hi - lo on every axis: 21 bits each (ranges 2^21 - 1, 2^20 and 2^20, the last with mixed signs)."""
    assert (hi - lo).bit_length() == 21
    v = 0.25  # exact cells in both precisions
    points = np.array([[hi * v, lo * v, hi * v], [lo * v, hi * v, lo * v], [hi * v, lo * v, hi * v]], dtype)
    want = numpy_line(points, v)
    assert want.shape[0] == 2
    assert_same_rows(hip_voxelize(points, v), want, "21 bits x 3")


@pytest.mark.parametrize("widths", [(32, 32, 0), (0, 32, 32), (32, 0, 32), (22, 21, 21)])
def test_sixty_four_key_bits_pass(widths):
    v = 0.25
    span = [(1 << (w - 1)) - 1 if w else 0 for w in widths]  # cells -s .. s with s = 2^(w-1) - 1: a range of 2^w - 2, w bits, |cell| < 2^31
    a = [-s * v for s in span]
    b = [s * v for s in span]
    points = np.array([a, b, a, [a[0], b[1], a[2]]], np.float64)
    want = numpy_line(points, v)
    cells = np.round(points / v).astype(np.int64)
    assert [int(w).bit_length() for w in cells.max(0) - cells.min(0)] == list(widths) and sum(widths) == 64
    assert_same_rows(hip_voxelize(points, v), want, f"widths {widths}")


def test_past_the_key_and_past_the_cell_range_raise():
    v = 0.25
    s = float((1 << 31) - 1)
    too_wide = np.array([[-s, -s, 0.0], [s, s, 1.0]], np.float64) * v  # 32 + 32 + 1 bits
    with pytest.raises(ValueError, match="64"):
        SI.voxelize_sample(torch.from_numpy(too_wide).to(DEV), v)
    with pytest.raises(ValueError, match="64"):
        SI.create_from_pcd(torch.from_numpy(too_wide).to(DEV), v)  # after the read-back: nothing is returned
    for dtype in (np.float32, np.float64):
        far = np.array([[0.0, 0.0, 0.0], [0.0, float(1 << 31) * v, 0.0]], dtype)  # r = 2^31 exactly
        with pytest.raises(ValueError, match=r"2\^31"):
            SI.voxelize_sample(torch.from_numpy(far).to(DEV), v)
        near = np.array([[0.0, 0.0, 0.0], [0.0, -float((1 << 31) - 128) * v, 0.0]], dtype)  # the largest fp32 below 2^31: passes
        assert_same_rows(hip_voxelize(near, v), numpy_line(near, v), "just inside")
        nan = np.zeros((300, 3), dtype)
        nan[177, 1] = np.nan
        with pytest.raises(ValueError, match="not finite"):
            SI.voxelize_sample(torch.from_numpy(nan).to(DEV), v)
        with pytest.raises(ValueError, match="not finite"):
            SI.voxelize_sample(torch.from_numpy(np.ones((5, 3), dtype)).to(DEV), 0.0)


# ---- k-th smallest ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 257, 10_001])
def test_kth_smallest_is_kthvalue(n):
    g = torch.Generator().manual_seed(n)
    few = (torch.randint(0, max(2, n // 8), (n,), generator=g).float() * 0.37).to(DEV)  # many repeated values
    spread = (torch.rand(n, generator=g) * 10.0 ** torch.randint(-30, 30, (n,), generator=g).float()).to(DEV)
    spread[::7] = 0.0
    for values in (few, spread):
        for k in (1, int(n * 0.5), n):
            if k == 0:
                with pytest.raises(RuntimeError, match="out of range"):
                    SI.kth_smallest(values, k)
                continue
            got = SI.kth_smallest(values, k)
            assert SI.last_path == "hip" and got.is_cuda and got.dim() == 0
            want = torch.kthvalue(values, k).values
            assert got.view(torch.int32).item() == want.view(torch.int32).item(), (n, k, got.item(), want.item())


# ---- create_from_pcd ----------------------------------------------------------------------------------------------------------
def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("name", ["dense", "wide"])
def test_create_from_pcd(fixture_file, name):
    points, voxel_size, _want = load_case(fixture_file, name, "float32")
    dev_points = torch.from_numpy(points).to(DEV)
    K, F = 10, 32
    s = SI.create_from_pcd(dev_points, voxel_size, n_offsets=K, feat_dim=F)
    anchors = SI.voxelize_sample(dev_points, voxel_size)
    M = int(anchors.shape[0])
    assert s.voxel_size == voxel_size and isinstance(s.voxel_size, float)
    assert s._anchor.dtype == torch.float32 and torch.equal(s._anchor, anchors)
    for t, shape in ((s._offset, (M, K, 3)), (s._anchor_feat, (M, F)), (s._scaling, (M, 6)), (s._rotation, (M, 4)), (s._opacity, (M, 1)),
                     (s._uncertainty, (M, 1)), (s.max_radii2D, (M,)), (s.xyz_max, (1, 3))):
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
    # _scaling against fp64, bounded by torch's own error on the same values plus one ulp
    d = distCUDA2(anchors)
    assert torch.equal(s.dist2, d)
    exact = np.log(np.sqrt(np.maximum(d.cpu().numpy().astype(np.float64), np.float64(np.float32(1e-7)))))
    own = torch.log(torch.sqrt(d.clamp_min(0.0000001))).cpu().numpy().astype(np.float64)
    got = s._scaling.cpu().numpy().astype(np.float64)
    torch_err = float(np.abs(own - exact).max())
    kernel_err = np.abs(got[:, 0] - exact)
    print(f"{name}: _scaling max abs error {kernel_err.max():.3e} (torch's own: {torch_err:.3e}; largest ulp {ulp32(exact).max():.3e})")
    assert (kernel_err <= torch_err + ulp32(exact)).all(), \
        f"{name}: kernel error {kernel_err.max():.3e} against fp64, torch's own device evaluation {torch_err:.3e}"
    assert (s._scaling == s._scaling[:, :1]).all()  # the six columns are identical
    assert not s._offset.any() and not s._anchor_feat.any() and not s.max_radii2D.any()
    assert torch.equal(s._rotation, torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV).expand(M, 4))
    x = 0.1 * torch.ones((M, 1), dtype=torch.float)  # the reference's expression, on the CPU
    assert torch.equal(s._opacity.cpu(), torch.log(x / (1 - x))) and torch.equal(s._uncertainty, s._opacity)
    assert torch.equal(s.xyz_max, anchors.max(0).values.unsqueeze(0))
    again = SI.create_from_pcd(dev_points, voxel_size, n_offsets=K, feat_dim=F)
    for key in ("_anchor", "_scaling", "_opacity", "xyz_max", "dist2"):
        assert torch.equal(getattr(s, key).view(torch.int32), getattr(again, key).view(torch.int32)), key


def test_fp64_points_give_fp32_anchors(fixture_file):
    points, voxel_size, _want = load_case(fixture_file, "dense", "float64")
    dev_points = torch.from_numpy(points).to(DEV)
    s = SI.create_from_pcd(dev_points, voxel_size)
    assert torch.equal(s._anchor, SI.voxelize_sample(dev_points, voxel_size).float())  # the fp64 rule, then the reference's .float()


def test_voxel_size_from_the_median_distance(fixture_file):
    points, _v, _want = load_case(fixture_file, "dense", "float64")
    for pts in (points, points[:4001].astype(np.float32)):
        dev_points = torch.from_numpy(pts).to(DEV)
        n = pts.shape[0]
        want_v = float(torch.kthvalue(distCUDA2(dev_points.float()), int(n * 0.5)).values)
        for arg in (0.0, -1.0):
            s = SI.create_from_pcd(dev_points, arg)
            assert isinstance(s.voxel_size, float) and s.voxel_size == want_v
            assert torch.equal(s._anchor, SI.voxelize_sample(dev_points, want_v).float())
    with pytest.raises(RuntimeError, match="out of range"):
        SI.create_from_pcd(torch.zeros((1, 3), device=DEV), 0.0)  # int(1 * 0.5) == 0: the error torch raises


# ---- host stops ---------------------------------------------------------------------------------------------------------------
def last_frame_in(err, filename):
    frames = [f for f in traceback.extract_tb(err.value.__traceback__) if f.filename.endswith(filename)]
    return frames[-1]


@pytest.mark.parametrize("voxel_size", [0.01, 0.0])
def test_the_info_read_back_is_the_only_host_stop(fixture_file, voxel_size):
    points, _v, _want = load_case(fixture_file, "dense", "float32")
    dev_points = torch.from_numpy(points).to(DEV)
    SI.create_from_pcd(dev_points, voxel_size)  # library loading and first allocations out of the way
    info_host = SI._voxelize_hip(dev_points, 0.01)[1].tolist()
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, _info = SI._voxelize_hip(dev_points, 0.01)  # everything in front of the read-back: nothing raises
        anchors = out[:info_host[0]].clone()
        distCUDA2(anchors)                                # and the kNN behind it
        with pytest.raises(RuntimeError) as err_create:
            SI.create_from_pcd(dev_points, voxel_size)
        with pytest.raises(RuntimeError) as err_vox:
            SI.voxelize_sample(dev_points, 0.01)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    for err in (err_create, err_vox):
        frame = last_frame_in(err, "scene_init.py")
        assert "info_host = info.tolist()" in frame.line, frame.line  # exactly at the read-back
    assert last_frame_in(err_create, "scene_init.py").name == "create_from_pcd"
    assert last_frame_in(err_vox, "scene_init.py").name == "voxelize_sample"


def test_nothing_behind_the_read_back_stops_the_host(fixture_file, monkeypatch):
    """The same call with the read-back's answer supplied: the kNN, the allocations and the fill run under the error mode."""
    points, voxel_size, _want = load_case(fixture_file, "dense", "float32")
    dev_points = torch.from_numpy(points).to(DEV)
    want = SI.create_from_pcd(dev_points, voxel_size)
    real = SI._voxelize_hip

    class Known:
        def __init__(self, values):
            self.values = values

        def tolist(self):
            return self.values

    def supplied(*args, **kwargs):
        out, info = real(*args, **kwargs)
        return out, Known([int(want._anchor.shape[0]), 0, 0, 0])
    monkeypatch.setattr(SI, "_voxelize_hip", supplied)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = SI.create_from_pcd(dev_points, voxel_size)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    for key in ("_anchor", "_scaling", "_offset", "_rotation", "_opacity", "max_radii2D", "xyz_max"):
        assert torch.equal(getattr(got, key), getattr(want, key)), key


# ---- one iteration --------------------------------------------------------------------------------------------------------------
def test_one_iteration_on_the_initialised_model():
    from gscream_amd import fit as FT
    from gscream_amd import gaussian_renderer as GR
    from gscream_amd import synthetic as S
    W, H = 64, 48
    cloud = S.surface_point_cloud(3, 6_000, 0.6, H / W)
    model, s = SI.model_from_points(torch.from_numpy(cloud).to(DEV), voxel_size=0.001, seed=3)
    M = int(s._anchor.shape[0])
    assert 0 < M <= cloud.shape[0] and model._anchor.shape == (M, 3) and model._anchor.is_cuda
    assert torch.equal(model._anchor.detach(), s._anchor) and torch.equal(model._scaling.detach(), s._scaling)
    assert not model._offset.detach().any() and not model._anchor_feat.detach().any()
    cam = FT.orbit_cameras(1, W, H, 0.6, cloud.mean(0), device=DEV)[0]
    bg = torch.zeros(3, device=DEV)
    model.train()
    vis, _x, _y = GR.prefilter_position2D(cam, model, FT._Pipe, bg)
    pkg = GR.render(cam, model, FT._Pipe, bg, visible_mask=vis, retain_grad=True)
    image = pkg["render"]
    assert image.shape == (3, H, W) and torch.isfinite(image).all() and image.abs().sum() > 0
    image.square().mean().backward()
    for p in (model._scaling, model._offset, model._anchor_feat):
        assert p.grad is not None and torch.isfinite(p.grad).all()
    assert model._scaling.grad.abs().sum() > 0
