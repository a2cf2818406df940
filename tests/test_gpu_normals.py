"""gscream_amd.normals on the device: gsr_depth_points / gsr_point_normals against the per-pixel fp64 oracle of
tests/normals_helpers.py (bounds and their counting there), on the stored reference cases, at the tile edges of the kernel (16 x 16
pixels per workgroup), at window sizes 3 and 15, on IEEE edge values, on a full 567 x 1008 grid, and the launch behaviour (no host
stop, the current stream, identical bits)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.normals_helpers import (POINTS_K, U32, from_reference_layout, normal_tol, normals_oracle, points_oracle,  # noqa: E402
                                   synthetic_frame)
from tests.test_normals import CASES, SHAPES, stored  # noqa: E402

from gscream_amd import normals as N  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SYNTHETIC = {"one_tile": (16, 16), "past_the_tile": (17, 33), "one_pixel": (1, 1)}
EPS = 1e-5
_frames = {}
NORMALS_TORCH = N._normals_torch  # the statement itself, for the one test that compares against it (the fixture below disables the name)


@pytest.fixture
def HIP(monkeypatch):
    """The torch statements made to raise: these tests must run the kernels."""
    def no_fallback(*a, **k):
        raise AssertionError("took the torch path")
    monkeypatch.setattr(N, "_normals_torch", no_fallback)
    monkeypatch.setattr(N, "_points_torch", no_fallback)
    return N


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def frame(name):
    """(depth, K, c2w) of a stored or a synthetic case."""
    if name in CASES:
        d = stored(name)
        return d["depth"], d["K"], d["c2w"]
    if name not in _frames:
        _frames[name] = synthetic_frame(*SYNTHETIC[name], seed=len(name))
    return _frames[name]


def check_normals(r, points, size, h, w):
    """The returned [1, 3, w, h] against the oracle run on `points` [3, h, w]; the inputs must sit on no det threshold."""
    o = normals_oracle(points, size, 0.15, EPS)
    assert np.abs(o["det"] / EPS - 1.0).min() >= 1e-6
    assert tuple(r.shape) == (1, 3, w, h) and r.dtype == torch.float32
    got = from_reference_layout(r.cpu().numpy()).astype(np.float64)
    dev_ = np.abs(got - o["normals"])
    tol = normal_tol(o["cond"], size)
    print(f"{h}x{w} size {size}: largest deviation {dev_.max():.3g}, largest share of the bound {(dev_ / tol).max():.3g}, cond max {o['cond'].max():.3g}")
    assert (dev_ <= tol).all()
    return o


@pytest.mark.parametrize("name", CASES + tuple(SYNTHETIC))
def test_points_and_normals_against_the_oracle(name, HIP):
    depth, K, c2w = frame(name)
    h, w = depth.shape
    pts = N.depth2pcd_fromplane(dev(depth)[None], dev(c2w), dev(K), h, w)
    assert N.last_path == "hip" and tuple(pts.shape) == (1, 3, h, w) and pts.dtype == torch.float32
    P64, mag = points_oracle(depth, K, c2w)
    got = pts[0].cpu().numpy()
    assert (np.abs(got.astype(np.float64) - P64) <= POINTS_K * U32 * mag).all()
    if name in CASES:  # the stored map is another summation order of the same fp32 rule
        assert (np.abs(got.astype(np.float64) - stored(name)["points"]) <= 2 * POINTS_K * U32 * mag).all()
        points = stored(name)["points"]  # the oracle run is shared with the CPU tests
        r = N.least_square_normal_regress_fast01(dev(points)[None])
        assert N.last_path == "hip"
        o = stored(name)["oracle"]
        dev_ = np.abs(from_reference_layout(r.cpu().numpy()).astype(np.float64) - o["normals"])
        assert tuple(r.shape) == (1, 3, w, h) and (dev_ <= normal_tol(o["cond"], 9)).all(), dev_.max()
        # and within the bound of the reference's own fp64 run
        assert (np.abs(r.cpu().numpy().astype(np.float64) - stored(name)["normals_ref64"])
                <= 2 * normal_tol(o["cond"], 9).reshape(w, h, 1).transpose(2, 0, 1)[None]).all()
    else:
        r = N.least_square_normal_regress_fast01(pts)
        assert N.last_path == "hip"
        check_normals(r, got, 9, h, w)


@pytest.mark.parametrize("size", [3, 15])
def test_other_window_sizes(size, HIP):
    depth, K, c2w = frame("past_the_tile")
    h, w = depth.shape
    pts = N.depth2pcd_fromplane(dev(depth), dev(c2w), dev(K), h, w)
    r = N.least_square_normal_regress_fast01(pts, None, None, size)
    assert N.last_path == "hip"
    check_normals(r, pts[0].cpu().numpy(), size, h, w)


def edge_points():
    """A hand-made 12 x 13 point map of small integers (every sum is exact): z in {0, 2, -3, 40} by pixel, so that a centre with z = 0 sees
    neighbours with z = 0 (0/0: NaN, kept), z > 0 (+inf, dropped) and z < 0 (-inf, dropped); one point with z = +inf, one all-NaN."""
    rng = np.random.default_rng(11)
    h, w = 12, 13
    i, j = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    z = rng.choice(np.array([0, 0, 2, -3, 40], np.float32), size=(h, w))
    z[2, 2], z[2, 3], z[3, 2], z[1, 2] = 0, 2, -3, 0
    z[9, 2], z[9, 3], z[10, 2], z[8, 2] = 0, 2, -3, 0
    p = np.stack([j - 4, i - 5, z]).astype(np.float32)
    p[2, 8, 9] = np.inf
    p[:, 4, 5] = np.nan
    return p


def test_ieee_edge_semantics(HIP):
    p = edge_points()
    h, w = 12, 13
    o = normals_oracle(p, 9, 0.15, EPS)
    # what the oracle says about the rules.  Centre (9, 2), z = 0, a window without the inf / NaN points: exactly the points with
    # z != 0 are dropped (+-inf quotients), the points with z = 0 stay (NaN quotients), and the result is finite
    iy, ix = np.clip(np.arange(5, 14), 0, h - 1), np.clip(np.arange(-2, 7), 0, w - 1)
    win = p[2][iy[:, None], ix[None, :]]
    k = 9 * w + 2
    assert np.isfinite(win).all() and (win > 0).any() and (win < 0).any() and 0 < (win == 0).sum() < 81
    assert o["dropped"][k] == int((win != 0).sum()) and np.isfinite(o["normals"][k]).all() and o["normals"][k].any()
    # centre (2, 2), z = 0, with the NaN point in its window: it is kept, the sums are NaN, the output is 0
    assert not o["normals"][2 * w + 2].any() and not o["normals"][4 * w + 5].any()
    # the inf point is dropped from its neighbours' windows: centre (10, 11) stays finite
    assert np.isfinite(o["normals"][10 * w + 11]).all() and o["normals"][10 * w + 11].any()
    r = N.least_square_normal_regress_fast01(dev(p)[None])
    assert N.last_path == "hip"
    got = from_reference_layout(r.cpu().numpy()).astype(np.float64)
    assert np.isfinite(got).all()                                             # NaN -> 0
    assert (np.abs(got - o["normals"]) <= normal_tol(o["cond"], 9)).all()
    zero = ~o["normals"].any(axis=1)
    assert zero.sum() >= 20 and not got[zero].any()                           # the NaN windows are zeros exactly


def test_repeated_calls_give_identical_bits(HIP):
    depth, K, c2w = frame("benign")
    out = []
    for _ in range(3):
        pts = N.depth2pcd_fromplane(dev(depth)[None], dev(c2w), dev(K), 40, 48)
        out.append((bits(pts).clone(), bits(N.least_square_normal_regress_fast01(pts)).clone()))
    assert all(torch.equal(out[0][0], o[0]) and torch.equal(out[0][1], o[1]) for o in out[1:])


def test_the_calls_do_not_stop_the_host(HIP):
    depth, K, c2w = (dev(a) for a in frame("past_the_tile"))
    N.normal_map(depth[None], c2w, K)  # library loading and first allocations out of the way
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pts = N.depth2pcd_fromplane(depth[None], c2w, K, 17, 33)
        r = N.least_square_normal_regress_fast01(pts)
        pic = N.normal_map(depth[None], c2w, K)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert N.last_path == "hip" and tuple(r.shape) == (1, 3, 33, 17) and tuple(pic.shape) == (3, 17, 33)


def test_the_current_stream_is_honoured(HIP):
    """On a side stream, behind a delay and the copy that fills the input: a launch on any other stream would read the zeros."""
    depth, K, c2w = (dev(a) for a in frame("past_the_tile"))
    want_pts = N.depth2pcd_fromplane(depth, c2w, K, 17, 33)
    want = N.least_square_normal_regress_fast01(want_pts)
    staged_depth, staged_pts = torch.zeros_like(depth), torch.zeros_like(want_pts)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda._sleep(20_000_000)
        staged_depth.copy_(depth)
        staged_pts.copy_(want_pts)
        pts = N.depth2pcd_fromplane(staged_depth, c2w, K, 17, 33)
        r = N.least_square_normal_regress_fast01(staged_pts)
    st.synchronize()
    assert N.last_path == "hip" and torch.equal(bits(pts), bits(want_pts)) and torch.equal(bits(r), bits(want))
    assert want.abs().sum() > 0


def test_a_full_size_grid(HIP):
    """567 x 1008 (2304 workgroups): the HIP result against the torch statement in fp64 on the device, on three bands of 16 rows -- top,
    middle, bottom -- each cut out of the point map with its 4-row halo (replicate padding coincides with the image edge at the
    top and the bottom).  Both sides are within the bound of the exact value, so they differ by at most twice the bound."""
    h, w = 567, 1008
    depth, K, c2w = synthetic_frame(h, w, 7)
    pts = N.depth2pcd_fromplane(dev(depth)[None], dev(c2w), dev(K), h, w)
    r = N.least_square_normal_regress_fast01(pts)
    assert N.last_path == "hip" and tuple(r.shape) == (1, 3, w, h)
    pic = r.reshape(3, h, w)  # [c, i, j] is pixel (i, j)
    for top in (0, 272, h - 16):
        lo, hi = max(top - 4, 0), min(top + 20, h)
        band = pts[0, :, lo:hi, :].contiguous()
        v = NORMALS_TORCH(band, 9, 0.15, EPS, torch.float64)
        _X, A, _b = N._window_sums_torch(band, 9, 0.15, torch.float64)  # (for the bound: cond and det of each system)
        det = torch.linalg.det(A)
        rows = slice(top - lo, top - lo + 16)
        want = v.reshape(hi - lo, w, 3)[rows].cpu().numpy()
        det = det.reshape(hi - lo, w)[rows].cpu().numpy()
        assert np.isfinite(want).all() and np.abs(det / EPS - 1.0).min() >= 1e-6
        cond = np.where(det < EPS, 1.0, np.linalg.cond(A.reshape(hi - lo, w, 3, 3)[rows].cpu().numpy()))
        got = pic[:, top:top + 16, :].permute(1, 2, 0).cpu().numpy().astype(np.float64)
        dev_ = np.abs(got - want)
        tol = 2 * normal_tol(cond.reshape(-1), 9).reshape(16, w, 1)
        print(f"rows {top}..{top + 15}: largest deviation {dev_.max():.3g}, largest share of the bound {(dev_ / tol).max():.3g}, cond max {cond.max():.3g}")
        assert (dev_ <= tol).all()


def test_normal_map_is_the_composition_bit_for_bit(HIP):
    depth, K, c2w = (dev(a) for a in frame("benign"))
    got = N.normal_map(depth[None], c2w, K)
    assert N.last_path == "hip"
    pts = N.depth2pcd_fromplane(depth[None], c2w, K, 40, 48)
    n = N.least_square_normal_regress_fast01(pts).reshape(3, 40, 48).permute(1, 2, 0)
    want = (torch.nn.functional.normalize(n, p=2, dim=-1).permute(2, 0, 1) + 1) / 2
    assert tuple(got.shape) == (3, 40, 48) and torch.equal(bits(got), bits(want))
    assert float(got.min()) >= 0 and float(got.max()) <= 1


def test_what_the_hip_path_does_not_take_goes_to_torch():
    depth, K, c2w = (dev(a) for a in frame("tiny"))
    pts = N.depth2pcd_fromplane(depth, c2w, K, 5, 7)
    assert N.last_path == "hip"
    a = N.least_square_normal_regress_fast01(pts)
    assert N.last_path == "hip"
    b = N.least_square_normal_regress_fast01(pts, size=17)
    assert N.last_path == "torch" and tuple(b.shape) == (1, 3, 7, 5)
    c = N.least_square_normal_regress_fast01(pts.double())
    assert N.last_path == "torch" and c.dtype == torch.float64
    N.force_torch = True
    try:
        d = N.least_square_normal_regress_fast01(pts)
        assert N.last_path == "torch"
        e = N.depth2pcd_fromplane(depth, c2w, K, 5, 7)
        assert N.last_path == "torch"
    finally:
        N.force_torch = False
    o = normals_oracle(pts[0].cpu().numpy(), 9, 0.15, EPS)
    for r in (a, c, d):
        assert (np.abs(from_reference_layout(r.cpu().numpy()) - o["normals"]) <= normal_tol(o["cond"], 9)).all()
    P64, mag = points_oracle(*frame("tiny"))
    assert (np.abs(e[0].cpu().numpy() - P64) <= POINTS_K * U32 * mag).all()
