"""GPU parity tests: the HIP path (through the public API -> ctypes -> C ABI -> kernels) against the
committed golden vectors and against the live CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): integer results (radii, num_rendered, per-tile sorted id lists) bit-exact;
images within 1e-4 abs; gradients within 1e-3 rel (denominator |ref| + 1e-3 max|ref|)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers as Hh  # noqa: E402
from golden import make_golden as MG  # noqa: E402
from gscream_amd import _layout, set_tuning  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = sorted(MG.cases().keys())
NT = max(1, min(16, os.cpu_count() or 1))  # oracle threads of the live checks


@pytest.fixture(autouse=True)
def _default_tuning():
    set_tuning()
    yield
    set_tuning()


def _check_binning(s, got, exp_point_list, exp_tile_counts):
    P, R = s["means3D"].shape[0], got["num_rendered"]
    img = _layout.image_views(got["img"], P, s["W"], s["H"])
    rng = img["ranges"].cpu().numpy().astype(np.int64)
    counts = rng[:, 1] - rng[:, 0]
    assert (counts == exp_tile_counts.astype(np.int64)).all(), "per-tile instance counts"
    assert rng[0, 0] == 0 and (rng[1:, 0] == rng[:-1, 1]).all() and rng[-1, 1] == R, "ranges must partition [0,R)"
    pl = _layout.binning_views(got["binning"], R, got["binning_capacity"])["point_list"].cpu().numpy().astype(np.int64)
    assert (pl == exp_point_list.astype(np.int64)).all(), "sorted per-tile Gaussian id lists"


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_forward_backward(name):
    s, grads, exp = MG.load(name)
    got = Hh.hip_run(s, grads)
    assert (got["radii"] == exp["radii"]).all(), "radii must be bit-exact"
    # the bar itself, against the oracle run on the golden's inputs (round 6; the committed expectations are that oracle's outputs:
    # tests/test_oracle.py pins them on the CPU) ...
    st = Hh.oracle_forward(s)
    live = Hh.oracle_backward(s, st, grads)
    Hh.assert_parity_strict(got, st, live, s, grads, context=name, nthreads=NT)
    # ... and against the committed vectors themselves, at the plain tolerances with no allowance (every pixel, every element)
    for k in ("out_color", "out_depth", "out_unc"):
        Hh.assert_images_close(got[k], exp[k], f"{name}/{k}")
    ref = {k[5:]: exp[k] for k in exp if k.startswith("grad_")}
    keys = list(Hh.GRAD_KEYS) + ["dL_dsh", "dL_dcov3D"]
    Hh.assert_grads_close(got, ref, keys=keys, context=name)
    assert got["dL_dmeans2D"].shape == (s["means3D"].shape[0], 3) and not got["dL_dmeans2D"][:, 2].any()
    culled = exp["radii"] <= 0
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations"):
        if k in got:
            assert not got[k][culled].any(), f"{k}: culled Gaussians must get exact zeros (backward.cu:156,369)"


def _check_culled_binning(s, got, st):
    """With tile culling on, every tile's list must be the oracle's list minus instances that cannot change any
    pixel of that tile (max alpha over the tile's pixels < 1/255, checked here in float64), in the same order."""
    P, R = s["means3D"].shape[0], got["num_rendered"]
    W, H = s["W"], s["H"]
    gx = (W + 15) // 16
    img = _layout.image_views(got["img"], P, W, H)
    rng = img["ranges"].cpu().numpy().astype(np.int64)
    pl = _layout.binning_views(got["binning"], R, got["binning_capacity"])["point_list"].cpu().numpy().astype(np.int64)
    assert rng[0, 0] == 0 and (rng[1:, 0] == rng[:-1, 1]).all() and rng[-1, 1] == R
    ref_rng, ref_pl = st["ranges"].astype(np.int64), st["point_list"].astype(np.int64)
    m2, co = st["means2D"].astype(np.float64), st["conic_opacity"].astype(np.float64)
    dropped = kept = 0
    for t in range(rng.shape[0]):
        mine, ref = pl[rng[t, 0]:rng[t, 1]], ref_pl[ref_rng[t, 0]:ref_rng[t, 1]]
        keep = np.isin(ref, mine)
        assert np.array_equal(ref[keep], mine), f"tile {t}: not an order-preserving subset of the reference list"
        kept += len(mine)
        gone = ref[~keep]
        if len(gone) == 0:
            continue
        dropped += len(gone)
        tx, ty = t % gx, t // gx
        xs = np.arange(tx * 16, min(tx * 16 + 16, W), dtype=np.float64)
        ys = np.arange(ty * 16, min(ty * 16 + 16, H), dtype=np.float64)
        dx = m2[gone, 0][:, None, None] - xs[None, None, :]
        dy = m2[gone, 1][:, None, None] - ys[None, :, None]
        power = -0.5 * (co[gone, 0][:, None, None] * dx * dx + co[gone, 2][:, None, None] * dy * dy) - co[gone, 1][:, None, None] * dx * dy
        alpha = co[gone, 3][:, None, None] * np.exp(np.minimum(power, 0.0))
        alpha = np.where(power > 0, 0.0, alpha)
        assert alpha.max() < 1.0 / 255.0, f"tile {t}: a culled instance reaches alpha {alpha.max():.6f} >= 1/255"
    return kept, dropped


@pytest.mark.parametrize("name", ["cfg1", "stack", "odd_size", "moved_cam", "cov_precomp", "clamp"])
def test_tile_culling_only_drops_dead_instances(name):
    s, grads, exp = MG.load(name)
    st = Hh.oracle_forward(s)
    got = Hh.hip_run(s, keep_state=True)  # default tuning: culling on
    kept, dropped = _check_culled_binning(s, got, st)
    assert kept == got["num_rendered"] and kept + dropped == st["num_rendered"]
    assert dropped > 0.2 * st["num_rendered"], "the 3-sigma rectangles of these scenes are mostly empty corners"
    set_tuning(tile_cull=False)
    full = Hh.hip_run(s, keep_state=True)
    P, W, H = s["means3D"].shape[0], s["W"], s["H"]
    fT = [_layout.image_views(x["img"], P, W, H)["final_T"].cpu().numpy() for x in (full, got)]
    assert np.array_equal(fT[0], fT[1]), "culling must not change a single bit of the transmittance"
    for k in ("out_color", "out_depth", "out_unc"):
        # same terms, other association (segment boundaries are list positions): rounding of a float sum, nothing more
        assert np.abs(full[k] - got[k]).max() <= 2e-6 * max(1.0, np.abs(full[k]).max()), f"{k}: culling changed the image"
    ga, gb = Hh.hip_run(s, grads), None
    set_tuning(tile_cull=True)
    gb = Hh.hip_run(s, grads)
    Hh.assert_grads_nearly_equal(gb, ga, context="cull on vs off")


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_binning_is_bit_exact(name):
    """Reference-identical binning (tile culling off): num_rendered, ranges and sorted lists bit-exact."""
    s, _, exp = MG.load(name)
    set_tuning(tile_cull=False)
    got = Hh.hip_run(s, keep_state=True)
    assert got["num_rendered"] == int(exp["num_rendered"])
    _check_binning(s, got, exp["point_list"], exp["tile_counts"])
    img = _layout.image_views(got["img"], s["means3D"].shape[0], s["W"], s["H"])
    nc = img["n_contrib"].cpu().numpy()
    assert (nc != exp["n_contrib"].astype(np.int64)).mean() < 1e-3


def test_config1_against_live_oracle():
    """BASELINE.json config 1 (2k Gaussians @128x128) with the oracle run on this box."""
    s = S.scene_config1()
    grads = S.upstream_grads(1, s["W"], s["H"])
    st = Hh.oracle_forward(s)
    ref = Hh.oracle_backward(s, st, grads)
    got = Hh.hip_run(s, grads)
    assert (got["radii"] == st["radii"]).all()
    Hh.assert_parity_strict(got, st, ref, s, grads, context="config1", nthreads=NT)
    set_tuning(tile_cull=False)
    g2 = Hh.hip_run(s, keep_state=True)
    assert g2["num_rendered"] == st["num_rendered"]
    _check_binning(s, g2, st["point_list"], st["ranges"][:, 1] - st["ranges"][:, 0])


@pytest.mark.parametrize("P,W,H,seed", [(60_000, 504, 284, 21), (20_000, 252, 142, 22),
                                        (180_000, 400, 240, 23)])  # 180k: several hundred binning chunks, odd chunk sizes
def test_slab_scene_against_live_oracle(P, W, H, seed):
    """Down-scaled config 2/3 generator (the bench workload's distribution), depth + feature heads on."""
    s = S.scene_slab(seed, P, W, H)
    grads = S.upstream_grads(seed, W, H)
    nthreads = max(1, min(16, os.cpu_count() or 1))
    st = Hh.oracle_forward(s, nthreads=nthreads)
    ref = Hh.oracle_backward(s, st, grads, nthreads=nthreads)
    got = Hh.hip_run(s, grads)
    assert (got["radii"] == st["radii"]).all()
    Hh.assert_parity_strict(got, st, ref, s, grads, context=f"slab{P}", nthreads=NT)
    kept, dropped = _check_culled_binning(s, Hh.hip_run(s, keep_state=True), st)
    assert kept + dropped == st["num_rendered"]
    set_tuning(tile_cull=False)
    g2 = Hh.hip_run(s, keep_state=True)
    assert g2["num_rendered"] == st["num_rendered"]
    _check_binning(s, g2, st["point_list"], st["ranges"][:, 1] - st["ranges"][:, 0])


def test_surface_scene_against_live_oracle():
    """A cloud shaped like a trained scene (synthetic.scene_surfaces, the bench's `surfaces` workload scaled down): 85 % of the
    Gaussians on six thin surfaces -- per-tile depth keys in clusters (the tile sort's second counting level does the work), the
    front surface saturates most pixels early (short walks, many threshold decisions near T = 1e-4)."""
    P, W, H, seed = 90_000, 504, 284, 31
    s = S.scene_surfaces(seed, P, W, H)
    grads = S.upstream_grads(seed, W, H)
    nthreads = max(1, min(16, os.cpu_count() or 1))
    st = Hh.oracle_forward(s, nthreads=nthreads)
    ref = Hh.oracle_backward(s, st, grads, nthreads=nthreads)
    got = Hh.hip_run(s, grads)
    assert (got["radii"] == st["radii"]).all()
    Hh.assert_parity_strict(got, st, ref, s, grads, context="surfaces", nthreads=NT)
    kept, dropped = _check_culled_binning(s, Hh.hip_run(s, keep_state=True), st)
    assert kept + dropped == st["num_rendered"]
    set_tuning(tile_cull=False)
    g2 = Hh.hip_run(s, keep_state=True)
    assert g2["num_rendered"] == st["num_rendered"]
    _check_binning(s, g2, st["point_list"], st["ranges"][:, 1] - st["ranges"][:, 0])


@pytest.mark.parametrize("P,W,H,expect_class", [(14_000, 32, 32, "large"), (40_000, 32, 16, "global")])
def test_long_tile_lists_use_the_big_sort_paths(P, W, H, expect_class):
    """Tiny image + big cloud: per-tile lists beyond the 4096-entry LDS sort (-> 128 KiB LDS variant) and beyond
    16384 (-> global-memory variant).  The sorted lists must still equal the oracle's."""
    s = S.scene_config1(seed=31, P=P, W=W, H=H, lateral=0.3)
    s["scales"] *= 0.15
    st = Hh.oracle_forward(s)
    mx = int((st["ranges"][:, 1] - st["ranges"][:, 0]).max())
    assert (4096 < mx <= 16384) if expect_class == "large" else (mx > 16384), mx
    set_tuning(tile_cull=False, partial_sort=False)
    got = Hh.hip_run(s, keep_state=True)
    assert got["num_rendered"] == st["num_rendered"]
    _check_binning(s, got, st["point_list"], st["ranges"][:, 1] - st["ranges"][:, 0])
    Hh.assert_parity_strict(got, st, context="images", nthreads=NT)


@pytest.mark.parametrize("scale_mul,expect_fixup", [(6.0, False), (0.15, True)])
def test_partial_sort_of_long_lists(scale_mul, expect_fixup):
    """Lists beyond 2048 entries are depth-sorted only for their nearest <= 2048 instances (binning.hip).  With big
    splats every pixel saturates inside that prefix; with small ones most pixels never saturate, the tiles are flagged,
    sorted completely and blended again.  Either way images and gradients must match the oracle, the sorted prefix must
    be the oracle's list prefix, and the rest of each list must hold the remaining ids (in any order)."""
    s = S.scene_config1(seed=33, P=14_000, W=32, H=32, lateral=0.3)
    s["scales"] *= np.float32(scale_mul)
    if not expect_fixup:
        s["opacities"] = np.maximum(s["opacities"], np.float32(0.6))
    grads = S.upstream_grads(9, s["W"], s["H"])
    st = Hh.oracle_forward(s)
    ref = Hh.oracle_backward(s, st, grads)
    counts = st["ranges"][:, 1] - st["ranges"][:, 0]
    assert counts.max() > 4096
    set_tuning(tile_cull=False)  # the oracle's lists; partial sort stays on
    got = Hh.hip_run(s, grads, keep_state=True)
    assert got["num_rendered"] == st["num_rendered"]
    P, R = s["means3D"].shape[0], got["num_rendered"]
    img = _layout.image_views(got["img"], P, s["W"], s["H"])
    slen = img["sorted_len"].cpu().numpy().astype(np.int64)
    flagged = img["need_full"].cpu().numpy().astype(bool)
    assert flagged.any() == expect_fixup, (flagged.sum(), expect_fixup)
    pl = _layout.binning_views(got["binning"], R, got["binning_capacity"])["point_list"].cpu().numpy().astype(np.int64)
    partial = 0
    for tile, (a, b) in enumerate(st["ranges"]):
        a, b, m = int(a), int(b), int(slen[tile])
        if b - a <= 2048 or flagged[tile]:
            assert m == b - a and (pl[a:b] == st["point_list"][a:b]).all(), "short and redone lists are sorted completely"
        else:
            partial += 1
            assert 0 < m <= 2048 and (pl[a:a + m] == st["point_list"][a:a + m]).all(), "sorted prefix = the oracle's nearest instances"
            assert (np.sort(pl[a + m:b]) == np.sort(st["point_list"][a + m:b].astype(np.int64))).all(), "the rest: same ids, any order"
    assert (partial > 0) or expect_fixup
    Hh.assert_parity_strict(got, st, context=f"partial sort, scales x{scale_mul}: images", nthreads=NT)
    # (keep_state runs no backward: the gradients -- and where every walk ended -- come from a second call through the public API)
    Hh.assert_parity_strict(Hh.hip_run(s, grads), st, ref, s, grads, context=f"partial sort, scales x{scale_mul}", nthreads=NT)


def test_partial_sort_bet_is_dropped_after_it_was_lost():
    """Round 6 (api.hip gsr_partial_bet): on a frame where nothing saturates every long list loses the partial sort's bet -- its tile is
    sorted a second time and its quadrants resume in a second forward-blend launch.  A resumed quadrant reports the forward's serial
    number through a host-mapped word; the thread's next forwards then sort lists of up to 4096 entries completely at once (no flagged
    tile, no resumed quadrant), with the same bits; gsr_adaptive_reset (set_tuning) makes the next forward bet again."""
    import torch
    from gscream_amd import rasterizer as RZ
    s = S.scene_config1(seed=33, P=7_000, W=32, H=32, lateral=0.3)
    s["scales"] *= np.float32(0.15)                       # small faint splats: most pixels never saturate
    st = Hh.oracle_forward(s)
    counts = (st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0])
    assert 2048 < counts.max() <= 4096 and (counts > 2048).sum() >= 2, counts.max()
    P, W, H = s["means3D"].shape[0], s["W"], s["H"]

    def run():
        got = Hh.hip_run(s, keep_state=True)
        iv = _layout.image_views(got["img"], P, W, H)
        torch.cuda.synchronize()                          # (the report of this forward has landed)
        return got, iv["need_full"].cpu().numpy().astype(bool), iv["sorted_len"].cpu().numpy().astype(np.int64)

    set_tuning(tile_cull=False)                           # the oracle's lists; resets the library's feedback state
    a, flagged_a, _ = run()                               # two-stage (no capacity history yet): bets, loses
    assert flagged_a[counts > 2048].any(), "the scene must lose the bet"
    b, flagged_b, slen_b = run()                          # speculative, bet off: complete sorts at once
    assert RZ._last_stage1["speculative"] is True
    assert not flagged_b.any() and (slen_b == counts).all(), (int(flagged_b.sum()), int((slen_b != counts).sum()))
    c, flagged_c, slen_c = run()
    assert not flagged_c.any() and (slen_c == counts).all()
    for k in ("out_color", "out_depth", "out_unc", "radii"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    Hh.assert_parity_strict(b, st, context="bet off: images", nthreads=NT)
    RZ._native.load().gsr_adaptive_reset()                # (what set_tuning does, without clearing the capacity history)
    d, flagged_d, _ = run()
    assert RZ._last_stage1["speculative"] is True and flagged_d[counts > 2048].any(), "after a reset the next forward bets again"
    for k in ("out_color", "out_depth", "out_unc", "radii"):
        assert np.array_equal(a[k], d[k]), k
    # gradients: bet on vs bet off, same bits
    grads = S.upstream_grads(9, W, H)
    set_tuning(tile_cull=False)
    g_on = Hh.hip_run(s, grads)
    torch.cuda.synchronize()
    g_off = Hh.hip_run(s, grads)
    for k in Hh.GRAD_KEYS:
        if k in g_on:
            assert np.array_equal(g_on[k], g_off[k]), k


def test_speculative_hint_exactly_at_the_partial_sort_cap():
    """A caller of the C ABI may pass max_tile_count_hint == GSR_NEAR_CAP (2048) while a real list is longer: the prefix-sort
    kernel is only launched for provisions > 2048, so the call must come back as NEED_CAPACITY and be redone, never
    return tiles rendered as background."""
    from gscream_amd import rasterizer as RZ
    s = S.scene_config1(seed=33, P=14_000, W=32, H=32, lateral=0.3)
    s["scales"] *= np.float32(6.0)
    s["opacities"] = np.maximum(s["opacities"], np.float32(0.6))
    st = Hh.oracle_forward(s)
    assert (st["ranges"][:, 1] - st["ranges"][:, 0]).max() > 2048
    set_tuning()
    ref = Hh.hip_run(s)
    for hint in (2048, 2049, 1024):
        RZ._capacity_hint[0] = (1 << 22, hint)
        got = Hh.hip_run(s)
        assert RZ._last_stage1["speculative"] is (hint > 2048), (hint, RZ._last_stage1)
        for k in ("out_color", "out_depth", "out_unc", "radii"):
            assert np.array_equal(got[k], ref[k]), (hint, k)
    Hh.assert_parity_strict(ref, st, context="hint at the cap", nthreads=NT)


@pytest.mark.parametrize("clustered_frac", [0.3, 0.6, 1.0])
def test_tile_sort_with_depth_clusters(clustered_frac):
    """The O(n) bucket sort of the tile lists spreads the keys over 1024 equal-width buckets of the tile's depth range;
    Gaussians sitting on a few exact depth planes put hundreds of keys into one bucket.  30 % of the cloud on two planes:
    those buckets are sorted on their own; the whole cloud on eight planes: the tile falls back to the sorting network;
    60 % on forty planes: dozens of buckets of 17 - 64 keys per tile, each sorted by one wave (rank by counting).
    The lists must equal the oracle's either way (ties on a plane -> ascending id)."""
    s = S.scene_config1(seed=35, P=4500, W=64, H=64, lateral=0.3)
    s["scales"] *= 0.5
    rng = np.random.default_rng(35)
    z = s["means3D"][:, 2]
    planes = (np.array([2.5, 4.0], np.float32) if clustered_frac < 0.5 else
              np.linspace(2.2, 5.8, 40 if clustered_frac < 1.0 else 8).astype(np.float32))
    pick = rng.random(z.shape[0]) < clustered_frac
    scale = np.where(pick, planes[rng.integers(0, len(planes), z.shape[0])] / z, 1.0).astype(np.float32)
    s["means3D"] = (s["means3D"] * scale[:, None]).astype(np.float32)  # same pixel, depth snapped to a plane
    st = Hh.oracle_forward(s)
    counts = st["ranges"][:, 1] - st["ranges"][:, 0]
    assert 300 < counts.max() <= 2048
    set_tuning(tile_cull=False)
    got = Hh.hip_run(s, keep_state=True)
    assert got["num_rendered"] == st["num_rendered"]
    _check_binning(s, got, st["point_list"], counts)
    Hh.assert_parity_strict(got, st, context="images", nthreads=NT)


def test_filters_match_oracle_and_known_answers():
    from oracle import oracle as O
    from gscream_amd import GaussianRasterizer
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "filter_known_answers.npz"))
    W, H, tfx = int(z["W"]), int(z["H"]), float(z["tanfovx"])
    s = S.scene_config1(seed=40, P=5, W=W, H=H, tanfovx=tfx)
    s["means3D"] = z["points"].copy()
    s["scales"] = np.full((5, 3), float(z["scale"]), np.float32)
    s["rotations"] = np.tile(np.array([1, 0, 0, 0], np.float32), (5, 1))
    r = GaussianRasterizer(raster_settings=Hh.hip_settings(s))
    t = lambda a: torch.from_numpy(a).cuda()
    radii, x, y = r.position2D_filter(t(s["means3D"]), scales=t(s["scales"]), rotations=t(s["rotations"]))
    assert radii.dtype == torch.int32 and x.dtype == torch.float32 and radii.is_cuda
    assert (radii.cpu().numpy() == z["radii"]).all()
    np.testing.assert_allclose(x.cpu().numpy(), z["x"], atol=2e-3)
    np.testing.assert_allclose(y.cpu().numpy(), z["y"], atol=2e-3)
    assert (r.visible_filter(t(s["means3D"]), scales=t(s["scales"]), rotations=t(s["rotations"])).cpu().numpy() == z["radii"]).all()
    vis = r.markVisible(t(s["means3D"]))
    assert vis.dtype == torch.bool and (vis.cpu().numpy().astype(np.uint8) == z["visible"]).all()

    # anchor-like cloud with a moved camera; scales passed as the strided slice GScream uses
    # (gaussian_renderer/__init__.py:297: scales[:, :3] of a [N, 6] tensor)
    rng = np.random.default_rng(41)
    s = S.scene_config1(seed=41, P=20_000, W=252, H=142, lateral=0.8, w2c=S.random_w2c(rng), cx=0.03, cy=0.02)
    kw = Hh.cam_kwargs(s)
    ro, xo, yo = O.position2D_filter(s["means3D"], s["scales"], s["rotations"], **kw)
    r = GaussianRasterizer(raster_settings=Hh.hip_settings(s))
    scal6 = torch.cat([t(s["scales"]), torch.rand(20_000, 3, device="cuda")], 1)
    radii, x, y = r.position2D_filter(t(s["means3D"]), scales=scal6[:, :3], rotations=t(s["rotations"]))
    assert (radii.cpu().numpy() == ro).all()
    assert np.array_equal(x.cpu().numpy(), xo) and np.array_equal(y.cpu().numpy(), yo), "pixel centres are bit-exact"
    assert (r.visible_filter(t(s["means3D"]), scales=scal6[:, :3], rotations=t(s["rotations"])).cpu().numpy() == ro).all()
    assert (r.markVisible(t(s["means3D"])).cpu().numpy() == O.mark_visible(s["means3D"], s["viewmatrix"])).all()


def test_preprocess_outputs_are_bit_exact():
    """means2D, conic, depth, rect, tiles, offsets straight out of the geometry records vs the oracle."""
    rng = np.random.default_rng(50)
    s = S.scene_config1(seed=50, P=30_000, W=320, H=200, lateral=0.8, w2c=S.random_w2c(rng), cx=-0.02, cy=0.05)
    st = Hh.oracle_forward(s)
    set_tuning(tile_cull=False)
    got = Hh.hip_run(s, keep_state=True)
    P = 30_000
    gv = _layout.geom_views(got["geom"], P)
    vis = st["radii"] > 0
    rec = gv["rec_f32"].cpu().numpy()
    assert (got["radii"] == st["radii"]).all()
    assert np.array_equal(rec[vis, 0:2], st["means2D"][vis]), "pixel centres"
    # the record keeps the RAW conic (round 4: the blend kernels scale it per staged instance and re-check decisions inside
    # the alpha = 1/255 guard band with the reference's own expression on it): bit-equal to the oracle's
    assert np.array_equal(rec[vis, 2:5], st["conic_opacity"][vis, :3]), "conic"
    assert np.array_equal(rec[vis, 5], st["conic_opacity"][vis, 3]) and np.array_equal(rec[vis, 6], st["depths"][vis])
    assert np.array_equal(rec[vis, 7], st["unc"][vis]) and np.array_equal(rec[vis, 8:11], s["colors"][vis])
    tiles = gv["tiles"].cpu().numpy().astype(np.int64)
    assert (tiles == st["tiles_touched"].astype(np.int64)).all()
    offs = gv["offsets"].cpu().numpy().astype(np.int64)
    assert (offs == np.concatenate([[0], np.cumsum(tiles)[:-1]])).all(), "exclusive scan of tiles_touched"
    # record tail: {rectangle width, x0 | y0 << 16, survivor mask lo, hi} (the slot offset lives in offsets[], written by the scatter);
    # word 11: the Gaussian's culling threshold ln(255 opacity) + margins (round 5: read by the blend kernels' box tests)
    tail = gv["rec_i32"].cpu().numpy()[vis, 12:16].astype(np.int64) & 0xffffffff
    rect = gv["rect"].cpu().numpy().astype(np.int64)[vis] & 0xffffffff
    assert (tail[:, 0] == (rect[:, 0] >> 16) - (rect[:, 0] & 0xffff)).all() and (tail[:, 1] == ((rect[:, 0] & 0xffff) | ((rect[:, 1] & 0xffff) << 16))).all()
    tau = rec[vis, 11].astype(np.float64)
    plain = np.log(255.0 * s["opacities"][vis, 0].astype(np.float64))
    assert (tau >= plain + 0.0099).all() and (tau <= plain + 0.0101 + 1e-6 * 3.0 * np.abs(rec[vis, 2:5]).max(axis=1) * (st["radii"][vis] + 16.0) ** 2 + 1e-5).all()


def test_empty_and_degenerate_inputs():
    from gscream_amd import GaussianRasterizer
    s = S.scene_config1(seed=60, P=0, W=40, H=24)
    got = Hh.hip_run(s, S.upstream_grads(1, 40, 24))
    assert got["out_color"].shape == (3, 24, 40) and not got["out_color"].any() and got["radii"].shape == (0,)
    assert got["dL_dmeans3D"].shape == (0, 3)
    # all culled: image = background, every gradient exactly zero
    s, grads, exp = MG.load("all_culled")
    got = Hh.hip_run(s, grads)
    assert np.allclose(got["out_color"], s["bg"][:, None, None]) and not got["out_depth"].any()
    assert not got["dL_dmeans3D"].any() and not got["dL_dcolors"].any()
    # single Gaussian, single pixel image
    s = S.scene_config1(seed=61, P=1, W=1, H=1)
    s["means3D"][:] = [0, 0, 3]
    got = Hh.hip_run(s, S.upstream_grads(2, 1, 1))
    st = Hh.oracle_forward(s)
    Hh.assert_images_close(got["out_color"], st["out_color"], "1x1")
    r = GaussianRasterizer(raster_settings=Hh.hip_settings(s))
    assert r.visible_filter(torch.zeros(0, 3, device="cuda"), scales=torch.zeros(0, 3, device="cuda"),
                            rotations=torch.zeros(0, 4, device="cuda")).shape == (0,)


def test_render_call_pattern_of_gaussian_renderer():
    """Replays gaussian_renderer/__init__.py:120-158: keyword call, screenspace_points = zeros + 0 with
    retain_grad, settings built the same way; checks shapes / dtypes / devices of everything returned."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    s = S.scene_config1(seed=70, P=3000, W=160, H=96)
    t = lambda a: torch.from_numpy(a).cuda()
    xyz = t(s["means3D"]).requires_grad_(True)
    color, opacity, unc = t(s["colors"]).requires_grad_(True), t(s["opacities"]).requires_grad_(True), t(s["uncertainties"]).requires_grad_(True)
    scaling, rot = t(s["scales"]).requires_grad_(True), t(s["rotations"]).requires_grad_(True)
    screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True, device="cuda") + 0
    screenspace_points.retain_grad()
    rs = GaussianRasterizationSettings(image_height=int(s["H"]), image_width=int(s["W"]), tanfovx=s["tanfovx"], tanfovy=s["tanfovy"],
                                       bg=t(s["bg"]), scale_modifier=1.0, viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]),
                                       sh_degree=1, campos=t(s["campos"]), prefiltered=False, debug=False)
    rasterizer = GaussianRasterizer(raster_settings=rs)
    rendered_image, rendered_depth, uncer, radii = rasterizer(
        means3D=xyz, means2D=screenspace_points, shs=None, colors_precomp=color, opacities=opacity,
        uncertainties=unc, scales=scaling, rotations=rot, cov3D_precomp=None)
    assert rendered_image.shape == (3, 96, 160) and rendered_depth.shape == (1, 96, 160) and uncer.shape == (1, 96, 160)
    assert radii.shape == (3000,) and radii.dtype == torch.int32 and not radii.requires_grad
    assert all(x.is_cuda and x.dtype == torch.float32 for x in (rendered_image, rendered_depth, uncer))
    visibility_filter = radii > 0
    loss = rendered_image.mean() + 0.1 * rendered_depth.mean()  # the uncertainty map is unused by train.py:532
    loss.backward(retain_graph=True)
    assert screenspace_points.grad.shape == (3000, 3) and screenspace_points.grad[visibility_filter, :2].abs().sum() > 0
    assert xyz.grad.shape == (3000, 3) and opacity.grad.shape == (3000, 1) and unc.grad.shape == (3000, 1)
    assert not unc.grad.any(), "no loss on the feature map -> zero feature gradient"
    # a second backward over the same saved forward state
    g1 = xyz.grad.clone()
    xyz.grad = None
    loss.backward(retain_graph=True)
    # the backward is bit-reproducible (per-wavefront LDS accumulators added in a fixed order)
    assert torch.equal(xyz.grad, g1), f"second backward differs by {(xyz.grad - g1).abs().max().item()}"
    # ... and a third one with OTHER upstream gradients: the flags the earlier backwards left set mark exactly the slots any
    # backward of this forward writes (the traversal depends on the forward state only), so nothing stale can be summed
    gen = torch.Generator(device="cuda").manual_seed(5)
    wimg = torch.rand(rendered_image.shape, device="cuda", generator=gen)
    wdep = torch.rand(rendered_depth.shape, device="cuda", generator=gen)
    leaves = (xyz, color, opacity, scaling, rot)
    got = torch.autograd.grad((rendered_image * wimg).sum() + (rendered_depth * wdep).sum(), leaves, retain_graph=True)
    fresh = rasterizer(means3D=xyz, means2D=screenspace_points, shs=None, colors_precomp=color, opacities=opacity,
                       uncertainties=unc, scales=scaling, rotations=rot, cov3D_precomp=None)
    want = torch.autograd.grad((fresh[0] * wimg).sum() + (fresh[1] * wdep).sum(), leaves)
    for g, w_ in zip(got, want):
        assert torch.equal(g, w_), "backward over a reused forward state differs from a fresh forward + backward"
    with torch.no_grad():  # eval path, train.py:756-763
        img2 = rasterizer(means3D=xyz, means2D=screenspace_points, shs=None, colors_precomp=color, opacities=opacity,
                          uncertainties=unc, scales=scaling, rotations=rot, cov3D_precomp=None)[0]
    assert torch.equal(img2, rendered_image)


def test_debug_mode_and_determinism():
    s, grads, exp = MG.load("cfg1")
    a = Hh.hip_run(s, grads, debug=True)
    b = Hh.hip_run(s, grads)
    c = Hh.hip_run(s, grads)
    for k in ("out_color", "out_depth", "out_unc"):
        assert np.array_equal(b[k], c[k]) and np.array_equal(a[k], b[k]), f"{k}: the forward is bit-reproducible"
    # no float atomics anywhere; each wavefront of a backward task adds into its own LDS accumulator and the two are
    # summed in a fixed order: gradients are bit-reproducible too
    for k in Hh.GRAD_KEYS:
        assert np.array_equal(b[k], c[k]) and np.array_equal(a[k], b[k]), f"{k}: the backward is bit-reproducible"


def test_prefiltered_promise_is_checked_in_debug_mode(tmp_path, monkeypatch):
    """DGR auxiliary.h:154-162: a point that fails the near plane although `prefiltered` is set is a contract violation (the
    reference prints and traps the kernel).  Here: an error of the call in debug mode, ignored otherwise."""
    from gscream_amd import GaussianRasterizer
    monkeypatch.chdir(tmp_path)  # debug mode dumps snapshot_fw.dump on failure, like the reference
    s = S.scene_config1(seed=3, P=500, W=64, H=64)
    s["means3D"][:7, 2] = 0.1  # seven points in front of the near plane (view-space z <= 0.2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = dict(means3D=t(s["means3D"]), means2D=torch.zeros(500, 3, device="cuda"), opacities=t(s["opacities"]),
                uncertainties=t(s["uncertainties"]), colors_precomp=t(s["colors"]), scales=t(s["scales"]), rotations=t(s["rotations"]))
    base = Hh.hip_settings(s)
    ref = GaussianRasterizer(base)(**args)
    out = GaussianRasterizer(base._replace(prefiltered=True))(**args)           # not debug: the flag changes nothing
    assert all(torch.equal(a, b) for a, b in zip(ref, out)) and int((out[3][:7] == 0).sum()) == 7
    with pytest.raises(RuntimeError, match="Point is filtered although prefiltered is set.*7 of 500"):
        GaussianRasterizer(base._replace(prefiltered=True, debug=True))(**args)
    with pytest.raises(RuntimeError, match="Point is filtered although prefiltered is set"):
        GaussianRasterizer(base._replace(prefiltered=True, debug=True)).visible_filter(args["means3D"], args["scales"], args["rotations"])
    s["means3D"][:7, 2] = 3.0                                                   # promise kept: debug mode passes
    args["means3D"] = t(s["means3D"])
    a = GaussianRasterizer(base._replace(prefiltered=True, debug=True))(**args)
    b = GaussianRasterizer(base)(**args)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_non_default_stream_and_strided_inputs():
    s, grads, exp = MG.load("cfg1")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = Hh.hip_run(s, grads)
    st.synchronize()
    for k in ("out_color", "out_depth", "out_unc"):
        Hh.assert_images_close(got[k], exp[k], k)
    from gscream_amd import GaussianRasterizer
    t = lambda a: torch.from_numpy(a).cuda()
    big = torch.zeros(s["means3D"].shape[0], 7, device="cuda")
    big[:, 2:5] = t(s["means3D"])
    r = GaussianRasterizer(raster_settings=Hh.hip_settings(s))
    img = r(big[:, 2:5], torch.zeros(s["means3D"].shape[0], 3, device="cuda"), t(s["opacities"]), t(s["uncertainties"]),
            colors_precomp=t(s["colors"]), scales=t(s["scales"]), rotations=t(s["rotations"]))[0]
    Hh.assert_images_close(img.cpu().numpy(), exp["out_color"], "strided means3D")


def test_speculative_forward_and_capacity_overflow():
    """gsr_forward enqueues stage 2 before the host knows num_rendered, against a workspace sized from previous
    frames.  A too-small guess must be detected and redone; a sufficient one must give the same bits as the
    two-stage path."""
    from gscream_amd import rasterizer as RZ
    s, grads, exp = MG.load("cfg1")
    set_tuning(speculative=False)
    ref = Hh.hip_run(s, grads)
    assert RZ._last_stage1["speculative"] is False
    set_tuning()                                   # clears the capacity history: first call is two-stage
    a = Hh.hip_run(s, grads)
    assert RZ._last_stage1["speculative"] is False and RZ._capacity_hint[0][0] > int(exp["num_rendered"])
    b = Hh.hip_run(s, grads)                        # now speculative, capacity sufficient
    assert RZ._last_stage1["speculative"] is True and RZ._last_stage1["binning_capacity"] >= RZ._last_stage1["num_rendered"]
    RZ._capacity_hint[0] = (64, 4096)               # far too small: kernels must not write out of bounds, call is redone
    c = Hh.hip_run(s, grads)
    assert RZ._last_stage1["speculative"] is False and RZ._last_stage1["binning_capacity"] == RZ._last_stage1["num_rendered"]
    for got in (a, b, c):
        for k in ("out_color", "out_depth", "out_unc", "radii"):
            assert np.array_equal(got[k], ref[k]), k
        Hh.assert_grads_nearly_equal(got, ref, context="speculative vs two-stage")
    RZ._capacity_hint[0] = (1 << 20, 8)              # workspace fine, but the longest list exceeds the hinted sort variant
    d = Hh.hip_run(s, grads)
    assert RZ._last_stage1["speculative"] is False
    for k in ("out_color", "out_depth", "out_unc", "radii"):
        assert np.array_equal(d[k], ref[k]), k
    st = Hh.hip_run(s, keep_state=True)             # speculative again, oversized workspace: lists still exact
    assert st["binning_capacity"] > st["num_rendered"]
    set_tuning(tile_cull=False)
    Hh.hip_run(s)
    st = Hh.hip_run(s, keep_state=True)
    assert RZ._last_stage1["speculative"] is True
    _check_binning(s, st, exp["point_list"], exp["tile_counts"])


def _vs_oracle(s, grads, name, img_frac=2e-5):
    st = Hh.oracle_forward(s)
    ref = Hh.oracle_backward(s, st, grads)
    got = Hh.hip_run(s, grads)
    assert (got["radii"] == st["radii"]).all(), f"{name}: radii"
    Hh.assert_parity_strict(got, st, ref, s, grads, context=name, nthreads=NT)
    assert all(np.isfinite(v).all() for k, v in got.items() if k.startswith("dL_"))
    return st, got


@pytest.mark.parametrize("variant", Hh.VARIANTS)
def test_more_cases_against_live_oracle(variant):
    s, grads = Hh.variant_scene(variant)
    st, got = _vs_oracle(s, grads, variant)
    if variant == "huge_gaussians":
        gx, gy = (s["W"] + 15) // 16, (s["H"] + 15) // 16
        assert st["tiles_touched"].max() > 64 and st["tiles_touched"].max() <= gx * gy
        # the first 64 Gaussians own far more than 1024 gradient slots: the per-Gaussian backward's cooperative (heavy-group)
        # kernel did their sums above; it must be as bit-reproducible as the one-wave path
        assert int(got["radii"][:64].astype(bool).sum()) > 0 and int(st["tiles_touched"][:64].sum()) > 4096
        # ... and the same bits come out of the one-wave kernel, which does the heavy groups itself when the caller's previous
        # backwards met too few to pay for the second launch (automatic mode: api.hip, gsr_heavy_groups_expected)
        set_tuning(heavy_groups=False)
        inline = Hh.hip_run(s, grads)                    # heavy groups done inline
        set_tuning(heavy_groups=True)
        again = Hh.hip_run(s, grads)                     # ... by the cooperative kernel
        set_tuning()
        for k in Hh.GRAD_KEYS:
            if k in got:
                assert np.array_equal(got[k], again[k]), f"{k}: the heavy-group backward is bit-reproducible"
                assert np.array_equal(inline[k], again[k]), f"{k}: one-wave and cooperative heavy-group sums differ"
        set_tuning(tile_cull=False)
        full = Hh.hip_run(s, keep_state=True)
        assert full["num_rendered"] == st["num_rendered"]
        _check_binning(s, full, st["point_list"], st["ranges"][:, 1] - st["ranges"][:, 0])


@pytest.mark.parametrize("deg", [0, 1, 2])
def test_sh_degree_ramp_leaves_unused_coefficients_with_zero_gradient(deg):
    """The usual 3DGS ramp: M = 16 coefficients allocated, only (deg+1)^2 active.  The gradient rows of the inactive
    coefficients must be exact zeros (the reference zero-fills dL_dsh, rasterize_points.cu:168) although the gradient
    tensors are torch.empty -- the allocator is poisoned first so stale memory would show."""
    rng = np.random.default_rng(300 + deg)
    s = S.scene_config1(seed=310 + deg, P=1500, W=112, H=80)
    s["shs"] = rng.normal(0, 0.35, size=(1500, 16, 3)).astype(np.float32)
    s["sh_degree"] = deg
    del s["colors"]
    grads = S.upstream_grads(91, s["W"], s["H"])
    poison = [torch.full((1500 * 16 * 3,), float("nan"), device="cuda") for _ in range(8)]
    del poison
    st, got = _vs_oracle(s, grads, f"sh_ramp_deg{deg}")
    n = (deg + 1) ** 2
    assert got["dL_dsh"].shape == (1500, 16, 3)
    assert (got["dL_dsh"][:, n:, :] == 0).all(), "inactive SH coefficients must get exact zeros"
    assert np.abs(got["dL_dsh"][:, :n, :]).max() > 0


def test_non_finite_inputs_do_not_fault():
    """NaN / inf inputs must never drive a kernel out of bounds: such Gaussians are culled (radius 0) or blended as
    garbage-in-garbage-out, but the call returns and the finite Gaussians' radii are untouched."""
    s = S.scene_config1(seed=95, P=2000, W=128, H=96)
    clean = Hh.oracle_forward(s)["radii"]
    bad = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in s.items()}
    bad["means3D"][0] = np.nan
    bad["means3D"][1] = [np.inf, 0, 3]
    bad["means3D"][2] = [0, 0, np.inf]
    bad["scales"][3] = np.nan
    bad["scales"][4] = np.inf
    bad["rotations"][5] = np.nan
    bad["scales"][6] = 1e30
    bad["means3D"][7] = [1e30, -1e30, 5]
    got = Hh.hip_run(bad, S.upstream_grads(3, 128, 96))
    torch.cuda.synchronize()
    assert (got["radii"][8:] == clean[8:]).all()
    assert got["radii"][0] == 0 and got["radii"][3] == 0 and got["radii"][5] == 0


def test_image_beyond_the_lds_tile_limit():
    """More than 36 864 tiles (3200x3200 px = 40 000 tiles): the binning falls back to global counters; results must
    match the oracle exactly as for ordinary sizes."""
    W = H = 3200
    s = S.scene_config1(seed=77, P=1500, W=W, H=H)
    # spread the cloud over the big frame and make the splats large enough to span several tiles
    s["scales"] = (s["scales"] * np.float32(0.5)).astype(np.float32)
    grads = S.upstream_grads(5, W, H)
    st = Hh.oracle_forward(s, nthreads=max(1, min(16, os.cpu_count() or 1)))
    ref = Hh.oracle_backward(s, st, grads, nthreads=max(1, min(16, os.cpu_count() or 1)))
    got = Hh.hip_run(s, grads)
    assert (got["radii"] == st["radii"]).all()
    # (splats of up to 400 px radius sum ~1e5 pixel contributions each; rounds 1-5 gave this case a looser bar -- measured in round 6:
    # worst element 1.1e-4, it needs none)
    Hh.assert_parity_strict(got, st, ref, s, grads, context="huge image", nthreads=NT)
    set_tuning(tile_cull=False)
    g2 = Hh.hip_run(s, keep_state=True)
    assert g2["num_rendered"] == st["num_rendered"]
    _check_binning(s, g2, st["point_list"], st["ranges"][:, 1] - st["ranges"][:, 0])


@pytest.mark.parametrize("absent", ["depth", "uncertainty"])
def test_one_absent_auxiliary_gradient_equals_zeros(absent):
    """A loss that touches the image and only ONE of the two auxiliary maps (train.py:532-561 uses depth, never the uncertainty map):
    the absent upstream gradient reaches the kernel as NULL, not as a zero-filled map -- same bits as explicit zeros."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    s = S.scene_config1(seed=33, P=2500, W=144, H=80)
    t = lambda a: torch.from_numpy(a).cuda()
    rs = GaussianRasterizationSettings(image_height=int(s["H"]), image_width=int(s["W"]), tanfovx=s["tanfovx"], tanfovy=s["tanfovy"],
                                       bg=t(s["bg"]), scale_modifier=1.0, viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]),
                                       sh_degree=1, campos=t(s["campos"]), prefiltered=False, debug=False)
    gc, gd, gu = (t(g) for g in S.upstream_grads(34, s["W"], s["H"]))
    res = []
    for explicit_zeros in (False, True):
        leaves = [t(s[k]).requires_grad_(True) for k in ("means3D", "opacities", "uncertainties", "colors", "scales", "rotations")]
        m3, op, un, col, sc, rot = leaves
        img, dep, unc, _ = GaussianRasterizer(rs)(means3D=m3, means2D=torch.zeros_like(m3, requires_grad=True), opacities=op, uncertainties=un,
                                                 colors_precomp=col, scales=sc, rotations=rot)
        outs, gos = [img], [gc]
        for name, o, g in (("depth", dep, gd), ("uncertainty", unc, gu)):
            if name != absent:
                outs.append(o); gos.append(g)
            elif explicit_zeros:
                outs.append(o); gos.append(torch.zeros_like(g))
        res.append(torch.autograd.grad(outs, leaves, gos, allow_unused=True))
    for a, b in zip(*res):
        if a is None or b is None:  # a head nothing flowed into at all
            assert (a is None or not a.any()) and (b is None or not b.any())
        else:
            assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["slab", "long_lists_resume", "beyond_lds_tiles"])
def test_inference_forward_is_bit_identical_to_the_training_forward(case):
    """Rendering under torch.no_grad() (the reference's eval / FPS loops, train.py:756-763,861-878) takes the inference
    forward (gsr_tuning.inference: no checkpoints, contributor counts, traversal depths, slot offsets): images and radii
    must equal the training forward bit for bit -- also when quadrants run off a partially sorted prefix and resume from
    the state they left (the one case in which the inference kernel stores per-pixel state)."""
    import torch
    if case == "slab":
        s = S.scene_slab(5, 60_000, 504, 284)
    elif case == "long_lists_resume":
        s = S.scene_config1(seed=33, P=14_000, W=32, H=32, lateral=0.3)
        s["scales"] *= np.float32(0.15)
    else:
        s = S.scene_slab(6, 40_000, 3200, 3200)
    train = Hh.hip_run(s, S.upstream_grads(1, s["W"], s["H"]))  # inputs require grad -> the autograd node
    from gscream_amd import GaussianRasterizer
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rast = GaussianRasterizer(raster_settings=Hh.hip_settings(s))
    kw = dict(means3D=t(s["means3D"]), means2D=torch.zeros(s["means3D"].shape, device="cuda"), opacities=t(s["opacities"]),
              uncertainties=t(s["uncertainties"]), colors_precomp=t(s["colors"]), scales=t(s["scales"]), rotations=t(s["rotations"]))
    leaf = kw["means3D"].clone().requires_grad_(True)
    with torch.no_grad():  # grad mode off, even with a leaf that requires grad
        c0, d0, u0, r0 = rast(**dict(kw, means3D=leaf))
    c1, d1, u1, r1 = rast(**kw)  # grad mode on, nothing requires grad
    assert not c0.requires_grad and not c1.requires_grad
    for (c, d, u, r) in ((c0, d0, u0, r0), (c1, d1, u1, r1)):
        assert np.array_equal(c.cpu().numpy(), train["out_color"]) and np.array_equal(d.cpu().numpy(), train["out_depth"])
        assert np.array_equal(u.cpu().numpy(), train["out_unc"]) and np.array_equal(r.cpu().numpy(), train["radii"])


@pytest.mark.gpu
@pytest.mark.parametrize("bands", [2, 3, 8, 64])
def test_banded_scatter_gives_the_same_lists(bands):
    """gsr_tuning.scatter_bands: the scatter launch split into bands of tile rows per chunk (what large images / instance counts
    take automatically, binning.hip) must produce the reference's lists bit for bit -- big splats spanning several bands, rectangles
    beyond 64 tiles (whose survivor mask has to be shifted), a last tile row that is only partly on the image, both the speculative
    one-call forward and the two-stage form -- and the same images, radii and gradients as the plain launch."""
    s = S.scene_config1(seed=91, P=6000, W=200, H=150, lateral=0.5)   # 13 x 10 tiles, bottom row 6 px high
    s["scales"][:300] *= np.float32(8.0)                              # some splats cover > 64 tiles
    grads = S.upstream_grads(2, s["W"], s["H"])
    st = Hh.oracle_forward(s)
    counts = (st["ranges"][:, 1] - st["ranges"][:, 0]).astype(np.int64)
    try:
        set_tuning(tile_cull=False)
        plain = Hh.hip_run(s, grads)
        for speculative in (False, True):
            set_tuning(tile_cull=False, scatter_bands=bands, speculative=speculative)   # (clears the capacity hint)
            for _rep in range(2 if speculative else 1):   # the second speculative call has a hint: the one-call form
                got = Hh.hip_run(s, keep_state=True)
                assert got["num_rendered"] == st["num_rendered"]
                _check_binning(s, got, st["point_list"], counts)
        banded = Hh.hip_run(s, grads)
        for k in ("out_color", "out_depth", "out_unc", "radii"):
            assert np.array_equal(banded[k], plain[k]), k
        for k in Hh.GRAD_KEYS:
            assert np.array_equal(banded[k], plain[k]), k   # the lists are the same lists: bit-identical gradients
        set_tuning(scatter_bands=bands)               # and with tile culling (the survivor masks now have holes)
        culled = Hh.hip_run(s, grads)
        set_tuning()
        ref = Hh.hip_run(s, grads)
        for k in ("out_color", "out_depth", "out_unc", "radii") + tuple(Hh.GRAD_KEYS):
            assert np.array_equal(culled[k], ref[k]), k
    finally:
        set_tuning()


def _tile_scan_words(s, one_call, bands, tile_cull=False, occlusion_cut=False):
    """One forward in the two-stage form (gsr_tile_scan_kernel writes the frame's tile-scan words) or the one-call form (workgroup 0
    of the scatter does): the binning state and the words both forms must agree on."""
    from gscream_amd import rasterizer as RZ
    set_tuning(tile_cull=tile_cull, scatter_bands=bands, speculative=one_call, occlusion_cut=occlusion_cut)   # (clears the capacity hint)
    for _rep in range(2 if one_call else 1):   # the second speculative call has a hint: the one-call form
        got = Hh.hip_run(s, keep_state=True)
    assert bool(RZ._last_stage1["speculative"]) == one_call
    img = _layout.image_views(got["img"], s["means3D"].shape[0], s["W"], s["H"])
    words = dict(num_rendered=got["num_rendered"], max_tile_count=RZ._last_stage1["max_tile_count"], num_occluded=RZ._last_stage1["num_occluded"])
    words.update({k: img[k].cpu().numpy().copy() for k in ("ranges", "sorted_len", "need_full")})
    return got, words


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,tiles", [(640, 480, 1200), (1296, 1040, 5265), (2064, 1600, 12900)])
def test_both_tile_scans_write_the_same_words(W, H, tiles):
    """The tile-scan words of a frame -- ranges, sorted_len, need_full, R, the longest list, the occluded count -- have two producers:
    gsr_tile_scan_kernel<PER> (two-stage forward) and workgroup 0 of the scatter (one-call forward).  Both must match the oracle and
    each other at every PER class of the kernel: 1200 tiles = two per thread (class 4), 81 x 65 = 5265 (class 12; the odd row width
    keeps band edges off the 64-tile group edges the banded scatter starts its scan from), 129 x 100 = 12900 (class 36) -- with the
    plain and the banded scatter.  These runs have tile culling off (the oracle's lists).  The occlusion part needs it ON: the library
    switches the cut-off off when tile culling is disabled (api.hip gsr_occlusion), so with it off there is no dropped count to sum."""
    assert ((W + 15) // 16) * ((H + 15) // 16) == tiles
    s = S.scene_config1(seed=78, P=3000, W=W, H=H)
    s["scales"] = (s["scales"] * np.float32(0.5)).astype(np.float32)   # spread over the frame, splats of several tiles
    st = Hh.oracle_forward(s, nthreads=NT)
    counts = (st["ranges"][:, 1] - st["ranges"][:, 0]).astype(np.int64)
    try:
        for bands in (0, 3):
            forms = {}
            for one_call in (False, True):
                got, forms[one_call] = _tile_scan_words(s, one_call, bands)
                assert got["num_rendered"] == st["num_rendered"]
                _check_binning(s, got, st["point_list"], counts)
            assert forms[False]["max_tile_count"] == int(counts.max())
            for k, v in forms[False].items():
                assert np.array_equal(v, forms[True][k]), (bands, k)
        if tiles == 1200:   # + the sum of the occlusion cut-off's dropped instances (it needs the tile culling): big opaque splats among small ones
            s["scales"][:500] *= np.float32(10.0)
            s["opacities"][:500] = np.float32(0.9)
            for bands in (0, 3):
                off = _tile_scan_words(s, False, bands, tile_cull=True)[1]
                forms = {one_call: _tile_scan_words(s, one_call, bands, tile_cull=True, occlusion_cut=True)[1] for one_call in (False, True)}
                for k, v in forms[False].items():
                    assert np.array_equal(v, forms[True][k]), (bands, k)
                assert off["num_occluded"] == 0 and forms[True]["num_occluded"] > 0
                assert forms[True]["num_rendered"] + forms[True]["num_occluded"] == off["num_rendered"]
    finally:
        set_tuning()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["stack_of_big_splats", "mixed", "bench_like", "walks_into_the_second_tier"])
def test_occlusion_cutoff_changes_no_output_bit(case):
    """gsr_tuning.occlusion_cut: instances behind the depth bucket at which a tile's whole-tile alphas already put every pixel's
    transmittance below 1e-4 are never binned.  Conservative by construction (DGR forward.cu:537 stops those pixels before them):
    images, radii, final T, contributor counts, traversal depths and every gradient must be BIT-identical with the pass on and
    off; only num_rendered and the lists shrink.  The kept lists must be an order-preserving subset of the full ones."""
    import torch
    from gscream_amd import rasterizer as RZ
    if case == "stack_of_big_splats":      # lists of thousands, saturated after a few dozen: most of every list goes
        s = S.scene_config1(seed=33, P=14_000, W=32, H=32, lateral=0.3)
        s["scales"] *= np.float32(6.0)
        s["opacities"] = np.maximum(s["opacities"], np.float32(0.6))
    elif case == "walks_into_the_second_tier":
        # case 5049 of tools/fuzz_parity.py (round 5): huge faint-ish splats, walks that go past list position 448 AND a cut-off that
        # shortens the lists -- with second-tier boundaries chosen from the list length the images moved in the last bit
        rng = np.random.default_rng(5049)
        rng.choice([1, 7, 64, 65, 300, 1500, 4000, 12000]); rng.integers(17, 700); rng.integers(17, 500)   # (the sweep's draws before the camera)
        s = S.scene_config1(seed=5049, P=12000, W=84, H=378)
        s["scales"] = (s["scales"] * np.float32(6.0)).astype(np.float32)
        s["viewmatrix"], s["projmatrix"], s["campos"] = S.camera_matrices(s["tanfovx"], s["tanfovy"], S.random_w2c(rng))
    elif case == "mixed":                  # big opaque splats in front of / between many small ones, partial last tile row
        s = S.scene_config1(seed=92, P=9000, W=200, H=150, lateral=0.5)
        s["scales"][:1500] *= np.float32(10.0)
        s["opacities"][:1500] = np.float32(0.9)
    else:                                  # small splats: nothing covers a tile, nothing may be dropped
        s = S.scene_slab(7, 40_000, 504, 284)
    grads = S.upstream_grads(3, s["W"], s["H"])
    P, W, H = s["means3D"].shape[0], s["W"], s["H"]
    out = {}
    try:
        for on in (False, True):
            set_tuning(occlusion_cut=on)
            st = Hh.hip_run(s, keep_state=True)
            img = _layout.image_views(st["img"], P, W, H)
            rng = img["ranges"].cpu().numpy().astype(np.int64)
            pl = _layout.binning_views(st["binning"], st["num_rendered"], st["binning_capacity"])["point_list"].cpu().numpy().astype(np.int64)
            out[on] = dict(R=st["num_rendered"], occluded=RZ._last_stage1["num_occluded"], rng=rng, pl=pl,
                           final_T=img["final_T"].cpu().numpy(), n_contrib=img["n_contrib"].cpu().numpy(), tile_work=img["tile_work"].cpu().numpy(),
                           radii=st["radii"], color=st["out_color"], depth=st["out_depth"], unc=st["out_unc"], g=Hh.hip_run(s, grads))
    finally:
        set_tuning()
    off, on = out[False], out[True]
    assert off["occluded"] == 0 and on["R"] + on["occluded"] == off["R"]
    if case == "bench_like":
        assert on["occluded"] <= 0.01 * off["R"]
    else:
        assert on["occluded"] > (0.5 if case == "stack_of_big_splats" else 0.0 if case == "walks_into_the_second_tier" else 0.1) * off["R"], (on["occluded"], off["R"])
    if case == "walks_into_the_second_tier":
        assert (off["n_contrib"].astype(np.int64) & 0x3fffffff).max() > 7 * 64, "some walk must pass the first tier of depth segments"
    for k in ("final_T", "n_contrib", "tile_work", "radii", "color", "depth", "unc"):
        assert np.array_equal(on[k], off[k]), k
    for k in Hh.GRAD_KEYS:
        assert np.array_equal(on["g"][k], off["g"][k]), k
    for t in range(off["rng"].shape[0]):   # every tile: the kept list is the FRONT of the full one (the cut-off is a depth)
        a, b = off["pl"][off["rng"][t, 0]:off["rng"][t, 1]], on["pl"][on["rng"][t, 0]:on["rng"][t, 1]]
        keep = np.isin(a, b)
        if len(a) <= 2048:   # (a longer list is in depth order only as far as the blend walks it, binning.hip: the sets are compared, not the order)
            assert np.array_equal(a[keep], b), f"tile {t}: not an order-preserving subset"
        else:
            assert np.array_equal(np.sort(a[keep]), np.sort(b)), f"tile {t}: not a subset"
        assert len(b) >= int(off["tile_work"][t]), f"tile {t}: the cut-off removed an instance the forward walks"


def _faint_splats_scene():
    """Scene, upstream gradients and oracle forward of a frame of faint splats: nothing saturates, every list is walked to its end.
    Scene and gradients are the caller's own; the oracle's result is computed once and shared, read-only."""
    s = S.scene_config1(seed=91, P=6000, W=64, H=48, lateral=0.35)
    s["opacities"] = (s["opacities"] * 0.02 + 0.004).astype(np.float32)       # 0.005 .. 0.023: T stays near 1 over thousands of blends
    s["scales"] = (s["scales"] * 2.0).astype(np.float32)
    if not _faint_splats_oracle:
        _faint_splats_oracle.append(Hh.oracle_forward(s))
    return s, S.upstream_grads(91, s["W"], s["H"]), _faint_splats_oracle[0]


_faint_splats_oracle = []


def test_second_tier_of_depth_segments():
    """Round 5: lists longer than seven tier-1 segments are cut into GSR_SEG2 more segments at fixed list positions
    (gsr_common.h gsr_ckpt_pos) instead of leaving everything behind position 448 to ONE backward task.  A frame of
    faint splats -- nothing saturates, every list is walked to its end, like an initialised, untrained scene -- with lists well
    beyond 448 entries: images and gradients against the oracle, the checkpoints a pixel wrote sit where the two-tier rule puts them
    (the sums of the closed segments + the open one reproduce the image), and the backward stays bit-reproducible."""
    s, grads, st = _faint_splats_scene()
    ref = Hh.oracle_backward(s, st, grads)
    ll = (st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0])
    assert ll.max() > 7 * 64 + 8 * 64, f"the scene must reach the second tier (longest list {ll.max()})"
    assert (st["n_contrib"] > 7 * 64).mean() > 0.5, "most pixels must walk into the second tier"
    got = Hh.hip_run(s, grads)
    assert (got["radii"] == st["radii"]).all()
    Hh.assert_parity_strict(got, st, ref, s, grads, context="second tier", nthreads=NT)
    again = Hh.hip_run(s, grads)
    for k in Hh.GRAD_KEYS:
        if k in got:
            assert np.array_equal(got[k], again[k]), f"{k}: the backward is bit-reproducible with second-tier tasks"
    # the checkpoints
    keep = Hh.hip_run(s, None, keep_state=True)
    P, W, H = s["means3D"].shape[0], s["W"], s["H"]
    iv = _layout.image_views(keep["img"], P, W, H)
    N, Np, SM = W * H, (W * H + 3) & ~3, _layout.SEG_MAX
    a = iv["ckpt"][:, :4 * Np].reshape(SM, Np, 4)[:, :N]
    npass = a[SM - 1, :, 0].view(torch.int32).long().cpu().numpy().reshape(H, W)
    assert npass.max() > _layout.SEG1, "some pixel passed a second-tier checkpoint"
    ranges = iv["ranges"].cpu().numpy().astype(np.int64)
    ncon = (iv["n_contrib"].cpu().numpy().astype(np.int64) & 0x3fffffff).reshape(H, W)
    gx = (W + 15) // 16
    for y in range(0, H, 5):
        for x in range(0, W, 7):
            t = (y // 16) * gx + x // 16
            n = int(ranges[t, 1] - ranges[t, 0])
            # a pixel passes checkpoint k iff its QUADRANT's walk reached that list position: at least every checkpoint in front
            # of its own last contributor
            must = sum(1 for k in range(SM - 1) if _layout.ckpt_pos(k, 64) < ncon[y, x])
            assert npass[y, x] >= must, (x, y, n, int(ncon[y, x]), int(npass[y, x]))
    k = torch.arange(SM - 1, device="cuda")[:, None]
    live = k < a[SM - 1, :, 0].view(torch.int32).long()[None, :]
    sums = torch.where(live[:, :, None], a[:SM - 1, :, 1:], torch.zeros_like(a[:SM - 1, :, 1:])).sum(0) + a[SM - 1, :, 1:]
    fT = iv["final_T"].reshape(-1)
    bg = torch.from_numpy(s["bg"]).cuda()
    img = sums.t().reshape(3, H, W) + fT.reshape(1, H, W) * bg[:, None, None]
    assert (img.cpu().numpy() - keep["out_color"]).max() < 1e-5


def _guard_band_pairs(s, st, width):
    """(pixel x, pixel y, Gaussian) of the blending pairs whose reference alpha o exp(power) lies within `width` / 255 of 1 / 255
    (float64 on the oracle's means2D / conic_opacity, over the oracle's own tile lists) + the number of blending pairs."""
    W, H = s["W"], s["H"]
    gx = (W + 15) // 16
    m2, co = st["means2D"].astype(np.float64), st["conic_opacity"].astype(np.float64)
    pairs, blending = [], 0
    for t, (a, b) in enumerate(st["ranges"].astype(np.int64)):
        g = st["point_list"][a:b].astype(np.int64)
        ys, xs = np.meshgrid(np.arange((t // gx) * 16, min((t // gx) * 16 + 16, H)), np.arange((t % gx) * 16, min((t % gx) * 16 + 16, W)), indexing="ij")
        xs, ys = xs.reshape(-1), ys.reshape(-1)
        dx, dy = m2[g, 0][:, None] - xs[None, :], m2[g, 1][:, None] - ys[None, :]
        power = -0.5 * (co[g, 0][:, None] * dx * dx + co[g, 2][:, None] * dy * dy) - co[g, 1][:, None] * dx * dy
        alpha = co[g, 3][:, None] * np.exp(np.minimum(power, 0.0))
        blending += int(((power <= 0) & (alpha >= 1.0 / 255.0)).sum())
        gi, pi = np.nonzero((power <= 0) & (np.abs(alpha - 1.0 / 255.0) < width / 255.0))
        pairs += [(int(xs[p_]), int(ys[p_]), int(g[g_])) for g_, p_ in zip(gi, pi)]
    return pairs, blending


def test_guard_band_entries_are_flagged_and_settled_alike():
    """The alpha = 1/255 guard band (blend.hip GSR_BAND, gsr_band_settle).  On the frame of faint splats nothing saturates, so every
    binned pair is walked: every (pixel, Gaussian) pair whose reference alpha lies in the inner half of the band -- 1.5e-5 relative, far
    more than the few 1e-7 by which the fast alpha differs -- must leave bit 31 set on that Gaussian's entry of the pixel's tile list
    (lists sorted once: partial_sort off, so the flags survive), and the backward, which settles the flagged entries only, must give
    the same bits as the one that settles every entry: flag-driven check = check everything.  The backward settles every entry of a
    tile whose list was sorted a second time (need_full: the flags of its first pass are lost), i.e. of a list beyond 2048 entries that
    lost the partial sort's bet.  With the default tuning tile culling may leave no such list on this scene, so the comparison is made
    a second time on the oracle's lists (tile_cull off), where a tile that holds an in-band pair must have been sorted twice."""
    s, grads, st = _faint_splats_scene()
    pairs, blending = _guard_band_pairs(s, st, 1.5e-5)
    print(f"guard band: {len(pairs)} pairs in its inner half of {blending} blending pairs")
    assert len(pairs) >= 4, "the scene must put some pairs inside the guard band"
    P, W, H = s["means3D"].shape[0], s["W"], s["H"]
    tile_of = lambda x, y: (y // 16) * ((W + 15) // 16) + x // 16
    try:
        for cull in (True, False):
            set_tuning(tile_cull=cull, partial_sort=False)
            keep = Hh.hip_run(s, keep_state=True)
            rng = _layout.image_views(keep["img"], P, W, H)["ranges"].cpu().numpy().astype(np.int64)
            bv = _layout.binning_views(keep["binning"], keep["num_rendered"], keep["binning_capacity"])
            pl, flag = bv["point_list"].cpu().numpy().astype(np.int64), bv["band_flag"].cpu().numpy()
            for x, y, g in pairs:
                a, b = rng[tile_of(x, y)]
                at = np.flatnonzero(pl[a:b] == g)
                assert at.size == 1, f"Gaussian {g} must be in the list of pixel ({x}, {y})'s tile"
                assert flag[a + at[0]], f"pixel ({x}, {y}) met Gaussian {g} inside the guard band: its list entry must carry bit 31"
            flagged_only = Hh.hip_run(s, grads)
            set_tuning(tile_cull=cull)                           # (set_tuning resets the partial sort's feedback: this forward bets)
            need_full = _layout.image_views(Hh.hip_run(s, keep_state=True)["img"], P, W, H)["need_full"].cpu().numpy().astype(bool)
            print(f"tile_cull={cull}: {int(need_full.sum())} tiles sorted twice, in-band pairs in {sum(bool(need_full[tile_of(x, y)]) for x, y, _ in pairs)} of them")
            if not cull:
                assert any(need_full[tile_of(x, y)] for x, y, _ in pairs), "a tile with an in-band pair must lose the partial sort's bet"
            set_tuning(tile_cull=cull)
            every_entry = Hh.hip_run(s, grads)
            for k in Hh.GRAD_KEYS:
                if k in flagged_only:
                    assert np.array_equal(flagged_only[k], every_entry[k]), f"{k} (tile_cull={cull}): settling the flagged entries = settling every entry"
    finally:
        set_tuning()


def test_init_state_frame_against_the_oracle():
    """The frame GScream renders at iteration 0 (synthetic.scene_init_state: a surface point cloud through create_from_pcd restated and
    the fused decode), at a size the oracle does in seconds: faint splats (half of the pixels end their walk near T = 1e-4 after
    500 - 2800 instances: second tier of depth segments, partially sorted lists, the stop replay), five to ten COINCIDENT Gaussians per anchor (zero offsets: equal depth keys, order by id, SURVEY A-9),
    anchor scales up to tens of pixels next to pin-point ones.  Element-wise against the oracle with the full-size gate: a pixel may
    exceed 1e-4 only on an expf tie of the oracle's own walk, a gradient element 1e-3 only inside the reference's order-noise range or
    in the walk of such a pixel."""
    W, H = 336, 189
    s = S.scene_init_state(7, W, H, n_points=12_000)
    assert 30_000 < s["means3D"].shape[0] < 90_000
    grads = S.upstream_grads(7, W, H, True, True, False)
    nt = min(8, os.cpu_count() or 1)
    st = Hh.oracle_forward(s, nthreads=nt)
    ref = Hh.oracle_backward(s, st, grads, nthreads=nt)
    ll = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    assert ll.max() > 2048 and (st["n_contrib"] > 7 * 64).mean() > 0.3, "long lists (partial sort) and walks deep into the second tier of depth segments"
    dk = st["depths"][st["radii"] > 0]
    assert np.unique(dk).size < 0.6 * dk.size, "coincident Gaussians: many equal depth keys"
    got = Hh.hip_run(s, grads)
    assert (got["radii"] == st["radii"]).all()
    rep = Hh.parity_report(got, st, ref, nthreads=nt, s=s, grads=grads)
    ties = sum(1 for p_ in rep["outlier_pixels"] if p_["expf_tie"])
    assert rep["px_gt_1e-4"] <= ties <= 2, rep["outlier_pixels"]
    assert rep["last_contributor_differs"]["pixels"] <= ties + rep["last_contributor_differs"]["expf_tie_at_the_T_stop"], rep["last_contributor_differs"]
    env = rep.get("order_noise_envelope")
    assert env is None or env["elements_outside_not_in_an_expf_tie_walk"] == 0, [e for e in env["elements"] if not e["inside_envelope"] and not e["in_expf_tie_walk"]]
    assert rep["grad_elems_gt_1e-3"] <= 16 + 64 * ties
    # the replay's band assumes the fast T chain stays within GSR_TBAND = 1e-4 (relative) of the reference chain's; the error
    # accumulates per blend, and these are the deepest walks any test has (500 - 2800 instances per pixel)
    print(f"init-state frame: fast-walk final T vs the oracle's chain, max relative difference where both stop at the same Gaussian: "
          f"{rep['final_T_max_rel_where_same_stop']:.2e} (band 1e-4)")
    assert ties or rep["final_T_max_rel_where_same_stop"] < 1e-4, rep["final_T_max_rel_where_same_stop"]


def test_view_cache_orders_the_forward_and_changes_nothing():
    """Round 5: per-view walk depths (gsr_tuning.walk_depths, rasterizer._walk_depths).  The second visit of a view dispatches the
    forward's quadrant tasks deepest-first from what the first visit recorded; images, radii, gradients and the state the backward reads
    are bit-identical to a forward without the cache, whatever the array holds (a scribbled one included); the dispatch order is a
    permutation of every XCD's task slots; the recorded depths are the walks."""
    import torch
    from gscream_amd import rasterizer as RZ, _layout
    s = S.scene_config1(seed=23, P=30000, W=400, H=208)      # 25 x 13 = 325 tiles
    grads = S.upstream_grads(23, s["W"], s["H"])
    P, W, H = s["means3D"].shape[0], s["W"], s["H"]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    try:
        RZ.set_tuning(view_cache=False, occlusion_cut=False)   # (the automatic cut-off would shorten the lists between two visits)
        base = Hh.hip_run(s, grads)
        RZ.set_tuning(view_cache=True, occlusion_cut=False)
        rs = Hh.hip_settings(s)
        first = Hh.hip_run(s, grads, rs=rs)                  # records
        cache = RZ._view_cache_tls.cache
        assert len(cache) == 1
        walk = next(iter(cache.values()))[1]  # (entry = (weak reference to the view matrix, depths))
        assert walk.shape == (4 * T,) and walk.dtype == torch.int32
        recorded = walk.clone()
        second = Hh.hip_run(s, grads, rs=rs)                 # orders by the recorded depths
        assert len(cache) == 1 and next(iter(cache.values()))[1] is walk
        diff = (walk != recorded).nonzero().flatten().cpu().numpy()
        assert len(diff) == 0, ("the same view walks the same depths", len(diff), diff[:8], walk[diff[:8]].cpu().numpy(), recorded[diff[:8]].cpu().numpy())
        keep = Hh.hip_run(s, None, keep_state=True, rs=rs)
        iv = _layout.image_views(keep["img"], P, W, H)
        xt = _layout.xcd_tiles(T)
        order = iv["qorder"].cpu().numpy()
        assert order.shape == (8, 4 * xt)
        for x in range(8):
            assert np.array_equal(np.sort(order[x]), np.arange(4 * xt)), f"XCD {x}: the dispatch order is a permutation of its task slots"
            d = np.array([int(recorded[4 * _layout.xcd_tile(x, i >> 2, T) + (i & 3)]) >> 3 if _layout.xcd_tile(x, i >> 2, T) >= 0 else -1
                          for i in order[x]])
            assert (np.diff(np.minimum(d, 255)) <= 0).all(), f"XCD {x}: deepest recorded walks first, slots without a tile last"
        # the recorded depth of a quadrant covers its deepest contributor (and is a multiple of the 64-instance batch or the list end)
        ncon = (iv["n_contrib"].cpu().numpy().astype(np.int64) & 0x3fffffff).reshape(H, W)
        rec = recorded.cpu().numpy().astype(np.int64)
        gx = (W + 15) // 16
        for t in range(0, T, 7):
            for q in range(4):
                y0, x0 = (t // gx) * 16 + (q >> 1) * 8, (t % gx) * 16 + (q & 1) * 8
                if y0 < H and x0 < W:
                    assert rec[4 * t + q] >= ncon[y0:y0 + 8, x0:x0 + 8].max(), (t, q)
        walk.random_(0, 1 << 30)                             # garbage in the array: still the same frame
        third = Hh.hip_run(s, grads, rs=rs)
        # the two-stage form (no speculation): the ordering is a launch of its own in front of the blend instead of eight workgroups
        # of the column scan
        RZ.set_tuning(view_cache=True, occlusion_cut=False, speculative=False)
        rs2 = Hh.hip_settings(s)
        Hh.hip_run(s, grads, rs=rs2)
        fourth = Hh.hip_run(s, grads, rs=rs2)
        keep2 = Hh.hip_run(s, None, keep_state=True, rs=rs2)
        order2 = _layout.image_views(keep2["img"], P, W, H)["qorder"].cpu().numpy()
        assert np.array_equal(np.sort(order2, axis=1), np.tile(np.arange(4 * xt), (8, 1))) and not np.array_equal(order2, np.tile(np.arange(4 * xt), (8, 1)))
        for other, what in ((first, "recording visit"), (second, "ordered visit"), (third, "scribbled depths"), (fourth, "two-stage form")):
            for k in ("out_color", "out_depth", "out_unc", "radii", "final_T") + tuple(Hh.GRAD_KEYS):
                if k in base:
                    assert np.array_equal(base[k], other[k]), f"{what}: {k} differs from the forward without the view cache"
    finally:
        RZ.set_tuning()


def test_backward_with_a_too_small_longest_list_hint_still_traverses_everything():
    """gsr_backward's `max_tile_count` sizes the grid of depth-segment tasks (round 6: as many segment ranks as the longest list has).
    A binding that passes a figure SMALLER than the forward's must not lose gradients: the grid's last segment takes whatever is left of a
    list (one longer task; the pixels start it from their final state like the reference, backward.cu:500-520)."""
    from gscream_amd import GaussianRasterizer
    s = S.scene_config1(seed=91, P=6000, W=64, H=48, lateral=0.35)
    s["opacities"] = (s["opacities"] * 0.02 + 0.004).astype(np.float32)
    s["scales"] = (s["scales"] * 2.0).astype(np.float32)
    grads = S.upstream_grads(91, s["W"], s["H"])
    ref = Hh.hip_run(s, grads)
    t = lambda a, rg=False: torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(rg)
    leaves = {k: t(s[k], True) for k in ("means3D", "opacities", "uncertainties", "colors", "scales", "rotations")}
    m2d = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, depth, unc, _radii = GaussianRasterizer(raster_settings=Hh.hip_settings(s))(
        means3D=leaves["means3D"], means2D=m2d, opacities=leaves["opacities"], uncertainties=leaves["uncertainties"],
        colors_precomp=leaves["colors"], scales=leaves["scales"], rotations=leaves["rotations"])
    assert int(color.grad_fn.max_tile_count) > 7 * 64 + 8 * 64
    color.grad_fn.max_tile_count = 100  # a stale / wrong hint: far below the longest list
    gc, gd, gu = (torch.from_numpy(g).cuda() for g in grads)
    ((color * gc).sum() + (depth * gd).sum() + (unc * gu).sum()).backward()
    for name, key in (("means3D", "dL_dmeans3D"), ("opacities", "dL_dopacity"), ("colors", "dL_dcolors"), ("scales", "dL_dscales"), ("rotations", "dL_drotations")):
        g = leaves[name].grad.cpu().numpy()
        scale = np.abs(ref[key]).max()
        assert np.abs(g - ref[key]).max() <= 2e-4 * scale, (name, float(np.abs(g - ref[key]).max()), float(scale))
        assert np.abs(g).max() > 0
