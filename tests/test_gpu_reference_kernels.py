"""The reference's OWN rasterizer kernels (oracle/_ref/libgsref.so: its three .cu files compiled unedited for gfx950 behind
stand-in CUDA headers, oracle/ref_cuda/) against the CPU oracle, and the HIP library against those kernels.

Every other rasterizer gate of the suite compares the library with oracle/gs_oracle.c, our restatement of those files; a
misreading shared by the restatement and the kernels (a glm product in the other order, another tie rule of the sort, a wrong
term in the depth or uncertainty backward) would pass them all.  Here the restatement meets the text it restates:
  * per-Gaussian stage: integers equal, floats equal as bits (both sides are IEEE fp32 without contraction, correctly rounded
    divide and sqrt: equality is the expected bar, not a measured one);
  * binning: num_rendered, tile ranges and every tile's list equal (`ties`: equal key -> ascending index);
  * blend and backward: helpers.assert_parity_strict, BASELINE's bars, applied to the thing they were defined against; the
    reference sums with real unordered atomicAdd, which is what the order-noise envelope claims to model;
  * library vs reference kernels: radii, lists, filters, markVisible equal; images within 2e-4 (two 1e-4 bars).
What this does not pin: CUDA's own libm and nvcc's FMA contraction (this build uses ocml and -ffp-contract=off).

The library is built by `make -C oracle ref` (build() does it when the reference checkout is present); without it these
tests skip.  Nothing here is larger than 3000 Gaussians or 320x256."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers as Hh  # noqa: E402
from golden import make_golden as MG  # noqa: E402
from gscream_amd import GaussianRasterizer, _layout, set_tuning  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import ref_cuda as RC  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not RC.available(), reason="oracle/_ref/libgsref.so is not built (make -C oracle ref needs the reference checkout)")]

GOLDEN = ("cfg1", "stack", "odd_size", "moved_cam", "cov_precomp", "clamp", "sh_deg3", "ties", "white_bg", "rgb_only", "all_culled")
SCENES = GOLDEN + Hh.VARIANTS + ("gscream_call",)
NT = max(1, min(16, os.cpu_count() or 1))
ALL_KEYS = Hh.STRICT_KEYS + ("dL_dconic", "dL_ddepths")


@pytest.fixture(autouse=True)
def _default_tuning():
    set_tuning()
    yield
    set_tuning()


def _scene(name):
    if name in GOLDEN:
        s, grads, _ = MG.load(name)
        return s, grads
    if name in Hh.VARIANTS:
        return Hh.variant_scene(name)
    # GScream's own call form (gaussian_renderer/__init__.py): precomputed colours, scales + rotations, a loss on the image and
    # on the depth map, none on the uncertainty map
    s = S.scene_config1(seed=95, P=2000, W=126, H=71, lateral=0.7, w2c=S.random_w2c(np.random.default_rng(95)), cx=0.02, cy=-0.03)
    return s, S.upstream_grads(96, s["W"], s["H"], True, True, False)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Scene, oracle forward + backward, reference-kernel forward + backward: computed once per scene, shared, never written."""
    s, grads = _scene(name)
    st = Hh.oracle_forward(s, nthreads=NT)
    ob = Hh.oracle_backward(s, st, grads, nthreads=NT)
    rf = RC.forward(s)
    rb = RC.backward(s, rf, grads)
    for d in (s, st, ob, rf, rb):   # (a state's `colors` / `cov3D` may be the scene's own array)
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return s, grads, st, ob, rf, rb


def _ulps(a, b):
    """Distance in units of the last place between two fp32 arrays (ordered-integer trick; +0 and -0 are 0 apart)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def _as_got(s, rf, rb=None):
    """A reference-kernel run in the shape helpers.hip_run returns: images, final_T, the Gaussian every pixel blended last (from
    the reference's own n_contrib and lists) and the gradient families."""
    got = {k: rf[k] for k in ("out_color", "out_depth", "out_unc", "radii", "final_T")}
    got["last_gid"] = Hh.last_gaussian(rf["ranges"], rf["point_list"], rf["n_contrib"], s["W"], s["H"])
    if rb is not None:
        got.update(rb)   # (with SH input dL_dcolors is an intermediate; the oracle returns the same one and it is compared like the rest)
    return got


@pytest.mark.parametrize("name", SCENES)
def test_per_gaussian_stage_is_bit_equal_to_the_oracle(name):
    s, _, st, _, rf, _ = _case(name)
    assert np.array_equal(rf["radii"], st["radii"]), "radii"
    assert np.array_equal(rf["tiles_touched"], st["tiles_touched"]), "tiles_touched"
    assert np.array_equal(rf["clamped"].astype(bool), st["clamped"].astype(bool)), "clamped"
    worst = {}
    for k in ("means2D", "depths", "cov3D", "conic_opacity", "colors", "unc"):
        a, b = np.ascontiguousarray(rf[k], np.float32), np.ascontiguousarray(st[k], np.float32).reshape(rf[k].shape)
        u = _ulps(a, b)
        worst[k] = int(u.max()) if u.size else 0
        if worst[k]:
            print(f"[ulp] {name}/{k}: max {worst[k]} ulp, {int((u > 0).sum())} of {u.size} elements differ")
    print(f"[refkernels] {name}: per-Gaussian stage max ulp {worst}, visible {int((st['radii'] > 0).sum())} of {st['radii'].size}")
    for k in worst:
        a, b = np.ascontiguousarray(rf[k], np.float32), np.ascontiguousarray(st[k], np.float32).reshape(rf[k].shape)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{k}: bits differ (max {worst[k]} ulp)"
    if name == "all_culled":
        assert not (st["radii"] > 0).any()
    if name.startswith("sh_deg"):
        assert (st["radii"] > 0).sum() > 100 and "shs" in s
    if name == "sh_deg3":
        assert st["clamped"][st["radii"] > 0].any(), "the colour clamp is reached"


@pytest.mark.parametrize("name", SCENES)
def test_binning_is_equal_to_the_oracle(name):
    s, _, st, _, rf, _ = _case(name)
    assert rf["num_rendered"] == st["num_rendered"]
    assert np.array_equal(rf["point_offsets"].astype(np.int64), np.cumsum(st["tiles_touched"].astype(np.int64))), "inclusive scan"
    # the reference leaves ranges of empty tiles at their zero fill, and so does the oracle
    assert np.array_equal(rf["ranges"], st["ranges"]), "tile ranges"
    assert np.array_equal(rf["point_list"], st["point_list"]), "sorted per-tile lists"
    assert np.array_equal(rf["point_keys"], st["point_keys"]), "sorted keys"
    if name == "ties":
        keys, ids = rf["point_keys"], rf["point_list"].astype(np.int64)
        same = keys[1:] == keys[:-1]
        assert same.sum() > 50, "the scene holds equal (tile, depth) keys"
        assert (ids[1:][same] > ids[:-1][same]).all(), "equal key -> ascending Gaussian index (stable sort of index-ordered input)"
    if name == "stack":
        counts = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
        assert counts.max() > 256, "more than one 256-instance batch in a tile"
    if name == "huge_gaussians":
        assert st["tiles_touched"].max() > 64
    print(f"[refkernels] {name}: binning equal, R = {st['num_rendered']}")


def _gate(name, s, grads, st, ob, rf, rb):
    got = _as_got(s, rf, rb)
    rep = Hh.assert_parity_strict(got, st, ob, s, grads, context=f"reference kernels/{name}", keys=ALL_KEYS, nthreads=NT)
    env = rep.get("order_noise_envelope", {})
    print(f"[refkernels] {name}: reference vs oracle: image max abs {rep['max_abs']:.3e}, pixels > 1e-4: {rep['px_gt_1e-4']} {rep['px_by_cause']}, "
          f"walks differing {rep['last_contributor_differs']}, T drift {rep['final_T_max_rel_where_same_stop']:.2e}, "
          f"gradient worst rel {rep.get('worst_rel', 0.0):.3e}, elements > 1e-3: {rep.get('grad_elems_gt_1e-3', 0)} "
          f"(inside envelope {env.get('elements_inside', 0)}, outside {env.get('elements_outside', 0)}) "
          f"per family {({k: round(v['max'], 6) for k, v in rep.get('grads', {}).items()})}")
    return rep


@pytest.mark.parametrize("name", SCENES)
def test_blend_and_backward_pass_the_strict_gate_against_the_oracle(name):
    s, grads, st, ob, rf, rb = _case(name)
    _gate(name, s, grads, st, ob, rf, rb)
    if name == "all_culled":
        assert not rf["out_depth"].any() and all(not rb[k].any() for k in rb)
    culled = st["radii"] <= 0
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dcov3D"):
        assert not rb[k][culled].any(), f"{k}: culled Gaussians get exact zeros"
    if name == "stack":
        # unordered atomicAdd: a second run of the same kernels sums in another order; it must pass the same gate
        rf2 = RC.forward(s)
        rb2 = RC.backward(s, rf2, grads)
        for k in ("out_color", "out_depth", "out_unc", "final_T", "n_contrib", "point_list"):
            assert np.array_equal(rf2[k], rf[k]), f"{k}: the forward is deterministic"
        _gate(name + " (second run)", s, grads, st, ob, rf2, rb2)
        moved = {k: float(np.abs(rb2[k].astype(np.float64) - rb[k]).max()) for k in rb if rb[k].size}
        print(f"[refkernels] stack: run-to-run max abs difference of the reference's own gradients {moved}")


@pytest.mark.parametrize("name", SCENES)
def test_library_matches_the_reference_kernels(name):
    s, _, _, _, rf, _ = _case(name)
    s = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in s.items()}   # (torch wants writable arrays)
    P, W, H = s["means3D"].shape[0], s["W"], s["H"]
    set_tuning(tile_cull=False)
    got = Hh.hip_run(s, keep_state=True)
    assert np.array_equal(got["radii"], rf["radii"]), "radii"
    assert got["num_rendered"] == rf["num_rendered"]
    R = got["num_rendered"]
    rng = _layout.image_views(got["img"], P, W, H)["ranges"].cpu().numpy().astype(np.int64)
    ref_counts = rf["ranges"][:, 1].astype(np.int64) - rf["ranges"][:, 0]
    assert np.array_equal(rng[:, 1] - rng[:, 0], ref_counts), "per-tile instance counts"
    pl = _layout.binning_views(got["binning"], R, got["binning_capacity"])["point_list"].cpu().numpy().astype(np.int64)
    # (the library's ranges partition [0, R) in tile order, as the reference's sorted list does: same positions)
    assert np.array_equal(pl, rf["point_list"].astype(np.int64)), "sorted per-tile lists"
    set_tuning()
    dflt = Hh.hip_run(s)
    worst = 0.0
    for run in (got, dflt):
        for k in ("out_color", "out_depth", "out_unc"):
            d = float(np.abs(run[k].astype(np.float64) - rf[k]).max())
            worst = max(worst, d)
            assert d <= 2e-4, f"{k}: {d:.3e} from the reference kernels' image"
    print(f"[refkernels] {name}: library vs reference kernels: radii / lists equal, image max abs {worst:.3e}")


@pytest.mark.parametrize("name", SCENES)
def test_library_filters_match_the_reference_kernels(name):
    s, _, _, _, rf, _ = _case(name)
    s = {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in s.items()}   # (torch wants writable arrays)
    kw = dict(Hh.cam_kwargs(s), scale_modifier=s["scale_modifier"])
    cov = s.get("cov3D_precomp")
    sc, ro = (None, None) if cov is not None else (s["scales"], s["rotations"])
    r_vis = RC.visible_filter(s["means3D"], sc, ro, cov3D_precomp=cov, **kw)
    r_pos, x_ref, y_ref = RC.position2D_filter(s["means3D"], sc, ro, cov3D_precomp=cov, **kw)
    vis_ref = RC.mark_visible(s["means3D"], s["viewmatrix"], s["projmatrix"])
    assert np.array_equal(r_vis, rf["radii"]) and np.array_equal(r_pos, rf["radii"]), "the reference's filters repeat its forward's radii"
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
    r = GaussianRasterizer(raster_settings=Hh.hip_settings(s))
    pair = dict(cov3D_precomp=t(cov)) if cov is not None else dict(scales=t(sc), rotations=t(ro))
    radii, x, y = r.position2D_filter(t(s["means3D"]), **pair)
    assert np.array_equal(radii.cpu().numpy(), r_pos), "position2D_filter radii"
    assert np.array_equal(x.cpu().numpy().view(np.uint32), x_ref.view(np.uint32)), "x bits"
    assert np.array_equal(y.cpu().numpy().view(np.uint32), y_ref.view(np.uint32)), "y bits"
    assert np.array_equal(r.visible_filter(t(s["means3D"]), **pair).cpu().numpy(), r_vis), "visible_filter radii"
    assert np.array_equal(r.markVisible(t(s["means3D"])).cpu().numpy(), vis_ref), "markVisible"
    # ... and the oracle's three restatements of them
    assert np.array_equal(O.visible_filter(s["means3D"], sc, ro, cov3D_precomp=cov, **kw), r_vis)
    ro_, xo, yo = O.position2D_filter(s["means3D"], sc, ro, cov3D_precomp=cov, **kw)
    assert np.array_equal(ro_, r_pos) and np.array_equal(xo.view(np.uint32), x_ref.view(np.uint32)) and np.array_equal(yo.view(np.uint32), y_ref.view(np.uint32))
    assert np.array_equal(O.mark_visible(s["means3D"], s["viewmatrix"]), vis_ref)
