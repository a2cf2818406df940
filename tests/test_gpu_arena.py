"""Every native entry point inside guarded, poisoned device buffers (tests/arena_helpers.py): one case per entry-point family, each
through the public wrapper, so the wrappers' own sizing code -- the gsr_*_bytes and capacity formulas, the `N // 256 + 2` scratch,
the "buffers sized M" outputs -- is what is held to account.

A case runs three times on the same inputs: plain, inside an arena poisoned with 0xA5, inside one poisoned with 0xFF (NaN as a float,
-1 as an integer).  After an arena run every guard byte must still hold the poison (no write outside a buffer), every writable
pointer the library was handed must have been inside an arena body, and every const input must be unchanged; then the three runs
must agree BIT FOR BIT on everything the wrapper documents as defined (rows up to a returned count, a PNG buffer up to each file's
byte count, accumulators in full).  A row the kernel leaves unwritten, or a result that depends on what a workspace held, differs
between the two poisons.  No tolerance appears anywhere: every comparison is equality of bytes.

The rasterizer's adaptive state (gsr_adaptive_reset, the capacity hints, the occlusion state, the view cache) is reset by
set_tuning() before each run, so the three runs take the same path.  Each run prints the number of native calls intercepted and of
guarded buffers; the module prints the totals per family at the end."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arena_helpers as A  # noqa: E402
import helpers as Hh  # noqa: E402
from gscream_amd import set_tuning  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MiB = 1 << 20
TOTALS = {}  # family -> [runs, native calls, guarded buffers, arena bodies]


@pytest.fixture(scope="module", autouse=True)
def _totals():
    yield
    for family, (runs, calls, guarded, bodies) in sorted(TOTALS.items()):
        print(f"\narena totals: {family}: {runs} arena runs, {calls} native calls intercepted, {guarded} guarded writable buffers, {bodies} bodies")


@pytest.fixture(autouse=True)
def _default_tuning():
    set_tuning()
    yield
    set_tuning()


def _host(v):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def three_runs(monkeypatch, family, what, run, mib=256, expect=()):
    """run(arena or None) -> {name: tensor}; plain, 0xA5 and 0xFF; the arena checks, then equality of every byte of every output.
    expect: native functions every arena run must have gone through (the wrapper reached its kernels)."""
    runs = {}
    for name, poison in (("plain", None), ("arena_a5", 0xA5), ("arena_ff", 0xFF)):
        if poison is None:
            out = run(None)
        else:
            with A.guarded(monkeypatch, mib * MiB, poison, DEV) as (arena, proxy):
                out = run(arena)
            calls, guarded, bodies = proxy.stats()
            print(f"arena {family} / {what} / poison 0x{poison:02X}: {calls} native calls intercepted {dict(proxy.calls)}, "
                  f"{guarded} guarded writable buffers, {bodies} bodies, {arena.cursor} of {arena.nbytes} bytes")
            missing = [fn for fn in expect if not proxy.calls.get(fn)]
            assert not missing, f"{what}: the wrapper never called {missing}"
            assert guarded > 0, f"{what}: the proxy saw no writable buffer"
            t = TOTALS.setdefault(family, [0, 0, 0, 0])
            t[0], t[1], t[2], t[3] = t[0] + 1, t[1] + calls, t[2] + guarded, t[3] + bodies
        runs[name] = {k: _host(v) for k, v in out.items()}
    A.assert_same_bits(runs, f"{family} / {what}")
    return runs["plain"]


def dev(a):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(DEV)


# ==== rasterizer ================================================================================================================

def _raster(s, grads=None, rgb_only=False, rs=None):
    """tests/helpers.py hip_run with torch results: forward (+ backward on `grads`; rgb_only: no gradient into depth and feature)."""
    from gscream_amd import GaussianRasterizer
    t = lambda a, rg=False: dev(a).requires_grad_(rg)
    rg = grads is not None
    rs = Hh.hip_settings(s, DEV) if rs is None else rs
    inp = dict(means3D=t(s["means3D"], rg), opacities=t(s["opacities"], rg), uncertainties=t(s["uncertainties"], rg))
    kw = {}
    if "cov3D_precomp" in s:
        kw["cov3D_precomp"] = t(s["cov3D_precomp"], rg)
    else:
        kw["scales"], kw["rotations"] = t(s["scales"], rg), t(s["rotations"], rg)
    if "shs" in s:
        kw["shs"] = t(s["shs"], rg)
    else:
        kw["colors_precomp"] = t(s["colors"], rg)
    means2D = torch.zeros_like(inp["means3D"], requires_grad=True) + 0
    if rg:
        means2D.retain_grad()
    color, depth, unc, radii = GaussianRasterizer(raster_settings=rs)(means2D=means2D, **inp, **kw)
    out = dict(out_color=color, out_depth=depth, out_unc=unc, radii=radii)
    if rg and color.grad_fn is not None:
        gc, gd, gu = (dev(g) for g in grads)
        loss = (color * gc).sum() if rgb_only else (color * gc).sum() + (depth * gd).sum() + (unc * gu).sum()
        loss.backward()
        out["dL_dmeans2D"] = means2D.grad
        out.update({"dL_d" + k: v.grad for k, v in {**inp, **kw}.items()})
    return out


def _raster_scene(name):
    """-> (scene, upstream gradients, tuning)"""
    from tests import test_gpu_gauss_bwd as GB
    from golden import make_golden as MG
    if name in GB.SCENES:
        s = GB.SCENES[name][0]()
        return s, S.upstream_grads(90, s["W"], s["H"]), {}
    if name in ("odd_size", "cov_precomp"):
        s, grads, _ = MG.load(name)
        return s, grads, {}
    if name == "sh_deg2":
        return Hh.variant_scene("sh_deg2") + ({},)
    P, W, H = {"long_14000": (14_000, 32, 32), "long_40000": (40_000, 32, 16)}[name]
    s = S.scene_config1(seed=31, P=P, W=W, H=H, lateral=0.3)
    s["scales"] *= 0.15
    return s, S.upstream_grads(9, W, H), dict(tile_cull=False, partial_sort=False)


RASTER_SCENES = ["equal_splats", "mixed_splats", "wall", "huge_gaussians", "tiny", "tiny_behind", "odd_size", "cov_precomp", "sh_deg2",
                 "long_14000", "long_40000"]


@pytest.mark.parametrize("name", RASTER_SCENES)
def test_rasterizer_forward_backward(name, monkeypatch):
    """gsr_forward_stage1 / _stage2 / gsr_forward / gsr_backward.  The six scenes of test_gpu_gauss_bwd.py (P < 64, no slots at all,
    heavy groups, flag passes past 512 and 2048), the golden odd image size and precomputed covariances, SH input, and per-tile lists
    beyond 4096 (the 128 KiB LDS sort) and beyond 16384 (the global-memory sort).  Each run is: the two-stage training forward and a
    backward on full upstream gradients; the same view again, which takes the speculative single call, with a backward on RGB-only
    gradients (NULL depth and feature gradients: the cheaper blend variant); the inference forward."""
    from gscream_amd import rasterizer as RZ
    s, grads, tuning = _raster_scene(name)

    def run(arena):
        set_tuning(**tuning)
        rs = Hh.hip_settings(s, DEV)
        out = {"first/" + k: v for k, v in _raster(s, grads, rs=rs).items()}
        assert RZ._last_stage1["speculative"] is False
        out.update({"second/" + k: v for k, v in _raster(s, grads, rgb_only=True, rs=rs).items()})
        assert RZ._last_stage1["speculative"] is True
        with torch.no_grad():
            out.update({"inference/" + k: v for k, v in _raster(s, rs=rs).items()})
        return out
    got = three_runs(monkeypatch, "rasterizer", name, run, mib=768,
                     expect=("gsr_forward_stage1", "gsr_forward_stage2", "gsr_forward", "gsr_backward"))
    for k in ("out_color", "out_depth", "out_unc", "radii"):
        assert np.array_equal(got["first/" + k].view(np.uint32), got["second/" + k].view(np.uint32)), k
        assert np.array_equal(got["first/" + k].view(np.uint32), got["inference/" + k].view(np.uint32)), k


def test_rasterizer_capacity_redo(monkeypatch):
    """GSR_NEED_CAPACITY: after the 37 Gaussians of `tiny` the hint provides for a few hundred instances; `huge_gaussians` on the same
    device then overflows it -- gsr_forward must leave the too-small binning buffer's guards alone -- and stage 2 is redone."""
    from gscream_amd import rasterizer as RZ
    small, _, _ = _raster_scene("tiny")
    big, grads, _ = _raster_scene("huge_gaussians")

    def run(arena):
        set_tuning()
        _raster(small, None)
        cap = RZ._capacity_hint[0][0]
        out = _raster(big, grads)
        ls = RZ._last_stage1
        assert ls["speculative"] is False and ls["num_rendered"] > cap > 0, (ls, cap)
        return out
    three_runs(monkeypatch, "rasterizer", "capacity_redo", run, expect=("gsr_forward", "gsr_forward_stage2", "gsr_backward"))


@pytest.mark.parametrize("name", ["tiny", "mixed_splats", "cov_precomp"])
def test_rasterizer_filters(name, monkeypatch):
    """gsr_filter (radii alone, and with the pixel centres) and gsr_mark_visible: P = 37 (less than a wave), 200, and the
    precomputed-covariance input."""
    from gscream_amd import GaussianRasterizer
    s, _, _ = _raster_scene(name)

    def run(arena):
        rast = GaussianRasterizer(Hh.hip_settings(s, DEV))
        m = dev(s["means3D"])
        kw = dict(cov3D_precomp=dev(s["cov3D_precomp"])) if "cov3D_precomp" in s else dict(scales=dev(s["scales"]), rotations=dev(s["rotations"]))
        radii, px, py = rast.position2D_filter(m, **kw)
        return dict(visible_filter=rast.visible_filter(m, **kw), radii=radii, px=px, py=py, present=rast.markVisible(m))
    three_runs(monkeypatch, "rasterizer", "filters/" + name, run, mib=16, expect=("gsr_filter", "gsr_mark_visible"))


# ==== decode and statistics =====================================================================================================

CAM = [0.3, -0.2, -6.0]
DECODE_NAMES = ("xyz", "color", "opacity", "uncertainty", "scaling", "rot", "neural_opacity", "mask")


def _decode_case(monkeypatch, N, K, vis, what, backward=True, stats=False):
    from oracle import decode_oracle as DO
    from gscream_amd.densify_stats import training_statis
    from gscream_amd.neural_gaussians import generate_neural_gaussians
    ref = DO.Model(N, K, seed=40 + N % 7 + K, dtype=torch.float32)
    g = torch.Generator().manual_seed(N + K)
    vm = None if vis is None else (torch.rand(N, generator=g) < vis)
    drawn = {}

    def draw(key, make):  # the same random tensors in every run, drawn once the shapes are known
        if key not in drawn:
            drawn[key] = make()
        return drawn[key]

    def run(arena):
        dut = copy.deepcopy(ref).to(DEV)
        cam = DO.Camera(dev(torch.tensor(CAM, dtype=torch.float32)))
        vmd = None if vm is None else dev(vm)
        outs = generate_neural_gaussians(cam, dut, vmd, True)
        res = dict(zip(DECODE_NAMES, outs))
        M = outs[0].shape[0]
        if backward:
            ups = draw("ups", lambda: [torch.randn(o.shape, generator=g) for o in outs[:6]])
            sum((o * dev(u)).sum() for o, u in zip(outs[:6], ups)).backward()
            res.update({"grad " + k: p.grad for k, p in dut.named_parameters()})
        if stats:
            uf = draw("uf", lambda: torch.rand(M, generator=g) > 0.4)
            vg = draw("vg", lambda: torch.randn(M, 3, generator=g))
            for how in ("own_mask", "copied_mask"):  # the decode's own tensors (its bookkeeping is reused), then a copy of the mask
                z = lambda *shape: torch.zeros(shape, device=DEV)
                acc = types.SimpleNamespace(n_offsets=K, opacity_accum=z(N, 1), anchor_demon=z(N, 1), offset_gradient_accum=z(N * K, 1),
                                            offset_denom=z(N * K, 1))
                for _ in range(2):  # twice: the accumulators add up in place
                    training_statis(acc, types.SimpleNamespace(grad=dev(vg)), outs[6], dev(uf), outs[7], vmd if how == "own_mask" else dev(vm))
                res.update({f"{how}/{k}": getattr(acc, k) for k in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")})
        return res
    expect = ["gsr_decode_count", "gsr_decode_emit"] + (["gsr_decode_visible_rows"] if vm is not None else [])
    if backward:
        expect += ["gsr_decode_backward"] + (["gsr_decode_zero_hidden_rows"] if vm is not None else [])
    if stats:
        expect.append("gsr_training_stats")
    return three_runs(monkeypatch, "decode", what, run, mib=128, expect=expect)


@pytest.mark.parametrize("N,K", [(1, 10), (15, 10), (17, 10), (255, 10), (257, 10), (1025, 10), (257, 1), (257, 3)])
def test_decode_every_row(N, K, monkeypatch):
    """gsr_decode_count / _emit / _backward without a row list: anchor counts around the 16-anchor step of the matrix-core kernels and
    the 256-anchor scan block (1, 15, 17, 255, 257, 1025 = five blocks), offset counts that leave second-layer tile rows unused (K = 1,
    3).  Every d_* row and all 16 weight gradients come from torch.empty tensors and a torch.empty workspace."""
    _decode_case(monkeypatch, N, K, None, f"N{N}_K{K}")


@pytest.mark.parametrize("vis", [0.65, 0.0])
def test_decode_with_a_visibility_mask_and_statistics(vis, monkeypatch):
    """N = 257 (one block and one anchor) with a device mask: gsr_decode_visible_rows, the row-list kernels, and the backward whose
    visible rows come from gsr_decode_backward and whose hidden rows from gsr_decode_zero_hidden_rows -- all of them, for the all-false
    mask.  gsr_training_stats accumulates in place into guarded model-sized tensors, with the decode's tensors and with a copied mask."""
    got = _decode_case(monkeypatch, 257, 10, vis, f"N257_vis{vis}", stats=True)
    assert (got["xyz"].shape[0] > 0) == (vis > 0)


@pytest.mark.parametrize("N", [0, 255, 256, 257])
def test_decode_visible_rows_block_edges(N, monkeypatch):
    """gsr_decode_visible_rows around its 256-row block (scratch of N // 256 + 2 words), and no rows at all."""
    _decode_case(monkeypatch, N, 10, 0.65, f"visible_rows_N{N}", backward=False)


# ==== RGB loss, depth loss ======================================================================================================

@pytest.mark.parametrize("C,H,W", [(3, 16, 32), (1, 33, 65), (3, 71, 112)])
@pytest.mark.parametrize("weighted", [False, True])
def test_rgb_loss(C, H, W, weighted, monkeypatch):
    """gsr_rgb_loss_forward_window / _backward_window: one tile exactly (16 x 32), one pixel past it both ways with one channel, several
    tiles that are no multiple of it; windows 11 and 3; forward with kept state and backward from a torch.empty workspace."""
    from gscream_amd import loss_utils as L
    rng = np.random.default_rng(C * 1000 + H)
    gt = rng.random((C, H, W)).astype(np.float32)
    img = np.clip(gt + 0.2 * rng.standard_normal(gt.shape), 0, 1).astype(np.float32)
    w = rng.random((1, H, W)).astype(np.float32) if weighted else None

    def run(arena):
        out = {}
        y, m = dev(gt), None if w is None else dev(w)
        x = dev(img).requires_grad_(True)
        loss, l1, ss = L.rgb_loss(x, y, m, 0.2, 1.0, return_parts=True)
        loss.backward()
        out.update(loss11=loss, l1=l1, ssim11=ss, grad11=x.grad)
        x3 = dev(img).requires_grad_(True)
        v = L.ssim(x3, y, window_size=3) if m is None else L.ssim_masked(x3, y, m, window_size=3)
        (0.7 * v).backward()  # a non-unit upstream gradient
        out.update(ssim3=v, grad3=x3.grad)
        return out
    three_runs(monkeypatch, "rgb_loss", f"{C}x{H}x{W}{'_weighted' if weighted else ''}", run, mib=32,
               expect=("gsr_rgb_loss_forward_window", "gsr_rgb_loss_backward_window"))


@pytest.mark.parametrize("H,W", [(1, 33), (9, 17), (64, 64), (142, 252)])
def test_depth_loss(H, W, monkeypatch):
    """gsr_depth_loss_forward / _backward: one row (no vertical neighbour at any of the four scales), sizes the 2^k subsampling does not
    divide, a power of two, and the quarter-resolution training frame; without masks, with three DISTINCT masks (three buffers of their
    own between guard bands, so a kernel that reads one in another's place reads other values), and with the foreground term folded
    into the weight map."""
    from gscream_amd import loss_utils as L
    rng = np.random.default_rng(H * 1000 + W)
    depth = (2.0 + rng.random((1, H, W))).astype(np.float32)
    target = (0.5 * depth + 0.3 + 0.05 * rng.standard_normal(depth.shape)).astype(np.float32)
    mask = (rng.random((1, H, W)) > 0.3).astype(np.float32)
    fg = (rng.random((1, H, W)) > 0.7).astype(np.float32)
    weight = (1.5 * rng.random((1, H, W)) * (rng.random((1, H, W)) > 0.2)).astype(np.float32)
    gmask = (rng.random((1, H, W)) > 0.25).astype(np.float32)

    def run(arena):
        out = {}
        y, m, f = dev(target), dev(mask), dev(fg)
        for how, kw in (("plain", {}), ("masked", dict(lsq_mask=m, l1_weight=dev(weight), grad_mask=dev(gmask))), ("fg", dict(lsq_mask=m, fg_mask=f, lambda_fg=99.0))):
            d = dev(depth).requires_grad_(True)
            loss, parts = L.depth_loss(d, y, lambda_l1=1.0, lambda_smooth=0.5, return_parts=True, **kw)
            (1.3 * loss).backward()
            out.update({how + "/loss": loss, how + "/parts": parts, how + "/grad": d.grad})
        return out
    three_runs(monkeypatch, "depth_loss", f"{H}x{W}", run, mib=32, expect=("gsr_depth_loss_forward", "gsr_depth_loss_backward"))


# ==== kNN =======================================================================================================================

@pytest.mark.parametrize("name", ["P4", "P257", "P5000", "P20000_clustered"])
def test_knn(name, monkeypatch):
    """gsr_knn_mean_dist2: exactly the three neighbours it needs (P = 4), one point past a block, several blocks, and 20 000 points in
    tight clusters of very different sizes: Morton buckets of uneven size, most of them empty."""
    from gscream_amd.simple_knn import distCUDA2
    rng = np.random.default_rng(len(name))
    if name == "P20000_clustered":
        sizes = np.array([9000, 5000, 3000, 1500, 900, 400, 150, 40, 9, 1])
        centres = rng.uniform(-5, 5, (len(sizes), 3))
        pts = np.concatenate([c + 0.01 * (k + 1) * rng.standard_normal((n, 3)) for k, (c, n) in enumerate(zip(centres, sizes))])
        counts = Hh.morton_bucket_counts(pts.astype(np.float32))
        assert pts.shape[0] == 20_000 and counts.max() > 50 * max(1, int(np.median(counts[counts > 0])))
    else:
        pts = rng.uniform(-1, 1, (int(name[1:]), 3))
    pts = pts.astype(np.float32)
    three_runs(monkeypatch, "knn", name, lambda arena: dict(dist2=distCUDA2(dev(pts))), mib=64, expect=("gsr_knn_mean_dist2",))


# ==== anchor growth, scatter_max ================================================================================================

@pytest.fixture
def hip_growth(monkeypatch):
    from gscream_amd import anchor_growing as AG

    def no_fallback(*a, **k):
        raise AssertionError("grow_level fell back to the torch expressions")
    monkeypatch.setattr(AG, "reference_level", no_fallback)
    return AG


@pytest.mark.parametrize("name", ["N1", "N7", "N1000", "N30000", "N300000", "later_level", "empty_and_occupied"])
def test_anchor_growth(name, monkeypatch, hip_growth):
    """gsr_anchor_grow_keys / _emit at the three cell sizes, on the scenes of test_gpu_anchor_grow.py: 1 .. 300 000 anchors, a mask
    shorter than N * K, no candidate at all (M = 0) and candidates that all fall on occupied cells (C = 0).  The outputs are buffers
    sized M of which C rows are defined."""
    from tests.test_gpu_anchor_grow import SIZES, scene

    def run(arena):
        out = {}
        if name == "empty_and_occupied":
            anchor, offset, scaling, feat, mask = scene(2000, seed=4)
            variants = {"empty": (anchor, offset, scaling, feat, torch.zeros_like(mask)),
                        "occupied": (anchor, torch.zeros_like(offset), scaling, feat, torch.ones_like(mask)),
                        "mostly_occupied": (anchor, offset * 0.02, scaling, feat, torch.ones_like(mask))}
        elif name == "later_level":
            variants = {"": scene(5000, seed=3, L=4000 * 10, p=0.3)}
        else:
            N = int(name[1:])
            variants = {"": scene(N, seed=N, p=0.1 if N > 1 else 1.0)}
        for v, args in variants.items():
            for s in SIZES:
                cand, feat = hip_growth.grow_level(*args, s)
                out[f"{v}/{s}/candidate_anchor"], out[f"{v}/{s}/new_feat"] = cand, feat
                if v in ("empty", "occupied"):
                    assert cand.shape[0] == 0
        return out
    three_runs(monkeypatch, "anchor_growth", name, run, mib=2048 if name == "N300000" else 256,
               expect=("gsr_anchor_grow_keys",) + (() if name == "N1" else ("gsr_anchor_grow_emit",)))


@pytest.mark.parametrize("R,F,S_", [(1, 32, 1), (1000, 32, 50), (5000, 1, 7), (3000, 5, 6000), (100000, 32, 20000)])
def test_scatter_max(R, F, S_, monkeypatch):
    """gsr_scatter_max in the shapes of test_gpu_anchor_grow.py; with dim_size = S + 3 the last slots are reached by no row, and at
    (3000, 5, 6000) about two slots in three are empty."""
    from gscream_amd import scatter as SC
    monkeypatch.setattr(SC, "_torch_scatter_max", lambda *a: (_ for _ in ()).throw(AssertionError("took the torch path")))
    g = torch.Generator().manual_seed(R + S_)
    src = torch.randint(-40, 40, (R, F), generator=g).float() / 8
    index = torch.randint(0, S_, (R,), generator=g)

    def run(arena):
        s, i = dev(src), dev(index)
        out, arg = SC.scatter_max(s, i.unsqueeze(1).expand(-1, F), dim=0, dim_size=S_)
        out2, arg2 = SC.scatter_max(s, i, dim=0, dim_size=S_ + 3)
        return dict(out=out, arg=arg, out2=out2, arg2=arg2)
    got = three_runs(monkeypatch, "anchor_growth", f"scatter_max_{R}_{F}_{S_}", run, mib=128, expect=("gsr_scatter_max",))
    assert not got["out2"][S_:].any() and (got["arg2"][S_:] == R).all()


# ==== cross-attention ===========================================================================================================

@pytest.mark.parametrize("b,i,j", [(1, 1, 5), (1, 12, 12), (1, 777, 1301), (2, 300, 450)])
@pytest.mark.parametrize("masked", [False, True])
def test_crossattn(b, i, j, masked, monkeypatch):
    """gsr_crossattn_forward / _backward: a single query row, less than one 16-row tile, sizes that are no multiple of any tile with
    more than one workgroup per direction, and a batch of two; with and without the two masks.  The workspace (row maxima and sums,
    then scratch of the backward) and the four input gradients are torch.empty."""
    from tests.crossattn_helpers import run_module
    from gscream_amd.crossattn import BidirectionalCrossAttention
    torch.manual_seed(b * 100 + i)
    module = BidirectionalCrossAttention(dim=32, heads=2, dim_head=64, context_dim=24).eval()
    g = torch.Generator().manual_seed(i + j)
    x, context = torch.randn(b, i, 32, generator=g), torch.randn(b, j, 24, generator=g)
    g_out, g_cout = torch.randn(b, i, 32, generator=g), torch.randn(b, j, 24, generator=g)
    mask, cmask = torch.rand(b, i, generator=g) < 0.8, torch.rand(b, j, generator=g) < 0.7
    mask[:, 0] = cmask[:, 0] = True

    def run(arena):
        mod = copy.deepcopy(module).to(DEV)
        kw = dict(mask=dev(mask), context_mask=dev(cmask)) if masked else {}
        res = run_module(mod, dev(x), dev(context), dev(g_out), dev(g_cout), **kw)
        assert mod.last_path == "hip"
        return res
    three_runs(monkeypatch, "crossattn", f"{b}_{i}_{j}{'_masked' if masked else ''}", run, mib=128,
               expect=("gsr_crossattn_forward", "gsr_crossattn_backward"))


# ==== anchor sampler, anchor adjust / prune, Adam ===============================================================================

@pytest.mark.parametrize("case", ["N1", "N63", "N4099", "cap17_class13", "not_ok", "empty_rect"])
def test_anchor_sampler(case, monkeypatch):
    """gsr_anchor_sample on the smallest cases of test_gpu_anchor_sampler.py: one anchor, less than a wave, several workgroups with a
    ragged tail, min_num set by a class, a sample that is not ok (all-zero masks) and an empty rectangle.  Defined: both masks in
    full, rows[:min_num] (the rest keeps the caller's -1), info."""
    from tests import anchor_sampler_helpers as AH
    from tests.test_gpu_anchor_sampler import CASES
    from gscream_amd import anchor_sampler as AS
    (visible, x, y, gt, rect), max_pairs = CASES[case]()

    def run(arena):
        src_mask, dst_mask, src_rows, dst_rows, info = AS.sample_crossattn_anchors(*AH.to_torch(visible, x, y, gt, DEV), rect,
                                                                                   max_pairs=max_pairs, seed=0x9E3779B97F4A7C15)
        assert AS.last_path == "hip"
        n = info.tolist()
        k = n[3] if n[4] else 0
        assert bool((src_rows[k:] == -1).all()) and bool((dst_rows[k:] == -1).all()), "entries from min_num on are left untouched"
        return dict(src_mask=src_mask, dst_mask=dst_mask, src_rows=src_rows[:k], dst_rows=dst_rows[:k], info=info)
    three_runs(monkeypatch, "anchor_sampler", case, run, mib=32, expect=("gsr_anchor_sample",))


@pytest.mark.parametrize("N", [7, 257])
@pytest.mark.parametrize("how", ["adjust", "prune"])
def test_anchor_adjust(N, how, monkeypatch):
    """gsr_anchor_adjust_offsets / _plan / _gather through adjust_anchor (growth patched out) and prune_anchor, on stand-ins of 7
    anchors and of one compaction block plus one, keeping every other anchor, all of them and none.  The gathered parameters, moments
    and accumulators are new torch.empty tensors whose pointers travel in a host table; the proxy reads them out of it."""
    from tests.test_anchor_grow import PARAMS
    from tests.test_gpu_anchor_adjust import MOMENTS, base_tensors, build, keep_pattern, no_growth
    from gscream_amd import anchor_adjust as AA
    STATS = ("offset_denom", "offset_gradient_accum", "opacity_accum", "anchor_demon", "uncertainty_accum")

    def run(arena):
        no_growth(monkeypatch)
        out = {}
        base = base_tensors(N, 10, 32, seed=N)
        for pattern in ("alternating", "all", "none"):
            keep = keep_pattern(pattern, N)
            m = build(base, N, 10, 32, keep)
            with torch.no_grad():
                AA.adjust_anchor(m) if how == "adjust" else AA.prune_anchor(m, ~keep)
            assert AA.last_path == "hip"
            for p in PARAMS:
                t = getattr(m, "_" + p)
                out[f"{pattern}/{p}"] = t
                for s in MOMENTS:
                    out[f"{pattern}/{s}_{p}"] = m.optimizer.state[t][s]
            for s in STATS:
                out[f"{pattern}/{s}"] = getattr(m, s)
        return out
    expect = ("gsr_anchor_adjust_plan", "gsr_anchor_adjust_gather") + (("gsr_anchor_adjust_offsets",) if how == "adjust" else ())
    three_runs(monkeypatch, "anchor_adjust", f"{how}_N{N}", run, mib=128, expect=expect)


@pytest.mark.parametrize("count", [1, 33, 65])
def test_adam(count, monkeypatch):
    """gsr_adam_step: one tensor, and more tensors than one table of 32 holds (33: a second launch of one; 65: a third).  Sizes 1 .. 4099
    cover the 16-byte body and the n % 4 tail; one parameter is a view four bytes into its storage (the float-by-float path), one
    gradient is non-contiguous.  Parameters and moments are updated in place inside guarded bodies; their pointers travel in a host
    table, which the proxy reads.  Two steps."""
    from gscream_amd.adam import Adam
    g = torch.Generator().manual_seed(count)
    sizes = [(1, 2, 3, 4, 5, 63, 257, 1023, 4099)[k % 9] for k in range(count)]
    values = [torch.randn(n, generator=g) for n in sizes]
    grads = [[torch.randn(n, generator=g) for n in sizes] for _ in range(2)]

    def run(arena):
        params = []
        for k, v in enumerate(values):
            t = dev(torch.cat([torch.zeros(1), v]))[1:] if k == 2 else dev(v)  # k = 2: 4-byte aligned only
            params.append(torch.nn.Parameter(t))
        groups = [{"params": params[:count // 2 + 1], "lr": 0.01}, {"params": params[count // 2 + 1:], "lr": 0.002}]
        opt = Adam([g_ for g_ in groups if g_["params"]], eps=1e-15)
        for step in range(2):
            for k, p in enumerate(params):
                p.grad = dev(torch.stack([grads[step][k], grads[step][k]], 1))[:, 0] if k == 1 % count else dev(grads[step][k])
            assert params[1 % count].grad.is_contiguous() == (params[1 % count].numel() == 1)
            opt.step()
            assert opt.last_path == "hip"
        out = {}
        for k, p in enumerate(params):
            out[f"p{k}"], out[f"m{k}"], out[f"v{k}"] = p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
        return out
    three_runs(monkeypatch, "adam", f"{count}_tensors", run, mib=64, expect=("gsr_adam_step",))


# ==== normals, metrics, frames ==================================================================================================

def test_normals(monkeypatch):
    """gsr_depth_points / gsr_point_normals on 37 x 53: neither a multiple of the 16 x 16 tile, three by four workgroups, every
    border pixel's 9 x 9 window clamped; and window sizes 3 and 15."""
    from tests.normals_helpers import synthetic_frame
    from gscream_amd import normals as Nm
    depth, K, c2w = synthetic_frame(37, 53, seed=7)

    def run(arena):
        d, k, c = dev(np.asarray(depth, np.float32))[None], dev(np.asarray(K, np.float32)), dev(np.asarray(c2w, np.float32))
        pts = Nm.depth2pcd_fromplane(d, c, k, 37, 53)
        assert Nm.last_path == "hip"
        out = dict(points=pts, picture=Nm.normal_map(d, c, k))
        for size in (3, 9, 15):
            out[f"normals{size}"] = Nm.least_square_normal_regress_fast01(pts, size=size)
            assert Nm.last_path == "hip"
        return out
    three_runs(monkeypatch, "normals", "37x53", run, mib=32, expect=("gsr_depth_points", "gsr_point_normals"))


@pytest.mark.parametrize("flags", [dict(), dict(clamp=True, quantize=True)])
def test_metrics(flags, monkeypatch):
    """gsr_image_metrics on a batch of two 37 x 53 RGB images (the tile is 16 x 32: three by two tiles, none full at the edges), without a
    mask, with a [B,1,H,W] mask (channel stride 0) and with one [H,W] mask for the whole batch (batch stride 0)."""
    from tests.metrics_helpers import noise_pair, random_mask
    from gscream_amd import metrics as M
    pred, gt = noise_pair(37, 53, c=3, b=2, seed=3)
    mask_b, mask_1 = random_mask((2, 1, 37, 53), 1), random_mask((37, 53), 2)

    def run(arena):
        p, g = dev(pred), dev(gt)
        out = {}
        for how, m in (("plain", None), ("mask_b", dev(mask_b)), ("mask_1", dev(mask_1))):
            r = M.image_metrics(p, g, m, **flags)
            assert M.last_path == "hip"
            out.update({f"{how}/{k}": v for k, v in zip(r._fields, r)})
        return out
    three_runs(monkeypatch, "metrics", "2x3x37x53" + ("_clamp_quantize" if flags else ""), run, mib=32, expect=("gsr_image_metrics",))


def test_frames(monkeypatch):
    """gsr_frame_stats / gsr_frame_compose.  37 x 53 (a byte-store tail: 4 * 53 * 3 is no multiple of 4 pixels' dwords) as one view
    through rgbd_frame and view_frames (flipped panels, the interleaved normal layout, a stride-0 channel, the four-channel
    picture), and a batch of two 5 x 7 frames (panels narrower than one thread's four pixels) through frame_stats and compose."""
    from tests import frames_helpers as O
    from gscream_amd import frames as Fr
    v = O.view_inputs(37, 53, 11)
    pair = [O.view_inputs(5, 7, 20 + b) for b in range(2)]
    two = {k: np.stack([p[k] for p in pair]) for k in pair[0]}

    def run(arena):
        t = {k: dev(a) for k, a in v.items()}
        fr = Fr.rgbd_frame(t["render"], t["depth"], t["uncertainty"], t["normals"], panels=True)
        vf = Fr.view_frames(*[t[k] for k in ("render", "uncertainty", "gt", "depth", "midas", "mask")])
        assert Fr.last_path == "hip"
        out = dict(rgbd=fr.rgbd, sheet=vf.sheet, depth=vf.depth, params=vf.params, u8=Fr.to_uint8(t["render"], clamp=True))
        b = {k: dev(a) for k, a in two.items()}
        stats, params = Fr.frame_stats(b["depth"][:, 0], b["midas"][:, 0], 1 - b["mask"][:, 0])
        lut = Fr.colormap_lut("viridis", DEV)
        out.update(stats2=stats, params2=params,
                   sheet2=Fr.compose([Fr.Panel(Fr.QUANT_CLAMP, b["render"], flip=True), Fr.Panel(Fr.ABSDIFF, b["render"], b["gt"]),
                                      Fr.Panel(Fr.CMAP_CV, b["depth"], lut=lut)], params=params),
                   depth2=Fr.compose([Fr.Panel(Fr.CMAP_MPL_ALIGNED, b["depth"], lut=lut), Fr.Panel(Fr.CMAP_MPL, b["midas"], lut=lut)],
                                     channels=4, params=params))
        assert Fr.last_path == "hip"
        return out
    three_runs(monkeypatch, "frames", "37x53_and_2x5x7", run, mib=32, expect=("gsr_frame_stats", "gsr_frame_compose"))


# ==== PNG encode and decode =====================================================================================================

PNG_SHAPES = {"small_C1": (23, 31, 1), "small_C3": (23, 31, 3), "small_C4": (23, 31, 4), "cut_C1": (80, 417, 1), "cut_C3": (71, 157, 3),
              "cut_C4": (70, 117, 4)}


def _png_files(arena_run):
    """Encode the six pictures and the strided panel -> ({name: file bytes}, outputs to compare)."""
    from gscream_amd import png
    out, files = {}, {}
    for name, (H, W, C) in PNG_SHAPES.items():
        stream = H * (1 + W * C)
        assert (stream < png.CHUNK) if name.startswith("small") else (stream > png.CHUNK and png.CHUNK % (1 + W * C) != 0)
        batch = png.encode(dev(S.picture("texture", H, W, C, seed=H + W)))
        assert png.last_path == "hip"
        (files[name],) = png.to_bytes(batch)
        out[name + "/header"] = batch.data[0, :png.HEADER]
    sheet = dev(np.concatenate([S.picture(k, 37, 53, 3, seed=5) for k in ("texture", "colormap", "mask", "noise")], 1))
    panel = sheet[:, 53:106]
    assert not panel.is_contiguous()
    (files["panel"],) = png.to_bytes(png.encode(panel))
    files["panels"] = b"".join(png.to_bytes(png.encode(png._panels(sheet, 4))))
    out.update({k + "/file": np.frombuffer(v, np.uint8) for k, v in files.items()})
    return files, out


def test_png_encode(monkeypatch):
    """gsr_png_encode for C = 1, 3, 4: pictures whose stream is less than one 32 KiB chunk, pictures whose stream crosses the chunk
    boundary in the middle of a row, a strided panel of a wider sheet read in place, and a batch of four such panels.  Defined: the
    16 header bytes and each file up to its byte count; nothing behind a file's last byte may be written, which the poison of the
    exactly sized output buffer and the guards behind it hold."""
    three_runs(monkeypatch, "png_encode", "six_pictures_and_panels", lambda arena: _png_files(arena)[1], mib=64, expect=("gsr_png_encode",))


def test_png_decode(monkeypatch):
    """gsr_png_decode on the files gsr_png_encode wrote (several IDATs: the parallel path), a PIL-written file (one IDAT, zlib's
    own blocks: the serial path) and a truncated file, in ONE call.  The truncated file ends in its status code; its picture is
    unspecified and is left out of the comparison, but it must write nothing outside its own picture: the other pictures, the
    status words and every guard are compared."""
    import io
    from PIL import Image
    from tests.png_decode_helpers import TRUNCATED, corrupt
    from gscream_amd import png_decode as PD
    bad = next(c for c in corrupt() if c.name == "corrupt-truncated")
    buf = io.BytesIO()
    pil_image = S.picture("colormap", 37, 53, 3, seed=2)
    Image.fromarray(pil_image).save(buf, format="PNG")

    def run(arena):
        files, _ = _png_files(arena)
        names = [k for k in files if k != "panels"] + ["pil", "truncated"]
        data = [files[k] for k in names[:-2]] + [buf.getvalue(), bad.data]
        pics = PD.decode(data, DEV, verify_crc=True, names=names)
        assert PD.last_path == "hip"
        status = pics.status.tolist()
        assert status[:-1] == [0] * (len(names) - 1) and status[-1] == TRUNCATED == bad.status, status
        out = dict(status=pics.status, paths=pics.paths)
        out.update({n: im for n, im in zip(names[:-1], pics.images[:-1])})
        assert np.array_equal(out["pil"].cpu().numpy(), pil_image)
        return out
    three_runs(monkeypatch, "png_decode", "encoded_pil_truncated", run, mib=64, expect=("gsr_png_encode", "gsr_png_decode"))


# ==== scene initialisation ======================================================================================================

def _sort_sizes():
    from gscream_amd import _native
    B = int(_native.load().gsr_sort_block_keys())
    return B, [0, 1, B - 1, B, B + 1, 3 * B + 17]


def test_sort_keys_and_kth_smallest(monkeypatch):
    """gsr_sort_keys_u64 and gsr_kth_smallest_f32 at n = 0, 1, B - 1, B, B + 1, 3 B + 17 with B the keys one workgroup ranks: nothing,
    one key, one short of a block, a block, a block and one key, three blocks and a ragged tail.  Keys with all eight digits in use,
    and keys whose upper digits are constant (the skipped passes)."""
    from gscream_amd import scene_init as SI
    B, sizes = _sort_sizes()
    g = torch.Generator().manual_seed(B)
    keys = {n: torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), generator=g, dtype=torch.int64) for n in sizes}
    low = {n: torch.randint(0, 70000, (n,), generator=g, dtype=torch.int64) for n in sizes}
    vals = {n: torch.randn(n, generator=g) for n in sizes}

    def run(arena):
        out = {}
        for n in sizes:
            out[f"sorted{n}"], out[f"sorted_low{n}"] = SI.sort_keys(dev(keys[n])), SI.sort_keys(dev(low[n]))
            if n == 0:
                with pytest.raises(IndexError):
                    SI.kth_smallest(dev(vals[n]), 1)
                continue
            for k in sorted({1, (n + 1) // 2, n}):
                out[f"kth{n}_{k}"] = SI.kth_smallest(dev(vals[n]), k)
                assert SI.last_path == "hip"
        return out
    got = three_runs(monkeypatch, "scene_init", "sort_and_kth", run, mib=128, expect=("gsr_sort_keys_u64", "gsr_kth_smallest_f32"))
    n = sizes[-1]
    assert np.array_equal(got[f"sorted{n}"].view(np.uint64), np.sort(keys[n].numpy().view(np.uint64)))
    assert got[f"kth{n}_{(n + 1) // 2}"] == np.sort(vals[n].numpy())[(n + 1) // 2 - 1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_voxelize_and_create_from_pcd(dtype, monkeypatch):
    """gsr_voxelize, gsr_knn_mean_dist2, gsr_kth_smallest_f32 and gsr_scene_init_fill through voxelize_sample and create_from_pcd on the
    5000-point `dense` cloud (about six points per occupied voxel, so M < N and the out buffer sized N is part written), in fp32 and
    fp64, with a given voxel size and with voxel_size <= 0 (the median 3-NN distance, read from the device)."""
    from tests.scene_init_helpers import case_points
    from gscream_amd import scene_init as SI
    pts = case_points("dense", dtype)
    fields = ("_anchor", "_offset", "_anchor_feat", "_scaling", "_rotation", "_opacity", "_uncertainty", "max_radii2D", "xyz_max", "dist2")

    def run(arena):
        out = dict(voxels=SI.voxelize_sample(dev(pts), 0.01))
        assert SI.last_path == "hip" and 0 < out["voxels"].shape[0] < pts.shape[0]
        for how, v in (("given", 0.01), ("median", 0.0)):
            s = SI.create_from_pcd(dev(pts), voxel_size=v, n_offsets=10, feat_dim=32, device=DEV)
            out.update({f"{how}/{k}": getattr(s, k) for k in fields})
            out[f"{how}/voxel_size"] = np.float64(s.voxel_size)
        return out
    three_runs(monkeypatch, "scene_init", f"pcd_{np.dtype(dtype).name}", run, mib=64,
               expect=("gsr_voxelize", "gsr_knn_mean_dist2", "gsr_kth_smallest_f32", "gsr_scene_init_fill"))
