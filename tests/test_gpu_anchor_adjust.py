"""Anchor pruning on the HIP path, bit-exact (torch.equal / int32 views, no tolerances).

* gscream_amd.anchor_adjust.adjust_anchor on a stand-in replays tests/golden/ref_adjust_anchor.npz (the reference's own method,
  recorded on the CPU) with the HIP growing step in the middle;
* the HIP path against the package's torch path (the reference's expression sequence, which tests/test_anchor_adjust.py replays
  against the fixture) on the same device, with the growing step patched out or replaced by a deterministic stand-in that adds rows;
* what the kernels rely on: torch's fp32 comparison with / product by a Python scalar, and the IEEE division;
* no host stop besides the one read-back of `info`; one training iteration before and after a real adjust_anchor."""
import os
import sys
import traceback
import types

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_anchor_adjust import FIXTURE, CASES, STATS, adjust_args, assert_matches_fixture, load_case  # noqa: E402
from tests.test_anchor_grow import PARAMS, Standin, replay  # noqa: E402
from tests.test_gpu_anchor_grow import HostExpStandin, device_constants  # noqa: E402

from gscream_amd import anchor_adjust as _AA  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH_PATH = (_AA._adjust_torch, _AA._prune_torch)  # the real ones: the AA fixture below makes the module's raise
MOMENTS = ("exp_avg", "exp_avg_sq")


@pytest.fixture
def AA(monkeypatch):
    """The module with its torch path (and the growing step's torch fallback) made to raise: these tests must run the kernels."""
    from gscream_amd import anchor_growing as AG
    A = _AA

    def no_fallback(*a, **k):
        raise AssertionError("took the torch path")
    for name in ("_adjust_torch", "_prune_torch"):
        monkeypatch.setattr(A, name, no_fallback)
    monkeypatch.setattr(AG, "reference_level", no_fallback)
    return A


def no_growth(monkeypatch):
    from gscream_amd import anchor_growing as AG
    monkeypatch.setattr(AG, "anchor_growing", lambda model, grads, threshold, offset_mask: None)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- the fixture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_adjust_anchor_replays_the_reference(case, monkeypatch, AA):
    z = np.load(FIXTURE)
    m, draws, mlp_before = load_case(z, case, DEV, cls=HostExpStandin)
    replay(monkeypatch, draws)
    with torch.no_grad():
        AA.adjust_anchor(m, **adjust_args(z))
    assert AA.last_path == "hip"
    assert_matches_fixture(z, case, m, mlp_before, device_constants(z))


# ---- HIP against the torch path on the device ----------------------------------------------------------------------------------
def base_tensors(N, K, F, seed):
    """Seeded tensors of a model of N anchors on the device, with NaN and -0.0 sprinkled over every one of them."""
    g = torch.Generator().manual_seed(seed)
    shapes = dict(anchor=(N, 3), offset=(N, K, 3), anchor_feat=(N, F), opacity=(N, 1), uncertainty=(N, 1), scaling=(N, 6), rotation=(N, 4))

    def spoil(t, zeros=True):
        r = torch.rand(t.shape, generator=g)
        t[r < 0.02] = float("nan")
        if zeros:
            t[(r >= 0.02) & (r < 0.04)] = -0.0
        return t.to(DEV)
    out = {}
    for p, sh in shapes.items():
        out[p] = spoil(torch.randn(sh, generator=g) * (0.08 if p == "scaling" else 1.0))  # scaling: both sides of 0.05
        for s in MOMENTS:
            out[f"{s}_{p}"] = spoil(torch.randn(sh, generator=g))
    out["uncertainty_accum"] = spoil(torch.rand(N, 1, generator=g) * 9)
    out["offset_denom"] = spoil(torch.randint(0, 100, (N * K, 1), generator=g).float())
    out["offset_gradient_accum"] = spoil(torch.rand(N * K, 1, generator=g) * 0.01 * out["offset_denom"].cpu().nan_to_num())
    out["demon_kept"] = spoil(torch.randint(0, 200, (N, 1), generator=g).float())
    out["demon_pruned"] = torch.randint(81, 200, (N, 1), generator=g).float().to(DEV)
    out["opacity_kept"] = spoil(5.0 + torch.rand(N, 1, generator=g), zeros=False)  # (an accumulated -0.0 would be pruned, rightly)
    return out


def keep_pattern(name, N):
    i = torch.arange(N)
    if name in ("random5", "random95"):
        return (torch.rand(N, generator=torch.Generator().manual_seed(N)) >= (0.05 if name == "random5" else 0.95)).to(DEV)
    return {"all": i >= 0, "none": i < 0, "alternating": i % 2 == 0, "first": i == 0, "last": i == N - 1}[name].to(DEV)


PATTERNS = ("all", "none", "alternating", "first", "last", "random5", "random95")


def build(base, N, K, F, keep, state=True):
    """A stand-in whose adjust_anchor keeps exactly `keep`: pruned anchors were seen > 80 times with no opacity."""
    m = Standin(n_offsets=K, feat_dim=F)
    groups = []
    for p in PARAMS:
        t = nn.Parameter(base[p].clone())
        setattr(m, "_" + p, t)
        groups.append({"params": [t], "lr": 0.01, "name": p})
    m.mlp_color = nn.Linear(3, 2).to(DEV)
    groups.insert(3, {"params": list(m.mlp_color.parameters()), "lr": 0.002, "name": "mlp_color"})
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    if state:
        for grp in m.optimizer.param_groups:
            if grp["name"] in PARAMS:
                m.optimizer.state[grp["params"][0]] = {"step": torch.tensor(5.0), **{s: base[f"{s}_{grp['name']}"].clone() for s in MOMENTS}}
    k = keep.view(-1, 1)
    m.anchor_demon = torch.where(k, base["demon_kept"], base["demon_pruned"])
    m.opacity_accum = torch.where(k, base["opacity_kept"], torch.zeros_like(base["opacity_kept"]))
    for a in ("uncertainty_accum", "offset_denom", "offset_gradient_accum"):
        setattr(m, a, base[a].clone())
    return m


def assert_same_model(a, b, what):
    """Two stand-ins after adjust_anchor: every tensor bit for bit, the optimiser keyed alike."""
    for p in PARAMS:
        ta, tb = getattr(a, "_" + p), getattr(b, "_" + p)
        assert ta.shape == tb.shape and ta.dtype == tb.dtype and torch.equal(bits(ta), bits(tb)), (what, p)
        assert isinstance(ta, nn.Parameter) and ta.requires_grad and ta.grad is None and ta.is_contiguous(), (what, p)
        ga = next(g for g in a.optimizer.param_groups if g["name"] == p)
        assert ga["params"][0] is ta, (what, p)
        sa, sb = a.optimizer.state.get(ta, None), b.optimizer.state.get(tb, None)
        assert (sa is None) == (sb is None), (what, p)
        if sa is not None:
            assert float(sa["step"]) == float(sb["step"]) and set(sa) == set(sb)
            for s in MOMENTS:
                assert sa[s].shape == sb[s].shape and torch.equal(bits(sa[s]), bits(sb[s])), (what, p, s)
    assert len(a.optimizer.state) == len(b.optimizer.state), what
    for s in STATS + ("max_radii2D",):
        ta, tb = getattr(a, s), getattr(b, s)
        assert ta.shape == tb.shape and ta.dtype == tb.dtype == torch.float32 and torch.equal(bits(ta), bits(tb)), (what, s)


def both_paths(AA, monkeypatch, base, N, K, F, keep, state=True, call=None):
    """Two equal stand-ins, one through the HIP path and one through the torch path (force_torch, the real functions back in place)."""
    call = call or (lambda mod, m: mod.adjust_anchor(m))
    hip, ref = build(base, N, K, F, keep, state), build(base, N, K, F, keep, state)
    with torch.no_grad():
        call(AA, hip)
        assert AA.last_path == "hip"
        with monkeypatch.context() as mp:
            mp.setattr(AA, "force_torch", True)
            mp.setattr(AA, "_adjust_torch", TORCH_PATH[0])
            mp.setattr(AA, "_prune_torch", TORCH_PATH[1])
            call(AA, ref)
            assert AA.last_path == "torch"
    return hip, ref


def sizes():
    from gscream_amd.anchor_adjust import BLOCK_ANCHORS as B
    return [1, 7, B - 1, B, B + 1, 2 * B + 1, 4097, 300000]


@pytest.mark.parametrize("N", [1, 7, 255, 256, 257, 513, 4097, 300000])
def test_hip_equals_the_torch_path(N, monkeypatch, AA):
    assert N in sizes()  # B - 1, B, B + 1, 2 B + 1 of the compaction kernel's block
    no_growth(monkeypatch)
    for K, F in ((10, 32),) + (((1, 1),) if N <= 4097 else ()):
        base = base_tensors(N, K, F, seed=N + K)
        for pattern in PATTERNS:
            keep = keep_pattern(pattern, N)
            hip, ref = both_paths(AA, monkeypatch, base, N, K, F, keep)
            assert_same_model(hip, ref, (N, K, F, pattern))
            n_keep = int(keep.sum())
            assert hip._anchor.shape[0] == n_keep and tuple(hip.offset_denom.shape) == (n_keep * K, 1)
            assert torch.equal(bits(hip._anchor_feat), bits(base["anchor_feat"][keep]))
    hip, ref = both_paths(AA, monkeypatch, base, N, K, F, keep_pattern("alternating", N), state=False)
    assert_same_model(hip, ref, (N, "no state"))
    assert len(hip.optimizer.state) == 0


@pytest.mark.parametrize("N", [7, 257, 4097])
def test_prune_anchor_hip_equals_the_torch_path(N, monkeypatch, AA):
    base = base_tensors(N, 10, 32, seed=N)
    for pattern in PATTERNS:
        keep = keep_pattern(pattern, N)
        hip, ref = both_paths(AA, monkeypatch, base, N, 10, 32, keep, call=lambda mod, m: mod.prune_anchor(m, ~keep))
        for p in PARAMS:
            ta, tb = getattr(hip, "_" + p), getattr(ref, "_" + p)
            assert torch.equal(bits(ta), bits(tb)) and ta.grad is None and hip.optimizer.state[ta]["exp_avg"].shape == ta.shape, (pattern, p)
            for s in MOMENTS:
                assert torch.equal(bits(hip.optimizer.state[ta][s]), bits(ref.optimizer.state[tb][s])), (pattern, p, s)
        for s in STATS:  # left to the caller, as in the reference
            assert torch.equal(bits(getattr(hip, s)), bits(getattr(ref, s)))


def test_zero_anchors(monkeypatch, AA):
    no_growth(monkeypatch)
    m = build(base_tensors(0, 10, 32, seed=1), 0, 10, 32, keep_pattern("all", 0))
    leaf = m._anchor
    with torch.no_grad():
        AA.adjust_anchor(m)
    assert AA.last_path == "hip" and m._anchor is leaf
    assert tuple(m.offset_denom.shape) == (0, 1) and tuple(m.anchor_demon.shape) == (0, 1) and tuple(m.max_radii2D.shape) == (0,)


def test_after_growth_the_offset_statistics_are_padded(monkeypatch, AA):
    """N1 > N0 with offset_denom still N0 * K long: rows the growing step added read zero statistics."""
    from gscream_amd import anchor_growing as AG
    from tests.test_anchor_grow import ACCUMS
    N0, K, F = 1000, 10, 32
    seen = []

    def fake_growing(model, grads, threshold, offset_mask):
        seen.append((grads.clone(), offset_mask.clone()))
        C, g = 337, torch.Generator().manual_seed(3)
        d = {p: torch.randn((C,) + tuple(getattr(model, "_" + p).shape[1:]), generator=g).to(DEV) for p in PARAMS}
        for a in ACCUMS:
            setattr(model, a, torch.cat([getattr(model, a), torch.zeros([C, 1], device=DEV)], dim=0))
        for k, v in model.cat_tensors_to_optimizer(d).items():
            setattr(model, "_" + k, v)
    monkeypatch.setattr(AG, "anchor_growing", fake_growing)
    base = base_tensors(N0, K, F, seed=8)
    keep = keep_pattern("random5", N0)
    hip, ref = both_paths(AA, monkeypatch, base, N0, K, F, keep)
    assert_same_model(hip, ref, "after growth")
    n_keep = int(keep.sum()) + 337
    assert hip._anchor.shape[0] == n_keep and hip.offset_denom.shape[0] == n_keep * K
    assert not hip.offset_denom[-337 * K:].any() and not hip.offset_gradient_accum[-337 * K:].any() and not hip.anchor_demon[-337:].any()
    (g_hip, m_hip), (g_ref, m_ref) = seen  # what the growing step was handed: :916-919 on both paths
    assert g_hip.shape == (N0 * K,) and torch.equal(bits(g_hip), bits(g_ref)) and m_hip.dtype == torch.bool and torch.equal(m_hip, m_ref)


def test_nan_and_negative_zero_survive_and_resets_write_positive_zero(monkeypatch, AA):
    no_growth(monkeypatch)
    N, K, F = 600, 10, 32
    base = base_tensors(N, K, F, seed=11)
    odd = torch.tensor([0x7FC12345, -0x3FFFFF, -0x80000000, 0x7F800001, 1, -0x7FFFFFFF], dtype=torch.int32, device=DEV)  # NaNs, -0.0, denormals
    for k, t in base.items():
        if k.startswith(("anchor", "offset", "opacity", "uncertainty", "rotation", "exp_avg")) and not k.startswith("offset_"):
            spots = bits(t).view(-1)[:: max(1, t.numel() // 50)]  # a view: writes land in the tensor
            spots.copy_(odd[torch.arange(spots.numel(), device=DEV) % 6])
    base["demon_kept"] = torch.where(torch.arange(N, device=DEV).view(-1, 1) % 3 == 0, torch.full((N, 1), 120.0, device=DEV), torch.full((N, 1), 10.0, device=DEV))
    base["opacity_kept"] = torch.full((N, 1), 7.0, device=DEV)
    base["uncertainty_accum"] = torch.full((N, 1), -0.0, device=DEV)
    base["offset_denom"] = torch.where(torch.arange(N * K, device=DEV).view(-1, 1) % 2 == 0, torch.full((N * K, 1), 90.0, device=DEV),
                                       torch.full((N * K, 1), -0.0, device=DEV))
    base["offset_gradient_accum"] = torch.full((N * K, 1), -0.0, device=DEV)
    keep = keep_pattern("random5", N)
    m = build(base, N, K, F, keep)
    with torch.no_grad():
        AA.adjust_anchor(m)
    for p in PARAMS:
        if p != "scaling":
            assert torch.equal(bits(getattr(m, "_" + p)), bits(base[p][keep])), p
        for s in MOMENTS:
            assert torch.equal(bits(m.optimizer.state[getattr(m, "_" + p)][s]), bits(base[f"{s}_{p}"][keep])), (p, s)
    sc = base["scaling"][keep]
    want = torch.cat([sc[:, :3], torch.where(sc[:, 3:] > 0.05, torch.full_like(sc[:, 3:], 0.05), sc[:, 3:])], dim=1)
    assert torch.equal(bits(m._scaling), bits(want)) and m._scaling[:, 3:].isnan().any() and (sc[:, 3:] > 0.05).any()
    was_reset = (base["demon_kept"] > 80)[keep]
    neg_zero = -0x80000000
    u = bits(m.uncertainty_accum)
    assert bool((u[was_reset] == 0).all()) and bool((u[~was_reset] == neg_zero).all()) and was_reset.any() and (~was_reset).any()
    assert bool((bits(m.anchor_demon)[was_reset] == 0).all()) and bool((m.anchor_demon[~was_reset] == 10.0).all())
    d = bits(m.offset_denom).view(-1, K)
    assert bool((d[:, 0::2] == 0).all()) and bool((d[:, 1::2] == neg_zero).all())  # denom > 40: reset to +0.0; -0.0 rows are copied
    assert bool((bits(m.offset_gradient_accum).view(-1, K)[:, 1::2] == neg_zero).all())


def test_plan_is_reproducible_and_keep_rows_ascend(AA):
    N = 70001
    g = torch.Generator().manual_seed(5)
    demon = torch.randint(0, 200, (N, 1), generator=g).float().to(DEV)
    acc = (torch.rand(N, 1, generator=g) * 0.01 * demon.cpu()).to(DEV)
    a = AA._plan_hip(N, torch.device(DEV), acc, demon, None, 0.005, 80.0)
    b = AA._plan_hip(N, torch.device(DEV), acc, demon, None, 0.005, 80.0)
    prune = ((acc < 0.005 * demon) & (demon > 80)).view(-1)
    n_keep, n_prune, n_reset, zero = a[2].tolist()
    assert (n_keep, n_prune, n_reset, zero) == (int((~prune).sum()), int(prune.sum()), int((demon > 80).sum()), 0) and 0 < n_prune < n_keep
    rows = a[0][:n_keep]
    assert bool((rows[1:] > rows[:-1]).all()) and torch.equal(rows.long(), torch.nonzero(~prune).view(-1))
    assert torch.equal(a[0][:n_keep], b[0][:n_keep]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert torch.equal(a[1], (demon > 80).view(-1))
    m = AA._plan_hip(N, torch.device(DEV), prune_mask=prune)  # the standalone prune_anchor: the mask as given, no resets
    assert m[2].tolist() == [n_keep, n_prune, 0, 0] and torch.equal(m[0][:n_keep], rows) and not m[1].any()


# ---- what the kernels rely on ------------------------------------------------------------------------------------------------
def test_python_scalars_meet_fp32_tensors_in_fp32(AA):
    """The thresholds are Python products compared in fp32, min_opacity * anchor_demon is one fp32 product: what torch does on the
    device, on values where the fp32 and the fp64 reading differ, and what the kernels do."""
    check_interval, success_threshold, min_opacity = 100, 0.7, 0.005
    rounded_up = 0
    for thr in (check_interval * success_threshold * 0.5, check_interval * success_threshold, 3 * success_threshold, 0.1, 1 / 3):
        t32 = np.float32(thr)
        assert float(t32) != thr or thr in (35.0, 70.0)   # (100 * 0.7 happens to be exact; the others are not)
        x = np.array([t32, np.nextafter(t32, np.float32(1e9)), np.nextafter(t32, np.float32(-1e9)), 2.0, 3.0, 35.0, 36.0, 69.0, 70.0, 71.0], np.float32)
        xd = torch.from_numpy(x).to(DEV).view(-1, 1)
        got = (xd > thr).view(-1).cpu().numpy()
        assert np.array_equal(got, x > t32)
        if float(t32) > thr:  # rounded up: x == (float)thr is above the fp64 threshold and not above the fp32 one
            assert not np.array_equal(got, x.astype(np.float64) > thr)
            rounded_up += 1
        _g, mask = AA._offsets_hip(torch.zeros_like(xd), xd, thr)
        assert np.array_equal(mask.cpu().numpy(), x > t32)
        _rows, reset, _info = AA._plan_hip(len(x), torch.device(DEV), torch.zeros_like(xd), xd, None, min_opacity, thr)
        assert np.array_equal(reset.cpu().numpy(), x > t32)
    assert rounded_up >= 2
    g = torch.Generator().manual_seed(6)
    demon = torch.randint(81, 100000, (1 << 16, 1), generator=g).float()
    prod32 = np.float32(min_opacity) * demon.numpy()
    acc = torch.from_numpy(np.where(np.arange(1 << 16).reshape(-1, 1) % 2 == 0, prod32, np.nextafter(prod32, np.float32(-1))).astype(np.float32))
    want = acc.numpy() < prod32
    got = (acc.to(DEV) < min_opacity * demon.to(DEV)).cpu().numpy()
    assert np.array_equal(got, want) and want[1::2].all() and not want[0::2].any()
    assert not np.array_equal(acc.numpy().astype(np.float64) < min_opacity * demon.numpy().astype(np.float64), want)
    rows, _reset, info = AA._plan_hip(1 << 16, torch.device(DEV), acc.to(DEV), demon.to(DEV), None, min_opacity, 80.0)
    assert info.tolist()[:2] == [1 << 15, 1 << 15] and torch.equal(rows[:1 << 15].cpu(), torch.arange(0, 1 << 16, 2, dtype=torch.int32))


def test_offset_division_is_torchs(AA):
    """accum / denom, NaN -> 0, |.|: kernel against torch on 2^20 pairs with 0/0, x/0, denormal operands and denormal quotients."""
    g = torch.Generator().manual_seed(7)
    n = 1 << 20
    accum = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 8)
    denom = torch.randint(0, 300, (n,), generator=g).float()
    denom[::5] = (torch.rand(n, generator=g) * 100)[::5]
    accum[::7] = 0.0
    accum[3::64] = torch.randn(n, generator=g)[3::64] * 1e-41          # denormal numerators
    denom[5::64] = torch.rand(n, generator=g)[5::64] * 1e-40           # denormal denominators
    accum[9::64] = torch.randn(n, generator=g)[9::64] * 1e-37
    denom[9::64] = 200.0                                               # normal / normal -> denormal
    accum, denom = accum.to(DEV).view(-1, 1), denom.to(DEV).view(-1, 1)
    grads = accum / denom
    assert grads.isnan().any() and grads.isinf().any()
    tiny = grads[(grads != 0) & grads.isfinite()].abs().min()
    assert float(tiny) < 1.1754944e-38  # denormal quotients are present (nothing flushes them)
    grads[grads.isnan()] = 0.0
    want = torch.norm(grads, dim=-1)
    got, mask = AA._offsets_hip(accum, denom, 40.0)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(mask, (denom > 40.0).view(-1))
    with np.errstate(all="ignore"):  # and both are the correctly rounded quotient (53 >= 2 * 24 + 2: rounding the fp64 quotient again is exact)
        exact = np.abs(np.nan_to_num((accum.cpu().numpy().astype(np.float64) / denom.cpu().numpy().astype(np.float64)).astype(np.float32),
                                     nan=0.0, posinf=np.inf, neginf=-np.inf)).reshape(-1)
    assert np.array_equal(got.cpu().numpy().view(np.int32), exact.view(np.int32))


# ---- host stops ---------------------------------------------------------------------------------------------------------------
def test_the_info_read_back_is_the_only_host_stop(monkeypatch, AA):
    no_growth(monkeypatch)
    N, K, F = 5000, 10, 32
    base = base_tensors(N, K, F, seed=9)
    keep = keep_pattern("random5", N)
    warm, a, b = (build(base, N, K, F, keep) for _ in range(3))
    with torch.no_grad():
        AA.adjust_anchor(warm)  # library loading and first allocations out of the way
        n_keep = int(keep.sum())
        info = [n_keep, N - n_keep, 0, 0]
        torch.cuda.synchronize()
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            AA._adjust_hip(a, 100, 0.8, 0.0002, 0.005, info=info)  # offsets, plan, gather and the re-keying: nothing raises
            with pytest.raises(RuntimeError) as err:
                AA.adjust_anchor(b)
        finally:
            torch.cuda.set_sync_debug_mode(before)
    frames = [f for f in traceback.extract_tb(err.value.__traceback__) if f.filename.endswith("anchor_adjust.py")]
    assert "info_dev.tolist()" in frames[-1].line, frames[-1].line  # exactly at the read-back
    assert_same_model(a, warm, "info supplied")
    assert b._anchor.shape[0] == N  # raised before anything was replaced


# ---- one training iteration on either side ---------------------------------------------------------------------------------
def test_densification_end_to_end_on_a_small_scene():
    from gscream_amd import anchor_adjust as A
    from gscream_amd import densify_stats as DS
    from gscream_amd import fit as FT
    from gscream_amd import gaussian_renderer as GR
    from gscream_amd import loss_utils as L
    from gscream_amd import simple_knn as KN
    from gscream_amd import standin_model as SM
    from gscream_amd import synthetic as S
    W, H, K = 160, 90, 10
    ts = FT.teacher_scene(103, 30_000, W, H, 0.6, DEV)
    cams = FT.orbit_cameras(2, W, H, 0.6, ts["means3D"].astype(np.float64).mean(0), device=DEV)
    gts, _depths = FT.render_teacher(ts, cams, DEV)
    anchors = torch.from_numpy(SM.voxelize(S.surface_point_cloud(3, 8_000, 0.6, H / W), 0.001)).float().to(DEV)
    m = SM.Model.from_pcd(anchors, torch.clamp_min(KN.distCUDA2(anchors), 0.0000001), K=K, seed=3).to(DEV)
    N0 = int(anchors.shape[0])
    # what GaussianModel has and the decode's stand-in leaves out: the remaining parameters, the fifth accumulator, the growth settings
    m._opacity, m._uncertainty = nn.Parameter(torch.zeros(N0, 1, device=DEV)), nn.Parameter(torch.zeros(N0, 1, device=DEV))
    m._rotation = nn.Parameter(m._rotation.detach().clone())
    m.uncertainty_accum = torch.zeros(N0, 1, device=DEV)
    m.voxel_size, m.update_depth, m.update_init_factor, m.update_hierachy_factor = 0.001, 3, 16, 4
    m.cat_tensors_to_optimizer = types.MethodType(Standin.cat_tensors_to_optimizer, m)
    groups = FT.adam_groups(m) + [{"params": [getattr(m, "_" + p)], "lr": 0.0, "name": p} for p in ("anchor", "opacity", "uncertainty", "rotation")]
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    bg = torch.zeros(3, device=DEV)
    m.train()

    def iteration(v, stats):
        vis, _x, _y = GR.prefilter_position2D(cams[v], m, FT._Pipe, bg)
        pkg = GR.render(cams[v], m, FT._Pipe, bg, visible_mask=vis, retain_grad=True)
        loss = L.rgb_loss(pkg["render"], gts[v], None, 0.2, 1.0)
        loss.backward()
        if stats:
            with torch.no_grad():
                DS.training_statis(m, pkg["viewspace_points"], pkg["neural_opacity"], pkg["visibility_filter"], pkg["selection_mask"], vis)
        m.optimizer.step()
        m.optimizer.zero_grad(set_to_none=True)
        return float(loss.detach()), pkg["render"].detach()
    iteration(0, True)
    assert m.anchor_demon.max() == 1 and m.offset_denom.max() == 1 and m.opacity_accum.max() > 0
    seen_before = m._offset in m.optimizer.state
    assert seen_before
    # force the statistics: every third anchor was seen 100 times and never contributed -> pruned; another third is reset only
    i = torch.arange(N0, device=DEV).view(-1, 1)
    m.anchor_demon.copy_(torch.where(i % 3 == 2, torch.zeros_like(i), torch.full_like(i, 100)).float())
    m.opacity_accum.copy_(torch.where(i % 3 == 0, torch.zeros_like(i), torch.full_like(i, 30)).float())
    m.offset_denom.mul_(60.0)
    m.offset_gradient_accum.mul_(60.0)
    old_anchor, old_feat = m._anchor.detach().clone(), m._anchor_feat.detach().clone()
    torch.manual_seed(0)
    with torch.no_grad():
        A.adjust_anchor(m, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005)
    assert A.last_path == "hip"
    N2 = int(m._anchor.shape[0])
    kept_old = int((i % 3 != 0).sum())
    assert N2 >= kept_old
    assert torch.equal(m._anchor[:kept_old].detach(), old_anchor[(i % 3 != 0).view(-1)])          # the pruned rows are gone, in order
    assert torch.equal(m._anchor_feat[:kept_old].detach(), old_feat[(i % 3 != 0).view(-1)])
    for p, w in (("anchor", (3,)), ("offset", (K, 3)), ("anchor_feat", (32,)), ("opacity", (1,)), ("uncertainty", (1,)), ("scaling", (6,)), ("rotation", (4,))):
        t = getattr(m, "_" + p)
        assert tuple(t.shape) == (N2,) + w and t.isfinite().all() and t.grad is None, p
        grp = next(g for g in m.optimizer.param_groups if g["name"] == p)
        assert grp["params"][0] is t
        st = m.optimizer.state.get(t, None)
        if st is not None:
            assert st["exp_avg"].shape == t.shape and st["exp_avg_sq"].shape == t.shape and st["exp_avg"].isfinite().all()
    assert m._offset in m.optimizer.state
    for a, n in (("anchor_demon", N2), ("opacity_accum", N2), ("uncertainty_accum", N2), ("offset_denom", N2 * K), ("offset_gradient_accum", N2 * K)):
        assert tuple(getattr(m, a).shape) == (n, 1) and getattr(m, a).isfinite().all(), a
    assert not m.anchor_demon[:kept_old][(i[(i % 3 != 0)] % 3 == 1)].any() and tuple(m.max_radii2D.shape) == (N2,)
    assert m._scaling[:, 3:].max() <= 0.05
    loss, image = iteration(1, True)   # the next iteration runs on the new N, the optimiser steps the re-keyed parameters
    assert np.isfinite(loss) and image.isfinite().all() and tuple(image.shape) == (3, H, W)
    assert m.anchor_demon.shape[0] == N2 and m.anchor_demon.max() == 1
    assert all(p.isfinite().all() for g in m.optimizer.param_groups for p in g["params"])
