"""Anchor pruning (gscream_amd.anchor_adjust): the CPU side.

tests/golden/ref_adjust_anchor.npz was recorded by running the reference's own GaussianModel.adjust_anchor
(tests/golden/make_reference_vectors6.py).  The package's torch path must reproduce it bit for bit on the CPU, with the growing
step it calls replaced by the restatement tests/test_anchor_grow.py checks against its own fixture (the HIP growing step needs a
device); that makes the torch path the ground truth the GPU tests (tests/test_gpu_anchor_adjust.py) compare the kernels with."""
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_anchor_grow import PARAMS, Standin, ref_anchor_growing, replay  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_adjust_anchor.npz")
CASES = ("mixed", "quiet", "all_pruned", "no_state", "clamp", "edges")
STATS = ("anchor_demon", "opacity_accum", "uncertainty_accum", "offset_gradient_accum", "offset_denom")
NEW_SYMBOLS = ("gsr_anchor_adjust_workspace_bytes", "gsr_anchor_adjust_offsets", "gsr_anchor_adjust_plan", "gsr_anchor_adjust_gather")


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


def adjust_args(z):
    a = z["args"]
    return dict(check_interval=int(a[0]), success_threshold=float(a[1]), grad_threshold=float(a[2]), min_opacity=float(a[3]))


def load_case(z, case, device="cpu", cls=Standin):
    """-> (stand-in model on `device`, the rand_like draws, the mlp group's parameters as they were)."""
    g = lambda k: torch.from_numpy(np.array(z[f"{case}/{k}"])).to(device)
    s = z["settings"]
    m = cls(voxel_size=float(s[0]), update_depth=int(s[2]), update_init_factor=int(s[3]), update_hierachy_factor=int(s[4]),
            n_offsets=int(z[f"{case}/offset"].shape[1]), feat_dim=int(z[f"{case}/anchor_feat"].shape[1]))
    groups = []
    for p in PARAMS:
        t = nn.Parameter(g(p).clone())
        setattr(m, "_" + p, t)
        groups.append({"params": [t], "lr": 0.01, "name": p})
    m.mlp_opacity = nn.Linear(4, 2).to(device)
    groups.append({"params": list(m.mlp_opacity.parameters()), "lr": 0.002, "name": "mlp_opacity"})
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    if f"{case}/exp_avg_anchor" in z.files:
        for grp in m.optimizer.param_groups:
            if grp["name"] in PARAMS:
                p = grp["name"]
                m.optimizer.state[grp["params"][0]] = {"step": torch.tensor(3.0), "exp_avg": g(f"exp_avg_{p}").clone(),
                                                       "exp_avg_sq": g(f"exp_avg_sq_{p}").clone()}
    for a in STATS:
        setattr(m, a, g(a).clone())
    draws = [g(f"draw{i}") for i in range(m.update_depth)]
    return m, draws, [p.detach().clone() for p in m.mlp_opacity.parameters()]


def assert_matches_fixture(z, case, model, mlp_before, expect=None):
    """Everything adjust_anchor leaves behind, bit for bit (values through expect(name, tensor) when given)."""
    N2 = int(z[f"{case}/N_after"])
    want = lambda k, name: (lambda t: expect(name, t) if expect else t)(torch.from_numpy(z[f"{case}/{k}"]))
    for p in PARAMS:
        t = getattr(model, "_" + p)
        assert isinstance(t, nn.Parameter) and t.requires_grad and t.grad is None, (case, p)
        assert t.shape[0] == N2 and torch.equal(t.detach().cpu(), want(f"out_{p}", p)), (case, p)
        grp = next(g for g in model.optimizer.param_groups if g["name"] == p)
        assert len(grp["params"]) == 1 and grp["params"][0] is t, (case, p)
        st = model.optimizer.state.get(t, None)
        if f"{case}/exp_avg_anchor" in z.files:
            assert float(st["step"]) == 3.0 and set(st) == {"step", "exp_avg", "exp_avg_sq"}
            for s in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(st[s].cpu(), torch.from_numpy(z[f"{case}/out_{s}_{p}"])), (case, p, s)
        else:
            assert st is None, (case, p)
    assert len(model.optimizer.state) == (len(PARAMS) if f"{case}/exp_avg_anchor" in z.files else 0)  # no stale keys
    for a in STATS:
        t = getattr(model, a)
        assert t.dtype == torch.float32 and torch.equal(t.cpu(), torch.from_numpy(z[f"{case}/out_{a}"])), (case, a)
    r = model.max_radii2D
    assert tuple(r.shape) == (N2,) and r.dtype == torch.float32 and not r.any() and r.device == model._anchor.device
    grp = next(g for g in model.optimizer.param_groups if g["name"] == "mlp_opacity")
    for p, q, before in zip(grp["params"], model.mlp_opacity.parameters(), mlp_before):
        assert p is q and torch.equal(p.detach(), before)


# ---- tests ----------------------------------------------------------------------------------------------------------
def test_fixture_covers_the_cases(fixture):
    z = fixture
    assert tuple(z["cases"]) == CASES
    n = lambda c, k: int(z[f"{c}/{k}"])
    N0 = lambda c: z[f"{c}/anchor"].shape[0]
    for c in CASES:
        assert n(c, "N_after") == n(c, "N_grown") - n(c, "n_prune") == z[f"{c}/out_anchor"].shape[0]
    for c in ("mixed", "no_state", "clamp", "edges"):
        assert n(c, "N_grown") > N0(c) and 0 < n(c, "n_prune") < N0(c) and n(c, "n_reset") > n(c, "n_prune")
    assert n("quiet", "n_prune") == n("quiet", "n_reset") == 0 and n("quiet", "N_after") == N0("quiet")
    assert (z["quiet/offset_denom"] > 40).any() and not z["quiet/out_offset_denom"].max() > 40  # only the offset resets
    assert n("all_pruned", "N_after") == 0 and n("all_pruned", "n_prune") == N0("all_pruned")
    assert "no_state/exp_avg_anchor" not in z.files and "mixed/exp_avg_anchor" in z.files
    tail_in, tail_out = z["clamp/scaling"][:, 3:], z["clamp/out_scaling"][:z["clamp/anchor"].shape[0], 3:]
    lim = np.float32(0.05)
    assert (tail_in == lim).any() and (tail_in == np.nextafter(lim, np.float32(1))).any() and (tail_in < lim).any() and (tail_in > 1).any()
    assert tail_out.max() == lim and (tail_out == np.nextafter(lim, np.float32(0))).any() and (tail_out < 0).any()
    d, a, o = z["edges/anchor_demon"], z["edges/opacity_accum"], z["edges/offset_denom"]
    prod = np.float32(0.005) * d
    assert (d == 80).any() and (d == 81).any() and (o == 40).any() and (o == 41).any()
    assert ((a == prod) & (d > 80)).any() and ((a == np.nextafter(prod, np.float32(-1))) & (d > 80)).any()
    assert ((z["edges/offset_gradient_accum"] == 0) & (o == 0)).any()
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("case", CASES)
def test_torch_path_replays_the_reference(fixture, case, monkeypatch):
    from gscream_amd import anchor_adjust as AA
    from gscream_amd import anchor_growing as AG
    z = fixture
    m, draws, mlp_before = load_case(z, case)
    replay(monkeypatch, draws)
    monkeypatch.setattr(AG, "anchor_growing", ref_anchor_growing)
    with torch.no_grad():
        AA.adjust_anchor(m, **adjust_args(z))
    assert AA.last_path == "torch"
    assert_matches_fixture(z, case, m, mlp_before)


def small_model(N, K=3, F=5, seed=0, state=True, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    m = Standin(n_offsets=K, feat_dim=F)
    shapes = dict(anchor=(N, 3), offset=(N, K, 3), anchor_feat=(N, F), opacity=(N, 1), uncertainty=(N, 1), scaling=(N, 6), rotation=(N, 4))
    groups = []
    for p in PARAMS:
        t = nn.Parameter((torch.randn(shapes[p], generator=g) * (0.1 if p == "scaling" else 1.0)).to(device))
        setattr(m, "_" + p, t)
        groups.append({"params": [t], "lr": 0.01, "name": p})
    m.mlp_cov = nn.Linear(3, 2).to(device)
    groups.append({"params": list(m.mlp_cov.parameters()), "lr": 0.002, "name": "mlp_cov"})
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    if state:
        for grp in m.optimizer.param_groups[:len(PARAMS)]:
            t = grp["params"][0]
            m.optimizer.state[t] = {"step": torch.tensor(7.0), "exp_avg": torch.randn(t.shape, generator=g).to(device),
                                    "exp_avg_sq": torch.rand(t.shape, generator=g).to(device)}
    m.anchor_demon = torch.randint(0, 200, (N, 1), generator=g).float().to(device)
    m.opacity_accum = (torch.rand(N, 1, generator=g) * 0.01 * m.anchor_demon.cpu()).to(device)
    m.uncertainty_accum = torch.rand(N, 1, generator=g).to(device)
    m.offset_denom = torch.randint(0, 100, (N * K, 1), generator=g).float().to(device)
    m.offset_gradient_accum = (torch.rand(N * K, 1, generator=g) * m.offset_denom.cpu()).to(device)
    return m


@pytest.mark.parametrize("state", [True, False])
def test_prune_anchor_torch_path_equals_a_row_loop(state):
    from gscream_amd import anchor_adjust as AA
    N = 37
    m = small_model(N, seed=1, state=state)
    mask = torch.rand(N, generator=torch.Generator().manual_seed(2)) < 0.4
    before = {p: getattr(m, "_" + p).detach().clone() for p in PARAMS}
    moments = {p: {s: m.optimizer.state[getattr(m, "_" + p)][s].clone() for s in ("exp_avg", "exp_avg_sq")} for p in PARAMS} if state else None
    stats = {a: getattr(m, a).clone() for a in STATS}
    with torch.no_grad():
        AA.prune_anchor(m, mask)
    assert AA.last_path == "torch"
    rows = [i for i in range(N) if not bool(mask[i])]
    assert 0 < len(rows) < N
    for p in PARAMS:
        t = getattr(m, "_" + p)
        assert t.shape[0] == len(rows) and t.grad is None and isinstance(t, nn.Parameter)
        for j, i in enumerate(rows):
            want = before[p][i].clone()
            if p == "scaling":
                for c in range(3, 6):
                    if float(want[c]) > 0.05:
                        want[c] = 0.05
            assert torch.equal(t[j].detach(), want), (p, i)
        st = m.optimizer.state.get(t, None)
        assert (st is not None) == state
        if state:
            assert float(st["step"]) == 7.0
            for s in ("exp_avg", "exp_avg_sq"):
                for j, i in enumerate(rows):
                    assert torch.equal(st[s][j], moments[p][s][i]), (p, s, i)
    assert (before["scaling"][rows][:, 3:] > 0.05).any()
    for a in STATS:  # prune_anchor alone leaves the accumulators to its caller
        assert torch.equal(getattr(m, a), stats[a])


def test_new_symbols_in_header_binding_and_library(native_lib):
    import ctypes
    from gscream_amd import _abi, _native
    hdr = _abi.header()
    for s in NEW_SYMBOLS:
        assert s in hdr.functions, s
        assert s in _native.EXPORTED_SYMBOLS, s
        assert hasattr(native_lib, s), s
    assert native_lib.gsr_anchor_adjust_workspace_bytes(1000) > 0
    assert hdr.constants["GSR_ADJUST_MAX_COPIES"] == _native.ADJUST_MAX_COPIES == 32
    assert [f for _, f, _ in hdr.structs["gsr_adjust_copy"]] == [n for n, _t in _native.AdjustCopy._fields_]
    assert ctypes.sizeof(_native.AdjustCopy) == 24
    assert [hdr.constants["GSR_ADJUST_" + m] for m in ("COPY", "CLAMP_TAIL", "OFFSET_STAT", "ANCHOR_STAT")] == [0, 1, 2, 3]
    assert (_native.ADJUST_COPY, _native.ADJUST_CLAMP_TAIL, _native.ADJUST_OFFSET_STAT, _native.ADJUST_ANCHOR_STAT) == (0, 1, 2, 3)
    assert hdr.constants["GSR_ABI_VERSION"] == 9


def test_native_argument_checks(native_lib):
    """Bad sizes and tables are refused on the host, before any launch (no device needed)."""
    from gscream_amd import _native
    L = native_lib
    assert L.gsr_anchor_adjust_offsets(-1, None, None, 1.0, None, None, None) != 0
    assert L.gsr_anchor_adjust_plan(-1, None, None, None, 0.005, 80.0, None, None, None, None, None) != 0
    assert L.gsr_anchor_adjust_plan(5, None, None, None, 0.005, 80.0, None, None, None, None, None) != 0
    assert b"NULL" in L.gsr_last_error()
    t = (_native.AdjustCopy * 1)()
    t[0].src, t[0].dst, t[0].width, t[0].mode = 256, 512, 0, 0
    assert L.gsr_anchor_adjust_gather(10, 5, 1, t, 1024, None, 0, None, None) != 0 and b"width" in L.gsr_last_error()
    t[0].width, t[0].mode = 3, 7
    assert L.gsr_anchor_adjust_gather(10, 5, 1, t, 1024, None, 0, None, None) != 0
    t[0].mode = 0
    assert L.gsr_anchor_adjust_gather(10, 11, 1, t, 1024, None, 0, None, None) != 0      # n_keep > N
    assert L.gsr_anchor_adjust_gather(10, 5, 33, t, 1024, None, 0, None, None) != 0      # more copies than the table holds
    t[0].mode, t[0].width = 3, 2
    assert L.gsr_anchor_adjust_gather(10, 5, 1, t, 1024, None, 0, 2048, None) != 0       # ANCHOR_STAT is one column
    assert L.gsr_anchor_adjust_gather(10, 0, 1, t, 1024, None, 0, None, None) == 0       # nothing kept: nothing to do


def test_mismatched_shapes_raise_value_error():
    from gscream_amd import anchor_adjust as AA
    for name, n in (("opacity_accum", 36), ("anchor_demon", 38), ("uncertainty_accum", 1), ("offset_denom", 37 * 3 - 1),
                    ("offset_gradient_accum", 37 * 3 + 3)):
        m = small_model(37, seed=3)
        setattr(m, name, torch.zeros(n, 1))
        with pytest.raises(ValueError, match=name), torch.no_grad():
            AA.adjust_anchor(m)
        assert m._anchor.shape[0] == 37
    m = small_model(37, seed=3)
    m.optimizer.param_groups[2]["params"][0] = nn.Parameter(torch.zeros(36, 5))
    with pytest.raises(ValueError, match="anchor_feat"), torch.no_grad():
        AA.adjust_anchor(m)
    m = small_model(37, seed=3)
    with pytest.raises(ValueError, match="mask"), torch.no_grad():
        AA.prune_anchor(m, torch.zeros(36, dtype=torch.bool))


def test_zero_anchors_on_the_torch_path(monkeypatch):
    from gscream_amd import anchor_adjust as AA
    from gscream_amd import anchor_growing as AG
    monkeypatch.setattr(AG, "anchor_growing", lambda *a: None)
    m = small_model(0, seed=4)
    leaf = m._anchor
    with torch.no_grad():
        AA.adjust_anchor(m)
    assert m._anchor is leaf and tuple(m.offset_denom.shape) == (0, 1) and tuple(m.max_radii2D.shape) == (0,)
