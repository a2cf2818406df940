"""Anchor growing (gscream_amd.anchor_growing) and the torch_scatter drop-in: the CPU side.

tests/golden/ref_anchor_grow.npz was recorded by running the reference's own GaussianModel.anchor_growing
(tests/golden/make_reference_vectors5.py).  This file restates the reference's per-level expressions
(scene/gaussian_model.py:829-874) and the method around them in torch; the restatement must reproduce the fixture exactly on
the CPU, which makes it the ground truth the GPU tests (tests/test_gpu_anchor_grow.py) run on the device."""
import os
import sys
import types
from functools import reduce

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "ref_anchor_grow.npz")
PARAMS = ("anchor", "offset", "anchor_feat", "opacity", "uncertainty", "scaling", "rotation")
ACCUMS = ("anchor_demon", "opacity_accum", "uncertainty_accum")
NEW_SYMBOLS = ("gsr_anchor_grow_workspace_bytes", "gsr_anchor_grow_keys", "gsr_anchor_grow_emit", "gsr_scatter_max")


# ---- the restatement ------------------------------------------------------------------------------------------------
def ref_level(anchor, offset, scaling, anchor_feat, candidate_mask, cur_size):
    """scene/gaussian_model.py:829-874 for one level: -> (candidate_anchor, new_feat).  scaling = the activated get_scaling."""
    N, K, F = anchor.shape[0], offset.shape[1], anchor_feat.shape[1]
    mask = candidate_mask.reshape(-1).bool()
    if mask.numel() < N * K:
        mask = torch.cat([mask, torch.zeros(N * K - mask.numel(), dtype=torch.bool, device=mask.device)])
    all_xyz = anchor.unsqueeze(dim=1) + offset * scaling[:, :3].unsqueeze(dim=1)
    grid_coords = torch.round(anchor / cur_size).int()
    sel = torch.round(all_xyz.view([-1, 3])[mask] / cur_size).int()
    uniq, inverse = torch.unique(sel, return_inverse=True, dim=0)
    chunks = [(uniq.unsqueeze(1) == grid_coords[j:j + 4096, :]).all(-1).any(-1).view(-1) for j in range(0, N, 4096)]
    keep = ~reduce(torch.logical_or, chunks)
    candidate_anchor = uniq[keep] * cur_size
    feat = anchor_feat.unsqueeze(dim=1).repeat([1, K, 1]).view([-1, F])[mask]
    idx = inverse.unsqueeze(1).expand(-1, F)
    new_feat = feat.new_zeros((uniq.shape[0], F)).scatter_reduce(0, idx, feat, "amax", include_self=False)[keep]
    return candidate_anchor, new_feat


class Standin(types.SimpleNamespace):
    """What GaussianModel.anchor_growing reads from `self` (get_anchor :269-270, get_scaling :241-242)."""
    get_anchor = property(lambda self: self._anchor)
    get_scaling = property(lambda self: 1.0 * torch.exp(self._scaling))

    def cat_tensors_to_optimizer(self, tensors_dict):  # scene/gaussian_model.py:705-725
        out = {}
        for group in self.optimizer.param_groups:
            if "mlp" in group["name"] or "conv" in group["name"] or "feat_base" in group["name"]:
                continue
            ext = tensors_dict[group["name"]]
            st = self.optimizer.state.get(group["params"][0], None)
            if st is not None:
                st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0)
                st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
                del self.optimizer.state[group["params"][0]]
                group["params"][0] = nn.Parameter(torch.cat((group["params"][0], ext), dim=0).requires_grad_(True))
                self.optimizer.state[group["params"][0]] = st
            else:
                group["params"][0] = nn.Parameter(torch.cat((group["params"][0], ext), dim=0).requires_grad_(True))
            out[group["name"]] = group["params"][0]
        return out


def load_case(z, case, device="cpu"):
    """-> (stand-in model on `device`, grads, offset_mask, draws) from the fixture's inputs."""
    g = lambda k: torch.from_numpy(np.array(z[f"{case}/{k}"])).to(device)
    s = z["settings"]
    m = Standin(voxel_size=float(s[0]), update_depth=int(s[2]), update_init_factor=int(s[3]), update_hierachy_factor=int(s[4]),
                n_offsets=int(z[f"{case}/offset"].shape[1]), feat_dim=int(z[f"{case}/anchor_feat"].shape[1]))
    groups = []
    for p in PARAMS:
        t = nn.Parameter(g(p).clone())
        setattr(m, "_" + p, t)
        groups.append({"params": [t], "lr": 0.01, "name": p})
    m.mlp_opacity = nn.Linear(4, 2).to(device)
    groups.append({"params": list(m.mlp_opacity.parameters()), "lr": 0.002, "name": "mlp_opacity"})
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for grp in m.optimizer.param_groups:
        if grp["name"] in PARAMS:
            p = grp["name"]
            m.optimizer.state[grp["params"][0]] = {"step": torch.tensor(3.0), "exp_avg": g(f"exp_avg_{p}").clone(),
                                                   "exp_avg_sq": g(f"exp_avg_sq_{p}").clone()}
    for a in ACCUMS:
        setattr(m, a, g(a).clone())
    draws = [g(f"draw{i}") for i in range(m.update_depth)]
    return m, g("grads"), g("offset_mask"), draws


def ref_anchor_growing(model, grads, threshold, offset_mask, level=ref_level):
    """GaussianModel.anchor_growing (:808-900) around `level`."""
    init_length = model.get_anchor.shape[0] * model.n_offsets
    for i in range(model.update_depth):
        cand = torch.logical_and(grads >= threshold * ((model.update_hierachy_factor // 2) ** i), offset_mask)
        cand = torch.logical_and(cand, torch.rand_like(cand.float()) > (0.5 ** (i + 1)))
        if model.get_anchor.shape[0] * model.n_offsets - init_length == 0 and i > 0:
            continue
        cur_size = model.voxel_size * (model.update_init_factor // (model.update_hierachy_factor ** i))
        with torch.no_grad():
            anchor, feat = level(model.get_anchor, model._offset, model.get_scaling, model._anchor_feat, cand, cur_size)
        if anchor.shape[0] == 0:
            continue
        C, dev = anchor.shape[0], anchor.device
        d = {"anchor": anchor, "scaling": torch.log(torch.ones_like(anchor).repeat([1, 2]) * cur_size),
             "rotation": torch.zeros([C, 4], device=dev), "anchor_feat": feat,
             "offset": torch.zeros([C, model.n_offsets, 3], device=dev),
             "opacity": torch.log(0.1 * torch.ones((C, 1), device=dev) / (1 - 0.1 * torch.ones((C, 1), device=dev))),
             "uncertainty": torch.log(0.1 * torch.ones((C, 1), device=dev) / (1 - 0.1 * torch.ones((C, 1), device=dev)))}
        d["rotation"][:, 0] = 1.0
        for a in ACCUMS:
            setattr(model, a, torch.cat([getattr(model, a), torch.zeros([C, 1], device=dev)], dim=0))
        for k, v in model.cat_tensors_to_optimizer(d).items():
            setattr(model, "_" + k, v)


def replay(monkeypatch, draws):
    """torch.rand_like returns the fixture's draws, one per level, in order."""
    it = iter(draws)

    def rand_like(t, **kw):
        d = next(it)
        assert tuple(d.shape) == tuple(t.shape) and d.device == t.device
        return d.clone()
    monkeypatch.setattr(torch, "rand_like", rand_like)


def assert_matches_fixture(z, case, model, expect=None):
    """Every parameter, optimiser state and accumulator: the rows the model had are unchanged, the new rows are the fixture's
    (passed through expect(name, tensor) when given)."""
    N0 = z[f"{case}/anchor"].shape[0]
    N1 = int(z[f"{case}/N_after"])
    for p in PARAMS:
        t = getattr(model, "_" + p).detach().cpu()
        assert t.shape[0] == N1, (case, p, t.shape)
        assert torch.equal(t[:N0], torch.from_numpy(z[f"{case}/{p}"])), (case, p)
        want = torch.from_numpy(z[f"{case}/out_{p}"])
        assert torch.equal(t[N0:], expect(p, want) if expect else want), (case, p, "new rows")
        grp = next(g for g in model.optimizer.param_groups if g["name"] == p)
        assert grp["params"][0] is getattr(model, "_" + p)
        st = model.optimizer.state[grp["params"][0]]
        for s in ("exp_avg", "exp_avg_sq"):
            v = st[s].cpu()
            assert v.shape == t.shape and torch.equal(v[:N0], torch.from_numpy(z[f"{case}/{s}_{p}"])) and not v[N0:].any(), (case, p, s)
    for a in ACCUMS:
        t = getattr(model, a).cpu()
        assert t.shape == (N1, 1) and torch.equal(t[:N0], torch.from_numpy(z[f"{case}/{a}"])) and not t[N0:].any(), (case, a)


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


# ---- tests ----------------------------------------------------------------------------------------------------------
def test_fixture_covers_the_cases(fixture):
    z = fixture
    assert list(z["cases"]) == ["grow", "none", "ties", "occupied", "onecell"]
    assert int(z["none/N_after"]) == z["none/anchor"].shape[0]  # level 0 adds nothing, the later levels are skipped
    for c in ("grow", "ties", "occupied", "onecell"):
        assert int(z[f"{c}/N_after"]) > z[f"{c}/anchor"].shape[0]
    assert os.path.getsize(FIXTURE) < 1 << 20


@pytest.mark.parametrize("case", ["grow", "none", "ties", "occupied", "onecell"])
def test_restatement_reproduces_the_reference(fixture, case, monkeypatch):
    z = fixture
    m, grads, offset_mask, draws = load_case(z, case)
    replay(monkeypatch, draws)
    ref_anchor_growing(m, grads, float(z["settings"][1]), offset_mask)
    assert_matches_fixture(z, case, m)


def test_tie_case_has_ties(fixture):
    """The "ties" case really puts candidates on half-cell ties, of both signs, at level 0."""
    z = fixture
    a, o = z["ties/anchor"].astype(np.float64), z["ties/offset"].astype(np.float64)
    q = (a[:, None, :] + o) / (z["settings"][0] * 16)
    frac = q - np.floor(q)
    assert (frac == 0.5).sum() > 100 and ((frac == 0.5) & (q < 0)).any() and ((frac == 0.5) & (q > 0)).any()


def test_torch_scatter_resolves_to_the_drop_in():
    import torch_scatter
    from torch_scatter import scatter_max
    from gscream_amd import scatter as S
    assert scatter_max is S.scatter_max
    assert os.path.dirname(os.path.abspath(torch_scatter.__file__)) == os.path.join(ROOT, "torch_scatter")


def test_scatter_max_torch_path_contract():
    """The exact torch path (here: CPU tensors): values = scatter_reduce amax, empty slots 0 / argmax = src.size(dim), ties ->
    the smallest source position, dim_size, a 1-D index along dim 0 of a 2-D src, and dim = -1."""
    from torch_scatter import scatter_max
    src = torch.tensor([[1.0, 5.0], [3.0, 5.0], [3.0, -1.0], [0.5, 7.0]])
    idx = torch.tensor([0, 0, 0, 2])
    out, arg = scatter_max(src, idx.unsqueeze(1).expand(-1, 2), dim=0, dim_size=4)
    assert torch.equal(out, torch.tensor([[3.0, 5.0], [0.0, 0.0], [0.5, 7.0], [0.0, 0.0]]))
    assert torch.equal(arg, torch.tensor([[1, 0], [4, 4], [3, 3], [4, 4]]))
    out1, arg1 = scatter_max(src, idx, dim=0)
    assert torch.equal(out1, out[:3]) and torch.equal(arg1, arg[:3])
    x = torch.tensor([[2.0, -3.0, 2.0, -4.0]])
    o, a = scatter_max(x, torch.tensor([[1, 1, 1, 0]]))
    assert torch.equal(o, torch.tensor([[-4.0, 2.0]])) and torch.equal(a, torch.tensor([[3, 0]]))


def test_new_symbols_in_header_binding_and_library(native_lib):
    from gscream_amd import _abi, _native
    for s in NEW_SYMBOLS:
        assert s in _abi.header().functions, s
        assert s in _native.EXPORTED_SYMBOLS, s
        assert hasattr(native_lib, s), s
    assert native_lib.gsr_anchor_grow_workspace_bytes(1000, 10000) > 0


def test_grow_level_refuses_cpu_tensors(native_lib):
    from gscream_amd import anchor_growing as AG
    with pytest.raises(RuntimeError, match="HIP device"):
        AG.grow_level(torch.zeros(2, 3), torch.zeros(2, 10, 3), torch.ones(2, 6), torch.zeros(2, 32), torch.ones(20, dtype=torch.bool), 0.08)
