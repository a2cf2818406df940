"""Anchor growing and scatter_max on the HIP path, bit-exact (torch.equal, no tolerances).

* gscream_amd.anchor_growing.anchor_growing on a stand-in replays tests/golden/ref_anchor_grow.npz (the reference's own
  method, recorded on the CPU with power-of-two cell sizes) with the fixture's torch.rand_like draws;
* grow_level against the restated reference expressions (tests/test_anchor_grow.ref_level) run on the same device, at
  GScream's cell sizes 0.005 x {16, 4, 1}, for random scenes of 1 .. 300k anchors, empty masks, all-duplicate levels, ties and
  coordinates beyond the keys' +-2^20 cells (the torch fallback);
* scatter_max against scatter_reduce("amax"), with the argmax contract of gscream_amd/scatter.py."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_anchor_grow import FIXTURE, Standin, assert_matches_fixture, load_case, ref_level, replay  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [0.005 * f for f in (16, 4, 1)]  # run.py: voxel_size 0.005, update_init_factor 16, update_hierachy_factor 4


@pytest.fixture
def hip_only(monkeypatch):
    """grow_level must not take the torch fallback in these tests."""
    from gscream_amd import anchor_growing as AG

    def no_fallback(*a, **k):
        raise AssertionError("grow_level fell back to the torch expressions")
    monkeypatch.setattr(AG, "reference_level", no_fallback)
    return AG


def scene(N, K=10, F=32, seed=0, extent=10.0, offset_sd=1.0, p=0.1, L=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    anchor = torch.round((torch.rand(N, 3, generator=g) * 2 - 1) * extent / 0.005) * 0.005   # voxelised like create_from_pcd
    offset = torch.randn(N, K, 3, generator=g) * offset_sd
    scaling = torch.exp(torch.randn(N, 6, generator=g) * 0.5 - 3.5)
    feat = torch.randn(N, F, generator=g)
    mask = torch.rand((L if L is not None else N * K), generator=g) < p
    return [t.to(DEV) for t in (anchor.float(), offset, scaling, feat, mask)]


def check_level(AG, args, cur_size):
    got = AG.grow_level(*args, cur_size)
    want = ref_level(*args, cur_size)
    for a, b, what in ((got[0], want[0], "candidate_anchor"), (got[1], want[1], "new_feat")):
        assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
        assert a.dtype == b.dtype and torch.equal(a, b), what
    return int(got[0].shape[0])


class HostExpStandin(Standin):
    """The stand-in with its scaling activation evaluated on the host: the fixture was recorded with the CPU's expf, which
    differs from the device's in the last bit for some inputs, and the activation is an INPUT of the growth step."""
    get_scaling = property(lambda self: (1.0 * torch.exp(self._scaling.detach().cpu())).to(self._scaling.device))


def device_constants(z):
    """The new rows' constants -- log(cur_size) (scaling) and inverse_sigmoid(0.1) (opacity, uncertainty) -- are computed by the
    growth step itself, on the device: map each CPU value in the fixture to the device's value of the same expression."""
    s = z["settings"]
    pairs = {"scaling": [], "opacity": [], "uncertainty": []}
    for f in (16, 4, 1):
        c = float(s[0]) * f
        pairs["scaling"].append(tuple(torch.log(torch.ones(1, device=d) * c).cpu() for d in ("cpu", DEV)))
    for k in ("opacity", "uncertainty"):
        pairs[k].append(tuple(torch.log(0.1 * torch.ones(1, device=d) / (1 - 0.1 * torch.ones(1, device=d))).cpu() for d in ("cpu", DEV)))

    def expect(name, want):
        want = want.clone()
        for cpu_v, dev_v in pairs.get(name, []):
            want[want == cpu_v] = dev_v
        return want
    return expect


@pytest.mark.parametrize("case", ["grow", "none", "ties", "occupied", "onecell"])
def test_anchor_growing_replays_the_reference(case, monkeypatch, hip_only):
    z = np.load(FIXTURE)
    m, grads, offset_mask, draws = load_case(z, case, DEV)
    m.__class__ = HostExpStandin
    replay(monkeypatch, draws)
    hip_only.anchor_growing(m, grads, float(z["settings"][1]), offset_mask)
    assert_matches_fixture(z, case, m, device_constants(z))


def test_division_by_a_python_scalar_is_a_reciprocal_multiply():
    """What grow_level relies on (and what makes true division the wrong model on the device): x / s with a Python float s is
    x * (1.0f / float(s)) in PyTorch's GPU kernel, checked on values where the two differ."""
    x = torch.randn(1 << 20, device=DEV) * 30
    for s in SIZES:
        inv = np.float32(1.0) / np.float32(s)
        assert torch.equal(x / s, x * float(inv))
    assert not torch.equal((x.double() / np.float32(SIZES[2])).float(), x * float(np.float32(1.0) / np.float32(SIZES[2])))


@pytest.mark.parametrize("N", [1, 7, 1000, 30000, 300000])
def test_grow_level_random_scenes(N, hip_only):
    args = scene(N, seed=N, p=0.1 if N > 1 else 1.0)
    added = [check_level(hip_only, args, s) for s in SIZES]
    if N >= 1000:
        assert min(added) > 0


def test_grow_level_later_level_shapes(hip_only):
    """A level after growth: the model has N > N0 anchors and the mask covers the first N0 * K rows only."""
    args = scene(5000, seed=3, L=4000 * 10, p=0.3)
    for s in SIZES:
        check_level(hip_only, args, s)


def test_grow_level_empty_and_all_duplicate(hip_only):
    anchor, offset, scaling, feat, mask = scene(2000, seed=4)
    for s in SIZES:
        assert check_level(hip_only, (anchor, offset, scaling, feat, torch.zeros_like(mask)), s) == 0
        # zero offsets: every candidate sits in its own anchor's cell
        assert check_level(hip_only, (anchor, torch.zeros_like(offset), scaling, feat, torch.ones_like(mask)), s) == 0
        # small offsets at the coarse level: most candidates are duplicates, a few are not
        check_level(hip_only, (anchor, offset * 0.02, scaling, feat, torch.ones_like(mask)), s)


def test_grow_level_ties_and_crowded_cells(hip_only):
    g = torch.Generator().manual_seed(5)
    N, K = 3000, 10
    for s in SIZES + [2.0 ** -4]:
        s32 = float(np.float32(s))
        anchor = (torch.randint(-50, 50, (N, 3), generator=g).float() * s32).to(DEV)
        # offsets of odd multiples of half a cell, scale 1: candidates on or within one rounding of the half-cell ties
        offset = ((torch.randint(-20, 20, (N, K, 3), generator=g) * 2 + 1).float() * (0.5 * s32)).to(DEV)
        ones = torch.ones(N, 6, device=DEV)
        feat = torch.randn(N, 32, generator=g).to(DEV)
        check_level(hip_only, (anchor, offset, ones, feat, torch.ones(N * K, dtype=torch.bool, device=DEV)), s)
        # thousands of candidates in a handful of cells
        crowd = (-anchor[:, None, :] + torch.rand(N, K, 3, generator=g).to(DEV) * (2 * s32)).contiguous()
        check_level(hip_only, (anchor, crowd, ones, feat, torch.ones(N * K, dtype=torch.bool, device=DEV)), s)


def test_grow_level_beyond_the_key_range_falls_back(monkeypatch):
    from gscream_amd import anchor_growing as AG
    calls = []
    real = AG.reference_level
    monkeypatch.setattr(AG, "reference_level", lambda *a: calls.append(1) or real(*a))
    anchor, offset, scaling, feat, mask = scene(3000, seed=6)
    far = anchor.clone()
    far[::7] *= 2000.0  # |x| up to 2e4: cells of 0.005 reach 4e6 > 2^20
    check_level(AG, (far, offset, scaling, feat, mask), SIZES[2])
    assert len(calls) == 1
    check_level(AG, (far, offset, scaling, feat, mask), SIZES[0])  # cells of 0.08: in range again
    assert len(calls) == 1


# ---- scatter_max ----------------------------------------------------------------------------------------------------
def _scatter_ref(src, index, S):
    """amax + the smallest source row holding it; empty slots 0 / argmax R (torch on the device)."""
    R = src.shape[0]
    idx = index.view(-1, *([1] * (src.dim() - 1))).expand_as(src)
    out = src.new_zeros((S,) + tuple(src.shape[1:])).scatter_reduce(0, idx, src, "amax", include_self=False)
    pos = torch.arange(R, device=src.device).view(-1, *([1] * (src.dim() - 1))).expand_as(src)
    hit = src == out.gather(0, idx)
    arg = torch.full(out.shape, R, dtype=torch.long, device=src.device).scatter_reduce(
        0, idx, torch.where(hit, pos, torch.full_like(pos, R)), "amin", include_self=True)
    return out, arg


@pytest.mark.parametrize("R,F,S", [(1, 32, 1), (1000, 32, 50), (100000, 32, 20000), (5000, 1, 7), (3000, 5, 6000)])
def test_scatter_max_hip_path(R, F, S, monkeypatch):
    from gscream_amd import scatter as SC
    from torch_scatter import scatter_max
    monkeypatch.setattr(SC, "_torch_scatter_max", lambda *a: (_ for _ in ()).throw(AssertionError("took the torch path")))
    g = torch.Generator().manual_seed(R + S)
    src = (torch.randint(-40, 40, (R, F), generator=g).float() / 8).to(DEV)  # coarse values: many ties
    index = torch.randint(0, S, (R,), generator=g).to(DEV)
    want, warg = _scatter_ref(src, index, S)
    out, arg = scatter_max(src, index.unsqueeze(1).expand(-1, F), dim=0, dim_size=S)  # gaussian_model.py:874's form
    assert torch.equal(out, want) and torch.equal(arg, warg)
    out, arg = scatter_max(src, index, dim=0, dim_size=S + 3)  # 1-D index, extra empty slots
    assert out.shape == (S + 3, F) and not out[S:].any() and (arg[S:] == R).all()
    assert torch.equal(out[:S], want) and torch.equal(arg[:S], warg)
    if F == 1:
        o1, a1 = scatter_max(src[:, 0], index, dim=0, dim_size=S)
        assert torch.equal(o1, want[:, 0]) and torch.equal(a1, warg[:, 0])
    o2, a2 = scatter_max(src, index.unsqueeze(1).expand(-1, F), dim=0)  # dim_size = index.max() + 1
    S2 = int(index.max()) + 1
    assert torch.equal(o2, want[:S2]) and torch.equal(a2, warg[:S2])


def test_scatter_max_other_forms_take_the_exact_torch_path():
    from torch_scatter import scatter_max
    g = torch.Generator().manual_seed(9)
    src = torch.randn(40, 6, 3, generator=g).to(DEV)
    idx = torch.randint(0, 4, (40, 6, 3), generator=g).to(DEV)
    out, arg = scatter_max(src, idx, dim=1, dim_size=5)
    ref = torch.zeros(40, 5, 3, device=DEV).scatter_reduce(1, idx, src, "amax", include_self=False)
    assert torch.equal(out, ref)
    hit = arg < src.shape[1]  # argmax src.size(dim) = an empty slot
    picked = src.gather(1, arg.clamp(max=src.shape[1] - 1))
    assert torch.equal(torch.where(hit, picked, torch.zeros_like(picked)), out) and not out[~hit].any()
    src64 = torch.randn(100, 4, generator=g, dtype=torch.float64).to(DEV)
    i64 = torch.randint(0, 9, (100,), generator=g).to(DEV)
    o64, a64 = scatter_max(src64, i64, dim=0, dim_size=9)
    w64, wa64 = _scatter_ref(src64, i64, 9)
    assert o64.dtype == torch.float64 and torch.equal(o64, w64) and torch.equal(a64, wa64)
