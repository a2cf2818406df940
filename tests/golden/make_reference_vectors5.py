"""Golden vectors for anchor growing, produced by RUNNING the reference's own GaussianModel.anchor_growing.

    python tests/golden/make_reference_vectors5.py        # needs /root/reference; runs on the CPU

scene/gaussian_model.py is imported in place (make_reference_vectors2.import_reference: stubs for the modules the method never
touches); `GaussianModel.anchor_growing` (:808-900) and `GaussianModel.cat_tensors_to_optimizer` (:705-725) are called
unbound on a stand-in namespace that carries the seeded parameters, the densification accumulators and a real
torch.optim.Adam whose parameter groups are named like the reference's (training_setup, :376-390; one "mlp_*" group shows the
skip).  Nothing of the reference is copied: only inputs and the tensors it left behind are stored (ref_anchor_grow.npz).

Three redirections, none of which touches the reference's arithmetic:
  * `.cuda()` and `device='cuda'` (torch.zeros / torch.ones) stay on the CPU, as make_reference_vectors2 does for torch.zeros;
  * `scatter_max` (torch_scatter, :20) is a CPU restatement through torch.scatter_reduce("amax"): a maximum is exact in any
    order, so the values are the ones torch_scatter computes (the method reads only [0] of its result);
  * `torch.rand_like` returns seeded draws and records them (uniform on multiples of 1/256, which store compactly).
Cell sizes are powers of two (voxel_size 2^-8; factors 16, 4, 1), so that x / cur_size is exact and the GPU's
multiplication by the reciprocal agrees with the CPU's true division bit for bit.  The raw scalings are chosen so that
exp() of them lies well away from a rounding midpoint (CPU and GPU exp then agree), and the constants the method takes a log
of are checked the same way.

Cases: "grow" (three levels that all add anchors), "none" (level 0 adds nothing: levels 1 and 2 draw and are skipped),
"ties" (candidates exactly on half-cell ties, positive and negative), "occupied" (most candidates land in anchors' cells),
"onecell" (hundreds of candidates in one empty cell).  Per case, prefix "<case>/": the inputs, draw<i> per level, and
out_<name> = the rows each tensor gained (the generator checks that the rows it had are unchanged).
"""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

K, F = 10, 32
VOXEL = 2.0 ** -8
PARAMS = ("anchor", "offset", "anchor_feat", "opacity", "uncertainty", "scaling", "rotation")
ACCUMS = ("anchor_demon", "opacity_accum", "uncertainty_accum")
SETTINGS = dict(voxel_size=VOXEL, update_depth=3, update_init_factor=16, update_hierachy_factor=4, n_offsets=K, feat_dim=F)
THRESHOLD = 0.0002


def _midpoint_margin(x32):
    """Distance of exp(x) (float64) from the nearest float32 rounding midpoint, in float32 ulps (0.5 = exactly representable)."""
    e = np.exp(x32.astype(np.float64))
    f = e.astype(np.float32)
    ulp = np.spacing(np.abs(f)).astype(np.float64)
    return 0.5 - np.abs(e - f.astype(np.float64)) / ulp


def _scalings(rng, shape):
    """Raw scalings in log(0.02) .. log(0.2) whose exp is >= 0.2 ulp away from a rounding midpoint."""
    x = np.log(rng.uniform(0.02, 0.2, size=shape)).astype(np.float32)
    bad = _midpoint_margin(x) < 0.2
    while bad.any():
        x[bad] = np.log(rng.uniform(0.02, 0.2, size=int(bad.sum()))).astype(np.float32)
        bad = _midpoint_margin(x) < 0.2
    return x


def case_inputs(name, seed):
    rng = np.random.default_rng(seed)
    q = lambda a, step: (np.round(np.asarray(a) / step) * step).astype(np.float32)
    if name == "grow":
        N = 400
        anchor = q(rng.uniform(-1.5, 1.5, (N, 3)), VOXEL)
        offset = q(rng.normal(0, 2.0, (N, K, 3)), 2 ** -10)
        scaling = _scalings(rng, (N, 6))
        grads = q(rng.uniform(0, 5 * THRESHOLD, N * K), THRESHOLD / 16)
    elif name == "none":
        N = 200
        anchor = q(rng.uniform(-1, 1, (N, 3)), VOXEL)
        offset = q(rng.normal(0, 1.0, (N, K, 3)), 2 ** -10)
        scaling = _scalings(rng, (N, 6))
        grads = q(rng.uniform(0, 0.9 * THRESHOLD, N * K), THRESHOLD / 64)  # below the level-0 threshold everywhere
    elif name == "ties":
        N = 200
        anchor = q(rng.uniform(-0.5, 0.5, (N, 3)), 16 * VOXEL)
        # offsets on half-cell ties (scale 1): odd multiples of half a cell of level 0 (16 voxels) or of level 2 (1 voxel)
        half = np.where(rng.random((N, K, 1)) < 0.5, 8 * VOXEL, 0.5 * VOXEL)
        offset = (rng.integers(-6, 6, (N, K, 3)) * 2 + 1).astype(np.float32) * half.astype(np.float32)
        scaling = np.zeros((N, 6), np.float32)
        grads = q(rng.uniform(THRESHOLD, 8 * THRESHOLD, N * K), THRESHOLD / 16)
    elif name == "occupied":
        N = 300
        anchor = q(rng.uniform(-0.6, 0.6, (N, 3)), VOXEL)
        offset = q(rng.normal(0, 0.04, (N, K, 3)), 2 ** -10)
        scaling = _scalings(rng, (N, 6))
        grads = q(rng.uniform(THRESHOLD, 8 * THRESHOLD, N * K), THRESHOLD / 16)
    elif name == "onecell":
        N = 300
        d = rng.normal(size=(N, 3))
        anchor = q(d / np.linalg.norm(d, axis=1, keepdims=True) * 0.4, VOXEL)  # a shell around an empty coarse cell
        offset = q(-anchor[:, None, :] + rng.uniform(-0.02, 0.02, (N, K, 3)), 2 ** -12)  # scale 1: every candidate near 0
        scaling = np.zeros((N, 6), np.float32)
        grads = q(rng.uniform(THRESHOLD, 8 * THRESHOLD, N * K), THRESHOLD / 16)
    else:
        raise ValueError(name)
    inp = dict(
        anchor=anchor, offset=offset.astype(np.float32), scaling=scaling,
        anchor_feat=q(np.clip(rng.normal(0, 1, (N, F)), -2, 2), 2 ** -3),
        opacity=q(rng.normal(0, 1, (N, 1)), 2 ** -8), uncertainty=q(rng.normal(0, 1, (N, 1)), 2 ** -8),
        rotation=q(rng.normal(0, 1, (N, 4)), 2 ** -8),
        grads=grads.astype(np.float32), offset_mask=rng.random(N * K) < (0.6 if name == "grow" else 0.85),
        anchor_demon=rng.integers(0, 200, (N, 1)).astype(np.float32), opacity_accum=q(rng.uniform(0, 50, (N, 1)), 2 ** -4),
        uncertainty_accum=q(rng.uniform(0, 50, (N, 1)), 2 ** -4))
    for p in PARAMS:
        sh = inp[p].shape
        inp[f"exp_avg_{p}"] = (rng.integers(-8, 8, sh) * 2.0 ** -12).astype(np.float32)
        inp[f"exp_avg_sq_{p}"] = (rng.integers(0, 8, sh) * 2.0 ** -20).astype(np.float32)
    return inp


class Standin(types.SimpleNamespace):
    """What GaussianModel.anchor_growing reads: the parameters, get_anchor / get_scaling (:269-270, :241-242), the growth
    settings, the accumulators and the optimiser."""
    get_anchor = property(lambda self: self._anchor)
    get_scaling = property(lambda self: 1.0 * torch.exp(self._scaling))


def make_standin(inp, cat_tensors_to_optimizer):
    m = Standin(**SETTINGS)
    groups = []
    for p in PARAMS:
        t = nn.Parameter(torch.from_numpy(inp[p].copy()).requires_grad_(True))
        setattr(m, "_" + p, t)
        groups.append({"params": [t], "lr": 0.01, "name": p})
    m.mlp_opacity = nn.Linear(F + 4, K)
    groups.append({"params": m.mlp_opacity.parameters(), "lr": 0.002, "name": "mlp_opacity"})
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for g in m.optimizer.param_groups:
        if g["name"] in PARAMS:
            p = g["name"]
            m.optimizer.state[g["params"][0]] = {"step": torch.tensor(3.0), "exp_avg": torch.from_numpy(inp[f"exp_avg_{p}"].copy()),
                                                 "exp_avg_sq": torch.from_numpy(inp[f"exp_avg_sq_{p}"].copy())}
    for a in ACCUMS:
        setattr(m, a, torch.from_numpy(inp[a].copy()))
    m.cat_tensors_to_optimizer = types.MethodType(cat_tensors_to_optimizer, m)
    return m


def state_of(m, p):
    g = next(g for g in m.optimizer.param_groups if g["name"] == p)
    return m.optimizer.state[g["params"][0]]


def cpu_scatter_max(src, index, dim=-1, out=None, dim_size=None):
    assert out is None and dim_size is None and dim == 0
    size = (int(index.max()) + 1 if index.numel() else 0,) + tuple(src.shape[1:])
    return src.new_zeros(size).scatter_reduce(0, index, src, "amax", include_self=False), None


def run_case(GM, name, seed):
    inp = case_inputs(name, seed)
    m = make_standin(inp, GM.GaussianModel.cat_tensors_to_optimizer)
    gen = torch.Generator().manual_seed(seed)
    draws = []

    def rand_like(t, **kw):
        d = torch.randint(0, 256, t.shape, generator=gen).float() / 256.0
        draws.append(d.numpy().copy())
        return d

    real = dict(zeros=torch.zeros, ones=torch.ones, rand_like=torch.rand_like, cuda=torch.Tensor.cuda, empty_cache=torch.cuda.empty_cache)
    drop_cuda = lambda fn: (lambda *a, **k: fn(*a, **{kk: v for kk, v in k.items() if not (kk == "device" and str(v).startswith("cuda"))}))
    torch.zeros, torch.ones, torch.rand_like = drop_cuda(real["zeros"]), drop_cuda(real["ones"]), rand_like
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.empty_cache = lambda: None
    GM.scatter_max = cpu_scatter_max
    try:
        with torch.no_grad():
            GM.GaussianModel.anchor_growing(m, torch.from_numpy(inp["grads"]), THRESHOLD, torch.from_numpy(inp["offset_mask"]))
    finally:
        torch.zeros, torch.ones, torch.rand_like = real["zeros"], real["ones"], real["rand_like"]
        torch.Tensor.cuda = real["cuda"]
        torch.cuda.empty_cache = real["empty_cache"]
    N0 = inp["anchor"].shape[0]
    out = {f"{name}/{k}": v for k, v in inp.items()}
    assert len(draws) == SETTINGS["update_depth"], len(draws)
    for i, d in enumerate(draws):
        out[f"{name}/draw{i}"] = d
    N1 = int(m._anchor.shape[0])
    for p in PARAMS:
        t = getattr(m, "_" + p).detach().numpy()
        assert np.array_equal(t[:N0], inp[p]), p
        out[f"{name}/out_{p}"] = t[N0:]
        st = state_of(m, p)
        assert st["exp_avg"].shape[0] == N1 and st["exp_avg_sq"].shape[0] == N1
        for s in ("exp_avg", "exp_avg_sq"):
            assert np.array_equal(st[s][:N0].numpy(), inp[f"{s}_{p}"]) and not st[s][N0:].any()
    for a in ACCUMS:
        t = getattr(m, a).numpy()
        assert np.array_equal(t[:N0], inp[a]) and not t[N0:].any()
    out[f"{name}/N_after"] = np.int64(N1)
    print(name, "N", N0, "->", N1)
    return out


def main():
    from make_reference_vectors2 import import_reference
    import_reference()
    GM = sys.modules["scene.gaussian_model"]
    # the logs the method takes of constants: log(cur_size) for powers of two, inverse_sigmoid(0.1) -- away from midpoints
    for c in [VOXEL * f for f in (16, 4, 1)]:
        lg = np.float32(np.log(np.float64(np.float32(c))))
        assert abs(np.log(np.float64(np.float32(c))) - np.float64(lg)) < 0.3 * np.spacing(abs(lg)), c
    out = {}
    for j, name in enumerate(("grow", "none", "ties", "occupied", "onecell")):
        out.update(run_case(GM, name, 500 + j))
    out["cases"] = np.array(["grow", "none", "ties", "occupied", "onecell"])
    out["settings"] = np.array([VOXEL, THRESHOLD] + [float(SETTINGS[k]) for k in ("update_depth", "update_init_factor", "update_hierachy_factor")])
    path = os.path.join(HERE, "ref_anchor_grow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
