"""Golden vectors for anchor pruning, produced by RUNNING the reference's own GaussianModel.adjust_anchor.

    python tests/golden/make_reference_vectors6.py        # needs /root/reference; runs on the CPU

As make_reference_vectors5.py does for anchor_growing: scene/gaussian_model.py is imported in place
(make_reference_vectors2.import_reference) and `GaussianModel.adjust_anchor` (:914-973) is called unbound on a stand-in namespace
with the reference's own `anchor_growing`, `cat_tensors_to_optimizer`, `prune_anchor` and `_prune_anchor_optimizer` bound to it, a
real torch.optim.Adam whose groups are named like the reference's plus one "mlp_*" group, and the five densification
accumulators.  Nothing of the reference is copied: only inputs, the torch.rand_like draws and the tensors it left behind are
stored (ref_adjust_anchor.npz).  The redirections are make_reference_vectors5's (`.cuda()` / `device='cuda'` stay on the CPU,
scatter_max through scatter_reduce("amax"), seeded rand_like draws on multiples of 1/256, empty_cache a no-op); cell sizes are
powers of two.  The arguments are the reference's defaults: check_interval 100, success_threshold 0.8 (thresholds 40 and 80, exact
in fp32), grad_threshold 0.0002, min_opacity 0.005.

Cases (K = 10, F = 32):
  mixed       grows, prunes and resets
  quiet       no anchor seen more than 80 times: nothing pruned or reset, only the offset statistics reset
  all_pruned  every anchor seen often with no opacity, nothing grown: everything is pruned
  no_state    like mixed, with an optimiser that has not stepped (no state)
  clamp       kept rows with scaling[:, 3:] below, at, one ulp above and far above 0.05 (and negative)
  edges       anchor_demon exactly 80 and 81, offset_denom exactly 40 and 41, opacity_accum equal to and one ulp below
              min_opacity * anchor_demon (the fp32 product), offsets with 0 / 0
Per case, prefix "<case>/": the inputs, draw<i> per level, out_<name> = every tensor the method left behind, N_grown (anchors
after growing), n_prune, n_reset."""
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_vectors5 as V5  # noqa: E402

K, F, VOXEL, THRESHOLD, PARAMS, ACCUMS = V5.K, V5.F, V5.VOXEL, V5.THRESHOLD, V5.PARAMS, V5.ACCUMS
OFFSET_STATS = ("offset_gradient_accum", "offset_denom")
CASES = ("mixed", "quiet", "all_pruned", "no_state", "clamp", "edges")
ARGS = dict(check_interval=100, success_threshold=0.8, grad_threshold=THRESHOLD, min_opacity=0.005)


def case_inputs(name, seed):
    rng = np.random.default_rng(seed)
    q = lambda a, step: (np.round(np.asarray(a) / step) * step).astype(np.float32)
    N = 200 if name == "mixed" else 100
    grows = name in ("mixed", "no_state", "clamp", "edges")
    anchor = q(rng.uniform(-1.5, 1.5, (N, 3)), VOXEL)
    offset = q(rng.normal(0, 2.0 if grows else 1.0, (N, K, 3)), 2 ** -10)
    scaling = V5._scalings(rng, (N, 6))
    denom = rng.integers(0, 101, (N * K, 1)).astype(np.float32)
    denom[rng.random((N * K, 1)) < 0.1] = 0.0
    per_view = rng.uniform(0, 5 * THRESHOLD if grows else 0.9 * THRESHOLD, (N * K, 1))  # below the level-0 threshold when nothing may grow
    accum = q(per_view * denom * (0.999 if not grows else 1.0), THRESHOLD / 64)
    demon = rng.integers(0, 200, (N, 1)).astype(np.float32)
    if name == "quiet":
        demon = rng.integers(0, 81, (N, 1)).astype(np.float32)
    if name == "all_pruned":
        demon = rng.integers(81, 200, (N, 1)).astype(np.float32)
    opacity_accum = (rng.uniform(0, 2, (N, 1)) * 0.005 * demon).astype(np.float32)
    if name == "all_pruned":
        opacity_accum = np.zeros((N, 1), np.float32)
    if name == "clamp":
        tail = np.array([0.04, 0.05, np.nextafter(np.float32(0.05), np.float32(1)), 0.06, 1.5, -0.5, np.nextafter(np.float32(0.05), np.float32(0))],
                        np.float32)
        scaling[:, 3:] = tail[rng.integers(0, len(tail), (N, 3))]
    if name == "edges":
        demon[0::4] = 80.0
        demon[1::4] = 81.0
        prod = np.float32(0.005) * demon  # min_opacity * anchor_demon as torch computes it: one fp32 product
        opacity_accum[0::3] = prod[0::3]
        opacity_accum[1::3] = np.nextafter(prod[1::3], np.float32(-1))
        denom[0::5] = 40.0
        denom[1::5] = 41.0
        denom[2::5] = 0.0
        accum[2::5] = 0.0  # 0 / 0
        accum[7::10] = -accum[7::10]
    inp = dict(
        anchor=anchor, offset=offset, scaling=scaling, anchor_feat=q(np.clip(rng.normal(0, 1, (N, F)), -2, 2), 2 ** -3),
        opacity=q(rng.normal(0, 1, (N, 1)), 2 ** -8), uncertainty=q(rng.normal(0, 1, (N, 1)), 2 ** -8), rotation=q(rng.normal(0, 1, (N, 4)), 2 ** -8),
        offset_gradient_accum=accum.astype(np.float32), offset_denom=denom, anchor_demon=demon, opacity_accum=opacity_accum,
        uncertainty_accum=q(rng.uniform(0, 50, (N, 1)), 2 ** -4))
    if name != "no_state":
        for p in PARAMS:
            sh = inp[p].shape
            inp[f"exp_avg_{p}"] = (rng.integers(-8, 8, sh) * 2.0 ** -12).astype(np.float32)
            inp[f"exp_avg_sq_{p}"] = (rng.integers(0, 8, sh) * 2.0 ** -20).astype(np.float32)
    return inp


def make_standin(inp, GaussianModel):
    m = V5.Standin(**V5.SETTINGS)
    groups = []
    for p in PARAMS:
        t = nn.Parameter(torch.from_numpy(inp[p].copy()).requires_grad_(True))
        setattr(m, "_" + p, t)
        groups.append({"params": [t], "lr": 0.01, "name": p})
    m.mlp_opacity = nn.Linear(F + 4, K)
    groups.append({"params": m.mlp_opacity.parameters(), "lr": 0.002, "name": "mlp_opacity"})
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for g in m.optimizer.param_groups:
        if g["name"] in PARAMS and f"exp_avg_{g['name']}" in inp:
            p = g["name"]
            m.optimizer.state[g["params"][0]] = {"step": torch.tensor(3.0), "exp_avg": torch.from_numpy(inp[f"exp_avg_{p}"].copy()),
                                                 "exp_avg_sq": torch.from_numpy(inp[f"exp_avg_sq_{p}"].copy())}
    for a in ACCUMS + OFFSET_STATS:
        setattr(m, a, torch.from_numpy(inp[a].copy()))
    for meth in ("cat_tensors_to_optimizer", "anchor_growing", "prune_anchor", "_prune_anchor_optimizer"):
        setattr(m, meth, types.MethodType(getattr(GaussianModel, meth), m))
    return m


def run_case(GM, name, seed):
    inp = case_inputs(name, seed)
    m = make_standin(inp, GM.GaussianModel)
    gen = torch.Generator().manual_seed(seed)
    draws, seen = [], {}

    def rand_like(t, **kw):
        d = torch.randint(0, 256, t.shape, generator=gen).float() / 256.0
        draws.append(d.numpy().copy())
        return d

    prune = m.prune_anchor

    def prune_anchor(mask):
        seen["N_grown"], seen["n_prune"] = int(mask.shape[0]), int(mask.sum())
        prune(mask)
    m.prune_anchor = prune_anchor
    mlp_before = [p.detach().clone() for p in m.mlp_opacity.parameters()]

    real = dict(zeros=torch.zeros, ones=torch.ones, rand_like=torch.rand_like, cuda=torch.Tensor.cuda, empty_cache=torch.cuda.empty_cache)
    drop_cuda = lambda fn: (lambda *a, **k: fn(*a, **{kk: v for kk, v in k.items() if not (kk == "device" and str(v).startswith("cuda"))}))
    torch.zeros, torch.ones, torch.rand_like = drop_cuda(real["zeros"]), drop_cuda(real["ones"]), rand_like
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.empty_cache = lambda: None
    GM.scatter_max = V5.cpu_scatter_max
    try:
        with torch.no_grad():
            GM.GaussianModel.adjust_anchor(m, **ARGS)
    finally:
        torch.zeros, torch.ones, torch.rand_like = real["zeros"], real["ones"], real["rand_like"]
        torch.Tensor.cuda = real["cuda"]
        torch.cuda.empty_cache = real["empty_cache"]
    out = {f"{name}/{k}": v for k, v in inp.items()}
    assert len(draws) == V5.SETTINGS["update_depth"], len(draws)
    for i, d in enumerate(draws):
        out[f"{name}/draw{i}"] = d
    N2 = int(m._anchor.shape[0])
    for p in PARAMS:
        t = getattr(m, "_" + p)
        assert t.shape[0] == N2 and t.grad is None, p
        out[f"{name}/out_{p}"] = t.detach().numpy()
        g = next(g for g in m.optimizer.param_groups if g["name"] == p)
        assert g["params"][0] is t
        st = m.optimizer.state.get(t, None)
        assert (st is None) == (name == "no_state")
        if st is not None:
            assert float(st["step"]) == 3.0
            for s in ("exp_avg", "exp_avg_sq"):
                out[f"{name}/out_{s}_{p}"] = st[s].numpy()
    for a in ACCUMS + OFFSET_STATS:
        out[f"{name}/out_{a}"] = getattr(m, a).numpy()
    assert tuple(m.max_radii2D.shape) == (N2,) and not m.max_radii2D.any() and m.max_radii2D.dtype == torch.float32
    assert all(torch.equal(a, b) for a, b in zip(mlp_before, m.mlp_opacity.parameters()))
    n_reset = int((inp["anchor_demon"] > 80).sum())  # grown anchors start at 0
    out[f"{name}/N_after"] = np.int64(N2)
    out[f"{name}/N_grown"] = np.int64(seen["N_grown"])
    out[f"{name}/n_prune"] = np.int64(seen["n_prune"])
    out[f"{name}/n_reset"] = np.int64(n_reset)
    assert seen["N_grown"] - seen["n_prune"] == N2
    print(name, "N", inp["anchor"].shape[0], "-> grown", seen["N_grown"], "-> pruned", seen["n_prune"], "reset", n_reset, "->", N2)
    return out


def main():
    from make_reference_vectors2 import import_reference
    import_reference()
    GM = sys.modules["scene.gaussian_model"]
    out = {}
    for j, name in enumerate(CASES):
        out.update(run_case(GM, name, 600 + j))
    out["cases"] = np.array(CASES)
    out["settings"] = np.array([VOXEL, THRESHOLD] + [float(V5.SETTINGS[k]) for k in ("update_depth", "update_init_factor", "update_hierachy_factor")])
    out["args"] = np.array([float(ARGS[k]) for k in ("check_interval", "success_threshold", "grad_threshold", "min_opacity")])
    path = os.path.join(HERE, "ref_adjust_anchor.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
