#!/usr/bin/env python
"""Time anchor pruning: the HIP path of gscream_amd.anchor_adjust.adjust_anchor against its force_torch path, which is the
reference's eager method (scene/gaussian_model.py:914-973 with prune_anchor, :762-805).

    python tools/anchor_adjust_bench.py [--out profiles/anchor_adjust_timing.json] [--calls 15] [--sizes 200000,500000]

Whole calls, each ending with the host knowing the new N and the device idle:
    hip    gsr_anchor_adjust_offsets + _plan, the one read-back of info, gsr_anchor_adjust_gather, the optimiser re-keying
    eager  the reference's expression sequence on the device: ~26 boolean-mask gathers (a nonzero and a size read-back each), three
           .sum() evaluated on the host, two masked assignments, a masked clamp
N anchors, K = 10 offsets, F = 32 features, Adam state on all seven parameter groups (about 1 KB per anchor); 5 % of the anchors
were seen more than check_interval * success_threshold times without opacity and are pruned, half of the rest are reset.  The
growing step is patched to a no-op in both paths, so that only the pruning half is compared.  A call consumes its model, so every
call gets a fresh copy (made outside the timed region); a call is timed with the host clock between two device synchronisations.
Both paths run in one process on one device, alternating call by call, after untimed warm-up calls of the same size; each figure
is the median over --calls calls.  The two results are compared bit for bit before anything is timed.  There is no CPU fallback:
without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd import anchor_adjust as AA  # noqa: E402
from gscream_amd import anchor_growing as AG  # noqa: E402

K, F, PRUNED = 10, 32, 0.05
PARAMS = {"anchor": (3,), "offset": (K, 3), "anchor_feat": (F,), "opacity": (1,), "uncertainty": (1,), "scaling": (6,), "rotation": (4,)}
STATS = ("anchor_demon", "opacity_accum", "uncertainty_accum", "offset_denom", "offset_gradient_accum")


class Model(types.SimpleNamespace):
    get_anchor = property(lambda self: self._anchor)


def make_base(N, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    base = {}
    for p, w in PARAMS.items():
        for k in (p, "exp_avg_" + p, "exp_avg_sq_" + p):
            base[k] = torch.randn((N,) + w, generator=g, device=dev) * 0.1
    pruned = torch.rand(N, 1, generator=g, device=dev) < PRUNED
    seen = torch.randint(0, 200, (N, 1), generator=g, device=dev).float()
    base["anchor_demon"] = torch.where(pruned, torch.full_like(seen, 150.0), seen)
    base["opacity_accum"] = torch.where(pruned, torch.zeros_like(seen), 5.0 + seen)
    base["uncertainty_accum"] = torch.rand(N, 1, generator=g, device=dev)
    base["offset_denom"] = torch.randint(0, 100, (N * K, 1), generator=g, device=dev).float()
    base["offset_gradient_accum"] = torch.rand(N * K, 1, generator=g, device=dev) * 0.001 * base["offset_denom"]
    return base, int(pruned.sum())


def make_model(base):
    m = Model(n_offsets=K)
    groups = []
    for p in PARAMS:
        t = nn.Parameter(base[p].clone())
        setattr(m, "_" + p, t)
        groups.append({"params": [t], "lr": 0.01, "name": p})
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for grp in m.optimizer.param_groups:
        p = grp["name"]
        m.optimizer.state[grp["params"][0]] = {"step": torch.tensor(1.0), "exp_avg": base["exp_avg_" + p].clone(),
                                               "exp_avg_sq": base["exp_avg_sq_" + p].clone()}
    for a in STATS:
        setattr(m, a, base[a].clone())
    return m


def one_call(base, path):
    """-> (ms, model): one adjust_anchor on a fresh model through `path`, host clock between two device synchronisations."""
    m = make_model(base)
    AA.force_torch = path == "eager"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        AA.adjust_anchor(m)
    n = int(m._anchor.shape[0])  # the host knows the new N
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    assert AA.last_path == ("torch" if path == "eager" else "hip") and n == int(m.max_radii2D.shape[0])
    return ms, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_adjust_timing.json"))
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="200000,500000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("anchor_adjust_bench needs a GPU (there is nothing to time on a CPU)")
    AG.anchor_growing = lambda model, grads, threshold, offset_mask: None  # only the pruning half is compared
    rows = []
    try:
        for size in a.sizes.split(","):
            N = int(size)
            base, n_pruned = make_base(N, 1, "cuda")
            (_t, hip), (_t, eager) = one_call(base, "hip"), one_call(base, "eager")
            assert hip._anchor.shape[0] == eager._anchor.shape[0] == N - n_pruned
            for p in PARAMS:
                th, te = getattr(hip, "_" + p), getattr(eager, "_" + p)
                assert torch.equal(th, te), p
                for s in ("exp_avg", "exp_avg_sq"):
                    assert torch.equal(hip.optimizer.state[th][s], eager.optimizer.state[te][s]), (p, s)
            for s in STATS:
                assert torch.equal(getattr(hip, s), getattr(eager, s)), s
            del hip, eager
            samples = {"hip": [], "eager": []}
            for i in range(a.warmup + a.calls):  # alternate the paths call by call
                for path in samples:
                    ms, _m = one_call(base, path)
                    if i >= a.warmup:
                        samples[path].append(ms)
            row = {"N": N, "K": K, "F": F, "pruned": n_pruned, "calls": a.calls, "warmup": a.warmup,
                   "bytes_moved": 2 * 4 * (N - n_pruned) * (3 * sum(int(torch.Size(w).numel()) for w in PARAMS.values()) + 2 * K + 3)}
            for path, v in samples.items():
                row[f"{path}_ms"] = statistics.median(v)
                row[f"{path}_ms_min_max"] = [min(v), max(v)]
            row["eager_over_hip"] = row["eager_ms"] / row["hip_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            del base
            torch.cuda.empty_cache()
    finally:
        AA.force_torch = False
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "what": "whole adjust_anchor call with anchor_growing patched out, ending with the host knowing the new N and the device idle; "
                      "median ms over the timed calls (host clock between device synchronisations); bytes_moved = kept rows read + written",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
