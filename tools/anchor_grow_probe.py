"""Times one anchor-growing level and the whole anchor_growing call, reference expressions vs the HIP path, on one GPU.

    python tools/anchor_grow_probe.py [--sizes 100000,300000,1000000] [--reps 5]

Per N (K = 10, F = 32, ~10 % of the offsets candidates, GScream's cell sizes 0.005 x {16, 4, 1}) and level, with HIP events:
  ref_ms   the reference's per-level expressions in torch (chunked U x N test + scatter_reduce amax: tests' restatement)
  hip_ms   gscream_amd.anchor_growing.grow_level (host syncs included), and of that the torch.sort of the keys (sort_ms) and
           the HIP kernels alone (kern_ms = everything on the stream minus the sort, measured by timing the two calls apart)
  peak     torch.cuda.max_memory_allocated above the inputs, MB
and the whole anchor_growing call (three levels on a fresh stand-in each repetition) both ways.  One JSON line per row."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd import _native, anchor_growing as AG  # noqa: E402
from tests.test_anchor_grow import Standin, ref_anchor_growing, ref_level  # noqa: E402

DEV = "cuda:0"
SIZES = [0.005 * f for f in (16, 4, 1)]


def scene(N, K=10, F=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    extent = 10.0 * (N / 300000) ** (1 / 3)  # same density at every N
    anchor = torch.round((torch.rand(N, 3, generator=g) * 2 - 1) * extent / 0.005) * 0.005
    offset = torch.randn(N, K, 3, generator=g)
    raw_scaling = torch.randn(N, 6, generator=g) * 0.5 - 3.5
    feat = torch.randn(N, F, generator=g)
    grads = torch.rand(N * K, generator=g) * 0.0004   # ~half above the 2e-4 threshold: ~10 % candidates after the random pick
    offset_mask = torch.rand(N * K, generator=g) < 0.4
    return [t.to(DEV) for t in (anchor.float(), offset, raw_scaling, feat, grads, offset_mask)]


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def kernels_only_ms(args, cur_size, reps):
    """The two native calls alone (keys, then emit on the pre-sorted keys), timed with events: the HIP kernels of a level."""
    lib = _native.load()
    anchor, offset, scaling, feat, mask = args
    N, K, F = anchor.shape[0], offset.shape[1], feat.shape[1]
    m8 = mask.view(torch.uint8).contiguous()
    L = m8.numel()
    ws = torch.empty(int(lib.gsr_anchor_grow_workspace_bytes(N, L)), dtype=torch.uint8, device=DEV)
    keys = torch.empty(L, dtype=torch.int64, device=DEV)
    rows = torch.empty(L, dtype=torch.int32, device=DEV)
    info = torch.empty(4, dtype=torch.int32, device=DEV)
    P = _native.ptr
    inv = float(np.float32(1.0) / np.float32(cur_size))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call_keys = lambda: _native.check(lib.gsr_anchor_grow_keys(N, K, L, P(anchor), P(offset), P(scaling), P(m8), inv, P(ws), P(keys), P(rows),
                                                               P(info), st), "keys")
    call_keys()
    M = int(info[0])
    skeys, order = torch.sort(keys[:M], stable=True)
    cand = torch.empty((M, 3), device=DEV)
    nf = torch.empty((M, F), device=DEV)
    call_emit = lambda: _native.check(lib.gsr_anchor_grow_emit(N, K, F, L, M, P(feat), P(skeys), P(order), P(rows), float(np.float32(cur_size)),
                                                               P(ws), P(cand), P(nf), P(info), st), "emit")
    sort_ms = timed(lambda: torch.sort(keys[:M], stable=True), reps)
    return timed(lambda: (call_keys(), call_emit()), reps), sort_ms, M


def model_of(anchor, offset, raw_scaling, feat):
    from torch import nn
    N, K = offset.shape[0], offset.shape[1]
    m = Standin(voxel_size=0.005, update_depth=3, update_init_factor=16, update_hierachy_factor=4, n_offsets=K, feat_dim=feat.shape[1])
    z = lambda *s: torch.zeros(*s, device=DEV)
    params = dict(anchor=anchor, offset=offset, anchor_feat=feat, opacity=z(N, 1), uncertainty=z(N, 1), scaling=raw_scaling, rotation=z(N, 4))
    groups = []
    for k, v in params.items():
        p = nn.Parameter(v.clone())
        setattr(m, "_" + k, p)
        groups.append({"params": [p], "lr": 0.01, "name": k})
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for g in m.optimizer.param_groups:
        p = g["params"][0]
        m.optimizer.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    for a in ("anchor_demon", "opacity_accum", "uncertainty_accum"):
        setattr(m, a, z(N, 1))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,300000,1000000")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for N in [int(s) for s in a.sizes.split(",")]:
        anchor, offset, raw, feat, grads, omask = scene(N)
        scaling = torch.exp(raw)
        total = {"ref_ms": 0.0, "hip_ms": 0.0, "kern_ms": 0.0, "sort_ms": 0.0}
        for i, s in enumerate(SIZES):
            torch.manual_seed(i)
            mask = torch.logical_and(torch.logical_and(grads >= 0.0002 * 2 ** i, omask), torch.rand(N * 10, device=DEV) > 0.5 ** (i + 1))
            args = (anchor, offset, scaling, feat, mask)
            got, want = AG.grow_level(*args, s), ref_level(*args, s)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (N, s)
            ref_ms = timed(lambda: ref_level(*args, s), a.reps)
            hip_ms = timed(lambda: AG.grow_level(*args, s), a.reps)
            kern_ms, sort_ms, M = kernels_only_ms(args, s, a.reps)
            row = dict(N=N, level=i, cur_size=s, M=M, C=int(got[0].shape[0]), ref_ms=ref_ms, hip_ms=hip_ms, kern_ms=kern_ms, sort_ms=sort_ms,
                       speedup=ref_ms / hip_ms, ref_peak_mb=peak_mb(lambda: ref_level(*args, s)),
                       hip_peak_mb=peak_mb(lambda: AG.grow_level(*args, s)))
            for k in total:
                total[k] += row[k]
            print(json.dumps(row), flush=True)

        def whole(fn):
            gen = torch.Generator(device=DEV).manual_seed(7)
            real = torch.rand_like
            torch.rand_like = lambda t, **k: torch.rand(t.shape, device=t.device, generator=gen)
            try:
                m = model_of(anchor, offset, raw, feat)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(m)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, m
            finally:
                torch.rand_like = real
        ref_call = [whole(lambda m: ref_anchor_growing(m, grads, 0.0002, omask)) for _ in range(3)]
        hip_call = [whole(lambda m: AG.anchor_growing(m, grads, 0.0002, omask)) for _ in range(3)]
        assert torch.equal(ref_call[-1][1]._anchor, hip_call[-1][1]._anchor)
        print(json.dumps(dict(N=N, levels_total=total, call_ref_ms=float(np.median([t for t, _ in ref_call])),
                              call_hip_ms=float(np.median([t for t, _ in hip_call])), N_after=int(hip_call[-1][1]._anchor.shape[0]))), flush=True)


if __name__ == "__main__":
    main()
