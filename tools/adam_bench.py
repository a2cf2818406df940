#!/usr/bin/env python
"""Time the optimiser step: gscream_amd.adam.Adam (one table-driven HIP launch) against torch.optim.Adam, default and fused=True.

    python tools/adam_bench.py [--out profiles/adam_timing.json] [--rounds 15] [--sizes 200000,500000]

The reference's full group list (scene/gaussian_model.py:376-390 with the rates of arguments/__init__.py:96-133): seven anchor
parameters of N anchors, K = 10 offsets, F = 32 features, and the four MLPs (feat + 3 + 1 -> feat -> K, K, 7 K, 3 K), eleven groups,
23 tensors, lr = 0 / eps = 1e-15 defaults as in training_setup, gradients on every tensor.  Each path owns a copy of the
parameters; all three see the same gradients.

Two figures per path, the paths alternating round by round in one process on one device after untimed warm-up rounds:
    event_ms   HIP-event time of one step() (events recorded on the stream around the call, the device idle before it)
    host_ms    host wall time per step() of a loop of --loop steps that ends in ONE synchronise: what a host-paced loop feels
each the median over --rounds rounds, with min and max.  gbytes_per_s = 28 bytes x elements / event time (p, g, m, v read; p, m, v
written).  The new path must not be slower than torch's fused Adam in either figure at either size: `hip_not_slower` records it and the
tool exits non-zero otherwise.  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd.adam import Adam  # noqa: E402

K, F = 10, 32
ANCHOR_PARAMS = (("anchor", (3,), 0.0), ("offset", (K, 3), 0.01), ("anchor_feat", (F,), 0.0075), ("opacity", (1,), 0.02),
                 ("uncertainty", (1,), 0.02), ("scaling", (6,), 0.007), ("rotation", (4,), 0.002))
MLPS = (("mlp_opacity", K, 0.002), ("mlp_uncertainty", K, 0.002), ("mlp_cov", 7 * K, 0.004), ("mlp_color", 3 * K, 0.008))
PATHS = ("torch_default", "torch_fused", "hip")


def make_groups(N, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    groups = [{"params": [nn.Parameter(torch.randn((N,) + w, generator=g, device=dev) * 0.1)], "lr": lr, "name": name}
              for name, w, lr in ANCHOR_PARAMS]
    for name, out, lr in MLPS:
        shapes = ((F, F + 3 + 1), (F,), (out, F), (out,))
        groups.append({"params": [nn.Parameter(torch.randn(sh, generator=g, device=dev) * 0.1) for sh in shapes], "lr": lr, "name": name})
    return groups


def make_optimizer(path, groups):
    if path == "hip":
        return Adam(groups, lr=0.0, eps=1e-15)
    if path == "torch_fused":
        return torch.optim.Adam(groups, lr=0.0, eps=1e-15, fused=True)
    return torch.optim.Adam(groups, lr=0.0, eps=1e-15)


def event_ms(opt):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    opt.step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def host_ms(opt, loop):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(loop):
        opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / loop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_timing.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop", type=int, default=50)
    ap.add_argument("--sizes", default="200000,500000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("adam_bench needs a GPU (there is nothing to time on a CPU)")
    rows, ok = [], True
    for size in a.sizes.split(","):
        N = int(size)
        opts = {path: make_optimizer(path, make_groups(N, 1, "cuda")) for path in PATHS}
        g = torch.Generator(device="cuda").manual_seed(2)
        first = [p for grp in opts["hip"].param_groups for p in grp["params"]]
        grads = [torch.randn(p.shape, generator=g, device="cuda") * 0.01 for p in first]
        elements = sum(p.numel() for p in first)
        for opt in opts.values():
            for p, gr in zip((p for grp in opt.param_groups for p in grp["params"]), grads):
                p.grad = gr
        samples = {path: {"event": [], "host": []} for path in PATHS}
        for i in range(a.warmup + a.rounds):  # alternate the paths round by round
            for path, opt in opts.items():
                e, h = event_ms(opt), host_ms(opt, a.loop)
                if i >= a.warmup:
                    samples[path]["event"].append(e)
                    samples[path]["host"].append(h)
        assert opts["hip"].last_path == "hip"
        row = {"N": N, "K": K, "F": F, "groups": len(opts["hip"].param_groups), "tensors": len(first), "elements": elements,
               "bytes_per_step": 28 * elements, "rounds": a.rounds, "warmup": a.warmup, "loop": a.loop}
        for path, v in samples.items():
            row[f"{path}_event_ms"] = statistics.median(v["event"])
            row[f"{path}_event_ms_min_max"] = [min(v["event"]), max(v["event"])]
            row[f"{path}_host_ms"] = statistics.median(v["host"])
            row[f"{path}_host_ms_min_max"] = [min(v["host"]), max(v["host"])]
            row[f"{path}_gbytes_per_s"] = 28 * elements / (row[f"{path}_event_ms"] * 1e-3) / 1e9
        row["hip_not_slower"] = bool(row["hip_event_ms"] <= row["torch_fused_event_ms"] and row["hip_host_ms"] <= row["torch_fused_host_ms"])
        ok = ok and row["hip_not_slower"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del opts, grads, first
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "what": "one optimiser step over the reference's eleven parameter groups (23 tensors) with gradients on every tensor; event_ms = "
                      "HIP events around one step(), host_ms = host wall time per step() of a loop ending in one synchronise; medians over "
                      "the timed rounds, the three paths alternating in one process; gbytes_per_s = 28 B x elements / event time",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not ok:
        raise SystemExit("the HIP path is slower than torch's fused Adam in at least one figure")


if __name__ == "__main__":
    main()
