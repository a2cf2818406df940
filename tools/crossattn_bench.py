#!/usr/bin/env python
"""Time BidirectionalCrossAttention (the whole module: projections + attention core) on the HIP path and on the eager torch path.

    python tools/crossattn_bench.py [--out profiles/crossattn_timing.json] [--blocks 7] [--sizes 2000x2000,512x512,64x64]

Forward and forward + backward, heads 8 x 64, 32-wide features, batch 1 (the shapes train.py:499 / scripts/run.py:70-71 fix), both
paths in one process on one device, alternating, on the same standard-normal inputs.  Each figure is the median over `--blocks`
blocks of the mean call time of one block; a block is bracketed by device events and runs enough calls to last >= 50 ms (sized
from an untimed warm-up of the same shape and path).  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bidirectional_cross_attention import BidirectionalCrossAttention  # noqa: E402

HEADS, DIM_HEAD, DIM = 8, 64, 32


def attention_flops(i, j):
    """Matrix-product FLOPs of the attention core as the algorithm states it (sim once, two value products; the backward's five
    products of the same size).  The HIP path recomputes sim per direction: it executes 4/3 (forward) and 10/8 (backward) of this."""
    one = 2.0 * HEADS * i * j * DIM_HEAD
    return {"forward": 3 * one, "backward": 8 * one}


def time_calls(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossattn_timing.json"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--sizes", default="2000x2000,512x512,64x64")
    ap.add_argument("--block-ms", type=float, default=50.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("crossattn_bench needs a GPU (there is nothing to time on a CPU)")
    dev = "cuda"
    torch.manual_seed(0)
    mod = BidirectionalCrossAttention(dim=DIM, heads=HEADS, dim_head=DIM_HEAD, context_dim=DIM).to(dev)
    rows = []
    for size in a.sizes.split(","):
        i, j = (int(t) for t in size.split("x"))
        x = torch.randn(1, i, DIM, device=dev)
        c = torch.randn(1, j, DIM, device=dev)
        g1, g2 = torch.randn(1, i, DIM, device=dev), torch.randn(1, j, DIM, device=dev)
        mask = torch.ones(1, i, dtype=torch.bool, device=dev)   # run_crossattn passes all-true masks
        cmask = torch.ones(1, j, dtype=torch.bool, device=dev)

        def fwd():
            with torch.no_grad():
                mod(x, c, mask=mask, context_mask=cmask)

        def fwd_bwd():
            mod.zero_grad(set_to_none=True)
            o, co = mod(x, c, mask=mask, context_mask=cmask)
            ((o * g1).sum() + (co * g2).sum()).backward()

        work = {"forward": fwd, "forward_backward": fwd_bwd}
        calls, samples = {}, {}
        for path in ("hip", "torch"):
            mod.force_torch = path == "torch"
            for name, fn in work.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                assert mod.last_path == path, (mod.last_path, path)
                per_call = time_calls(fn, 5)
                calls[path, name] = max(5, int(a.block_ms / max(per_call, 1e-3)) + 1)
                samples[path, name] = []
        for _ in range(a.blocks):           # alternate the paths block by block
            for name, fn in work.items():
                for path in ("hip", "torch"):
                    mod.force_torch = path == "torch"
                    samples[path, name].append(time_calls(fn, calls[path, name]))
        mod.force_torch = False
        fl = attention_flops(i, j)
        row = {"i": i, "j": j, "heads": HEADS, "dim_head": DIM_HEAD, "blocks": a.blocks}
        for name in work:
            for path in ("hip", "torch"):
                s = samples[path, name]
                row[f"{path}_{name}_ms"] = statistics.median(s)
                row[f"{path}_{name}_ms_min_max"] = [min(s), max(s)]
                row[f"{path}_{name}_calls_per_block"] = calls[path, name]
            row[f"{name}_torch_over_hip"] = row[f"torch_{name}_ms"] / row[f"hip_{name}_ms"]
        row["attention_gflop"] = {k: v / 1e9 for k, v in fl.items()}
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "what": "whole module call, median of per-block mean ms",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
