#!/usr/bin/env python
"""Time the cross-attention anchor sampler: the HIP path against the eager torch statement of the block it replaces.

    python tools/anchor_sampler_bench.py [--out profiles/anchor_sampler_timing.json] [--blocks 7] [--sizes 200000,500000]

Whole calls, each ending with the host knowing the result:
    hip    sample_crossattn_anchors (gsr_anchor_sample) + the one read-back of info
    eager  the block of train.py:436-511 as eager torch on the device (`eager_block` below): boolean-mask gathers and assignments,
           .sum() compared on the host, two nonzero, two CPU randperm whose indices are copied to the device -- what a trainer
           runs today
N anchors project uniformly over a 567 x 1008 image and a margin around it, 90 % visible; the mask is 1 left of a slanted edge and
0 right of it; the 256-pixel patch straddles the edge, so both classes pass the reference's 2000.  Both paths run in one process
on one device, alternating block by block.  Each figure is the median over `--blocks` blocks of the mean call time of one block; a
block is timed with the host clock between two device synchronisations and runs enough calls to last >= --block-ms (sized from an
untimed warm-up of the same size and path).  The two results are compared before anything is timed: same counts, same set sizes
(the sets differ, the draws are different generators).  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd import anchor_sampler as AS  # noqa: E402

H, W, PATCH, MAX_PAIRS = 567, 1008, 256, 2000


def make_scene(N, seed, dev):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.05 * W, 1.05 * W, N).astype(np.float32)
    y = rng.uniform(-0.05 * H, 1.05 * H, N).astype(np.float32)
    visible = rng.random(N) < 0.9
    cols, rows = np.meshgrid(np.arange(W), np.arange(H))
    gt = (cols < 0.45 * W + 0.2 * rows).astype(np.float32)
    min_y, min_x = (H - PATCH) // 2, int(0.45 * W + 0.1 * H) - PATCH // 2
    rect = (min_y, min_y + PATCH, min_x, min_x + PATCH)
    return (torch.from_numpy(visible).to(dev), torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(gt).to(dev)), rect


def eager_block(visible, x, y, gt, rect, max_pairs=MAX_PAIRS):
    """The sampler as a trainer states it today, in eager torch on the device: -> (src_mask, dst_mask) or None where the reference
    gives up.  Every boolean-mask index is a nonzero and a size read-back; the comparisons of .sum() and the shapes stop the host."""
    h, w = gt.shape
    min_y, max_y, min_x, max_x = rect
    in_view = ((y > 0) & (y < h)) & ((x > 0) & (x < w)) & visible
    iy, ix = y.long(), x.long()
    patch = torch.zeros_like(gt).long()
    patch[min_y:max_y, min_x:max_x] = 1
    in_patch = patch[iy[in_view], ix[in_view]]
    n_patch = in_patch.sum()
    if not (n_patch > 0):
        return None
    sampled = -1 * torch.ones_like(visible, dtype=torch.long)
    sampled[in_view] = in_patch
    label = -1 * torch.ones_like(visible, dtype=torch.long)
    label[in_view] = gt.long()[iy[in_view], ix[in_view]]
    label_in_patch = label[sampled > 0]
    fg_at = torch.nonzero(label_in_patch > 0).squeeze()
    bg_at = torch.nonzero(label_in_patch == 0).squeeze()
    if label_in_patch.shape[0] <= 11 or fg_at.shape[0] <= 11 or bg_at.shape[0] <= 11:
        return None
    n = min(bg_at.shape[0], fg_at.shape[0], max_pairs)
    bg_take = bg_at[torch.randperm(bg_at.size(0))][:n]
    fg_take = fg_at[torch.randperm(fg_at.size(0))][:n]
    masks = []
    for take in (fg_take, bg_take):
        used = torch.zeros(int(n_patch), device=visible.device).bool()
        used[take] = True
        m = torch.zeros_like(visible)
        m[sampled > 0] = used
        masks.append(m)
    return masks[0], masks[1]


def hip_call(args, rect):
    out = AS.sample_crossattn_anchors(*args, rect, max_pairs=MAX_PAIRS)
    return out, out[4].tolist()


def time_calls(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "anchor_sampler_timing.json"))
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--sizes", default="200000,500000")
    ap.add_argument("--block-ms", type=float, default=200.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("anchor_sampler_bench needs a GPU (there is nothing to time on a CPU)")
    dev = "cuda"
    torch.manual_seed(0)
    rows = []
    for size in a.sizes.split(","):
        N = int(size)
        args, rect = make_scene(N, 1, dev)
        (_sm, _dm, _sr, _dr, _info), info = hip_call(args, rect)
        assert AS.last_path == "hip"
        eager = eager_block(*args, rect)
        assert eager is not None and info[4] == 1
        assert int(eager[0].sum()) == int(eager[1].sum()) == info[3] == MAX_PAIRS, (int(eager[0].sum()), info)
        work = {"hip": lambda: hip_call(args, rect), "eager": lambda: eager_block(*args, rect)}
        calls, samples = {}, {}
        for path, fn in work.items():
            for _ in range(5):
                fn()
            calls[path] = max(5, int(a.block_ms / max(time_calls(fn, 10), 1e-3)) + 1)
            samples[path] = []
        for _ in range(a.blocks):           # alternate the paths block by block
            for path, fn in work.items():
                samples[path].append(time_calls(fn, calls[path]))
        row = {"N": N, "H": H, "W": W, "patch": PATCH, "max_pairs": MAX_PAIRS, "blocks": a.blocks, "n_sampled": info[0], "n_fg": info[1],
               "n_bg": info[2], "min_num": info[3]}
        for path in work:
            row[f"{path}_ms"] = statistics.median(samples[path])
            row[f"{path}_ms_min_max"] = [min(samples[path]), max(samples[path])]
            row[f"{path}_calls_per_block"] = calls[path]
        row["eager_over_hip"] = row["eager_ms"] / row["hip_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "what": "whole sampler call including the host read-back, median of per-block mean ms (host clock between device synchronisations)",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
