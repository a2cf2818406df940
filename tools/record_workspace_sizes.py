#!/usr/bin/env python3
"""Record what every workspace size query of libgsraster.so returns over a small grid -> tests/golden/workspace_sizes.json,
as {query: [[[args...], bytes], ...]}.  tests/test_workspace_sizes.py holds the built library to these numbers: a change of a
workspace layout shows there, on the CPU, before a kernel writes past a caller's allocation.  Run it on the commit whose sizes
are to be kept (the library loads without a device):

    python tools/record_workspace_sizes.py [--out FILE]

The grid: each term of each layout moves on its own at least once, and every query that rejects sizes gets two rejected
inputs (they give 0).  gsr_geom_bytes, gsr_binning_bytes, gsr_backward_scratch_bytes' counts, the loss, knn and depth-loss
queries reject nothing (a count below 1 is sized as 1): their two out-of-range inputs record that.
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COUNTS = [0, 1, 63, 64, 65, 2048, 2049, 100000]
# (W, H): the last three have more tiles than GSR_OCC_MAX_TILES (8192; 1920x1080 has 8160), more than GSR_MAX_TILES_LDS
# (36864), and -- like 1x1 -- so few pixels that the occlusion tables outgrow the checkpoint planes they alias
IMAGES = [(1, 1), (16, 16), (17, 33), (1008, 567), (1920, 1080), (1936, 1088), (3088, 3088), (3, 2)]
SMALL_IMAGES = IMAGES[:5]
JPEG_INTERVAL_BLOCKS = 1024  # GSR_JPEG_INTERVAL_BLOCKS


def grid():
    g = {}
    g["gsr_geom_bytes"] = [(p,) for p in COUNTS + [-1, -100000]]
    g["gsr_binning_bytes"] = [(r,) for r in COUNTS + [-1, -100000]]
    # P = 300000: the count table has all GSR_MAX_CHUNKS rows
    g["gsr_image_bytes"] = [(p, w, h) for p in (0, 1, 2049, 100000, 300000) for w, h in IMAGES] + [(-1, 16, 16), (1, 0, 0)]
    g["gsr_backward_scratch_bytes"] = list(itertools.product(COUNTS, COUNTS)) + [(-1, -1), (1, -100000)]
    g["gsr_loss_workspace_bytes"] = [(c, h, w) for c in (1, 3) for w, h in SMALL_IMAGES] + [(0, 0, 0), (-1, 16, 16)]
    g["gsr_knn_workspace_bytes"] = [(p,) for p in COUNTS + [-1, -100000]]
    g["gsr_decode_weight_grad_workspace_bytes"] = [()]
    g["gsr_depth_loss_workspace_bytes"] = [(h, w) for w, h in SMALL_IMAGES] + [(0, 0), (-1, 16)]
    g["gsr_anchor_grow_workspace_bytes"] = list(itertools.product(COUNTS, COUNTS)) + [(-1, 1), (1, -1)]
    g["gsr_crossattn_workspace_bytes"] = [(1, 1, 1, 1), (2, 4, 63, 65), (1, 8, 2048, 100), (3, 2, 100, 2049), (1, 1, 64, 100000),
                                          (0, 1, 1, 1), (1, 1, 0, 1)]
    g["gsr_anchor_sample_workspace_bytes"] = [(n, m) for n in COUNTS for m in (0, 4096)] + [(-1, 0), (1, -1)]
    g["gsr_anchor_adjust_workspace_bytes"] = [(n,) for n in COUNTS + [-1, 0x7fffff01]]
    g["gsr_image_metrics_workspace_bytes"] = [(b, c, h, w) for b, c in ((1, 1), (2, 3)) for w, h in ((3, 3), (32, 16), (33, 17), (1008, 567), (1920, 1080))] \
        + [(0, 3, 16, 16), (1, 3, 2, 16)]
    g["gsr_lpips_workspace_bytes"] = [(b, h, w) for b in (1, 3) for w, h in ((16, 16), (17, 33), (33, 17), (1008, 567), (1919, 1079))] \
        + [(0, 16, 16), (1, 15, 16)]
    g["gsr_frame_stats_workspace_bytes"] = [(b, h, w) for b in (1, 3) for w, h in SMALL_IMAGES + [(64, 64), (65, 64)]] + [(0, 16, 16), (1, 0, 16)]
    g["gsr_png_capacity"] = [(h, w, c) for c in (1, 3, 4) for w, h in SMALL_IMAGES] + [(0, 16, 3), (16, 16, 2)]
    g["gsr_png_workspace_bytes"] = [(b, h, w, c) for b in (1, 3) for c in (1, 3, 4) for w, h in SMALL_IMAGES] + [(0, 16, 16, 3), (1, 16, 16, 2)]
    jpeg = [(1, 444), (3, 444), (3, 420)]
    g["gsr_jpeg_capacity"] = [(h, w, c, s) for c, s in jpeg for w, h in SMALL_IMAGES] + [(16, 16, 1, 420), (16, 16, 2, 444)]
    g["gsr_jpeg_workspace_bytes"] = [(b, h, w, c, s, ri) for b in (1, 3) for c, s in jpeg for w, h in SMALL_IMAGES
                                     for ri in (0, 1, JPEG_INTERVAL_BLOCKS // (1 if c == 1 else 6 if s == 420 else 3))] \
        + [(1, 16, 16, 3, 444, JPEG_INTERVAL_BLOCKS // 3 + 1), (1, 16, 16, 1, 420, 0)]
    # npieces * 12 and nfiles * 4 off a multiple of 16 (and on one), stream_bytes on and off one
    g["gsr_png_decode_workspace_bytes"] = [(s, f, p) for s in (0, 16, 17, 4096, 1000003) for f, p in ((1, 1), (3, 5), (4, 4), (7, 2049))] \
        + [(16, 0, 1), (1 << 40, 1, 1)]
    for q in ("gsr_sort_keys_workspace_bytes", "gsr_voxelize_workspace_bytes", "gsr_kth_smallest_workspace_bytes"):
        g[q] = [(n,) for n in COUNTS + [1 << 20, -1, (1 << 30) + 1]]
    return g


def record():
    from gscream_amd import _native
    lib = _native.load()
    return {q: [[list(a), int(getattr(lib, q)(*a))] for a in args] for q, args in grid().items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "workspace_sizes.json"))
    args = ap.parse_args()
    sizes = record()
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{q}": {json.dumps(rows)}' for q, rows in sizes.items()) + "\n}\n")
    print(f"{args.out}: {sum(len(r) for r in sizes.values())} sizes of {len(sizes)} queries")


if __name__ == "__main__":
    main()
