#!/usr/bin/env python3
"""Record what gscream_amd/_layout.py says about the rasterizer's workspaces over record_workspace_sizes.py's grid ->
tests/golden/workspace_layouts.json: byte offset, dtype and shape of every view geom_views / image_views / binning_views cut
from the buffer (point_list and band_flag are computed from point_list_raw, not cut), the four constants, and ckpt_pos,
num_chunks, xcd_tiles and xcd_tile over small sets.  tests/test_workspace_sizes.py holds _layout to these numbers.  The
buffers are meta tensors of the library's own gsr_*_bytes (the 3088x3088 image workspace is 6.2 GB), so this runs on the CPU:

    python tools/record_workspace_layouts.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from record_workspace_sizes import COUNTS, IMAGES  # noqa: E402

COMPUTED = ("point_list", "band_flag")
SEG_LENGTHS = (64, 128)
CHUNK_COUNTS = (0, 1, 1024, 1025, 100000, 262144, 1000000)
TILE_COUNTS = (1, 3, 4, 31, 32, 33, 2268, 8160)


def grid():
    return {"geom": [(p,) for p in COUNTS],
            "image": [(p, w, h) for p in (0, 1, 2049, 100000, 300000) for w, h in IMAGES],
            "binning": [(r, None) for r in COUNTS] + [(100, 2049), (0, 64)]}


def _describe(views):
    return {name: [v.storage_offset() * v.element_size(), str(v.dtype).replace("torch.", ""), list(v.shape)]
            for name, v in views.items() if name not in COMPUTED}


def record():
    import torch
    from gscream_amd import _layout, _native
    lib = _native.load()

    def meta(n):
        return torch.empty(int(n), dtype=torch.uint8, device="meta")
    out = {"constants": {k: int(getattr(_layout, k)) for k in ("SEG1", "SEG2", "SEG_MAX", "XCD_CHUNK")}}
    out["ckpt_pos"] = {str(L): [int(_layout.ckpt_pos(k, L)) for k in range(out["constants"]["SEG_MAX"] - 1)] for L in SEG_LENGTHS}
    out["num_chunks"] = [[p, int(_layout.num_chunks(p))] for p in CHUNK_COUNTS]
    out["xcd"] = [[t, int(_layout.xcd_tiles(t)), [[int(_layout.xcd_tile(x, i, t)) for i in range(_layout.xcd_tiles(t))] for x in range(8)]]
                  for t in TILE_COUNTS]
    g = grid()
    out["geom"] = [[list(a), _describe(_layout.geom_views(b, *a))] for a in g["geom"] for b in [meta(lib.gsr_geom_bytes(*a))]]
    out["image"] = [[list(a), _describe(_layout.image_views(b, *a))] for a in g["image"] for b in [meta(lib.gsr_image_bytes(*a))]]
    out["binning"] = [[[r, cap], _describe(_layout.binning_views(b, r, cap))] for r, cap in g["binning"]
                      for b in [meta(lib.gsr_binning_bytes(r if cap is None else cap))]]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "workspace_layouts.json"))
    args = ap.parse_args()
    layouts = record()
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": ' + (json.dumps(v) if not isinstance(v, list) else "[\n  " + ",\n  ".join(json.dumps(r) for r in v) + "]")
                                   for k, v in layouts.items()) + "\n}\n")
    print(f"{args.out}: {sum(len(layouts[k]) for k in grid())} layouts")


if __name__ == "__main__":
    main()
