#!/usr/bin/env python
"""Time render_set's PNG files: gscream_amd.png on the HIP path (encode + to_bytes: three launches and ONE copy to the host) against PIL's
encoder on the same host, and record the files' sizes.

    python tools/png_bench.py [--out profiles/png_timing.json] [--rounds 15] [--warmup 2]

Pictures (gscream_amd.synthetic.picture, seeded): the 567x1008x3 render, the 567x4032x3 sheet of view_frames (render | colour map | mask |
render) and the 567x2016x4 depth picture (two colour-map panels, RGBA).  Per picture three paths alternate round by round in one process
after untimed warm-up rounds:
    hip      png.encode of the picture on the device + png.to_bytes: the wall clock from an idle device to the files' bytes on the host
             (event_ms: HIP events around the three launches alone)
    pil1     PIL's Image.save(format="png", compress_level=1) of the same picture already on the host
    pil6     the same at PIL's default level 6 (what torchvision.utils.save_image and plt.imsave use)
PIL's side is not charged for the copy of the raw picture to the host, which the reference pays on top.  Medians over --rounds rounds
with min and max.  The second table is bytes: the device's file, PIL at both levels and the zlib Z_RLE model (the host path of
gscream_amd.png) for each content at 567x1008x3.  Nothing is asserted: the output is the record (the device's median against pil1's is
the acceptance figure of INTEGRATION U).  There is no CPU fallback: without a GPU this fails."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd import png as P  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402


def pictures():
    H, W = 567, 1008
    sheet = np.concatenate([S.picture(k, H, W, 3, seed=s) for s, k in enumerate(("texture", "colormap", "mask", "texture"))], 1)
    depth = np.concatenate([S.picture("colormap", H, W, 4, seed=s) for s in (4, 5)], 1)
    return {"render 567x1008x3": S.picture("texture", H, W, 3, seed=0), "sheet 567x4032x3": sheet, "depth 567x2016x4": np.ascontiguousarray(depth)}


def pil_bytes(image, level):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(image[..., 0] if image.shape[2] == 1 else image).save(buf, format="png", compress_level=level)
    return buf.getvalue()


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_timing.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("png_bench needs a GPU (there is nothing to time on a CPU)")
    import PIL
    rows = []
    for name, image in pictures().items():
        dev = torch.from_numpy(image).cuda()
        samples = {"hip": [], "hip_event": [], "pil1": [], "pil6": []}
        sizes = {}
        for i in range(a.warmup + a.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start = time.perf_counter()
            t0.record()
            batch = P.encode(dev)
            t1.record()
            files = P.to_bytes(batch)
            wall = (time.perf_counter() - start) * 1e3
            assert P.last_path == "hip"
            torch.cuda.synchronize()
            timed = {"hip": wall, "hip_event": t0.elapsed_time(t1)}
            sizes["hip"] = len(files[0])
            for level in (1, 6):
                start = time.perf_counter()
                data = pil_bytes(image, level)
                timed[f"pil{level}"] = (time.perf_counter() - start) * 1e3
                sizes[f"pil{level}"] = len(data)
            if i >= a.warmup:
                for k, v in timed.items():
                    samples[k].append(v)
        from PIL import Image
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[0]))).reshape(image.shape), image)
        row = {"picture": name, "raw_bytes": int(image.size), "rounds": a.rounds, "warmup": a.warmup, "bytes": sizes}
        row.update({k: summary(v) for k, v in samples.items()})
        row["hip_below_pil1"] = row["hip"]["median_ms"] < row["pil1"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    size_rows = []
    for kind in ("texture", "colormap", "mask", "constant", "noise"):
        image = S.picture(kind, 567, 1008, 3, seed=1)
        files = P.to_bytes(P.encode(torch.from_numpy(image).cuda()))
        P.force_torch = True
        try:
            model = P.to_bytes(P.encode(torch.from_numpy(image)))
        finally:
            P.force_torch = False
        row = {"content": kind, "raw_stream_bytes": 567 * (1 + 1008 * 3), "hip": len(files[0]), "zlib_rle_model": len(model[0]),
               "pil1": len(pil_bytes(image, 1)), "pil6": len(pil_bytes(image, 6))}
        size_rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "pil": PIL.__version__, "cpus": os.cpu_count(),
              "what": "hip = png.encode on the device + png.to_bytes (one copy), wall clock from an idle device to the files' bytes on the "
                      "host; hip_event = HIP events around the three launches; pil1 / pil6 = PIL Image.save(png, compress_level) of the "
                      "picture already on the host; medians over the timed rounds with min and max, the paths alternating in one process; "
                      "sizes = file bytes per content at 567x1008x3, zlib_rle_model = the host path of gscream_amd.png",
              "rows": rows, "sizes": size_rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| picture | hip (median, min .. max) ms | launches alone ms | PIL level 1 ms | PIL level 6 ms |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['picture']} | {r['hip']['median_ms']:.2f} ({r['hip']['min_ms']:.2f} .. {r['hip']['max_ms']:.2f}) | {r['hip_event']['median_ms']:.2f} "
              f"| {r['pil1']['median_ms']:.1f} ({r['pil1']['min_ms']:.1f} .. {r['pil1']['max_ms']:.1f}) "
              f"| {r['pil6']['median_ms']:.1f} ({r['pil6']['min_ms']:.1f} .. {r['pil6']['max_ms']:.1f}) |")
    print("| content 567x1008x3 | device | zlib Z_RLE model | PIL level 1 | PIL level 6 |")
    print("|---|---|---|---|---|")
    for r in size_rows:
        print(f"| {r['content']} | {r['hip']} | {r['zlib_rle_model']} | {r['pil1']} | {r['pil6']} |")


if __name__ == "__main__":
    main()
