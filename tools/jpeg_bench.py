#!/usr/bin/env python
"""Time the spiral video's JPEG frames: gscream_amd.jpeg on the HIP path (encode + to_bytes: four launches and ONE copy to the host)
against PIL's encoder at the same settings on the same host, and record the files' sizes.

    python tools/jpeg_bench.py [--out profiles/jpeg_timing.json] [--rounds 15] [--warmup 2]

Pictures (gscream_amd.synthetic.picture, seeded): the 567x1008x3 render at 4:2:0 and the 567x4032x3 sheet at 4:4:4 (its 567 rows are
odd: what video.save_rgbd_video picks) and at 4:2:0, quality 95.  Per picture two paths alternate round by round in one process after
untimed warm-up rounds:
    hip      jpeg.encode of the picture on the device + jpeg.to_bytes: the wall clock from an idle device to the file's bytes on the
             host (event_ms: HIP events around the four launches alone)
    pil      PIL's Image.save(format="JPEG", quality, subsampling, optimize=False, restart_marker_blocks = the same interval) of the
             same picture already on the host
PIL's side is not charged for the copy of the raw picture to the host.  Medians over --rounds rounds with min and max.  Nothing is
asserted: the output is the record, win or loss (INTEGRATION Y).  There is no CPU fallback: without a GPU this fails."""
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
from gscream_amd import jpeg as Jp  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402

QUALITY = 95


def pictures():
    H, W = 567, 1008
    sheet = np.ascontiguousarray(np.concatenate([S.picture(k, H, W, 3, seed=s) for s, k in enumerate(("texture", "colormap", "texture", "mask"))], 1))
    return [("render 567x1008x3", S.picture("texture", H, W, 3, seed=0), "4:2:0"), ("sheet 567x4032x3", sheet, "4:4:4"),
            ("sheet 567x4032x3", sheet, "4:2:0")]


def pil_bytes(image, subsampling, ri):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, format="JPEG", quality=QUALITY, subsampling={"4:4:4": 0, "4:2:0": 2}[subsampling], optimize=False,
                                restart_marker_blocks=ri)
    return buf.getvalue()


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_timing.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("jpeg_bench needs a GPU (there is nothing to time on a CPU)")
    import PIL
    from PIL import Image
    rows = []
    for name, image, sub in pictures():
        dev = torch.from_numpy(image).cuda()
        samples = {"hip": [], "hip_event": [], "pil": []}
        sizes = {}
        for i in range(a.warmup + a.rounds):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start = time.perf_counter()
            t0.record()
            batch = Jp.encode(dev, QUALITY, sub)
            t1.record()
            files = Jp.to_bytes(batch)
            wall = (time.perf_counter() - start) * 1e3
            assert Jp.last_path == "hip" and Jp.last_info["reencoded"] == 0
            torch.cuda.synchronize()
            timed = {"hip": wall, "hip_event": t0.elapsed_time(t1)}
            sizes["hip"] = len(files[0])
            start = time.perf_counter()
            data = pil_bytes(image, sub, batch.restart_interval)
            timed["pil"] = (time.perf_counter() - start) * 1e3
            sizes["pil"] = len(data)
            if i >= a.warmup:
                for k, v in timed.items():
                    samples[k].append(v)
        ours, theirs = (np.asarray(Image.open(io.BytesIO(d)), dtype=np.float64) for d in (files[0], data))
        psnr = {k: float(10 * np.log10(255.0 ** 2 / np.mean((v - image) ** 2))) for k, v in (("hip", ours), ("pil", theirs))}
        row = {"picture": name, "subsampling": sub, "quality": QUALITY, "restart_interval": batch.restart_interval, "raw_bytes": int(image.size),
               "rounds": a.rounds, "warmup": a.warmup, "bytes": sizes, "psnr_db": psnr}
        row.update({k: summary(v) for k, v in samples.items()})
        row["hip_below_pil"] = row["hip"]["median_ms"] < row["pil"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "pil": PIL.__version__, "cpus": os.cpu_count(),
              "what": "hip = jpeg.encode on the device + jpeg.to_bytes (one copy), wall clock from an idle device to the file's bytes on the "
                      "host; hip_event = HIP events around the four launches; pil = PIL Image.save(JPEG) at the same quality, subsampling "
                      "and restart interval, optimize=False, of the picture already on the host; medians over the timed rounds with min "
                      "and max, the paths alternating in one process",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| picture | hip (median, min .. max) ms | launches alone ms | PIL ms | bytes hip / PIL | PSNR hip / PIL dB |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['picture']} {r['subsampling']} | {r['hip']['median_ms']:.2f} ({r['hip']['min_ms']:.2f} .. {r['hip']['max_ms']:.2f}) "
              f"| {r['hip_event']['median_ms']:.2f} | {r['pil']['median_ms']:.1f} ({r['pil']['min_ms']:.1f} .. {r['pil']['max_ms']:.1f}) "
              f"| {r['bytes']['hip']} / {r['bytes']['pil']} | {r['psnr_db']['hip']:.2f} / {r['psnr_db']['pil']:.2f} |")


if __name__ == "__main__":
    main()
