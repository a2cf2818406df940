#!/usr/bin/env python
"""Time Image.resize: gscream_amd.resize on the HIP path against PIL on the same host, from a picture's bytes in host memory to the
resized tensor on the device.

    python tools/resize_bench.py [--out profiles/resize_timing.json] [--rounds 5] [--warmup 1]

Inputs (seeded):
    mask1        one 2268x4032 L mask -> 567x1008, LANCZOS (readImages' mask.resize((1008, 567), Image.LANCZOS))
    mask40       40 such masks, one after the other
    rgb          1134x2016x3 -> 567x1008, BICUBIC (loadCam's pil_image.resize(resolution) at -r 2)
    depth_down   a 567x1008 F depth map -> 284x504, BICUBIC
    depth_up     the same map -> 1134x2016, BICUBIC
Per input two paths alternate round by round in one process after untimed warm-up rounds:
    hip          per picture: torch.from_numpy(...).cuda(), resize.resize; one synchronize at the end
    pil          per picture: Image.resize on the host, np.array, torch.from_numpy(...).cuda(); one synchronize at the end
Medians over --rounds rounds with min and max.  `device_ms` is the resize alone, pictures already on the device, between two events on
the stream (median over the same number of rounds).  The results of both paths are compared once: they must be equal.  Nothing else is
asserted: the output is the record, a loss is written down as a loss.  There is no CPU fallback: without a GPU this fails."""
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
from gscream_amd import resize as Z  # noqa: E402


def blobs(H, W, seed):
    """a binary mask of soft-edged blobs, as an inpainting mask is: 0 / 255 with a few grey pixels on the edges"""
    rng = np.random.default_rng(seed)
    coarse = rng.random((H // 63 + 2, W // 63 + 2)) > 0.6
    a = np.kron(coarse, np.ones((63, 63), bool))[:H, :W]
    return (a * 255).astype(np.uint8)


def pil_path(pictures, size, resample):
    from PIL import Image
    out = [torch.from_numpy(np.array(Image.fromarray(p).resize(size, resample))).cuda() for p in pictures]
    torch.cuda.synchronize()
    return out


def hip_path(pictures, size, resample):
    out = [Z.resize(torch.from_numpy(p).cuda(), size, resample) for p in pictures]
    torch.cuda.synchronize()
    return out


def device_only(pictures, size, resample, rounds):
    on_device = [torch.from_numpy(p).cuda() for p in pictures]
    times = []
    for _ in range(rounds + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for x in on_device:
            Z.resize(x, size, resample)
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return statistics.median(times[1:])


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def same(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    if a.dtype == np.float32:
        na, nb = np.isnan(a), np.isnan(b)
        return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))
    return np.array_equal(a, b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("resize_bench needs a GPU (there is nothing to time on a CPU)")
    import PIL
    rng = np.random.default_rng(0)
    masks = [blobs(2268, 4032, s) for s in range(40)]
    rgb = rng.integers(0, 256, (1134, 2016, 3), dtype=np.uint8)
    depth = (rng.random((567, 1008), dtype=np.float32) * 10).astype(np.float32)
    inputs = {"mask1": (masks[:1], (1008, 567), Z.LANCZOS), "mask40": (masks, (1008, 567), Z.LANCZOS), "rgb": ([rgb], (1008, 567), Z.BICUBIC),
              "depth_down": ([depth], (504, 284), Z.BICUBIC), "depth_up": ([depth], (2016, 1134), Z.BICUBIC)}
    rows = []
    for name, (pictures, size, resample) in inputs.items():
        samples = {"hip": [], "pil": []}
        for i in range(a.warmup + a.rounds):
            timed, got = {}, {}
            for path, fn in (("hip", hip_path), ("pil", pil_path)):
                torch.cuda.synchronize()
                start = time.perf_counter()
                got[path] = fn(pictures, size, resample)
                timed[path] = (time.perf_counter() - start) * 1e3
                if path == "hip":
                    assert Z.last_path == "hip"
            if i == 0:
                assert all(same(g, w) for g, w in zip(got["hip"], got["pil"])), name
            del got
            if i >= a.warmup:
                for k, v in timed.items():
                    samples[k].append(v)
        row = {"input": name, "pictures": len(pictures), "from": list(pictures[0].shape), "to": [size[1], size[0]],
               "filter": {Z.LANCZOS: "LANCZOS", Z.BICUBIC: "BICUBIC"}[resample], "host_bytes": int(sum(p.nbytes for p in pictures)),
               "rounds": a.rounds, "warmup": a.warmup, "device_ms": device_only(pictures, size, resample, a.rounds)}
        row.update({k: summary(v) for k, v in samples.items()})
        row["hip_below_pil"] = row["hip"]["median_ms"] < row["pil"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "pil": PIL.__version__, "cpus": os.cpu_count(),
              "what": "hip = upload + resize.resize per picture: wall clock from the picture in host memory to the synchronised resized tensor on "
                      "the device; pil = Image.resize + np.array + upload per picture on the same host, one synchronize; medians over the timed "
                      "rounds with min and max, the paths alternating in one process; device_ms = the launches alone between two events",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| input | hip: upload + resize (median, min .. max) ms | of which on the device ms | PIL + upload ms | hip below PIL |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['input']} | {r['hip']['median_ms']:.2f} ({r['hip']['min_ms']:.2f} .. {r['hip']['max_ms']:.2f}) | {r['device_ms']:.3f} "
              f"| {r['pil']['median_ms']:.1f} ({r['pil']['min_ms']:.1f} .. {r['pil']['max_ms']:.1f}) | {'yes' if r['hip_below_pil'] else 'no'} |")


if __name__ == "__main__":
    main()
