#!/usr/bin/env python
"""Time reading PNG files: gscream_amd.png_decode on the HIP path against PIL on the same host, from the files' bytes in host memory to
uint8 [H, W, C] pictures on the device.

    python tools/png_decode_bench.py [--out profiles/png_decode_timing.json] [--rounds 7] [--warmup 1]

Inputs (gscream_amd.synthetic.picture "texture", seeded, 567x1008x3):
    batch80    80 files: 40 written by png.encode (53 IDAT chunks each: the parallel path) and 40 by PIL's default (one segment: serial)
    own1       one file written by png.encode
    pil1       one file written by PIL's default
Per input two paths alternate round by round in one process after untimed warm-up rounds:
    hip        png_decode.decode + png_decode.check: parse, staging, one H2D copy, the launches, the status read-back (which waits)
    pil        per file np.asarray(Image.open(...)), torch.from_numpy(...).cuda(); one synchronize at the end
Medians over --rounds rounds with min and max.  One further decode per input runs under torch.profiler for the per-kernel split
(device time per kernel name, summed over the launch sequence).  The pictures of both paths are compared once: they must be equal.
Nothing else is asserted: the output is the record.  `batch80.hip_below_pil` is the acceptance figure of INTEGRATION V: it decides the
default reader of png_decode.evaluate_files.  There is no CPU fallback: without a GPU this fails."""
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
from gscream_amd import png_decode as D  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402


def pil_bytes(image):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, format="png")
    return buf.getvalue()


def own_bytes(image):
    (data,) = P.to_bytes(P.encode(torch.from_numpy(image).cuda()))
    return data


def pil_path(files):
    from PIL import Image
    out = [torch.from_numpy(np.asarray(Image.open(io.BytesIO(b)))).cuda() for b in files]
    torch.cuda.synchronize()
    return out


def hip_path(files):
    return D.check(D.decode(files, "cuda")).images


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def kernel_split(files):
    """device microseconds per kernel name over one decode, through torch.profiler; an error string when the profiler gives nothing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            hip_path(files)
            torch.cuda.synchronize()
        split = {}
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA and "png_" in e.name:
                split[e.name.split("(")[0]] = split.get(e.name.split("(")[0], 0.0) + float(e.device_time)
        return split or "the profiler recorded no png_* kernels"
    except Exception as e:  # the record says so
        return f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_decode_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("png_decode_bench needs a GPU (there is nothing to time on a CPU)")
    import PIL
    H, W = 567, 1008
    images = [S.picture("texture", H, W, 3, seed=s) for s in range(80)]
    own = [own_bytes(im) for im in images[:40]]
    pil = [pil_bytes(im) for im in images[40:]]
    inputs = {"batch80": (own + pil, images), "own1": (own[:1], images[:1]), "pil1": (pil[:1], images[40:41])}
    rows = []
    for name, (files, want) in inputs.items():
        samples = {"hip": [], "pil": []}
        for i in range(a.warmup + a.rounds):
            timed = {}
            for path, fn in (("hip", hip_path), ("pil", pil_path)):
                torch.cuda.synchronize()
                start = time.perf_counter()
                got = fn(files)
                timed[path] = (time.perf_counter() - start) * 1e3
                if i == 0:
                    for g, w in zip(got, want):
                        assert np.array_equal(g.cpu().numpy(), w), (name, path)
                del got
            assert D.last_path == "hip"
            if i >= a.warmup:
                for k, v in timed.items():
                    samples[k].append(v)
        info = dict(D.last_info)
        row = {"input": name, "files": len(files), "file_bytes": sum(len(b) for b in files), "rounds": a.rounds, "warmup": a.warmup, "info": info,
               "kernels_us": kernel_split(files)}
        row.update({k: summary(v) for k, v in samples.items()})
        row["hip_below_pil"] = row["hip"]["median_ms"] < row["pil"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "pil": PIL.__version__, "cpus": os.cpu_count(),
              "what": "hip = png_decode.decode + check: wall clock from the files' bytes in host memory to checked uint8 pictures on the "
                      "device; pil = np.asarray(Image.open) + upload per file on the same host, one synchronize; medians over the timed "
                      "rounds with min and max, the paths alternating in one process; kernels_us = device time per kernel of one decode",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| input | hip (median, min .. max) ms | PIL + upload ms | parallel / serial files |")
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['input']} | {r['hip']['median_ms']:.2f} ({r['hip']['min_ms']:.2f} .. {r['hip']['max_ms']:.2f}) "
              f"| {r['pil']['median_ms']:.1f} ({r['pil']['min_ms']:.1f} .. {r['pil']['max_ms']:.1f}) | {r['info']['parallel']} / {r['info']['serial']} |")


if __name__ == "__main__":
    main()
