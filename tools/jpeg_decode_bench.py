#!/usr/bin/env python
"""Time reading JPEG files: gscream_amd.jpeg_decode on the HIP path against PIL on the same host, from the files' bytes in host memory
to uint8 [H, W, C] pictures on the device with the host knowing the status.

    python tools/jpeg_decode_bench.py [--out profiles/jpeg_decode_timing.json] [--rounds 15] [--warmup 2]

Inputs (tests' "texture" picture, seeded, 567x1008x3, quality 95):
    own80      80 files of jpeg.encode, 4:4:4 (the odd height): a restart interval per MCU row, 71 each -> 5 680 wavefronts of work
    pil80      80 files of PIL's writer, 4:2:0, no restart markers: one interval, one wavefront, per file
    own1       one file of jpeg.encode
    pil1       one file of PIL's writer
Per input two paths alternate round by round in one process after untimed warm-up rounds:
    hip        jpeg_decode.decode + jpeg_decode.check: parse, staging, one H2D copy, the launches, the status read-back (which waits)
    pil        per file np.asarray(Image.open(...)), torch.from_numpy(...).cuda(); one synchronize at the end
Medians over --rounds rounds with min and max.  One further decode per input runs under torch.profiler for the per-kernel split
(device time per kernel name).  The pictures of both paths are compared once: they must be equal.  Nothing else is asserted: the
output is the record (INTEGRATION Z).  There is no CPU fallback: without a GPU this fails."""
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
from gscream_amd import jpeg as J  # noqa: E402
from gscream_amd import jpeg_decode as D  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402


def pil_bytes(image):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(image).save(buf, format="JPEG", quality=95, subsampling=2)
    return buf.getvalue()


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
            if e.device_type == torch.autograd.DeviceType.CUDA and "jpeg_decode_" in e.name:
                split[e.name.split("(")[0]] = split.get(e.name.split("(")[0], 0.0) + float(e.device_time)
        return split or "the profiler recorded no jpeg_decode_* kernels"
    except Exception as e:  # the record says so
        return f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_timing.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=80)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("jpeg_decode_bench needs a GPU (there is nothing to time on a CPU)")
    import PIL
    H, W = 567, 1008
    images = [S.picture("texture", H, W, 3, seed=s) for s in range(a.files)]
    own = []
    for at in range(0, a.files, 8):
        own += J.to_bytes(J.encode(torch.from_numpy(np.stack(images[at:at + 8])).cuda(), 95, "4:4:4"))
    pil = [pil_bytes(im) for im in images]
    inputs = {"own80": own, "pil80": pil, "own1": own[:1], "pil1": pil[:1]}
    rows = []
    for name, files in inputs.items():
        samples = {"hip": [], "pil": []}
        for i in range(a.warmup + a.rounds):
            timed, got = {}, {}
            for path, fn in (("hip", hip_path), ("pil", pil_path)):
                torch.cuda.synchronize()
                start = time.perf_counter()
                got[path] = fn(files)
                timed[path] = (time.perf_counter() - start) * 1e3
            if i == 0:
                for k, (g, w) in enumerate(zip(got["hip"], got["pil"])):
                    assert torch.equal(g, w), (name, k)
            del got
            assert D.last_path == "hip"
            if i >= a.warmup:
                for k, v in timed.items():
                    samples[k].append(v)
        row = {"input": name, "files": len(files), "file_bytes": sum(len(b) for b in files), "rounds": a.rounds, "warmup": a.warmup,
               "info": dict(D.last_info), "kernels_us": kernel_split(files)}
        row.update({k: summary(v) for k, v in samples.items()})
        row["hip_below_pil"] = row["hip"]["median_ms"] < row["pil"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "pil": PIL.__version__, "cpus": os.cpu_count(),
              "what": "hip = jpeg_decode.decode + check: wall clock from the files' bytes in host memory to checked uint8 pictures on the "
                      "device; pil = np.asarray(Image.open) + upload per file on the same host, one synchronize; medians over the timed "
                      "rounds with min and max, the paths alternating in one process; kernels_us = device time per kernel of one decode",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| input | hip (median, min .. max) ms | PIL + upload ms | intervals |")
    print("|---|---|---|---|")
    for r in rows:
        print(f"| {r['input']} | {r['hip']['median_ms']:.2f} ({r['hip']['min_ms']:.2f} .. {r['hip']['max_ms']:.2f}) "
              f"| {r['pil']['median_ms']:.1f} ({r['pil']['min_ms']:.1f} .. {r['pil']['max_ms']:.1f}) | {r['info']['intervals']} |")


if __name__ == "__main__":
    main()
