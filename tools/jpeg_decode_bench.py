#!/usr/bin/env python
"""Time reading JPEG files: gscream_amd.jpeg_decode on the HIP path -- one wavefront per restart interval, and the split decode of
include/gsraster_jpeg_split.h -- against PIL on the same host, from the files' bytes in host memory to uint8 [H, W, C] pictures on the
device with the host knowing the status.

    python tools/jpeg_decode_bench.py [--out profiles/jpeg_decode_timing.json] [--rounds 15] [--warmup 2] [--parent-lib libgsraster_parent.so]

Inputs (tests' "texture" picture, seeded, 567x1008x3, quality 95):
    own80      80 files of jpeg.encode, 4:4:4 (the odd height): a restart interval per MCU row, 71 each -> 5 680 wavefronts of work
    pil80      80 files of PIL's writer, 4:2:0, no restart markers: one interval per file
    own1       one file of jpeg.encode
    pil1       one file of PIL's writer
Per input the paths alternate round by round in one process after untimed warm-up rounds:
    hip        jpeg_decode.decode(split="never") + jpeg_decode.check: parse, staging, one H2D copy, the launches, the status read-back (which waits)
    split      the same with split="auto" at the chosen subsequence_bytes and min_bytes (below)
    pil        per file np.asarray(Image.open(...)), torch.from_numpy(...).cuda(); one synchronize at the end
Medians over --rounds rounds with min and max.  One further decode per input and device path runs under torch.profiler for the
per-kernel split (device time per kernel name).  The pictures of all paths are compared once: they must be equal.

In front of the rows two sweeps, same protocol, whose results choose what the rows' split path runs with:
    subsequence_bytes   split="always" at 64, 128, 256, 512 on pil80 and pil1; chosen: the best median on pil80
    min_bytes           8 files of jpeg.encode with a growing restart interval (MCUs per interval: --intervals), split="never" against
                        split="always" at the chosen subsequence_bytes; chosen: the smallest measured interval length (bytes of entropy-coded data, mean) from
                        which on the split path's median stays below the one-wave path's; none: recorded as null
--parent-lib: a libgsraster.so built from the parent commit; a fresh child process times its one-wave path ("parent") on the same four
inputs in the same session.  The rule for the default of `split` is then evaluated and recorded ("default_rule"): "auto" only if on both
marker-less rows the split median is below the parent's and on both rows with markers the min .. max ranges overlap.
Nothing else is asserted: the output is the record (INTEGRATION Z).  There is no CPU fallback: without a GPU this fails."""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd import jpeg as J  # noqa: E402
from gscream_amd import jpeg_decode as D  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402

H, W = 567, 1008


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


def hip_path(files, **split):
    return D.check(D.decode(files, "cuda", **split)).images


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs)}


def kernel_split(files, **split):
    """device microseconds per kernel name over one decode, through torch.profiler; an error string when the profiler gives nothing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            hip_path(files, **split)
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA and ("jpeg_decode_" in e.name or "jpeg_split_" in e.name):
                out[e.name.split("(")[0]] = out.get(e.name.split("(")[0], 0.0) + float(e.device_time)
        return out or "the profiler recorded no jpeg_decode_* / jpeg_split_* kernels"
    except Exception as e:  # the record says so
        return f"{type(e).__name__}: {e}"


def alternate(files, paths, rounds, warmup, name):
    """paths: {name: callable(files)}; they alternate round by round; the first round's pictures must all be equal -> {name: summary}"""
    samples = {k: [] for k in paths}
    for i in range(warmup + rounds):
        timed, got = {}, {}
        for path, fn in paths.items():
            torch.cuda.synchronize()
            start = time.perf_counter()
            got[path] = fn(files)
            timed[path] = (time.perf_counter() - start) * 1e3
        if i == 0:
            first = next(iter(got))
            for path in got:
                for k, (g, w) in enumerate(zip(got[path], got[first])):
                    assert torch.equal(g, w), (name, path, k)
        del got
        assert D.last_path == "hip"
        if i >= warmup:
            for k, v in timed.items():
                samples[k].append(v)
    return {k: summary(v) for k, v in samples.items()}


def make_inputs(n):
    images = [S.picture("texture", H, W, 3, seed=s) for s in range(n)]
    own = []
    for at in range(0, n, 8):
        own += J.to_bytes(J.encode(torch.from_numpy(np.stack(images[at:at + 8])).cuda(), 95, "4:4:4"))
    pil = [pil_bytes(im) for im in images]
    return images, {"own80": own, "pil80": pil, "own1": own[:1], "pil1": pil[:1]}


def child(a):
    """The one-wave path alone, for a library given through GSR_LIB that need not export the split family (split="never" never
    touches it): one JSON line."""
    _, inputs = make_inputs(a.files)
    rows = {}
    for name, files in inputs.items():
        rows[name] = alternate(files, {"hip": lambda f: hip_path(f, split="never"), "pil": pil_path}, a.rounds, a.warmup, name)["hip"]
    print("CHILD " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_timing.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=80)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--intervals", default="8,16,32,63,126,252,341", help="MCUs per restart interval of the min_bytes sweep (jpeg.encode: at most 1024 blocks)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("jpeg_decode_bench needs a GPU (there is nothing to time on a CPU)")
    if a.child:
        return child(a)
    import PIL
    images, inputs = make_inputs(a.files)

    # ---- sweep 1: subsequence_bytes on the marker-less inputs ----
    sweep_b = []
    for name in ("pil80", "pil1"):
        paths = {f"B{b}": (lambda f, b=b: hip_path(f, split="always", subsequence_bytes=b)) for b in (64, 128, 256, 512)}
        got = alternate(inputs[name], paths, a.rounds, a.warmup, name)
        sweep_b.append({"input": name, **{k: v for k, v in got.items()}})
        print(json.dumps(sweep_b[-1]), flush=True)
    B = int(min((k for k in sweep_b[0] if k != "input"), key=lambda k: sweep_b[0][k]["median_ms"])[1:])

    # ---- sweep 2: the interval length from which the split path wins ----
    sweep_m = []
    stack = torch.from_numpy(np.stack(images[:8])).cuda()
    for ri in (int(v) for v in a.intervals.split(",")):
        files = J.to_bytes(J.encode(stack, 95, "4:4:4", ri))
        got = alternate(files, {"hip": lambda f: hip_path(f, split="never"), "split": lambda f: hip_path(f, split="always", subsequence_bytes=B)},
                        a.rounds, a.warmup, f"ri{ri}")
        intervals = D.last_info["intervals"]
        # an interval's data as the device measures it (end - start): the scan without its RST markers and without EOI
        data_bytes = sum(len(f) - D.parse(f).scan - 2 for f in files) - 2 * (intervals - len(files))
        sweep_m.append({"restart_interval": ri, "files": len(files), "intervals": intervals, "interval_bytes": data_bytes / intervals,
                        "split_intervals": D.last_info.get("split_intervals"), "repaired_intervals": D.last_info.get("repaired_intervals"), **got})
        print(json.dumps(sweep_m[-1]), flush=True)
    least = None
    for r in reversed(sweep_m):  # from the longest down: while the split path stays below
        if r["split"]["median_ms"] < r["hip"]["median_ms"]:
            least = int(r["interval_bytes"])
        else:
            break

    # ---- the four rows ----
    chosen = {"subsequence_bytes": B, "min_bytes": least}
    auto = {"split": "auto", "subsequence_bytes": B, "min_bytes": least if least is not None else D.DEFAULT_MIN_BYTES}
    rows = []
    for name, files in inputs.items():
        got = alternate(files, {"hip": lambda f: hip_path(f, split="never"), "split": lambda f: hip_path(f, **auto), "pil": pil_path}, a.rounds, a.warmup, name)
        hip_path(files, **auto)
        info = dict(D.last_info)
        row = {"input": name, "files": len(files), "file_bytes": sum(len(b) for b in files), "rounds": a.rounds, "warmup": a.warmup, "info": info,
               "kernels_us": kernel_split(files, split="never"), "split_kernels_us": kernel_split(files, **auto)}
        row.update(got)
        row["hip_below_pil"] = row["hip"]["median_ms"] < row["pil"]["median_ms"]
        row["split_below_pil"] = row["split"]["median_ms"] < row["pil"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- the parent commit's library, a fresh process, the same session ----
    parent, rule = None, None
    if a.parent_lib:
        env = dict(os.environ, GSR_LIB=os.path.abspath(a.parent_lib))
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(a.rounds), "--warmup", str(a.warmup), "--files", str(a.files)],
                             env=env, capture_output=True, text=True)
        lines = [ln for ln in run.stdout.splitlines() if ln.startswith("CHILD ")]
        if run.returncode != 0 or not lines:
            parent = f"the child process failed ({run.returncode}): {run.stderr[-800:]}"
        else:
            parent = json.loads(lines[-1][6:])
            for r in rows:
                r["parent"] = parent[r["input"]]
            by = {r["input"]: r for r in rows}
            below = {n: by[n]["split"]["median_ms"] < by[n]["parent"]["median_ms"] for n in ("pil80", "pil1")}
            overlap = {n: by[n]["split"]["min_ms"] <= by[n]["parent"]["max_ms"] and by[n]["parent"]["min_ms"] <= by[n]["split"]["max_ms"] for n in ("own80", "own1")}
            rule = {"split_median_below_parent": below, "ranges_overlap": overlap, "selects": "auto" if all(below.values()) and all(overlap.values()) else "never"}

    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "pil": PIL.__version__, "cpus": os.cpu_count(),
              "what": "hip = jpeg_decode.decode(split='never') + check: wall clock from the files' bytes in host memory to checked uint8 pictures on "
                      "the device; split = the same with split='auto' at `chosen`; pil = np.asarray(Image.open) + upload per file on the same host, "
                      "one synchronize; parent = hip with the parent commit's library in a fresh process of the same session; medians over the "
                      "timed rounds with min and max, the paths alternating in one process; kernels_us / split_kernels_us = device time per kernel "
                      "of one decode; sweep_subsequence_bytes: split='always'; sweep_min_bytes: 8 jpeg.encode files per restart interval",
              "chosen": chosen, "shipped": {"subsequence_bytes": D.DEFAULT_SUBSEQUENCE_BYTES, "min_bytes": D.DEFAULT_MIN_BYTES, "split": D.DEFAULT_SPLIT},
              "default_rule": rule, "sweep_subsequence_bytes": sweep_b, "sweep_min_bytes": sweep_m, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("| input | one wave per interval (median, min .. max) ms | split ms | parent ms | PIL + upload ms | intervals |")
    print("|---|---|---|---|---|---|")

    def cell(s, digits=2):
        return f"{s['median_ms']:.{digits}f} ({s['min_ms']:.{digits}f} .. {s['max_ms']:.{digits}f})" if isinstance(s, dict) else "-"
    for r in rows:
        print(f"| {r['input']} | {cell(r['hip'])} | {cell(r['split'])} | {cell(r.get('parent'))} | {cell(r['pil'], 1)} | {r['info']['intervals']} |")
    print("chosen:", json.dumps(chosen), "default rule:", json.dumps(rule))


if __name__ == "__main__":
    main()
