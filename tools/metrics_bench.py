#!/usr/bin/env python
"""Time the metric loop of evaluate(): gscream_amd.metrics on the HIP path against the eager form the reference runs.

    python tools/metrics_bench.py [--out profiles/metrics_timing.json] [--rounds 15] [--views 40] [--sizes 567x1008,1080x1920]

Per frame size, --views seeded pairs (a smooth picture and a noisy copy, PSNR ~ 34 dB, passed through the PNG quantisation as
evaluate() reads them) with one [1,3,H,W] expanded mask each:
    hip         one image_metrics call over all the pairs (quantize=True, the masks stacked as [B,1,H,W]) and one read-back of the four
                values per view
    torch_fp32  the reference's loop over the views in its arithmetic: per view my_ssim and psnr, plain and masked
                (`_dssim_map_torch(dtype=float32)`: fp32 taps, one 5x5 conv2d per window sum, the map computed again for the masked
                value as evaluate() calls my_ssim twice; `value[mask]` gathers; fp32 means), then the four values read one by one:
                six host stops per view
The paths alternate round by round in one process on one device after untimed warm-up rounds.  event_ms is the HIP-event time
(events recorded on the stream around the path, the device idle before it, so it includes the first launch's latency); wall_ms is
the host clock around the same work, ending when the last value is on the host.  Medians over --rounds rounds, with min and max.
Per frame size the distance of the fp32 statement's values from the HIP result is recorded too (median / 99th percentile / max over
the views).  Nothing is asserted about the ratio: the output is the record.  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd import metrics as M  # noqa: E402

KEYS = ("ssim", "psnr", "ssim_masked", "psnr_masked")


def make_views(n, h, w, seed):
    """-> pred, gt [n,3,h,w] fp32 on the device, already quantised, and masks [n,1,h,w] bool (a disc and a band: ~40 % true)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    i = torch.arange(h, device="cuda", dtype=torch.float32)[None, None, :, None]
    j = torch.arange(w, device="cuda", dtype=torch.float32)[None, None, None, :]
    k = torch.arange(n * 3, device="cuda", dtype=torch.float32).reshape(n, 3, 1, 1)
    gt = 0.5 + 0.35 * torch.sin(0.011 * i + 0.007 * j + 0.9 * k) * torch.cos(0.05 * i - 0.013 * j + 0.4 * k)
    pred = gt + 0.02 * torch.randn(gt.shape, device="cuda", generator=gen)
    v = torch.arange(n, device="cuda", dtype=torch.float32).reshape(n, 1, 1, 1)
    disc = ((i - h / 2) ** 2 + (j - w * (0.3 + 0.01 * v)) ** 2) < (0.3 * h) ** 2
    band = (j > 0.7 * w) & (i > 0.2 * h)
    return M._transform_torch(pred, False, True).contiguous(), M._transform_torch(gt, False, True).contiguous(), (disc | band).contiguous()


def reference_view(x, y, mask):
    """evaluate()'s four values of one view ([1,3,H,W] images, [1,3,H,W] mask) in the reference's arithmetic, as 0-d device tensors."""
    ssim = 1 - 2 * torch.mean(M._dssim_map_torch(x, y, torch.float32))
    psnr = -10 * torch.log10(torch.mean((x - y) ** 2))
    ssim_m = 1 - 2 * torch.mean(M._dssim_map_torch(x, y, torch.float32)[mask])
    psnr_m = -10 * torch.log10(torch.mean(((x - y) ** 2)[mask]))
    return ssim, psnr, ssim_m, psnr_m


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    w0 = time.perf_counter()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), (time.perf_counter() - w0) * 1e3, out


def spread(v):
    v = sorted(v)
    return [statistics.median(v), v[min(len(v) - 1, int(0.99 * len(v)))], v[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_timing.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--sizes", default="567x1008,1080x1920")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("metrics_bench needs a GPU (there is nothing to time on a CPU)")
    rows = []
    for size in a.sizes.split(","):
        h, w = (int(x) for x in size.split("x"))
        pred, gt, masks = make_views(a.views, h, w, 7)
        expanded = [masks[k:k + 1].expand(1, 3, -1, -1) for k in range(a.views)]

        def hip():
            m = M.image_metrics(pred, gt, masks, quantize=True)
            return torch.stack([m.ssim, m.psnr, m.ssim_masked, m.psnr_masked], 1).cpu().tolist()

        def torch_fp32():
            out = []
            for k in range(a.views):
                out.append([v.item() for v in reference_view(pred[k:k + 1], gt[k:k + 1], expanded[k])])
            return out

        paths = {"hip": hip, "torch_fp32": torch_fp32}
        samples = {p: {"event": [], "wall": []} for p in paths}
        results = {}
        for i in range(a.warmup + a.rounds):  # alternate the paths round by round
            for p, fn in paths.items():
                ev, wall, out = timed(fn)
                if p == "hip":
                    assert M.last_path == "hip"
                if i >= a.warmup:
                    samples[p]["event"].append(ev)
                    samples[p]["wall"].append(wall)
                results[p] = out
        row = {"h": h, "w": w, "views": a.views, "rounds": a.rounds, "warmup": a.warmup}
        for p, v in samples.items():
            for kind in ("event", "wall"):
                row[f"{p}_{kind}_ms"] = statistics.median(v[kind])
                row[f"{p}_{kind}_ms_min_max"] = [min(v[kind]), max(v[kind])]
        row["speedup_event"] = row["torch_fp32_event_ms"] / row["hip_event_ms"]
        row["speedup_wall"] = row["torch_fp32_wall_ms"] / row["hip_wall_ms"]
        for c, key in enumerate(KEYS):  # how far the reference's fp32 arithmetic is from the fp64 evaluation, value by value
            row[f"fp32_vs_hip_{key}_median_p99_max"] = spread([abs(results["torch_fp32"][k][c] - results["hip"][k][c]) for k in range(a.views)])
        row["hip_values_view0"] = dict(zip(KEYS, results["hip"][0]))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pred, gt, masks, expanded, results
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "what": "evaluate()'s SSIM / PSNR, plain and masked, of `views` test views: hip = one image_metrics call and one read-back; "
                      "torch_fp32 = the reference's eager loop with six host stops per view; event_ms = HIP events around the path, the "
                      "device idle before it; wall_ms = host clock to the last value on the host; medians over the timed rounds with min "
                      "and max, the paths alternating in one process; fp32_vs_hip_* = |fp32 statement - HIP result| per view, "
                      "median / 99th percentile / max",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
