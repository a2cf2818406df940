#!/usr/bin/env python
"""Time LPIPS of evaluate()'s test views: gscream_amd.lpips on the HIP path against the eager fp32 torch statement.

    python tools/lpips_bench.py [--out profiles/lpips_timing.json] [--rounds 5] [--warmup 2] [--views 1,8] [--size 567x1008]

Seeded random weights at the real VGG-16 widths (LPIPS.random), seeded image pairs in [0, 1] with one bool mask each:
    hip         one lpips_views(core="hip") call over all the views: one VGG pass per pair gives the plain and the masked value
    eager       the fp32 torch statement (`_lpips_torch(dtype=float32)`: conv2d, max_pool2d, interpolate) on the same device, once
                per pair -- the same single pass, in eager torch
    four_pass   the reference's form (train.py:948, :952): per view the statement twice, once for the plain value and once for the
                spatial map whose masked mean is taken by a boolean gather; each runs VGG on both images
The paths alternate round by round in one process on one device after untimed warm-up rounds; every round is timed with HIP events
recorded on the stream around the path, the device idle before it.  Reported: the median ms per view with min and max, and TFLOP/s
of the convolution arithmetic actually needed (2 images per view, 2 FLOP per MAC) against the 157.3 TFLOP/s fp32 matrix peak; the
four-pass form is charged the same useful work.  --layers also times gsr_conv3x3_relu alone at each layer's own size (2 images)
against conv2d + relu.  Nothing is asserted about the ratio: the output is the record.  Without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gscream_amd import lpips as LP  # noqa: E402

PEAK_TFLOPS = 157.3


def layer_sizes(h, w):
    """[(Cin, Cout, H, W)] of the 13 convolutions."""
    out, layer = [], 0
    for l in range(5):
        if l:
            h, w = h // 2, w // 2
        while layer <= LP.GROUP_END[l]:
            out.append((*LP.WIDTHS[layer], h, w))
            layer += 1
    return out


def view_flops(h, w):
    return 2 * 2 * sum(ci * co * 9 * hh * ww for ci, co, hh, ww in layer_sizes(h, w))


def make_views(n, h, w, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    i = torch.arange(h, device="cuda", dtype=torch.float32)[None, None, :, None]
    j = torch.arange(w, device="cuda", dtype=torch.float32)[None, None, None, :]
    k = torch.arange(n * 3, device="cuda", dtype=torch.float32).reshape(n, 3, 1, 1)
    gt = 0.5 + 0.35 * torch.sin(0.011 * i + 0.007 * j + 0.9 * k) * torch.cos(0.05 * i - 0.013 * j + 0.4 * k)
    pred = (gt + 0.03 * torch.randn(gt.shape, device="cuda", generator=gen)).clamp(0, 1)
    masks = (((i - h / 2) ** 2 + (j - 0.4 * w) ** 2) < (0.3 * h) ** 2)[0].expand(n, h, w).contiguous()
    return pred.contiguous(), gt.contiguous(), masks


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def run_paths(paths, warmup, rounds):
    samples, results = {p: [] for p in paths}, {}
    for i in range(warmup + rounds):  # alternate the paths round by round
        for p, fn in paths.items():
            ms, out = timed(fn)
            if i >= warmup:
                samples[p].append(ms)
            results[p] = out
    return samples, results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_timing.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--views", default="1,8")
    ap.add_argument("--size", default="567x1008")
    ap.add_argument("--layers", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("lpips_bench needs a GPU (there is nothing to time on a CPU)")
    h, w = (int(x) for x in a.size.split("x"))
    model = LP.LPIPS.random(0, "cuda")
    flops = view_flops(h, w)
    rows = []
    for views in (int(v) for v in a.views.split(",")):
        pred, gt, masks = make_views(views, h, w, 7)

        def hip():
            out = LP.lpips_views(model, pred, gt, masks, core="hip")
            assert LP.last_path == "hip"
            return out

        def eager():
            rs = [LP._lpips_torch(model, pred[k:k + 1], gt[k:k + 1], masks[k], True, torch.float32) for k in range(views)]
            return torch.cat([r["plain"] for r in rs]), torch.cat([r["masked"] for r in rs])

        def four_pass():
            plain, masked = [], []
            for k in range(views):
                plain.append(LP._lpips_torch(model, pred[k:k + 1], gt[k:k + 1], None, True, torch.float32)["plain"])
                smap = LP._lpips_torch(model, pred[k:k + 1], gt[k:k + 1], None, True, torch.float32)["spatial"]
                masked.append(smap[0][masks[k]].mean()[None])  # (the boolean gather is a host stop, as in the reference)
            return torch.cat(plain), torch.cat(masked)

        samples, results = run_paths({"hip": hip, "eager": eager, "four_pass": four_pass}, a.warmup, a.rounds)
        row = {"h": h, "w": w, "views": views, "rounds": a.rounds, "warmup": a.warmup, "gflop_per_view": flops / 1e9}
        for p, v in samples.items():
            med = statistics.median(v)
            row[f"{p}_ms_per_view"] = med / views
            row[f"{p}_ms_per_view_min_max"] = [min(v) / views, max(v) / views]
            row[f"{p}_tflops"] = flops * views / (med * 1e-3) / 1e12
            row[f"{p}_fraction_of_peak"] = row[f"{p}_tflops"] / PEAK_TFLOPS
        row["speedup_over_eager"] = row["eager_ms_per_view"] / row["hip_ms_per_view"]
        row["speedup_over_four_pass"] = row["four_pass_ms_per_view"] / row["hip_ms_per_view"]
        for p in ("eager", "four_pass"):  # how far the fp32 statement's values are from the HIP result
            for c, key in enumerate(("plain", "masked")):
                row[f"{p}_vs_hip_{key}_max_rel"] = float(((results[p][c] - results["hip"][c]).abs() / results["hip"][c].abs()).max())
        row["hip_values_view0"] = [float(results["hip"][0][0]), float(results["hip"][1][0])]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pred, gt, masks, results
        torch.cuda.empty_cache()
    layer_rows = []
    if a.layers:
        convs, biases, _ = model.weights(torch.device("cuda"))
        seen = set()
        for i, (ci, co, hh, ww) in enumerate(layer_sizes(h, w)):
            if (ci, co, hh, ww) in seen:
                continue
            seen.add((ci, co, hh, ww))
            x = torch.randn((2, ci, hh, ww), device="cuda")
            packed = LP.pack_conv3x3(convs[i])
            samples, _ = run_paths({"hip": lambda: LP.conv3x3_relu(x, packed, biases[i]),
                                    "eager": lambda: F.relu(F.conv2d(x, convs[i], biases[i], padding=1))}, a.warmup, a.rounds)
            fl = 2 * 2 * ci * co * 9 * hh * ww
            r = {"cin": ci, "cout": co, "h": hh, "w": ww, "images": 2}
            for p, v in samples.items():
                r[f"{p}_ms"] = statistics.median(v)
                r[f"{p}_tflops"] = fl / (r[f"{p}_ms"] * 1e-3) / 1e12
            layer_rows.append(r)
            print(json.dumps(r), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "peak_tflops_fp32_matrix": PEAK_TFLOPS,
              "what": "LPIPS (VGG-16, random weights) of `views` pairs: hip = one lpips_views call, one VGG pass per pair; eager = the fp32 "
                      "torch statement once per pair; four_pass = the reference's form, the statement twice per view and a boolean gather; "
                      "HIP events around each path, the device idle before it, medians over the timed rounds with min and max, the paths "
                      "alternating in one process; tflops = the convolution FLOP of one pass per pair over the time",
              "rows": rows, "layers": layer_rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
