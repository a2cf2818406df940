#!/usr/bin/env python
"""Time the normal picture of render_set: gscream_amd.normals on the HIP path against the eager form the reference runs.

    python tools/normals_bench.py [--out profiles/normals_timing.json] [--rounds 15] [--sizes 567x1008,1080x1920]

Per frame size, window 9, a seeded synthetic depth with a real focal length (0.8 x the frame width):
    hip         depth2pcd_fromplane + least_square_normal_regress_fast01 on the HIP path; the two calls are also timed one by one
    torch_fp32  the point map in eager torch + `_normals_torch(dtype=float32)`: the reference's arithmetic (the unfolded
                [h*w, 81, 3] window tensor, batched matmul, det and inverse in fp32), with the caller's [h*w, 81, 1] ones allocated
                outside the timed region, as render_set holds them
    torch_fp64  (--with-fp64) the same statement in fp64: this package's fallback for tensors the HIP path does not take
The paths alternate round by round in one process on one device after untimed warm-up rounds.  event_ms is the HIP-event time of
one call (events recorded on the stream around it, the device idle before it): the median over --rounds rounds, with min and max.
peak_mbytes is torch.cuda.max_memory_allocated over the call minus what was allocated before it (inputs and the ones excluded).
Nothing is asserted about the ratio: the output is the record.  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gscream_amd import normals as N  # noqa: E402
from normals_helpers import synthetic_frame  # noqa: E402

SIZE = 9


def timed(fn):
    """-> (event ms, peak bytes above the starting allocation, the result)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), torch.cuda.max_memory_allocated() - base, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_timing.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="567x1008,1080x1920")
    ap.add_argument("--with-fp64", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("normals_bench needs a GPU (there is nothing to time on a CPU)")
    rows = []
    for size in a.sizes.split(","):
        h, w = (int(x) for x in size.split("x"))
        depth, K, c2w = (torch.from_numpy(x).cuda() for x in synthetic_frame(h, w, 7))
        depth = depth[None]
        ones32 = torch.ones(h * w, SIZE * SIZE, 1, device="cuda")
        ones64 = ones32.double() if a.with_fp64 else None
        state = {}

        def hip_points():
            state["pts"] = N.depth2pcd_fromplane(depth, c2w, K, h, w)
            return state["pts"]

        def hip_normals():
            return N.least_square_normal_regress_fast01(state["pts"])

        def hip():
            return N.least_square_normal_regress_fast01(N.depth2pcd_fromplane(depth, c2w, K, h, w))

        def torch_path(dtype, ones):
            def run():
                pts = N._points_torch(depth, c2w, K, h, w)
                return N._as_reference_returns(N._normals_torch(pts, SIZE, 0.15, 1e-5, dtype, None, ones).float(), h, w)
            return run

        paths = {"hip_points": hip_points, "hip_normals": hip_normals, "hip": hip, "torch_fp32": torch_path(torch.float32, ones32)}
        if a.with_fp64:
            paths["torch_fp64"] = torch_path(torch.float64, ones64)
        samples = {p: {"ms": [], "peak": []} for p in paths}
        results = {}
        for i in range(a.warmup + a.rounds):  # alternate the paths round by round
            for p, fn in paths.items():
                ms, peak, out = timed(fn)
                if p.startswith("hip"):
                    assert N.last_path == "hip"
                if i >= a.warmup:
                    samples[p]["ms"].append(ms)
                    samples[p]["peak"].append(peak)
                if i == 0:
                    results[p] = out.reshape(3, h, w).clone() if p in ("hip", "torch_fp32", "torch_fp64") else None
                del out
        row = {"h": h, "w": w, "size": SIZE, "rounds": a.rounds, "warmup": a.warmup}
        for p, v in samples.items():
            row[f"{p}_event_ms"] = statistics.median(v["ms"])
            row[f"{p}_event_ms_min_max"] = [min(v["ms"]), max(v["ms"])]
            row[f"{p}_peak_mbytes"] = max(v["peak"]) / 2 ** 20
        row["speedup_vs_torch_fp32"] = row["torch_fp32_event_ms"] / row["hip_event_ms"]
        # how far the reference's fp32 arithmetic is from the fp64 evaluation of the same expression on this frame (angle, radians)
        cos = (results["hip"].double() * results["torch_fp32"].double()).sum(0).clamp(-1, 1)
        ang = torch.acos(cos).flatten()
        row["fp32_vs_hip_angle_rad_median_p99_max"] = [float(ang.median()), float(ang.kthvalue(int(0.99 * ang.numel())).values), float(ang.max())]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del ones32, ones64, state, results, paths
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "what": "the normal picture of one frame, window 9: event_ms = HIP events around one call, the device idle before it; medians "
                      "over the timed rounds with min and max, the paths alternating in one process; peak_mbytes = "
                      "max_memory_allocated over the call above the allocation before it; hip = both calls, hip_points / hip_normals "
                      "= each alone; torch_fp32 = the reference's eager arithmetic",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
