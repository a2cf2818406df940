#!/usr/bin/env python
"""Time the first stage of a run: gscream_amd.scene_init on the HIP path against the host numpy line and the copies around it, and
its sort against torch.sort.

    python tools/scene_init_bench.py [--out profiles/scene_init_timing.json] [--rounds 7] [--warmup 1] [--sizes 200000,1000000]

Per cloud size (synthetic.surface_point_cloud, fp32, in host memory on both sides), two forms, each from the host array to device tensors:
    voxelize  numpy = np.unique(np.round(points / v), axis=0) * v on the host, then .float() and the copy to the device
              hip   = the copy of the points to the device, scene_init.voxelize_sample (its read-back of info included)
    create    numpy = the same line and copy, then create_from_pcd's lines (scene/gaussian_model.py:319-345) in torch on the device
                      with simple_knn.distCUDA2
              hip   = the copy of the points, scene_init.create_from_pcd
and per key count, on device tensors of random 64-bit keys and of 30-bit keys (what a voxelised cloud packs):
    sort      torch = torch.sort(keys).values;  hip = scene_init.sort_keys(keys)
The paths alternate round by round in one process after untimed warm-up rounds.  event_ms = HIP events on the stream around one call,
wall_ms = host clock from an idle device to the synchronise behind the call: medians over --rounds rounds with min and max.  Nothing
is asserted about the ratios: the output is the record.  There is no CPU fallback: without a GPU this fails."""
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
from gscream_amd import scene_init as SI  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402
from gscream_amd.simple_knn import distCUDA2  # noqa: E402

VOXEL = 0.001


def timed(fn):
    """-> (event ms, wall ms, the result)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start = time.perf_counter()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), (time.perf_counter() - start) * 1e3, out


def numpy_voxelize(points):
    return torch.from_numpy(np.unique(np.round(points / VOXEL), axis=0) * VOXEL).float().cuda()


def numpy_create(points, K=10, F=32):
    anchors = numpy_voxelize(points)
    n = anchors.shape[0]
    offsets = torch.zeros((n, K, 3), device="cuda")
    feat = torch.zeros((n, F), device="cuda")
    xyz_max = torch.max(anchors.clone(), 0)[0].unsqueeze(0)
    dist2 = torch.clamp_min(distCUDA2(anchors), 0.0000001)
    scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 6)
    rots = torch.zeros((n, 4), device="cuda")
    rots[:, 0] = 1
    x = 0.1 * torch.ones((n, 1), dtype=torch.float, device="cuda")
    opacities, uncertainties = torch.log(x / (1 - x)), torch.log(x / (1 - x))
    return anchors, offsets, feat, scales, rots, opacities, uncertainties, torch.zeros(n, device="cuda"), xyz_max


def run_paths(paths, rounds, warmup):
    samples = {p: {"event": [], "wall": []} for p in paths}
    for i in range(warmup + rounds):  # alternate the paths round by round
        for p, fn in paths.items():
            event, wall, out = timed(fn)
            if i >= warmup:
                samples[p]["event"].append(event)
                samples[p]["wall"].append(wall)
            del out
    row = {}
    for p, s in samples.items():
        for kind in ("event", "wall"):
            row[f"{p}_{kind}_ms"] = statistics.median(s[kind])
            row[f"{p}_{kind}_ms_min_max"] = [min(s[kind]), max(s[kind])]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_init_timing.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="200000,1000000")
    ap.add_argument("--sort-sizes", default="200000,1000000,16777216")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scene_init_bench needs a GPU (there is nothing to time on a CPU)")
    rows, sort_rows = [], []
    for n in (int(x) for x in a.sizes.split(",")):
        points = np.ascontiguousarray(S.surface_point_cloud(1, n).astype(np.float32))
        paths = {"numpy_voxelize": lambda: numpy_voxelize(points),
                 "hip_voxelize": lambda: SI.voxelize_sample(torch.from_numpy(points).cuda(), VOXEL),
                 "numpy_create": lambda: numpy_create(points),
                 "hip_create": lambda: SI.create_from_pcd(torch.from_numpy(points).cuda(), VOXEL)}
        m = int(paths["hip_voxelize"]().shape[0])
        assert SI.last_path == "hip" and m == int(paths["numpy_voxelize"]().shape[0])
        row = {"points": n, "anchors": m, "voxel_size": VOXEL, "dtype": "float32", "rounds": a.rounds, "warmup": a.warmup}
        row.update(run_paths(paths, a.rounds, a.warmup))
        for form in ("voxelize", "create"):
            row[f"{form}_wall_ratio"] = row[f"numpy_{form}_wall_ms"] / row[f"hip_{form}_wall_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for n in (int(x) for x in a.sort_sizes.split(",")):
        draw = lambda: torch.randint(0, 1 << 32, (n,), generator=g, dtype=torch.int64, device="cuda")
        for kind, keys in (("random 64-bit", (draw() << 32) | draw()), ("30-bit", draw() >> 2)):
            paths = {"torch_sort": lambda: torch.sort(keys).values, "hip_sort": lambda: SI.sort_keys(keys)}
            row = {"keys": n, "kind": kind, "rounds": a.rounds, "warmup": a.warmup}
            row.update(run_paths(paths, a.rounds, a.warmup))
            row["sort_event_ratio"] = row["torch_sort_event_ms"] / row["hip_sort_event_ms"]
            sort_rows.append(row)
            print(json.dumps(row), flush=True)
            del keys, paths
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "numpy": np.__version__,
              "what": "point cloud in host memory -> device tensors: event_ms = HIP events around one call, wall_ms = host clock from an "
                      "idle device to the synchronise behind it; medians over the timed rounds with min and max, the paths alternating in "
                      "one process; numpy_* = the host numpy line and the copy of its result (create: then create_from_pcd's lines in "
                      "torch on the device), hip_* = the copy of the points and gscream_amd.scene_init; sort rows: int64 keys on the "
                      "device (torch.sort orders the random 64-bit keys as signed, sort_keys as unsigned: the same work)",
              "rows": rows, "sort_rows": sort_rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
