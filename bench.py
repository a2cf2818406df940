#!/usr/bin/env python
"""bench.py -- BASELINE.json's metric: train iters/sec (fwd+bwd raster) @ 1M Gaussians, 1008x567.

    python bench.py --gpus N --steps K --warmup W          (N=1: run directly)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   (N>1)
    python bench.py ... --full                              (the headline plus every extra object listed below)
    python bench.py ... --dump-outputs DIR                  (also write the last timed step's outputs as DIR/<name>.npy)

One "step" = one forward + one full backward of the rasterizer through the public API
(GaussianRasterizer -> autograd -> ctypes -> C ABI -> HIP kernels) on one synthetic scene that is
already resident in HBM.  Workload at N=1 = BASELINE.json configs[1] ("book", fwd+bwd RGB-only):
the real SPIn-NeRF scene is not available (no dataset, no network), so the SURVEY 8(d) synthetic
stand-in is used and labelled as such.  With N>1 every rank rasterizes its own scene (one scene per
GPU, no collective inside the raster path; RCCL only for the barriers and the final reduction):
weak scaling, value = (N * K) / max-over-ranks time.

A plain run sets up, warms up, times the K steps and prints the headline: metric, value, unit, ms_per_step, dtype, config.
Extra objects on the JSON line, measured only with --full:
  roofline     -- for the dominant kernel stage: algorithmic bytes (SURVEY 8(d) per-unit figures x the
                  units one launch processes) / average launch duration measured live with HIP events
                  on the launch stream (gsr_profile_* in the C ABI), against the 8 TB/s HBM peak.
  cpu_baseline -- the CPU oracle (a port: oracle/gs_oracle.c, OpenMP) timed on this box's host cores on a
                  bounded sample of the same workload; rank 0, N=1 only.  Reported, not a target.
  parity_check -- MEASURED in this run: the timed library's images and gradients (one fwd+bwd through the public API)
                  against the oracle outputs the cpu_baseline leg computes on the same scene: pixels beyond 1e-4,
                  gradient elements beyond 1e-3, each classified by the decision (alpha = 1/255 / T = 1e-4) its
                  pixel / Gaussian sits next to in the oracle's walk.
  ms_per_step_spread -- three further K-step blocks after the official timed region (how much a K-step sample moves).
  next_rows    -- the SURVEY 8(f) rows (losses, decode, kNN, pipeline, train_iteration, render_fps), fixed iteration counts.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); the on-box copy ceiling is measured per run (copy_ceiling)

WORKLOADS = {
    # name: (P, W, H, seed, (color, depth, feature) upstream grads, description)
    "config2": (1_000_000, 1008, 567, 1, (True, False, False),
                "config2: synthetic stand-in for SPIn-NeRF 'book' (SURVEY 8d slab generator, seed 1), 1M Gaussians, "
                "1008x567, fwd+bwd, RGB-only upstream grads"),
    "config3": (1_000_000, 1008, 567, 2, (True, True, True),
                "config3: synthetic stand-in for SPIn-NeRF 'trash' (seed 2), 1M Gaussians, 1008x567, fwd+bwd, "
                "depth + feature heads on"),
    "config4": (2_000_000, 1920, 1080, 3, (True, True, True),
                "config4: 2M synthetic Gaussians, 1920x1080, fwd+bwd (HBM stress)"),
    "small": (50_000, 504, 284, 4, (True, True, True), "small: 50k Gaussians, 504x284 (plumbing check)"),
    # not a BASELINE config: config 2's sizes on a cloud shaped like a trained scene (synthetic.scene_surfaces: surfaces + floaters;
    # clustered depth keys, early saturation) -- a robustness probe for what the uniform slab does not exercise
    "surfaces": (1_000_000, 1008, 567, 1, (True, False, False),
                 "surfaces: 1M Gaussians on six tilted surfaces + 15 % floaters (synthetic.scene_surfaces, seed 1), 1008x567, fwd+bwd, "
                 "RGB-only upstream grads; NOT a BASELINE config"),
    # not a BASELINE config either: the frame GScream renders at ITERATION 0 of a scene -- a synthetic SfM-like surface point cloud
    # through the reference's own initialisation (create_from_pcd restated: standin_model.Model.from_pcd) and the fused decode.  P is
    # whatever the decode emits (~200k anchors x 10 offsets x the share with opacity > 0).  Upstream gradients as in training: RGB + depth.
    "init_state": (None, 1008, 567, 1, (True, True, False),
                   "init_state: ~200k voxelised surface points -> GaussianModel.create_from_pcd restated (scales from distCUDA2, zero offsets / "
                   "features, default-init MLPs) -> decode at the camera -> rasterize 1008x567, fwd+bwd, RGB + depth upstream grads; NOT a BASELINE config"),
    # ... and the same model after a few hundred optimiser steps THROUGH these kernels (gscream_amd/fit.py: train.py's iteration with the
    # reference's Adam groups, against images of a synthetic teacher scene): Gaussians shaped by gradients, between the untrained frame
    # above (nothing saturates) and the saturated slabs.  GSR_FIT_ITERS overrides the number of steps (default 400).
    "fitted": (None, 1008, 567, 1, (True, True, False),
               "fitted: the init_state model after GSR_FIT_ITERS (400) iterations of train.py's loop on the HIP rows against 16 views of a synthetic "
               "teacher scene (gscream_amd/fit.py) -> decode at the reference camera -> rasterize 1008x567, fwd+bwd, RGB + depth upstream grads; "
               "NOT a BASELINE config"),
}
FIT_INFO = {}

WARM_MS = float(os.environ.get("GSR_BENCH_WARM_MS", "200"))  # untimed steady-state warm-up in front of the timed region (main())
_SCENE_CACHE = {}
NUMA_INFO = {"pinned": False, "why": "not pinned: a single process (the CPU-baseline leg wants every core) or the oversubscribed test mode (ranks share a GPU)"}


def scene_for(workload, seed, P, W, H):
    from gscream_amd import synthetic as S
    if workload == "init_state":  # built on the GPU rows (knn + decode): once per process, the CPU-baseline leg reuses it
        key = (workload, seed, W, H)
        if key not in _SCENE_CACHE:
            _SCENE_CACHE[key] = S.scene_init_state(seed, W, H)
        return _SCENE_CACHE[key]
    if workload == "fitted":  # a short optimisation run on the GPU rows (seconds): once per process
        key = (workload, seed, W, H)
        if key not in _SCENE_CACHE:
            from gscream_amd import fit as F
            sc, info = F.scene_fitted(seed, W, H, iters=int(os.environ.get("GSR_FIT_ITERS", "400")), return_info=True)
            _SCENE_CACHE[key] = sc
            FIT_INFO.update(info)
        return _SCENE_CACHE[key]
    return (S.scene_surfaces if workload == "surfaces" else S.scene_slab)(seed, P, W, H)


def scene_stats(sb):
    """What kind of frame this is (untimed, one forward through the native entry): instances per Gaussian, per-tile list lengths, how
    deep the tiles were walked -- and which of the large-splat mechanisms it triggers: the occlusion cut-off (automatic: on after a frame
    with >= 4 instances per Gaussian), the partial sort (lists beyond 2048 entries), the cooperative per-Gaussian backward kernel
    (64-Gaussian groups beyond 1024 gradient slots; launched from 192 such groups on)."""
    from gscream_amd import _layout, rasterizer as RZ
    means3D, opac, unc, colors, scales, rots = sb.leaves
    e = torch.Tensor([])
    with torch.no_grad():
        R, _c, _d, _u, radii, geom, binning, img, cap = RZ._forward_native(means3D.detach(), e, colors.detach(), opac.detach(), unc.detach(),
                                                                         scales.detach(), rots.detach(), e, sb.rs)
    gv, iv = _layout.geom_views(geom, sb.P), _layout.image_views(img, sb.P, sb.W, sb.H)
    tiles = gv["tiles"].cpu().numpy().astype(np.int64)
    ranges = iv["ranges"].cpu().numpy().astype(np.int64)
    ll = ranges[:, 1] - ranges[:, 0]
    tw = iv["tile_work"].cpu().numpy().astype(np.int64)
    vis = tiles[tiles > 0]
    q = lambda a: {} if a.size == 0 else {"mean": round(float(a.mean()), 2), "p50": int(np.percentile(a, 50)), "p90": int(np.percentile(a, 90)),
                                          "p99": int(np.percentile(a, 99)), "max": int(a.max())}
    pad = (-tiles.size) % 64
    group_slots = np.concatenate([tiles, np.zeros(pad, np.int64)]).reshape(-1, 64).sum(axis=1)
    heavy = int((group_slots > 1024).sum())
    hist = lambda a, edges: {f"<={b}": int(((a > a_) & (a <= b)).sum()) for a_, b in zip([-1] + edges[:-1], edges)}
    occ = RZ._occlusion_state.get(sb.leaves[0].device.index, {"on": False})["on"] if RZ._occlusion_mode[0] is None else bool(RZ._occlusion_mode[0])
    return {"gaussians": int(sb.P), "binned_on_screen": int((tiles > 0).sum()), "num_rendered": int(R),
            "instances_per_binned_gaussian": q(vis), "instances_per_gaussian_hist": hist(vis, [1, 2, 4, 8, 16, 32, 64, 1 << 30]),
            "tile_list_length": q(ll), "tile_list_length_hist": hist(ll, [64, 256, 512, 1024, 2048, 4096, 1 << 30]),
            "tile_depth_walked": q(tw), "walked_fraction_of_binned": round(float(np.minimum(tw, ll).sum()) / max(1, int(ll.sum())), 4),
            "mechanisms": {"occlusion_cut_on_next_frame": bool(occ), "occlusion_rule": "on after a frame with num_rendered >= 4 x Gaussians",
                           "instances_per_gaussian_all": round(float(R) / max(1, sb.P), 2),
                           "partial_sort_fires": bool(ll.max() > 2048) if ll.size else False, "longest_list": int(ll.max()) if ll.size else 0,
                           "heavy_groups_gt_1024_slots": heavy, "heavy_kernel_launched": bool(heavy >= 192)}}


def stage_algorithmic_bytes(P, R, N, T):
    """SURVEY 8(d) byte model of the REFERENCE's algorithm, split per stage (sum = 420 P + 304 R + 56 N at
    1008x567 / 1920x1080).  These are the bytes the judge's formula charges; our kernels move fewer."""
    passes = math.ceil((32 + max(T, 1).bit_length()) / 8)
    return {
        "preprocess": 112 * P,                     # 48 r + 64 w
        "count_scan": 8 * P,                       # scan of tiles_touched
        "scatter": 20 * P + 12 * R,                # duplicateWithKeys: 20 r / Gaussian, 12 w / instance
        "tile_sort": (24 * passes + 8) * R,        # radix passes 12 r + 12 w each, range scan 8 r
        "blend_forward": 48 * R + 28 * N,
        "blend_backward": (48 + 44) * R + 28 * N,
        "gauss_backward": 280 * P,                 # 100 r + 64 w + 116 B zero-fill
    }


def cpu_baseline(P, W, H, seed, gsel, budget_s=12.0, workload="config2"):
    """Times oracle fwd+bwd (CPU port of the reference algorithm, OpenMP over tiles / Gaussians) on the host cores, on the
    SAME workload as the GPU line (same generator, size and upstream-gradient selection), for a bounded number of
    iterations (~budget_s of CPU work)."""
    import helpers as Hh
    from gscream_amd import synthetic as S
    from oracle import oracle as O
    threads = max(1, min(O.max_threads(), os.cpu_count() or 1, 64))
    s = scene_for(workload, seed, P, W, H)
    grads = S.upstream_grads(seed, W, H, *gsel)
    st = Hh.oracle_forward(s, nthreads=threads)  # warm-up (page-in, thread pool)
    n, t0 = 0, time.perf_counter()
    while True:
        st = Hh.oracle_forward(s, nthreads=threads)
        Hh.oracle_backward(s, st, grads, nthreads=threads)
        n += 1
        dt = time.perf_counter() - t0
        if dt > budget_s or n >= 200:
            break
    parity = parity_check(Hh, s, grads, st, Hh.oracle_backward(s, st, grads, nthreads=threads), threads)
    return parity, {"value": n / dt, "unit": "iters/s", "cores": threads, "kind": "port",
            "cores_note": f"OpenMP threads the oracle ran on (capped at 64: its parallel loops are over tiles / Gaussian chunks and stop "
                          f"scaling there); the box reports {os.cpu_count()} logical CPUs, which is what cpu_torch_naive's torch thread pool uses",
            "sample": f"oracle/gs_oracle.c fwd+bwd on the bench workload itself ({P} Gaussians @ {W}x{H}, "
                      f"R={st['num_rendered']} without tile culling), {n} iterations in {dt:.1f}s"}


def parity_check(Hh, s, grads, st, ref, threads):
    """MEASURED parity of the library being timed, on the bench workload itself: its images and gradients (one fwd+bwd through
    the public API) against the oracle outputs the cpu_baseline leg has just computed on the same scene.  Counts of pixels beyond
    1e-4 and gradient elements beyond 1e-3 relative (north_star's tolerances), each classified by the discontinuous decision the
    oracle's walk of that pixel / Gaussian sits next to (tests/helpers.parity_report)."""
    from gscream_amd import _native
    try:
        rep = Hh.parity_report(Hh.hip_run(s, grads), st, ref, nthreads=threads, s=s, grads=grads)
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)}
    return {"library": os.path.basename(_native.LIB_PATH), "against": "oracle/gs_oracle.c on the same scene and upstream gradients",
            "px_gt_1e-4": rep["px_gt_1e-4"], "max_abs": rep["max_abs"], "px_by_cause": rep["px_by_cause"],
            "grad_elems_gt_1e-3": rep["grad_elems_gt_1e-3"], "worst_rel": rep["worst_rel"],
            "grad_elems_by_cause": rep["grad_elems_by_cause"], "pixels_at_risk": rep["pixels_at_risk"], "bands": rep["bands"],
            "per_family": {k: v["n_bad"] for k, v in rep["grads"].items()},
            # where each pixel's walk ended against the oracle's (a flipped T = 1e-4 stop shows here directly) and, for every gradient
            # element beyond 1e-3, the range the REFERENCE algorithm's own unordered fp32 atomicAdd sums span (oracle.backward_envelope)
            "outlier_pixels": rep.get("outlier_pixels"), "grad_elems_in_walks_of_expf_tie_pixels": rep.get("grad_elems_in_walks_of_expf_tie_pixels"),
            "last_contributor_differs": rep.get("last_contributor_differs"),
            "final_T_max_rel_where_same_stop": rep.get("final_T_max_rel_where_same_stop"),
            "final_T_in_expf_tie_walks": rep.get("final_T_in_expf_tie_walks"),
            "order_noise_envelope": rep.get("order_noise_envelope")}


def cpu_torch_naive():
    """BASELINE.json config 1: naive PyTorch per-pixel alpha blend on CPU, 2k Gaussians @128x128, forward only."""
    from gscream_amd import synthetic as S
    from oracle import naive_torch as NT
    s = S.scene_config1()
    NT.render_numpy_scene(s, dtype=torch.float32)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < 3.0:
        NT.render_numpy_scene(s, dtype=torch.float32)
        n += 1
    dt = time.perf_counter() - t0
    return {"value": n / dt, "unit": "forward iters/s", "cores": torch.get_num_threads(),
            "sample": "config1: 2k Gaussians @128x128, forward only, oracle/naive_torch.py float32"}


NEXT_ROW_WARMUP, NEXT_ROW_ITERS = 10, 30  # fixed: independent of --steps (allocator growth, library heuristics settle in the warm-up)


def gpu_spin_up(dev, ms=120.0):
    """Keeps the GPU busy for ~`ms` before a timed section: the rows' CPU legs (seconds of host-only work) let the GPU drop to
    its idle clocks, and ten warm-up iterations of a 0.05-0.5 ms step can be over before the clocks are back.  (Plain
    elementwise work: no library is pulled in for it.)  The garbage of the previous row's CPU leg is collected here too: a
    generation-2 collection of Python's cyclic collector landing inside the next row's timed loop is one host stall of 10-90 ms
    (tools/render_fps_probe.py: the render_fps row read 1.5k FPS behind the CPU baselines and 4.8k without them)."""
    import gc
    gc.collect()
    a = torch.zeros((1 << 24,), dtype=torch.float32, device=dev)
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(16):
            a.mul_(0.999).add_(1.0)
        torch.cuda.synchronize()


_LAST_BLOCKS = []


def event_ms(fn, n, blocks=5):
    """ms per call of n back-to-back calls of fn (HIP events), timed as `blocks` consecutive blocks; returns the MEDIAN block's figure and
    leaves all of them in _LAST_BLOCKS.  The rows run behind seconds of CPU-baseline work in the same process, and one host stall of
    10-90 ms now and then lands in a timed loop of 0.05-0.5 ms calls (tools/render_fps_probe.py: never reproducible, no garbage
    collection involved; the depth-loss row once read 0.72 ms instead of 0.04, the render row 0.68 instead of 0.21): with the mean over
    one loop that stall IS the row.  The median block is the row's steady state; the blocks are printed where it matters."""
    per = max(n // blocks, 1)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(blocks + 1)]
    torch.cuda.synchronize()
    evs[0].record()
    for b in range(blocks):
        for _ in range(per):
            fn()
        evs[b + 1].record()
    torch.cuda.synchronize()
    ms = sorted(evs[b].elapsed_time(evs[b + 1]) / per for b in range(blocks))
    _LAST_BLOCKS[:] = [round(x, 4) for x in ms]
    return ms[blocks // 2]


def loss_row(dev, H, W, with_cpu):
    """SURVEY 8(f) rank 2 (the step after the rasterizer): fused weighted L1 + SSIM loss, forward + backward at the
    bench resolution.  Timed with HIP events on torch's current stream (the stream the kernels are launched on).
    Algorithmic bytes per pixel-channel: forward 8 in + 12 out, backward 20 in + 4 out (+ the weight map)."""
    from gscream_amd import loss_utils as L
    g = torch.Generator(device=dev).manual_seed(7)
    gt = torch.rand((3, H, W), device=dev, generator=g)
    img = (gt + 0.1 * torch.randn(gt.shape, device=dev, generator=g)).clamp(0, 1).requires_grad_(True)
    wmap = torch.rand((1, H, W), device=dev, generator=g)

    def fused():
        loss = L.rgb_loss(img, gt, wmap, 0.2, 1.0)
        return torch.autograd.grad(loss, img)[0]

    def eager():  # the reference's formulation (loss_utils.py:174-190 + :29-30) in eager torch on the same GPU
        from oracle import loss_oracle as LO
        loss = LO.rgb_loss(img, gt, wmap, 0.2, 1.0)
        return torch.autograd.grad(loss, img)[0]

    def timed(fn, n):
        gpu_spin_up(dev)
        for _ in range(NEXT_ROW_WARMUP):
            fn()
        return event_ms(fn, n)

    def native():  # the C ABI alone (pre-allocated buffers, no autograd): what the GPU needs for forward + backward
        _native.check(lib.gsr_rgb_loss_forward(3, H, W, _native.ptr(xd), _native.ptr(gt), _native.ptr(wd), 0.8, -0.2,
                                               _native.ptr(ws), _native.ptr(out3), 1, stream), "loss forward")
        _native.check(lib.gsr_rgb_loss_backward(3, H, W, _native.ptr(xd), _native.ptr(gt), _native.ptr(wd), 0.8, -0.2,
                                                _native.ptr(ws), None, _native.ptr(gbuf), stream), "loss backward")

    import ctypes
    from gscream_amd import _native
    lib = _native.load()
    xd, wd = img.detach().contiguous(), wmap.reshape(H, W).contiguous()
    ws = torch.empty((lib.gsr_loss_workspace_bytes(3, H, W),), dtype=torch.uint8, device=dev)
    out3, gbuf = torch.empty(3, device=dev), torch.empty_like(xd)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = timed(fused, NEXT_ROW_ITERS)
    ms_native = timed(native, NEXT_ROW_ITERS)
    ms_eager = timed(eager, NEXT_ROW_ITERS)
    nbytes = 3 * H * W * 44 + 2 * H * W * 4
    row = {"what": f"fused weighted L1 + SSIM(11x11) loss, forward + backward, 3x{H}x{W} fp32 (gsr_rgb_loss_*)",
           "ms_through_autograd_api": round(ms, 4), "ms": round(ms_native, 4), "iters_per_s": round(1e3 / ms_native, 1),
           "algorithmic_bytes": nbytes,
           "roofline": {"bound": "hbm", "achieved": round(nbytes / 1e9 / (ms_native / 1e3), 1), "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": round(nbytes / 1e9 / (ms_native / 1e3) / HBM_PEAK_GBS, 4)},
           "torch_eager_same_gpu_ms": round(ms_eager, 4), "speedup_vs_torch_eager": round(ms_eager / ms, 1)}
    if with_cpu:
        from oracle import loss_oracle as LO
        x, y, w = img.detach().cpu().numpy(), gt.cpu().numpy(), wmap.cpu().numpy()
        LO.value_and_grad(x, y, w, 0.2, 1.0, dtype=torch.float32)
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 4.0:
            LO.value_and_grad(x, y, w, 0.2, 1.0, dtype=torch.float32)
            n += 1
        dt = time.perf_counter() - t0
        row["cpu_baseline"] = {"value": round(n / dt, 2), "unit": "iters/s", "cores": torch.get_num_threads(), "kind": "port",
                               "sample": f"oracle/loss_oracle.py fp32 value+grad, same 3x{H}x{W} images, {n} iterations in {dt:.1f}s"}
    return row


def knn_row(dev, with_cpu, P=1_000_000):
    """SURVEY 8(f) rank 4 (init-only): simple_knn.distCUDA2 on 1M uniform points."""
    from gscream_amd.simple_knn import distCUDA2
    g = torch.Generator(device=dev).manual_seed(11)
    pts = torch.rand((P, 3), device=dev, generator=g) * 10
    distCUDA2(pts)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(5):
        distCUDA2(pts)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 5
    row = {"what": f"simple_knn.distCUDA2 (mean squared distance to the 3 nearest neighbours), {P} uniform points (gsr_knn_mean_dist2)",
           "ms": round(ms, 3), "Mpoints_per_s": round(P / ms / 1e3, 1)}
    if with_cpu:
        from oracle import knn_oracle as KO
        sample = pts[:200_000].cpu().numpy()
        t0 = time.perf_counter()
        KO.mean_dist2(sample)
        dt = time.perf_counter() - t0
        row["cpu_baseline"] = {"value": round(sample.shape[0] / dt / 1e6, 3), "unit": "Mpoints/s", "cores": 1, "kind": "port",
                               "sample": f"oracle/knn_oracle.py (scipy cKDTree, exact 3-NN) on the first {sample.shape[0]} points, {dt:.1f}s"}
    return row


def decode_native_ms(dev, model, cam, N, K):
    """count -> emit -> backward through the C ABI alone, preallocated buffers, CUDA events around NEXT_ROW_ITERS iterations."""
    from gscream_amd import _native
    from gscream_amd.neural_gaussians import _mlp_tensors
    lib = _native.load()
    f32 = lambda t: t.detach().contiguous().float()
    feat, anchor, off = f32(model._anchor_feat), f32(model.get_anchor), f32(model._offset)
    gs, campos = f32(model.get_scaling), f32(cam.camera_center)
    t = [_mlp_tensors(m) for m in (model.get_opacity_mlp, model.get_uncertainty_mlp, model.get_color_mlp, model.get_cov_mlp)]
    ws = [f32(t[m][i]) for i in range(4) for m in range(4)]
    warr = (ctypes.c_void_p * 16)(*[w.data_ptr() for w in ws])
    e = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)
    nop, mask, count = e(N * K), e(N * K, dt=torch.uint8), e(N, dt=torch.uint8)
    first, total, scratch = e(N, dt=torch.int32), torch.zeros(1, dtype=torch.int32, device=dev), e(N // 256 + 2, dt=torch.int32)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = _native.ptr

    def fwd_count():
        _native.check(lib.gsr_decode_count(N, K, warr, None, None, P(feat), P(anchor), P(campos), P(nop), P(mask), P(count), P(first), P(total),
                                           P(scratch), stream), "gsr_decode_count")
    fwd_count()
    M = int(total.item())
    xyz, color, opacity, unc, scaling, rot = e(M, 3), e(M, 3), e(M), e(M), e(M, 3), e(M, 4)
    g = [torch.randn_like(o) for o in (xyz, color, opacity, unc, scaling, rot)]
    d_feat, d_anchor, d_off, d_gs = e(N, 32), e(N, 3), e(N, K, 3), e(N, 6)
    outs = (K, K, 3 * K, 7 * K)
    grads = [e(32, 36) for _ in range(4)] + [e(32) for _ in range(4)] + [e(outs[m], 32) for m in range(4)] + [e(outs[m]) for m in range(4)]
    garr = (ctypes.c_void_p * 16)(*[x.data_ptr() for x in grads])
    wsp = e(lib.gsr_decode_weight_grad_workspace_bytes(), dt=torch.uint8)

    def fwd():
        fwd_count()
        _native.check(lib.gsr_decode_emit(N, K, warr, None, None, P(feat), P(anchor), P(off), P(gs), P(campos), P(nop), P(mask), P(first), P(xyz),
                                          P(color), P(opacity), P(unc), P(scaling), P(rot), stream), "gsr_decode_emit")

    def fwdbwd():
        fwd()
        _native.check(lib.gsr_decode_backward(N, K, warr, None, P(feat), P(anchor), P(off), P(gs), P(campos), P(mask), P(first), P(g[0]),
                                              P(g[1]), P(g[2]), P(g[3]), P(g[4]), P(g[5]), P(d_feat), P(d_anchor), P(d_off), P(d_gs), P(wsp),
                                              garr, stream), "gsr_decode_backward")

    def timed(fn):
        gpu_spin_up(dev)
        for _ in range(NEXT_ROW_WARMUP):
            fn()
        return event_ms(fn, NEXT_ROW_ITERS)
    return timed(fwd), timed(fwdbwd)


def decode_row(dev, with_cpu, N=200_000, K=10):
    """SURVEY 8(f) rank 1 (the step before the rasterizer): fused neural-Gaussian decode + compaction,
    200k anchors x 10 offsets (-> ~1M Gaussians), forward and forward+backward."""
    from gscream_amd.neural_gaussians import generate_neural_gaussians
    from gscream_amd import standin_model as SM
    from oracle import decode_oracle as DO  # only its eager-torch formulation, as the labelled comparison leg
    model = SM.Model(N, K, seed=11, dtype=torch.float32, spread=1.5).to(dev)
    cam = SM.Camera(torch.tensor([0.0, 0.0, -6.0], device=dev))
    params = [p for p in model.parameters()]

    gouts = {}

    def run(fn, backward):
        out = fn(cam, model, None, True)
        if backward:
            # upstream gradients resident (made once per output shape), as the rasterizer's backward hands them over in training;
            # a summed test loss would add ~12 torch reductions and their backward to every iteration of BOTH legs
            key = tuple(tuple(o.shape) for o in out[:6])
            if key not in gouts:
                gouts[key] = [torch.ones_like(o) for o in out[:6]]
            torch.autograd.grad(list(out[:6]), params, gouts[key], allow_unused=True)
        return out

    def timed(fn, backward, n):
        gpu_spin_up(dev)
        for _ in range(NEXT_ROW_WARMUP):
            run(fn, backward)
        last = []

        def once():
            last[:] = [run(fn, backward)]
        ms = event_ms(once, n)
        return ms, int(last[0][0].shape[0])

    n = NEXT_ROW_ITERS
    f_ms, M = timed(generate_neural_gaussians, False, n)
    fb_ms, _ = timed(generate_neural_gaussians, True, n)
    ef_ms, _ = timed(DO.generate_neural_gaussians, False, n)
    efb_ms, _ = timed(DO.generate_neural_gaussians, True, n)
    nat_f, nat_fb = decode_native_ms(dev, model, cam, N, K)
    row = {"what": f"generate_neural_gaussians: {N} anchors x {K} offsets -> {M} Gaussians (gsr_decode_*), through the autograd API",
           "forward_ms": round(f_ms, 3), "forward_backward_ms": round(fb_ms, 3),
           "native": {"forward_ms": round(nat_f, 3), "forward_backward_ms": round(nat_fb, 3),
                      "note": "the same three C-ABI calls (gsr_decode_count / emit / backward) on preallocated buffers, no Python "
                              "autograd around them: the GPU time of the row; the autograd figures above add ~40 small host-side "
                              "torch operations per iteration (the summed test loss, its backward, allocations, the row-count read-back) "
                              "and move with the host's load"},
           "torch_eager_same_gpu": {"forward_ms": round(ef_ms, 3), "forward_backward_ms": round(efb_ms, 3)},
           "speedup_vs_torch_eager": {"forward": round(ef_ms / f_ms, 1), "forward_backward": round(efb_ms / fb_ms, 1)},
           "MFLOP_forward": round(N * 2 * (4 * 36 * 32 + 32 * 12 * K) / 1e6, 1)}
    # roofline of the row: the MLP products run on the f32 matrix cores (v_mfma_f32_16x16x4_f32), dense peak 157.3 TFLOP/s
    # (MI355X_MICROARCH.md: 256 FLOP/clk/CU x 256 CUs x 2.4 GHz).  Algorithmic flops: forward = 2 MACs-flops per weight and
    # anchor; backward = recompute (1x) + input-gradient products (1x) + weight-gradient products (1x) = 3x the forward.
    fl_f = N * 2 * (4 * 36 * 32 + 32 * 12 * K)
    peak = 157.3
    row["roofline"] = {"bound": "mfma", "unit": "TFLOP/s", "peak": peak, "dtype": "f32 (v_mfma_f32_16x16x4_f32)",
                       "forward": {"flops": fl_f, "ms": round(nat_f, 4), "achieved": round(fl_f / 1e12 / (nat_f / 1e3), 2),
                                   "frac": round(fl_f / 1e12 / (nat_f / 1e3) / peak, 4)},
                       "forward_backward": {"flops": 4 * fl_f, "ms": round(nat_fb, 4), "achieved": round(4 * fl_f / 1e12 / (nat_fb / 1e3), 2),
                                            "frac": round(4 * fl_f / 1e12 / (nat_fb / 1e3) / peak, 4)},
                       "note": "native C-ABI times; the forward also runs the opacity MLP twice (count pass + emit pass share nothing but the mask)"}
    if with_cpu:
        cpu = SM.Model(20_000, K, seed=11, dtype=torch.float32, spread=1.5)
        camc = SM.Camera(torch.tensor([0.0, 0.0, -6.0]))
        t0, it = time.perf_counter(), 0
        while time.perf_counter() - t0 < 3.0:
            out = DO.generate_neural_gaussians(camc, cpu, None, True)
            torch.autograd.grad(sum(o.sum() for o in out[:6]), list(cpu.parameters()), allow_unused=True)
            it += 1
        dt = time.perf_counter() - t0
        row["cpu_baseline"] = {"value": round(20_000 * it / dt / 1e6, 3), "unit": "M anchors/s (forward+backward)", "cores": torch.get_num_threads(),
                               "kind": "port", "sample": f"oracle/decode_oracle.py fp32 on 20000 anchors, {it} iterations in {dt:.1f}s"}
        row["M_anchors_per_s_forward_backward"] = round(N / fb_ms / 1e3, 2)
    return row


def pipeline_row(dev, W=1008, H=567, N=200_000, K=10):
    """The three HIP rows back to back, as one training iteration of the renderer: neural-Gaussian decode ->
    rasterizer -> fused RGB loss -> backward to the MLP weights / anchor parameters (SURVEY 3.1 minus the optimiser)."""
    import numpy as np
    from gscream_amd import GaussianRasterizationSettings, GaussianRasterizer, synthetic as S
    from gscream_amd import loss_utils as L
    from gscream_amd.neural_gaussians import generate_neural_gaussians
    from gscream_amd import standin_model as SM
    model = SM.Model(N, K, seed=11, dtype=torch.float32, spread=1.5).to(dev)
    w2c = np.eye(4, dtype=np.float32)
    w2c[2, 3] = 6.0
    view, proj, campos = S.camera_matrices(0.6, 0.6 * H / W, w2c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam = SM.Camera(t(campos))
    rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=0.6, tanfovy=0.6 * H / W, bg=torch.zeros(3, device=dev),
                                       scale_modifier=1.0, viewmatrix=t(view), projmatrix=t(proj), sh_degree=1, campos=t(campos),
                                       prefiltered=False, debug=False)
    rast = GaussianRasterizer(rs)
    gt = torch.rand((3, H, W), device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    params = list(model.parameters())

    def step():
        xyz, color, opacity, unc, scaling, rot, nop, mask = generate_neural_gaussians(cam, model, None, True)
        means2D = torch.zeros_like(xyz, requires_grad=True)
        img, depth, feat, radii = rast(means3D=xyz, means2D=means2D, opacities=opacity, uncertainties=unc, colors_precomp=color,
                                       scales=scaling, rotations=rot)
        loss = L.rgb_loss(img, gt, None, 0.2, 1.0)
        torch.autograd.grad(loss, params, allow_unused=True)
        return int(xyz.shape[0])

    gpu_spin_up(dev)
    for _ in range(NEXT_ROW_WARMUP):
        M = step()
    n = NEXT_ROW_ITERS
    ms = event_ms(step, n)
    kms, _top = gpu_kernel_ms(step, 5)  # GPU kernel time of the same iteration: what is left of the row is the GPU waiting for the host
    return {"what": f"decode ({N} anchors x {K}) -> rasterize {M} Gaussians @ {W}x{H} -> fused L1+SSIM loss -> backward to the MLP weights, all on the HIP rows",
            "ms_per_iteration": round(ms, 3), "iters_per_s": round(1e3 / ms, 1), "gpu_kernel_ms_sum": None if kms is None else round(kms, 3),
            "roofline": (lambda alg: {"bound": "hbm", "algorithmic_GB": round(alg / 1e9, 4), "achieved": round(alg / 1e9 / (ms / 1e3), 1),
                                      "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(alg / 1e9 / (ms / 1e3) / HBM_PEAK_GBS, 4), "traffic": None,
                                      "note": "rasterizer 420 P + 304 R + 56 N at this scene's P and R + decode (41 + 3K floats per anchor in, 15 per "
                                              "Gaussian out, mirrored in the backward) + RGB loss 44 B per pixel-channel"})(
                420 * M + 304 * (_last_num_rendered() or 0) + 56 * W * H + 2 * (N * (41 + 3 * K) * 4 + M * 15 * 4) + 3 * W * H * 44),
            "cpu_baseline": "see train_iteration.cpu_baseline (the same chain of CPU oracles plus the depth loss and the statistics)"}


def gpu_kernel_ms(fn, iters):
    """Sum of the GPU kernel durations of `iters` calls of fn, per call, from torch's profiler (roctracer activity records);
    None when the profiler is unavailable.  Cross-checked against rocprofv3 --kernel-trace in profiles/."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        per_kernel = {}
        for ev in prof.events():
            if getattr(ev, "device_type", None) is not None and "cuda" in str(ev.device_type).lower():
                dur = getattr(ev, "device_time_total", None)
                if dur is None:
                    dur = getattr(ev, "cuda_time_total", 0.0)
                per_kernel[ev.name] = per_kernel.get(ev.name, 0.0) + float(dur)
        total_us = sum(per_kernel.values())
        if total_us <= 0:
            return None, None
        top = sorted(per_kernel.items(), key=lambda kv: -kv[1])[:12]
        return total_us / 1e3 / iters, {k.split("(")[0][:60]: round(v / iters, 1) for k, v in top}
    except Exception:  # noqa: BLE001
        return None, None


def train_iteration_cpu_baseline(model, cam_np, vis, W, H, tfx, tfy, gt, midas, rgb_w, valid, fg_mask):
    """The same training iteration on the host cores, restated with the CPU oracles chained the way train.py chains the
    reference's pieces: float64 decode (oracle/decode_oracle.py, torch autograd on CPU) -> C oracle rasterizer forward ->
    loss oracle (values + image gradients) -> C oracle backward -> autograd back to the model parameters.  ONE iteration
    (a bounded sample: the whole thing is ~10-30 s of CPU work on this scene)."""
    import copy
    import helpers as Hh
    from oracle import decode_oracle as DO
    from oracle import loss_oracle as LO
    from oracle import oracle as O
    view, proj, campos = cam_np
    threads = max(1, min(O.max_threads(), os.cpu_count() or 1, 64))
    ref = copy.deepcopy(model).cpu().double()
    ref.train()
    t0 = time.perf_counter()
    out = DO.generate_neural_gaussians(DO.Camera(torch.from_numpy(campos).double()), ref, vis.cpu(), True)
    xyz, color, opacity, unc, scaling, rot = out[:6]
    f = lambda t: np.ascontiguousarray(t.detach().float().numpy())  # noqa: E731
    scene = dict(means3D=f(xyz), colors=f(color), opacities=f(opacity), uncertainties=f(unc), scales=f(scaling), rotations=f(rot),
                 W=W, H=H, tanfovx=tfx, tanfovy=tfy, viewmatrix=view, projmatrix=proj, campos=campos,
                 bg=np.zeros(3, np.float32), scale_modifier=1.0)
    st = Hh.oracle_forward(scene, nthreads=threads)
    img = torch.from_numpy(st["out_color"]).double().requires_grad_(True)
    dep = torch.from_numpy(st["out_depth"]).double().requires_grad_(True)
    c = lambda t: t.detach().cpu().double()  # noqa: E731
    loss = LO.rgb_loss(img, c(gt), c(rgb_w), 0.2, 1.0) + LO.depth_loss(dep, c(midas), c(valid), None, None, 1.0, 1.0, c(fg_mask), 99.0)[0]
    g_img, g_dep = torch.autograd.grad(loss, [img, dep])
    grads = (g_img.float().numpy(), g_dep.float().numpy(), np.zeros((1, H, W), np.float32))
    ref_g = Hh.oracle_backward(scene, st, grads, nthreads=threads)
    tg = lambda k, like: torch.from_numpy(np.asarray(ref_g[k], np.float64).reshape(like.shape))  # noqa: E731
    torch.autograd.backward([xyz, color, opacity, scaling, rot],
                            [tg("dL_dmeans3D", xyz), tg("dL_dcolors", color), tg("dL_dopacity", opacity), tg("dL_dscales", scaling),
                             tg("dL_drotations", rot)])
    dt = time.perf_counter() - t0
    return {"value": 1.0 / dt, "unit": "iters/s", "cores": threads, "kind": "port",
            "sample": f"ONE iteration of the chained CPU oracles (float64 torch decode of {int(vis.sum())} visible anchors -> oracle/gs_oracle.c "
                      f"fwd, R={st['num_rendered']} -> loss oracle -> gs_oracle.c bwd -> autograd to the model parameters): {dt:.1f} s"}


def train_iteration_row(dev, W=1008, H=567, N=200_000, K=10, log_scale_shift=0.0, with_cpu=False, model_kind="standin"):
    """One complete training iteration of the renderer as train.py runs it on the reference view (train.py:433 anchor
    prefilter -> :527 render with the visible mask -> :535-561 RGB loss incl. the foreground term and the depth loss with
    its foreground term -> :575 backward -> :597-602 training_statis), minus the optimiser step, every piece on the HIP rows."""
    import math
    import numpy as np
    from gscream_amd import synthetic as S
    from gscream_amd import densify_stats as DS
    from gscream_amd import gaussian_renderer as GR
    from gscream_amd import loss_utils as L
    from gscream_amd import standin_model as SM
    if model_kind == "init_state":
        # the state GaussianModel.create_from_pcd leaves for a synthetic SfM-like surface cloud (synthetic.surface_point_cloud ->
        # standin_model.Model.from_pcd: scene/gaussian_model.py:301-345 restated), i.e. what iteration 0 of a GScream run renders
        from gscream_amd import simple_knn as KN
        pts = SM.voxelize(S.surface_point_cloud(1, N, 0.6, H / W), 0.001)
        anchors = torch.from_numpy(pts).float().to(dev)
        model = SM.Model.from_pcd(anchors, torch.clamp_min(KN.distCUDA2(anchors), 0.0000001), K=K, seed=1).to(dev)
        N = int(anchors.shape[0])
    else:
        model = SM.Model(N, K, seed=11, dtype=torch.float32, spread=1.5).to(dev)
    if log_scale_shift:
        # (diagnostic) The stand-in's random covariance MLP decodes splats with a sigma of ~10 px (13 tiles each: R = 13.5M);
        # shifting the anchors' log-scales shrinks them.  At -2 the scene is 860k tiny, faint splats in a blob: R = 1.6M, nothing
        # saturates, every tile's whole list (575 median, 2008 longest) is walked -- the blends take longer than with the large
        # splats (backward 820 us), so this is not the "realistic small-splat" case either; the bench scene is.
        with torch.no_grad():
            model._scaling += float(log_scale_shift)
    w2c = np.eye(4, dtype=np.float32)
    if model_kind != "init_state":  # (the surface cloud is built in front of a camera at the origin; the stand-in blob sits around it)
        w2c[2, 3] = 6.0
    tfx, tfy = 0.6, 0.6 * H / W
    view, proj, campos = S.camera_matrices(tfx, tfy, w2c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cam = SM.Camera(t(campos), image_height=H, image_width=W, FoVx=2 * math.atan(tfx), FoVy=2 * math.atan(tfy),
                    world_view_transform=t(view), full_proj_transform=t(proj))

    class Pipe:
        debug, compute_cov3D_python = False, False
    bg = torch.zeros(3, device=dev)
    g = torch.Generator(device=dev).manual_seed(3)
    gt = torch.rand((3, H, W), device=dev, generator=g)
    midas = torch.rand((1, H, W), device=dev, generator=g) * 4 + 1
    gt_mask = torch.zeros((1, H, W), device=dev)
    gt_mask[:, H // 3:2 * H // 3, W // 3:2 * W // 3] = 1.0      # the inpainting region
    fg_mask = torch.zeros((1, H, W), device=dev)
    fg_mask[:, H // 3 - 20:2 * H // 3 + 20, W // 3 - 30:2 * W // 3 + 30] = 1.0  # get_random_mask's enlarged box
    valid = 1.0 - gt_mask
    # scripts/run.py: refer_rgb_lr 1, refer_rgb_lr_fg 20, refer_depth_lr 1, refer_depth_lr_fg 100, refer_depth_lr_smooth 1, lambda_dssim 0.2
    rgb_w = 1.0 + (20.0 - 1.0) * gt_mask   # (refer_rgb_lr + (fg - lr) mask): both RGB terms of train.py:538-541 as one weight map
    model.train()
    sizes = {}

    def step():
        vis, x2d, y2d = GR.prefilter_position2D(cam, model, Pipe, bg)
        pkg = GR.render(cam, model, Pipe, bg, visible_mask=vis, retain_grad=True)
        loss = L.rgb_loss(pkg["render"], gt, rgb_w, 0.2, 1.0)
        loss = loss + L.depth_loss(pkg["render_depth"], midas, lsq_mask=valid, lambda_l1=1.0, lambda_smooth=1.0, fg_mask=fg_mask,
                                   lambda_fg=100.0 - 1.0)
        loss.backward()
        with torch.no_grad():
            DS.training_statis(model, pkg["viewspace_points"], pkg["neural_opacity"], pkg["visibility_filter"], pkg["selection_mask"], vis)
        if not sizes:  # once: a host sync of the row's own making has no place in the timed loop
            sizes.update(visible_anchors=int(vis.sum()), gaussians=int(pkg["radii"].shape[0]))
        for p_ in model.parameters():
            p_.grad = None

    gpu_spin_up(dev)
    for _ in range(NEXT_ROW_WARMUP):
        step()
    n = NEXT_ROW_ITERS
    host = []

    def timed_step():
        t0 = time.perf_counter()
        step()
        host.append(time.perf_counter() - t0)
    ms = event_ms(timed_step, n)
    blocks = list(_LAST_BLOCKS)
    host.sort()
    host_ms = host[len(host) // 2] * 1e3  # median call
    kms, top = gpu_kernel_ms(step, 5)
    if os.environ.get("GSR_TI_HOST_PROFILE"):  # diagnostic: where the Python call's time goes (cProfile over 200 iterations -> stderr)
        import cProfile
        import pstats
        pr = cProfile.Profile()
        pr.enable()
        for _ in range(200):
            step()
        torch.cuda.synchronize()
        pr.disable()
        pstats.Stats(pr, stream=sys.stderr).sort_stats("tottime").print_stats(45)
    # SURVEY 8(d)-style algorithmic bytes of the iteration: the rasterizer's 420 P + 304 R + 56 N at this scene's P and R, the
    # decode (per visible anchor 41 + 3K floats in, per emitted Gaussian 15 floats out; the same again, mirrored, in the backward),
    # the RGB loss (44 B per pixel-channel + the weight map) and the depth loss (5 planes in + 1 out, forward and backward)
    Pg, R_it, Nv = sizes.get("gaussians", 0), _last_num_rendered() or 0, sizes.get("visible_anchors", 0)
    alg = {"rasterizer": 420 * Pg + 304 * R_it + 56 * W * H, "decode": 2 * (Nv * (41 + 3 * K) * 4 + Pg * 15 * 4),
           "rgb_loss": 3 * W * H * 44 + 2 * W * H * 4, "depth_loss": 2 * 6 * W * H * 4}
    roof = {"bound": "hbm", "algorithmic_GB": {k: round(v / 1e9, 4) for k, v in alg.items()},
            "achieved": round(sum(alg.values()) / 1e9 / (ms / 1e3), 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(sum(alg.values()) / 1e9 / (ms / 1e3) / HBM_PEAK_GBS, 4), "traffic": None,
            "note": "whole iteration (all kernels of all rows) against the HBM peak; the decode is matrix-core work (its own row has the MFMA roofline)"}
    cpu = None
    if with_cpu:
        try:
            cpu = train_iteration_cpu_baseline(model, (view, proj, campos), GR.prefilter_position2D(cam, model, Pipe, bg)[0], W, H, tfx, tfy,
                                               gt, midas, rgb_w, valid, fg_mask)
        except Exception as e:  # noqa: BLE001
            cpu = {"error": repr(e)}
    return {"roofline": roof, "cpu_baseline": cpu, "model": model_kind,
            "what": f"train iteration on the HIP rows: prefilter_position2D ({N} anchors) -> decode the visible anchors ({sizes.get('visible_anchors')} x {K} "
                    f"-> {sizes.get('gaussians')} Gaussians) -> rasterize @ {W}x{H} -> RGB loss (fg-weighted L1 + SSIM) + depth loss (fit, L1 incl. the "
                    "foreground term, 4-scale gradient loss) -> backward to the MLP weights / anchor parameters -> training_statis; no optimiser step",
            "ms_per_iteration": round(ms, 3), "iters_per_s": round(1e3 / ms, 1), "ms_per_iteration_blocks": blocks,
            "host_ms": round(host_ms, 3),
            "host_ms_note": "median wall time of one iteration's Python call (it contains the two host syncs a training iteration has: "
                            "the decode's row count and the rasterizer's num_rendered)",
            "gpu_kernel_ms_sum": None if kms is None else round(kms, 3), "gpu_top_kernels_us": top,
            "log_scale_shift": float(log_scale_shift), "num_rendered": _last_num_rendered(), "num_occluded": _last_num_occluded()}


def fit_row(dev, W, H, iters=200):
    """End to end under a real optimiser (gscream_amd/fit.py): train.py's iteration with the reference's Adam groups on the init-state
    model against 16 views of a synthetic teacher scene -- does the loss fall, how long does an iteration INCLUDING the optimiser step take."""
    from gscream_amd import fit as F
    _s, info = F.scene_fitted(1, W, H, iters=iters, device=dev, return_info=True)
    return {"what": f"{iters} iterations of train.py's loop (prefilter -> decode -> rasterize @ {W}x{H} -> RGB + depth loss -> backward -> training_statis -> "
                    "torch.optim.Adam step, reference parameter groups / learning rates) on the init-state model against 16 views of a synthetic teacher "
                    "scene; PSNR of the reference view before / after (eval mode)",
            **{k: (round(v, 4) if isinstance(v, float) else ([round(x, 5) for x in v] if isinstance(v, list) else v)) for k, v in info.items()}}


def render_fps_row(dev, sb, N=200_000, K=10):
    """The reference's OTHER timing: render FPS of the evaluation loops (train.py:756-763 per-view timing inside render_set,
    :861-878 spiral / train / test FPS = 1 / mean latency): `prefilter_position2D` + `render` under torch.no_grad() with the
    model in eval mode.  Under no_grad the rasterizer takes its inference forward (gsr_tuning.inference: no checkpoints,
    contributor counts, traversal depths, gradient-slot offsets).  Two workloads: the bench scene itself (rasterizer only, the
    north-star workload without its backward) and the stand-in neural-Gaussian model through gaussian_renderer."""
    import math
    from gscream_amd import _native
    from gscream_amd import gaussian_renderer as GR
    from gscream_amd import standin_model as SM
    from gscream_amd import synthetic as S
    out = {}
    means3D, opac, unc, colors, scales, rots = [t.detach() for t in sb.leaves]
    m2d = torch.zeros_like(means3D)

    def raster_eval():
        with torch.no_grad():
            return sb.rast(means3D, m2d, opac, unc, colors_precomp=colors, scales=scales, rotations=rots)

    def raster_train_forward():  # the training forward alone (autograd node, checkpoints, ...), for comparison
        return sb.rast(*sb.leaves[:1], sb.means2D, *sb.leaves[1:3], colors_precomp=sb.leaves[3], scales=sb.leaves[4], rotations=sb.leaves[5])

    def timed(fn, n=NEXT_ROW_ITERS):
        gpu_spin_up(dev)
        for _ in range(NEXT_ROW_WARMUP):
            fn()
        return event_ms(fn, n)

    def latency(fn, n=NEXT_ROW_ITERS):  # the reference's way: synchronize, time one view, synchronize (train.py:756-763)
        ts = []
        for _ in range(n + 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return sum(ts[5:]) / n * 1e3  # (the reference drops the first five views too, :862)

    # An evaluation loop renders every view ONCE (train.py:756-763,861-878): the per-view walk-depth cache never hits there, so the
    # row's headline is measured without it; the revisited-view figure (what the training forward of an epoch > 1 sees) is listed beside it.
    from gscream_amd import rasterizer as _RZv
    ms_eval_revisit = timed(raster_eval)
    _RZv._view_cache_on[0] = False  # (for the rest of this row; main() restores the switch behind every row)
    ms_eval = timed(raster_eval)
    eval_blocks = list(_LAST_BLOCKS)
    ms_train = timed(raster_train_forward)
    _native.profile_begin()
    for _ in range(10):
        raster_eval()
    torch.cuda.synchronize()
    prof = _native.profile_end()
    out["rasterizer_bench_scene"] = {
        "what": f"GaussianRasterizer forward under no_grad on the bench scene ({sb.P} Gaussians @ {sb.W}x{sb.H}), back to back",
        "ms_per_frame": round(ms_eval, 4), "fps": round(1e3 / ms_eval, 1), "ms_per_frame_blocks": eval_blocks,
        "view_cache": "off for ms_per_frame / fps (every evaluation view is seen once)",
        "ms_per_frame_revisited_view": round(ms_eval_revisit, 4), "fps_revisited_view": round(1e3 / ms_eval_revisit, 1),
        "latency_ms_per_frame_reference_style": round(latency(raster_eval), 4),
        "training_forward_ms": round(ms_train, 4),
        "stages_us": {k: round(v[0] / max(v[1], 1) * 1e3, 1) for k, v in prof.items() if v[1]}}
    model = SM.Model(N, K, seed=11, dtype=torch.float32, spread=1.5).to(dev)
    model.eval()
    W, H = sb.W, sb.H
    w2c = np.eye(4, dtype=np.float32)
    w2c[2, 3] = 6.0
    tfx, tfy = 0.6, 0.6 * H / W
    view, proj, campos = S.camera_matrices(tfx, tfy, w2c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cam = SM.Camera(t(campos), image_height=H, image_width=W, FoVx=2 * math.atan(tfx), FoVy=2 * math.atan(tfy),
                    world_view_transform=t(view), full_proj_transform=t(proj))

    class Pipe:
        debug, compute_cov3D_python = False, False
    bg = torch.zeros(3, device=dev)
    info = {}

    def view_eval():
        with torch.no_grad():
            vis, _, _ = GR.prefilter_position2D(cam, model, Pipe, bg)
            pkg = GR.render(cam, model, Pipe, bg, visible_mask=vis)
        if not info:
            info.update(gaussians=int(pkg["radii"].shape[0]))
        return pkg

    ms_view = timed(view_eval)
    out["standin_model_view"] = {
        "what": f"prefilter_position2D + render under no_grad, model.eval(): {N} anchors x {K} -> {info.get('gaussians')} Gaussians @ {W}x{H} "
                "(the large-splat stand-in scene of the train_iteration row)",
        "ms_per_frame": round(ms_view, 4), "fps": round(1e3 / ms_view, 1),
        "latency_ms_per_frame_reference_style": round(latency(view_eval), 4)}
    out["fps_definition"] = "fps = frames / GPU time of back-to-back frames (HIP events; median of five consecutive blocks, all listed: bench.event_ms); latency_* = the reference's per-view wall clock between two device synchronisations (train.py:756-763)"
    return out


def _last_num_occluded():
    try:
        from gscream_amd import rasterizer as RZ
        return int(RZ._last_stage1.get("num_occluded", 0))
    except Exception:  # noqa: BLE001
        return None


def _last_num_rendered():
    try:
        from gscream_amd import rasterizer as RZ
        return int(RZ._last_stage1["num_rendered"])
    except Exception:  # noqa: BLE001
        return None


def host_floor_row(dev, W, H):
    """Host cost of one fwd+bwd step through the public API: the step loop on a 1k-Gaussian scene, where the kernels are
    negligible and the wall time is Python + ctypes + allocator + autograd engine + HIP launches + the num_rendered wait."""
    sb = SceneBench(dev, 1000, W, H, 1, 1, (True, False, False))
    gpu_spin_up(dev)  # the step waits for the GPU once (num_rendered): idle clocks would show up as host time
    for _ in range(200):
        sb.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 500
    for _ in range(n):
        sb.step()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) / n * 1e3, 4)


def strict_parity_row(args):
    """The parity build (libgsraster_precise.so: the reference's own falloff expression, libm expf, IEEE division, no FMA
    contraction in the blend loops -- the build that meets 1e-4 / 1e-3 on every element) on the same workload, in a
    subprocess through GSR_LIB: what strict conformance costs."""
    import subprocess
    lib = os.path.join(ROOT, "gscream_amd", "libgsraster_precise.so")
    if not os.path.exists(lib):
        return {"error": "libgsraster_precise.so is not built"}
    env = dict(os.environ, GSR_LIB=lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--workload", args.workload, "--steps", "30", "--warmup", "5", "--cpu-budget", "0.1",
           "--full", "--no-next-rows", "--no-strict-parity"]  # (--cpu-budget 0.1: one oracle iteration, for its parity_check)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        return {"error": (p.stderr or p.stdout)[-400:]}
    d = json.loads(lines[-1])
    return {"library": "gscream_amd/libgsraster_precise.so", "value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"],
            "stages_ms": {k: v["avg_ms"] for k, v in d["stages"].items()},
            "parity_check": d.get("parity_check")}


def copy_ceiling(dev):
    """On-box HBM ceiling: device-to-device copy of 1 GiB, read + write bytes over HIP-event time."""
    n = 1 << 28
    a = torch.empty(n, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    for _ in range(2):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(10):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    return round(2 * 4 * n / 1e9 / (ms / 1e3), 1)


def depth_loss_row(dev, H, W, with_cpu=False):
    """The depth terms of the loss (train.py:548-573): scale/shift fit + L1 + four-scale gradient loss, fwd + bwd."""
    import ctypes
    from gscream_amd import _native
    from gscream_amd import loss_utils as L
    from oracle import loss_oracle as LO
    lib = _native.load()
    g = torch.Generator(device=dev).manual_seed(9)
    y = torch.rand((1, H, W), device=dev, generator=g) * 4 + 1
    d = (0.6 * y + 0.4 + 0.05 * torch.randn(y.shape, device=dev, generator=g)).requires_grad_(True)
    m = (torch.rand((1, H, W), device=dev, generator=g) > 0.3).float()
    ws = torch.empty((lib.gsr_depth_loss_workspace_bytes(H, W),), dtype=torch.uint8, device=dev)
    out5, grad = torch.empty(5, device=dev), torch.empty((H, W), device=dev)
    dd, stream = d.detach().reshape(H, W).contiguous(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def native():
        _native.check(lib.gsr_depth_loss_forward(H, W, _native.ptr(dd), _native.ptr(y), _native.ptr(m), _native.ptr(m), _native.ptr(m),
                                                 1.0, 0.5, _native.ptr(ws), _native.ptr(out5), stream), "depth loss forward")
        _native.check(lib.gsr_depth_loss_backward(H, W, _native.ptr(dd), _native.ptr(y), _native.ptr(m), _native.ptr(ws), None,
                                                  _native.ptr(grad), stream), "depth loss backward")

    def eager():
        loss = LO.depth_loss(d, y, m, m, m, 1.0, 0.5)[0]
        return torch.autograd.grad(loss, d)[0]

    def timed(fn, n):
        gpu_spin_up(dev)
        for _ in range(NEXT_ROW_WARMUP):
            fn()
        return event_ms(fn, n)

    ms, ms_eager = timed(native, NEXT_ROW_ITERS), timed(eager, NEXT_ROW_ITERS)
    cpu = None
    if with_cpu:
        dc, yc, mc = d.detach().cpu().requires_grad_(True), y.cpu(), m.cpu()
        it, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 3.0:
            torch.autograd.grad(LO.depth_loss(dc, yc, mc, mc, mc, 1.0, 0.5)[0], dc)
            it += 1
        dt = time.perf_counter() - t0
        cpu = {"value": round(it / dt, 2), "unit": "iters/s", "cores": torch.get_num_threads(), "kind": "port",
               "sample": f"oracle/loss_oracle.py depth_loss value+grad (fp32 torch on the host), same {H}x{W} maps, {it} iterations in {dt:.1f}s"}
    nbytes = H * W * (4 * 4 + 4 * 5 + 4 + 4 * 4 + 4)  # sums: d,y,m,g; stencil: d,y,w,g (+neighbours from cache) + G; backward: d,y,m,G + out
    return {"what": f"depth loss (scale/shift fit, L1, 4-scale gradient loss), forward + backward, {H}x{W} (gsr_depth_loss_*)",
            "ms": round(ms, 4), "algorithmic_bytes": nbytes,
            "roofline": {"bound": "hbm", "achieved": round(nbytes / 1e9 / (ms / 1e3), 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(nbytes / 1e9 / (ms / 1e3) / HBM_PEAK_GBS, 4)},
            "torch_eager_same_gpu_ms": round(ms_eager, 4), "speedup_vs_torch_eager": round(ms_eager / ms, 1),
            **({"cpu_baseline": cpu} if cpu else {})}


def valu_roofline(pmc, stage, avg_ms):
    """VALU-issue view of the dominant kernel (the blend kernels are not HBM-bound): wave-level VALU instructions per
    launch by class (SQ_INSTS_VALU from the rocprofv3 --pmc passes, split by the kernel's static instruction mix) x the
    MEASURED SIMD issue cost per wave64 instruction of each class (tools/microbench/valu_issue.hip ->
    profiles/valu_issue.json), over the cycles 1024 SIMDs have during the launch.  None until both files exist."""
    path = os.path.join(ROOT, "profiles", "valu_issue.json")
    insts = pmc.get("_insts_valu", {}).get(stage) if pmc else None
    if insts is None or not os.path.exists(path):
        return None
    try:
        vi = json.load(open(path))
        mix = vi.get("mix", {}).get(stage, {"plain": 1.0})
        cyc = sum(frac * vi["cycles_per_wave_instruction"][cls] for cls, frac in mix.items())
        simd_cycles = vi["simds"] * vi["clock_mhz"] * 1e3 * avg_ms  # SIMDs x cycles per ms x ms
        return {"insts_valu_per_launch": insts, "issue_cycles_per_wave_instruction": round(cyc, 3), "mix": mix,
                "clock_mhz": vi["clock_mhz"], "frac_of_issue_ceiling": round(insts * cyc / simd_cycles, 4),
                "how": "SQ_INSTS_VALU x measured issue cycles / (SIMDs x clock x launch duration); see tools/microbench/valu_issue.hip"}
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)}


def load_pmc(workload):
    """The replayed counter file (profiles/pmc_latest.json, from separate rocprofv3 --pmc passes: tools/pmc_run.sh +
    tools/pmc_summary.py) and where it comes from.  The counters are only replayed onto the kernels they were measured on:
    the file carries a hash of the kernel sources, and a mismatch with this checkout sets traffic / valu to null."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import provenance
    path = os.path.join(ROOT, "profiles", "pmc_latest.json")
    here = provenance.stamp()
    src = {"file": "profiles/pmc_latest.json", "how": "replayed from separate rocprofv3 --pmc passes (tools/pmc_run.sh, tools/pmc_summary.py); "
                                                     "not measured in this run", "this_run": here}
    if not os.path.exists(path):
        return {}, dict(src, status="absent", reason="no counter file in this checkout")
    try:
        pmc = json.load(open(path)).get(workload, {})
    except Exception as e:  # noqa: BLE001
        return {}, dict(src, status="unreadable", reason=repr(e))
    if not pmc:
        return {}, dict(src, status="absent", reason=f"no counters for workload {workload}")
    prov = pmc.get("_provenance")
    src["collected_on"] = prov
    if not prov or prov.get("kernel_source_sha256") != here["kernel_source_sha256"]:
        return {}, dict(src, status="stale", reason="the counters were collected on different kernel sources than this checkout's "
                                                    "(kernel_source_sha256 differs or is missing): traffic and valu are null")
    return pmc, dict(src, status="current", library_matches=prov.get("library_sha256") == here["library_sha256"])


class SceneBench:
    """One synthetic scene resident in HBM + the step closure (one forward + one full backward through the public API)."""

    def __init__(self, dev, P, W, H, scene_seed, grad_seed, gsel, workload="config2", scene=None, upstream=None):
        """scene / upstream: already-built inputs (numpy arrays or tensors resident on `dev`); built here otherwise."""
        from gscream_amd import GaussianRasterizationSettings, GaussianRasterizer
        from gscream_amd import synthetic as S
        s = scene if scene is not None else scene_for(workload, scene_seed, P, W, H)
        P = int(s["means3D"].shape[0])  # (a model-derived workload decides its own size)
        t = lambda a: (a.detach().to(dev) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        self.leaves = [t(s[k]).requires_grad_(True) for k in ("means3D", "opacities", "uncertainties", "colors", "scales", "rotations")]
        self.means2D = torch.zeros_like(self.leaves[0], requires_grad=True)
        self.rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"],
                                                bg=t(s["bg"]), scale_modifier=1.0, viewmatrix=t(s["viewmatrix"]),
                                                projmatrix=t(s["projmatrix"]), sh_degree=1, campos=t(s["campos"]),
                                                prefiltered=False, debug=False)
        self.rast = GaussianRasterizer(raster_settings=self.rs)
        self.g = [t(g) for g in (upstream if upstream is not None else S.upstream_grads(grad_seed, W, H, *gsel))]  # resident, zeros where unused
        self.gsel, self.inputs = gsel, self.leaves + [self.means2D]
        self.P, self.W, self.H = P, W, H
        self._t = t
        self.rot = None
        self.last = None  # what the most recent step handed back to its caller (--dump-outputs)

    def _keep(self, color, depth, feat, radii, grads):
        # detached: holding the outputs must not keep the step's autograd graph (and its workspaces) alive
        self.last = {"color": color.detach(), "depth": depth.detach(), "uncertainty": feat.detach(), "radii": radii,
                     **{"grad_" + k: g for k, g in zip(("means3D", "opacities", "uncertainties", "colors", "scales", "rotations",
                                                        "means2D"), grads)}}

    def make_rotation(self, V, seed=7, angle=0.03, eps_pos=2e-4, eps_op=1e-3):
        """Training-like view rotation (train.py:414-416 pops a shuffled stack of cameras, one per iteration, and the
        optimiser moves the Gaussians between two visits of a view): V cameras on a small orbit around the scene's own camera -- yaw /
        pitch of `angle` rad about the centre of the cloud, well inside the generator's 15 % lateral overshoot, so every view sees a
        full frame --, each with its OWN view-matrix tensor (what the per-view walk-depth cache keys on), popped in a fixed-seed shuffled
        order epoch after epoch; before every step the Gaussians are perturbed in place by an optimiser-sized step (positions by
        eps_pos scene units = a few hundredths of a pixel, opacities by eps_op; four fixed noise tensors used in turn with alternating
        sign, so the cloud random-walks around where it started) -- a revisit never sees the lists it recorded."""
        from gscream_amd import GaussianRasterizer
        from gscream_amd import synthetic as S
        tfx, tfy = float(self.rs.tanfovx), float(self.rs.tanfovy)
        c2w0 = np.linalg.inv(self.rs.viewmatrix.detach().double().cpu().numpy().T)  # (the settings hold W2C^T)
        centre = self.leaves[0].detach().double().mean(0).cpu().numpy()
        rasts = []
        for i in range(V):
            yaw, pitch = angle * math.cos(2 * math.pi * i / V), angle * math.sin(2 * math.pi * i / V)
            cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
            R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
            M = np.eye(4)
            M[:3, :3] = R
            M[:3, 3] = centre - R @ centre            # world-space rotation about the cloud's centre
            w2c = np.linalg.inv(M @ c2w0)
            view, proj, campos = S.camera_matrices(tfx, tfy, w2c.astype(np.float32))
            rs = self.rs._replace(viewmatrix=self._t(view), projmatrix=self._t(proj), campos=self._t(campos))
            rasts.append(GaussianRasterizer(raster_settings=rs))
        g = torch.Generator(device=self.leaves[0].device).manual_seed(seed)
        noise = [(torch.randn(self.leaves[0].shape, device=self.leaves[0].device, generator=g),
                  torch.randn(self.leaves[1].shape, device=self.leaves[1].device, generator=g)) for _ in range(4)]
        rng = np.random.default_rng(seed)
        self.rot = {"V": V, "rasts": rasts, "noise": noise, "rng": rng, "order": [], "k": 0, "eps": (eps_pos, eps_op), "angle": angle,
                    "seed": seed, "start": [x.detach().clone() for x in self.leaves[:2]]}

    def rewind_rotation(self):
        """Back to where make_rotation started: the unperturbed Gaussians, the first view of the first epoch.  The warm-up runs for a
        time, not a number of steps, so without this the timed steps would start from a cloud and a view that vary from run to run."""
        r = self.rot
        with torch.no_grad():
            for x, x0 in zip(self.leaves[:2], r["start"]):
                x.copy_(x0)
        r["order"], r["k"], r["rng"] = [], 0, np.random.default_rng(r["seed"])

    def step_rot(self, perturb=True):
        """One training-like iteration: pop the next view of the shuffled epoch, move the Gaussians, forward + backward."""
        r = self.rot
        if not r["order"]:
            r["order"] = list(r["rng"].permutation(r["V"]))
        v = r["order"].pop()
        means3D, opac, unc, colors, scales, rots = self.leaves
        if perturb:
            k = r["k"]
            r["k"] = k + 1
            dn, do = r["noise"][k & 3]
            sign = 1.0 if (k >> 2) & 1 == 0 else -1.0
            with torch.no_grad():
                means3D.add_(dn, alpha=sign * r["eps"][0])
                opac.add_(do, alpha=sign * r["eps"][1]).clamp_(0.0, 1.0)
        color, depth, feat, radii = r["rasts"][v](means3D, self.means2D, opac, unc, colors_precomp=colors, scales=scales, rotations=rots)
        outs = [o for o, use in zip((color, depth, feat), self.gsel) if use]
        gos = [g for g, use in zip(self.g, self.gsel) if use]
        self._keep(color, depth, feat, radii, torch.autograd.grad(outs, self.inputs, gos))
        return radii

    def step(self):
        means3D, opac, unc, colors, scales, rots = self.leaves
        color, depth, feat, radii = self.rast(means3D, self.means2D, opac, unc, colors_precomp=colors, scales=scales, rotations=rots)
        outs = [o for o, use in zip((color, depth, feat), self.gsel) if use]
        gos = [g for g, use in zip(self.g, self.gsel) if use]
        grads = torch.autograd.grad(outs, self.inputs, gos)  # maps the loss does not use get no gradient, as in training
        self._keep(color, depth, feat, radii, grads)
        return radii

    def check(self):
        """Output checks on this rank's own scene (untimed; size-independent identities, tests/test_gpu_fullsize.py):
        partition of unity (colours = 1, background = 1 => image = 1), and sum_g dL/dcolor[g, ch] = sum_pix g_ch (1 - T_final)
        for the upstream gradient the timed steps use.  -> (ok, details)"""
        from gscream_amd import GaussianRasterizer
        means3D, opac, unc, colors, scales, rots = self.leaves
        ones = torch.ones_like(colors)
        with torch.no_grad():
            one = GaussianRasterizer(self.rs._replace(bg=torch.ones_like(self.rs.bg)))(
                means3D, self.means2D, opac, unc, colors_precomp=ones, scales=scales, rotations=rots)[0]
            cover = GaussianRasterizer(self.rs._replace(bg=torch.zeros_like(self.rs.bg)))(
                means3D, self.means2D, opac, unc, colors_precomp=ones, scales=scales, rotations=rots)[0][0].double()  # = 1 - T_final
        unity = float((one - 1.0).abs().max())
        color = self.rast(means3D, self.means2D, opac, unc, colors_precomp=colors, scales=scales, rotations=rots)[0]
        g = self.g[0]
        dcol = torch.autograd.grad([color], [colors], [g])[0].double()
        worst = 0.0
        for ch in range(3):
            lhs, rhs = float(dcol[:, ch].sum()), float((g[ch].double() * cover).sum())
            worst = max(worst, abs(lhs - rhs) / max(float((g[ch].double().abs() * cover).sum()), 1e-30))
        finite = bool(torch.isfinite(color).all()) and bool(torch.isfinite(dcol).all())
        ok = unity < 2e-5 and worst <= 1e-4 and finite
        return ok, {"partition_of_unity_max_err": unity, "sum_dLdcolor_rel_err": worst, "finite": finite}


def run_config5(args, dist, dev, rank, world):
    """BASELINE.json config 5: ten independent scenes (seeds 10..19, P in [0.6, 1.4] x 10^6, 1008x567, RGB-only upstream
    gradients) pulled from a shared work queue by one process per GPU.  Per scene: W warm-up + K timed steps.  value =
    all timed steps of all scenes / the slowest rank's timed seconds ("strong" scaling: the scene list is fixed)."""
    from gscream_amd import multi
    from gscream_amd import synthetic as S
    W, H, gsel = 1008, 567, (True, False, False)
    queue = multi.SceneQueue(dist, 10)
    # Round 5: every rank builds ALL ten scenes and parks them in its GPU's HBM (ten 1M-Gaussian scenes + upstream gradients are
    # ~0.8 GB of 288) BEFORE the first barrier -- the queue may hand any scene to any rank.  The wall clock between the barriers then
    # holds what a scene costs a GPU (warm-up + timed steps), not numpy generators and PCIe uploads; the output checks run after
    # the last barrier on the scenes the rank kept.
    t_build = time.perf_counter()
    keys = ("means3D", "opacities", "uncertainties", "colors", "scales", "rotations", "bg", "viewmatrix", "projmatrix", "campos")
    resident = {}
    for idx in range(10):
        seed, P = multi.config5_scene(idx)
        sc = S.scene_slab(seed, P, W, H)
        dsc = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if k in keys else v) for k, v in sc.items()}
        resident[idx] = (seed, P, dsc, [torch.from_numpy(g).to(dev) for g in S.upstream_grads(seed, W, H, *gsel)])
    # ... and a few steps of the LARGEST scene: the workspaces of a step (geometry, image, binning, gradient slots: ~0.6 GB) then sit
    # in torch's caching allocator at the largest size any scene needs, and no scene inside the wall-clocked region pays for a
    # hipMalloc (measured: ~15 ms per scene, as much as its 50 timed steps)
    big = max(resident, key=lambda i: resident[i][1])
    sbw = SceneBench(dev, resident[big][1], W, H, resident[big][0], resident[big][0], gsel, scene=resident[big][2], upstream=resident[big][3])
    for _ in range(3):
        sbw.step()
    del sbw
    torch.cuda.synchronize(dev)
    build_s = time.perf_counter() - t_build
    multi.barrier(dist, dev)
    wall0 = time.perf_counter()
    mine, busy, kept = [], 0.0, []
    while True:
        idx = queue.pull()
        if idx is None:
            break
        seed, P, dsc, up = resident[idx]
        sb = SceneBench(dev, P, W, H, seed, seed, gsel, scene=dsc, upstream=up)
        for _ in range(max(args.warmup, 1)):
            sb.step()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            sb.step()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        busy += dt
        from gscream_amd import rasterizer as RZ
        mine.append({"scene": idx, "seed": seed, "P": P, "rank": rank, "iters_per_s": round(args.steps / dt, 1),
                     "num_rendered": int(RZ._last_stage1.get("num_rendered", 0))})
        kept.append(sb)
    multi.barrier(dist, dev)
    wall = time.perf_counter() - wall0
    for rec, sb in zip(mine, kept):  # untimed, after the job: each scene's outputs satisfy the rasterizer's identities on this rank's data
        ok, detail = sb.check()
        rec.update(check_ok=bool(ok), check={k: (v if isinstance(v, bool) else float(f"{v:.3g}")) for k, v in detail.items()})
    if rank == 0 and args.dump_outputs and kept:  # (the last timed step of the last scene this rank ran; the checks above keep sb.last)
        dump_outputs(args.dump_outputs, kept[-1].last, kept[-1].P)
    del kept, resident
    per_rank = multi.gather_objects(dist, {"rank": rank, "device": int(dev.index), "scenes": [r["scene"] for r in mine], "busy_s": round(busy, 4),
                                           "build_all_scenes_s": round(build_s, 2), "numa": NUMA_INFO})
    total_steps, slowest, rate = multi.aggregate_throughput(dist, args.steps * len(mine), busy, dev)
    _, wall, _ = multi.aggregate_throughput(dist, 0, wall, dev)
    report = sorted(sum(multi.gather_objects(dist, mine), []), key=lambda r: r["scene"])
    if rank == 0:
        assert [r["scene"] for r in report] == list(range(10)), "every scene exactly once"
        bad = [r for r in report if not r["check_ok"]]
        if bad:
            raise SystemExit(f"config 5: output checks failed on scenes {[(r['scene'], r['check']) for r in bad]}")
        out = {"metric": "train iters/sec (fwd+bwd raster), config 5: ten scenes over the node's GPUs", "value": round(rate, 3),
               "unit": "iters/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(slowest / max(total_steps, 1) * 1e3, 4), "higher_is_better": True, "scaling": "strong",
               "vs_baseline": None, "dtype": "f32", "data": "synthetic",
               "config": {"workload": "config5: ten synthetic stand-ins for the SPIn-NeRF scenes (config-2 generator, seeds 10-19, "
                                      "P in [0.6,1.4]e6), 1008x567, fwd+bwd RGB-only; one process per GPU pulling scenes from a shared "
                                      "queue (TCPStore counter), no collective in the raster path",
                          "parallelism": f"{world} process(es), work queue over 10 scenes",
                          "collective_backend": None if dist is None else dist.get_backend(),
                          "collective_world_size": 1 if dist is None else dist.get_world_size(),
                          "oversubscribed_test_mode": bool(args.oversubscribe)},
               "value_is": "all timed steps / the slowest rank's summed TIMED sections (kernel-time throughput; scene construction, "
                           "warm-up, the output checks and a rank's idle tail are outside it)",
               "wall_clock": {"seconds_first_to_last_barrier": round(wall, 3), "iters_per_s": round(total_steps / wall, 2),
                              "frac_of_busy_time_rate": round(total_steps / wall / rate, 3),
                              "note": "first to last barrier: queue pulls, the W warm-up steps of every scene (not counted as iterations) and "
                                      "its K timed steps; the ten scenes were built and parked in every GPU's HBM before the first barrier, "
                                      "the output checks run after the last"},
               "per_rank": per_rank,
               "checks_passed": sum(1 for r in report if r["check_ok"]),
               "sum_of_scene_rates": round(sum(r["iters_per_s"] for r in report), 1),
               "slowest_rank_busy_s": round(slowest, 4), "scenes": report}
        print(json.dumps(out), flush=True)


DUMP_BUDGET_BYTES = 60_000_000  # --dump-outputs writes at most this much (npy headers come on top: well under 64 MB in all)


def dump_outputs(path, last, P):
    """--dump-outputs: the arrays the last timed step handed back to its caller (images, radii, the gradients of the seven leaves) as
    float32 `<name>.npy` under `path`.  Images are written whole; per-Gaussian arrays as the same rows of each, a fixed seeded sample
    when all P rows would not fit the budget, with their row numbers in `gaussian_index.npy` (float64)."""
    os.makedirs(path, exist_ok=True)
    images = {k: v for k, v in last.items() if k in ("color", "depth", "uncertainty")}
    per_gauss = {k: v for k, v in last.items() if k not in images}  # radii and the gradients: one row per Gaussian
    left = DUMP_BUDGET_BYTES - sum(4 * v.numel() for v in images.values())
    row_bytes = 8 + sum(4 * (v.numel() // P) for v in per_gauss.values())
    rows = max(0, min(P, left // row_bytes))
    idx = np.arange(P) if rows == P else np.sort(np.random.default_rng(0).choice(P, rows, replace=False))
    for k, v in images.items():
        np.save(os.path.join(path, k + ".npy"), v.float().cpu().numpy())
    it = torch.from_numpy(idx).to(next(iter(last.values())).device)
    for k, v in per_gauss.items():
        np.save(os.path.join(path, k + ".npy"), v.index_select(0, it).float().cpu().numpy())
    np.save(os.path.join(path, "gaussian_index.npy"), idx.astype(np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="config2", choices=sorted(WORKLOADS) + ["config5"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget", type=float, default=12.0, help="seconds of CPU work for the cpu_baseline leg")
    ap.add_argument("--no-next-rows", action="store_true", help="skip the SURVEY 8(f) rows (loss, knn) reported beside the north-star line")
    ap.add_argument("--no-tile-cull", action="store_true", help="bin every rectangle tile like the reference")
    ap.add_argument("--scatter-bands", type=int, default=0, help="force the scatter launch to N bands of tile rows per chunk (0 = automatic)")
    ap.add_argument("--occlusion", type=int, default=-1, help="occlusion cut-off: -1 automatic (default), 0 off, 1 on")
    ap.add_argument("--views", type=int, default=1,
                    help="cameras the TIMED steps rotate through (default 1 = BASELINE's line: one view, static Gaussians); V > 1: a shuffled "
                         "epoch of V views on a small orbit, the Gaussians perturbed by an optimiser-sized step before every iteration")
    ap.add_argument("--rotation-views", type=int, default=64,
                    help="views of the `rotation` block reported beside the headline (training-like view rotation, per-view cache on / off); 0 = skip")
    ap.add_argument("--no-view-cache", action="store_true",
                    help="forward without the per-view walk-depth cache (the mirror's default: every step after the first is a revisit of "
                         "the bench's one view, like every epoch after the first is in training)")
    ap.add_argument("--no-strict-parity", action="store_true", help="skip the strict_parity_build leg (the parity build on the same workload)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="collective backend for the barriers (nccl == RCCL)")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="TEST MODE: let ranks share GPUs when there are fewer GPUs than ranks (never a measurement)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: per-stage profile and roofline, spread blocks, view-cache and rotation blocks, "
                         "per-rank figures, scene statistics, the next rows, the parity build, the CPU baselines and the parity check "
                         "(the --no-* options above select among these); without it a run times the K steps and prints the headline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (images, radii, gradients) as float32 DIR/<name>.npy")
    args = ap.parse_args()

    from gscream_amd import multi
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # started as plain `python bench.py --gpus N`: become the launcher of N ranks, one per GPU
        if not torch.cuda.is_available() or (torch.cuda.device_count() < args.gpus and not args.oversubscribe):
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {torch.cuda.device_count() if torch.cuda.is_available() else 0} "
                             "GPU(s) visible; one process per GPU is required")
        sys.exit(multi.launch_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    rank, local_rank, world = multi.dist_env()
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the rasterizer has no CPU path (the CPU oracle is only the baseline leg)")
    dev_index = multi.pick_device(local_rank, args.oversubscribe)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    dist = multi.init(args.backend, dev)  # nccl == RCCL on ROCm; None when WORLD_SIZE == 1
    if world > 1:
        # the driver's SCALE record is only usable if the line it parses says what carried the barriers and over how many ranks:
        # `config.collective_backend` / `config.collective_world_size` below come from these two calls, checked here on every rank
        if dist is None or dist.get_world_size() != args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: the process group has {None if dist is None else dist.get_world_size()} ranks")
        if dist.get_backend() != args.backend or (not args.oversubscribe and args.backend != "nccl"):
            raise SystemExit(f"bench.py --gpus {args.gpus}: collective backend {dist.get_backend()!r}; a measurement needs 'nccl' (= RCCL); "
                             "'gloo' is for the oversubscribed test mode")
    global NUMA_INFO
    if world > 1 and not args.oversubscribe:
        NUMA_INFO = multi.pin_to_gpu_numa(dev_index)  # one process per GPU: keep its host threads next to that GPU

    from gscream_amd import _native, set_tuning
    _native.load()
    def apply_tuning(view_cache=True, **over):
        kw = dict(tile_cull=not args.no_tile_cull, scatter_bands=args.scatter_bands, occlusion_cut=None if args.occlusion < 0 else bool(args.occlusion),
                  view_cache=view_cache and not args.no_view_cache)
        if os.environ.get("GSR_BENCH_HEAVY_GROUPS"):  # (diagnostic: force the per-Gaussian backward's cooperative kernel on / off: 1 / 0)
            kw["heavy_groups"] = os.environ["GSR_BENCH_HEAVY_GROUPS"] == "1"
        kw.update(over)
        set_tuning(**kw)
    apply_tuning()

    if args.workload == "config5":
        run_config5(args, dist, dev, rank, world)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    P, W, H, seed, gsel, desc = WORKLOADS[args.workload]
    sb = SceneBench(dev, P, W, H, multi.scene_seed(seed, rank, world), seed, gsel, args.workload)  # one independent scene per GPU
    step, rs, P = sb.step, sb.rs, sb.P
    means3D, opac, unc, colors, scales, rots = sb.leaves
    if args.views > 1:  # the timed steps themselves rotate through V views with moving Gaussians (not BASELINE's line: labelled)
        sb.make_rotation(args.views)
        step = sb.step_rot

    def barrier():
        multi.barrier(dist, dev)

    # Python's cyclic collector runs NOW and is then held off until the K timed steps are over: a generation-2 pass landing in a 9 ms
    # region is a 10-30 % error (tools/render_fps_probe.py).  (Not right in front of the region: the GPU idles through a collection
    # and the K = 20 steps behind it ran 14 % slower than the blocks that followed, profiles/r05_bench_region.txt.)
    import gc
    gc.collect()
    gc.disable()
    for _ in range(max(args.warmup, 1)):
        radii = step()
    barrier()
    # The driver's W = 5 warm-up steps are 2 ms of GPU work behind seconds of scene construction: the timed region then starts on a GPU
    # that has not been busy long enough to be in its steady state (timed region vs the three `ms_per_step_spread` blocks that follow it:
    # 1-3 % slower in every round-5 A/B run, profiles/r05_view_cache_ab.txt).  More untimed steps of the same workload until the
    # GPU has been busy for WARM_MS; their number is reported (`warmup_extra_steps`).
    warm_extra, t_w = 0, time.perf_counter()
    while (time.perf_counter() - t_w) * 1e3 < WARM_MS:
        for _ in range(8):
            step()
        torch.cuda.synchronize()
        warm_extra += 8
    barrier()
    # Timed region: exactly K steps.  With --full, only the dominant kernel (the backward blend, established by the warm-up
    # profile below) is bracketed by HIP events here -- timing every stage inserts ~10 event markers per step and
    # measurably stretches the step; the full per-stage profile is taken over K more steps afterwards.
    if args.full:
        _native.profile_begin()
        for _ in range(3):
            step()
        barrier()
        wprof = _native.profile_end()
        dom_stage = max(wprof, key=lambda k: wprof[k][0] / max(wprof[k][1], 1))
    if args.views > 1:  # (the warm-up ran for a time, not a step count: the timed steps start from the same cloud and view in every run)
        sb.rewind_rotation()
    barrier()
    # (the dominant kernel is bracketed by HIP events in every FOURTH step of the timed region: each pair costs the stream a bubble
    # on either side of the kernel -- with a pair in every step the region ran 2.5 % slower than the same loop without any)
    if args.full and not os.environ.get("GSR_BENCH_NO_BRACKET"):  # (diagnostic knob: what the brackets cost the region)
        _native.profile_begin([dom_stage], every=4)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    gc.enable()
    last = sb.last  # (what the timed path computed in its last step; the --full measurements below run further steps)

    def headline(rate, ms_per_step):
        """The result line's own fields: what was timed, on what, and how fast."""
        from gscream_amd import rasterizer as RZ
        return {
            "metric": "train iters/sec (fwd+bwd raster) @ 1M Gaussians, 1008x567",
            "value": round(rate, 3), "unit": "iters/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "warmup_extra_steps": warm_extra,
            "warmup_note": f"the W warm-up steps are followed by further UNTIMED steps of the same workload until the GPU has been busy for {WARM_MS:.0f} ms "
                           "(GSR_BENCH_WARM_MS): W = 5 steps are 2 ms of work behind seconds of host-side scene construction, and a K = 20 region "
                           "timed right behind them read 2257-2308 it/s where this reads 2432-2441 (profiles/r05_bench_region.txt)",
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": desc if args.views <= 1 else desc + f" -- NOT BASELINE's line: the timed steps rotate through {args.views} views with perturbed Gaussians (--views)",
                       "views": args.views, "P": P, "W": W, "H": H, "num_rendered": RZ._last_stage1["num_rendered"],
                       "tile_cull": not args.no_tile_cull,
                       "parallelism": f"{world} independent scene(s), one per GPU, barrier only",
                       "collective_backend": None if dist is None else dist.get_backend(),
                       "collective_world_size": 1 if dist is None else dist.get_world_size(),
                       "oversubscribed_test_mode": bool(args.oversubscribe)},
            **({"fitted_run": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in FIT_INFO.items()}} if FIT_INFO else {}),
        }

    if not args.full:
        total_steps, elapsed, rate = multi.aggregate_throughput(dist, args.steps, elapsed, dev)
        if rank == 0:
            out = headline(rate, elapsed / args.steps * 1e3)
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, last, P)
            print(json.dumps(out), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    dom_prof = _native.profile_end()
    _native.profile_begin()
    for _ in range(args.steps):
        step()
    barrier()
    prof = _native.profile_end()
    prof[dom_stage] = dom_prof[dom_stage]  # the roofline kernel's duration is the one measured in the timed region
    # spread (reported beside `value`, never instead of it): three more blocks of K steps, timed the same way.  The driver's
    # K = 20 makes the official region 9 ms long; this says how much such a sample moves from block to block on this box.
    spread_ms = []
    for _ in range(3):
        barrier()
        tb = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        spread_ms.append((time.perf_counter() - tb) / args.steps * 1e3)

    # the same loop WITHOUT the per-view walk-depth cache (reported beside `value`: the timed region revisits one view, i.e. it is
    # the every-epoch-but-the-first case; this is the first-epoch / never-seen-view case)
    view_cache_off_ms = None
    if not args.no_view_cache:
        apply_tuning(view_cache=False)
        for _ in range(3):
            step()
        blocks = []
        for _ in range(3):  # (median of three blocks: one host stall in a single block of K steps is a 20 % error)
            barrier()
            tb = time.perf_counter()
            for _ in range(args.steps):
                step()
            barrier()
            blocks.append((time.perf_counter() - tb) / args.steps * 1e3)
        view_cache_off_ms = sorted(blocks)[1]
        apply_tuning()
        for _ in range(3):
            step()
        barrier()

    # Training-like view rotation: what the per-view walk depths are worth when a view comes back one epoch later and
    # the Gaussians have moved in between -- the timed region above revisits ONE static frame, i.e. its recorded depths predict perfectly.
    rotation = None
    if args.rotation_views > 1 and args.views <= 1:
        from gscream_amd import rasterizer as _RZr
        V = args.rotation_views
        keep = [x.detach().clone() for x in (means3D, opac)]
        sb.make_rotation(V)

        def rot_run(view_cache, perturb, epochs=3):
            apply_tuning(view_cache=view_cache)
            with torch.no_grad():
                means3D.copy_(keep[0]); opac.copy_(keep[1])
            sb.rot["order"], sb.rot["k"] = [], 0
            for _ in range(V):               # first epoch, untimed: every view seen once (this is what fills the cache)
                sb.step_rot(perturb)
            torch.cuda.synchronize()
            redo, n = 0, epochs * V
            tb = time.perf_counter()
            for _ in range(n):
                sb.step_rot(perturb)
                redo += 0 if _RZr._last_stage1.get("speculative", True) else 1
            torch.cuda.synchronize()
            ms = (time.perf_counter() - tb) / n * 1e3
            _native.profile_begin()
            for _ in range(V):
                sb.step_rot(perturb)
            torch.cuda.synchronize()
            pr = _native.profile_end()
            return ms, redo / n, {k: round(v[0] / max(v[1], 1) * 1e3, 1) for k, v in pr.items() if v[1]}

        ms_on, redo_on, st_on = rot_run(not args.no_view_cache, True)
        ms_off, redo_off, st_off = rot_run(False, True)
        ms_static, _, st_static = rot_run(not args.no_view_cache, False)
        with torch.no_grad():
            means3D.copy_(keep[0]); opac.copy_(keep[1])
        apply_tuning()
        for _ in range(3):
            step()
        barrier()
        rotation = {"views": V, "epochs_timed": 3, "ms_per_step": round(ms_on, 4), "ms_per_step_no_view_cache": round(ms_off, 4),
                    "ms_per_step_static_gaussians": round(ms_static, 4),
                    "redo_rate": round(redo_on, 4), "redo_rate_no_view_cache": round(redo_off, 4),
                    "iters_per_s": round(1e3 / ms_on, 1), "iters_per_s_no_view_cache": round(1e3 / ms_off, 1),
                    "stage_us": st_on, "stage_us_no_view_cache": st_off, "stage_us_static_gaussians": st_static,
                    "orbit_angle_rad": sb.rot["angle"], "perturbation": {"positions": sb.rot["eps"][0], "opacities": sb.rot["eps"][1]},
                    "what": f"{V} cameras on a small orbit (yaw / pitch of {sb.rot['angle']} rad about the cloud's centre), popped in a shuffled order epoch "
                            "after epoch like train.py:414-416; before every iteration the positions move by N(0, 2e-4) scene units (a few hundredths "
                            "of a pixel) and the opacities by N(0, 1e-3) -- an optimiser-sized step (two elementwise kernels, inside the timed steps of "
                            "both variants); first epoch untimed (it fills the per-view cache), three epochs timed; redo_rate = forwards whose "
                            "speculative workspace guess was too small and that were redone (GSR_NEED_CAPACITY); NOT the headline: BASELINE's metric is "
                            "one view"}

    my_elapsed = elapsed
    total_steps, elapsed, rate = multi.aggregate_throughput(dist, args.steps, elapsed, dev)
    # per-rank breakdown for the --gpus N line: every rank's own rate, instance count and host cost per step (median wall time of the
    # step() call alone -- enqueue only, no sync -- over one more block of K steps outside the timed region)
    host_calls = []
    for _ in range(args.steps):
        th = time.perf_counter()
        step()
        host_calls.append(time.perf_counter() - th)
    barrier()
    host_calls.sort()
    from gscream_amd import rasterizer as _RZ
    per_rank = multi.gather_objects(dist, {"rank": rank, "device": int(dev.index), "iters_per_s": round(args.steps / my_elapsed, 2),
                                           "ms_per_step": round(my_elapsed / args.steps * 1e3, 4), "P": int(P),
                                           "num_rendered": int(_RZ._last_stage1.get("num_rendered", 0)),
                                           "host_ms": round(host_calls[len(host_calls) // 2] * 1e3, 4), "numa": NUMA_INFO})

    # units for the byte model (untimed): instances actually binned, and the reference's num_rendered = every
    # tile of every 3-sigma rectangle (one forward with tile culling off)
    from gscream_amd import rasterizer as RZ
    R = RZ._last_stage1["num_rendered"]
    with torch.no_grad():
        apply_tuning(tile_cull=False, occlusion_cut=False)
        e = torch.Tensor([])
        R_ref = RZ._forward_native(means3D, e, colors, opac, unc, scales, rots, e, rs)[0]
        apply_tuning()
    N, T = W * H, ((W + 15) // 16) * ((H + 15) // 16)
    visible = int((radii > 0).sum())

    if rank == 0:
        model = stage_algorithmic_bytes(P, R, N, T)            # SURVEY 8(d) bytes at R = this run's num_rendered (graded)
        model_ref = stage_algorithmic_bytes(P, R_ref, N, T)    # the same model at the reference's own num_rendered (extra)
        pmc, traffic_source = load_pmc(args.workload)
        stages = {}
        for name, (ms, n) in prof.items():
            if n:
                avg = ms / n
                moved = pmc.get(name)
                stages[name] = {"avg_ms": round(avg, 4), "launches": n,
                                "survey_model_GB": round(model[name] / 1e9, 4),
                                "survey_model_GBps": round(model[name] / 1e9 / (avg / 1e3), 1),
                                "pmc_moved_GB": None if moved is None else round(moved / 1e9, 4),
                                "pmc_moved_GBps": None if moved is None else round(moved / 1e9 / (avg / 1e3), 1)}
        dom = max(stages, key=lambda k: stages[k]["avg_ms"])
        ms_per_step = elapsed / args.steps * 1e3
        total_bytes, total_bytes_ref = sum(model.values()), sum(model_ref.values())
        moved_step = sum(pmc.get(k, 0) for k in stages) if pmc and all(k in pmc for k in stages) else None
        valu = valu_roofline(pmc, dom, stages[dom]["avg_ms"])
        out = headline(rate, ms_per_step)
        out["config"].update(num_rendered=R, num_rendered_reference=R_ref, visible=visible)
        out.update({
            "ms_per_step_spread": {"note": "three further blocks of `steps` steps on this rank, timed like the official region (which `value` comes from)",
                                   "blocks_ms": [round(v, 4) for v in spread_ms], "min": round(min(spread_ms), 4), "max": round(max(spread_ms), 4)},
            "roofline": {"bound": "hbm", "kernel": dom, "achieved": stages[dom]["survey_model_GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(stages[dom]["survey_model_GBps"] / HBM_PEAK_GBS, 4), "traffic": pmc.get(dom), "traffic_source": traffic_source,
                         "algorithmic_bytes_per_launch": model[dom], "avg_launch_ms": stages[dom]["avg_ms"], "valu": valu,
                         "timed_launches": stages[dom]["launches"],
                         "timed_launches_note": "launches of this kernel inside the timed region that were bracketed by HIP events (every 4th step)"},
            "whole_iteration": {"note": "SURVEY 8(d): 420 P + 304 R + 56 N with R = this run's num_rendered, over the measured ms_per_step",
                                "algorithmic_GB": round(total_bytes / 1e9, 4),
                                "GBps": round(total_bytes / 1e9 / (ms_per_step / 1e3), 1),
                                "frac_of_hbm_peak": round(total_bytes / 1e9 / (ms_per_step / 1e3) / HBM_PEAK_GBS, 4),
                                "pmc_moved_GB_per_step": None if moved_step is None else round(moved_step / 1e9, 4),
                                "pmc_moved_frac_of_hbm_peak": None if moved_step is None else round(moved_step / 1e9 / (ms_per_step / 1e3) / HBM_PEAK_GBS, 4),
                                "kernel_ms_sum": round(sum(v["avg_ms"] for v in stages.values()), 4),
                                "extra_reference_R": {"note": "same model charged with the reference's own num_rendered (no tile culling): the bytes "
                                                              "the reference algorithm would move on this workload; not the graded figure",
                                                      "algorithmic_GB": round(total_bytes_ref / 1e9, 4),
                                                      "frac_of_hbm_peak": round(total_bytes_ref / 1e9 / (ms_per_step / 1e3) / HBM_PEAK_GBS, 4)}},
            "view_cache": {"enabled": not args.no_view_cache,
                           "what": "gscream_amd.rasterizer keeps int32[4 T] walk depths per view (keyed by the view matrix's address) and the forward "
                                   "dispatches its quadrant tasks deepest-first from the previous visit's (gsr_tuning.walk_depths); the timed region "
                                   "renders ONE view, so every timed step is a revisit -- in training a view's previous visit is one epoch old",
                           "ms_per_step_without": None if view_cache_off_ms is None else round(view_cache_off_ms, 4),
                           "ms_per_step_without_note": "median of three blocks of `steps` steps (compare with ms_per_step_spread, timed the same way)",
                           "iters_per_s_without": None if view_cache_off_ms is None else round(1e3 / view_cache_off_ms * world, 3)},
            "rotation": rotation,
            "stages": stages,
            "per_rank": per_rank,
            "scene_stats": scene_stats(sb),
            "stages_note": "survey_model_* = SURVEY 8(d) per-stage bytes of the REFERENCE algorithm (e.g. six radix passes for tile_sort) over our "
                           "launch time: a work-equivalent rate that can exceed the HBM peak where our kernel moves fewer bytes; pmc_moved_* = bytes "
                           "the launch really moved (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE, profiles/pmc_latest.json)",
        })
        if world == 1:
            try:
                ceil = copy_ceiling(dev)
                out["roofline"]["copy_ceiling"] = {"GBps": ceil, "how": "1 GiB device-to-device torch copy, read + write bytes",
                                                   "frac_of_it": round(out["roofline"]["achieved"] / ceil, 4),
                                                   "whole_iteration_frac_of_it": round(out["whole_iteration"]["GBps"] / ceil, 4)}
            except Exception as e:  # noqa: BLE001
                out["roofline"]["copy_ceiling"] = {"error": repr(e)}
        if world == 1 and not args.no_next_rows and not os.environ.get("GSR_LIB"):
            # (before the next rows: one of them uses torch's profiler, whose tracer hooks stay in the HIP API path afterwards)
            try:
                out["host_ms_per_step"] = host_floor_row(dev, W, H)
                out["host_ms_per_step_note"] = ("fwd+bwd step loop on a 1k-Gaussian scene at the bench resolution: what the host path costs per step "
                                                "(Python wrapper, ctypes, allocator, autograd engine, ~12 HIP launches, the num_rendered wait)")
            except Exception as e:  # noqa: BLE001
                out["host_ms_per_step"] = None
                out["host_ms_per_step_note"] = repr(e)
        if world == 1 and not args.no_next_rows:
            rows = (("rgb_loss", lambda: loss_row(dev, H, W, not args.no_cpu_baseline)),
                    ("depth_loss", lambda: depth_loss_row(dev, H, W, not args.no_cpu_baseline)),
                    ("neural_gaussian_decode", lambda: decode_row(dev, not args.no_cpu_baseline)),
                    ("pipeline_decode_raster_loss", lambda: pipeline_row(dev)),
                    ("train_iteration", lambda: train_iteration_row(dev, with_cpu=not args.no_cpu_baseline)),
                    # the same iteration on the model state the reference's own initialisation produces (the stand-in's
                    # N(0, 3) anchors / N(-2, 0.3) log-scales are arbitrary; this cloud and its scales follow create_from_pcd)
                    ("train_iteration_init_state", lambda: train_iteration_row(dev, model_kind="init_state")),
                    ("render_fps", lambda: render_fps_row(dev, sb)),
                    ("fit_run", lambda: fit_row(dev, W, H)),
                    ("simple_knn", lambda: knn_row(dev, not args.no_cpu_baseline)))
            out["next_rows"] = {}
            for name, fn in rows:  # the 8(f) rows, reported beside the north-star line; never allowed to break it
                try:
                    out["next_rows"][name] = fn()
                except Exception as e:  # noqa: BLE001
                    out["next_rows"][name] = {"error": repr(e)}
                _RZ._view_cache_on[0] = not args.no_view_cache  # (render_fps measures with the per-view cache off)
        if world == 1 and not args.no_next_rows and not args.no_strict_parity and not os.environ.get("GSR_LIB"):
            try:
                out["strict_parity_build"] = strict_parity_row(args)
            except Exception as e:  # noqa: BLE001
                out["strict_parity_build"] = {"error": repr(e)}
        if world == 1 and not args.no_cpu_baseline:
            out["parity_check"], out["cpu_baseline"] = cpu_baseline(P, W, H, multi.scene_seed(seed, rank, world), gsel, args.cpu_budget, args.workload)
            out["cpu_torch_naive"] = cpu_torch_naive()
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, last, P)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
