#!/usr/bin/env python
"""Time render_set's output frames: gscream_amd.frames on the HIP path against the sequence the reference runs between the render and
the PNG encoder.

    python tools/frames_bench.py [--out profiles/frames_timing.json] [--rounds 15] [--warmup 2] [--sizes 567x1008,1080x1920]

Per frame size, seeded synthetic inputs, two forms:
    spiral  train.py:804-834: reference = min, max, normalise, .cpu(), numpy quantise, a 256-entry table lookup (in place of
            cv2.applyColorMap, which is not on this stack), three flips, F.normalize, expand, three fp32 .cpu() copies, a CPU concat, and
            save_image's mul(255).add_(0.5).clamp_(0, 255).permute.to("cpu", uint8) for the four files;  hip = rgbd_frame(panels=True) and
            one copy of the [H, 4W, 3] buffer into pinned memory
    test    train.py:776-800: reference = compute_scale_and_shift restated (five masked sums, a nonzero, masked assignments), the
            aligned | MiDaS panel to the host, matplotlib's to_rgba(bytes=True) (imsave without its encoder; a numpy statement of the
            same rule where matplotlib is absent), and save_image's tensor half for the four images;  hip = view_frames and two copies
            into pinned memory
Both run to the last byte on the host; no PNG is encoded on either side.  The paths alternate round by round in one process after
untimed warm-up rounds.  event_ms = HIP events on the stream around one call, wall_ms = host clock from an idle device to the
synchronise behind the call: medians over --rounds rounds with min and max.  Nothing is asserted about the ratio: the output is the
record.  There is no CPU fallback: without a GPU this fails."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gscream_amd import frames as Fr  # noqa: E402
from frames_helpers import cmap_mpl, view_inputs  # noqa: E402


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


def save_image_bytes(x):
    """torchvision.utils.save_image up to the encoder, for one image (make_grid repeats a single channel)."""
    if x.shape[0] == 1:
        x = torch.cat((x, x, x), 0)
    return x.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).numpy()


def reference_spiral(t, lut):
    rendering, uncertainty = torch.clamp(t["render"], 0.0, 1.0), torch.clamp(t["uncertainty"], 0.0, 1.0)
    depth = t["depth"]
    h, w = depth.shape[-2:]
    depth = (depth - depth.min()) / (depth.max() - depth.min())
    depth = (255 * depth.cpu().numpy()).astype(np.uint8)[0]
    depth = lut[depth]
    depth = torch.FloatTensor(depth).permute([2, 0, 1]) / 255.
    rendered = torch.flip(rendering.unsqueeze(0), dims=[3])[0]
    uncertainty = torch.flip(uncertainty.unsqueeze(0), dims=[3])[0].expand([3, -1, -1])
    depth = torch.flip(depth.unsqueeze(0), dims=[3])[0]
    normal = t["normal"].reshape(3, h, w).permute([1, 2, 0])
    normal = (torch.nn.functional.normalize(normal, p=2, dim=-1)).permute([2, 0, 1])
    normal = (normal + 1) / 2
    normal = torch.flip(normal.unsqueeze(0), dims=[3])[0]
    rgbd = torch.concat([rendered.cpu(), depth, normal.cpu(), uncertainty.cpu()], 2)
    return [save_image_bytes(x) for x in (rendered, uncertainty, rgbd, depth)]


def reference_test(t, to_rgba):
    rendering, uncertainty = torch.clamp(t["render"], 0.0, 1.0), torch.clamp(t["uncertainty"], 0.0, 1.0)
    prediction, target, mask = t["depth"], t["midas"], 1 - t["mask"]
    a_00 = torch.sum(mask * prediction * prediction, (1, 2))
    a_01 = torch.sum(mask * prediction, (1, 2))
    a_11 = torch.sum(mask, (1, 2))
    b_0 = torch.sum(mask * prediction * target, (1, 2))
    b_1 = torch.sum(mask * target, (1, 2))
    x_0, x_1 = torch.zeros_like(b_0), torch.zeros_like(b_1)
    det = a_00 * a_11 - a_01 * a_01
    valid = det.nonzero()
    x_0[valid] = (a_11[valid] * b_0[valid] - a_01[valid] * b_1[valid]) / det[valid]
    x_1[valid] = (-a_01[valid] * b_0[valid] + a_00[valid] * b_1[valid]) / det[valid]
    depth = prediction * torch.abs(x_0) + x_1
    panel = torch.cat((depth[0], target[0]), dim=1).cpu().numpy()
    errormap = (rendering - t["gt"]).abs()
    return [to_rgba(panel)] + [save_image_bytes(x) for x in (rendering, uncertainty, errormap, t["gt"])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_timing.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="567x1008,1080x1920")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("frames_bench needs a GPU (there is nothing to time on a CPU)")
    inferno, viridis = Fr.colormap_lut("inferno").numpy(), Fr.colormap_lut("viridis").numpy()
    try:
        import matplotlib
        from matplotlib import cm
        mappable, panel_by = cm.ScalarMappable(cmap="viridis"), f"matplotlib {matplotlib.__version__} to_rgba(bytes=True)"

        def to_rgba(panel):
            mappable.set_clim(None, None)
            return mappable.to_rgba(panel, bytes=True)
    except ImportError:
        panel_by = "numpy statement of the imsave rule (matplotlib absent)"

        def to_rgba(panel):
            return cmap_mpl(panel, panel.min(), panel.max(), viridis)
    rows = []
    for size in a.sizes.split(","):
        h, w = (int(x) for x in size.split("x"))
        v = view_inputs(h, w, 7)
        t = {k: torch.from_numpy(x).cuda() for k, x in v.items()}
        t["normal"] = t["normals"].view(1, w, h, 3).permute(0, 3, 1, 2)  # least_square_normal_regress_fast01's return
        pin_rgbd = torch.empty((h, 4 * w, 3), dtype=torch.uint8).pin_memory()
        pin_depth = torch.empty((h, 2 * w, 4), dtype=torch.uint8).pin_memory()

        def hip_spiral():
            f = Fr.rgbd_frame(t["render"], t["depth"], t["uncertainty"], t["normal"], panels=True)
            pin_rgbd.copy_(f.rgbd, non_blocking=True)
            return f

        def hip_test():
            f = Fr.view_frames(t["render"], t["uncertainty"], t["gt"], t["depth"], t["midas"], t["mask"])
            pin_rgbd.copy_(f.sheet, non_blocking=True)
            pin_depth.copy_(f.depth, non_blocking=True)
            return f

        paths = {"reference_spiral": lambda: reference_spiral(t, inferno), "hip_spiral": hip_spiral,
                 "reference_test": lambda: reference_test(t, to_rgba), "hip_test": hip_test}
        samples = {p: {"event": [], "wall": []} for p in paths}
        for i in range(a.warmup + a.rounds):  # alternate the paths round by round
            for p, fn in paths.items():
                event, wall, out = timed(fn)
                if p.startswith("hip"):
                    assert Fr.last_path == "hip"
                if i >= a.warmup:
                    samples[p]["event"].append(event)
                    samples[p]["wall"].append(wall)
                del out
        row = {"h": h, "w": w, "rounds": a.rounds, "warmup": a.warmup}
        for p, s in samples.items():
            for kind in ("event", "wall"):
                row[f"{p}_{kind}_ms"] = statistics.median(s[kind])
                row[f"{p}_{kind}_ms_min_max"] = [min(s[kind]), max(s[kind])]
        for form in ("spiral", "test"):
            row[f"{form}_wall_ratio"] = row[f"reference_{form}_wall_ms"] / row[f"hip_{form}_wall_ms"]
        row["spiral_host_bytes_reference_fp32"] = 4 * h * w * (1 + 3 + 3 + 3)  # the depth and the three fp32 .cpu() copies
        row["spiral_host_bytes_hip"] = 12 * h * w
        rows.append(row)
        print(json.dumps(row), flush=True)
        del t, pin_rgbd, pin_depth, paths
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "depth_panel_by": panel_by,
              "what": "one frame of render_set from the render to the last byte on the host, no PNG encoding on either side: event_ms = HIP "
                      "events around one call, wall_ms = host clock from an idle device to the synchronise behind it; medians over the "
                      "timed rounds with min and max, the paths alternating in one process; reference_* = the reference's sequence "
                      "restated in torch and numpy with its .cpu() copies, hip_* = gscream_amd.frames and its copies into pinned memory",
              "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
