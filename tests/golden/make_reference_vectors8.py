"""Golden vectors for the PSNR half of the test-view metrics, produced by RUNNING the reference's own utils/image_utils.py.

    python tests/golden/make_reference_vectors8.py        # needs /root/reference; runs on the CPU

utils/image_utils.py imports only torch, so it is loaded in place and unmodified; nothing of the reference is copied, only inputs and
the fp32 values `mse` / `psnr` returned are stored (ref_metrics.npz).  The SSIM half (my_ssim) is kornia's metrics.ssim; kornia
cannot be imported on this stack, so nothing of it is stored: that half rests on the written rule (include/gsraster.h).

Per case, prefix "<case>/": pred, gt [1,3,h,w] fp32; mask [1,1,h,w] bool (given to the reference as evaluate() builds it: expanded to
[1,3,h,w]); mse, psnr, mse_masked, psnr_masked: the reference's 0-d fp32 results.

  tiny    3x3     every window tap reflected
  wide    3x70    one dimension all halo
  tall    70x3
  smooth  37x53   a smooth image and a noisy copy, PSNR ~ 34 dB
  noise   37x53   two uniform-noise images

The figures printed at the end (the reference's fp32 results against the fp64 oracle of tests/metrics_helpers.py) are the bound that
tests/test_metrics.py measures again and holds the torch path to.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF_IMAGE_UTILS = "/root/reference/utils/image_utils.py"
CASES = {"tiny": (3, 3), "wide": (3, 70), "tall": (70, 3), "smooth": (37, 53), "noise": (37, 53)}


def load_reference():
    spec = importlib.util.spec_from_file_location("reference_image_utils", REF_IMAGE_UTILS)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def case_inputs(name, seed):
    from metrics_helpers import noise_pair, random_mask, smooth_pair
    h, w = CASES[name]
    pred, gt = noise_pair(h, w, seed=seed) if name == "noise" else smooth_pair(h, w, seed=seed)
    mask = random_mask((1, 1, h, w), seed)
    mask[0, 0, 0, 0], mask[0, 0, -1, -1] = True, False  # neither empty nor full, whatever the size
    return pred, gt, mask


def main():
    from metrics_helpers import metrics_oracle
    ref = load_reference()
    out = {}
    for seed, name in enumerate(CASES):
        pred, gt, mask = case_inputs(name, seed)
        p, g = torch.from_numpy(pred), torch.from_numpy(gt)
        m = torch.from_numpy(mask).expand(1, 3, -1, -1)
        with torch.no_grad():
            got = {"mse": ref.mse(p, g), "psnr": ref.psnr(p, g), "mse_masked": ref.mse(p, g, m), "psnr_masked": ref.psnr(p, g, m)}
        assert all(v.dtype == torch.float32 and v.dim() == 0 for v in got.values())
        o = metrics_oracle(pred, gt, mask)["metrics"][0]
        want = {"mse": o[1], "psnr": o[2], "mse_masked": o[5], "psnr_masked": o[6]}
        print(name, CASES[name], {k: (float(v), abs(float(v) - want[k]) / abs(want[k])) for k, v in got.items()})
        out.update({f"{name}/pred": pred, f"{name}/gt": gt, f"{name}/mask": mask})
        out.update({f"{name}/{k}": v.numpy().copy() for k, v in got.items()})
    out["cases"] = np.array(list(CASES))
    path = os.path.join(HERE, "ref_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
