"""The anchor sampler of GScream's cross-attention step (train.py:436-511) on the device, and the step itself.

From what `prefilter_position2D` returns, the view's mask and the patch rectangle, `sample_crossattn_anchors` gives the two anchor
sets `run_crossattn` pairs up.  Per anchor a, x = position2D_x[a], y = position2D_y[a], image h x w, rect = (min_y, max_y, min_x, max_x):

    valid    visible[a] and 0 < x < w and 0 < y < h          strict, floating point; NaN is invalid
    pixel    (int)y, (int)x                                  truncation, as .long()
    sampled  valid and min_y <= py < max_y and min_x <= px < max_x
    label    (long)gt_mask[py, px]
    fg       sampled and label > 0;   bg  sampled and label == 0   (a negative label is in neither class)
    ok       n_fg > 11 and n_bg > 11                         (the reference's exit() guards inside its bare except)
    min_num  min(n_fg, n_bg, max_pairs)
    src      a uniformly random min_num-subset of fg;   dst the same of bg;   both empty when not ok

The reference draws the subsets with randperm and keeps only the sets.  Here every anchor gets a 32-bit key from a keyed bijection
of its index, and a class's subset is its min_num members with the smallest (key, index).  Modulo 2^32, with s_lo / s_hi the
halves of a 64-bit seed drawn from torch's CPU generator (torch.manual_seed makes a run repeatable) and i the anchor index:

    mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
    key(i) = mix(((mix((i ^ s_lo) + s_hi)) + s_lo) ^ s_hi)

fp32 CUDA inputs take gsr_anchor_sample (gscream_amd/csrc/anchor_sample.hip): a fixed number of launches, no host stop; a missing
library raises.  CPU tensors, or force_torch=True, take the torch statement of the same rules below (it may synchronise; it is
what the CPU tests run).  `last_path` says which one the last call took ("hip" / "torch").

`crossattn_step` is the whole step: sample, read `info` once (the one host stop: the reference's `continue` needs the host to know
`ok`, the attention shapes need `min_num`), run_crossattn_rows.  The rectangle stays the caller's job (sample_patch_in_mask_region)."""
import ctypes

import torch

from . import _native
from .crossattn import run_crossattn_rows

__all__ = ["sample_crossattn_anchors", "crossattn_step", "anchor_keys", "draw_seed"]

MASK32 = 0xFFFFFFFF
last_path = None  # "hip" / "torch": the path the last sample_crossattn_anchors() took


def draw_seed():
    """A 64-bit seed from torch's CPU generator (two 32-bit draws, high word first)."""
    hi, lo = (int(v) for v in torch.randint(0, 1 << 32, (2,), dtype=torch.int64))
    return (hi << 32) | lo


def _mix(x):
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & MASK32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & MASK32
    return x ^ (x >> 16)


def anchor_keys(index, seed):
    """key(i) of the module docstring for an int64 tensor of anchor indices -> int64 in [0, 2^32)."""
    s_lo, s_hi = seed & MASK32, (seed >> 32) & MASK32
    x = _mix((((index & MASK32) ^ s_lo) + s_hi) & MASK32)
    return _mix(((x + s_lo) & MASK32) ^ s_hi)


def _mask2d(gt_mask):
    if gt_mask.dim() < 2 or gt_mask.numel() != gt_mask.shape[-2] * gt_mask.shape[-1]:
        raise ValueError(f"gt_mask must be [h, w] (leading dimensions of 1 allowed), got {tuple(gt_mask.shape)}")
    return gt_mask.reshape(gt_mask.shape[-2], gt_mask.shape[-1])


def _sample_torch(visible, x, y, gt, rect, max_pairs, seed):
    h, w = int(gt.shape[0]), int(gt.shape[1])
    min_y, max_y, min_x, max_x = (int(v) for v in rect)
    N, dev = int(visible.shape[0]), visible.device
    valid = visible.bool() & (x > 0) & (x < w) & (y > 0) & (y < h)
    px = torch.where(valid, x, torch.zeros_like(x)).long()
    py = torch.where(valid, y, torch.zeros_like(y)).long()
    sampled = valid & (py >= min_y) & (py < max_y) & (px >= min_x) & (px < max_x)
    label = gt[py, px].long()
    classes = sampled & (label > 0), sampled & (label == 0)
    n_sampled, n_fg, n_bg = int(sampled.sum()), int(classes[0].sum()), int(classes[1].sum())
    ok = n_fg > 11 and n_bg > 11
    min_num = min(n_fg, n_bg, int(max_pairs))
    masks, rows = [], []
    for cls in classes:
        mask = torch.zeros(N, dtype=torch.bool, device=dev)
        row = torch.full((int(max_pairs),), -1, dtype=torch.int64, device=dev)
        if ok and min_num > 0:
            members = torch.nonzero(cls).reshape(-1)
            order = torch.argsort((anchor_keys(members, seed) << 31) + members)  # (key, index): index < 2^31, key < 2^32
            chosen = torch.sort(members[order[:min_num]]).values
            mask[chosen] = True
            row[:min_num] = chosen
        masks.append(mask)
        rows.append(row)
    info = torch.tensor([n_sampled, n_fg, n_bg, min_num, int(ok), 0, 0, 0], dtype=torch.int32, device=dev)
    return masks[0], masks[1], rows[0], rows[1], info


def _sample_hip(visible, x, y, gt, rect, max_pairs, seed, src_rows, dst_rows):
    """gsr_anchor_sample into the caller's row lists (int64 [max_pairs]; entries from min_num on are left as they are)."""
    lib = _native.load()
    N, dev = int(visible.shape[0]), visible.device
    visible = visible.detach().to(torch.bool).contiguous()
    x, y, gt = x.detach().contiguous(), y.detach().contiguous(), gt.detach().contiguous()
    src_mask = torch.empty(N, dtype=torch.bool, device=dev)
    dst_mask = torch.empty(N, dtype=torch.bool, device=dev)
    info = torch.empty(8, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.gsr_anchor_sample_workspace_bytes(N, int(max_pairs))), dtype=torch.uint8, device=dev)
    min_y, max_y, min_x, max_x = (max(-(1 << 31), min((1 << 31) - 1, int(v))) for v in rect)
    _native.run(
        "gsr_anchor_sample", dev,
        N, int(gt.shape[0]), int(gt.shape[1]), _native.ptr(visible), _native.ptr(x), _native.ptr(y), _native.ptr(gt), min_y, max_y,
        min_x, max_x, int(max_pairs), ctypes.c_uint64(seed), _native.ptr(ws), _native.ptr(src_mask), _native.ptr(dst_mask),
        _native.ptr(src_rows), _native.ptr(dst_rows), _native.ptr(info))
    return src_mask, dst_mask, src_rows, dst_rows, info


def sample_crossattn_anchors(visible_mask, position2D_x, position2D_y, gt_mask, rect, max_pairs=2000, seed=None, force_torch=False):
    """-> (src_mask, dst_mask [N] bool, src_rows, dst_rows [max_pairs] int64, info [8] int32 on the inputs' device).
    rows[:min_num] are the selected anchors in ascending order (= nonzero of the mask), the rest is -1;
    info = (n_sampled, n_fg, n_bg, min_num, ok, 0, 0, 0).  rect = (min_y, max_y, min_x, max_x); seed=None draws one (draw_seed)."""
    global last_path
    if not (visible_mask.dim() == 1 and visible_mask.shape == position2D_x.shape == position2D_y.shape):
        raise ValueError("visible_mask, position2D_x and position2D_y must be one-dimensional and of one length")
    if int(max_pairs) < 0:
        raise ValueError(f"max_pairs must be >= 0 (got {max_pairs})")
    seed = draw_seed() if seed is None else int(seed) & ((1 << 64) - 1)
    gt = _mask2d(gt_mask)
    if gt.dtype != torch.float32:
        gt = gt.float()
    x, y = position2D_x, position2D_y
    if visible_mask.is_cuda and not force_torch:
        if not (x.is_cuda and y.is_cuda and gt.is_cuda and x.dtype == y.dtype == torch.float32):
            raise RuntimeError("sample_crossattn_anchors: the HIP path takes fp32 CUDA positions and a CUDA mask")
        last_path = "hip"
        rows = torch.full((2, int(max_pairs)), -1, dtype=torch.int64, device=visible_mask.device)
        return _sample_hip(visible_mask, x, y, gt, rect, max_pairs, seed, rows[0], rows[1])
    last_path = "torch"
    return _sample_torch(visible_mask, x.float(), y.float(), gt, rect, max_pairs, seed)


def crossattn_step(model, visible_mask, position2D_x, position2D_y, gt_mask, rect, ema, is_ref, max_pairs=2000):
    """The cross-attention step of one training iteration (train.py:436-521) -> the reference's `cross_flag`.  False (and the model
    untouched) where the reference prints 'No valid sampled anchors...' and continues."""
    _src_mask, _dst_mask, src_rows, dst_rows, info = sample_crossattn_anchors(visible_mask, position2D_x, position2D_y, gt_mask, rect,
                                                                              max_pairs=max_pairs)
    n = info.tolist()  # the one host stop of the step
    if not n[4]:
        return False
    run_crossattn_rows(model, src_rows[:n[3]], dst_rows[:n[3]], ema=ema, is_ref=is_ref)
    return True
