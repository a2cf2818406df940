"""Test-view metrics on the HIP path: what the reference's evaluate() (train.py:905-990) and training_report (train.py:655-708) log.

Drop-ins under the reference's names and signatures; integration is two rebindings (INTEGRATION R):

    from gscream_amd.metrics import psnr      # for: from utils.image_utils import psnr
    from gscream_amd.metrics import my_ssim   # for: from utils.loss_utils import my_ssim

or `evaluate_views(renders, gts, masks, image_names)` for the loop of evaluate() in one launch per 65535 planes and one read-back,
or `image_metrics(pred, gt, mask)` for the per-image device tensors.  The rules (include/gsraster.h has them in full):

  transform  clamp: x := min(max(x, 0), 1);  quantize: x := trunc(min(max(x*255 + 0.5, 0), 255)) / 255 (save_image + to_tensor, the
             PNG round trip between render_set and evaluate()); fp32, one rounding per operation, pred and gt alike
  d = x - y  in fp32;  l1 = mean |d|, mse = mean d^2, psnr = -10 log10(mse), the sums and quotients in fp64
  ssim       5x5 Gaussian window (sigma 1.5, taps in fp64), reflect padding without repeating the edge; mu, E[x^2], E[y^2], E[xy] and
             the variances E[.] - mu^2 in fp64; ssim_map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2) + 1e-12),
             dssim = clamp((1 - ssim_map) / 2, 0, 1), ssim = 1 - 2 mean(dssim)
  each over all C*H*W elements of an image and over the elements where the mask is true; every value rounded to fp32 once.

The PSNR half is pinned by a run of the reference's utils/image_utils.py (tests/golden/ref_metrics.npz).  The SSIM half is not pinned by
a reference run: my_ssim is kornia 0.6.12's metrics.ssim(img1, img2, 5, 1.0, 1e-12, 'same'), kornia is not on this stack, and the
expression above is written down from its source.  The reference evaluates E[x^2] - mu^2 in fp32 against C2 = 9e-4; both paths here
carry the window sums in fp64 and return the value the expression defines (the measured gap: INTEGRATION R).

The HIP path (gscream_amd/csrc/metrics.hip; `last_path = "hip"`) takes fp32, contiguous tensors on a HIP device with H, W >= 3; it
launches on torch's current stream, allocates its workspace and outputs, reads nothing back and never synchronises.  Everything else
-- CPU tensors, other dtypes, `force_torch = True` -- takes `_metrics_torch`, a torch statement of the same rules
(`last_path = "torch"`).  A missing library raises; nothing falls back quietly."""
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F

from . import _native

__all__ = ["ImageMetrics", "image_metrics", "mse", "psnr", "my_ssim", "evaluate_views"]

force_torch = False
last_path = None  # "hip" / "torch": the path the last call took

MAX_PLANES = 65535         # gsr_image_metrics: B*C per call
MAX_ELEMENTS = 0x7FFFFF00  # its limit on C*H*W
CLAMP, QUANTIZE = _native.METRICS_CLAMP, _native.METRICS_QUANTIZE
C1, C2, SSIM_EPS = 1e-4, 9e-4, 1e-12
FIELDS = ("l1", "mse", "psnr", "ssim", "l1_masked", "mse_masked", "psnr_masked", "ssim_masked")


class ImageMetrics(NamedTuple):
    """[B] fp32 device tensors, and `sums` [B, 8] fp64 = {n, sum|d|, sum d^2, sum dssim} over the image, then under the mask."""
    l1: torch.Tensor
    mse: torch.Tensor
    psnr: torch.Tensor
    ssim: torch.Tensor
    l1_masked: torch.Tensor
    mse_masked: torch.Tensor
    psnr_masked: torch.Tensor
    ssim_masked: torch.Tensor
    sums: torch.Tensor


def window_taps():
    """g_k = exp(-(k-2)^2 / 4.5) / sum, k = 0 .. 4, in fp64 (the library forms them the same way)."""
    e = [math.exp(-((k - 2) ** 2) / 4.5) for k in range(3)]
    total = ((e[0] + e[1]) + e[2]) + (e[1] + e[0])
    g = [v / total for v in e]
    return [g[0], g[1], g[2], g[1], g[0]]


# ---- arguments ----
def _images(pred, gt):
    if not (isinstance(pred, torch.Tensor) and isinstance(gt, torch.Tensor)):
        raise TypeError("image metrics: pred and gt are tensors")
    if pred.dim() == 3:
        pred = pred[None]
    if gt.dim() == 3:
        gt = gt[None]
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError(f"image metrics: pred is {tuple(pred.shape)}, gt is {tuple(gt.shape)} (need equal [C,H,W] or [B,C,H,W])")
    if pred.device != gt.device:
        raise ValueError(f"image metrics: pred is on {pred.device}, gt on {gt.device}")
    return pred, gt


def _mask4(mask, shape, device):
    """A bool mask of shape [H,W], [1,H,W], [B,1,H,W] or [B,C,H,W] -> an expanded [B,C,H,W] view.  Only the batch and channel dimensions
    broadcast: the last two are the image's H and W, so the view's rows are the mask's own."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise TypeError("image metrics: the mask is a torch.bool tensor")
    if mask.device != device:
        raise ValueError(f"image metrics: the mask is on {mask.device}, the images on {device}")
    if mask.dim() < 2 or mask.dim() > 4 or tuple(mask.shape[-2:]) != tuple(shape[-2:]):
        raise ValueError(f"image metrics: the mask is {tuple(mask.shape)} (need [H,W], [1,H,W], [B,1,H,W] or [B,C,H,W] for images of {tuple(shape)})")
    while mask.dim() < 4:
        mask = mask[None]
    try:
        return mask.expand(shape)
    except RuntimeError:
        raise ValueError(f"image metrics: a mask of {tuple(mask.shape)} does not broadcast to {tuple(shape)}") from None


def _mask_for_kernel(mask, shape, device):
    """-> the expanded view the kernel reads as bytes through (stride_b, stride_c, W, 1): a mask whose [H,W] planes are not dense rows
    of W is made contiguous first (its H and W are the image's, so that fixes them); broadcast batch / channel dimensions keep
    stride 0.  Anything else would send the kernel past the mask's storage, so it raises."""
    m4 = _mask4(mask, shape, device)
    if m4 is None:
        return None
    W = shape[3]
    if m4.stride(3) != 1 or m4.stride(2) != W:
        m4 = _mask4(mask.contiguous(), shape, device)
    if m4.stride(3) != 1 or m4.stride(2) != W or m4.stride(0) < 0 or m4.stride(1) < 0:
        raise RuntimeError(f"image metrics: mask strides {m4.stride()} are not (b, c, {W}, 1)")
    return m4


def _hip_tensor(t):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


# ---- the torch statement ----
def _transform_torch(x, clamp, quantize):
    """The input transform in fp32; each eager operation rounds once, torch.clamp keeps a NaN."""
    x = x.to(torch.float32)
    if clamp:
        x = torch.clamp(x, 0.0, 1.0)
    if quantize:
        q = x * 255.0
        q = q + 0.5
        x = torch.trunc(torch.clamp(q, 0.0, 255.0)) / 255.0
    return x


def _dssim_map_torch(x, y, dtype):
    """x, y [B,C,H,W] fp32 (transformed) -> the dssim map in `dtype`.  float64: the rules (fp64 taps, the window separable: rows, then
    columns); float32: the reference's arithmetic (fp32 taps, their outer product as one 5x5 depthwise conv2d, the variances in fp32)."""
    B, C, H, W = x.shape
    if dtype == torch.float32:
        g = torch.tensor(window_taps(), dtype=torch.float32, device=x.device)
        kernel = (g[:, None] @ g[None, :])[None, None].expand(C, 1, 5, 5).contiguous()

        def filt(t):
            return F.conv2d(F.pad(t, (2, 2, 2, 2), mode="reflect"), kernel, groups=C)
    else:
        taps = window_taps()
        x, y = x.to(dtype), y.to(dtype)

        def filt(t):
            p = F.pad(t, (2, 2, 2, 2), mode="reflect")
            rows = sum(taps[k] * p[..., k:k + W] for k in range(5))
            return sum(taps[k] * rows[..., k:k + H, :] for k in range(5))
    mu1, mu2 = filt(x), filt(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = filt(x * x) - mu1_sq, filt(y * y) - mu2_sq, filt(x * y) - mu1_mu2
    num = (2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2)
    den = (mu1_sq + mu2_sq + C1) * (s1 + s2 + C2)
    return torch.clamp((1.0 - num / (den + SSIM_EPS)) / 2, min=0, max=1)


def _metrics_torch(pred, gt, mask=None, clamp=False, quantize=False, dtype=torch.float64):
    """The rules in torch: pred, gt [B,C,H,W], mask None or bool as image_metrics takes it -> (sums [B,8] fp64, metrics [B,8] fp32).
    dtype=float64 is the product's fallback and synchronises nowhere.  dtype=float32 is the reference's arithmetic -- fp32 taps, a full
    5x5 conv2d, `torch.mean` in fp32 and the boolean-mask gather of `value[valid_mask]`, image by image -- and exists for
    tools/metrics_bench.py and the gap measurement only; its `sums` are its fp32 means times the counts."""
    pred, gt = _images(pred, gt)
    m4 = _mask4(mask, pred.shape, pred.device)
    B = pred.shape[0]
    n = pred[0].numel()
    x, y = _transform_torch(pred, clamp, quantize), _transform_torch(gt, clamp, quantize)
    d = x - y
    ds = _dssim_map_torch(x, y, dtype)
    if dtype == torch.float32:
        def four(b, select):
            l1, ms, dm = torch.mean(select(d[b].abs())), torch.mean(select(d[b] ** 2)), torch.mean(select(ds[b]))
            return [l1, ms, -10 * torch.log10(ms), 1 - 2 * dm]

        rows = []
        for b in range(B):
            plain = four(b, lambda v: v)
            rows.append(torch.stack(plain + (plain if m4 is None else four(b, lambda v: v[m4[b]]))))
        metrics = torch.stack(rows)
        whole = pred.new_full((B,), n, dtype=torch.float64)
        halves = []
        for h, count in ((0, whole), (4, whole if m4 is None else m4.reshape(B, -1).sum(1).double())):
            m = metrics[:, h:h + 4].double()
            halves += [count, m[:, 0] * count, m[:, 1] * count, (1 - m[:, 3]) / 2 * count]
        return torch.stack(halves, 1), metrics
    d64 = d.to(torch.float64)
    vals = (d64.abs(), d64 * d64, ds.to(torch.float64))
    cols = [pred.new_full((B,), n, dtype=torch.float64)] + [v.reshape(B, -1).sum(1) for v in vals]
    if m4 is None:
        cols = cols + cols
    else:  # selected, not multiplied: a NaN outside the mask stays outside
        cols += [m4.reshape(B, -1).sum(1).to(torch.float64)] + [torch.where(m4, v, v.new_zeros(())).reshape(B, -1).sum(1) for v in vals]
    sums = torch.stack(cols, 1)
    out = []
    for h in (0, 4):
        cnt = sums[:, h]
        ms = sums[:, h + 2] / cnt
        out += [sums[:, h + 1] / cnt, ms, -10.0 * torch.log10(ms), 1.0 - 2.0 * (sums[:, h + 3] / cnt)]
    return sums, torch.stack(out, 1).to(torch.float32)


# ---- the call ----
def _run(pred, gt, mask, clamp, quantize):
    """-> (sums [B,8] fp64, metrics [B,8] fp32) on the images' device."""
    global last_path
    pred, gt = _images(pred, gt)
    B, C, H, W = pred.shape
    if (force_torch or not _hip_tensor(pred) or not _hip_tensor(gt) or B == 0 or C == 0 or C > MAX_PLANES or H < 3 or W < 3
            or C * H * W >= MAX_ELEMENTS):
        last_path = "torch"
        return _metrics_torch(pred, gt, mask, clamp, quantize, torch.float64)
    m4 = _mask_for_kernel(mask, pred.shape, pred.device)
    last_path = "hip"
    dev = pred.device
    lib = _native.load()
    sums = torch.empty((B, 8), dtype=torch.float64, device=dev)
    metrics = torch.empty((B, 8), dtype=torch.float32, device=dev)
    per_call = MAX_PLANES // C
    workspace = torch.empty(int(lib.gsr_image_metrics_workspace_bytes(min(B, per_call), C, H, W)), dtype=torch.uint8, device=dev)
    flags = (CLAMP if clamp else 0) | (QUANTIZE if quantize else 0)
    for b0 in range(0, B, per_call):
        b1 = min(b0 + per_call, B)
        mp, sb, sc = (None, 0, 0) if m4 is None else (_native.ptr(m4[b0:b1]), m4.stride(0), m4.stride(1))
        _native.run("gsr_image_metrics", dev, b1 - b0, C, H, W, _native.ptr(pred[b0:b1]), _native.ptr(gt[b0:b1]), mp, sb, sc, flags,
                    _native.ptr(workspace), _native.ptr(sums[b0:b1]), _native.ptr(metrics[b0:b1]))
    return sums, metrics


def image_metrics(pred, gt, mask=None, clamp=False, quantize=False):
    """pred, gt [C,H,W] or [B,C,H,W]; mask None or torch.bool [H,W], [1,H,W], [B,1,H,W] or [B,C,H,W] (an expanded stride-0 channel
    dimension is passed on as stride 0, never materialised) -> ImageMetrics of [B] tensors.  Without a mask the masked fields equal
    the unmasked ones; an empty mask gives NaN in them."""
    sums, metrics = _run(pred, gt, mask, clamp, quantize)
    return ImageMetrics(*metrics.unbind(1), sums)


# ---- the reference's names ----
def _mean_value(image_pred, image_gt, mask, column):
    """The reference's mean over everything it is given.  One image: the field of image_metrics itself.  A batch: the images' sums
    added in fp64 and divided once (the reference's mean over the batch, or over all selected elements), rounded to fp32."""
    _images(image_pred, image_gt)  # (the shapes checked before anything runs)
    sums, metrics = _run(image_pred, image_gt, mask, False, False)
    h = 0 if mask is None else 4
    if metrics.shape[0] == 1:
        return metrics[0, column + h]
    total = sums.sum(0)
    if column == 3:
        return (1.0 - 2.0 * (total[h + 3] / total[h])).to(torch.float32)
    value = total[h + 2] / total[h]
    return (value if column == 1 else -10.0 * torch.log10(value)).to(torch.float32)


def mse(image_pred, image_gt, valid_mask=None, reduction="mean"):
    """utils/image_utils.py:22-28.  reduction != "mean" returns the (selected) squared differences, as the reference does, in torch."""
    global last_path
    if reduction != "mean":
        last_path = "torch"
        value = (image_pred - image_gt) ** 2
        return value if valid_mask is None else value[valid_mask]
    return _mean_value(image_pred, image_gt, valid_mask, 1)


def psnr(image_pred, image_gt, valid_mask=None, reduction="mean"):
    """utils/image_utils.py:31-32."""
    if reduction != "mean":
        return -10 * torch.log10(mse(image_pred, image_gt, valid_mask, reduction))
    return _mean_value(image_pred, image_gt, valid_mask, 2)


def my_ssim(image_pred, image_gt, mask=None, reduction="mean"):
    """utils/loss_utils.py:123-128: 1 - 2 mean(dssim), in [-1, 1].  The reference does not pass `reduction` on to ssim_loss, so every value
    of it gives the mean; here a value other than "mean" gives that same mean by the torch path."""
    global force_torch
    if reduction == "mean":
        return _mean_value(image_pred, image_gt, mask, 3)
    before, force_torch = force_torch, True
    try:
        return _mean_value(image_pred, image_gt, mask, 3)
    finally:
        force_torch = before


# ---- evaluate()'s loop ----
def _stack(images):
    return torch.cat([t[None] if t.dim() == 3 else t for t in images])


def _stack_masks(masks):
    """[1,C,H,W] masks whose channel dimension is an expand (stride 0), as readImages builds them, stay [B,1,H,W]."""
    four = []
    for m in masks:
        while m.dim() < 4:
            m = m[None]
        four.append(m[:, :1] if m.shape[1] > 1 and m.stride(1) == 0 else m)
    channels = max(m.shape[1] for m in four)
    return torch.cat([m.expand(-1, channels, -1, -1) for m in four])


def evaluate_views(renders, gts, masks=None, image_names=None, quantize=True, lpips=None):
    """The metric loop of evaluate() (train.py:943-953, :981-987), without LPIPS unless a model is passed: lists of equally sized images ([C,H,W] or [1,C,H,W]) and of
    bool masks -> (full, per_view) with the keys "SSIM", "PSNR", "masked SSIM", "masked PSNR": full[key] is the fp32 mean of the fp32
    per-view values, as evaluate() takes it; per_view[key] maps image name to value.  quantize=True applies the PNG round trip that
    lies between render_set and evaluate() to float images (a no-op on images read back from PNG).  One call per 65535 planes, one
    read-back.  Without masks the masked keys repeat the unmasked values.  lpips: a gscream_amd.lpips.LPIPS model adds the keys "LPIPS"
    and "masked LPIPS" (lpips.lpips_views on the images as they are, 2*x-1 applied: train.py:948, :952-953; without masks the masked
    key is the mean of the spatial map); their values join the one read-back.  Without it the result is exactly the four keys."""
    if len(renders) == 0 or len(renders) != len(gts) or (masks is not None and len(masks) != len(renders)):
        raise ValueError("evaluate_views: renders, gts and masks are non-empty lists of one length")
    names = [str(i) for i in range(len(renders))] if image_names is None else list(image_names)
    if len(names) != len(renders):
        raise ValueError("evaluate_views: one name per view")
    _sums, metrics = _run(_stack(renders), _stack(gts), None if masks is None else _stack_masks(masks), False, quantize)
    columns = (("SSIM", 3), ("PSNR", 2), ("masked SSIM", 7), ("masked PSNR", 6))
    if lpips is not None:
        from . import lpips as _lpips
        plain, masked = _lpips.lpips_views(lpips, renders, gts, masks)
        metrics = torch.cat([metrics, plain.to(metrics.device)[:, None], masked.to(metrics.device)[:, None]], 1)
        columns += (("LPIPS", 8), ("masked LPIPS", 9))
    host = metrics.cpu()  # the one read-back
    full, per_view = {}, {}
    for key, column in columns:
        values = host[:, column].contiguous()
        full[key] = values.mean().item()
        per_view[key] = dict(zip(names, values.tolist()))
    return full, per_view
