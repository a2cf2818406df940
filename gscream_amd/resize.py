"""PIL's Image.resize on the HIP path: byte for byte for 8-bit pictures, bit for bit for mode F.  This is the step between a decoded
picture and the tensor a Camera or a metric holds: readImages (train.py:887-902) resizes every mask with LANCZOS, loadCam
(utils/camera_utils.py:19-102) sends every image, mask and depth map through pil_image.resize(resolution) (utils/general_utils.py:35-75).

Integration (INTEGRATION X):

    mask.resize((W, H), Image.LANCZOS) + to_tensor + upload   ->  resize.resize(mask_u8, (W, H), resize.LANCZOS)
    pil_image.resize(resolution), np.array, upload            ->  resize.resize_pil_image(pil_image, resolution)
    PILtoTorch / PILtoTorch_01mask / PILtoTorch_depth         ->  gscream_amd.general_utils (the resize and the last step in two launches)

PIL's rule is closed: separable coefficient tables built in double, two passes, integer fixed point with a rounded uint8 intermediate
for 8-bit, sequential fp64 sums with a float32 intermediate for F (include/gsraster.h, "Resize", has it in full).  The host builds the
tables (`coefficients`, cached per (in, out, filter); their device copies cached per device as well), the device runs one launch per
axis (gscream_amd/csrc/resize.hip, `last_path = "hip"`) on torch's current stream with no host stop.

Host path (`last_path = "pil"`): CPU tensors, `force_host = True`, HAMMING (its mode-F rule is not restated here) and dtypes other
than uint8 / float32 go through PIL itself and are uploaded.  PIL premultiplies alpha around the resample for LA / RGBA and forces
NEAREST for modes 1 and P: `resize_pil_image` keeps those on the host too.  A missing library raises; nothing falls back quietly."""
import ctypes
import math

import numpy as np
import torch

from . import _native

__all__ = ["NEAREST", "LANCZOS", "BILINEAR", "BICUBIC", "BOX", "HAMMING", "coefficients", "fixed_point", "nearest_index", "resize",
           "resize_pil_image", "clear_cache"]

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5  # PIL.Image.Resampling
PRECISION_BITS = 22
_SUPPORT = {BOX: 0.5, BILINEAR: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
_MAX_SIDE = 65535  # what one launch takes (include/gsraster.h)

force_host = False
last_path = None  # "hip" / "pil": the path the last resize took
last_launches = 0  # native calls of the last resize on the HIP path

_tables = {}   # (in, out, filter) -> (bounds, coeffs) on the host
_nearest = {}  # (in, out) -> index table on the host
_device = {}   # (device, kind, in, out, filter) -> device tensors


def clear_cache():
    """Forget the host tables and their device copies (tests that want the uploads inside their own allocator)."""
    _tables.clear()
    _nearest.clear()
    _device.clear()


def _filter_values(resample, x):
    """f(x) elementwise in double, every operation in PIL's order."""
    if resample == BOX:
        return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)
    if resample == BILINEAR:
        x = np.abs(x)
        return np.where(x < 1.0, 1.0 - x, 0.0)
    if resample == BICUBIC:
        a = -0.5
        x = np.abs(x)
        near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        far = (((x - 5) * x + 8) * x - 4) * a
        return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))
    if resample == LANCZOS:
        def sinc(v):
            v = v * math.pi
            flat = v.reshape(-1)
            s = np.array([math.sin(t) for t in flat.tolist()], np.float64).reshape(v.shape)  # libm's sine, not numpy's
            with np.errstate(invalid="ignore", divide="ignore"):
                return np.where(v == 0.0, 1.0, s / v)
        return np.where((x >= -3.0) & (x < 3.0), sinc(x) * sinc(x / 3), 0.0)
    raise ValueError(f"resize: unknown filter {resample!r} (have NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX; HAMMING on the host path)")


def coefficients(in_size, out_size, resample):
    """-> (bounds int32 [out, 2] = (xmin, n), coeffs float64 [out, ksize], zero behind n) of one axis, as PIL builds them; cached."""
    in_size, out_size = int(in_size), int(out_size)
    key = (in_size, out_size, resample)
    hit = _tables.get(key)
    if hit is not None:
        return hit
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resize: sizes must be positive (got {in_size} -> {out_size})")
    if resample not in _SUPPORT:
        raise ValueError(f"resize: no coefficient table for filter {resample!r} (have LANCZOS, BILINEAR, BICUBIC, BOX)")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = _SUPPORT[resample] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)  # (astype truncates towards zero, as C's cast does)
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    inside = x < n[:, None]
    w = np.where(inside, _filter_values(resample, ((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]  # a sequential sum in index order (the zeros behind n add nothing)
    with np.errstate(invalid="ignore", divide="ignore"):
        kk = np.where(ww != 0.0, w / ww, w)
    kk = np.ascontiguousarray(np.where(inside, kk, 0.0))
    bounds = np.ascontiguousarray(np.stack([xmin, n], 1).astype(np.int32))
    kk.setflags(write=False)
    bounds.setflags(write=False)
    _tables[key] = (bounds, kk)
    return _tables[key]


def fixed_point(coeffs):
    """The 8-bit tables: int32 trunc(k 2^22 +- 0.5), with the sign of k."""
    coeffs = np.asarray(coeffs, np.float64)
    scaled = coeffs * float(1 << PRECISION_BITS)
    return np.where(coeffs < 0, -0.5 + scaled, 0.5 + scaled).astype(np.int32)


def nearest_index(in_size, out_size):
    """NEAREST's index table of one axis: the ACCUMULATED xo = 0.5 a, xo += a (a = in / out), index int(xo); cached."""
    in_size, out_size = int(in_size), int(out_size)
    key = (in_size, out_size)
    hit = _nearest.get(key)
    if hit is not None:
        return hit
    if in_size < 1 or out_size < 1:
        raise ValueError(f"resize: sizes must be positive (got {in_size} -> {out_size})")
    a = in_size / out_size
    idx = np.cumsum(np.concatenate([[a * 0.5], np.full(out_size - 1, a)])).astype(np.int64)  # cumsum adds in index order
    idx = np.minimum(idx, in_size - 1).astype(np.int32)
    idx.setflags(write=False)
    _nearest[key] = idx
    return idx


def _device_tables(device, kind, in_size, out_size, resample):
    """The device copies of one axis' tables: kind "u8" -> (bounds, int32 K, ksize), "f32" -> (bounds, double k, ksize), "nearest" -> (idx,)."""
    key = (device, kind, in_size, out_size, resample)
    hit = _device.get(key)
    if hit is None:
        if kind == "nearest":
            hit = (torch.from_numpy(np.array(nearest_index(in_size, out_size))).to(device),)
        else:
            bounds, kk = coefficients(in_size, out_size, resample)
            table = fixed_point(kk) if kind == "u8" else np.array(kk)
            hit = (torch.from_numpy(np.array(bounds)).to(device), torch.from_numpy(np.ascontiguousarray(table)).to(device), kk.shape[1])
        _device[key] = hit
    return hit


def _pil_mode_array(a):
    """numpy picture -> the PIL image(s) whose resize is the rule for it: L, RGB, F, or one L plane per channel."""
    from PIL import Image
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] not in (3,):
        return [Image.fromarray(np.ascontiguousarray(a[:, :, c])) for c in range(a.shape[2])], True
    return [Image.fromarray(a)], False


def _resize_pil(x, size, resample, device=None):
    """PIL itself on the host, then an upload: uint8 [H,W] / [H,W,C] / [B,H,W,C] (channels are independent: C other than 3 goes plane
    by plane, so no alpha is premultiplied), float32 [H,W] / [B,H,W], and whatever dtype PIL's fromarray takes as [H,W]."""
    global last_path
    last_path = "pil"
    device = x.device if device is None else torch.device(device)
    a = x.detach().cpu().numpy()
    batched = (a.dtype == np.uint8 and a.ndim == 4) or (a.dtype != np.uint8 and a.ndim == 3)
    outs = []
    for one in (a if batched else [a]):
        images, planes = _pil_mode_array(np.ascontiguousarray(one))
        got = [np.array(im.resize(tuple(size), resample)) for im in images]
        outs.append(np.stack(got, 2) if planes else got[0])
    out = np.stack(outs) if batched else outs[0]
    return torch.from_numpy(np.ascontiguousarray(out)).to(device)


def _check_args(x, size, resample):
    if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
        raise ValueError(f"resize: size={size!r} (need (W, H), both positive)")
    if resample not in (NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING):
        raise ValueError(f"resize: unknown filter {resample!r} (have NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING)")
    if x.dtype == torch.uint8:
        if x.dim() not in (2, 3, 4):
            raise ValueError(f"resize: a uint8 picture is [H,W], [H,W,C] or [B,H,W,C] (got {tuple(x.shape)})")
        C = 1 if x.dim() == 2 else x.shape[-1]
        if not 1 <= C <= 4:
            raise ValueError(f"resize: C={C} channels (need 1 .. 4)")
    elif x.dtype == torch.float32:
        if x.dim() not in (2, 3):
            raise ValueError(f"resize: a float32 picture is [H,W] or [B,H,W] (got {tuple(x.shape)})")
    elif x.dim() != 2:
        raise ValueError(f"resize: dtype {x.dtype} has no rule here beyond PIL's own for [H,W] (uint8 and float32 are resized on the device)")
    if x.numel() == 0:
        raise ValueError(f"resize: an empty picture {tuple(x.shape)}")


def _as4(x):
    """-> a [n, H, W, C] view of the picture with adjacent channels and pixels (a copy only where the layout asks for one)."""
    if x.dtype == torch.uint8:
        v = x[None, :, :, None] if x.dim() == 2 else (x[None] if x.dim() == 3 else x)
    else:
        v = x[None, :, :, None] if x.dim() == 2 else x[:, :, :, None]
    n, H, W, C = v.shape
    ok = (C == 1 or v.stride(3) == 1) and (W == 1 or v.stride(2) == C) and (H == 1 or v.stride(1) >= W * C) and \
         (n == 1 or v.stride(0) >= (H - 1) * max(v.stride(1), 0) + W * C)
    return v, ok


def _strides(v):
    n, H, W, C = v.shape
    row = v.stride(1) if H > 1 else W * C
    image = v.stride(0) if n > 1 else H * row
    return image, row


def _run(x4, size, resample, out4, epilogue):
    """The launches: x4 [n,H,W,C] -> out4 ([n,H',W',C] of x4's dtype, or float32 [n,C,H',W'] with a loader's epilogue).  -> launches."""
    n, H, W, C = x4.shape
    Wo, Ho = size
    device = x4.device
    f32 = x4.dtype == torch.float32
    src_image, src_row = _strides(x4)
    if epilogue == _native.RESIZE_U8:
        out_image, out_row = _strides(out4)
    else:
        out_image, out_row = C * Ho * Wo, Wo
    if max(n, H, W, Ho, Wo) > _MAX_SIDE:
        raise ValueError(f"resize: n, H, W and the output sizes are at most {_MAX_SIDE} on the device path (got {n} x {H} x {W} -> {Ho} x {Wo})")
    if resample == NEAREST or (H, W) == (Ho, Wo):
        yidx = None if H == Ho else _device_tables(device, "nearest", H, Ho, NEAREST)[0]
        xidx = None if W == Wo else _device_tables(device, "nearest", W, Wo, NEAREST)[0]
        if f32:
            _native.run("gsr_resize_nearest_f32", device, x4, src_image, src_row, n, H, W, Ho, Wo, yidx, xidx,
                        out4, out_image, out_row)
        else:
            _native.run("gsr_resize_nearest_u8", device, x4, src_image, src_row, n, H, W, C, Ho, Wo, yidx, xidx,
                        out4, out_image, out_row, epilogue)
        return 1
    kind = "f32" if f32 else "u8"
    launches = 0
    src, cur_W = x4, W
    if W != Wo:
        bounds, table, ksize = _device_tables(device, kind, W, Wo, resample)
        last = H == Ho
        if last:
            dst, dst_image, dst_row, ep = out4, out_image, out_row, epilogue
        else:  # the intermediate, rounded to the picture's own type
            dst = torch.empty((n, H, Wo, C), dtype=x4.dtype, device=device)
            dst_image, dst_row, ep = H * Wo * C, Wo * C, _native.RESIZE_U8
        if f32:
            _native.run("gsr_resize_f32", device, src, src_image, src_row, n, H, W, _native.RESIZE_HORIZONTAL, Wo, bounds,
                        table, ksize, dst, dst_image, dst_row)
        else:
            _native.run("gsr_resize_u8", device, src, src_image, src_row, n, H, W, C, _native.RESIZE_HORIZONTAL, Wo, bounds,
                        table, ksize, dst, dst_image, dst_row, ep)
        launches += 1
        src, src_image, src_row, cur_W = dst, dst_image, dst_row, Wo
    if H != Ho:
        bounds, table, ksize = _device_tables(device, kind, H, Ho, resample)
        if f32:
            _native.run("gsr_resize_f32", device, src, src_image, src_row, n, H, cur_W, _native.RESIZE_VERTICAL, Ho, bounds,
                        table, ksize, out4, out_image, out_row)
        else:
            _native.run("gsr_resize_u8", device, src, src_image, src_row, n, H, cur_W, C, _native.RESIZE_VERTICAL, Ho, bounds,
                        table, ksize, out4, out_image, out_row, epilogue)
        launches += 1
    return launches


def _on_device(x, resample):
    return x.is_cuda and not force_host and resample != HAMMING and x.dtype in (torch.uint8, torch.float32)


def resize(x, size, resample=BICUBIC, out=None):
    """Image.resize(size, resample) of PIL.  x: uint8 [H,W], [H,W,C] or [B,H,W,C] (C = 1 .. 4, channels independent) or float32 [H,W]
    or [B,H,W]; size = (W, H) as in PIL -> the same rank and dtype.  The row stride is free (a column slice of a wider tensor is read in
    place); `out` may be such a view as well.  On a HIP device: at most two launches on torch's current stream, no host stop.  Equal
    sizes give a copy."""
    global last_path, last_launches
    _check_args(x, size, resample)
    size = (int(size[0]), int(size[1]))
    if not _on_device(x, resample):
        got = _resize_pil(x, size, resample)
        if out is not None:
            out.copy_(got)
            return out
        return got
    x4, ok = _as4(x)
    if not ok:
        x4, _ = _as4(x.contiguous())
    n, H, W, C = x4.shape
    shape4 = (n, size[1], size[0], C)
    lead = x.shape[:-3] if x.dtype == torch.uint8 and x.dim() >= 3 else (x.shape[:-2] if x.dtype == torch.float32 else ())
    tail = (C,) if x.dtype == torch.uint8 and x.dim() >= 3 else ()
    final = tuple(lead) + (size[1], size[0]) + tail
    if out is None:
        out = torch.empty(final, dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != final or out.dtype != x.dtype or out.device != x.device:
        raise ValueError(f"resize: out is {tuple(out.shape)} {out.dtype} on {out.device}, the result is {final} {x.dtype} on {x.device}")
    out4, ok = _as4(out)
    if not ok or tuple(out4.shape) != shape4:
        raise ValueError("resize: out needs adjacent channels and pixels (rows and pictures may be strided)")
    last_path = "hip"
    last_launches = _run(x4, size, resample, out4, _native.RESIZE_U8)
    return out


def to_float_chw(x, size, resample, epilogue):
    """The loaders' form: uint8 [H,W] / [H,W,C] -> float32 [C,H',W'] = resize, then `/ 255.0` (RESIZE_DIV255) or `> 0` (RESIZE_GT0) and
    the permute, the last step fused into the last launch; equal sizes run the epilogue alone."""
    global last_path, last_launches
    _check_args(x, size, resample)
    if x.dtype != torch.uint8 or x.dim() > 3 or not _on_device(x, resample):
        raise ValueError("resize: the fused loaders take uint8 [H,W] or [H,W,C] on a HIP device")
    size = (int(size[0]), int(size[1]))
    x4, ok = _as4(x)
    if not ok:
        x4, _ = _as4(x.contiguous())
    C = x4.shape[3]
    out = torch.empty((C, size[1], size[0]), dtype=torch.float32, device=x.device)
    last_path = "hip"
    last_launches = _run(x4, size, resample, out, epilogue)
    return out


def pil_route(mode, resample):
    """PIL's mode rules -> ("hip" or "host", the filter PIL uses).  resample=None is BICUBIC; modes 1 and P force NEAREST; LA / RGBA
    premultiply alpha around the resample; only L, RGB and F have their rule on the device."""
    if resample is None:
        resample = BICUBIC
    if mode in ("1", "P"):
        return "host", NEAREST
    if mode not in ("L", "RGB", "F") or resample == HAMMING:
        return "host", resample
    return "hip", resample


def resize_pil_image(image, size, resample=None, device="cuda"):
    """image.resize(size, resample) for a PIL.Image, on the device: its bytes are uploaded once and resized there.  -> uint8 [H,W] (L),
    [H,W,3] (RGB) or float32 [H,W] (F); the other modes are resized by PIL on the host and uploaded as np.array gives them."""
    global last_path
    device = torch.device(device)
    route, resample = pil_route(image.mode, resample)
    if route == "host" or device.type != "cuda" or force_host:
        last_path = "pil"
        a = np.array(image.resize(tuple(size), resample))
        if a.dtype == np.bool_:
            a = a.astype(np.uint8) * 255
        return torch.from_numpy(a).to(device)
    return resize(torch.from_numpy(np.array(image)).to(device), size, resample)
