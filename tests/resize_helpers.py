"""PIL's Image.resize restated in numpy, one scalar loop per rule, and the case list of the resize tests.

The statement is held against PIL itself (tests/test_resize.py: bytes for 8-bit pictures, bits for mode F), so that what the device
path is compared with in tests/test_gpu_resize.py -- PIL, called in the test -- and what gscream_amd.resize's tables are compared with
on the host -- this file -- are the same rule.

Tables (all double): scale = inS / outS, fs = max(scale, 1), support = s * fs, ksize = ceil(support) * 2 + 1; per output index xx:
c = (xx + 0.5) * scale, xmin = max(int(c - support + 0.5), 0), n = min(int(c + support + 0.5), inS) - xmin,
w[x] = f((x + xmin - c + 0.5) * (1 / fs)), ww = the sum of w in index order, k[x] = w[x] / ww where ww != 0.
8-bit: K = trunc(k * 2^22 +- 0.5), acc = 2^21 + sum src * K in int32, out = clamp(acc >> 22, 0, 255).  Mode F: a sequential fp64 sum of
double(src) * k over every tap of the bound, rounded to float32.  The horizontal pass runs first, its result rounded to the picture's
own type.  NEAREST: per axis an accumulated xo = 0.5 a, xo += a with a = inS / outS, index int(xo)."""
import math

import numpy as np

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5
FILTERS = (BOX, BILINEAR, BICUBIC, LANCZOS)
NAMES = {NEAREST: "nearest", LANCZOS: "lanczos", BILINEAR: "bilinear", BICUBIC: "bicubic", BOX: "box"}
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
PRECISION_BITS = 22

#: ((H, W) -> (H, W)): the smallest shapes at which a pass can go wrong
CASES = (
    ((37, 53), (9, 13)),      # non-integer downscale, widths off the wave size
    ((129, 200), (33, 47)),   # the same over more than one tile of outputs and more than one block of rows
    ((23, 31), (57, 70)),     # upscale: fs = 1, bounds clipped at both edges
    ((64, 48), (64, 12)),     # the horizontal pass only
    ((30, 30), (7, 30)),      # the vertical pass only
    ((20, 20), (20, 20)),     # a copy
    ((5, 7), (1, 1)),         # one output, every input a tap
    ((1, 1), (4, 5)),         # one input, one tap per output
    ((3, 200), (3, 7)),       # LANCZOS: 173 taps, the path past the LDS tile
    ((16, 300), (16, 299)),   # scale just above 1: the bounds slide by one somewhere in the row
    ((3, 1300), (3, 130)),    # a tile's source segment past the LDS tile (700 pixels: C = 4 and float32) with the coefficients inside it
    ((2, 2200), (2, 3)),      # segment and coefficients both past it, for every type (LANCZOS: 4401 taps)
)


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def filter_value(resample, x):
    if resample == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if resample == BILINEAR:
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if resample == BICUBIC:
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    if resample == LANCZOS:
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    raise ValueError(resample)


def tables(in_size, out_size, resample):
    """-> (bounds int32 [out, 2] = (xmin, n), coefficients float64 [out, ksize], zero behind n)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[resample] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.float64)
    for xx in range(out_size):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), in_size) - xmin
        w = [filter_value(resample, (x + xmin - c + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            kk[xx, x] = w[x] / ww if ww != 0.0 else w[x]
        bounds[xx] = (xmin, n)
    return bounds, kk


def fixed(kk):
    """The 8-bit tables: trunc(k * 2^22 +- 0.5), the sign of k."""
    out = np.zeros(kk.shape, np.int32)
    flat, src = out.reshape(-1), kk.reshape(-1)
    for i in range(src.size):
        v = float(src[i])
        flat[i] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return out


def pass_u8(a, axis, out_size, resample):
    """One pass over uint8 [H, W, C] along axis 0 or 1."""
    a = np.moveaxis(a, axis, 0)
    bounds, kk = tables(a.shape[0], out_size, resample)
    K = fixed(kk).astype(np.int64)
    out = np.zeros((out_size,) + a.shape[1:], np.uint8)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        acc = np.full(a.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(n):
            acc += a[xmin + x].astype(np.int64) * K[xx, x]
        assert np.abs(acc).max() < 2 ** 31  # (the int32 of the rule does not wrap)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def pass_f32(a, axis, out_size, resample):
    """One pass over float32 [H, W] along axis 0 or 1: the sequential fp64 chain, rounded to float32 at the end."""
    a = np.moveaxis(a, axis, 0)
    bounds, kk = tables(a.shape[0], out_size, resample)
    out = np.zeros((out_size,) + a.shape[1:], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for xx in range(out_size):
            xmin, n = bounds[xx]
            ss = np.zeros(a.shape[1:], np.float64)
            for x in range(n):
                ss = ss + a[xmin + x].astype(np.float64) * kk[xx, x]
            out[xx] = ss.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def nearest_table(in_size, out_size):
    a = in_size / out_size
    xo = a * 0.5
    idx = np.zeros(out_size, np.int32)
    for x in range(out_size):
        idx[x] = int(xo)
        xo += a
    return idx


def resize(a, size, resample):
    """a: uint8 [H, W] / [H, W, C] or float32 [H, W]; size = (W, H) as in PIL."""
    W, H = size
    if (a.shape[0], a.shape[1]) == (H, W):
        return a.copy()
    if resample == NEAREST:
        return np.ascontiguousarray(a[nearest_table(a.shape[0], H)][:, nearest_table(a.shape[1], W)])
    one = pass_u8 if a.dtype == np.uint8 else pass_f32
    flat = a.ndim == 2 and a.dtype == np.uint8
    if flat:
        a = a[:, :, None]
    if a.shape[1] != W:
        a = one(a, 1, W, resample)
    if a.shape[0] != H:
        a = one(a, 0, H, resample)
    return np.ascontiguousarray(a[:, :, 0] if flat else a)


def pil_resize(a, size, resample):
    """PIL itself on a numpy picture: uint8 [H, W] (L), [H, W, 3] (RGB), [H, W, 4] as four L planes (no premultiplication), float32 [H, W] (F)."""
    from PIL import Image
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] not in (1, 3):
        return np.stack([pil_resize(np.ascontiguousarray(a[:, :, c]), size, resample) for c in range(a.shape[2])], 2)
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 1:
        return pil_resize(np.ascontiguousarray(a[:, :, 0]), size, resample)[:, :, None]
    return np.array(Image.fromarray(a).resize(size, resample))


def picture_u8(H, W, C, seed, binary=False):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if binary:  # blobs of 0 and 255: ringing overshoots both ends of the clamp
        a = ((a[:, :, :1] > 127) * 255).astype(np.uint8).repeat(C, 2) if (H < 4 or W < 4) else \
            (np.kron(rng.integers(0, 2, ((H + 3) // 4, (W + 3) // 4, C), dtype=np.uint8), np.ones((4, 4, 1), np.uint8))[:H, :W] * 255)
    return np.ascontiguousarray(a)


def picture_f32(H, W, seed, special=False):
    rng = np.random.default_rng(seed)
    a = (rng.random((H, W), dtype=np.float32) * 2e4 - 1e4).astype(np.float32)
    if special:
        a[H // 2, W // 3] = np.inf
        a[H // 3, (2 * W) // 3] = np.nan
        a[0, 0] = -np.inf
    return a


def same_bits(a, b):
    """Equality of float32 pictures bit for bit, NaN positions compared as a mask (a NaN's payload is not part of the rule)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))
