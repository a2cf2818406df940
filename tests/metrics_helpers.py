"""The shared yardstick of test_metrics.py / test_gpu_metrics.py (and of tests/golden/make_reference_vectors8.py): an fp64 numpy
statement of the rules of gsr_image_metrics (include/gsraster.h), the bound on the kernel's fp64 sums, and seeded image pairs.

The oracle.  The input transform and d = x - y are numpy fp32 operations (one rounding each); everything after is fp64.  The five
window sums are scipy.ndimage.correlate with the 5x5 kernel w_ij = g_i g_j and mode='mirror' (reflect without repeating the edge);
`loop=True` evaluates them by an explicit per-pixel loop with the index rule written out, for the smallest case.  The per-image sums
are math.fsum (exact, rounded once), so the oracle's own summation adds one rounding.

The bound on a sum, with u = 2^-53.  n, n_m are exact.  |d| and d^2 are exact per element (fp32 difference widened; its square is
exact in fp64), dssim is not: per pixel, with a_i = w*|x_i| >= |mu_i| and b_ij = w*|x_i x_j| >= |e_ij| (the magnitudes the roundings
of a window sum are relative to; for non-negative images a_i = mu_i),
    |d mu_i|        <= T u a_i,  |d e_ij| <= T u b_ij     T = 40: the kernel's 5 + 5 fused taps, the oracle's 25 products + 25 additions
                                                           with w_ij itself rounded, against each other (10 + 27, rounded up)
    |d(mu_i mu_j)|  <= (2 T + 2) u a_i a_j
    |d s_ij|        <= t_ij = (T + 2) u b_ij + (2 T + 4) u a_i a_j                       (s = e - mu mu: this is what 1/C2 amplifies)
    |d N1| <= (4 T + 4) u a_1 a_2 + 4 u D1',  |d D1| <= (2 T + 6) u D1'                 D1' = a_1^2 + a_2^2 + C1
    |d N2| <= 2 t_12 + 4 u |N2|,              |d D2| <= t_11 + t_22 + 4 u D2
    |d ssim| <= (|N2| dN1 + |N1| dN2 + 2 u |N1 N2| + |ssim| (D2 dD1 + D1 dD2 + 4 u D1 D2)) / (D1 D2) + 2 u |ssim|
    |d dssim| <= |d ssim| / 2 + 2 u                                                      (the clamp does not expand)
(first order; the bound takes 1.01 times the total for the second-order terms).  The sum of these over the selected pixels, plus the
summation itself: an element of the kernel's sum passes through at most L = 2 + 6 + 3 + ceil(C tiles / 256) + 6 + 3 additions (a
thread's two pixels, the wave butterfly, the four waves; a finish thread's share, its butterfly, its waves), the oracle's fsum
through one: (L + 1) u sum|v|.  On 3 x 37 x 53 uniform noise this bound is 1.8e-10 on a dssim sum of 2.9e3; two fp64 statements (torch
and scipy) were seen 3e-13 apart per map pixel, which gives the scale and is not the bound."""
import math

import numpy as np
from scipy import ndimage

U64 = 2.0 ** -53
C1, C2, EPS = 1e-4, 9e-4, 1e-12
TILE_H, TILE_W = 16, 32   # metrics.hip's MET_TH x MET_TW
T_TAPS = 40.0


def taps():
    g = np.exp(-(np.arange(5, dtype=np.float64) - 2.0) ** 2 / 4.5)
    return g / g.sum()


def transform(x, clamp=False, quantize=False):
    """The input transform in numpy fp32: one rounding per operation, comparisons that keep a NaN."""
    x = np.asarray(x, np.float32)
    one, zero = np.float32(1), np.float32(0)
    with np.errstate(invalid="ignore"):
        if clamp:
            x = np.where(x < zero, zero, np.where(x > one, one, x)).astype(np.float32)
        if quantize:
            q = x * np.float32(255)
            q = q + np.float32(0.5)
            q = np.where(q < zero, zero, np.where(q > np.float32(255), np.float32(255), q)).astype(np.float32)
            x = (np.trunc(q) / np.float32(255)).astype(np.float32)
    return x


def mirror(i, n):
    """The padding rule written out: -1 -> 1, -2 -> 2, n -> n-2, n+1 -> n-3."""
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    return i


def _filter(plane, w2, mode, loop):
    if not loop:
        return ndimage.correlate(plane, w2, mode=mode, cval=0.0)
    assert mode == "mirror"
    h, w = plane.shape
    out = np.zeros_like(plane)
    for i in range(h):
        for j in range(w):
            s = 0.0
            for a in range(5):
                for b in range(5):
                    s += w2[a, b] * plane[mirror(i + a - 2, h), mirror(j + b - 2, w)]
            out[i, j] = s
    return out


def dssim_map(x, y, mode="mirror", loop=False, with_bound=False):
    """x, y [..., H, W] fp32 (already transformed) -> the dssim map in fp64 (and the per-pixel bound of the module text)."""
    x64, y64 = np.asarray(x, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    g = taps()
    w2 = np.outer(g, g)
    out, bound = np.empty_like(x64), np.empty_like(x64)
    with np.errstate(invalid="ignore", over="ignore"):
        for idx in np.ndindex(x64.shape[:-2]):
            p, q = x64[idx], y64[idx]
            f = lambda t: _filter(t, w2, mode, loop)  # noqa: E731
            mu1, mu2, e11, e22, e12 = f(p), f(q), f(p * p), f(q * q), f(p * q)
            s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
            N1, N2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
            D1, D2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
            ssim = (N1 * N2) / (D1 * D2 + EPS)
            ds = (1 - ssim) / 2
            out[idx] = np.where(ds < 0, 0.0, np.where(ds > 1, 1.0, ds))
            if with_bound:
                a1, a2 = f(np.abs(p)), f(np.abs(q))
                b11, b22, b12 = e11, e22, f(np.abs(p * q))
                T, u = T_TAPS, U64
                t = lambda b, aa: (T + 2) * u * b + (2 * T + 4) * u * aa  # noqa: E731
                t11, t22, t12 = t(b11, a1 * a1), t(b22, a2 * a2), t(b12, a1 * a2)
                D1p = a1 * a1 + a2 * a2 + C1
                dN1, dD1 = (4 * T + 4) * u * a1 * a2 + 4 * u * D1p, (2 * T + 6) * u * D1p
                dN2, dD2 = 2 * t12 + 4 * u * np.abs(N2), t11 + t22 + 4 * u * np.abs(D2)
                D2a = np.abs(D2)
                dss = ((np.abs(N2) * dN1 + np.abs(N1) * dN2 + 2 * u * np.abs(N1 * N2)
                        + np.abs(ssim) * (D2a * dD1 + D1 * dD2 + 4 * u * D1 * D2a)) / (D1 * D2a) + 2 * u * np.abs(ssim))
                bound[idx] = 1.01 * (dss / 2 + 2 * u)
    return (out, bound) if with_bound else out


def _fsum(v):
    v = np.asarray(v, np.float64).ravel()
    if not np.isfinite(v).all():
        return float(np.sum(v))  # NaN / inf: IEEE semantics decide
    return math.fsum(v.tolist())


def kernel_additions(C, H, W):
    tiles = -(-H // TILE_H) * -(-W // TILE_W)
    return 2 + 6 + 3 + -(-C * tiles // 256) + 6 + 3


def metrics_oracle(pred, gt, mask=None, clamp=False, quantize=False, mode="mirror", loop=False, with_bound=False):
    """pred, gt [B,C,H,W] fp32, mask None or bool broadcastable to them -> {"sums" [B,8] fp64, "metrics" [B,8] fp64 (not yet rounded
    to fp32), "dssim" the map, and with_bound: "sum_bound" [B,8]}."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    assert pred.ndim == 4 and pred.shape == gt.shape
    B, C, H, W = pred.shape
    x, y = transform(pred, clamp, quantize), transform(gt, clamp, quantize)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x - y).astype(np.float32).astype(np.float64)
    ad, dd = np.abs(d), d * d
    r = dssim_map(x, y, mode, loop, with_bound)
    ds, pix = r if with_bound else (r, None)
    m = np.ones(pred.shape, bool) if mask is None else np.broadcast_to(np.asarray(mask, bool), pred.shape)
    sums, bound = np.zeros((B, 8)), np.zeros((B, 8))
    L = kernel_additions(C, H, W)
    for b in range(B):
        for h, sel in ((0, np.ones((C, H, W), bool)), (4, m[b])):
            sums[b, h] = float(sel.sum())
            for k, v in ((1, ad[b]), (2, dd[b]), (3, ds[b])):
                sums[b, h + k] = _fsum(v[sel])
                if with_bound:
                    bound[b, h + k] = (L + 1) * U64 * float(np.sum(np.abs(v[sel]))) + (float(np.sum(pix[b][sel])) if k == 3 else 0.0)
    out = np.zeros((B, 8))
    with np.errstate(invalid="ignore", divide="ignore"):
        for h in (0, 4):
            n = sums[:, h]
            out[:, h] = sums[:, h + 1] / n
            out[:, h + 1] = sums[:, h + 2] / n
            out[:, h + 2] = -10.0 * np.log10(out[:, h + 1])
            out[:, h + 3] = 1.0 - 2.0 * (sums[:, h + 3] / n)
    res = {"sums": sums, "metrics": out, "dssim": ds}
    if with_bound:
        res["sum_bound"] = bound
    return res


def within_one_ulp(got32, want64):
    """got (fp32) is the fp64 value rounded to fp32, or one of its two fp32 neighbours; NaN matches NaN, an infinity itself."""
    got = np.asarray(got32, np.float32)
    with np.errstate(over="ignore"):
        want = np.asarray(want64, np.float64).astype(np.float32)
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    with np.errstate(invalid="ignore"):
        ok = (got == want) | (got == lo) | (got == hi)
    return ok | (np.isnan(got) & np.isnan(want))


def smooth_pair(h, w, c=3, b=1, seed=0, noise=0.02):
    """A smooth image in [0, 1] and a noisy copy of it (PSNR ~ 34 dB at noise 0.02), fp32 [b,c,h,w]."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    planes = [0.5 + 0.35 * np.sin(0.11 * i + 0.07 * j + 0.9 * k) * np.cos(0.05 * i - 0.13 * j + 0.4 * k) for k in range(b * c)]
    gt = np.stack(planes).reshape(b, c, h, w)
    pred = gt + noise * rng.standard_normal(gt.shape)
    return pred.astype(np.float32), gt.astype(np.float32)


def noise_pair(h, w, c=3, b=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((b, c, h, w), dtype=np.float32), rng.random((b, c, h, w), dtype=np.float32)


def random_mask(shape, seed=0, share=0.4):
    return np.random.default_rng(1000 + seed).random(shape) < share


# name: (H, W, C, B, kind, seed).  The sizes are the smallest at which each part of the kernel can go wrong: every tap reflected, one
# dimension all halo, more than one tile both ways and no multiple of the tile, one past the tile, one short of one and of two tiles.
CASES = {
    "3x3": (3, 3, 3, 1, "noise", 0),
    "3x70": (3, 70, 1, 1, "smooth", 1),
    "70x3": (70, 3, 1, 3, "noise", 2),
    "37x53": (37, 53, 3, 1, "noise", 0),
    "past_the_tile": (TILE_H + 1, TILE_W + 1, 3, 3, "smooth", 3),
    "short_of_the_tile": (2 * TILE_H - 1, TILE_W - 1, 1, 1, "smooth", 4),
}
_cache = {}


def case(name):
    """(pred, gt, mask [B,1,H,W]) of a case and its oracle runs without and with the mask (computed once, shared, never written to)."""
    if name not in _cache:
        h, w, c, b, kind, seed = CASES[name]
        pred, gt = (noise_pair if kind == "noise" else smooth_pair)(h, w, c=c, b=b, seed=seed)
        mask = random_mask((b, 1, h, w), seed)
        mask[:, 0, 0, 0], mask[:, 0, -1, -1] = True, False
        d = {"pred": pred, "gt": gt, "mask": mask, "plain": metrics_oracle(pred, gt, with_bound=True),
             "masked": metrics_oracle(pred, gt, mask, with_bound=True)}
        for v in (pred, gt, mask):
            v.setflags(write=False)
        _cache[name] = d
    return _cache[name]
