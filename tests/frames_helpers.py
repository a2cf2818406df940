"""The numpy oracle of gscream_amd.frames and the inputs its tests share.

The oracle states the rules of include/gsraster.h ("Output frames") in numpy: every per-pixel value is an fp32 array operation (one
rounding each, numpy never contracts), the least-squares sums are exactly rounded (`math.fsum` over the fp64 terms), the quotients are
fp64.  Panels are described as dicts {mode, src [B,C,H,w], src2, lut, flip}; `compose_oracle` lays them side by side."""
import math

import numpy as np

F = np.float32
QUANT, QUANT_CLAMP, ABSDIFF, NORMAL, CMAP_CV, CMAP_MPL_ALIGNED, CMAP_MPL = range(7)
U64 = 2.0 ** -53  # the unit roundoff of fp64


# ---- the rules ----
def clamp01(x):
    x = np.asarray(x, F)
    return np.where(x < 0, F(0), np.where(x > 1, F(1), x)).astype(F)  # comparisons: a NaN stays


def byte(v):
    """trunc(min(max(v, 0), 255)), NaN -> 0."""
    v = np.asarray(v, F)
    v = np.where(v < 0, F(0), np.where(v > 255, F(255), v))
    return np.where(np.isnan(v), F(0), v).astype(np.uint8)  # (astype truncates)


def quantise(x, clamp=False):
    x = np.asarray(x, F)
    if clamp:
        x = clamp01(x)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x * F(255)).astype(F)
        v = (v + F(0.5)).astype(F)
    return byte(v)


def absdiff(a, b):
    with np.errstate(invalid="ignore"):
        return quantise(np.abs((clamp01(a) - np.asarray(b, F)).astype(F)))


def normal_picture(n):
    """n [..., 3, H, w] raw normals -> uint8, same shape."""
    n = np.asarray(n, F)
    x, y, z = n[..., 0:1, :, :], n[..., 1:2, :, :], n[..., 2:3, :, :]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = (x * x).astype(F)
        s = (s + (y * y).astype(F)).astype(F)
        s = (s + (z * z).astype(F)).astype(F)
        r = np.sqrt(s).astype(F)
        r = np.where(r < F(1e-12), F(1e-12), r).astype(F)
        c = (n / r).astype(F)
        c = (c + F(1)).astype(F)
        c = (c / F(2)).astype(F)
    return quantise(c)


def aligned(d, scale, shift):
    with np.errstate(invalid="ignore", over="ignore"):
        a = (np.asarray(d, F) * F(scale)).astype(F)
        return (a + F(shift)).astype(F)


def extrema(x):
    """(min, max) as fp32, both NaN if anything is."""
    x = np.asarray(x, F)
    return (F(np.nan), F(np.nan)) if np.isnan(x).any() else (x.min(), x.max())


def lsq_terms(d, y, m):
    """The fp64 terms of the five sums, as the rule forms them: m d and m y exact, m d d and m d y rounded once."""
    d, y, m = (np.asarray(v, F).astype(np.float64).ravel() for v in (d, y, m))
    md = m * d
    return [md * d, md, m, md * y, m * y]


def solve(a00, a01, a11, b0, b1):
    """-> (det, x0, x1) in fp64, one rounding per operation."""
    det = a00 * a11 - a01 * a01
    if det == 0:
        return det, 0.0, 0.0
    return det, (a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det


def frame_params(d, y=None, m=None):
    """One frame -> dict: params [8] fp32 as gsr_frame_stats defines it, sums [5] exactly rounded, sum_bound [5] (what any order of n fp64
    additions can be off by: n u sum|t|), det, x0, x1 (fp64, from the exact sums)."""
    d = np.asarray(d, F)
    lo, hi = extrema(d)
    out = {"params": np.array([lo, hi, 0, 0, 0, 0, 0, 0], F), "sums": np.zeros(5), "sum_bound": np.zeros(5), "det": 0.0, "x0": 0.0, "x1": 0.0}
    if y is None:
        return out
    m = np.ones_like(d) if m is None else m
    terms = lsq_terms(d, y, m)
    sums = [math.fsum(t) if np.isfinite(t).all() else float(np.sum(t)) for t in terms]
    det, x0, x1 = solve(*sums)
    scale, shift = np.abs(F(x0)), F(x1)
    lo2, hi2 = extrema(np.concatenate([aligned(d, scale, shift).ravel(), np.asarray(y, F).ravel()]))
    out.update(params=np.array([lo, hi, scale, shift, lo2, hi2, 0, 0], F), sums=np.array(sums),
               sum_bound=np.array([t.size * U64 * math.fsum(np.abs(t)) if np.isfinite(t).all() else np.nan for t in terms]), det=det, x0=x0, x1=x1)
    return out


def lut_rgba(lut, i):
    rgb = np.asarray(lut, np.uint8)[i]
    return np.concatenate([rgb, np.full(rgb.shape[:-1] + (1,), 255, np.uint8)], -1)


def cmap_cv(d, lo, hi, lut):
    """d [H, w] -> uint8 [H, w, 4]."""
    d, lo, hi = np.asarray(d, F), F(lo), F(hi)
    i = np.zeros(d.shape, np.int64)
    if hi != lo and np.isfinite(lo) and np.isfinite(hi):
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            t = ((d - lo).astype(F) / F(hi - lo)).astype(F)
            i = byte((F(255) * t).astype(F)).astype(np.int64)
    return lut_rgba(lut, i)


def cmap_mpl(v, lo2, hi2, lut):
    """v [H, w] -> uint8 [H, w, 4]: plt.imsave's bytes for a panel whose extrema are lo2, hi2."""
    v, lo, hi = np.asarray(v, F), F(lo2), F(hi2)
    if np.isnan(lo) or np.isnan(hi):
        return np.zeros(v.shape + (4,), np.uint8)
    if hi == lo:
        return lut_rgba(lut, np.zeros(v.shape, np.int64))
    den = F(np.float64(hi) - np.float64(lo))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = ((v - lo).astype(F) / den).astype(F)
        t = (t * F(256)).astype(F)
    blank = np.isnan(t)
    i = np.where(blank, F(0), np.where(t < 0, F(0), np.where(t > 255, F(255), t))).astype(np.int64)  # (astype truncates)
    out = lut_rgba(lut, i)
    out[blank] = 0
    return out


def panel_oracle(p, params):
    """One panel dict -> uint8 [B, H, w, 4]."""
    s = np.asarray(p["src"], F)
    mode = p["mode"]
    if mode in (QUANT, QUANT_CLAMP):
        rgb = quantise(s, mode == QUANT_CLAMP)
    elif mode == ABSDIFF:
        rgb = absdiff(s, p["src2"])
    elif mode == NORMAL:
        rgb = normal_picture(s)
    else:
        rows = []
        for b in range(s.shape[0]):
            q = params[b]
            if mode == CMAP_CV:
                rows.append(cmap_cv(s[b, 0], q[0], q[1], p["lut"]))
            else:
                rows.append(cmap_mpl(aligned(s[b, 0], q[2], q[3]) if mode == CMAP_MPL_ALIGNED else s[b, 0], q[4], q[5], p["lut"]))
        out = np.stack(rows)
        return out[:, :, ::-1] if p.get("flip") else out
    rgb = np.broadcast_to(rgb, (s.shape[0], 3) + s.shape[2:]).transpose(0, 2, 3, 1)
    out = np.concatenate([rgb, np.full(rgb.shape[:-1] + (1,), 255, np.uint8)], -1)
    return out[:, :, ::-1] if p.get("flip") else out


def compose_oracle(panels, params=None, channels=3):
    """Panel dicts laid side by side in order -> uint8 [B, H, W_out, channels]."""
    return np.ascontiguousarray(np.concatenate([panel_oracle(p, params) for p in panels], 2)[..., :channels])


# ---- inputs ----
def view_inputs(H, W, seed):
    """One view's tensors, as render_set holds them: render [3,H,W] and uncertainty [1,H,W] reaching outside [0, 1], gt [3,H,W], a
    smooth depth [1,H,W] with noise, a MiDaS-like target (an affine image of the depth, with noise), an object mask [1,H,W] of 0 / 1, raw
    normals [H*W, 3] of every length (some exactly zero)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = 2.5 + 0.03 * j - 0.02 * i + 0.4 * np.sin(0.31 * i + 0.2) * np.cos(0.23 * j) + 0.05 * rng.standard_normal((H, W))
    midas = 0.37 * depth + 0.8 + 0.04 * rng.standard_normal((H, W))
    mask = (rng.random((H, W)) < 0.3).astype(F)
    normals = rng.standard_normal((H * W, 3)) * np.exp(rng.uniform(-3, 3, (H * W, 1)))
    normals[rng.random(H * W) < 0.05] = 0.0
    return {"render": (rng.random((3, H, W)) * 1.4 - 0.2).astype(F), "uncertainty": (rng.random((1, H, W)) * 1.4 - 0.2).astype(F),
            "gt": rng.random((3, H, W)).astype(F), "depth": depth.astype(F)[None], "midas": midas.astype(F)[None], "mask": mask[None],
            "normals": normals.astype(F)}


def rgbd_oracle(v, params, lut, flip=True):
    """rgbd_frame's picture [H, 4W, 3] from view_inputs and params [1, 8]."""
    _, H, W = v["render"].shape
    raw = v["normals"].reshape(1, H, W, 3).transpose(0, 3, 1, 2)
    return compose_oracle([{"mode": QUANT_CLAMP, "src": v["render"][None], "flip": flip},
                           {"mode": CMAP_CV, "src": v["depth"][None], "lut": lut, "flip": flip},
                           {"mode": NORMAL, "src": raw, "flip": flip},
                           {"mode": QUANT_CLAMP, "src": v["uncertainty"][None], "flip": flip}], params)[0]


def view_oracle(v, params, lut):
    """view_frames' (sheet [H, 4W, 3], depth picture [H, 2W, 4]) from view_inputs and params [1, 8]."""
    sheet = compose_oracle([{"mode": QUANT_CLAMP, "src": v["render"][None]}, {"mode": QUANT_CLAMP, "src": v["uncertainty"][None]},
                            {"mode": ABSDIFF, "src": v["render"][None], "src2": v["gt"][None]}, {"mode": QUANT, "src": v["gt"][None]}])[0]
    picture = compose_oracle([{"mode": CMAP_MPL_ALIGNED, "src": v["depth"][None], "lut": lut},
                              {"mode": CMAP_MPL, "src": v["midas"][None], "lut": lut}], params, 4)[0]
    return sheet, picture


def within_one_ulp(got, want64):
    """fp32 `got` against an fp64 value: no further than one fp32 ulp from it."""
    got, want64 = np.asarray(got, F), np.asarray(want64, np.float64)
    w = want64.astype(F)
    return np.abs(got.astype(np.float64) - want64) <= np.spacing(np.abs(w)).astype(np.float64)
