"""The RGB loss' gate (tests/test_gpu_rgb_loss.py; proven without a GPU in tests/test_rgb_loss_gate.py): every REGION of a structured
frame is held to its own scale, and the bound of each comes from the error of the reference's own float32 arithmetic there.

Why not "1e-4 of the largest entry of the tensor" (tests/test_gpu_loss.py's rule, which stays for its white-noise inputs): on a frame
with flat, saturated and equal regions the gradients of those regions are 2-30 % of the tensor's maximum and may be wrong by tens of
percent inside that rule, while in a white == white region D = (E[x^2 + y^2] - mu1^2 - mu2^2) + C2 is rounding noise over C2 = 9e-4
and the reference's own eager float32 is off by almost 1e-4 of the maximum: a fixed share of the maximum is wrong in both directions.

    region_gate        per region k:   max|got - fp64| <= 4 * max(max|eager fp32 - fp64|, 2^-24 * max|fp64|)
    pooled_gate        small shapes, per window size: the same with both errors relative to each shape's largest entry, pooled over
                       the shapes (on tensors of a few elements eager lands on the oracle by chance)
    region_means_gate  the forward's region means (read through an indicator weight) against the largest per-pixel error of the
                       eager float32 map in the region

The factor 4 is tests/test_gpu_crossattn.py's for "a different but equally valid summation order": here two 11-tap passes against
one 121-tap conv2d.  `kernel_statement` restates gscream_amd/csrc/loss.hip's expression sequence in torch; it stands in for
the device in the CPU tests, and its `fault=` names are the structural mistakes the gate must catch.
No GPU import here."""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import loss_oracle as LO  # noqa: E402

EPS = 2.0 ** -24     # half an ulp of 1 in float32: the floor of every bound, times the reference's largest entry
FACTOR = 4.0         # tests/test_gpu_crossattn.py: a different but equally valid summation order
OLD_RULE = 1e-4      # tests/test_gpu_loss.py: of the largest gradient entry
UP = 1.5             # every case runs with a non-unit upstream gradient
LAM = 0.2
NAMES = ["textured", "black = black", "white = white", "two flats", "equal texture", "ramp", "near white"]
#: region -> (rows, columns) of the 64 x 96 frame; they straddle the 32 x 16 tile borders at x = 32, 64 and y = 16, 48
RECTS = {1: ((0, 24), (0, 30)), 2: ((0, 24), (34, 66)), 3: ((0, 24), (70, 96)),
         4: ((40, 64), (0, 30)), 5: ((40, 64), (34, 66)), 6: ((40, 64), (70, 96))}
MARGIN = 5           # the window's radius: how far a pixel's gradient looks
SMALL_SHAPES = [(1, 1, 1), (3, 1, 1), (1, 1, 40), (1, 40, 1), (3, 5, 5), (2, 10, 10), (3, 11, 11), (3, 15, 31), (3, 16, 32), (4, 17, 33),
                (3, 32, 64), (1, 6, 70)]
WINDOWS = [3, 5, 7, 9, 11]
FAULTS = ["sign0_is_plus", "clamp_to_edge", "dmu1_without_d_minus_cc", "planes_without_weight", "last_column_left_weight"]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def region_map(H=64, W=96):
    assert H >= 64 and W >= 96, "the rectangles are laid out for a frame of at least 64 x 96"
    region = np.zeros((H, W), np.int64)
    for k, ((r0, r1), (c0, c1)) in RECTS.items():
        region[r0:r1, c0:c1] = k
    return region


def structured_frame(seed, H=64, W=96, unclipped=False):
    """-> (img [3,H,W] float32, gt [3,H,W] float32, region [H,W] int): white noise (region 0; `unclipped` leaves the rendered side
    outside [0, 1] there, as the trainer's renderer does) with six rectangles: 1 both black, 2 both white, 3 two different flats,
    4 img == gt on texture (the L1 sign is 0), 5 a smooth ramp with a little noise, 6 gt white and img white minus 0, 1 or 2 steps
    of 2^-10 (a third of it equal)."""
    rng = np.random.default_rng(seed)
    region = region_map(H, W)
    gt = rng.random((3, H, W)).astype(np.float32)
    img = (gt + 0.2 * rng.standard_normal(gt.shape)).astype(np.float32)
    if not unclipped:
        img = np.clip(img, 0, 1).astype(np.float32)
    sel = lambda k: (slice(None), slice(*RECTS[k][0]), slice(*RECTS[k][1]))
    img[sel(1)] = 0.0
    gt[sel(1)] = 0.0
    img[sel(2)] = 1.0
    gt[sel(2)] = 1.0
    img[sel(3)] = 0.25
    gt[sel(3)] = 0.75
    img[sel(4)] = gt[sel(4)]
    (r0, r1), (c0, c1) = RECTS[5]
    ramp = np.linspace(0.1, 0.9, c1 - c0, dtype=np.float32)
    gt[sel(5)] = ramp[None, None, :]
    img[sel(5)] = (gt[sel(5)] + 0.02 * rng.standard_normal((3, r1 - r0, c1 - c0))).astype(np.float32)
    (r0, r1), (c0, c1) = RECTS[6]
    gt[sel(6)] = 1.0
    img[sel(6)] = (1.0 - rng.integers(0, 3, (3, r1 - r0, c1 - c0)) * 2.0 ** -10).astype(np.float32)
    return img, gt, region


def object_rectangle(seed, H=64, W=96):
    """(r0, r1, c0, c1) of the "object" weight's zero block: 28 x 38, moved by the seed; it cuts regions 1, 2, 4, 5 and the texture."""
    rng = np.random.default_rng(1000 + seed)
    r0, c0 = 12 + int(rng.integers(0, 5)), 18 + int(rng.integers(0, 5))
    return r0, r0 + 28, c0, c0 + 38


def block_interior(seed, H=64, W=96):
    """[H,W] bool: the pixels at least MARGIN px inside the zero block -- nothing they hold reaches a pixel of nonzero weight."""
    r0, r1, c0, c1 = object_rectangle(seed, H, W)
    inside = np.zeros((H, W), bool)
    inside[r0 + MARGIN:r1 - MARGIN, c0 + MARGIN:c1 - MARGIN] = True
    return inside


def weights(kind, seed, H, W):
    """-> [1,H,W] float32 or None.  "fractional": uniform in [0, 1) with about 5 % exact zeros (never all of them); "object": a binary
    mask with one zero rectangle of 28 x 38 -- what GScream's masked views pass -- placed so that no region lies wholly inside it."""
    if kind == "none":
        return None
    rng = np.random.default_rng(500 + seed)
    if kind == "fractional":
        w = (rng.random((1, H, W)) * (rng.random((1, H, W)) > 0.05)).astype(np.float32)
        if not w.any():
            w.reshape(-1)[0] = 0.5
        return w
    assert kind == "object", kind
    r0, r1, c0, c1 = object_rectangle(seed, H, W)
    assert r1 - r0 >= 20 and c1 - c0 >= 30 and r1 <= H and c1 <= W
    w = np.ones((1, H, W), np.float32)
    w[0, r0:r1, c0:c1] = 0.0
    region = region_map(H, W)
    for k in range(len(NAMES)):
        assert w[0][region == k].any(), ("region", k, "lies wholly inside the zero block")
    assert block_interior(seed, H, W).sum() >= 15 * 25
    return w


def small_case(seed, C, H, W):
    """White noise at a small shape with a fractional weight -> (img, gt, weight)."""
    rng = np.random.default_rng(seed * 100 + C * 1000 + H * 7 + W)
    gt = rng.random((C, H, W)).astype(np.float32)
    img = np.clip(gt + 0.2 * rng.standard_normal(gt.shape), 0, 1).astype(np.float32)
    return img, gt, weights("fractional", seed + H + W, H, W)


def _t(a):
    return torch.tensor(np.asarray(a))   # a copy: the tests share read-only arrays


# ---- objectives ----------------------------------------------------------------------------------------------------------------------
def objective(x, y, m, lam, window_size=11):
    """train.py:538-545 in torch, any dtype: (1 - lam) mean(|x - y| m) + lam (1 - mean(ssim_map(x, y) m)).  m: [1,H,W] or None."""
    ad, sm = torch.abs(x - y), LO.ssim_map(x, y, window_size)
    if m is not None:
        ad, sm = ad * m, sm * m
    return (1.0 - lam) * ad.mean() + lam * (1.0 - sm.mean())


def oracle(img, gt, w, lam=LAM, window_size=11, dtype=torch.float64, upstream=1.0):
    """The reference's arithmetic on the CPU in `dtype` (float64: the oracle; float32: "eager", the yardstick).
    -> (loss, d(upstream loss)/d img [C,H,W], ssim map [C,H,W], |img - gt| [C,H,W]), the arrays as float64 numpy, unweighted maps."""
    x = _t(img).to(dtype).clone().requires_grad_(True)
    y = _t(gt).to(dtype)
    m = None if w is None else _t(w).to(dtype).reshape(1, *x.shape[-2:])
    loss = objective(x, y, m, lam, window_size)
    (upstream * loss).backward()
    with torch.no_grad():
        sm, ad = LO.ssim_map(x, y, window_size), torch.abs(x - y)
    return float(loss.detach()), x.grad.double().numpy(), sm.double().numpy(), ad.double().numpy()


# ---- loss.hip restated ---------------------------------------------------------------------------------------------------------------
def taps(window_size):
    """gsl_make_taps: create_window's 1-D taps (float32 exp, float32 running sum, float32 division) centred in the 11-tap frame.
    Window 11 is a table in the source, GSL_G11, equal to torch's gaussian(11) (whose sum is not a running one; asserted in
    tests/test_rgb_loss_gate.py)."""
    assert 1 <= window_size <= 11 and window_size % 2 == 1
    if window_size == 11:
        return LO.gaussian(11).numpy().astype(np.float32)
    r = window_size // 2
    g = [np.float32(math.exp(-float((x - r) * (x - r)) / (2.0 * 1.5 * 1.5))) for x in range(window_size)]
    s = np.float32(0.0)
    for v in g:
        s = np.float32(s + v)
    t = np.zeros(11, np.float32)
    t[MARGIN - r:MARGIN - r + window_size] = np.array(g, np.float32) / s
    return t


def source_taps11():
    """GSL_G11 as gscream_amd/csrc/loss.hip spells it (the kernel's taps for window_size 11)."""
    import re
    with open(os.path.join(ROOT, "gscream_amd", "csrc", "loss.hip")) as f:
        body = re.search(r"GSL_G11\[11\]\s*=\s*\{([^}]*)\}", f.read()).group(1)
    return np.array([float.fromhex(v.strip().rstrip("f")) for v in body.split(",")], np.float32)


def _pass(p, g, dim, clamp):
    """One 1-D pass over [C,H,W] along `dim` (2: horizontal, 1: vertical): zero padding (gsl_load), taps added in ascending order."""
    pad = (MARGIN, MARGIN, 0, 0) if dim == 2 else (0, 0, MARGIN, MARGIN)
    q = F.pad(p[None], pad, mode="replicate" if clamp else "constant")[0]
    acc = torch.zeros_like(p)
    for k in range(11):
        acc = acc + float(g[k]) * q.narrow(dim, k, p.shape[dim])
    return acc


def kernel_statement(img, gt, w, lam=LAM, window_size=11, fault=None, upstream=1.0):
    """gsl_forward_kernel<true>, gsl_finish_kernel and gsl_backward_kernel, expression by expression, in torch on the CPU: the forward's two
    passes in float64 as the kernel runs them, everything else in float32 (no contraction: the compiler may fuse a multiply into an
    add on the device, which only removes a rounding).  Same return as `oracle`.
    fault: None, or one of FAULTS --
      sign0_is_plus            copysignf(1, d) for the L1 sign: +1 where img == gt
      clamp_to_edge            gsl_load clamps its coordinates instead of returning 0 outside the image
      dmu1_without_d_minus_cc  d ssim / d mu1 loses its 2 mu1 ssim (D - Cc) term
      planes_without_weight    the three derivative planes are stored without the weight
      last_column_left_weight  the pixel at x = W - 1 reads the weight of x = W - 2"""
    assert fault is None or fault in FAULTS, fault
    f32 = torch.float32
    x, y = _t(img).to(f32), _t(gt).to(f32)
    C, H, W = x.shape
    m = None if w is None else _t(w).to(f32).reshape(1, H, W).clone()
    if m is not None and fault == "last_column_left_weight" and W > 1:
        m[:, :, W - 1] = m[:, :, W - 2]
    g = taps(window_size)
    clamp = fault == "clamp_to_edge"
    blur = lambda p: _pass(_pass(p, g, 2, clamp), g, 1, clamp)      # horizontal into LDS, then vertical per pixel
    xd, yd = x.double(), y.double()                                 # the forward filters in float64 and rounds once, at A, B, Cc, D
    m1, m2, eS, e12 = blur(xd), blur(yd), blur(xd * xd + yd * yd), blur(xd * yd)
    C1, C2 = float(np.float32(0.01) * np.float32(0.01)), float(np.float32(0.03) * np.float32(0.03))
    m1_sq, m2_sq, m12 = m1 * m1, m2 * m2, m1 * m2
    mu1, mu2 = m1.to(f32), m2.to(f32)
    A, B, Cc, D = ((2.0 * m12 + C1).to(f32), (2.0 * (e12 - m12) + C2).to(f32), (m1_sq + m2_sq + C1).to(f32),
                   ((eS - m1_sq - m2_sq) + C2).to(f32))
    inv = 1.0 / (Cc * D)
    ssim = A * B * inv
    one = torch.ones((1, H, W), dtype=f32) if m is None else m
    ad = torch.abs(x - y)
    count = float(C) * float(H) * float(W)
    ml1, mss = float((ad * one).double().sum()) / count, float((ssim * one).double().sum()) / count
    a_l1, a_ssim = float(np.float32(1.0 - lam)), float(np.float32(-lam))
    loss = float(np.float32(np.float32(a_l1 * ml1 + a_ssim * mss) + np.float32(lam)))   # rgb_loss adds lambda to the kernel's out[0]
    dmu1 = 2.0 * mu2 * (B - A)
    if fault != "dmu1_without_d_minus_cc":
        dmu1 = dmu1 - 2.0 * mu1 * ssim * (D - Cc)
    dmu1, de11, de12 = dmu1 * inv, -ssim / D, 2.0 * A * inv
    pm = torch.ones_like(one) if fault == "planes_without_weight" else one
    f0, f1, f2 = blur(dmu1 * pm), blur(de11 * pm), blur(de12 * pm)
    d = x - y
    sgn = torch.where(d > 0, 1.0, torch.where(d < 0, -1.0, 1.0 if fault == "sign0_is_plus" else 0.0)).to(f32)
    c_l1, c_ssim = float(np.float32(a_l1 / count)), float(np.float32(a_ssim / count))
    grad = float(np.float32(upstream)) * (c_ssim * (f0 + 2.0 * x * f1 + y * f2) + c_l1 * sgn * one)
    assert grad.dtype == f32 and ssim.dtype == f32
    return loss, grad.double().numpy(), ssim.double().numpy(), ad.double().numpy()


# ---- the gates -----------------------------------------------------------------------------------------------------------------------
def region_gate(got, eager, ref, region, context="", yardstick=True):
    """got, eager, ref: [C,H,W] (under test, the reference in float32, the reference in float64); region: [H,W] int, negative = not
    looked at.  Per region k over all channels:  e_got = max|got - ref| <= 4 * max(e_ref, 2^-24 * value),  e_ref = max|eager - ref|,
    value = max|ref|; all three printed.  `yardstick`: on the structured frame eager's error, not the floor, sets the bound in every
    region (asserted: a region that fails it has the wrong inputs).  -> the worst ratio e_got / max(e_ref, 2^-24 value)."""
    got, eager, ref = (np.asarray(a, np.float64) for a in (got, eager, ref))
    assert got.shape == ref.shape == eager.shape and region.shape == ref.shape[-2:], (got.shape, eager.shape, ref.shape, region.shape)
    assert np.isfinite(got).all(), (context, "non-finite entries")
    worst, failures = 0.0, []
    for k in sorted(int(v) for v in np.unique(region) if v >= 0):
        sel = np.broadcast_to(region == k, ref.shape)
        e_got, e_ref, value = np.abs(got - ref)[sel].max(), np.abs(eager - ref)[sel].max(), np.abs(ref)[sel].max()
        bound = FACTOR * max(e_ref, EPS * value)
        ratio = 0.0 if e_got == 0 else (np.inf if bound == 0 else FACTOR * e_got / bound)
        name = NAMES[k] if k < len(NAMES) else ""
        print(f"[region gate] {context}: region {k} ({name}): e_got {e_got:.3g}, e_ref {e_ref:.3g}, value {value:.3g}, ratio {ratio:.3g}")
        if yardstick:
            assert e_ref > EPS * value, (context, "region", k, "eager's error does not set the bound: wrong inputs", e_ref, value)
        if not e_got <= bound:
            failures.append((k, name, "e_got", e_got, "bound", bound, "ratio", ratio))
        worst = max(worst, ratio)
    assert not failures, (context, "regions beyond 4 x the reference's own float32 error", failures)
    return worst


def relative_error(a, ref):
    """max|a - ref| / max|ref| (0 for two tensors of zeros)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    e, v = np.abs(a - ref).max(), np.abs(ref).max()
    return 0.0 if e == 0 else (np.inf if v == 0 else e / v)


def pooled_gate(cases):
    """cases: iterable of (window_size, got, eager, ref).  Per window size:  E_got = max over its cases of relative_error(got, ref)
    <= 4 * max(E_ref, 2^-24), E_ref likewise from eager.  -> {window_size: E_got / max(E_ref, 2^-24)}."""
    pool = {}
    for ws, got, eager, ref in cases:
        assert np.isfinite(np.asarray(got)).all(), (ws, np.asarray(ref).shape, "non-finite entries")
        e = pool.setdefault(int(ws), [0.0, 0.0, 0])
        e[0], e[1], e[2] = max(e[0], relative_error(got, ref)), max(e[1], relative_error(eager, ref)), e[2] + 1
    ratios = {}
    for ws, (E_got, E_ref, n) in sorted(pool.items()):
        ratios[ws] = E_got / max(E_ref, EPS)
        print(f"[pooled gate] window {ws}, {n} shapes: E_got {E_got:.3g}, E_ref {E_ref:.3g}, ratio {ratios[ws]:.3g}")
    bad = {ws: r for ws, r in ratios.items() if not r <= FACTOR}
    assert not bad, ("windows beyond 4 x the reference's own float32 error", bad)
    return ratios


def region_means_gate(means, img, gt, region, window_size=11, context=""):
    """The forward's maps, which the kernel reduces before anyone sees them, read region by region with an indicator weight:
    means(img, gt, indicator [1,H,W] float32) -> (mean(ssim_map 1_k), mean(|img - gt| 1_k)) over C H W, as ssim_masked and
    l1_loss_masked return them; times C H W / n_k they are the region's means.  Each within 4 * max(delta_k, 2^-24 * max|map64|) of the
    float64 map's mean, delta_k the largest per-pixel error of the eager float32 map in the region (the error of a mean is at most the
    largest per-pixel error; no division by one eager scalar that may be exact by chance).  -> the worst ratio."""
    _, _, s64, a64 = oracle(img, gt, None, LAM, window_size, torch.float64)
    _, _, s32, a32 = oracle(img, gt, None, LAM, window_size, torch.float32)
    C, H, W = s64.shape
    worst, failures = 0.0, []
    for k in sorted(int(v) for v in np.unique(region) if v >= 0):
        ind = (region == k).astype(np.float32)[None]
        sel = np.broadcast_to(region == k, s64.shape)
        n_k = int(sel.sum())
        got = [float(v) * (C * H * W) / n_k for v in means(img, gt, ind)]
        for what, g_, m64, m32 in (("ssim", got[0], s64, s32), ("l1", got[1], a64, a32)):
            delta, value = np.abs(m32 - m64)[sel].max(), np.abs(m64)[sel].max()
            bound = FACTOR * max(delta, EPS * value)
            err = abs(g_ - m64[sel].mean())
            ratio = 0.0 if err == 0 else (np.inf if bound == 0 else FACTOR * err / bound)
            print(f"[region means] {context}: region {k} ({NAMES[k]}) {what}: mean {m64[sel].mean():.9g}, error {err:.3g}, eager's worst pixel "
                  f"{delta:.3g}, ratio {ratio:.3g}")
            if not (np.isfinite(g_) and err <= bound):
                failures.append((k, NAMES[k], what, "got", g_, "ref", m64[sel].mean(), "bound", bound))
            worst = max(worst, ratio)
    assert not failures, (context, failures)
    return worst
