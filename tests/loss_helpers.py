"""The depth loss' gate (tests/test_gpu_loss.py, test_gpu_training_sizes.py, iteration_helpers.check_losses; proven without a GPU
in tests/test_loss_oracle.py): every pixel of dL/d(depth) within 1e-4 of the largest entry, and a pixel beyond that only where the
float64 oracle itself names a |.| term of that pixel within float32 rounding of zero -- by no more than that term's sign can move it.

The loss (oracle.loss_oracle.depth_loss, train.py:548-573) is a sum of |.| terms of the aligned depth a = |s0| d + t:

    L1 term at pixel p        c = (lambda_l1 w + lambda_fg fg)[p] / (H W)           value  r_p = a_p - y_p
    edge (p, q) at scale k    c = 0.5 lambda_smooth / M_k * g_p g_q                 value  g_q r_q - g_p r_p
                              (q the right or the lower neighbour of p on the ::2^k lattice, M_k the sum of g over that lattice)

so dL/da_p = sum of c * sign(value) * (the value's derivative by a_p: 1 for the L1 term, -g_p at p and +g_q at q for an edge).  A term
whose value float32 rounds to the other side of zero moves dL/da at its pixel(s) by 2 c g and dL/dd by |s0| times that.  An edge's
sign reaches other pixels only through the fit's sums (sum G, sum G d), by 2 c g / (H W)-ish each: far inside 1e-4 of the largest
entry.  An L1 term's sign at a pixel of weight 100 does not stay inside it (iteration_helpers._depth_gradient_choices), so L1 kinks
are not classified here: inputs are built without them (kink_free) or the caller enumerates them."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import loss_oracle as LO  # noqa: E402

KINK = 4e-6         # a |.| argument below this is inside float32's rounding of values the size of a depth (below 8): either sign
KINK_MARGIN = 1e-5  # inputs are BUILT with every |.| argument this far from zero
GRAD_TOL = 1e-4     # of the largest gradient entry: the depth loss' gradient bound since its first test
MAX_KINK_SHARE = 1e-4
#: the shapes of tests/test_gpu_loss.py's depth cases (tests/test_loss_oracle.py shows on the CPU that each can be made kink-free)
SHAPES = [(1, 1), (1, 2), (2, 2), (1, 33), (33, 1), (7, 9), (8, 8), (9, 8), (8, 9), (16, 17), (17, 16), (23, 41), (1, 255), (1, 256),
          (1, 257), (64, 64), (71, 112), (142, 252), (257, 256)]


def _map(a, H=None, W=None):
    if a is None:
        return None
    a = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a.detach().cpu()).double()
    return a.reshape(a.shape[-2:] if H is None else (H, W))


def depth_terms(d, y, lsq=None, w=None, g=None, lambda_l1=1.0, lambda_smooth=1.0, fg=None, lambda_fg=0.0):
    """Every |.| term of the depth loss in float64 from the (float32) inputs, the fit by LO.compute_scale_and_shift.
    -> namespace: H, W, s0 (signed), scale = |s0|, shift, det, Ms [4], residual [H, W], fit (the fit mask [H, W]), largest (max
    |aligned|, |target|), and per term the flat arrays  value, coef, k (-1: L1; 0..3: the edge's scale), p, q (flat pixel indices; q = p for an L1 term),
    cp, cq (|d(term)/da| at p and at q: coef for an L1 term and 0; coef g_p and coef g_q for an edge)."""
    D, Y = _map(d), _map(y)
    H, W = D.shape
    ones = torch.ones_like(D)
    M = ones if lsq is None else _map(lsq, H, W)
    Wt = ones if w is None else _map(w, H, W)
    G = ones if g is None else _map(g, H, W)
    s0, t = LO.compute_scale_and_shift(D[None], Y[None], M[None])
    s0, t = float(s0), float(t)
    det = float((M * D * D).sum() * M.sum() - (M * D).sum() ** 2)
    aligned = abs(s0) * D + t
    r = aligned - Y
    cl1 = lambda_l1 * Wt / (H * W)
    if fg is not None:
        cl1 = cl1 + lambda_fg * _map(fg, H, W) / (H * W)
    idx = torch.arange(H * W).reshape(H, W)
    zero = torch.zeros(H * W, dtype=torch.float64)
    cols = dict(value=[r.reshape(-1)], coef=[cl1.reshape(-1)], k=[torch.full((H * W,), -1)], p=[idx.reshape(-1)], q=[idx.reshape(-1)],
                cp=[cl1.reshape(-1)], cq=[zero])
    Ms = []
    for k in range(4):
        st = 2 ** k
        gk, ik = G[::st, ::st], idx[::st, ::st]
        diff = gk * r[::st, ::st]                                  # gradient_loss: mask * (prediction - target)
        Mk = float(gk.sum())
        Ms.append(Mk)
        c = 0.0 if Mk == 0 else 0.5 * lambda_smooth / Mk           # reduction_batch_based: 0 when the divisor is 0
        for a, b in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))),      # grad_x: [:, 1:] - [:, :-1]
                     ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):     # grad_y: [1:, :] - [:-1, :]
            co = c * gk[b] * gk[a]
            cols["value"].append((diff[b] - diff[a]).reshape(-1))
            cols["coef"].append(co.reshape(-1))
            cols["k"].append(torch.full((co.numel(),), k))
            cols["p"].append(ik[a].reshape(-1))
            cols["q"].append(ik[b].reshape(-1))
            cols["cp"].append((co * gk[a]).reshape(-1))
            cols["cq"].append((co * gk[b]).reshape(-1))
    out = types.SimpleNamespace(H=H, W=W, s0=s0, scale=abs(s0), shift=t, det=det, Ms=Ms, residual=r.numpy(), fit=M.numpy(),
                                largest=max(float(aligned.abs().max()), float(Y.abs().max())))
    for name, parts in cols.items():
        setattr(out, name, torch.cat(parts).numpy())
    return out


def kink_margin(terms):
    """KINK, sized for depths below 8, scaled with the largest |aligned| or |target| beyond that."""
    return KINK * max(1.0, terms.largest / 8.0)


def kink_terms(terms, margin):
    """Indices (into the term arrays) of the terms with a nonzero coefficient whose |value| < margin."""
    return np.nonzero((terms.coef != 0) & (np.abs(terms.value) < margin))[0]


def kink_free(d, y, lsq=None, w=None, g=None, lambda_l1=1.0, lambda_smooth=1.0, fg=None, lambda_fg=0.0, rng=None, rounds=20):
    """A copy of the target `y` (float32) with no term of the loss within KINK_MARGIN of zero: while there is one, the target at one
    endpoint of each (the pixel of an L1 term, the far end q of an edge) moves by +-3e-3 and everything, the fit included, is
    computed again.  A condition on the INPUTS, from the oracle alone; asserted.  -> (y, terms of the result, rounds used)"""
    rng = rng or np.random.default_rng(0)
    y = np.array(y, dtype=np.float32, copy=True)
    args = (lsq, w, g, lambda_l1, lambda_smooth, fg, lambda_fg)
    for used in range(rounds + 1):
        terms = depth_terms(d, y, *args)
        hits = kink_terms(terms, KINK_MARGIN)
        if hits.size == 0:
            return y, terms, used
        for q in np.unique(terms.q[hits]):
            y.reshape(-1)[q] += np.float32(3e-3 * rng.choice((-1.0, 1.0)))
    raise AssertionError(f"kink_free: {hits.size} terms still within {KINK_MARGIN} of zero after {rounds} rounds")


def depth_case3(seed, H, W, slope=0.6, offset=0.4):
    """Inputs that tell the three masks apart: depth d = slope y + offset + noise, target y in [1, 6), a binary fit mask, a
    FRACTIONAL L1 weight in [0, 1.5) with about 20 % zeros, a different binary gradient mask, a rectangle fg.  The fit mask keeps at
    least three pixels where the picture has them (a fit through two points is exact: every residual a kink); a two-pixel picture gets
    the fit mask (1, 0), which the reference calls singular (det = 0: scale = shift = 0).  -> namespace d, y, m, w, g, fg"""
    rng = np.random.default_rng(seed)
    y = (rng.random((H, W)) * 5 + 1).astype(np.float32)
    d = (slope * y + offset + 0.08 * rng.standard_normal((H, W))).astype(np.float32)
    m = (rng.random((H, W)) > 0.3).astype(np.float32)
    if H * W >= 3 and m.sum() < 3:
        m.reshape(-1)[:3] = 1.0
    if H * W == 2:
        m.reshape(-1)[:] = (1.0, 0.0)
    w = (rng.random((H, W)) * 1.5 * (rng.random((H, W)) > 0.2)).astype(np.float32)
    g = (rng.random((H, W)) > 0.25).astype(np.float32)
    fg = np.zeros((H, W), np.float32)
    fg[H // 5:(4 * H) // 5 + 1, W // 4:(3 * W) // 4 + 1] = 1.0
    return types.SimpleNamespace(d=d, y=y, m=m, w=w, g=g, fg=fg, H=H, W=W)


def case_config(c, how):
    """The three ways every shape runs -> kwargs of depth_terms / kink_free / the oracle (lsq, w, g, lambdas, fg)."""
    if how == "plain":
        return dict(lsq=None, w=None, g=None, lambda_l1=0.7, lambda_smooth=0.4, fg=None, lambda_fg=0.0)
    if how == "masks":
        return dict(lsq=c.m, w=c.w, g=c.g, lambda_l1=0.7, lambda_smooth=0.4, fg=None, lambda_fg=0.0)
    assert how == "fg", how
    return dict(lsq=c.m, w=None, g=None, lambda_l1=1.0, lambda_smooth=1.0, fg=c.fg, lambda_fg=99.0)


def oracle_run(dtype):
    """The oracle as the side under test: run(d, y, upstream, **config) -> (loss, |scale|, shift, gradient of upstream * loss)."""
    def run(d, y, upstream, lsq, w, g, lambda_l1, lambda_smooth, fg, lambda_fg):
        loss, s, t, grad = LO.depth_value_and_grad(d, y, lsq, w, g, lambda_l1, lambda_smooth, dtype=dtype, fg_mask=fg, lambda_fg=lambda_fg)
        return loss, s, t, upstream * grad.astype(np.float64)
    return run


def check_depth_case(run, d, y, cfg, upstream=1.5, context="", values=True, kinks=0, worst=None):
    """One case against the float64 oracle: loss within 2e-6 (relative beyond 1), scale 2e-6, shift 5e-6 (`values`), the gradient by
    assert_depth_grad with exactly `kinks` explained pixels (0: none beyond the bound at all).  `worst` collects the errors."""
    ref_loss, ref_s, ref_t, ref_g = oracle_run(torch.float64)(d, y, upstream, **cfg)
    terms = depth_terms(d, y, **cfg)
    assert abs(terms.scale - ref_s) <= 1e-12 * max(1.0, ref_s) and abs(terms.shift - ref_t) <= 1e-12 * max(1.0, abs(ref_t))
    loss, s, t, grad = run(d, y, upstream, **cfg)
    e = {"loss": abs(loss - ref_loss) / max(1.0, abs(ref_loss)), "scale": abs(s - ref_s) / max(1.0, abs(ref_s)),
         "shift": abs(t - ref_t) / max(1.0, abs(ref_t)),
         "grad": float(np.abs(np.asarray(grad, np.float64).reshape(ref_g.shape) - ref_g).max() / max(np.abs(ref_g).max(), 1e-300))}
    if worst is not None:
        for k_, v in e.items():
            worst[k_] = max(worst.get(k_, 0.0), v)
    print(f"\n[depth case] {context}: " + ", ".join(f"{k_} {v:.3g}" for k_, v in e.items()))
    if values:
        assert e["loss"] < 2e-6 and e["scale"] < 2e-6 and e["shift"] < 5e-6, (context, e, (loss, ref_loss), (s, ref_s), (t, ref_t))
    n = assert_depth_grad(grad, ref_g, terms, ref_s, upstream=upstream, context=context)
    assert n == kinks, (context, "pixels beyond the bound", n, "expected", kinks)
    return types.SimpleNamespace(ref_loss=ref_loss, ref_s=ref_s, ref_t=ref_t, ref_g=ref_g, terms=terms, loss=loss, scale=s, shift=t, grad=grad, err=e)


def kinks_of_continuous_data(terms, wide=100):
    """How many terms a picture of continuous data may hold within kink_margin of zero, from the oracle's terms alone: values spread
    smoothly across zero put 1 / wide of those within wide * kink_margin inside kink_margin itself.  Twice that share plus 4 (a
    Poisson count of a few is often twice its mean).  For GIVEN pictures (a rendered depth): a fixed share of the pixels does not fit
    them -- the float32 oracle chain of tests/test_iteration.py holds up to 14 such terms in its 17 472 pixels, two of them within
    5e-7 of zero in one picture -- but a count far above this one means a picture whose zeros are no accident of rounding (flat
    regions, repeated values), which this check must not wave through term by term."""
    m = kink_margin(terms)
    return 2.0 * kink_terms(terms, wide * m).size / wide + 4.0


def assert_depth_grad(got, ref64, terms, scale, upstream=1.0, context="", l1_enumerated=False, max_kinks=None):
    """`got` [H, W]: dL/d(depth) under test, `ref64` the float64 oracle's, both of `upstream` times the loss; `terms` =
    depth_terms of the same inputs, `scale` the oracle's |scale|.
      * the terms within kink_margin of zero, from the oracle alone, are at most MAX_KINK_SHARE of the pixel count (`max_kinks`:
        another cap, for given pictures: kinks_of_continuous_data), asserted BEFORE `got` is looked at.  An L1 term among them fails
        the check unless the caller enumerates its signs (`l1_enumerated`: ref64 is then one of
        iteration_helpers._depth_gradient_choices)
      * every pixel within GRAD_TOL of the largest |ref64|, except an endpoint of such an edge term, which may deviate by
        upstream * scale * sum(2 * that term's coefficient at the pixel) on top of it
      * a pixel the loss does not depend on (outside the fit mask and every coefficient that reaches it zero; every pixel when the
        fit is singular, det = 0: |scale| = 0 has the derivative 0) is exactly zero.  A pixel where nonzero terms happen to cancel
        in float64 is not meant: float32 need not cancel there
    -> number of pixels beyond the plain bound that the kink terms explain (0 on kink-free inputs), printed."""
    got, ref64 = np.asarray(got, np.float64).reshape(terms.H, terms.W), np.asarray(ref64, np.float64).reshape(terms.H, terms.W)
    hits = kink_terms(terms, kink_margin(terms))
    cap = MAX_KINK_SHARE * terms.H * terms.W if max_kinks is None else max_kinks
    assert hits.size <= cap, (context, "terms on a kink", hits.size, "of", terms.H * terms.W, "pixels; at most", cap)
    l1 = hits[terms.k[hits] < 0]
    assert l1_enumerated or l1.size == 0, (context, "L1 terms on the kink, not enumerated", l1.tolist())
    edges = hits[terms.k[hits] >= 0]
    slack = np.zeros(terms.H * terms.W)
    np.add.at(slack, terms.p[edges], 2.0 * terms.cp[edges])
    np.add.at(slack, terms.q[edges], 2.0 * terms.cq[edges])
    slack = (abs(upstream) * scale * slack).reshape(terms.H, terms.W)
    assert np.isfinite(got).all(), (context, "non-finite gradient")
    bound = GRAD_TOL * np.abs(ref64).max()
    err = np.abs(got - ref64)
    beyond = err > bound
    unexplained = err > bound + slack
    touch = np.zeros(terms.H * terms.W)                              # sum of the coefficients that reach a pixel
    np.add.at(touch, terms.p, np.abs(terms.cp))
    np.add.at(touch, terms.q, np.abs(terms.cq))
    structural = ((terms.fit == 0) & (touch.reshape(terms.H, terms.W) == 0)) | (terms.det == 0)
    assert not np.any(ref64[structural]), (context, "the oracle is not zero where the loss does not depend on the depth")
    zero_rows = structural & (slack == 0)
    n = int(beyond.sum())
    print(f"\n[depth grad] {context}: worst {err.max() / max(np.abs(ref64).max(), 1e-300):.3g} of the largest entry, {hits.size} kink term(s), "
          f"{n} pixel(s) beyond {GRAD_TOL:g}, {int(unexplained.sum())} unexplained")
    if unexplained.any():
        yy, xx = np.unravel_index(int(np.argmax(err - slack)), err.shape)
        raise AssertionError((context, "pixels beyond the bound that no kink explains", int(unexplained.sum()), "worst at", (int(yy), int(xx)),
                              "got", float(got[yy, xx]), "ref", float(ref64[yy, xx]), "bound", float(bound), "slack", float(slack[yy, xx])))
    bad_zero = zero_rows & (got != 0)
    assert not bad_zero.any(), (context, "pixels whose reference gradient is exactly zero are not", int(bad_zero.sum()))
    return n
