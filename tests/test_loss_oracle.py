"""CPU tests of the loss oracle (oracle/loss_oracle.py) and of the committed loss fixtures, and the depth loss' gate
(tests/loss_helpers.py) proven without a GPU: the "device" is the loss oracle in float32.  It passes on kink-free inputs with no
pixel beyond the bound, each planted fault fails, and a deliberate kink is classified by the oracle's own terms -- no further.
tests/test_gpu_loss.py runs the same checks on the HIP kernels."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_helpers as LH  # noqa: E402
from golden import make_loss_golden as MLG  # noqa: E402
from oracle import loss_oracle as LO  # noqa: E402


def test_window_matches_the_published_constants():
    g = LO.gaussian(11, 1.5)
    assert abs(float(g.sum()) - 1.0) < 1e-6 and g.argmax() == 5 and torch.allclose(g, g.flip(0))
    assert abs(float(g[5]) - 0.26601171) < 1e-7 and abs(float(g[0]) - 0.00102838) < 1e-8
    # the 2-D window is the outer product, so it is separable -- the property the HIP kernel relies on
    w = LO.create_window(11, 3, torch.float64)[0, 0]
    assert torch.allclose(w, torch.outer(g.double(), g.double()), atol=1e-9)


def test_identities():
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.random((3, 24, 31)))
    assert abs(float(LO.ssim(x, x)) - 1.0) < 1e-9 and float(LO.l1_loss(x, x)) == 0.0
    m = torch.from_numpy((rng.random((1, 24, 31)) > 0.5).astype(np.float64))
    assert abs(float(LO.ssim_masked(x, x, m)) - float(m.mean())) < 1e-9
    assert abs(float(LO.rgb_loss(x, x)) - 0.0) < 1e-9
    y = torch.from_numpy(rng.random((3, 24, 31)))
    assert abs(float(LO.ssim(x, y)) - float(LO.ssim(y, x))) < 1e-12  # symmetric in its arguments


def test_gradient_against_finite_differences():
    rng = np.random.default_rng(1)
    x, y = rng.random((2, 9, 12)), rng.random((2, 9, 12))
    w = rng.random((1, 9, 12))
    _, _, _, g = LO.value_and_grad(x, y, w, 0.3, 1.7)
    eps = 1e-6
    for idx in [(0, 0, 0), (1, 4, 7), (0, 8, 11), (1, 3, 0)]:
        xp, xm = x.copy(), x.copy()
        xp[idx] += eps
        xm[idx] -= eps
        fd = (LO.value_and_grad(xp, y, w, 0.3, 1.7)[0] - LO.value_and_grad(xm, y, w, 0.3, 1.7)[0]) / (2 * eps)
        assert abs(fd - g[idx]) < 1e-6 * max(1.0, abs(fd)), (idx, fd, g[idx])


def test_fixtures_reproduce():
    for name, c in MLG.cases().items():
        img, gt, w = MLG.make_inputs(c)
        exp = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        loss, l1, ss, grad = LO.value_and_grad(img, gt, w, c["lam"], c["scale"])
        assert abs(loss - float(exp["loss"])) < 1e-12 and abs(ss - float(exp["ssim"])) < 1e-12
        assert np.allclose(grad, exp["grad"], rtol=0, atol=1e-14)
        # fp32 evaluation of the same restatement stays within the GPU test's tolerance of the fp64 fixture
        l32 = LO.value_and_grad(img, gt, w, c["lam"], c["scale"], dtype=torch.float32)[0]
        assert abs(l32 - loss) < 2e-6


def test_knn_oracle_against_brute_force():
    """oracle/knn_oracle.py (exact 3-NN through a k-d tree) against the O(P^2) definition."""
    from oracle import knn_oracle as KO
    rng = np.random.default_rng(3)
    pts = rng.random((400, 3))
    pts[10:20] = pts[0:10]  # coincident points are neighbours at distance 0
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d2, np.inf)
    ref = np.sort(d2, axis=1)[:, :3].mean(1)
    assert np.allclose(KO.mean_dist2(pts), ref, rtol=1e-12, atol=1e-15)
    assert KO.mean_dist2(pts[:0]).shape == (0,) and np.all(KO.mean_dist2(pts[:3]) > 1e37)


def test_depth_oracle_gradient_and_fixtures():
    """The depth terms: autograd gradient (through the least-squares fit) against finite differences, the closed-form
    fit against numpy's lstsq, and the committed fixtures."""
    rng = np.random.default_rng(5)
    y = rng.random((7, 9)) * 4 + 1
    d = 0.8 * y - 0.3 + 0.1 * rng.standard_normal(y.shape)
    m = (rng.random(y.shape) > 0.25).astype(np.float64)
    loss, s, t, g = LO.depth_value_and_grad(d, y, m, m, m, 0.9, 0.6)
    A = np.stack([d[m > 0], np.ones(int(m.sum()))], 1)
    sol = np.linalg.lstsq(A, y[m > 0], rcond=None)[0]
    assert abs(abs(sol[0]) - s) < 1e-9 and abs(sol[1] - t) < 1e-9
    eps = 1e-6
    for idx in [(0, 0), (3, 4), (6, 8), (2, 7)]:
        dp, dm = d.copy(), d.copy()
        dp[idx] += eps
        dm[idx] -= eps
        fd = (LO.depth_value_and_grad(dp, y, m, m, m, 0.9, 0.6)[0] - LO.depth_value_and_grad(dm, y, m, m, m, 0.9, 0.6)[0]) / (2 * eps)
        assert abs(fd - g[idx]) < 1e-6 * max(1.0, abs(fd)), (idx, fd, g[idx])
    for name, c in MLG.depth_cases().items():
        dd, yy, mm, wg = MLG.make_depth_inputs(c)
        exp = np.load(os.path.join(ROOT, "tests", "golden", "loss_" + name + ".npz"))
        l2, s2, t2, g2 = LO.depth_value_and_grad(dd, yy, mm, wg, wg, c["l1"], c["sm"])
        assert abs(l2 - float(exp["loss"])) < 1e-12 and np.allclose(g2, exp["grad"], rtol=0, atol=1e-14)


# ==== the depth loss gate of tests/loss_helpers.py, proven on the oracle in float32 ==================================================
F32 = LH.oracle_run(torch.float32)
UP = 1.5


def _case(seed, H, W, how, **kw):
    c = LH.depth_case3(seed, H, W, **kw)
    cfg = LH.case_config(c, how)
    y, terms, rounds = LH.kink_free(c.d, c.y, **cfg, rng=np.random.default_rng(seed))
    return c, cfg, y, terms, rounds


@pytest.mark.parametrize("how", ["plain", "masks", "fg"])
@pytest.mark.parametrize("H,W", [(1, 33), (8, 9), (23, 41), (71, 112), (257, 256)])
def test_float32_oracle_passes_on_kink_free_inputs(H, W, how):
    """The reference's own arithmetic in float32 (fit included) against float64, gradient only: no pixel beyond 1e-4 of the largest
    entry, no kink term.  kink_free needs at most one round.  Worst measured over the fifteen cases: 2.3e-6 of the largest entry (1e-4)."""
    c, cfg, y, terms, rounds = _case(H * 100 + W, H, W, how)
    assert rounds <= 1 and LH.kink_terms(terms, LH.KINK_MARGIN).size == 0
    LH.check_depth_case(F32, c.d, y, cfg, upstream=UP, context=f"{H}x{W} {how}", values=False)


def test_every_shape_of_the_gpu_tests_can_be_made_kink_free():
    """All shapes of tests/test_gpu_loss.py, the three ways each (1x2 without masks is an exact fit: every residual a kink, so that
    one is checked by value only): kink_free ends within two rounds."""
    for H, W in LH.SHAPES:
        for how in ("plain", "masks", "fg"):
            if (H, W, how) == (1, 2, "plain"):
                continue
            *_, rounds = _case(H * 100 + W, H, W, how)
            assert rounds <= 2, (H, W, how, rounds)


def test_committed_golden_inputs_hold_no_kink():
    for name, c in MLG.depth_cases().items():
        d, y, m, wg = MLG.make_depth_inputs(c)
        terms = LH.depth_terms(d, y, m, wg, wg, c["l1"], c["sm"])
        assert LH.kink_terms(terms, LH.KINK_MARGIN).size == 0, name


# ---- planted faults: each must fail ---------------------------------------------------------------------------------------------------
def _swapped(d, y, upstream, lsq, w, g, **kw):
    return F32(d, y, upstream, lsq=lsq, w=g, g=w, **kw)


def _fit_mask_as_gradient_mask(d, y, upstream, lsq, w, g, **kw):
    return F32(d, y, upstream, lsq=lsq, w=w, g=lsq, **kw)


def _sign_factor_dropped(d, y, upstream, lsq, w, g, lambda_l1, lambda_smooth, fg, lambda_fg):
    """The oracle's composition in float32 with d|s0|/ds0 taken as +1: the value |s0|, the derivative that of s0."""
    t = lambda a: None if a is None else torch.as_tensor(a).float().reshape(1, *np.shape(a)[-2:])
    x = t(d).clone().requires_grad_(True)
    s0, shift = LO.compute_scale_and_shift(x, t(y), t(lsq))
    scale = s0 + (s0.abs() - s0).detach()
    aligned = scale.view(-1, 1, 1) * x + shift.view(-1, 1, 1)
    loss = lambda_l1 * LO.l1_loss_masked(aligned, t(y), t(w))
    for k in range(4):
        st = 2 ** k
        loss = loss + 0.5 * lambda_smooth * LO.gradient_loss(aligned[:, ::st, ::st], t(y)[:, ::st, ::st], t(g)[:, ::st, ::st])
    loss.backward()
    return float(loss.detach()), float(scale.detach()), float(shift.detach()), upstream * x.grad[0].double().numpy()


@pytest.mark.parametrize("fault", [_swapped, _fit_mask_as_gradient_mask], ids=["l1_weight_and_grad_mask_swapped", "fit_mask_as_gradient_mask"])
def test_mask_mixups_fail(fault):
    c, cfg, y, terms, _ = _case(7, 23, 41, "masks")
    LH.check_depth_case(F32, c.d, y, cfg, upstream=UP, context="untouched", values=False)
    with pytest.raises(AssertionError):
        LH.check_depth_case(fault, c.d, y, cfg, upstream=UP, context=fault.__name__, values=False)


def test_dropped_sign_factor_fails_on_a_negative_slope_only():
    c, cfg, y, terms, _ = _case(8, 23, 41, "masks", slope=-0.6, offset=5.0)
    assert terms.s0 < 0
    LH.check_depth_case(F32, c.d, y, cfg, upstream=UP, context="negative slope", values=False)
    with pytest.raises(AssertionError):
        LH.check_depth_case(_sign_factor_dropped, c.d, y, cfg, upstream=UP, context="sign dropped", values=False)
    c, cfg, y, terms, _ = _case(8, 23, 41, "masks")   # with s0 > 0 the factor is +1: the same "device" is right
    assert terms.s0 > 0
    LH.check_depth_case(_sign_factor_dropped, c.d, y, cfg, upstream=UP, context="sign dropped, positive slope", values=False)


def test_last_coarse_lattice_column_wrong_passes_the_old_rule_and_fails_this_one():
    """142x252: the gradient wrong on the 18 pixels of the ::8 lattice's last column (x = 248) only -- 5e-4 of the pixels, inside the
    old `2e-3 of the pixels may be anything` allowance, which is why that allowance had to go."""
    H, W = 142, 252
    c, cfg, y, terms, _ = _case(9, H, W, "masks")
    ref = F32(c.d, y, UP, **cfg)

    def wrong(*a, **k):
        grad = ref[3].copy()
        grad[::8, 248] += 0.5 * np.abs(grad).max()
        return ref[0], ref[1], ref[2], grad
    ref64 = LH.oracle_run(torch.float64)(c.d, y, UP, **cfg)[3]
    old_rule = (np.abs(wrong()[3] - ref64) > 1e-4 * np.abs(ref64).max()).mean()
    assert 0 < old_rule <= 2e-3, old_rule
    with pytest.raises(AssertionError):
        LH.check_depth_case(wrong, c.d, y, cfg, upstream=UP, context="last ::8 column", values=False)


# ---- one deliberate kink ------------------------------------------------------------------------------------------------------------
def test_a_deliberate_edge_kink_is_classified_and_bounded():
    """A full-resolution edge (both gradient-mask values 1, the far end outside the fit mask, so the fit does not move) has its
    target moved until the edge's value is float32's nearest to zero (below 5e-7).  The side under test is the oracle with that edge
    on the OTHER side of zero: two pixels beyond the bound, both explained by the one kink term; the same gradient with one of the two
    pixels moved by three times the term's coefficient (the allowance is two) fails, and so does a pixel that is no endpoint of the
    term.  The picture is 105x105 so that one kink term is within the cap of 1e-4 of the pixel count; the same single term in a
    picture of 64x64 is refused before the side under test is looked at."""
    H = W = 105
    c, cfg, y, terms, _ = _case(10, H, W, "masks")
    m, g = c.m.reshape(-1), c.g.reshape(-1)
    e = next(i for i in np.nonzero(terms.k == 0)[0] if g[terms.p[i]] == 1 and g[terms.q[i]] == 1 and m[terms.q[i]] == 0)
    p, q = int(terms.p[e]), int(terms.q[e])
    y = y.copy()
    for _ in range(3):   # the target is float32: step onto the representable value nearest to the root
        y.reshape(-1)[q] = np.float32(np.float64(y.reshape(-1)[q]) + LH.depth_terms(c.d, y, **cfg).value[e])
    terms = LH.depth_terms(c.d, y, **cfg)
    v = terms.value[e]
    assert 0 < abs(v) < 5e-7 and LH.kink_terms(terms, LH.kink_margin(terms)).tolist() == [e]
    assert 1 <= LH.MAX_KINK_SHARE * H * W < 2
    ref64 = LH.oracle_run(torch.float64)(c.d, y, UP, **cfg)[3]
    other = y.copy()
    other.reshape(-1)[q] += np.float32(2 * LH.KINK * np.sign(v))      # value = ... - y_q: the edge lands on the other side of zero
    assert LH.depth_terms(c.d, other, **cfg).value[e] * v < 0
    flipped = LH.oracle_run(torch.float64)(c.d, other, UP, **cfg)[3]
    step = 2 * UP * terms.scale * terms.cp[e]
    assert abs(abs(flipped.reshape(-1)[p] - ref64.reshape(-1)[p]) - step) < 1e-3 * step and step > 2 * LH.GRAD_TOL * np.abs(ref64).max()
    assert LH.assert_depth_grad(flipped, ref64, terms, terms.scale, upstream=UP, context="edge flipped") == 2
    assert LH.assert_depth_grad(F32(c.d, y, UP, **cfg)[3], ref64, terms, terms.scale, upstream=UP, context="float32 oracle on the kink") in (0, 2)
    too_far = flipped.copy()
    too_far.reshape(-1)[p] = ref64.reshape(-1)[p] + 1.5 * (flipped.reshape(-1)[p] - ref64.reshape(-1)[p])
    with pytest.raises(AssertionError):
        LH.assert_depth_grad(too_far, ref64, terms, terms.scale, upstream=UP, context="three coefficients")
    elsewhere = flipped.copy()
    elsewhere[50, 50] += 3 * LH.GRAD_TOL * np.abs(ref64).max()      # a pixel that is no endpoint of the kink: never explained
    assert 50 * W + 50 not in (p, q)
    with pytest.raises(AssertionError):
        LH.assert_depth_grad(elsewhere, ref64, terms, terms.scale, upstream=UP, context="another pixel")
    # the cap: the same single kink term in a picture of fewer than 10 000 pixels is refused before the device's output is read
    small = LH.depth_terms(c.d[:64, :64], y[:64, :64], **{k: (v_[:64, :64] if isinstance(v_, np.ndarray) else v_) for k, v_ in cfg.items()})
    small.coef[0], small.value[0] = 1.0, 1e-7
    small.k[0] = 0
    with pytest.raises(AssertionError, match="terms on a kink"):
        LH.assert_depth_grad(np.zeros((64, 64)), np.zeros((64, 64)), small, small.scale)


def test_an_l1_kink_is_refused_unless_enumerated():
    c, cfg, y, terms, _ = _case(11, 105, 105, "masks")
    i = int(np.nonzero((terms.k < 0) & (terms.coef != 0))[0][0])
    terms.value[i] = 1e-7
    ref64 = LH.oracle_run(torch.float64)(c.d, y, UP, **cfg)[3]
    with pytest.raises(AssertionError, match="L1 terms"):
        LH.assert_depth_grad(ref64, ref64, terms, terms.scale, upstream=UP)
    assert LH.assert_depth_grad(ref64, ref64, terms, terms.scale, upstream=UP, l1_enumerated=True) == 0


# ---- the singular fits the kernel used to solve -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d0,y0", [(0.7, 2.3), (1.3, 4.1), (3.1, 0.9)])
def test_one_pixel_fit_is_singular_in_the_reference_and_not_in_float32_products_widened_late(d0, y0):
    """What depth_loss.hip's sums did before they widened first: the float32 square, then double.  The reference's float32 det and the
    float64 det are exactly 0; that one was the rounding error of one float32 square, and the solve returned noise over noise."""
    d, y = np.float32(d0), np.float32(y0)
    assert np.float32(np.float32(d * d) * np.float32(1) - np.float32(d * d)) == 0 and np.float64(d) * np.float64(d) * 1.0 - np.float64(d) ** 2 == 0
    late = np.float64(np.float32(d * d)) * 1.0 - np.float64(d) * np.float64(d)
    assert late != 0 and abs((1.0 * np.float64(np.float32(d * y)) - np.float64(d) * np.float64(y)) / late) > 0.1
    early = (np.float64(d) * np.float64(d)) * 1.0 - np.float64(d) * np.float64(d)
    assert early == 0
