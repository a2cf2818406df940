"""GPU parity tests of the fused RGB loss (gscream_amd.loss_utils -> ctypes -> gsr_rgb_loss_*) and of the depth loss
(gsr_depth_loss_*) against the CPU oracle (float64 restatement of GScream's utils/loss_utils.py) and the committed fixtures.

Tolerances (floating point; fp32 kernel vs fp64 oracle): loss / terms 2e-6 abs; gradient 1e-4 of its largest entry
(the separable window reorders the 121-term sums; measured differences are ~1e-6).  Depth loss: see the section's header."""
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

pytestmark = pytest.mark.gpu


def _run(img, gt, w, lam, scale):
    from gscream_amd import loss_utils as L
    x = torch.from_numpy(img).cuda().requires_grad_(True)
    y = torch.from_numpy(gt).cuda()
    m = None if w is None else torch.from_numpy(w).cuda()
    loss, l1, ss = L.rgb_loss(x, y, m, lam, scale, return_parts=True)
    loss.backward()
    return float(loss.detach()), float(l1), float(ss), x.grad.cpu().numpy()


@pytest.mark.parametrize("name", sorted(MLG.cases().keys()))
def test_golden(name):
    c = MLG.cases()[name]
    img, gt, w = MLG.make_inputs(c)
    exp = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    loss, l1, ss, grad = _run(img, gt, w, c["lam"], c["scale"])
    assert abs(loss - float(exp["loss"])) < 2e-6 and abs(l1 - float(exp["l1"])) < 2e-6 and abs(ss - float(exp["ssim"])) < 2e-6
    assert np.abs(grad - exp["grad"]).max() <= 1e-4 * np.abs(exp["grad"]).max()


@pytest.mark.parametrize("C,H,W,weighted", [(3, 71, 112, False), (3, 142, 252, True), (1, 33, 65, True), (3, 16, 32, False)])
def test_against_live_oracle(C, H, W, weighted):
    rng = np.random.default_rng(C * 1000 + H)
    gt = rng.random((C, H, W)).astype(np.float32)
    img = np.clip(gt + 0.2 * rng.standard_normal(gt.shape), 0, 1).astype(np.float32)
    w = rng.random((1, H, W)).astype(np.float32) if weighted else None
    ref = LO.value_and_grad(img, gt, w, 0.2, 1.0)
    got = _run(img, gt, w, 0.2, 1.0)
    for a, b in zip(got[:3], ref[:3]):
        assert abs(a - b) < 2e-6
    assert np.abs(got[3] - ref[3]).max() <= 1e-4 * np.abs(ref[3]).max()


def test_mirrored_functions_and_upstream_gradient():
    """The four names the trainer imports, with a non-unit upstream gradient (train.py:538-545 mixes them)."""
    from gscream_amd import loss_utils as L
    rng = np.random.default_rng(5)
    gt = rng.random((3, 48, 80)).astype(np.float32)
    img = np.clip(gt + 0.1 * rng.standard_normal(gt.shape), 0, 1).astype(np.float32)
    mask = (rng.random((1, 48, 80)) > 0.5).astype(np.float32)
    x = torch.from_numpy(img).cuda().requires_grad_(True)
    y, m = torch.from_numpy(gt).cuda(), torch.from_numpy(mask).cuda()
    total = 0.8 * L.l1_loss(x, y) + 0.2 * (1.0 - L.ssim(x, y)) + 0.5 * (0.8 * L.l1_loss_masked(x, y, m) + 0.2 * (1.0 - L.ssim_masked(x, y, m)))
    total.backward()
    xr = torch.from_numpy(img).double().requires_grad_(True)
    yr, mr = torch.from_numpy(gt).double(), torch.from_numpy(mask).double()
    ref = 0.8 * LO.l1_loss(xr, yr) + 0.2 * (1.0 - LO.ssim(xr, yr)) + 0.5 * (0.8 * LO.l1_loss_masked(xr, yr, mr) + 0.2 * (1.0 - LO.ssim_masked(xr, yr, mr)))
    ref.backward()
    assert abs(float(total.detach()) - float(ref.detach())) < 3e-6
    assert (x.grad.cpu().double() - xr.grad).abs().max() <= 1e-4 * xr.grad.abs().max()
    # other window sizes (loss_utils.py:131 `window_size`): odd, up to 11 -- the same kernels with zero taps at both ends
    for ws in (1, 3, 7):
        x2 = torch.from_numpy(img).cuda().requires_grad_(True)
        v = L.ssim(x2, y, window_size=ws)
        vm = L.ssim_masked(x2, y, m, window_size=ws)
        (v + 0.5 * vm).backward()
        x3 = torch.from_numpy(img).double().requires_grad_(True)
        r = LO.ssim_map(x3, yr, ws).mean()
        rm = (LO.ssim_map(x3, yr, ws) * mr).mean()
        (r + 0.5 * rm).backward()
        assert abs(float(v.detach()) - float(r.detach())) < 3e-6 and abs(float(vm.detach()) - float(rm.detach())) < 3e-6, ws
        assert (x2.grad.cpu().double() - x3.grad).abs().max() <= 1e-4 * x3.grad.abs().max(), ws
    with pytest.raises(NotImplementedError):
        L.ssim(x, y, window_size=8)   # even: the reference's map changes size
    with pytest.raises(NotImplementedError):
        L.ssim(x, y, window_size=13)  # beyond the 11-tap frame
    with pytest.raises(RuntimeError):
        L.ssim(x.detach().cpu(), y.cpu())
    # size_average=False (loss_utils.py:157-160): one mean per image of a [B,C,H,W] batch; B = 1 here
    per = L.ssim(x.detach()[None], y[None], size_average=False)
    assert per.shape == (1,) and abs(float(per[0]) - float(LO.ssim(xr.detach(), yr))) < 3e-6
    with pytest.raises(NotImplementedError):
        L.ssim(x, y, size_average=False)  # the reference's .mean(1).mean(1).mean(1) needs the batch dimension too


def test_full_size_properties_and_reproducibility():
    """BASELINE's image size (3 x 567 x 1008): identities that need no oracle, and bit-reproducibility."""
    from gscream_amd import loss_utils as L
    g = torch.Generator(device="cuda").manual_seed(0)
    y = torch.rand((3, 567, 1008), device="cuda", generator=g)
    assert abs(float(L.ssim(y, y)) - 1.0) < 1e-5 and float(L.l1_loss(y, y)) == 0.0
    x = (y + 0.1 * torch.randn(y.shape, device="cuda", generator=g)).clamp(0, 1).requires_grad_(True)
    a = L.rgb_loss(x, y)
    a.backward()
    g1 = x.grad.clone()
    x.grad = None
    b = L.rgb_loss(x, y)
    b.backward()
    assert float(a) == float(b) and torch.equal(g1, x.grad), "fixed-order reductions: bit-reproducible"
    assert abs(float(L.ssim(x, y)) - float(L.ssim(y, x.detach()))) < 1e-6  # symmetric
    # directional derivative check at full size: L(x + eps d) - L(x - eps d) ~= 2 eps <grad, d>
    d = torch.sign(g1)  # steepest-ascent direction: the derivative along it is sum |grad|, far above fp32 noise
    eps = 1e-3
    with torch.no_grad():
        fd = (float(L.rgb_loss(x + eps * d, y)) - float(L.rgb_loss(x - eps * d, y))) / (2 * eps)
    an = float((g1 * d).sum())
    assert an > 0 and abs(fd - an) < 5e-2 * an, (fd, an)


# ---- depth terms --------------------------------------------------------------------------------------------------
# Gate (tests/loss_helpers.py; proven without a GPU in tests/test_loss_oracle.py): loss and scale within 2e-6, shift within 5e-6
# (relative beyond 1), EVERY pixel of the gradient within 1e-4 of the largest entry -- the inputs are built with every |.| argument
# at least 1e-5 from zero (kink_free), so no sign is float32's to choose -- and exact zeros where the reference has them.
UP = 1.5   # every case runs with a non-unit upstream gradient
SHAPES = LH.SHAPES
_depth_case3 = LH.depth_case3


def _hip(d, y, upstream, lsq, w, g, lambda_l1, lambda_smooth, fg, lambda_fg):
    """gscream_amd.loss_utils.depth_loss as loss_helpers.check_depth_case runs it -> (loss, |scale|, shift, d(upstream loss)/dd)."""
    from gscream_amd import loss_utils as L
    H, W = d.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().reshape(1, H, W)
    x = t(d).requires_grad_(True)
    kw = dict(fg_mask=t(fg), lambda_fg=lambda_fg) if fg is not None else {}
    loss, parts = L.depth_loss(x, t(y), t(lsq), t(w), t(g), lambda_l1, lambda_smooth, return_parts=True, **kw)
    (upstream * loss).backward()
    return float(loss.detach()), float(parts[3]), float(parts[4]), x.grad.cpu().numpy().reshape(H, W).astype(np.float64)


def _check(d, y, cfg, context, seed=0):
    y, terms, _ = LH.kink_free(d, y, **cfg, rng=np.random.default_rng(seed))
    res = LH.check_depth_case(_hip, d, y, cfg, upstream=UP, context=context)
    res.y = y
    return res


@pytest.mark.parametrize("how", ["plain", "masks", "fg"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_depth_loss_shapes_three_ways(H, W, how):
    """Every shape without masks, with three DISTINCT masks (binary fit mask, fractional L1 weight with zeros, another binary
    gradient mask) and as the reference view (fit mask + foreground rectangle, lambda_fg = 99): one pixel, one row, one column, H or
    W below 8 (coarse lattices of one node), 8 / 9 and 16 / 17 (a lattice gains a node), H W = 255 / 256 / 257 (one workgroup, two)
    and 257 x 256 (257 workgroups: the partial totals take a second row).  A picture of one pixel, and of two with the fit mask
    (1, 0), has det = 0: scale = shift = 0.  1x2 without masks is an exact fit, every residual a kink: values only.
    Worst measured on an MI355X over the 56 gated cases, next to the bound: loss 3.5e-7 (2e-6), scale 3.2e-8 (2e-6), shift 5.0e-8
    (5e-6), gradient 4.2e-7 of the largest entry (1e-4), no pixel beyond; kink_free took at most one round."""
    c = LH.depth_case3(H * 100 + W, H, W)
    cfg = LH.case_config(c, how)
    if (H, W, how) == (1, 2, "plain"):
        loss, s, t, grad = _hip(c.d, c.y, UP, **cfg)
        ref_loss, ref_s, ref_t, _ = LO.depth_value_and_grad(c.d, c.y, None, None, None, cfg["lambda_l1"], cfg["lambda_smooth"])
        assert ref_loss < 2e-6 and loss < 2e-6 and np.isfinite(grad).all()
        assert abs(s - ref_s) < 2e-6 * max(1.0, ref_s) and abs(t - ref_t) < 5e-6 * max(1.0, abs(ref_t))
        return
    res = _check(c.d, c.y, cfg, f"{H}x{W} {how}", seed=H * 100 + W)
    if H * W == 1 or (H * W == 2 and how != "plain"):
        assert res.terms.det == 0 and res.ref_s == 0 and res.ref_t == 0 and res.scale == 0 and res.shift == 0


def test_depth_loss_negative_slope():
    """d = -0.6 y + 5 + noise: s0 < 0, so d|s0|/ds0 = -1 in the fit-chain coefficients A, B, C (every other case has s0 > 0).
    Worst measured: loss 7.0e-8 (2e-6), scale 2.0e-8 (2e-6), shift 5.4e-8 (5e-6), gradient 4.4e-7 of the largest entry (1e-4)."""
    for H, W in ((23, 41), (71, 112)):
        c = LH.depth_case3(H + W, H, W, slope=-0.6, offset=5.0)
        for how in ("plain", "masks", "fg"):
            res = _check(c.d, c.y, LH.case_config(c, how), f"negative slope {H}x{W} {how}")
            assert res.terms.s0 < 0 and res.scale > 0.5


def _det32(d, m):
    """det of compute_scale_and_shift as the reference forms it, float32 throughout."""
    D, M = torch.from_numpy(d)[None], torch.from_numpy(m)[None]
    a00, a01, a11 = torch.sum(M * D * D, (1, 2)), torch.sum(M * D, (1, 2)), torch.sum(M, (1, 2))
    return float(a00 * a11 - a01 * a01)


@pytest.mark.parametrize("fit", ["empty", "one_pixel", "two_pixels_of_one_depth"])
@pytest.mark.parametrize("H,W", [(23, 41), (71, 112)])
def test_depth_loss_singular_fit(H, W, fit):
    """det = 0 in the reference's float32 and in float64 (asserted): scale = shift = 0, the loss is lambda_l1 mean(|y| w) plus the
    smooth part of -y, and -- |scale| being zero with derivative zero -- the gradient is exactly zero.  (Until its sums widened before
    multiplying, the kernel had det = the rounding error of a float32 square here and returned scales like 12.3.)
    Worst measured: loss 2.7e-8 (2e-6); scale, shift and every gradient entry exactly 0."""
    c = LH.depth_case3(3 * H + W, H, W)
    m = np.zeros((H, W), np.float32)
    d = c.d.copy()
    if fit != "empty":
        m[H // 2, W // 3] = 1.0
    if fit == "two_pixels_of_one_depth":
        m[H // 3, W // 2] = 1.0
        d[H // 3, W // 2] = d[H // 2, W // 3]
    cfg = dict(LH.case_config(c, "masks"), lsq=m)
    res = _check(d, c.y, cfg, f"singular fit {fit} {H}x{W}")
    assert _det32(d, m) == 0 and res.terms.det == 0 and int(m.sum()) == ("empty", "one_pixel", "two_pixels_of_one_depth").index(fit)
    assert res.ref_s == 0 and res.ref_t == 0 and res.scale == 0 and res.shift == 0, (res.scale, res.shift)
    Z, Y, G = (torch.from_numpy(a.astype(np.float64))[None] for a in (np.zeros_like(res.y), res.y, c.g))
    smooth = sum(0.5 * cfg["lambda_smooth"] * float(LO.gradient_loss(Z[:, ::st, ::st], Y[:, ::st, ::st], G[:, ::st, ::st])) for st in (1, 2, 4, 8))
    want = cfg["lambda_l1"] * float(np.mean(np.abs(res.y.astype(np.float64)) * c.w)) + smooth
    assert abs(res.ref_loss - want) < 1e-9 and abs(res.loss - want) < 2e-6 * max(1.0, want)
    assert not np.any(res.ref_g) and not np.any(res.grad)


def test_depth_loss_gradient_mask_edge_cases():
    """The gradient mask zero on every ::8 lattice node but not elsewhere (M_3 = 0 < M_2: cs[3] = 0, that scale drops out); all zero
    (no smooth term at all); fractional (the kernel multiplies by the mask's values, edge weights g_p g_q); and the L1 weight all zero.
    Worst measured: loss 1.1e-8 (2e-6), scale 1.2e-8 (2e-6), shift 2.7e-8 (5e-6), gradient 1.1e-7 of the largest entry (1e-4)."""
    H, W = 23, 41
    c = LH.depth_case3(77, H, W)
    base = LH.case_config(c, "masks")
    g8 = c.g.copy()
    g8[::8, ::8] = 0.0
    res = _check(c.d, c.y, dict(base, g=g8), "gradient mask zero on the ::8 lattice")
    assert res.terms.Ms[3] == 0 < res.terms.Ms[2]
    res = _check(c.d, c.y, dict(base, g=np.zeros_like(c.g)), "gradient mask all zero")
    assert res.terms.Ms == [0, 0, 0, 0] and res.ref_loss > 0
    frac = (np.random.default_rng(5).random((H, W)) * 1.2 * (c.g > 0)).astype(np.float32)
    res = _check(c.d, c.y, dict(base, g=frac), "fractional gradient mask")
    assert 0 < np.count_nonzero(frac) < frac.size and len(np.unique(frac)) > H * W // 2
    res = _check(c.d, c.y, dict(base, w=np.zeros_like(c.w)), "L1 weight all zero")
    assert res.ref_loss > 0 and np.any(res.ref_g)


def _depth_case(seed, H, W, masked):
    rng = np.random.default_rng(seed)
    y = (rng.random((H, W)) * 5 + 1).astype(np.float32)                      # "midas" target
    d = (0.6 * y + 0.4 + 0.08 * rng.standard_normal((H, W))).astype(np.float32)  # rendered depth: affine + noise
    m = (rng.random((H, W)) > 0.3).astype(np.float32)
    return d, y, m, (m if masked else None)


@pytest.mark.parametrize("H,W,masked,seed", [(71, 112, False, 1), (142, 252, True, 2), (9, 17, True, 3), (1, 33, False, 4), (64, 64, True, 5)])
def test_depth_loss_against_oracle(H, W, masked, seed):
    """compute_scale_and_shift + |scale| + L1 + four-scale gradient loss, value and gradient through the fit; one mask in all three
    places, as train.py:563-573 passes it.  Worst measured: loss 2.5e-8 (2e-6), scale 2.9e-8 (2e-6), shift 2.9e-8 (5e-6),
    gradient 1.2e-7 of the largest entry (1e-4), no pixel beyond."""
    d, y, m, wg = _depth_case(seed, H, W, masked)
    _check(d, y, dict(lsq=m, w=wg, g=wg, lambda_l1=0.7, lambda_smooth=0.4, fg=None, lambda_fg=0.0), f"{H}x{W} masked={masked}", seed=seed)


def test_depth_loss_reference_view_with_foreground_term():
    """The shipped run config (scripts/run.py: refer_depth_lr_fg = 100 > refer_depth_lr = 1) adds
    (fg - lr) * l1_loss_masked(aligned, midas, fg_mask) at train.py:555-557 -- the dominant depth term.
    Worst measured: loss 1.1e-8 (2e-6), scale 1.4e-8, shift 8.1e-9, gradient 1.3e-7 of the largest entry (1e-4), no pixel beyond."""
    H, W = 96, 160
    d, y, m, _ = _depth_case(11, H, W, False)
    fg = np.zeros((H, W), np.float32)
    fg[20:70, 40:120] = 1.0
    cfg = dict(lsq=m, w=None, g=None, lambda_l1=1.0, lambda_smooth=1.0, fg=fg, lambda_fg=99.0)
    res = _check(d, y, cfg, "reference view with the foreground term")
    plain, *_ = LO.depth_value_and_grad(d, y, m, None, None, 1.0, 1.0)
    assert res.ref_loss > 3 * plain, "the foreground term dominates in the shipped configuration"


def test_depth_loss_properties_full_size():
    from gscream_amd import loss_utils as L
    g = torch.Generator(device="cuda").manual_seed(3)
    y = torch.rand((1, 567, 1008), device="cuda", generator=g) * 4 + 1
    exact = (0.5 * y + 2.0)                       # exactly affine: the fit recovers it, every term vanishes
    loss, parts = L.depth_loss(exact, y, None, None, None, 1.0, 1.0, return_parts=True)
    assert float(loss) < 1e-5 and abs(float(parts[3]) - 2.0) < 1e-4 and abs(float(parts[4]) + 4.0) < 1e-3
    d = (exact + 0.05 * torch.randn(y.shape, device="cuda", generator=g)).requires_grad_(True)
    a = L.depth_loss(d, y, None, None, None, 1.0, 0.5)
    a.backward()
    g1 = d.grad.clone()
    d.grad = None
    b = L.depth_loss(d, y, None, None, None, 1.0, 0.5)
    b.backward()
    assert float(a) == float(b) and torch.equal(g1, d.grad), "bit-reproducible"
    # the loss is invariant to an affine change of the input depth (the fit absorbs it): gradient is orthogonal to 1 and d
    assert abs(float(g1.sum())) < 1e-4 * float(g1.abs().sum()) and abs(float((g1 * d.detach()).sum())) < 1e-4 * float((g1.abs() * d.detach().abs()).sum())


@pytest.mark.parametrize("name", sorted(MLG.depth_cases().keys()))
def test_depth_golden(name):
    """The committed vectors (their inputs hold no term within 1e-5 of zero: tests/test_loss_oracle.py): loss and scale within 2e-6
    of the stored values, the stored gradient through assert_depth_grad, no pixel beyond.  Worst measured: gradient 1.1e-7 of the largest entry (1e-4)."""
    c = MLG.depth_cases()[name]
    d, y, m, wg = MLG.make_depth_inputs(c)
    exp = np.load(os.path.join(ROOT, "tests", "golden", "loss_" + name + ".npz"))
    cfg = dict(lsq=m, w=wg, g=wg, lambda_l1=c["l1"], lambda_smooth=c["sm"], fg=None, lambda_fg=0.0)
    terms = LH.depth_terms(d, y, **cfg)
    loss, s, t, grad = _hip(d, y, 1.0, **cfg)
    assert abs(loss - float(exp["loss"])) < 2e-6 and abs(s - float(exp["scale"])) < 2e-6 and abs(t - float(exp["shift"])) < 5e-6
    assert LH.assert_depth_grad(grad, exp["grad"], terms, float(exp["scale"]), context=name) == 0


