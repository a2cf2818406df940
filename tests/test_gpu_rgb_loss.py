"""GPU tests of the fused RGB loss (gscream_amd.loss_utils -> gsr_rgb_loss_*; gscream_amd/csrc/loss.hip) on STRUCTURED frames: flat,
saturated, equal and smooth regions, a block of zero weight, shapes below the 11-tap window and around the 32 x 16 tile, every window
size.  Each region of the gradient is held to its own scale, the bound taken from the error of the reference's own float32 arithmetic
there (tests/rgb_loss_helpers.py; the gate is proven on the CPU, fault by fault, in tests/test_rgb_loss_gate.py).
tests/test_gpu_loss.py keeps the white-noise cases and their rule.  Every case: upstream gradient 1.5, lambda 0.2."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgb_loss_helpers as R  # noqa: E402

pytestmark = pytest.mark.gpu
H, W = 64, 96
KINDS = ["none", "fractional", "object"]


@functools.lru_cache(maxsize=None)
def _reference(seed, kind, unclipped=False):
    """One structured frame with its float64 oracle and eager float32 gradient, computed once on the CPU and never written to."""
    img, gt, region = R.structured_frame(seed, H, W, unclipped)
    w = R.weights(kind, seed, H, W)
    loss, g64, sm, ad = R.oracle(img, gt, w, R.LAM, 11, torch.float64, R.UP)
    g32 = R.oracle(img, gt, w, R.LAM, 11, torch.float32, R.UP)[1]
    one = 1.0 if w is None else w.astype(np.float64)
    parts = (loss, float((ad * one).mean()), float((sm * one).mean()))
    for a in (img, gt, region, g64, g32) + (() if w is None else (w,)):
        a.setflags(write=False)
    return img, gt, region, w, parts, g64, g32


def _cuda(a):
    return None if a is None else torch.tensor(np.asarray(a)).cuda()


def _run(img, gt, w):
    """L.rgb_loss with its parts, backward of 1.5 times the loss -> ((loss, L1 part, SSIM part), gradient as numpy)."""
    from gscream_amd import loss_utils as L
    x = _cuda(img).requires_grad_(True)
    loss, l1, ss = L.rgb_loss(x, _cuda(gt), _cuda(w), R.LAM, 1.0, return_parts=True)
    (R.UP * loss).backward()
    assert x.grad.shape == x.shape
    return (float(loss.detach()), float(l1), float(ss)), x.grad.cpu().numpy()


CASES = [(k, s, False) for k in KINDS for s in (1, 2, 3)] + [("fractional", 2, True)]


@pytest.mark.parametrize("kind,seed,unclipped", CASES)
def test_structured_frame_each_region_on_its_own_scale(kind, seed, unclipped):
    """The gradient of L.rgb_loss on the structured frame, without a weight, with a fractional one and with the binary object mask;
    one case with the rendered side left outside [0, 1].  Every region within 4 times eager float32's own error there (region_gate),
    and eager's error, not the floor, sets the bound in every region.  The values of the same runs are held to 2e-6 in
    test_structured_frame_values_within_2e_6, so that a miss there does not hide this result.
    Worst measured on an MI355X over the 10 cases: ratio 0.92 of the allowed 4 (fractional weight, seed 2, white == white; 0.89 in
    black == black of seed 3): the kernel's error is below eager's in every region.  Of the largest entry of the whole tensor the
    kernel is off by 2.0e-5 ... 3.1e-5 and eager by 7.0e-5 ... 9.4e-5, both in white == white.  (With the forward filter in float32,
    as it was until these tests, the worst ratio was 1.25.)"""
    img, gt, region, w, parts, g64, g32 = _reference(seed, kind, unclipped)
    got, grad = _run(img, gt, w)
    print(f"\n[gradient] {kind} seed {seed} unclipped {unclipped}: {R.relative_error(grad, g64):.3g} of the largest entry, eager "
          f"{R.relative_error(g32, g64):.3g}")
    worst = R.region_gate(grad, g32, g64, region, f"{kind} seed {seed} unclipped {unclipped}")
    print(f"[worst region ratio] {worst:.3g}")
    assert worst <= R.FACTOR


@pytest.mark.parametrize("kind,seed,unclipped", CASES)
def test_structured_frame_values_within_2e_6(kind, seed, unclipped):
    """Loss, L1 part and SSIM part of the same ten runs within 2e-6 of the float64 oracle, tests/test_gpu_loss.py's bound.
    Worst measured on an MI355X: loss 7.2e-9, L1 part 2.8e-9, SSIM part 4.8e-8.
    These frames are why gsl_forward_kernel filters in float64.  With a float32 filter the SSIM part was off by 7.38e-6 ... 7.56e-6
    without a weight and with the object mask and by 3.57e-6 ... 3.76e-6 with the fractional weight, the loss by up to 1.51e-6.  In
    the two-flats region (img 0.25, gt 0.75) the variances are exactly 0 and D = (E[x^2 + y^2] - mu1^2 - mu2^2) + C2 is the
    difference of numbers near 0.625 over C2 = 9e-4: three ulps of 0.625 are 2e-4 of D.  Every pixel of a flat region holds the same
    data, so every pixel makes the SAME rounding error and the mean does not average it away, as it does on white noise: the
    region's mean SSIM was off by 8.3e-5, on a tenth of the frame.  The reference's own eager float32 has the same defect, 5.0e-6 ...
    5.5e-6 on these frames (tests/test_rgb_loss_gate.py asserts that on the CPU).  Second moments about the tile's mean, tried in the
    restatement, also bring the SSIM part to 1e-7, but black == black then fails region_gate by a factor of 130 ... 400 (its zeros
    are no longer exact) and values under a zero weight reach their tile's other pixels (test_zero_weight_block_gets_exact_zeros)."""
    img, gt, region, w, parts, g64, g32 = _reference(seed, kind, unclipped)
    got, _ = _run(img, gt, w)
    errors = [abs(a - b) for a, b in zip(got, parts)]
    print(f"\n[values] {kind} seed {seed} unclipped {unclipped}: loss {errors[0]:.3g}, L1 {errors[1]:.3g}, SSIM {errors[2]:.3g} (2e-6)")
    assert max(errors) < 2e-6, (errors, got, parts)


def _means(img, gt, indicator):
    from gscream_amd import loss_utils as L
    x, y, m = _cuda(img), _cuda(gt), _cuda(indicator)
    return float(L.ssim_masked(x, y, m)), float(L.l1_loss_masked(x, y, m))


def test_region_means_of_the_forward_map():
    """The kernel reduces its SSIM and |img - gt| maps before anyone sees them; ssim_masked and l1_loss_masked with a region's
    indicator as the mask read them region by region.  Each region's mean within 4 times the largest per-pixel error of the eager
    float32 map in that region (exactly 0 for the L1 mean of the three equal regions).
    Worst measured on an MI355X: ratio 0.27 of the allowed 4 (the L1 mean of near white, off by 3.2e-11 where eager's map is exact
    and the floor 2^-24 max|map| sets the bound); the SSIM means at most 0.037 (the two flats off by 4.4e-7, eager's worst pixel
    there 2.1e-4 -- 8.3e-5 with the float32 filter); the L1 means of the equal regions exactly 0."""
    for seed, unclipped in ((1, False), (2, True)):
        img, gt, region = R.structured_frame(seed, H, W, unclipped)
        worst = R.region_means_gate(_means, img, gt, region, context=f"seed {seed} unclipped {unclipped}")
        print(f"[worst region mean ratio] {worst:.3g}")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_zero_weight_block_gets_exact_zeros(seed):
    """The object mask: every pixel at least 5 px inside the zero rectangle has gradient == 0, the rest is held to region_gate.  Run
    again with the images inside that interior replaced by other finite values, the loss and the gradient everywhere else are the
    same bits: nothing leaks out of a masked region.
    Worst measured on an MI355X: 0 nonzero entries among the 504 x 3 of the interior in both runs, bit-identical outside; region
    ratios 0.73, 0.70, 0.54 of the allowed 4."""
    img, gt, region, w, parts, g64, g32 = _reference(seed, "object")
    inside = R.block_interior(seed, H, W)
    got, grad = _run(img, gt, w)
    assert not g64[:, inside].any() and not g32[:, inside].any()
    nonzero = np.count_nonzero(grad[:, inside])
    print(f"\n[zero block] seed {seed}: {inside.sum()} interior pixels, {nonzero} nonzero gradient entries among them")
    assert nonzero == 0
    worst = R.region_gate(grad, g32, g64, np.where(inside, -1, region), f"object seed {seed}, outside the block's interior")
    print(f"[worst region ratio] {worst:.3g}")
    rng = np.random.default_rng(seed)
    img2, gt2 = img.copy(), gt.copy()
    img2[:, inside] = rng.uniform(-3, 8, img2[:, inside].shape).astype(np.float32)
    gt2[:, inside] = rng.uniform(-3, 8, gt2[:, inside].shape).astype(np.float32)
    got2, grad2 = _run(img2, gt2, w)
    assert got2 == got and not grad2[:, inside].any()
    assert np.array_equal(grad2[:, ~inside].view(np.uint32), grad[:, ~inside].view(np.uint32))


@pytest.mark.parametrize("ws", R.WINDOWS)
def test_small_shapes_and_windows(ws):
    """(1 - lambda) l1_loss_masked + lambda (1 - ssim_masked(window_size=ws)) with a fractional weight at twelve shapes: one pixel, one
    row, one column, below the window, around the 32 x 16 tile (15 x 31, 16 x 32, 17 x 33), C = 1 ... 4.  pooled_gate per window size;
    every case alone finite, of the input's shape and within the old 1e-4 of its largest entry, so none hides in the pool.
    Worst measured on an MI355X: pooled ratios 0.39, 0.52, 0.61, 0.42, 0.34 of the allowed 4 for windows 3, 5, 7, 9, 11; a single case
    at most 2.8e-7 of its largest entry (1e-4), the composed loss within 1.7e-8 (3e-6, the bound of
    test_mirrored_functions_and_upstream_gradient)."""
    from gscream_amd import loss_utils as L
    cases = []
    for C, H_, W_ in R.SMALL_SHAPES:
        img, gt, w = R.small_case(0, C, H_, W_)
        x, y, m = _cuda(img).requires_grad_(True), _cuda(gt), _cuda(w)
        loss = (1.0 - R.LAM) * L.l1_loss_masked(x, y, m) + R.LAM * (1.0 - L.ssim_masked(x, y, m, window_size=ws))
        (R.UP * loss).backward()
        grad = x.grad.cpu().numpy()
        ref_loss, g64, _, _ = R.oracle(img, gt, w, R.LAM, ws, torch.float64, R.UP)
        g32 = R.oracle(img, gt, w, R.LAM, ws, torch.float32, R.UP)[1]
        e = R.relative_error(grad, g64)
        print(f"\n[small] window {ws} shape {(C, H_, W_)}: loss {abs(float(loss.detach()) - ref_loss):.3g}, gradient {e:.3g} of the largest entry, "
              f"eager {R.relative_error(g32, g64):.3g}")
        assert grad.shape == (C, H_, W_) and np.isfinite(grad).all() and e <= R.OLD_RULE, (ws, C, H_, W_, e)
        assert abs(float(loss.detach()) - ref_loss) < 3e-6, (ws, C, H_, W_)
        cases.append((ws, grad, g32, g64))
    ratios = R.pooled_gate(cases)
    assert list(ratios) == [ws]


def test_layouts_give_the_same_bits():
    """The structured frame as [C,H,W], as [1,C,H,W] and as a non-contiguous permute(2,0,1) view of an HWC tensor; the fractional weight
    as [1,H,W] and [H,W]; the object mask as float32 and as bool.  Within one weight, every way gives the same bits of loss and gradient,
    and the gradient has the shape of what was passed in.
    Measured on an MI355X: all 18 combinations bit-identical to the [C,H,W] run."""
    from gscream_amd import loss_utils as L
    img, gt, _ = R.structured_frame(1, H, W)
    x0, y0 = _cuda(img), _cuda(gt)

    def run(layout, weight):
        if layout == "chw":
            leaf = x0.clone().requires_grad_(True)
            x, y, back = leaf, y0, lambda g: g
        elif layout == "1chw":
            leaf = x0.clone()[None].requires_grad_(True)
            x, y, back = leaf, y0[None], lambda g: g[0]
        else:
            leaf = x0.permute(1, 2, 0).contiguous().requires_grad_(True)
            x, y, back = leaf.permute(2, 0, 1), y0.permute(1, 2, 0).contiguous().permute(2, 0, 1), lambda g: g.permute(2, 0, 1)
            assert not x.is_contiguous() and not y.is_contiguous()
        loss = L.rgb_loss(x, y, weight, R.LAM)
        (R.UP * loss).backward()
        assert leaf.grad.shape == leaf.shape
        return loss.detach(), back(leaf.grad)

    frac, obj = _cuda(R.weights("fractional", 1, H, W)), _cuda(R.weights("object", 1, H, W))
    for name, ways in (("none", [None]), ("fractional", [frac, frac[0]]), ("object", [obj, obj.bool(), obj[0].bool()])):
        base = run("chw", ways[0])
        assert torch.isfinite(base[1]).all() and base[1].abs().max() > 0
        for layout in ("chw", "1chw", "hwc view"):
            for i, weight in enumerate(ways):
                loss, grad = run(layout, weight)
                assert torch.equal(loss, base[0]) and torch.equal(grad, base[1]), (name, layout, i)
