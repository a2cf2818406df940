"""GPU parity at training sizes: the kernels around the rasterizer against their fp64 oracles at the sizes where their
persistent / grid-stride code paths run (a wave's second and later groups, the emit kernel's second input buffer, the
count kernel's second pass over the blocks, scans with several block totals per thread, finish loops over more partials
than threads, depth sums past the 512-workgroup cap, a Morton bucket beyond the in-LDS sort).

Tolerances are those of the small-size siblings (tests/test_gpu_decode.py, test_gpu_loss.py, test_gpu_knn.py).  The decode
compares rows by key (tests/helpers.py align_decode_rows): with millions of offsets, a few `tanh(z) > 0` decisions sit
within fp32 rounding of zero.  Each test's docstring records the worst error measured on an MI355X, next to its bound."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers as H  # noqa: E402
from oracle import decode_oracle as DO  # noqa: E402
from oracle import knn_oracle as KO  # noqa: E402
from oracle import loss_oracle as LO  # noqa: E402

pytestmark = pytest.mark.gpu
CAM = [0.3, -0.2, -6.0]
K = 10
NAMES = ("xyz", "color", "opacity", "uncertainty", "scaling", "rot")
WIDTHS = (3, 3, 1, 1, 3, 4)


def _report(what, worst):
    print(f"\n[worst] {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def _cams():
    return (DO.Camera(torch.tensor(CAM, dtype=torch.float64)), DO.Camera(torch.tensor(CAM, dtype=torch.float32, device="cuda")))


def _vis_mask(N, frac, g):
    return None if frac is None else torch.rand(N, generator=g) < frac


def _check_forward(out_d, out_r, al, worst):
    for nm, a, b in zip(NAMES, out_d[:6], out_r[:6]):
        worst[nm] = e = H.max_scaled_err(a.detach().cpu()[al.rows_got], b.detach()[al.rows_ref])
        assert e <= 2e-5, (nm, e)
    worst["neural_opacity"] = e = H.max_scaled_err(out_d[6], out_r[6])
    assert out_d[6].shape == out_r[6].shape and e <= 2e-5, ("neural_opacity", e)
    assert out_d[7].dtype == torch.bool and out_d[0].shape[0] == int(out_d[7].sum())


# ---- decode forward + backward -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,seed,vis,mean", [(20_000, 61, None, 0.0), (200_000, 62, None, 0.0), (200_000, 63, 0.9, 0.0),
                                             (200_000, 64, None, 1.0)])
def test_decode_forward_and_backward_at_scale(N, seed, vis, mean):
    """generate_neural_gaussians against the fp64 oracle, K = 10: all seven outputs and the mask (forward 2e-5), every
    parameter gradient under random upstream gradients on the six outputs (2e-4 of each tensor's largest entry).  N = 20k
    gives a backward wave a second group of 16 anchors; 200k gives every emit wave groups in both input buffers and the
    weight-gradient finish 256 workgroup partials; vis = 0.9 takes the device row list and its count; mean = 1 makes the
    weight-gradient sums grow with N, so a dropped group or partial stands far above the tolerance.  The upstream gradient
    is zero on the ambiguous keys and on every key of an anchor whose hidden ReLU input sits within 1e-5 of zero (a few
    per 100k anchors: fp32 may take the other side of the kink there, as CPU fp32 torch does).
    Worst measured: forward rot 4.3e-6, the others <= 2.3e-7; gradients <= 3.2e-6
    (_anchor_feat; mean 1: <= 1.8e-6); no ambiguous key, 26 / 298 / 225 / 231 kinked anchors."""
    from gscream_amd.neural_gaussians import generate_neural_gaussians
    ref = DO.Model(N, K, seed=seed, dtype=torch.float64)
    dut = copy.deepcopy(ref).float().cuda()
    g = torch.Generator().manual_seed(seed)
    vm = _vis_mask(N, vis, g)
    cam_r, cam_d = _cams()
    seen, unhook = H.record_first_layers(ref)
    out_r = DO.generate_neural_gaussians(cam_r, ref, vm, True)
    unhook()
    out_d = generate_neural_gaussians(cam_d, dut, None if vm is None else vm.cuda(), True)
    Nv = N if vm is None else int(vm.sum())
    assert out_d[7].shape == (Nv * K,) and out_r[7].shape == (Nv * K,)
    al = H.align_decode_rows(out_d[7], out_r[7], out_r[6])
    # anchors with a hidden ReLU input within fp32 rounding of zero: their derivative is ambiguous like a mask bit near zero
    kinked = (torch.cat(seen, 1).abs() <= 1e-5).any(1)
    assert len(seen) == 4 and kinked.shape == (Nv,) and int(kinked.sum()) <= Nv // 200
    worst = {"ambiguous keys": int(al.ambiguous.sum()), "kinked anchors": int(kinked.sum())}
    _check_forward(out_d, out_r, al, worst)
    fields = H.upstream_fields(Nv * K, WIDTHS, al.ambiguous | kinked.repeat_interleave(K), g, mean=mean)
    (sum((o * f[al.keys_ref]).sum() for o, f in zip(out_r[:6], fields))).backward()
    kd = al.keys_got.cuda()
    (sum((o * f.float().cuda()[kd]).sum() for o, f in zip(out_d[:6], fields))).backward()
    pr, pd = dict(ref.named_parameters()), dict(dut.named_parameters())
    for k in pr:
        assert pd[k].grad is not None, k
        worst["grad " + k] = e = H.max_scaled_err(pd[k].grad, pr[k].grad)
        assert e <= 2e-4, ("grad " + k, e)
    _report(f"decode N={N} vis={vis} mean={mean}", worst)


# ---- count and scan past their thresholds ----------------------------------------------------------------------------
@pytest.mark.parametrize("vis", [1.0, 0.9])
def test_decode_count_and_scan_past_thresholds(vis):
    """N = 600 000 anchors, forward only: the count kernel walks its blocks in two passes (> 2048 x 256 anchors), the scans
    (visible rows and per-anchor counts) give each thread several block totals.  neural_opacity, the mask and the outputs
    against the oracle (2e-5), the row count against the oracle's, and the per-anchor first rows of the bookkeeping against
    an exclusive cumulative sum of the oracle's survivor counts (the ambiguous keys' own difference added).
    Worst measured: neural_opacity 7.6e-7, opacity 7.2e-7, rot 3.0e-6, the others <= 1.7e-7; no ambiguous key."""
    from gscream_amd.neural_gaussians import generate_neural_gaussians
    N = 600_000
    ref = DO.Model(N, K, seed=71, dtype=torch.float64)
    dut = copy.deepcopy(ref).float().cuda()
    vm = torch.rand(N, generator=torch.Generator().manual_seed(71)) < vis
    cam_r, cam_d = _cams()
    with torch.no_grad():
        out_r = DO.generate_neural_gaussians(cam_r, ref, vm, True)
        out_d = generate_neural_gaussians(cam_d, dut, vm.cuda(), True)
    Nv = int(vm.sum())
    assert Nv * K == out_r[7].numel() == out_d[7].numel() and Nv > 524_288
    al = H.align_decode_rows(out_d[7], out_r[7], out_r[6])
    worst = {"ambiguous keys": int(al.ambiguous.sum())}
    _check_forward(out_d, out_r, al, worst)
    mg, mr = out_d[7].cpu(), out_r[7]
    flips = (mg.long() - mr.long()).view(Nv, K).sum(1)  # nonzero only on anchors with an ambiguous key
    assert out_d[0].shape[0] == int(mr.sum()) + int(flips.sum()), "row count"
    book = out_d[7]._gsr_decode
    assert book.N == Nv and book.M == out_d[0].shape[0]
    assert torch.equal(book.vis.cpu().long(), torch.nonzero(vm).view(-1)), "visible rows"
    counts = mr.view(Nv, K).sum(1) + flips
    want = torch.cumsum(counts, 0) - counts
    assert torch.equal(book.first.cpu().long(), want), "first output row per anchor"
    _report(f"decode count/scan N={N} vis={vis}", worst)


# ---- training statistics at scale --------------------------------------------------------------------------------
@pytest.mark.parametrize("N,modes", [(200_000, ("copy", "same")), (600_000, ("same",))])
def test_training_statistics_at_scale(N, modes):
    """training_statis after the decode at training size against the restated reference (rtol 1e-6, atol 1e-7).  "copy":
    the visibility mask arrives as another tensor (everything re-derived from the masks); "same": the decode's own mask, so
    its bookkeeping -- row list and first rows from the scans, several block totals per thread at 600k -- is used.  Millions
    of rows cross the kernel's wave edges (an anchor's offsets starting in the previous wave).
    Worst measured: opacity_accum 2.4e-7, offset_gradient_accum 9.5e-7 (abs), the two counters exact."""
    from gscream_amd.densify_stats import training_statis
    from gscream_amd.neural_gaussians import generate_neural_gaussians
    dut = DO.Model(N, K, seed=81, dtype=torch.float32).cuda()
    g = torch.Generator().manual_seed(81)
    mk = lambda dev: types.SimpleNamespace(n_offsets=K, opacity_accum=torch.zeros(N, 1, device=dev), anchor_demon=torch.zeros(N, 1, device=dev),
                                           offset_gradient_accum=torch.zeros(N * K, 1, device=dev), offset_denom=torch.zeros(N * K, 1, device=dev))
    acc_d, acc_r = mk("cuda"), mk("cpu")
    cam_d = DO.Camera(torch.tensor(CAM, device="cuda"))
    for mode in modes:
        vm = torch.rand(N, generator=g) > 0.3
        vmd = vm.cuda()
        with torch.no_grad():
            xyz, *_, nop, mask = generate_neural_gaussians(cam_d, dut, vmd, True)
        M = xyz.shape[0]
        update_filter = torch.rand(M, generator=g) > 0.4
        grad = torch.randn(M, 3, generator=g)
        book = mask._gsr_decode
        assert book.matches(vmd, K) and book.M == M and (N < 600_000 or book.N > 1024 * 256)
        training_statis(acc_d, types.SimpleNamespace(grad=grad.cuda()), nop, update_filter.cuda(), mask, vm.cuda() if mode == "copy" else vmd)
        DO.training_statis(acc_r, types.SimpleNamespace(grad=grad), nop.cpu(), update_filter, mask.cpu(), vm)
    worst = {}
    for name in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom"):
        a, b = getattr(acc_d, name).cpu(), getattr(acc_r, name)
        worst[name] = float((a - b).abs().max())
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-6, atol=1e-7), name
    assert acc_d.anchor_demon.max() == len(modes) and acc_d.offset_denom.sum() > 0
    _report(f"training_statis N={N} {modes}", worst)


# ---- RGB loss at full frame size ---------------------------------------------------------------------------------
def _frame(seed, H_=567, W_=1008):
    rng = np.random.default_rng(seed)
    gt = rng.random((3, H_, W_)).astype(np.float32)
    img = np.clip(gt + 0.1 * rng.standard_normal(gt.shape), 0, 1).astype(np.float32)
    return rng, gt, img


@pytest.mark.parametrize("weighted", [False, True])
def test_rgb_loss_full_frame_against_oracle(weighted):
    """3 x 567 x 1008 (3456 tile partials: more than one per finishing thread) against LO.value_and_grad: loss, L1 and SSIM
    terms within 2e-6 abs, the gradient within 1e-4 of its largest entry.
    Worst measured: unweighted loss 6.8e-9, L1 5.9e-10, SSIM 2.8e-8, gradient 8.8e-7;
    weighted 5.5e-9, 1.8e-9, 9.6e-9, 4.9e-7."""
    from gscream_amd import loss_utils as L
    rng, gt, img = _frame(91 + weighted)
    w = rng.random((1,) + gt.shape[1:]).astype(np.float32) if weighted else None
    ref = LO.value_and_grad(img, gt, w, 0.2, 1.0)
    x = torch.from_numpy(img).cuda().requires_grad_(True)
    loss, l1, ss = L.rgb_loss(x, torch.from_numpy(gt).cuda(), None if w is None else torch.from_numpy(w).cuda(), 0.2, 1.0, return_parts=True)
    loss.backward()
    worst = {}
    for nm, a, b in zip(("loss", "l1", "ssim"), (float(loss.detach()), float(l1), float(ss)), ref[:3]):
        worst[nm] = abs(a - b)
        assert abs(a - b) < 2e-6, (nm, a, b)
    worst["grad"] = float(np.abs(x.grad.cpu().numpy() - ref[3]).max() / np.abs(ref[3]).max())
    assert worst["grad"] <= 1e-4
    _report(f"rgb_loss weighted={weighted}", worst)


def test_rgb_loss_mirrored_functions_full_frame():
    """The trainer's mix of l1_loss, ssim, l1_loss_masked and ssim_masked (train.py:538-545) at 3 x 567 x 1008 against the
    oracle's functions: value within 2e-6 abs, gradient within 1e-4 of its largest entry.
    Worst measured: value 1.1e-8, gradient 4.8e-7 of its largest entry."""
    from gscream_amd import loss_utils as L
    rng, gt, img = _frame(95)
    mask = (rng.random((1,) + gt.shape[1:]) > 0.5).astype(np.float32)
    x = torch.from_numpy(img).cuda().requires_grad_(True)
    y, m = torch.from_numpy(gt).cuda(), torch.from_numpy(mask).cuda()
    total = 0.8 * L.l1_loss(x, y) + 0.2 * (1.0 - L.ssim(x, y)) + 0.5 * (0.8 * L.l1_loss_masked(x, y, m) + 0.2 * (1.0 - L.ssim_masked(x, y, m)))
    total.backward()
    xr = torch.from_numpy(img).double().requires_grad_(True)
    yr, mr = torch.from_numpy(gt).double(), torch.from_numpy(mask).double()
    ref = 0.8 * LO.l1_loss(xr, yr) + 0.2 * (1.0 - LO.ssim(xr, yr)) + 0.5 * (0.8 * LO.l1_loss_masked(xr, yr, mr) + 0.2 * (1.0 - LO.ssim_masked(xr, yr, mr)))
    ref.backward()
    worst = {"value": abs(float(total.detach()) - float(ref.detach())),
             "grad": float((x.grad.cpu().double() - xr.grad).abs().max() / xr.grad.abs().max())}
    assert worst["value"] < 2e-6 and worst["grad"] <= 1e-4, worst
    _report("rgb_loss mirrored mix", worst)


# ---- depth loss past the workgroup cap ---------------------------------------------------------------------------
@pytest.mark.parametrize("H_,W_,masked,fg", [(567, 1008, True, False), (567, 1008, False, True), (256, 512, True, False),
                                             (1, 131_073, False, False), (1, 131_073, True, True)])
def test_depth_loss_past_the_workgroup_cap(H_, W_, masked, fg):
    """Scale-and-shift fit, L1 and four-scale gradient loss (optionally the foreground term of the shipped config) against
    LO.depth_value_and_grad at and past H*W = 512 workgroups x 256 pixels, on inputs with no |.| argument within 1e-5 of zero
    (loss_helpers.kink_free): loss and scale within 2e-6, shift within 5e-6 (relative beyond 1), EVERY pixel of the gradient within
    1e-4 of the largest entry (loss_helpers.assert_depth_grad; no share of the pixels is let off).
    Worst measured: loss 5.1e-8, scale 3.1e-8, shift 3.0e-8, gradient 1.7e-7 of the largest entry, no pixel beyond; kink_free one round."""
    import loss_helpers as LH
    from test_gpu_loss import _hip
    rng = np.random.default_rng(H_ * 7 + W_ + 3 * masked + fg)
    y = (rng.random((H_, W_)) * 5 + 1).astype(np.float32)
    d = (0.6 * y + 0.4 + 0.08 * rng.standard_normal((H_, W_))).astype(np.float32)
    m = (rng.random((H_, W_)) > 0.3).astype(np.float32)
    wg = m if masked else None
    fgm = None
    if fg:
        fgm = np.zeros((H_, W_), np.float32)
        fgm[H_ // 5:(4 * H_) // 5 + 1, W_ // 4:(3 * W_) // 4] = 1.0
    cfg = dict(lsq=m, w=wg, g=wg, lambda_l1=0.7, lambda_smooth=0.4, fg=fgm, lambda_fg=99.0 if fg else 0.0)
    y, terms, rounds = LH.kink_free(d, y, **cfg, rng=rng)
    res = LH.check_depth_case(_hip, d, y, cfg, upstream=1.0, context=f"{H_}x{W_} masked={masked} fg={fg}")
    _report(f"depth_loss {H_}x{W_} masked={masked} fg={fg}", dict(res.err, kink_free_rounds=rounds))


# ---- kNN at one million points -----------------------------------------------------------------------------------
def _cloud(kind, P=1_000_000):
    rng = np.random.default_rng(101 + len(kind))
    if kind == "uniform":
        return (rng.random((P, 3)) * 10).astype(np.float32)
    if kind == "sfm":  # a curved surface with noise, 5 % of its points duplicated exactly
        n = P - P // 20
        uv = rng.random((n, 2))
        s = np.stack([uv[:, 0] * 6, uv[:, 1] * 4, np.sin(uv[:, 0] * 7) + 0.01 * rng.standard_normal(n)], 1)
        return np.concatenate([s, s[rng.integers(0, n, P - n)]]).astype(np.float32)
    # collapsed: 200k points in a ball of radius 1e-3, a uniform background, 8 far outliers that double the bounding box
    ball = rng.standard_normal((200_000, 3))
    ball *= (1e-3 * rng.random((200_000, 1)) ** (1 / 3)) / np.linalg.norm(ball, axis=1, keepdims=True)
    ball += np.array([3.3, 2.2, 1.1])
    far = 16.0 - rng.random((8, 3))
    return np.concatenate([ball, rng.random((P - 200_008, 3)) * 8, far]).astype(np.float32)


@pytest.mark.parametrize("kind", ["uniform", "sfm", "collapsed"])
def test_knn_one_million_points_against_exact(kind):
    """distCUDA2 on 1M points against the exact 3-NN oracle (cKDTree, float64) at 2e-5 relative.  The collapsed cloud puts
    more than 16 384 keys into one 12-bit Morton bucket (checked on the host with the kernel's code), so that bucket is
    ordered by the global sort network.
    Worst measured: uniform 2.0e-7, sfm 1.9e-7, collapsed 2.1e-7 (largest bucket 201 525
    keys).  Before the box bounds and distances shared one rounding sequence (knn.hip gsk_len2), one point of the uniform
    cloud was 5.9e-2 off: its third neighbour sat on the nearest corner of its box, and the box was pruned."""
    from simple_knn._C import distCUDA2
    pts = _cloud(kind)
    counts = H.morton_bucket_counts(pts)
    if kind == "collapsed":
        assert counts.max() > 16_384 and counts.max() >= 200_000, int(counts.max())
    got = distCUDA2(torch.from_numpy(pts).cuda()).cpu().numpy().astype(np.float64)
    ref = KO.mean_dist2(pts)
    assert got.shape == ref.shape
    rel = np.abs(got - ref) / (np.abs(ref) + 1e-30)
    ok = np.abs(got - ref) <= 2e-5 * np.abs(ref) + 1e-12
    _report(f"knn {kind}", {"rel": float(rel[ref > 0].max()), "largest bucket": int(counts.max()), "zero refs": int((ref == 0).sum())})
    assert np.all(ok), float(rel[~ok].max())
