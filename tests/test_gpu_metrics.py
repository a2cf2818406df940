"""gscream_amd.metrics on the device: gsr_image_metrics against the fp64 oracle of tests/metrics_helpers.py (the bound on the sums and
its counting there) at the sizes where each part of the kernel can go wrong (tests/metrics_helpers.py CASES: the tile is 16 x 32), with
every kind of mask, both flags, a NaN in one image of a batch, identical images, on a full 567 x 1008 pair, and the launch behaviour
(no host stop, the current stream, identical bits).  The SSIM half is held to the written rule: there is no reference run of it."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.metrics_helpers import CASES, case, metrics_oracle, noise_pair, random_mask, smooth_pair, within_one_ulp  # noqa: E402

from gscream_amd import metrics as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def HIP(monkeypatch):
    """The torch statement made to raise: these tests must run the kernels."""
    def no_fallback(*a, **k):
        raise AssertionError("took the torch path")
    monkeypatch.setattr(M, "_metrics_torch", no_fallback)
    return M


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def rows(m):
    """ImageMetrics -> ([B,8] fp32 metrics, [B,8] fp64 sums) on the host."""
    return torch.stack(list(m[:8]), 1).cpu().numpy(), m.sums.cpu().numpy()


def bits(m):
    return [v.view(torch.int32) if v.dtype == torch.float32 else v.view(torch.int64) for v in m]


def same_bits(a, b):
    return all(torch.equal(x, y) for x, y in zip(bits(a), bits(b)))


def check(m, o, what):
    """The call's result against an oracle run with_bound: metrics to one fp32 ulp, n and n_m exactly, the other sums to the bound."""
    got, sums = rows(m)
    assert got.dtype == np.float32 and got.shape == o["metrics"].shape and sums.dtype == np.float64
    assert np.array_equal(sums[:, [0, 4]], o["sums"][:, [0, 4]])
    dev_, bound = np.abs(sums - o["sums"]), o["sum_bound"]
    cols = [1, 2, 3, 5, 6, 7]
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.nanmax(np.where(bound[:, cols] > 0, dev_[:, cols] / bound[:, cols], 0.0))
    print(f"{what}: sums off by at most {dev_[:, cols].max():.3g} (largest share of the bound {share:.3g}; dssim bound "
          f"{bound[:, 3].max():.3g} on {o['sums'][:, 3].max():.6g}); metrics {got[0].tolist()}")
    assert (dev_[:, cols] <= bound[:, cols]).all(), (dev_, bound)
    ok = within_one_ulp(got, o["metrics"])
    assert ok.all(), (got, o["metrics"])


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_oracle(name, HIP):
    d = case(name)
    p, g = dev(d["pred"]), dev(d["gt"])
    plain = M.image_metrics(p, g)
    assert M.last_path == "hip" and all(v.shape == (p.shape[0],) and v.dtype == torch.float32 for v in plain[:8])
    assert plain.sums.dtype == torch.float64 and plain.sums.shape == (p.shape[0], 8)
    check(plain, d["plain"], f"{name} plain")
    got, sums = rows(plain)
    assert np.array_equal(got[:, :4].view(np.int32), got[:, 4:].view(np.int32)) and np.array_equal(sums[:, :4], sums[:, 4:])
    check(M.image_metrics(p, g, dev(d["mask"])), d["masked"], f"{name} masked")


def test_masks(HIP):
    d = case("past_the_tile")  # B = 3, C = 3, four tiles
    p, g, mask = dev(d["pred"]), dev(d["gt"]), dev(d["mask"])
    want = M.image_metrics(p, g, mask)
    check(want, d["masked"], "a [B,1,H,W] mask")
    expanded = mask.expand(-1, 3, -1, -1)
    assert expanded.stride(1) == 0
    assert same_bits(M.image_metrics(p, g, expanded), want) and same_bits(M.image_metrics(p, g, expanded.contiguous()), want)
    one = mask[:1].expand(1, 3, -1, -1)  # evaluate()'s [1,3,H,W]
    single = M.image_metrics(p[:1], g[:1], one)
    assert same_bits(single, [v[:1] for v in want]) and same_bits(M.image_metrics(p[0], g[0], mask[0, 0]), single)
    per_channel = random_mask(d["pred"].shape, 77)
    check(M.image_metrics(p, g, dev(per_channel)), metrics_oracle(d["pred"], d["gt"], per_channel, with_bound=True), "a per-channel mask")
    plain = M.image_metrics(p, g)
    full = M.image_metrics(p, g, torch.ones_like(mask))
    assert same_bits(full, plain) and same_bits(full[4:8], plain[:4])
    empty = M.image_metrics(p, g, torch.zeros_like(mask))
    assert same_bits(empty[:4], plain[:4]) and all(torch.isnan(v).all() for v in empty[4:8])
    assert torch.equal(empty.sums[:, :4], plain.sums[:, :4]) and (empty.sums[:, 4:] == 0).all()


def test_a_nan_stays_in_its_image(HIP):
    d = case("past_the_tile")
    bad = np.array(d["pred"])
    bad[0, 1, 5, 7] = np.nan
    p, g, mask = dev(bad), dev(d["gt"]), dev(d["mask"])
    m = M.image_metrics(p, g, mask)
    assert all(torch.isnan(v[0]) for v in m[:4])
    for b in (1, 2):
        assert same_bits([v[b:b + 1] for v in m], M.image_metrics(p[b:b + 1], g[b:b + 1], mask[b:b + 1]))
    # outside the mask, the NaN reaches the masked entries only through the windows that hold it
    away = np.ones(d["mask"].shape, bool)
    away[:, :, :, 4:] = False
    got, _ = rows(M.image_metrics(p, g, dev(away)))
    o = metrics_oracle(bad, d["gt"], away)
    assert np.isnan(got[0, :4]).all() and np.isfinite(got[0, 4:]).all() and within_one_ulp(got, o["metrics"]).all()


def test_flags(HIP):
    """Inputs outside [0, 1], the tie values (k + 0.5) / 255 and their fp32 neighbours."""
    ties = (np.arange(255, dtype=np.float32) + np.float32(0.5)) / np.float32(255)
    rng = np.random.default_rng(12)
    x = np.concatenate([ties, np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(1)),
                        (rng.random(3 * 19 * 41 - 765, dtype=np.float32) * 1.6 - 0.3).astype(np.float32)])
    x = rng.permutation(x).astype(np.float32).reshape(1, 3, 19, 41)
    y = (rng.random(x.shape, dtype=np.float32) * 1.6 - 0.3).astype(np.float32)
    mask = random_mask((1, 1, 19, 41), 5)
    for clamp, quantize in ((True, False), (False, True), (True, True)):
        m = M.image_metrics(dev(x), dev(y), dev(mask), clamp=clamp, quantize=quantize)
        check(m, metrics_oracle(x, y, mask, clamp=clamp, quantize=quantize, with_bound=True), f"clamp={clamp} quantize={quantize}")
    plain, _ = rows(M.image_metrics(dev(x), dev(y)))
    clamped, _ = rows(M.image_metrics(dev(x), dev(y), clamp=True))
    assert (plain[:, :3] != clamped[:, :3]).all()


def test_identical_images(HIP):
    _, gt = smooth_pair(37, 53, c=3, b=2, seed=6)
    m = M.image_metrics(dev(gt), dev(gt))
    got, sums = rows(m)
    assert (got[:, [0, 1, 4, 5]] == 0).all() and (sums[:, [1, 2, 5, 6]] == 0).all()
    assert np.isposinf(got[:, [2, 6]]).all()
    o = metrics_oracle(gt, gt, with_bound=True)
    check(m, o, "identical images")
    assert (got[:, 3] > 0.99999).all()


def test_repeated_calls_give_identical_bits(HIP):
    d = case("37x53")
    p, g, mask = dev(d["pred"]), dev(d["gt"]), dev(d["mask"])
    out = [[v.clone() for v in M.image_metrics(p, g, mask, clamp=True)] for _ in range(3)]
    assert same_bits(out[0], out[1]) and same_bits(out[0], out[2])


def test_the_calls_do_not_stop_the_host(HIP):
    d = case("past_the_tile")
    p, g, mask = dev(d["pred"]), dev(d["gt"]), dev(d["mask"])
    M.image_metrics(p, g, mask)  # library loading and first allocations out of the way
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m = M.image_metrics(p, g, mask.expand(-1, 3, -1, -1), quantize=True)
        a = M.psnr(p[:1], g[:1], mask[:1].expand(1, 3, -1, -1))
        b = M.my_ssim(p[0], g[0])
        c = M.mse(p[:1], g[:1])
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert M.last_path == "hip" and m.psnr.shape == (3,) and a.dim() == b.dim() == c.dim() == 0


def test_the_current_stream_is_honoured(HIP):
    """On a side stream, behind a delay and the copy that fills the input: a launch on any other stream would read the zeros."""
    d = case("past_the_tile")
    p, g, mask = dev(d["pred"]), dev(d["gt"]), dev(d["mask"])
    want = M.image_metrics(p, g, mask)
    staged = torch.zeros_like(p)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda._sleep(20_000_000)
        staged.copy_(p)
        got = M.image_metrics(staged, g, mask)
    st.synchronize()
    assert M.last_path == "hip" and same_bits(got, want) and float(want.mse.min()) > 0


def test_a_full_size_pair(HIP):
    """B = 2, 3 x 567 x 1008 (1152 tiles a plane, 14 partials a finish thread) against the scipy oracle."""
    pred, gt = smooth_pair(567, 1008, c=3, b=2, seed=13)
    mask = random_mask((2, 1, 567, 1008), 13)
    m = M.image_metrics(dev(pred), dev(gt), dev(mask).expand(-1, 3, -1, -1))
    assert M.last_path == "hip"
    check(m, metrics_oracle(pred, gt, mask, with_bound=True), "567x1008")


def test_a_mask_batch_stride_past_2_to_the_31(HIP):
    """The second image's mask lies 2^31 bytes behind the first's in one buffer (a [2,C,H,W] view with batch stride 2^31): the byte
    offset b * stride_b does not fit 32 bits.  The result equals the dense mask's bit for bit."""
    d = case("past_the_tile")
    p, g = dev(d["pred"][:2]), dev(d["gt"][:2])
    _, C, H, W = p.shape
    dense = dev(random_mask((2, C, H, W), 31))
    store = torch.zeros(2 ** 31 + C * H * W, dtype=torch.bool, device=DEV)
    far = store.as_strided((2, C, H, W), (2 ** 31, H * W, W, 1))
    far.copy_(dense)
    assert far.stride(0) == 2 ** 31 and far.data_ptr() == store.data_ptr()
    got = M.image_metrics(p, g, far)
    assert M.last_path == "hip" and same_bits(got, M.image_metrics(p, g, dense))
    assert not torch.equal(got.sums[0, 4:], got.sums[1, 4:]) and (got.sums[:, 4] > 0).all()


def test_the_drop_ins_and_what_goes_to_torch():
    d = case("37x53")
    p, g = dev(d["pred"]), dev(d["gt"])
    mask = dev(d["mask"]).expand(1, 3, -1, -1)
    m = M.image_metrics(p, g, mask)
    assert M.last_path == "hip"
    for fn, plain, masked in ((M.mse, m.mse, m.mse_masked), (M.psnr, m.psnr, m.psnr_masked), (M.my_ssim, m.ssim, m.ssim_masked)):
        a, b = fn(p, g), fn(p, g, mask)
        assert M.last_path == "hip" and a.dim() == 0 and a.is_cuda
        assert same_bits([a, b], [plain[0], masked[0]])
    # a batch: the reference's mean over all of it, from the images' sums
    b3 = case("past_the_tile")
    total = b3["masked"]["sums"].sum(0)
    bp, bg, bm = dev(b3["pred"]), dev(b3["gt"]), dev(b3["mask"]).expand(-1, 3, -1, -1)
    assert within_one_ulp(M.psnr(bp, bg, bm).cpu().numpy(), -10 * np.log10(total[6] / total[4])) and M.last_path == "hip"
    assert within_one_ulp(M.my_ssim(bp, bg).cpu().numpy(), 1 - 2 * total[3] / total[0]) and M.last_path == "hip"
    # a mask whose rows would broadcast is refused before anything is launched
    with pytest.raises(ValueError):
        M.image_metrics(bp, bg, bm[:1, :1, :1])
    pred, gt = smooth_pair(20, 35, c=3, b=4, seed=2)
    masks = [dev(random_mask((1, 1, 20, 35), k)).expand(1, 3, -1, -1) for k in range(4)]
    full, per_view = M.evaluate_views([dev(pred[k]) for k in range(4)], [dev(gt[k])[None] for k in range(4)], masks, list("abcd"))
    assert M.last_path == "hip"
    q = M.image_metrics(dev(pred), dev(gt), torch.cat([k[:, :1] for k in masks]), quantize=True)
    for key, field in (("SSIM", q.ssim), ("PSNR", q.psnr), ("masked SSIM", q.ssim_masked), ("masked PSNR", q.psnr_masked)):
        assert list(per_view[key].values()) == field.tolist() and list(per_view[key]) == list("abcd")
        assert full[key] == field.cpu().mean().item()
    # what the HIP path does not take
    o = d["masked"]["metrics"]
    for args in ((p.double(), g.double(), mask), (p.cpu(), g.cpu(), mask.cpu()), (p[..., ::2], g[..., ::2], None)):
        r = M.image_metrics(*args)
        assert M.last_path == "torch"
        if args[2] is not None:
            assert within_one_ulp(torch.stack(list(r[:8]), 1).cpu().numpy(), o).all()
    M.force_torch = True
    try:
        r = M.image_metrics(p, g, mask)
        assert M.last_path == "torch" and within_one_ulp(torch.stack(list(r[:8]), 1).cpu().numpy(), o).all()
    finally:
        M.force_torch = False
    # more planes than one call takes: two calls, the same rows
    noise, other = noise_pair(3, 3, c=1, b=65535 + 7, seed=3)
    many = M.image_metrics(dev(noise), dev(other))
    assert M.last_path == "hip"
    tail = M.image_metrics(dev(noise[-9:]), dev(other[-9:]))
    assert same_bits([v[-9:] for v in many], tail)
