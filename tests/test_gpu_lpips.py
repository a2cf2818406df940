"""GPU tests of the LPIPS path (gscream_amd/csrc/lpips.hip) against the fp64 oracle of tests/lpips_helpers.py.

One layer: the bound per element is the forward error of a K-term fma chain, (K + 2) 2^-24 (sum|w||x| + |b|) with K = 9 Cin --
derived, not measured; ReLU is 1-Lipschitz.

Whole chain: no fixed tolerance.  For each case the test computes the deviation d_ref of the eager fp32 torch statement on the CPU
from the oracle, prints it, and requires of the HIP path   deviation <= 8 max(d_ref, 2^-24 |value|)   for the plain, per-layer and
masked values and the spatial map, each taken as one quantity: deviation = the largest absolute difference over its elements, |value|
= its largest magnitude.  (A quantity, not an element: one element of an fp32 result can land on the oracle by chance, which says
nothing about the error scale of fp32 arithmetic on the case.)  Why 8: an MFMA fma chain is up to 3.5e-7 sum|ab| at K = 4096 against
about 1e-7 for blocked eager sums; the factor leaves about 2x headroom over that ratio."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import arena_helpers as A  # noqa: E402
import lpips_helpers as LH  # noqa: E402
from gscream_amd import lpips as LP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("plain", "layers", "masked", "spatial")


@functools.lru_cache(maxsize=None)
def weights():
    return LH.make_weights(0)


@functools.lru_cache(maxsize=None)
def models():
    """(the model on the CPU, the model on the device), same weights."""
    w = weights()
    return LP.LPIPS(w), LP.LPIPS(tuple([t.to(DEV) for t in group] for group in w))


@functools.lru_cache(maxsize=None)
def case(H, W, B=3):
    """Inputs, the oracle and the eager fp32 statement's results for one shape; computed once, shared, never changed."""
    in0, in1 = LH.make_images(H * 1000 + W, B, H, W)
    mask = LH.make_masks(H * 1000 + W, B, H, W)
    want = LH.lpips_oracle(weights(), in0, in1, mask)
    eager = LP._lpips_torch(models()[0], in0, in1, mask, dtype=torch.float32)
    return in0, in1, mask, want, eager


def hip(in0, in1, mask=None, normalize=False, spatial=True):
    r = LP._run(models()[1], in0.to(DEV), in1.to(DEV), None if mask is None else mask.to(DEV), normalize, spatial=spatial)
    assert LP.last_path == "hip"
    return r


# ---- one layer ----
@pytest.mark.parametrize("hw", [(5, 7), (19, 33)])
@pytest.mark.parametrize("pair", LH.PAIRS)
def test_conv_layer_within_the_fma_chain_bound(pair, hw):
    cin, cout = pair
    g = torch.Generator().manual_seed(cin * 7 + cout + hw[0])
    x = torch.randn((3, cin, *hw), generator=g)
    w = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = 0.05 * torch.randn((cout,), generator=g)
    want, scale = LH.conv_oracle(x, w, b, with_scale=True)
    packed, xd, bd = LP.pack_conv3x3(w).to(DEV), x.to(DEV), b.to(DEV)
    got = LP.conv3x3_relu(xd, packed, bd)
    again = LP.conv3x3_relu(xd, packed, bd)
    torch.cuda.synchronize()
    assert torch.equal(got, again), "two runs on the same inputs differ"
    K = 9 * cin
    bound = (K + 2) * 2.0 ** -24 * scale
    err = (got.cpu().double() - want).abs()
    worst = float((err / bound).max())
    print(f"conv {cin}->{cout} at {hw}: worst error / bound = {worst:.3f}, max abs error {float(err.max()):.3e}")
    assert float((want > 0).double().mean()) > 0.2, "ReLU must leave something to compare"
    assert worst <= 1.0


def test_first_layer_input_steps():
    """Cin = 3 with the normalise and scaling flags: the two steps in fp32 on the pixels inside the image, the padding 0 afterwards."""
    g = torch.Generator().manual_seed(11)
    x = torch.rand((3, 3, 19, 33), generator=g)
    w = torch.randn((64, 3, 3, 3), generator=g) * (2.0 / 27) ** 0.5
    b = 0.05 * torch.randn((64,), generator=g)
    shift, scale = torch.tensor(LH.SHIFT).view(1, 3, 1, 1), torch.tensor(LH.SCALE).view(1, 3, 1, 1)
    packed, bd = LP.pack_conv3x3(w).to(DEV), b.to(DEV)
    for flags, xin in ((LP.SCALING, (x - shift) / scale), (LP.SCALING | LP.NORMALIZE, ((2 * x - 1) - shift) / scale), (LP.NORMALIZE, 2 * x - 1)):
        want, s = LH.conv_oracle(xin, w, b, with_scale=True)  # xin: the same fp32 roundings, one per operation
        got = LP.conv3x3_relu(x.to(DEV), packed, bd, flags)
        assert float(((got.cpu().double() - want).abs() / (29 * 2.0 ** -24 * s)).max()) <= 1.0, flags


# ---- the whole chain ----
@pytest.mark.parametrize("hw", [(16, 16), (37, 53), (44, 140)])
def test_chain_against_the_oracle(hw):
    """16x16: the minimum, the last stage is 1x1 and every tap there is a border.  37x53: odd at several levels (37 -> 18 -> 9 -> 4 -> 2,
    53 -> 26 -> 13 -> 6 -> 3), the pool drops a row and a column, tiles are partial.  44x140: at least two 8x32 output tiles in each
    direction at the first three stages (44x140, 22x70, 11x35), partial ones among them."""
    in0, in1, mask, want, eager = case(*hw)
    got = hip(in0, in1, mask)
    torch.cuda.synchronize()
    failures = []
    for key in KEYS:
        d_ref, d_hip = LH.deviation(eager[key], want[key]), LH.deviation(got[key], want[key])
        value = float(want[key].abs().max())
        allowed = 8 * max(d_ref, 2.0 ** -24 * value)
        print(f"lpips {hw} {key}: |value| {value:.6e}  d_ref {d_ref:.3e}  d_hip {d_hip:.3e}  allowed {allowed:.3e}")
        if not d_hip <= allowed:
            failures.append((key, d_hip, allowed))
    assert not failures, failures
    assert float(want["plain"].min()) > 1e-4, "the pair must differ visibly"


def test_identical_images_and_symmetry():
    in0, in1, mask, _, _ = case(37, 53)
    same = hip(in0, in0.clone(), mask)
    assert not same["plain"].any() and not same["layers"].any() and not same["spatial"].any() and not same["masked"].any()
    ab, ba = hip(in0, in1, mask), hip(in1, in0, mask)
    for key in KEYS:
        assert torch.equal(ab[key], ba[key]), key
    again = hip(in0, in1, mask)
    for key in KEYS:
        assert torch.equal(ab[key], again[key]), f"{key}: two runs differ"


def test_masks():
    in0, in1, mask, _, _ = case(37, 53)
    B, H, W = mask.shape
    none, full = hip(in0, in1, None), hip(in0, in1, torch.ones((H, W), dtype=torch.bool))
    assert torch.equal(none["masked"], full["masked"]) and torch.equal(none["spatial"], full["spatial"])
    mean = none["spatial"].double().mean((1, 2))
    assert LH.deviation(none["masked"], mean) <= 2.0 ** -23 * float(mean.abs().max()), "an all-true mask gives the mean of the spatial map"
    empty = hip(in0, in1, torch.zeros((B, H, W), dtype=torch.bool))
    assert empty["masked"].isnan().all() and torch.equal(empty["plain"], none["plain"])
    per_view = hip(in0, in1, mask)
    assert len(set(per_view["masked"].tolist())) == B
    for b in range(B):  # each view under its own mask, as if it were alone
        alone = hip(in0[b:b + 1], in1[b:b + 1], mask[b])
        assert torch.equal(alone["masked"], per_view["masked"][b:b + 1]) and torch.equal(alone["plain"], per_view["plain"][b:b + 1])
    one_empty = mask.clone()
    one_empty[1] = False
    r = hip(in0, in1, one_empty)
    assert r["masked"].isnan().tolist() == [False, True, False]
    without_map = hip(in0, in1, mask, spatial=False)  # out_spatial = NULL
    assert without_map["spatial"] is None
    assert torch.equal(without_map["plain"], per_view["plain"]) and torch.equal(without_map["masked"], per_view["masked"])


def test_package_call_and_normalize():
    in0, in1, _, want, _ = case(37, 53)
    plain, spatial = models()[1], LP.LPIPS(tuple([t.to(DEV) for t in group] for group in weights()), spatial=True)
    a, b = in0.to(DEV), in1.to(DEV)
    val, layers = plain(a, b, retPerLayer=True)
    assert LP.last_path == "hip" and val.shape == (3, 1, 1, 1) and len(layers) == 5 and layers[4].shape == (3, 1, 1, 1)
    assert spatial(a, b).shape == (3, 1, 37, 53)
    assert LH.deviation(val.reshape(3), want["plain"]) <= 1e-4 * float(want["plain"].max())
    u, v = (a + 1) / 2, (b + 1) / 2
    assert torch.equal(plain(u, v, normalize=True), plain(2 * u - 1, 2 * v - 1))
    with pytest.raises(NotImplementedError):
        spatial(a, b, retPerLayer=True)


def test_lpips_views_never_synchronises_and_joins_evaluate_views(monkeypatch):
    from gscream_amd import metrics as M
    in0, in1, mask, want, _ = case(37, 53)
    model = models()[1]
    a, b, m = ((in0 + 1) / 2).to(DEV), ((in1 + 1) / 2).to(DEV), mask.to(DEV)
    LP.lpips_views(model, a, b, m, core="hip")  # (first use: allocator warm-up)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        plain, masked = LP.lpips_views(model, a, b, m, core="hip")
        small = LP.lpips_views(model, a, b, m, max_workspace_bytes=1, core="hip")  # one view per call
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert LP.last_path == "hip" and plain.shape == (3,) and plain.is_cuda
    assert torch.equal(plain, small[0]) and torch.equal(masked, small[1])
    assert LH.deviation(plain, want["plain"]) <= 1e-4 * float(want["plain"].max())  # (2 ((x+1)/2) - 1 is x to an ulp)
    eight = LP.lpips_views(model, a.repeat(3, 1, 1, 1)[:8], b.repeat(3, 1, 1, 1)[:8], m.repeat(3, 1, 1)[:8])  # the default core from 8 views on
    assert LP.last_path == "hip" and torch.equal(eight[0][:3], plain) and torch.equal(eight[1][3:6], masked)
    monkeypatch.setattr(LP, "HIP_MIN_VIEWS", 1)  # three views through the default core
    masks = [v[None, None].expand(1, 3, -1, -1) for v in m]
    full, per_view = M.evaluate_views(list(a), list(b), masks, ["a", "b", "c"], lpips=model)
    assert LP.last_path == "hip"
    assert list(full) == ["SSIM", "PSNR", "masked SSIM", "masked PSNR", "LPIPS", "masked LPIPS"]
    assert [per_view["LPIPS"][n] for n in "abc"] == plain.tolist() and [per_view["masked LPIPS"][n] for n in "abc"] == masked.tolist()
    assert full["LPIPS"] == plain.cpu().mean().item() and full["masked LPIPS"] == masked.cpu().mean().item()
    four, _ = M.evaluate_views(list(a), list(b), masks, ["a", "b", "c"])
    assert list(four) == ["SSIM", "PSNR", "masked SSIM", "masked PSNR"] and all(four[k] == full[k] for k in four)


# ---- the arena ----
def test_arena(monkeypatch):
    """2 views of 37x53 inside guarded, poisoned buffers: plain, poison 0xA5, poison 0xFF.  Guards intact, every output bit-equal: the
    workspace formula holds, and nothing is read before it is written."""
    in0, in1, mask, _, _ = case(37, 53)
    model = models()[1]
    model.packed(torch.device(DEV))
    runs = {}
    for name, poison in (("plain", None), ("arena_a5", 0xA5), ("arena_ff", 0xFF)):
        if poison is None:
            r = LP._run(model, in0[:2].to(DEV), in1[:2].to(DEV), mask[:2].to(DEV), False, spatial=True)
        else:
            with A.guarded(monkeypatch, 64 << 20, poison, DEV) as (arena, proxy):
                a, b, m = arena.put(in0[:2], "in0"), arena.put(in1[:2], "in1"), arena.put(mask[:2], "mask")
                r = LP._run(model, a, b, m, False, spatial=True)
                layer = LP.conv3x3_relu(a, LP.pack_conv3x3(weights()[0][0]).to(DEV), weights()[1][0].to(DEV), LP.SCALING)
            assert proxy.calls.get("gsr_lpips") == 1 and proxy.calls.get("gsr_conv3x3_relu") == 1
            guarded = {p for fn, p, _ in proxy.guarded if fn == "gsr_lpips"}
            assert guarded == {"workspace", "out_plain", "out_layers", "out_masked", "out_spatial"}, guarded
            r["layer"] = layer
        if poison is None:
            r["layer"] = LP.conv3x3_relu(in0[:2].to(DEV), LP.pack_conv3x3(weights()[0][0]).to(DEV), weights()[1][0].to(DEV), LP.SCALING)
        runs[name] = {k: r[k].cpu() for k in KEYS + ("layer",)}
    A.assert_same_bits(runs, "lpips / 2 views of 37x53")
