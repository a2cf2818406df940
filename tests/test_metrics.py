"""gscream_amd.metrics without a GPU: the fp64 oracle the GPU tests measure against (tests/metrics_helpers.py), that its inputs tell
a wrong halo from a right one, the module's torch path, the stored run of the reference's mse / psnr, the PNG round trip, the edge
semantics, the drop-ins, evaluate_views, and the argument checks of gsr_image_metrics.

The SSIM half has no stored reference run: my_ssim is kornia's metrics.ssim and kornia is not on this stack, so these tests hold it
to the written rule alone."""
import inspect
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.metrics_helpers import (CASES, TILE_H, TILE_W, case, dssim_map, metrics_oracle, random_mask, smooth_pair,  # noqa: E402
                                   transform, within_one_ulp)

GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_metrics.npz")
STORED = {"tiny": (3, 3), "wide": (3, 70), "tall": (70, 3), "smooth": (37, 53), "noise": (37, 53)}


def t(a):
    return torch.from_numpy(np.array(a))


def test_the_loop_and_scipy_forms_of_the_oracle_agree_on_3x3():
    d = case("3x3")
    a = metrics_oracle(d["pred"], d["gt"], d["mask"], loop=True)
    dev = np.abs(a["dssim"] - d["masked"]["dssim"]).max()
    print(f"3x3: explicit loop against scipy correlate(mode='mirror'), max per map pixel {dev:.3g}")
    assert dev <= 1e-12
    assert np.abs(a["sums"] - d["masked"]["sums"]).max() <= 1e-11
    x = (np.arange(15, dtype=np.float32) / 16).reshape(1, 1, 3, 5)  # and on a ramp, where every padding rule gives another value
    y = x[..., ::-1].copy()
    assert np.abs(dssim_map(x, y, loop=True) - dssim_map(x, y)).max() <= 1e-12


@pytest.mark.parametrize("name", ["37x53", "3x3"])
def test_the_inputs_tell_a_wrong_halo_from_a_right_one(name):
    """The mean over the image moves by more than 1e-3 (the GPU tests hold it to one fp32 ulp) under each of the three other padding rules.
    That shift is a sum of per-pixel shifts of either sign and varies by draw (2e-4 .. 3e-3 over ten draws at 37x53 for 'reflect');
    the draw fixed in CASES is the one the GPU tests use, and this shows that it separates.  Per map pixel the shift is > 1e-2."""
    d = case(name)
    want = d["plain"]
    for mode in ("reflect", "nearest", "constant"):
        o = metrics_oracle(d["pred"], d["gt"], mode=mode)
        moved = abs(o["metrics"][0, 3] - want["metrics"][0, 3])
        print(f"{name} padding {mode}: ssim moves by {moved:.3g}, per map pixel by up to {np.abs(o['dssim'] - want['dssim']).max():.3g}")
        assert moved > 1e-3 and np.abs(o["dssim"] - want["dssim"]).max() > 1e-2


@pytest.mark.parametrize("name", list(CASES))
def test_the_torch_path_on_cpu_tensors_equals_the_oracle(name):
    from gscream_amd import metrics as M
    d = case(name)
    for mask, key in ((None, "plain"), (d["mask"], "masked")):
        m = M.image_metrics(t(d["pred"]), t(d["gt"]), None if mask is None else t(mask))
        assert M.last_path == "torch"
        got = np.stack([getattr(m, f).numpy() for f in M.FIELDS], 1)
        o = d[key]
        assert got.dtype == np.float32 and got.shape == o["metrics"].shape and m.sums.dtype == torch.float64
        assert within_one_ulp(got, o["metrics"]).all(), (got, o["metrics"])
        assert np.array_equal(m.sums.numpy()[:, [0, 4]], o["sums"][:, [0, 4]])
        if mask is None:
            assert np.array_equal(got[:, :4], got[:, 4:])


def test_mask_shapes_and_a_stride_0_channel_dimension():
    from gscream_amd import metrics as M
    d = case("past_the_tile")
    p, g, mask = t(d["pred"]), t(d["gt"]), t(d["mask"])
    want = M.image_metrics(p, g, mask)
    for m in (mask.expand(-1, 3, -1, -1), mask.expand(-1, 3, -1, -1).contiguous()):
        got = M.image_metrics(p, g, m)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    one = M.image_metrics(p[0], g[0], mask[0, 0])          # [C,H,W] images, an [H,W] mask
    also = M.image_metrics(p[0], g[0], mask[0])            # [1,H,W]
    assert all(torch.equal(a, b[:1]) and torch.equal(a, c) for a, b, c in zip(one, want, also))
    with pytest.raises(TypeError):
        M.image_metrics(p, g, mask.float())
    with pytest.raises(ValueError):
        M.image_metrics(p, g, mask[:, :, :-1])
    with pytest.raises(ValueError):
        M.image_metrics(p, g[:, :2])


@pytest.mark.parametrize("name", list(STORED))
def test_mse_and_psnr_against_the_stored_reference_run(name):
    """The reference's fp32 results are off the fp64 oracle by its own fp32 summation error; the product is held to be no further off."""
    from gscream_amd import metrics as M
    z = np.load(GOLDEN)
    assert tuple(z["cases"]) == tuple(STORED)
    pred, gt, mask = z[f"{name}/pred"], z[f"{name}/gt"], z[f"{name}/mask"]
    assert pred.shape == (1, 3) + STORED[name] and pred.dtype == np.float32 and mask.shape == (1, 1) + STORED[name] and mask.dtype == bool
    o = metrics_oracle(pred, gt, mask)["metrics"][0]
    m = M.image_metrics(t(pred), t(gt), t(mask).expand(1, 3, -1, -1))
    assert M.last_path == "torch"
    for field, column in (("mse", 1), ("psnr", 2), ("mse_masked", 5), ("psnr_masked", 6)):
        ref, got = float(z[f"{name}/{field}"]), float(getattr(m, field)[0])
        ref_off, got_off = abs(ref - o[column]), abs(got - o[column])
        print(f"{name} {field}: reference {ref!r} is {ref_off:.3g} off the oracle, the torch path {got!r} is {got_off:.3g} off")
        assert got_off <= ref_off
        # and the drop-in under the reference's name returns that field
        fn, mk = getattr(M, field.split("_")[0]), (t(mask).expand(1, 3, -1, -1) if field.endswith("masked") else None)
        assert float(fn(t(pred), t(gt), mk)) == got


def test_quantize_is_the_png_round_trip():
    """save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8), written as PNG, read back and divided by 255 as to_tensor does."""
    from PIL import Image

    from gscream_amd import metrics as M
    ties = (np.arange(255, dtype=np.float32) + np.float32(0.5)) / np.float32(255)  # the 255 values (k + 0.5) / 255
    rng = np.random.default_rng(5)
    x = np.concatenate([ties, np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(1)),
                        rng.random(1245, dtype=np.float32), np.float32([-0.3, 0.0, 1.0, 1.7, -0.0, 1e-9])])[:2016]
    x = x.astype(np.float32).reshape(1, 3, 24, 28)
    u8 = np.clip(x * np.float32(255) + np.float32(0.5), 0, 255).astype(np.uint8)  # .to(uint8) truncates
    buf = io.BytesIO()
    Image.fromarray(u8[0].transpose(1, 2, 0)).save(buf, format="PNG")
    back = np.asarray(Image.open(io.BytesIO(buf.getvalue()))).transpose(2, 0, 1)[None]
    assert np.array_equal(back, u8)
    want = (torch.from_numpy(back.copy()).to(torch.float32) / 255).numpy()
    assert np.array_equal(transform(x, quantize=True).view(np.int32), want.view(np.int32))
    assert np.array_equal(M._transform_torch(t(x), False, True).numpy().view(np.int32), want.view(np.int32))
    # so quantize=True on the floats equals quantize=False on the round-tripped images, bit for bit
    y = np.roll(x, 1, axis=-1)
    a = M.image_metrics(t(x), t(y), quantize=True)
    b = M.image_metrics(t(transform(x, quantize=True)), t(transform(y, quantize=True)))
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    o = metrics_oracle(x, y, quantize=True)
    assert within_one_ulp(np.stack([getattr(a, f).numpy() for f in M.FIELDS], 1), o["metrics"]).all()


def test_clamp_is_torch_clamp():
    from gscream_amd import metrics as M
    x = np.float32([-0.5, -0.0, 0.0, 0.25, 1.0, 1.5, np.nan, np.inf, -np.inf]).reshape(1, 1, 3, 3)
    want = torch.clamp(t(x), 0.0, 1.0).numpy()
    assert np.array_equal(transform(x, clamp=True), want, equal_nan=True)
    assert np.array_equal(M._transform_torch(t(x), True, False).numpy(), want, equal_nan=True)


def test_edge_semantics_on_the_torch_path():
    from gscream_amd import metrics as M
    pred, gt = smooth_pair(9, 11, c=3, b=2, seed=8)
    empty = np.zeros((2, 1, 9, 11), bool)
    m = M.image_metrics(t(pred), t(gt), t(empty))
    plain = M.image_metrics(t(pred), t(gt))
    for f in M.FIELDS[:4]:
        assert torch.equal(getattr(m, f), getattr(plain, f)) and torch.isnan(getattr(m, f + "_masked")).all()
    assert (m.sums[:, 4:] == 0).all()
    same = M.image_metrics(t(gt), t(gt))
    assert (same.mse == 0).all() and (same.l1 == 0).all() and torch.isinf(same.psnr).all() and (same.psnr > 0).all()
    assert within_one_ulp(same.ssim.numpy(), metrics_oracle(gt, gt)["metrics"][:, 3]).all() and (same.ssim > 0.999999).all()
    bad = pred.copy()
    bad[0, 1, 4, 5] = np.nan
    mask = np.ones((2, 1, 9, 11), bool)
    mask[:, :, :, 3:] = False  # the NaN and every window that holds it lie outside the mask
    n = M.image_metrics(t(bad), t(gt), t(mask))
    clean = M.image_metrics(t(pred), t(gt), t(mask))
    for f in M.FIELDS[:4]:
        assert torch.isnan(getattr(n, f)[0]) and torch.equal(getattr(n, f)[1], getattr(clean, f)[1])
        assert torch.equal(getattr(n, f + "_masked"), getattr(clean, f + "_masked"))
    o = metrics_oracle(bad, gt, mask)
    assert within_one_ulp(np.stack([getattr(n, f).numpy() for f in M.FIELDS], 1), o["metrics"]).all()


def test_the_drop_ins_have_the_references_signatures():
    from gscream_amd import metrics as M
    assert str(inspect.signature(M.mse)) == '(image_pred, image_gt, valid_mask=None, reduction=\'mean\')'
    assert str(inspect.signature(M.psnr)) == str(inspect.signature(M.mse))
    assert str(inspect.signature(M.my_ssim)) == '(image_pred, image_gt, mask=None, reduction=\'mean\')'
    d = case("37x53")
    p, g, mask = t(d["pred"]), t(d["gt"]), t(d["mask"]).expand(1, 3, -1, -1)
    m = M.image_metrics(p, g, mask)
    for fn, plain, masked in ((M.mse, m.mse, m.mse_masked), (M.psnr, m.psnr, m.psnr_masked), (M.my_ssim, m.ssim, m.ssim_masked)):
        a, b = fn(p, g), fn(p, g, mask)
        assert a.dim() == 0 and a.dtype == torch.float32 and torch.equal(a, plain[0]) and torch.equal(b, masked[0])
        assert torch.equal(fn(p[0], g[0]), a)
    # reduction != "mean": the reference's elementwise results, in torch
    v = M.mse(p, g, mask, reduction="none")
    assert torch.equal(v, ((p - g) ** 2)[mask]) and torch.equal(M.psnr(p, g, None, "none"), -10 * torch.log10((p - g) ** 2))
    # my_ssim does not pass `reduction` on (utils/loss_utils.py:127): every value gives the mean, here by the torch path
    for reduction in ("none", "sum", "median"):
        assert torch.equal(M.my_ssim(p, g, mask, reduction=reduction), m.ssim_masked[0]) and M.last_path == "torch" and not M.force_torch


def test_the_drop_ins_take_a_batch_as_the_reference_does():
    """The reference's mean runs over everything it is given: for a batch, over all its (selected) elements."""
    from gscream_amd import metrics as M
    d = case("past_the_tile")  # B = 3
    p, g, mask = t(d["pred"]), t(d["gt"]), t(d["mask"]).expand(-1, 3, -1, -1)
    for m4, key, h in ((None, "plain", 0), (mask, "masked", 4)):
        total = d[key]["sums"].sum(0)
        mse = total[h + 2] / total[h]
        for fn, want in ((M.mse, mse), (M.psnr, -10 * np.log10(mse)), (M.my_ssim, 1 - 2 * total[h + 3] / total[h])):
            got = fn(p, g, m4)
            assert got.dim() == 0 and got.dtype == torch.float32 and within_one_ulp(got.numpy(), want), (fn.__name__, key, got, want)
    x = p.double() - g.double()
    assert abs(float(M.mse(p, g)) - float((x * x).mean())) < 1e-9 and abs(float(M.mse(p, g, mask)) - float((x * x)[mask].mean())) < 1e-9


def test_the_mask_the_kernel_is_given():
    """What goes to the call: rows of W bytes, broadcast batch / channel dimensions as stride 0; a mask whose H or W would broadcast
    is refused on both paths (an expanded row has stride 0, and the kernel reads rows W bytes apart)."""
    from gscream_amd import metrics as M
    B, C, H, W = 2, 3, 5, 7
    shape, cpu = (B, C, H, W), torch.device("cpu")
    full = torch.rand(shape) < 0.5
    for mask, strides in ((full, (C * H * W, H * W, W, 1)), (full[0, 0], (0, 0, W, 1)), (full[0, :1], (0, 0, W, 1)), (full[:, :1], (C * H * W, 0, W, 1)),
                          (full[:, :1].contiguous(), (H * W, 0, W, 1)), (full[:, :1].expand(shape), (C * H * W, 0, W, 1)),
                          (full[..., ::2, :][..., :1, :, :].expand(B, C, 3, W), None)):
        if strides is None:  # rows 2 W apart: made dense
            m4 = M._mask_for_kernel(mask, (B, C, 3, W), cpu)
            assert m4.stride()[2:] == (W, 1) and torch.equal(m4, mask)
            continue
        m4 = M._mask_for_kernel(mask, shape, cpu)
        assert m4.stride() == strides and tuple(m4.shape) == shape and m4.data_ptr() == mask.data_ptr(), (mask.shape, m4.stride())
        # every byte the kernel reads lies inside the mask's storage
        last = (B - 1) * strides[0] + (C - 1) * strides[1] + (H - 1) * W + (W - 1)
        assert m4.storage_offset() + last < m4.untyped_storage().nbytes()
    transposed = (torch.rand(B, 1, W, H) < 0.5).transpose(2, 3)
    m4 = M._mask_for_kernel(transposed, shape, cpu)
    assert m4.stride() == (H * W, 0, W, 1) and torch.equal(m4, transposed.expand(shape))
    p, g = torch.rand(shape), torch.rand(shape)
    for bad in (full[0, 0, :1], full[:, :1, :1], full[..., :1], full[0, 0, 0], full[:, :, :-1]):  # [1,W], [B,1,1,W], [B,C,H,1], [W], H - 1 rows
        with pytest.raises(ValueError):
            M._mask_for_kernel(bad, shape, cpu)
        with pytest.raises(ValueError):
            M.image_metrics(p, g, bad)


def test_evaluate_views_takes_fp32_means_of_the_per_view_values():
    import gscream_amd
    from gscream_amd import metrics as M
    assert gscream_amd.evaluate_views is M.evaluate_views and gscream_amd.image_metrics is M.image_metrics
    pred, gt = smooth_pair(12, 10, c=3, b=5, seed=9)
    masks = [t(random_mask((1, 1, 12, 10), k)).expand(1, 3, -1, -1) for k in range(5)]
    names = [f"{k:05d}.png" for k in range(5)]
    renders, gts = [t(pred[k]) for k in range(5)], [t(gt[k])[None] for k in range(5)]  # [C,H,W] and [1,C,H,W] both
    full, per_view = M.evaluate_views(renders, gts, masks, names)
    assert list(full) == list(per_view) == ["SSIM", "PSNR", "masked SSIM", "masked PSNR"]
    m = M.image_metrics(t(pred), t(gt), torch.cat([k[:, :1] for k in masks]), quantize=True)
    for key, field in (("SSIM", m.ssim), ("PSNR", m.psnr), ("masked SSIM", m.ssim_masked), ("masked PSNR", m.psnr_masked)):
        assert list(per_view[key]) == names and list(per_view[key].values()) == field.tolist()
        assert full[key] == torch.tensor(field.tolist()).mean().item()  # evaluate()'s torch.tensor(list).mean().item()
    plain, _ = M.evaluate_views(renders, gts, quantize=False)
    m = M.image_metrics(t(pred), t(gt))
    assert plain["PSNR"] == m.psnr.mean().item() and plain["masked PSNR"] == plain["PSNR"]
    with pytest.raises(ValueError):
        M.evaluate_views(renders, gts[:4])


def test_fp32_is_the_references_arithmetic():
    """_metrics_torch(dtype=float32) on the stored cases: mse and psnr are the reference's stored fp32 values to within 2 ulp (the same
    fp32 mean, possibly another reduction order), and its ssim is within 1e-3 of the oracle: the mean cannot be further off than the map's worst pixel, which the fp32
    variances against C2 put at 3.1e-4 on a smooth 67x131 pair (INTEGRATION R's table; 4.7e-4 on the pair of the check that
    motivated the fp64 rule); 1e-3 is twice the larger, rounded up."""
    from gscream_amd import metrics as M
    z = np.load(GOLDEN)
    for name in STORED:
        pred, gt, mask = z[f"{name}/pred"], z[f"{name}/gt"], z[f"{name}/mask"]
        _s, m = M._metrics_torch(t(pred), t(gt), t(mask).expand(1, 3, -1, -1), dtype=torch.float32)
        for field, column in (("mse", 1), ("psnr", 2), ("mse_masked", 5), ("psnr_masked", 6)):
            ref, got = np.float32(z[f"{name}/{field}"]), m[0, column].numpy()
            assert abs(float(got) - float(ref)) <= 2 * float(np.spacing(ref)), (name, field, got, ref)
        o = metrics_oracle(pred, gt, mask)["metrics"][0]
        assert abs(float(m[0, 3]) - o[3]) < 1e-3 and abs(float(m[0, 7]) - o[7]) < 1e-3


def test_header_binding_and_library_have_the_two_calls(native_lib):
    from gscream_amd import _abi, _native
    hdr = _abi.header()
    assert hdr.constants["GSR_ABI_VERSION"] == 9 and _native.ABI_VERSION == 9 and native_lib.gsr_abi_version() == 9
    assert hdr.constants["GSR_METRICS_CLAMP"] == 1 and hdr.constants["GSR_METRICS_QUANTIZE"] == 2
    assert hdr.functions["gsr_image_metrics_workspace_bytes"][0] == "size_t" and hdr.functions["gsr_image_metrics"][0] == "int"
    for name in ("gsr_image_metrics_workspace_bytes", "gsr_image_metrics"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(native_lib, name)
    assert len(native_lib.gsr_image_metrics.argtypes) == 14 and len(native_lib.gsr_image_metrics_workspace_bytes.argtypes) == 4
    import ctypes
    for lib in ("libgsraster_precise.so", "libgsraster_replayall.so"):  # the two test builds link the same objects
        path = os.path.join(os.path.dirname(_native.LIB_PATH), lib)
        if os.path.exists(path):
            assert hasattr(ctypes.CDLL(path), "gsr_image_metrics")


def test_argument_checks_without_a_gpu(native_lib):
    """Everything the call rejects, it rejects before launching (there is no device here to launch on)."""
    call, size, err = native_lib.gsr_image_metrics, native_lib.gsr_image_metrics_workspace_bytes, native_lib.gsr_last_error
    a, b, c, d, e, f = 256, 512, 768, 1024, 1280, 1536  # never dereferenced on the host

    def run(B=1, C=3, H=5, W=7, pred=a, gt=b, mask=c, sb=0, sc=0, flags=0, ws=d, sums=e, metrics=f):
        return call(B, C, H, W, pred, gt, mask, sb, sc, flags, ws, sums, metrics, None)

    for k in ("pred", "gt", "ws", "sums", "metrics"):
        assert run(**{k: None}) == -1 and b"NULL" in err(), k
    for bc in ((0, 3), (1, 0), (-1, 3), (2, -3)):
        assert run(B=bc[0], C=bc[1]) == -1 and b"need both > 0" in err(), bc
        assert size(bc[0], bc[1], 5, 7) == 0
    for bc in ((65536, 1), (21846, 3), (1, 65536), (1 << 20, 1 << 20)):
        assert run(B=bc[0], C=bc[1]) == -1 and b"too many planes" in err(), bc
    for hw in ((2, 7), (5, 2), (0, 7), (5, -1)):
        assert run(H=hw[0], W=hw[1]) == -1 and b"need both >= 3" in err(), hw
        assert size(1, 3, *hw) == 0
    for chw in ((3, 26755, 26755), (1, 715827798, 3), (1, 46341, 46341), (65535, 32768, 3)):
        assert run(C=chw[0], H=chw[1], W=chw[2]) == -1 and b"too many elements" in err(), chw
    for flags in (4, 8, 7, -1, 1 << 20):
        assert run(flags=flags) == -1 and b"unknown flag" in err(), flags
    for s in ((-1, 0), (0, -1), (-(1 << 40), 5)):
        assert run(sb=s[0], sc=s[1]) == -1 and b"negative mask stride" in err(), s
    # the workspace: eight doubles per tile and plane
    assert size(1, 1, 3, 3) == 64 and size(2, 3, TILE_H, TILE_W) == 6 * 64 and size(2, 3, TILE_H + 1, TILE_W + 1) == 24 * 64
    assert size(40, 3, 567, 1008) == 40 * 3 * 36 * 32 * 64
