"""gscream_amd.resize on the device.  Every comparison is equality with PIL, called here: bytes for 8-bit pictures (C = 4 as four L
planes: the channels are independent and nothing is premultiplied), bits for mode F with the NaN positions compared as a mask.  The
shapes are tests/resize_helpers.py's CASES: the smallest at which a pass can go wrong."""
import numpy as np
import pytest
import torch
from PIL import Image

from tests import arena_helpers as A
from tests import resize_helpers as R
from gscream_amd import _native
from gscream_amd import general_utils as G
from gscream_amd import resize as Z

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = R.FILTERS + (R.NEAREST,)
IDS = [f"{a[0]}x{a[1]}_to_{b[0]}x{b[1]}" for a, b in R.CASES]
MiB = 1 << 20


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _hip(x, size, f, **kw):
    got = Z.resize(x, size, f, **kw)
    assert Z.last_path == "hip"
    return got


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_8bit_equals_pil(case):
    (hi, wi), (ho, wo) = case
    for C in (1, 2, 3, 4):
        for binary in (False, True):
            a = R.picture_u8(hi, wi, C, 11 + C, binary)
            x = dev(a)
            for f in ALL:
                got = _hip(x, (wo, ho), f)
                assert got.dtype == torch.uint8 and got.shape == (ho, wo, C)
                assert np.array_equal(got.cpu().numpy(), R.pil_resize(a, (wo, ho), f)), (R.NAMES[f], C, binary)
            if C == 1:  # the [H, W] form
                got = _hip(x[:, :, 0], (wo, ho), Z.LANCZOS)
                assert got.shape == (ho, wo) and np.array_equal(got.cpu().numpy(), R.pil_resize(a[:, :, 0], (wo, ho), Z.LANCZOS))


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_mode_f_equals_pil(case):
    (hi, wi), (ho, wo) = case
    for special in (False, True):  # values in +-1e4; then an inf, a -inf and a NaN among them
        a = R.picture_f32(hi, wi, 21, special)
        x = dev(a)
        for f in ALL:
            got = _hip(x, (wo, ho), f)
            assert got.dtype == torch.float32 and got.shape == (ho, wo)
            assert R.same_bits(got.cpu().numpy(), R.pil_resize(a, (wo, ho), f)), (R.NAMES[f], special)


def test_a_batch_of_three():
    batch = np.stack([R.picture_u8(37, 53, 3, s) for s in (1, 2, 3)])
    depth = np.stack([R.picture_f32(37, 53, s) for s in (4, 5, 6)])
    for f in ALL:
        got = _hip(dev(batch), (13, 9), f)
        assert got.shape == (3, 9, 13, 3)
        got_f = _hip(dev(depth), (70, 57), f)
        assert got_f.shape == (3, 57, 70)
        for b in range(3):
            assert np.array_equal(got[b].cpu().numpy(), R.pil_resize(batch[b], (13, 9), f)), (R.NAMES[f], b)
            assert R.same_bits(got_f[b].cpu().numpy(), R.pil_resize(depth[b], (70, 57), f)), (R.NAMES[f], b)


def test_strided_source_and_destination():
    """The source is a column slice of a wider tensor (its row stride is not W C), and so is `out`; what lies beside them is untouched."""
    wide = R.picture_u8(37, 53 + 24, 3, 7)
    wide_f = R.picture_f32(37, 53 + 24, 8)
    batch = np.stack([R.picture_u8(37, 53 + 24, 3, s) for s in (1, 2)])
    for f in ALL:
        for (wo, ho) in ((13, 9), (53, 9), (13, 37), (53, 37)):
            sheet = torch.full((ho, wo + 7, 3), 0x5A, dtype=torch.uint8, device=DEV)
            src = dev(wide)[:, 11:11 + 53]
            assert not src.is_contiguous()
            _hip(src, (wo, ho), f, out=sheet[:, 5:5 + wo])
            want = np.full((ho, wo + 7, 3), 0x5A, np.uint8)
            want[:, 5:5 + wo] = R.pil_resize(np.ascontiguousarray(wide[:, 11:11 + 53]), (wo, ho), f)
            assert np.array_equal(sheet.cpu().numpy(), want), (R.NAMES[f], wo, ho)
        sheet = torch.full((9, 13 + 7), -7.0, dtype=torch.float32, device=DEV)
        _hip(dev(wide_f)[:, 11:11 + 53], (13, 9), f, out=sheet[:, 5:18])
        want = np.full((9, 20), -7.0, np.float32)
        want[:, 5:18] = R.pil_resize(np.ascontiguousarray(wide_f[:, 11:11 + 53]), (13, 9), f)
        assert R.same_bits(sheet.cpu().numpy(), want), R.NAMES[f]
        got = _hip(dev(batch)[:, 3:3 + 30, 11:11 + 53], (13, 9), f)  # rows and pictures strided as well
        for b in range(2):
            assert np.array_equal(got[b].cpu().numpy(), R.pil_resize(np.ascontiguousarray(batch[b, 3:33, 11:64]), (13, 9), f))
    # channels that are not adjacent take a copy first
    a = R.picture_u8(37, 53, 4, 9)
    got = _hip(dev(a)[:, :, ::2], (13, 9), Z.BICUBIC)
    assert np.array_equal(got.cpu().numpy(), R.pil_resize(np.ascontiguousarray(a[:, :, ::2]), (13, 9), Z.BICUBIC))


@pytest.mark.parametrize("size", [(13, 9), (53, 9), (13, 37), (53, 37), (70, 57)])
def test_fused_epilogues_equal_resize_then_the_torch_line(size):
    rgb, gray = R.picture_u8(37, 53, 3, 1), R.picture_u8(37, 53, 1, 2, True)[:, :, 0]
    for a in (rgb, gray):
        x = dev(a)
        for f in ALL:
            small = _hip(x, size, f)
            # the torch line runs where the reference runs it, on the host: `uint8 / 255.0` is one IEEE division there, while torch's
            # device kernel multiplies by the rounded reciprocal of a scalar divisor and differs from it in the last bit
            small = (small if small.dim() == 3 else small[:, :, None]).cpu()
            got = Z.to_float_chw(x, size, f, _native.RESIZE_DIV255)
            assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got.cpu(), small.permute(2, 0, 1) / 255.0), (R.NAMES[f], "div255")
            got = Z.to_float_chw(x, size, f, _native.RESIZE_GT0)
            assert torch.equal(got.cpu(), (small.permute(2, 0, 1) > 0).to(torch.float32)), (R.NAMES[f], "gt0")
            assert Z.last_launches == (size[0] != 53) + (size[1] != 37) if f != Z.NEAREST and size != (53, 37) else Z.last_launches == 1
        # the loaders against the reference's own lines on the host
        img = Image.fromarray(a)
        want = torch.from_numpy(np.array(img.resize(size))) / 255.0
        want = want.permute(2, 0, 1) if want.dim() == 3 else want.unsqueeze(dim=-1).permute(2, 0, 1)
        got = G.PILtoTorch(img, size, device=DEV)
        assert G.last_path == "hip" and got.is_cuda and got.shape == want.shape and torch.equal(got.cpu(), want)
        want = torch.from_numpy((np.array(img.resize(size)) > 0).astype(np.float32))
        want = want.permute(2, 0, 1) if want.dim() == 3 else want.unsqueeze(dim=-1).permute(2, 0, 1)
        got = G.PILtoTorch_01mask(img, size, device=DEV)
        assert G.last_path == "hip" and got.shape == want.shape and torch.equal(got.cpu(), want)
    depth = Image.fromarray(R.picture_f32(37, 53, 3))
    want = torch.from_numpy(np.array(depth.resize(size)).astype(np.float32)).unsqueeze(dim=-1).permute(2, 0, 1)
    got = G.PILtoTorch_depth(depth, size, device=DEV)
    assert G.last_path == "hip" and got.shape == (1, size[1], size[0]) and R.same_bits(got.cpu().numpy(), want.numpy())


def test_all_256_bytes_through_the_division():
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    got = Z.to_float_chw(dev(v), (16, 16), Z.BICUBIC, _native.RESIZE_DIV255)
    assert torch.equal(got.cpu(), (torch.from_numpy(v) / 255.0)[None])


def test_resize_pil_image_on_the_device():
    rgb = Image.fromarray(R.picture_u8(37, 53, 3, 5))
    for img in (rgb, rgb.convert("L"), Image.fromarray(R.picture_f32(37, 53, 6))):
        got = Z.resize_pil_image(img, (13, 9), device=DEV)
        assert Z.last_path == "hip" and got.is_cuda
        want = np.array(img.resize((13, 9)))
        assert R.same_bits(got.cpu().numpy(), want) if img.mode == "F" else np.array_equal(got.cpu().numpy(), want)
    for img in (rgb.convert("RGBA"), rgb.convert("P"), rgb.convert("LA")):
        got = Z.resize_pil_image(img, (13, 9), device=DEV)
        assert Z.last_path == "pil" and got.is_cuda and np.array_equal(got.cpu().numpy(), np.array(img.resize((13, 9))))
    a = R.picture_u8(37, 53, 3, 5)
    got = Z.resize(dev(a), (13, 9), Z.HAMMING)
    assert Z.last_path == "pil" and got.is_cuda and np.array_equal(got.cpu().numpy(), np.array(Image.fromarray(a).resize((13, 9), Image.HAMMING)))


def _everything(x8, xf):
    out = {}
    for f in ALL:
        out[f"u8/{f}"] = Z.resize(x8, (13, 9), f)
        out[f"f32/{f}"] = Z.resize(xf, (13, 9), f)
        out[f"up/{f}"] = Z.resize(x8, (70, 57), f)
    out["long"] = Z.resize(x8[:3], (7, 3), Z.LANCZOS)
    out["div255"] = Z.to_float_chw(x8, (13, 9), Z.BICUBIC, _native.RESIZE_DIV255)
    out["gt0"] = Z.to_float_chw(x8, (53, 37), Z.BICUBIC, _native.RESIZE_GT0)
    return out


def test_two_runs_are_bit_identical():
    x8, xf = dev(R.picture_u8(37, 53, 3, 1)), dev(R.picture_f32(37, 53, 2, True))
    A.assert_same_bits({"first": _everything(x8, xf), "second": _everything(x8, xf)}, "resize")


def test_no_host_stop():
    x8, xf = dev(R.picture_u8(37, 53, 3, 1)), dev(R.picture_f32(37, 53, 2))
    first = _everything(x8, xf)  # (the library is loaded, the tables are on the device, the allocator warm)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = _everything(x8, xf)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    A.assert_same_bits({"first": first, "second": second}, "resize without a host stop")


def test_read_images_resizes_masks_on_the_device(tmp_path):
    from gscream_amd import png_decode
    dirs = {k: tmp_path / k for k in ("renders", "gt", "masks")}
    for d in dirs.values():
        d.mkdir()
    for k in range(3):
        Image.fromarray(R.picture_u8(24, 40, 3, k)).save(dirs["renders"] / f"{k:05d}.png")
        Image.fromarray(R.picture_u8(24, 40, 3, k + 10)).save(dirs["gt"] / f"{k:05d}.png")
    Image.fromarray(R.picture_u8(96, 160, 1, 20, True)[:, :, 0]).save(dirs["masks"] / "out_00001.png")
    Image.fromarray(R.picture_u8(96, 160, 1, 21)[:, :, 0]).save(dirs["masks"] / "out_00002.png")
    Image.fromarray(R.picture_u8(24, 40, 1, 22, True)[:, :, 0]).save(dirs["masks"] / "out_00003.png")  # already the render's size
    got = {}
    for how in ("pil", "hip"):
        got[how] = png_decode.read_images(dirs["renders"], dirs["gt"], dirs["masks"], device=DEV, mask_resize=how)
        info = png_decode.last_info
        assert info["masks_resized"] == 2 and info["masks_resized_hip"] == (2 if how == "hip" else 0) and info["host_decoded"] == 0, (how, info)
    assert got["pil"][2] == got["hip"][2]
    for part in (0, 1, 3):
        for a, b in zip(got["pil"][part], got["hip"][part]):
            assert a.shape == b.shape and a.dtype == b.dtype and a.is_cuda and b.is_cuda and torch.equal(a, b)
    # the default is today's behaviour
    png_decode.read_images(dirs["renders"], dirs["gt"], dirs["masks"], device=DEV)
    assert png_decode.last_info["masks_resized_hip"] == 0
    # a mask with an alpha channel keeps the PIL call (PIL premultiplies); readImages then refuses its two channels on either path
    la = Image.merge("LA", [Image.fromarray(R.picture_u8(96, 160, 1, s, s == 23)[:, :, 0]) for s in (23, 24)])
    la.save(dirs["masks"] / "out_00002.png")
    for how in ("pil", "hip"):
        with pytest.raises(ValueError, match="2 channels"):
            png_decode.read_images(dirs["renders"], dirs["gt"], dirs["masks"], device=DEV, mask_resize=how)
        info = png_decode.last_info
        names = got["pil"][2]
        before = sum(1 for n in names[:names.index("00001.png")] if n == "00000.png")  # the resized L mask, if it came first
        assert info["masks_resized"] == before + 1 and info["masks_resized_hip"] == (before if how == "hip" else 0), (how, info)


def test_the_arena(monkeypatch):
    """Every new entry point once inside guarded, poisoned, exact-size buffers at odd sizes, (37, 53, 3) -> (9, 13): both passes for
    both types, the two fused epilogues, the epilogue alone, NEAREST for both types; the tables are uploaded inside the arena, so the
    proxy holds them (const) to their bytes.  Plain, 0xA5 and 0xFF runs must agree bit for bit."""
    a8, af = R.picture_u8(37, 53, 3, 1), R.picture_f32(37, 53, 2)
    wide = R.picture_u8(37, 53 + 24, 3, 7)
    expect = ("gsr_resize_u8", "gsr_resize_f32", "gsr_resize_nearest_u8", "gsr_resize_nearest_f32")

    def run():
        Z.clear_cache()
        x8, xf = dev(a8), dev(af)
        out = _everything(x8, xf)
        sheet = torch.zeros((9, 13 + 7, 3), dtype=torch.uint8, device=DEV)
        Z.resize(dev(wide)[:, 11:11 + 53], (13, 9), Z.LANCZOS, out=sheet[:, 5:18])
        out["sheet"] = sheet
        return out

    runs = {"plain": {k: v.cpu() for k, v in run().items()}}
    for name, poison in (("arena_a5", 0xA5), ("arena_ff", 0xFF)):
        with A.guarded(monkeypatch, 32 * MiB, poison, DEV) as (arena, proxy):
            got = run()
            runs[name] = {k: v.cpu() for k, v in got.items()}
            for k, v in got.items():  # exact-size bodies: the result is the whole body
                assert arena.owns(v), k
        calls, guarded, bodies = proxy.stats()
        print(f"arena resize / poison 0x{poison:02X}: {calls} native calls {dict(proxy.calls)}, {guarded} guarded writable buffers, {bodies} bodies")
        assert not [fn for fn in expect if not proxy.calls.get(fn)] and guarded > 0
    Z.clear_cache()
    A.assert_same_bits(runs, "resize")
    assert np.array_equal(runs["plain"]["u8/1"].numpy(), R.pil_resize(a8, (13, 9), Z.LANCZOS))
