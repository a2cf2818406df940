"""CPU tests of gscream_amd.resize and gscream_amd.general_utils: the numpy statement of PIL's rule (tests/resize_helpers.py) against PIL
itself -- bytes for 8-bit pictures, bits for mode F -- the host tables against that statement, the host path and the loaders against
the reference's own lines, PIL's mode rules, the C ABI entries and the argument errors.  No tolerance appears: every comparison is
equality."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from tests import arena_helpers as A
from tests import resize_helpers as R
from gscream_amd import general_utils as G
from gscream_amd import resize as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = R.FILTERS + (R.NEAREST,)
IDS = [f"{a[0]}x{a[1]}_to_{b[0]}x{b[1]}" for a, b in R.CASES]


def test_constants_are_pils():
    for name in ("NEAREST", "LANCZOS", "BILINEAR", "BICUBIC", "BOX", "HAMMING"):
        assert getattr(Z, name) == getattr(R, name) == int(getattr(Image.Resampling, name)), name


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_the_statement_is_pils_8bit(case):
    (hi, wi), (ho, wo) = case
    for f in ALL:
        for C in (1, 3):
            for binary in (False, True):
                a = R.picture_u8(hi, wi, C, 3 + C, binary)
                a = a[:, :, 0] if C == 1 else a
                assert np.array_equal(R.resize(a, (wo, ho), f), R.pil_resize(a, (wo, ho), f)), (R.NAMES[f], C, binary)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_the_statement_is_pils_mode_f(case):
    (hi, wi), (ho, wo) = case
    for f in ALL:
        for special in (False, True):
            a = R.picture_f32(hi, wi, 5, special)
            assert R.same_bits(R.resize(a, (wo, ho), f), R.pil_resize(a, (wo, ho), f)), (R.NAMES[f], special)


def test_the_clamp_is_hit_at_both_ends():
    """Binary content under LANCZOS rings past 0 and 255 before the clamp: the case list's binary pictures exercise both ends."""
    a = R.picture_u8(37, 53, 1, 4, True)
    bounds, kk = R.tables(53, 13, R.LANCZOS)
    K = R.fixed(kk).astype(np.int64)
    acc = np.stack([(1 << 21) + sum(a[:, bounds[x, 0] + t, 0].astype(np.int64) * K[x, t] for t in range(bounds[x, 1])) for x in range(13)], 1) >> 22
    assert acc.min() < 0 and acc.max() > 255


def test_coefficients_equal_the_statement_and_are_cached():
    sizes = sorted({(a[k], b[k]) for a, b in R.CASES for k in (0, 1)} | {(4032, 1008), (567, 1134)})
    for in_size, out_size in sizes:
        for f in R.FILTERS:
            bounds, kk = Z.coefficients(in_size, out_size, f)
            want_bounds, want_kk = R.tables(in_size, out_size, f)
            assert bounds.dtype == np.int32 and kk.dtype == np.float64 and bounds.shape == (out_size, 2) and kk.shape[1] % 2 == 1
            assert np.array_equal(bounds, want_bounds), (in_size, out_size, f)
            assert np.array_equal(kk.view(np.uint64), want_kk.view(np.uint64)), (in_size, out_size, f)
            assert np.array_equal(Z.fixed_point(kk), R.fixed(want_kk))
            again = Z.coefficients(in_size, out_size, f)
            assert again[0] is bounds and again[1] is kk
            # what the kernels rely on: the bounds lie in the row and are monotone (a tile's sources are one segment)
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= in_size).all() and (bounds[:, 1] <= kk.shape[1]).all()
            assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds[:, 0] + bounds[:, 1]) >= 0).all()
        assert np.array_equal(Z.nearest_index(in_size, out_size), R.nearest_table(in_size, out_size))
        assert Z.nearest_index(in_size, out_size) is Z.nearest_index(in_size, out_size)
    assert Z.coefficients(200, 7, Z.LANCZOS)[1].shape[1] == 173


def test_nearest_is_the_accumulated_sum():
    """The closed form int((x + 0.5) a) is NOT PIL's table: somewhere they differ, and the accumulated one is what PIL reads."""
    differ = 0
    for in_size, out_size in ((200, 47), (53, 13), (300, 299), (31, 70), (129, 33), (4032, 1008), (1000, 3)):
        a = in_size / out_size
        closed = np.array([int((x + 0.5) * a) for x in range(out_size)])
        table = Z.nearest_index(in_size, out_size)
        differ += int((closed != table).any())
        row = np.arange(in_size, dtype=np.float32)[None]
        assert np.array_equal(np.array(Image.fromarray(row).resize((out_size, 1), Image.NEAREST))[0], table.astype(np.float32))
    assert differ > 0


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_host_path_equals_pil(case):
    (hi, wi), (ho, wo) = case
    for f in ALL + (R.HAMMING,):
        a3, a1, af = R.picture_u8(hi, wi, 3, 7), R.picture_u8(hi, wi, 1, 8)[:, :, 0], R.picture_f32(hi, wi, 9)
        for a in (a3, a1, af):
            got = Z.resize(torch.from_numpy(a), (wo, ho), f)
            assert Z.last_path == "pil" and got.dtype == torch.from_numpy(a).dtype
            assert np.array_equal(got.numpy(), np.array(Image.fromarray(a).resize((wo, ho), f)))
    a4 = R.picture_u8(hi, wi, 4, 10)
    assert np.array_equal(Z.resize(torch.from_numpy(a4), (wo, ho), Z.BICUBIC).numpy(), R.pil_resize(a4, (wo, ho), Z.BICUBIC))
    batch = np.stack([R.picture_u8(hi, wi, 3, s) for s in (1, 2)])
    got = Z.resize(torch.from_numpy(batch), (wo, ho), Z.LANCZOS)
    assert got.shape == (2, ho, wo, 3) and all(np.array_equal(got[b].numpy(), R.pil_resize(batch[b], (wo, ho), Z.LANCZOS)) for b in range(2))
    out = torch.zeros(ho, wo + 3, 3, dtype=torch.uint8)
    assert Z.resize(torch.from_numpy(a3), (wo, ho), Z.BOX, out=out[:, 1:1 + wo]).data_ptr() == out[:, 1:].data_ptr()
    assert np.array_equal(out[:, 1:1 + wo].numpy(), R.pil_resize(a3, (wo, ho), Z.BOX))


def test_the_division_by_255_over_all_bytes():
    """The fused epilogue is __fdiv_rn(float(v), 255.0f): one IEEE float32 division, which is what torch's `uint8 / 255.0` gives."""
    v = np.arange(256, dtype=np.uint8)
    want = (torch.from_numpy(v) / 255.0).numpy()
    assert want.dtype == np.float32
    assert np.array_equal(want.view(np.uint32), (v.astype(np.float32) / np.float32(255.0)).view(np.uint32))
    img = Image.fromarray(v.reshape(16, 16))
    got = G.PILtoTorch(img, (16, 16), device="cpu")
    assert got.shape == (1, 16, 16) and np.array_equal(got.numpy().reshape(-1).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("size", [(13, 9), (53, 37), (70, 57)])
def test_loaders_on_the_host_equal_the_reference_lines(size):
    rgb, gray, depth = R.picture_u8(37, 53, 3, 1), R.picture_u8(37, 53, 1, 2, True)[:, :, 0], R.picture_f32(37, 53, 3)
    for a in (rgb, gray):
        img = Image.fromarray(a)
        want = torch.from_numpy(np.array(img.resize(size))) / 255.0
        want = want.permute(2, 0, 1) if want.dim() == 3 else want.unsqueeze(dim=-1).permute(2, 0, 1)
        got = G.PILtoTorch(img, size, device="cpu")
        assert G.last_path == "pil" and got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, want)
        want = torch.from_numpy((np.array(img.resize(size)) > 0).astype(np.float32))
        want = want.permute(2, 0, 1) if want.dim() == 3 else want.unsqueeze(dim=-1).permute(2, 0, 1)
        got = G.PILtoTorch_01mask(img, size, device="cpu")
        assert got.dtype == torch.float32 and got.shape == want.shape and torch.equal(got, want)
    img = Image.fromarray(depth)
    want = torch.from_numpy(np.array(img.resize(size)).astype(np.float32)).unsqueeze(dim=-1).permute(2, 0, 1)
    got = G.PILtoTorch_depth(img, size, device="cpu")
    assert got.shape == (1, size[1], size[0]) and torch.equal(got, want)


class _Stub:
    """Stands in for the native library: records the calls, launches nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("gsr_resize"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append(name)
            return 0
        return call


def _stub_the_launches(monkeypatch):
    """Make a CPU tensor pass for a device one: `.to("cuda")` is the identity, the route check says yes, the launch is recorded."""
    from gscream_amd import _native
    stub = _Stub()
    monkeypatch.setattr(_native, "run", lambda name, device, *args: getattr(stub, name)(*args))
    # (the pointers go to the stub, never to a kernel: ptr() without its refusal of host memory)
    monkeypatch.setattr(_native, "ptr", lambda t: None if t is None or t.numel() == 0 else _native.ctypes.c_void_p(t.data_ptr()))
    monkeypatch.setattr(Z, "_on_device", lambda x, resample: not Z.force_host and resample != Z.HAMMING and x.dtype in (torch.uint8, torch.float32))
    real_to = torch.Tensor.to
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self if a and isinstance(a[0], torch.device) and a[0].type == "cuda" else real_to(self, *a, **k))
    return stub


def test_resize_pil_image_routes_by_mode(monkeypatch):
    stub = _stub_the_launches(monkeypatch)
    rgb = Image.fromarray(R.picture_u8(23, 31, 3, 1))
    images = {"L": rgb.convert("L"), "RGB": rgb, "F": Image.fromarray(R.picture_f32(23, 31, 2)), "P": rgb.convert("P"), "1": rgb.convert("1"),
              "LA": rgb.convert("LA"), "RGBA": rgb.convert("RGBA")}
    for mode, img in images.items():
        assert img.mode == mode
        del stub.calls[:]
        got = Z.resize_pil_image(img, (13, 9), device="cuda")
        if mode in ("L", "RGB", "F"):
            assert Z.last_path == "hip" and len(stub.calls) == 2 and stub.calls[0] == ("gsr_resize_f32" if mode == "F" else "gsr_resize_u8"), mode
            assert got.shape[:2] == (9, 13) and got.dtype == (torch.float32 if mode == "F" else torch.uint8)
        else:
            assert Z.last_path == "pil" and not stub.calls, mode
            want = np.array(img.resize((13, 9)))
            want = want.astype(np.uint8) * 255 if want.dtype == np.bool_ else want
            assert np.array_equal(got.numpy(), want), mode
    assert Z.pil_route("P", Z.LANCZOS) == ("host", Z.NEAREST) and Z.pil_route("1", None) == ("host", Z.NEAREST)
    assert Z.pil_route("L", None) == ("hip", Z.BICUBIC) and Z.pil_route("RGB", Z.HAMMING) == ("host", Z.HAMMING)
    assert Z.pil_route("RGBA", None) == ("host", Z.BICUBIC) and Z.pil_route("I;16", None) == ("host", Z.BICUBIC)
    # the launch counts of the public forms: two passes, one pass, a copy, NEAREST; the loaders fuse their last step
    x = torch.from_numpy(R.picture_u8(23, 31, 3, 1))
    for size, f, launches in (((13, 9), Z.LANCZOS, 2), ((31, 9), Z.BOX, 1), ((13, 23), Z.BILINEAR, 1), ((31, 23), Z.BICUBIC, 1), ((13, 9), Z.NEAREST, 1)):
        del stub.calls[:]
        Z.resize(x, size, f)
        assert Z.last_path == "hip" and len(stub.calls) == launches == Z.last_launches, (size, f, stub.calls)
    for size, launches in (((13, 9), 2), ((31, 23), 1)):
        del stub.calls[:]
        assert G.PILtoTorch(rgb, size).shape == (3, size[1], size[0]) and G.last_path == "hip" and len(stub.calls) == launches
        assert G.PILtoTorch_01mask(images["L"], size).shape == (1, size[1], size[0]) and G.PILtoTorch_depth(images["F"], size).shape == (1, size[1], size[0])
    # `out` on the device path: the result's shape and dtype, adjacent channels and pixels
    with pytest.raises(ValueError, match="out is"):
        Z.resize(x, (13, 9), out=torch.zeros(9, 14, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="adjacent"):
        Z.resize(x, (13, 9), out=torch.zeros(9, 13, 6, dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(ValueError, match="at most 65535"):
        Z.resize(x, (65536, 9))
    monkeypatch.setattr(Z, "force_host", True)
    Z.resize(x, (13, 9), Z.LANCZOS)
    assert Z.last_path == "pil"


def test_abi_entries(native_lib):
    from gscream_amd import _abi, _native
    hdr = _abi.header()
    assert hdr.constants["GSR_ABI_VERSION"] == 9 and native_lib.gsr_abi_version() == 9 and _native.ABI_VERSION == 9
    table = A.header_table()
    names = ("gsr_resize_u8", "gsr_resize_f32", "gsr_resize_nearest_u8", "gsr_resize_nearest_f32")
    for name in names:
        assert hdr.functions[name][0] == "int" and name in _native.EXPORTED_SYMBOLS and hasattr(native_lib, name)
        params = table[name]
        assert params[-1] == ("void*", "stream", True, False)
        assert len(params) == len(getattr(native_lib, name).argtypes)
        # device pointers only: every pointer parameter but the stream is device memory, so none is on the host-parameter list
        assert not [p for p in params if (name, p[1]) in A.HOST_PARAMS]
        assert [p[1] for p in params if p[2] and not p[3]] == ["out", "stream"]
    assert hdr.constants["GSR_RESIZE_PRECISION_BITS"] == 22
    assert [hdr.constants["GSR_RESIZE_" + n] for n in ("HORIZONTAL", "VERTICAL", "U8", "DIV255", "GT0")] == [0, 1, 0, 1, 2]
    assert (_native.RESIZE_HORIZONTAL, _native.RESIZE_VERTICAL, _native.RESIZE_U8, _native.RESIZE_DIV255, _native.RESIZE_GT0) == (0, 1, 0, 1, 2)
    buf = (_native.ctypes.c_uint8 * 64)()
    assert native_lib.gsr_resize_u8(buf, 64, 8, 1, 8, 8, 5, 0, 4, buf, buf, 3, buf, 32, 4, 0, None) == -1 and b"C=5" in native_lib.gsr_last_error()
    assert native_lib.gsr_resize_u8(None, 64, 8, 1, 8, 8, 1, 0, 4, buf, buf, 3, buf, 32, 4, 0, None) == -1 and b"NULL" in native_lib.gsr_last_error()
    assert native_lib.gsr_resize_u8(buf, 64, 8, 1, 8, 8, 1, 0, 0, buf, buf, 3, buf, 32, 4, 0, None) == -1 and b"out_len" in native_lib.gsr_last_error()
    assert native_lib.gsr_resize_u8(buf, 64, 7, 1, 8, 8, 1, 0, 4, buf, buf, 3, buf, 32, 4, 0, None) == -1 and b"strides" in native_lib.gsr_last_error()
    assert native_lib.gsr_resize_u8(buf, 64, 8, 1, 8, 8, 1, 2, 4, buf, buf, 3, buf, 32, 4, 0, None) == -1 and b"axis" in native_lib.gsr_last_error()
    assert native_lib.gsr_resize_u8(buf, 64, 8, 1, 8, 8, 1, 0, 4, buf, buf, 3, buf, 32, 5, 1, None) == -1 and b"contiguous" in native_lib.gsr_last_error()
    assert native_lib.gsr_resize_f32(buf, 64, 8, 1, 8, 8, 0, 4, buf, None, 3, buf, 32, 4, None) == -1 and b"NULL" in native_lib.gsr_last_error()
    assert native_lib.gsr_resize_nearest_u8(buf, 64, 8, 1, 8, 8, 1, 4, 8, None, None, buf, 32, 8, 0, None) == -1 and b"identity" in native_lib.gsr_last_error()
    assert native_lib.gsr_resize_nearest_f32(buf, 64, 8, 1, 8, 8, 4, 4, buf, buf, buf, 16, 3, None) == -1 and b"strides" in native_lib.gsr_last_error()


def test_the_fp64_chain_is_not_contracted(tmp_path):
    """resize.hip compiled with its Makefile flags holds separate fp64 products and sums and no fused fp64 instruction: with the
    pragma and the _rn intrinsics alone the chain came out fused and mode F was not PIL's bits on the device."""
    import subprocess
    csrc = os.path.join(ROOT, "gscream_amd", "csrc")
    flags = re.search(r"^SRCFLAGS_resize\s*=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = str(tmp_path / "resize.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, "-S", "--cuda-device-only", "-o", asm,
                    os.path.join(csrc, "resize.hip")], check=True, stderr=subprocess.DEVNULL)
    text = open(asm).read()
    assert "v_mul_f64" in text and "v_add_f64" in text
    assert not re.search(r"v_fma_f64|v_fmac_f64|v_mad_f64", text)


def test_argument_errors():
    x = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="C=5"):
        Z.resize(torch.zeros(8, 8, 5, dtype=torch.uint8), (4, 4))
    with pytest.raises(ValueError, match="size="):
        Z.resize(x, (0, 4))
    with pytest.raises(ValueError, match="size="):
        Z.resize(x, (4, 0))
    with pytest.raises(ValueError, match="size="):
        Z.resize(x, (4,))
    with pytest.raises(ValueError, match="dtype"):
        Z.resize(torch.zeros(8, 8, 3, dtype=torch.float64), (4, 4))
    with pytest.raises(ValueError, match="dtype"):
        Z.resize(torch.zeros(2, 8, 8, dtype=torch.int16), (4, 4))
    with pytest.raises(ValueError, match="unknown filter"):
        Z.resize(x, (4, 4), 6)
    with pytest.raises(ValueError, match="unknown filter"):
        Z.resize(x, (4, 4), "bicubic")
    with pytest.raises(ValueError, match="float32 picture"):
        Z.resize(torch.zeros(2, 8, 8, 3), (4, 4))
    with pytest.raises(ValueError, match="empty"):
        Z.resize(torch.zeros(0, 8, 3, dtype=torch.uint8), (4, 4))
    with pytest.raises(ValueError, match="no coefficient table"):
        Z.coefficients(8, 4, Z.NEAREST)
    with pytest.raises(ValueError, match="positive"):
        Z.coefficients(0, 4, Z.BOX)


def test_read_images_mask_resize_keyword_on_the_host(tmp_path):
    """mask_resize is accepted on a CPU device, where every mask takes the PIL call, and rejects other words."""
    from gscream_amd import png_decode
    dirs = {k: tmp_path / k for k in ("renders", "gt", "masks")}
    for d in dirs.values():
        d.mkdir()
    Image.fromarray(R.picture_u8(24, 40, 3, 1)).save(dirs["renders"] / "00000.png")
    Image.fromarray(R.picture_u8(24, 40, 3, 2)).save(dirs["gt"] / "00000.png")
    mask = R.picture_u8(96, 160, 1, 3, True)[:, :, 0]
    Image.fromarray(mask).save(dirs["masks"] / "out_00001.png")
    want = torch.from_numpy(np.array(Image.fromarray(mask).resize((40, 24), Image.LANCZOS)) > 0)
    for how in ("pil", "hip"):
        r, g, names, m = png_decode.read_images(dirs["renders"], dirs["gt"], dirs["masks"], device="cpu", mask_resize=how)
        assert png_decode.last_info["masks_resized"] == 1 and png_decode.last_info["masks_resized_hip"] == 0
        assert m[0].shape == (1, 3, 24, 40) and torch.equal(m[0][0, 0], want)
    with pytest.raises(ValueError, match="mask_resize"):
        png_decode.read_images(dirs["renders"], dirs["gt"], dirs["masks"], device="cpu", mask_resize="gpu")
