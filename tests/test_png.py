"""CPU tests of gscream_amd.png: the host statement of the rules through every decoder of record, the C ABI of the three new entry
points, the capacity formula, and the rules model of tests/png_helpers.py (which the GPU tests hold the kernels against byte for
byte) through the same decoders."""
import os

import numpy as np
import pytest
import torch

from tests import png_helpers as PH  # noqa: E402
from gscream_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("texture", "colormap", "mask", "constant", "noise")


def _host(image, filter="adaptive", out=None):
    from gscream_amd import png
    batch = png.encode(torch.from_numpy(image), filter, out=out)
    assert png.last_path == "torch"
    return png.to_bytes(batch), batch


@pytest.mark.parametrize("shape", PH.SHAPES + [(96, 250, 3)])
def test_host_path_decodes_for_every_shape(shape):
    H, W, C = shape
    image = S.picture("texture", H, W, C, seed=H + W)
    (data,), batch = _host(image)
    PH.check_file(data, image)
    assert batch.shape == shape and not batch.batched
    assert int(batch.data[0, :4].numpy().view("<u4")[0]) == len(data)


@pytest.mark.parametrize("kind", KINDS)
def test_host_path_contents_and_rules_model(kind):
    """Each content on a three-chunk picture whose cuts fall mid-row: the host path and the rules model both decode, with the same
    filter bytes."""
    image = S.picture(kind, 96, 250, 3, seed=3)
    (data,), _ = _host(image)
    a = PH.check_file(data, image)
    b = PH.check_file(PH.rules_file(image), image)
    assert a == b and len(PH.parse(data)[1]) == 3


@pytest.mark.parametrize("filter", [0, 1, 2, 3, 4, "adaptive"])
def test_host_path_filters(filter):
    image = S.picture("texture", 37, 53, 4, seed=1)
    code = PH.ADAPTIVE if filter == "adaptive" else filter
    (data,), _ = _host(image, filter)
    PH.check_file(data, image, code)
    PH.check_file(PH.rules_file(image, code), image, code)


def test_host_batch_out_buffer_and_save(tmp_path):
    from PIL import Image
    from gscream_amd import png
    images = np.stack([S.picture(k, 20, 31, 3, seed=7) for k in ("texture", "mask", "noise")])
    need = png.HEADER + png.capacity(20, 31, 3)
    out = torch.full((3, (need + 43) & ~3), 0xA5, dtype=torch.uint8)
    files, batch = _host(images, out=out)
    assert batch.batched and batch.data is out and len(files) == 3
    for b, data in enumerate(files):
        PH.check_file(data, images[b])
        assert bool((out[b, png.HEADER + len(data):] == 0xA5).all()), "bytes behind the file were written"
    paths = [str(tmp_path / f"{b}.png") for b in range(3)]
    png.save(torch.from_numpy(images), paths)
    png.save(torch.from_numpy(images[0]), str(tmp_path / "one.png"), filter=4)
    for b, path in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(path)), images[b])
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "one.png"))), images[0])
    with pytest.raises(ValueError):
        png.encode(torch.from_numpy(images), out=torch.zeros((3, need - 1), dtype=torch.uint8))
    with pytest.raises(ValueError):
        png.encode(torch.zeros((4, 4, 2), dtype=torch.uint8))
    with pytest.raises(TypeError):
        png.encode(torch.zeros((4, 4, 3)))
    with pytest.raises(ValueError):
        png.encode(torch.zeros((4, 4, 3), dtype=torch.uint8), filter="best")


def test_host_frames_files(tmp_path):
    """save_view_frames / save_rgbd_frame write the five files of the tuples frames.py returns; the panels are read as views."""
    from PIL import Image
    from gscream_amd import frames, png
    from tests import frames_helpers as FH
    v = {k: torch.from_numpy(x) for k, x in FH.view_inputs(12, 17, 5).items()}
    vf = frames.view_frames(v["render"], v["uncertainty"], v["gt"], v["depth"], v["midas"], v["mask"])
    paths = [str(tmp_path / f"v{k}.png") for k in range(5)]
    png.save_view_frames(vf, paths)
    for path, want in zip(paths, (vf.render, vf.uncertainty, vf.error, vf.gt, vf.depth)):
        assert np.array_equal(np.asarray(Image.open(path)), want.numpy())
    fr = frames.rgbd_frame(v["render"], v["depth"], v["uncertainty"], v["normals"], panels=True)
    paths = [str(tmp_path / f"r{k}.png") for k in range(5)]
    png.save_rgbd_frame(fr, paths)
    for path, want in zip(paths, fr):
        assert np.array_equal(np.asarray(Image.open(path)), want.numpy())


def test_rules_model_edge_chunks():
    """The rules model on the chunks the GPU tests use: one distinct byte, no repeats (no distance code), the code-length ladder."""
    zeros = np.zeros((40, 1000, 1), np.uint8)
    data = PH.rules_file(zeros, 0)
    PH.check_file(data, zeros, 0)
    assert len(data) <= 0.02 * zeros.size
    ladder, hist = PH.ladder_picture()
    assert PH.unlimited_depth(hist) > 15
    data = PH.rules_file(ladder, 0)
    PH.check_file(data, ladder, 0)
    assert max(PH.limited_lengths(list(hist), 15)) == 15
    for n in (3, 10, 11, 12, 18, 19, 130, 131, 227, 257, 258):
        s, eb, ev = PH.length_symbol(n)
        assert PH.LENGTH_BASE[s - 257] + ev == n and ev < (1 << eb) + (eb == 0)


def test_capacity_formula_against_noise(native_lib):
    from gscream_amd import png
    for H, W, C in PH.SHAPES + [(96, 250, 3), (567, 1008, 3)]:
        assert native_lib.gsr_png_capacity(H, W, C) == png.capacity(H, W, C) == PH.capacity(H, W, C)
    image = S.picture("noise", 96, 250, 3, seed=9)
    for data in (_host(image)[0][0], PH.rules_file(image)):
        PH.check_file(data, image)
        assert image.size < len(data) <= PH.capacity(96, 250, 3)
    assert native_lib.gsr_png_capacity(0, 4, 3) == 0 and native_lib.gsr_png_capacity(4, 4, 2) == 0
    assert native_lib.gsr_png_workspace_bytes(2, 96, 250, 3) >= 2 * (96 * 751 + 3 * 32768)
    assert native_lib.gsr_png_workspace_bytes(70000, 4, 4, 3) == 0


def test_abi_header_and_symbol_list(native_lib):
    from gscream_amd import _abi, _native
    hdr = _abi.header()
    assert hdr.constants["GSR_ABI_VERSION"] == 9 and _native.ABI_VERSION == 9 and native_lib.gsr_abi_version() == 9
    assert hdr.functions["gsr_png_encode"][0] == "int"
    for name in ("gsr_png_capacity", "gsr_png_workspace_bytes"):
        assert hdr.functions[name][0] == "size_t"
    for name in ("gsr_png_capacity", "gsr_png_workspace_bytes", "gsr_png_encode"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(native_lib, name)
    for name, value, stated in (("GSR_PNG_CHUNK", _native.PNG_CHUNK, 32768), ("GSR_PNG_HEADER_BYTES", _native.PNG_HEADER_BYTES, 16),
                                ("GSR_PNG_FILTER_ADAPTIVE", _native.PNG_FILTER_ADAPTIVE, 5)):
        assert hdr.constants[name] == value == stated
    assert (PH.CHUNK, PH.HEADER, PH.ADAPTIVE) == (_native.PNG_CHUNK, _native.PNG_HEADER_BYTES, _native.PNG_FILTER_ADAPTIVE)
    # rejected before any launch (no device is touched)
    buf = (_native.ctypes.c_uint8 * 64)()
    rc = native_lib.gsr_png_encode(buf, 12, 48, 1, 4, 4, 3, 9, buf, 4096, buf, None)
    assert rc == -1 and b"filter" in native_lib.gsr_last_error()
    rc = native_lib.gsr_png_encode(buf, 12, 48, 1, 4, 4, 3, 5, buf, 16, buf, None)
    assert rc == -1 and b"out_stride" in native_lib.gsr_last_error()
