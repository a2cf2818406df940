"""gscream_amd.png on the device: every file goes through the decoders of record (PIL, zlib, the chunk parser, the filter bytes) and, where
the picture is small enough for the Python statement of the rules (tests/png_helpers.py rules_file), is compared with it byte for byte."""
import numpy as np
import pytest
import torch

from tests import png_helpers as PH  # noqa: E402
from gscream_amd import synthetic as S

pytestmark = pytest.mark.gpu

THREE_CHUNKS = (96, 250, 3)  # 72 096 bytes of stream: cuts at 32 768 and 65 536, both inside a row of 751


def _encode(image, filter="adaptive", out=None):
    from gscream_amd import png
    images = image if isinstance(image, torch.Tensor) else torch.from_numpy(image).cuda()
    batch = png.encode(images, filter, out=out)
    assert png.last_path == "hip"
    return png.to_bytes(batch)


def _code(filter):
    return PH.ADAPTIVE if filter == "adaptive" else filter


def _check(image, filter="adaptive", model=True):
    (data,) = _encode(image, filter)
    PH.check_file(data, image, _code(filter))
    if model:
        assert data == PH.rules_file(image, _code(filter)), "the device's bytes differ from the rules'"
    return data


@pytest.mark.parametrize("shape", PH.SHAPES + [THREE_CHUNKS])
def test_shapes(shape):
    H, W, C = shape
    _check(S.picture("texture", H, W, C, seed=H + W))


@pytest.mark.parametrize("kind", ["texture", "colormap", "mask", "constant", "noise"])
def test_contents_over_three_chunks(kind):
    H, W, C = THREE_CHUNKS
    image = S.picture(kind, H, W, C, seed=3)
    data = _check(image)
    stream = H * (1 + W * C)
    if kind == "constant":  # runs across the 258 limit and both cuts: >= 2 bits per 258 bytes and a block header per chunk
        assert len(data) <= 0.02 * stream, (len(data), stream)
    if kind == "noise":     # the stored fallback
        assert stream < len(data) <= PH.capacity(H, W, C)


def test_batch_of_different_pictures():
    images = np.stack([S.picture(k, 37, 53, 3, seed=11) for k in ("texture", "mask", "noise")])
    files = _encode(images)
    assert len(files) == 3 and len(set(files)) == 3
    for b, data in enumerate(files):
        PH.check_file(data, images[b])
        assert data == _encode(images[b])[0]


def test_strided_panel_equals_its_dense_copy():
    """The panels of a [H, 4W, 3] sheet are read in place: as single views and as one batch of four."""
    from gscream_amd import png
    H, W = 37, 53
    sheet = torch.from_numpy(np.concatenate([S.picture(k, H, W, 3, seed=5) for k in ("texture", "colormap", "mask", "noise")], 1)).cuda()
    batch = _encode(png._panels(sheet, 4))
    for k in range(4):
        panel = sheet[:, k * W:(k + 1) * W]
        assert not panel.is_contiguous()
        (strided,), (dense,) = _encode(panel), _encode(panel.contiguous())
        assert strided == dense == batch[k]
        PH.check_file(strided, panel.cpu().numpy())


def test_one_distinct_byte_no_repeats_and_the_length_limit():
    zeros = np.zeros((40, 1000, 1), np.uint8)  # filter 0: every byte of both chunks is 0
    assert len(_check(zeros, 0)) <= 0.02 * zeros.size
    ladder, hist = PH.ladder_picture()         # filter 0: no byte equals its neighbour (no distance code), counts on a Fibonacci ladder
    assert PH.unlimited_depth(hist) > 15, "the ladder does not reach the limit"
    toks = PH.tokens(PH.filter_rule(ladder, 0).tobytes())
    assert not any(t[3] for t in toks)
    _check(ladder, 0)


@pytest.mark.parametrize("filter", [0, 1, 2, 3, 4, "adaptive"])
def test_filters(filter):
    _check(S.picture("texture", 37, 53, 4, seed=1), filter)


def test_determinism_paths_one_copy_and_poison(tmp_path, monkeypatch):
    from PIL import Image
    from gscream_amd import png
    image = S.picture("texture", 61, 77, 3, seed=2)
    dev = torch.from_numpy(image).cuda()
    first = _encode(dev)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")  # encode never synchronises
    try:
        again = png.encode(dev)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert png.to_bytes(again) == first
    need = png.HEADER + png.capacity(61, 77, 3)
    out = torch.full((1, (need + 67) & ~3), 0x5A, dtype=torch.uint8, device="cuda")
    batch = png.encode(dev, out=out)
    assert png.last_path == "hip" and batch.data is out
    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(self.shape), real(self, *a, **k))[1])
    (data,) = png.to_bytes(batch)
    monkeypatch.undo()
    assert len(copies) == 1
    PH.check_file(data, image)
    host = out.cpu()
    assert int(host[0, :4].numpy().view("<u4")[0]) == len(data) and bool((host[0, png.HEADER + len(data):] == 0x5A).all())
    path = str(tmp_path / "a.png")
    png.save(dev, path)
    assert np.array_equal(np.asarray(Image.open(path)), image)
    png.force_torch = True
    try:
        png.encode(dev)
        assert png.last_path == "torch"
    finally:
        png.force_torch = False


def test_frames_tuples_to_files(tmp_path):
    from PIL import Image
    from gscream_amd import frames, png
    from tests import frames_helpers as FH
    v = {k: torch.from_numpy(x).cuda() for k, x in FH.view_inputs(23, 31, 5).items()}
    vf = frames.view_frames(v["render"], v["uncertainty"], v["gt"], v["depth"], v["midas"], v["mask"])
    paths = [str(tmp_path / f"v{k}.png") for k in range(5)]
    png.save_view_frames(vf, paths)
    assert png.last_path == "hip"
    for path, want in zip(paths, (vf.render, vf.uncertainty, vf.error, vf.gt, vf.depth)):
        assert np.array_equal(np.asarray(Image.open(path)), want.cpu().numpy())
    fr = frames.rgbd_frame(v["render"], v["depth"], v["uncertainty"], v["normals"], panels=True)
    paths = [str(tmp_path / f"r{k}.png") for k in range(5)]
    png.save_rgbd_frame(fr, paths)
    for path, want in zip(paths, fr):
        assert np.array_equal(np.asarray(Image.open(path)), want.cpu().numpy())


@pytest.mark.parametrize("kind", ["texture", "colormap", "mask"])
def test_size_against_the_zlib_rle_model(kind):
    """The reference is zlib's Z_RLE strategy on the same filtered bytes and cuts.  Both sides code the same tokens with a Huffman
    code that is optimal unless the length limit binds, so the device may exceed the reference only by the construction of the
    limited code and of the block header (INTEGRATION U names the margin: 0.5 % and 8 bytes per chunk).  A missing run detector
    or fixed codes would cost tens of percent.  Measured on an MI355X: see the table in INTEGRATION U."""
    H, W, C = 189, 336, 3
    image = S.picture(kind, H, W, C, seed=4)
    data = _check(image, model=False)
    ref = PH.rle_model_size(image)
    chunks = -(-H * (1 + W * C) // PH.CHUNK)
    print(f"png size {kind}: device {len(data)} reference {ref} ratio {len(data) / ref:.4f} chunks {chunks}")
    assert len(data) <= 1.005 * ref + 8 * chunks, (len(data), ref)


def test_full_size_sheet_round_trips():
    image = np.concatenate([S.picture(k, 567, 1008, 3, seed=6) for k in ("texture", "colormap", "mask", "texture")], 1)
    assert image.shape == (567, 4032, 3)
    _check(image, model=False)
