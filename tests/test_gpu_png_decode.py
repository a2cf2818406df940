"""gscream_amd.png_decode on the device.  Every comparison is equality of bytes: with the source picture and with PIL.  The corpus is
tests/png_decode_helpers.py's; the corrupt files have been through the sanitizer-built host program in tests/test_png_decode.py and are
run here only as a check of the reported codes."""
import numpy as np
import pytest
import torch

from tests import png_decode_helpers as DH
from gscream_amd import png_decode

pytestmark = pytest.mark.gpu

COMBOS = [(c, l) for c in DH.COMPRESSORS for l in DH.LAYOUTS]


def _decode(cases, verify_crc=True):
    pictures = png_decode.decode([c.data for c in cases], "cuda", verify_crc=verify_crc, names=[c.name for c in cases])
    assert png_decode.last_path == "hip"
    return pictures


def _equal(cases, pictures):
    host = [im.cpu().numpy() for im in pictures.images]
    for case, got in zip(cases, host):
        assert got.dtype == np.uint8 and got.shape == case.image.shape, case.name
        assert np.array_equal(got, case.image), case.name
        assert np.array_equal(got, DH.pil_decode(case.data)), case.name


@pytest.mark.parametrize("compressor,layout", COMBOS)
def test_compressor_split_channels(compressor, layout):
    cases = DH.cross(compressor, layout)
    assert len(cases) == 80
    _equal(cases, png_decode.check(_decode(cases)))
    assert png_decode.last_info["files"] == 80


def test_edge_shapes_pil_and_own():
    cases = DH.edge_shapes()
    _equal(cases, png_decode.check(_decode(cases)))


def test_what_zlib_never_emits():
    cases = DH.never_emitted()
    _equal(cases, png_decode.check(_decode(cases)))


def test_own_files_take_the_parallel_path():
    from gscream_amd import png
    images = DH.own_pictures()
    for at in (0, 2):  # two batches of 3 cover the five kinds
        batch = np.stack(images[at:at + 3])
        files = png.to_bytes(png.encode(torch.from_numpy(batch).cuda()))
        assert png.last_path == "hip"
        cases = [DH.Case(f"own{at + k}", data, batch[k], DH.OK) for k, data in enumerate(files)]
        pictures = png_decode.check(_decode(cases))
        _equal(cases, pictures)
        assert png_decode.last_info == {"files": 3, "segments": 9, "parallel": 3, "serial": 0, "host_decoded": 0, "masks_resized": 0}
        assert pictures.paths.cpu().tolist() == [1, 1, 1]


def test_segments_that_do_and_do_not_stand_alone():
    for mode, parallel in (("full", 1), ("sync", 0)):
        cases = DH.flushed(mode)
        pictures = png_decode.check(_decode(cases))
        info = png_decode.last_info
        assert (info["segments"], info["parallel"], info["serial"]) == (15, parallel, 1 - parallel), (mode, info)
        _equal(cases, pictures)


def test_one_call_mixed_sizes_and_one_corrupt_file():
    cases = DH.mixed_sizes()
    _equal(cases, png_decode.check(_decode(cases)))
    bad = [c for c in DH.corrupt() if c.name == "corrupt-distance"]
    mixed = cases[:2] + bad + cases[2:]
    pictures = _decode(mixed)
    with pytest.raises(png_decode.PngError) as e:
        png_decode.check(pictures)
    assert e.value.failures == [(2, DH.DISTANCE)] and (e.value.index, e.value.code) == (2, DH.DISTANCE)
    _equal(cases, png_decode.PngPictures([pictures.images[i] for i in (0, 1, 3)], pictures.status, pictures.paths))


def test_corrupt_files_give_their_codes():
    cases = DH.corrupt()
    assert sorted(c.status for c in cases) == [1, 2, 3, 4, 6, 7, 8, 9, 10, 11]
    pictures = _decode(cases)
    assert pictures.status.cpu().tolist() == [c.status for c in cases], [c.name for c in cases]
    with pytest.raises(png_decode.PngError) as e:
        png_decode.check(pictures)
    assert e.value.failures == [(i, c.status) for i, c in enumerate(cases)]
    (crc,) = [c for c in cases if c.name == "corrupt-crc"]
    _equal([crc], png_decode.check(_decode([crc], verify_crc=False)))


def test_no_host_stop():
    cases = DH.mixed_sizes() + list(DH.flushed("full")) + list(DH.flushed("sync"))
    png_decode.check(_decode(cases))  # (the library is loaded, the LDS opt-in made, the allocator warm)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pictures = _decode(cases)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    _equal(cases, png_decode.check(pictures))


def test_the_consumer(tmp_path):
    from gscream_amd import metrics, png
    from gscream_amd import synthetic as S
    dirs = {k: tmp_path / k for k in ("renders", "gt", "masks")}
    for d in dirs.values():
        d.mkdir()
    H, W = 37, 53
    renders = [S.picture("texture", H, W, 3, seed=k) for k in range(3)]
    gts = [S.picture("texture", H, W, 3, seed=k + 10) for k in range(3)]
    masks = [S.picture("mask", H, W, 1, seed=k) for k in range(3)]
    for k in range(3):
        png.save(torch.from_numpy(renders[k]).cuda(), str(dirs["renders"] / f"{k:05d}.png"))
        png.save(torch.from_numpy(gts[k]).cuda(), str(dirs["gt"] / f"{k:05d}.png"))
        png.save(torch.from_numpy(masks[k]).cuda(), str(dirs["masks"] / ("out_%05d.png" % (k + 1))))
    r, g, names, m = png_decode.read_images(dirs["renders"], dirs["gt"], dirs["masks"])
    assert png_decode.last_path == "hip" and png_decode.last_info["files"] == 9 and png_decode.last_info["host_decoded"] == 0
    assert sorted(names) == [f"{k:05d}.png" for k in range(3)]
    tr, tg, tm = [], [], []
    for i, name in enumerate(names):
        k = int(name[:5])
        assert r[i].shape == g[i].shape == m[i].shape == (1, 3, H, W) and r[i].is_cuda
        assert r[i].dtype == g[i].dtype == torch.float32 and m[i].dtype == torch.bool and m[i].stride(1) == 0
        tr.append(torch.from_numpy(renders[k]).cuda().permute(2, 0, 1)[None].float() / 255.0)
        tg.append(torch.from_numpy(gts[k]).cuda().permute(2, 0, 1)[None].float() / 255.0)
        tm.append(torch.from_numpy(masks[k][..., 0] > 0).cuda()[None, None].expand(1, 3, -1, -1))
        assert torch.equal(r[i], tr[i]) and torch.equal(g[i], tg[i]) and torch.equal(m[i], tm[i])
    got = png_decode.evaluate_files(dirs["renders"], dirs["gt"], dirs["masks"], reader="hip")
    assert metrics.last_path == "hip"
    assert got == metrics.evaluate_views(tr, tg, tm, names)
