"""gscream_amd.jpeg_decode on the device.  Every comparison is equality of bytes with PIL's decode of the same file.  The corpus is
tests/jpeg_decode_helpers.py's; the corrupt files have been through the sanitizer-built host program in tests/test_jpeg_decode.py and
are data for the decoder's bounds checks here: the check is of the reported codes and of the guard bands.

tests/arena_helpers.py knows the main header only, so these tests bring their own guard bands: every device buffer of a call -- the
pictures, the status words, the workspace -- is cut out of a larger allocation filled with a poison byte, and the bands on both sides
are compared with it afterwards."""
import contextlib

import numpy as np
import pytest
import torch

from tests import jpeg_decode_helpers as DH
from tests import jpeg_helpers as JH
from gscream_amd import jpeg, jpeg_decode, video

pytestmark = pytest.mark.gpu

BAND, POISON = 4096, 0xA5


@contextlib.contextmanager
def guarded():
    """Inside: every buffer jpeg_decode.decode allocates lies between two bands of POISON.  Yields the list of (what, whole, n);
    check(list) synchronises and compares the bands."""
    taken = []
    plain = jpeg_decode._device_bytes

    def banded(n, device, what):
        whole = torch.full((BAND + ((n + 15) & ~15) + BAND,), POISON, dtype=torch.uint8, device=device)
        taken.append((what, whole, n))
        return whole[BAND:BAND + n]
    jpeg_decode._device_bytes = banded
    try:
        yield taken
    finally:
        jpeg_decode._device_bytes = plain


def bands_intact(taken):
    torch.cuda.synchronize()
    assert sorted(what for what, _, _ in taken) == sorted(["out", "status", "workspace"] * (len(taken) // 3)) and taken
    for what, whole, n in taken:
        assert bool((whole[:BAND] == POISON).all()), f"{what}: the band in front was written"
        assert bool((whole[BAND + n:] == POISON).all()), f"{what}: the band behind was written"


def _out_buffer(taken, call=-1):
    return [whole[BAND:BAND + n] for what, whole, n in taken if what == "out"][call]


def _pictures_of(buffer, cases):
    """the call's one picture buffer, read back once -> the pictures (each at the next multiple of 16)"""
    host = buffer.cpu().numpy()
    out, at = [], 0
    for case in cases:
        H, W, C = case.image.shape
        out.append(host[at:at + H * W * C].reshape(H, W, C))
        at += (H * W * C + 15) & ~15
    return out


def _decode(cases):
    pictures = jpeg_decode.decode([c.data for c in cases], "cuda", names=[c.name for c in cases])
    assert jpeg_decode.last_path == "hip"
    return pictures


def test_the_whole_corpus_in_mixed_batches_equals_pil():
    cases = DH.corpus()
    batches = DH.mixed_batches(cases)
    assert sum(len(b) for b in batches) == len(cases) == 6825
    files = intervals = 0
    for batch in batches:
        assert len({c.image.shape for c in batch}) > 8  # mixed sizes in every call
        with guarded() as taken:
            pictures = jpeg_decode.check(_decode(batch))
            bands_intact(taken)
        files += jpeg_decode.last_info["files"]
        intervals += jpeg_decode.last_info["intervals"]
        assert pictures.decoded.cpu().tolist() == list(pictures.intervals)
        for case, got, view in zip(batch, _pictures_of(_out_buffer(taken), batch), pictures.images):
            assert tuple(view.shape) == case.image.shape and view.dtype == torch.uint8
            assert np.array_equal(got, case.image), case.name
    assert files == 6825 and intervals == sum(jpeg_decode.parse(c.data).intervals for c in cases)


def test_a_second_run_gives_identical_bytes():
    batch = DH.mixed_batches(DH.corpus())[3]
    with guarded() as taken:
        jpeg_decode.check(_decode(batch))
        jpeg_decode.check(_decode(batch))
        bands_intact(taken)
    first, second = _pictures_of(_out_buffer(taken, 0), batch), _pictures_of(_out_buffer(taken, 1), batch)
    for case, a, b in zip(batch, first, second):
        assert np.array_equal(a, b) and np.array_equal(a, case.image), case.name


def test_no_host_stop():
    batch = DH.mixed_batches(DH.corpus())[5]
    jpeg_decode.check(_decode(batch))  # (the library is loaded, the allocator warm)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pictures = _decode(batch)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    jpeg_decode.check(pictures)
    for case, image in zip(batch, pictures.images):
        assert np.array_equal(image.cpu().numpy(), case.image), case.name


def test_corrupt_files_end_in_codes_and_leave_their_neighbours_alone():
    valid = DH.mixed_batches(DH.corpus())[7][:24]
    kinds = {}
    for case in DH.corrupt():  # one of each kind and writer: a cut at the first, a middle and the last byte, flips, the three marker faults
        tag, what = case.name.split("-", 1)
        key = (tag, "cut" if what.startswith("cut") else "flip" if what.startswith("flip") else what)
        kinds.setdefault(key, []).append(case)
    bad = []
    for key, cases in sorted(kinds.items()):
        bad += [cases[0], cases[len(cases) // 2], cases[-1]] if key[1] == "cut" else cases[::5] if key[1] == "flip" else cases
    bad += [c for c in DH.corrupt() if DH.status(c.data) not in (DH.TRUNCATED, DH.RESTART) and c not in bad]  # and every rarer code
    assert {k[1] for k in kinds} == {"cut", "flip", "rst-removed", "rst-duplicated", "rst-renumbered"} and len(bad) >= 36
    mixed, where = [], []
    for k, case in enumerate(valid):  # the corrupt files between the valid ones
        mixed.append(case)
        take = bad[k * len(bad) // len(valid):(k + 1) * len(bad) // len(valid)]
        where += range(len(mixed), len(mixed) + len(take))
        mixed += take
    assert len(where) == len(bad)
    # (a corrupt file's picture has the size its header says: the reference picture of the right shape stands in for the offsets)
    shapes = [c if c.image is not None else DH.Case(c.name, c.data, np.zeros(jpeg_decode.parse(c.data)[:3], np.uint8)) for c in mixed]
    with guarded() as taken:
        pictures = _decode(mixed)
        with pytest.raises(jpeg_decode.JpegDecodeError) as e:
            jpeg_decode.check(pictures)
        bands_intact(taken)
    codes = pictures.status.cpu().tolist()
    assert [i for i, c in enumerate(codes) if c] == where == [i for i, _ in e.value.failures]
    for i in where:
        assert codes[i] != DH.OK and codes[i] == DH.status(mixed[i].data), (mixed[i].name, codes[i])
    assert e.value.failures == [(i, codes[i]) for i in where] and (e.value.index, e.value.code) == (where[0], codes[where[0]])
    for case, got in zip(mixed, _pictures_of(_out_buffer(taken), shapes)):
        if case.image is not None:  # the valid pictures are what they are without the corrupt neighbours
            assert np.array_equal(got, case.image), case.name


@pytest.mark.parametrize("subsampling", ["4:4:4", "4:2:0"])
@pytest.mark.parametrize("restart_interval", [None, 1])
def test_encode_on_the_device_then_decode_on_the_device(subsampling, restart_interval):
    images = np.stack([JH.picture(kind, 33, 47, 3, seed=9) for kind in ("texture", "edges", "ramp")])
    files = jpeg.to_bytes(jpeg.encode(torch.from_numpy(images).cuda(), 90, subsampling, restart_interval))
    assert jpeg.last_path == "hip" and len(files) == 3
    cases = [DH.Case(f"own{k}", data, DH.pil_decode(data)) for k, data in enumerate(files)]
    with guarded() as taken:
        pictures = jpeg_decode.check(_decode(cases))
        bands_intact(taken)
    mcu = 16 if subsampling == "4:2:0" else 8
    rows, columns = -(-33 // mcu), -(-47 // mcu)
    assert list(pictures.intervals) == [rows * columns if restart_interval else rows] * 3
    for case, image in zip(cases, pictures.images):
        assert np.array_equal(image.cpu().numpy(), case.image), case.name


def test_writer_then_reader_equals_pil_frame_by_frame(tmp_path):
    frames = torch.from_numpy(np.stack([JH.picture("texture", 32, 48, 3, seed=k) for k in range(4)])).cuda()
    path = str(tmp_path / "spiral.avi")
    with video.MjpegWriter(path, 48, 32, fps=25) as w:
        w.add(frames)
    reader = video.MjpegReader(path)
    assert (reader.W, reader.H, reader.fps, len(reader)) == (48, 32, 25.0, 4)
    got = list(reader.frames("cuda", batch=3))
    assert jpeg_decode.last_path == "hip" and len(got) == 4
    for k, image in enumerate(got):
        assert image.is_cuda and np.array_equal(image.cpu().numpy(), DH.pil_decode(reader.frame_bytes(k))), k
    again = video.read_rgbd_video(path, "cuda")
    assert all(torch.equal(a, b) for a, b in zip(again, got))


def test_full_size_pair():
    image = JH.picture("texture", 567, 1008, 3, seed=1)
    (own,) = jpeg.to_bytes(jpeg.encode(torch.from_numpy(image).cuda(), 95, "4:4:4"))
    cases = [DH.Case("pil-567x1008", (data := DH.pil_encode(image, 95, 2)), DH.pil_decode(data)), DH.Case("own-567x1008", own, DH.pil_decode(own))]
    with guarded() as taken:
        pictures = jpeg_decode.check(_decode(cases))
        bands_intact(taken)
    assert list(pictures.intervals) == [1, 71] and jpeg_decode.last_info == {"files": 2, "intervals": 72, "host_decoded": 0}
    for case, image in zip(cases, pictures.images):
        assert np.array_equal(image.cpu().numpy(), case.image), case.name
