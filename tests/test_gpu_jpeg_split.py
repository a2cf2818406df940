"""The split JPEG decode on the device (include/gsraster_jpeg_split.h).  Pictures are compared with PIL's byte for byte; the
per-subsequence entry states and counts the device reports (the trace) and its per-file counts are compared with the rules' statement in
tests/jpeg_split_helpers.py, exactly: the device is held to the rule itself, not to the picture only.

Every device buffer of a call -- pictures, status and counts, workspace, trace -- is a body of tests/arena_helpers.py's poisoned arena,
and the library is called through its LibProxy with this family's and the decode family's parameter tables: a writable pointer outside
a body, a changed const input or a changed guard byte fails the test."""
import contextlib

import numpy as np
import pytest
import torch

from tests import arena_helpers as AH
from tests import jpeg_decode_helpers as DH
from tests import jpeg_helpers as JH
from tests import jpeg_split_helpers as SH
from gscream_amd import _abi, _native, jpeg_decode, video

pytestmark = pytest.mark.gpu

POISON = 0xA5
DEFAULT = jpeg_decode.DEFAULT_SUBSEQUENCE_BYTES


@contextlib.contextmanager
def guarded(monkeypatch, nbytes=48 << 20):
    """Inside: every buffer jpeg_decode.decode allocates is an arena body and every native call goes through the proxy.
    Yields (arena, proxy); on a clean exit the guard bands are checked."""
    jpeg_decode._split_library()  # (typed from the real library, before the proxy stands in)
    table = {name: params for header in (jpeg_decode.HEADER, jpeg_decode.SPLIT_HEADER) for name, (_, params) in _abi.extension(header).functions.items()}
    arena = AH.Arena(nbytes, POISON, "cuda")
    proxy = AH.LibProxy(_native.load(), arena, table)
    with monkeypatch.context() as m:
        m.setattr(_native, "_lib", proxy)
        m.setattr(jpeg_decode, "_device_bytes", lambda n, device, what: arena.alloc_bytes(n, what))
        yield arena, proxy
    arena.check()


def _rows(pictures):
    """The trace and the counts, read back: (rows used [n, 5], info [files, 4])."""
    info = pictures.info.cpu().numpy()
    return pictures.trace.cpu().numpy()[:int(info[:, 2].sum())], info


def _model_rows(cases, B, min_bytes=0):
    models = [SH.model(c.data, B, min_bytes) for c in cases]
    rows = [row for m in models for interval in m.rows for row in interval]
    return np.array(rows, np.int64).reshape(-1, 5), np.array([m.info for m in models], np.int64)


@pytest.fixture(scope="module")
def batches():
    out = SH.mixed_batches(SH.corpus())
    assert len(out) == 4 and all(len({c.image.shape for c in b}) >= 5 for b in out)  # mixed sizes in every call
    return out


@pytest.mark.parametrize("B", sorted({16, DEFAULT}))
def test_pictures_equal_pil_in_mixed_batches(monkeypatch, batches, B):
    for batch in batches:
        with guarded(monkeypatch) as (arena, proxy):
            pictures = jpeg_decode.check(jpeg_decode.decode([c.data for c in batch], "cuda", [c.name for c in batch], split="always", subsequence_bytes=B))
            assert jpeg_decode.last_path == "hip" and proxy.calls == {"gsr_jpeg_decode_split": 1}
            assert sorted(arena.names) == ["out", "status", "workspace"]
            assert pictures.status.cpu().tolist() == [0] * len(batch) and pictures.decoded.cpu().tolist() == list(pictures.intervals)
            for case, image in zip(batch, pictures.images):
                assert np.array_equal(image.cpu().numpy(), case.image), case.name
        assert jpeg_decode.last_info["repaired_intervals"] == 0


def test_the_trace_and_the_counts_are_the_rule(monkeypatch, batches):
    """Every subsequence's (bit, j, k, first_block, blocks) and every file's counts equal the model's, exactly; nothing is repaired, and
    every interval of at least two subsequences is split (the model's number of eligible intervals)."""
    shifted = SH.shifted_case(16)
    assert SH.on_a_stuffed_zero(shifted.data, 16)  # a nominal beginning on the 00 of an FF 00 pair is among the files
    assert any(shifted is c for b in batches for c in b)
    chunks = 0
    for batch in batches:
        with guarded(monkeypatch):
            pictures = jpeg_decode.decode([c.data for c in batch], "cuda", split="always", subsequence_bytes=16, trace=True)
            rows, info = _rows(pictures)
        want_rows, want_info = _model_rows(batch, 16)
        assert np.array_equal(info, want_info), [c.name for c, a, b in zip(batch, info, want_info) if tuple(a) != tuple(b)][:4]
        assert (info[:, 1] == 0).all()
        assert rows.shape == want_rows.shape and np.array_equal(rows, want_rows), np.flatnonzero((rows != want_rows).any(1))[:8]
        jpeg_decode.check(pictures)
        assert jpeg_decode.last_info["split_intervals"] == int(want_info[:, 0].sum()) and jpeg_decode.last_info["subsequences"] == rows.shape[0]
        chunks = max(chunks, int(info[:, 3].max()))
        for case, image in zip(batch, pictures.images):
            assert np.array_equal(image.cpu().numpy(), case.image), case.name
    assert chunks >= 3  # several chunks in one interval: the walk across chunks ran


def test_corrupt_files_get_the_serial_status_and_leave_their_neighbours_alone(monkeypatch, batches):
    valid = batches[1][:12]
    rgb = JH.picture("texture", 17, 23, 3, seed=5)
    plain, marked = DH.pil_encode(rgb, 50, 2), DH.pil_encode(rgb, 50, 2, restart_marker_rows=1)
    h = DH.header(plain)
    bad = [plain[:cut] for cut in range(h["scan"], len(plain))]  # a cut at every byte of the scan
    for byte in range(h["scan"], len(plain) - 2):  # one bit flip per byte of it, the bit walking with the byte
        flipped = bytearray(plain)
        flipped[byte] ^= 1 << ((byte * 3) & 7)
        bad.append(bytes(flipped))
    k = DH._rst_positions(marked, DH.header(marked))[0]
    renumbered = bytearray(marked)
    renumbered[k + 1] = 0xD0 + ((renumbered[k + 1] + 1) & 7)
    bad += [marked[:k] + marked[k + 2:], bytes(renumbered)]  # a removed and a renumbered RSTm
    files, where = [], []
    for i, data in enumerate(bad):  # a valid file between every 30 corrupt ones
        if i % 30 == 0:
            files.append(valid[(i // 30) % len(valid)])
        where.append(len(files))
        files.append(DH.Case(f"corrupt {i}", data, None))
    blobs = [c.data for c in files]
    codes = {}
    for split in ("never", "always"):
        with guarded(monkeypatch):
            pictures = jpeg_decode.decode(blobs, "cuda", split=split, subsequence_bytes=16)
            codes[split] = pictures.status.cpu().tolist()
            for case, image in zip(files, pictures.images):
                if case.image is not None:  # the valid pictures are what they are without the corrupt neighbours
                    assert np.array_equal(image.cpu().numpy(), case.image), (split, case.name)
        if split == "always":
            info = pictures.info.cpu().numpy()
    assert codes["always"] == codes["never"]
    assert all(codes["never"][i] == 0 for i in range(len(files)) if i not in set(where))
    flips = [codes["never"][i] for i in where[len(plain) - h["scan"]:-2]]
    assert all(codes["never"][i] != 0 for i in where[:len(plain) - h["scan"]]) and any(flips) and codes["never"][where[-1]] == codes["never"][where[-2]] == DH.RESTART
    # (a cut file has no closing marker and never reaches the split; the flipped ones do, and the failing ones go to the serial kernel)
    assert info[:, 0].sum() > len(bad) // 4 and info[:, 1].sum() > 10


def test_auto_splits_the_intervals_of_min_bytes_and_no_others(monkeypatch):
    rgb = JH.picture("noise", 48, 48, 3, seed=3)
    plain, marked = DH.pil_encode(rgb, 100, 2), DH.pil_encode(rgb, 100, 2, restart_marker_rows=1)
    lengths = [[len(iv.seg) for iv in SH.serial(d)] for d in (plain, marked)]
    least = (max(lengths[1]) + lengths[0][0]) // 2
    assert len(lengths[0]) == 1 and len(lengths[1]) == 3 and max(lengths[1]) < least < lengths[0][0] and min(lengths[1]) > 2 * 16
    with guarded(monkeypatch):
        pictures = jpeg_decode.check(jpeg_decode.decode([plain, marked], "cuda", split="auto", subsequence_bytes=16, min_bytes=least, trace=True))
        rows, info = _rows(pictures)
    want_rows, want_info = _model_rows([DH.Case("plain", plain, None), DH.Case("marked", marked, None)], 16, least)
    assert info.tolist() == want_info.tolist() and info[0, 0] == 1 and info[1].tolist() == [0, 0, 0, 0]
    assert np.array_equal(rows, want_rows)
    for data, image in zip((plain, marked), pictures.images):
        assert np.array_equal(image.cpu().numpy(), DH.pil_decode(data))
    assert jpeg_decode.last_info["split_intervals"] == 1 and jpeg_decode.last_info["intervals"] == 4


def test_two_calls_give_identical_pictures_trace_and_counts(monkeypatch, batches):
    batch, runs = batches[2], {}
    for run in ("first", "second"):
        with guarded(monkeypatch):
            pictures = jpeg_decode.check(jpeg_decode.decode([c.data for c in batch], "cuda", split="always", subsequence_bytes=16, trace=True))
            rows, info = _rows(pictures)
            runs[run] = {"trace": rows, "info": info, **{c.name: image.cpu().numpy() for c, image in zip(batch, pictures.images)}}
    AH.assert_same_bits(runs, "split decode")


def test_never_is_the_decode_entry_and_the_default_is_what_the_module_says(monkeypatch, batches):
    batch = batches[0][:8]
    for kwargs, want in (({"split": "never"}, "gsr_jpeg_decode"), ({}, "gsr_jpeg_decode" if jpeg_decode.DEFAULT_SPLIT == "never" else "gsr_jpeg_decode_split")):
        with guarded(monkeypatch) as (arena, proxy):
            pictures = jpeg_decode.check(jpeg_decode.decode([c.data for c in batch], "cuda", **kwargs))
            assert proxy.calls == {want: 1}
            for case, image in zip(batch, pictures.images):
                assert np.array_equal(image.cpu().numpy(), case.image), case.name


def test_mjpeg_reader_passes_split_through(tmp_path):
    frames = torch.from_numpy(np.stack([JH.picture("texture", 48, 48, 3, seed=k) for k in range(3)]))
    path = str(tmp_path / "three.avi")
    with video.MjpegWriter(path, 48, 48, fps=25) as writer:
        writer.add(frames.cuda())
    reader = video.MjpegReader(path)
    plain = [f.cpu().numpy() for f in reader.frames("cuda")]
    split = [f.cpu().numpy() for f in reader.frames("cuda", split="always")]
    assert jpeg_decode.last_info["split_intervals"] > 0 and jpeg_decode.last_info["repaired_intervals"] == 0
    assert len(plain) == len(split) == 3 and all(np.array_equal(a, b) for a, b in zip(plain, split))
    with pytest.raises(ValueError, match="split"):
        list(reader.frames("cuda", split="sometimes"))


def test_one_picture_of_near_production_size_at_the_shipped_defaults(monkeypatch):
    rgb = JH.picture("texture", 567, 1008, 3, seed=11)
    data = DH.pil_encode(rgb, 90, 2)
    with guarded(monkeypatch, 96 << 20):
        pictures = jpeg_decode.check(jpeg_decode.decode([data], "cuda", split="always" if jpeg_decode.DEFAULT_SPLIT == "never" else jpeg_decode.DEFAULT_SPLIT))
        got = pictures.images[0].cpu().numpy()
    assert jpeg_decode.last_info["split_intervals"] == 1 and jpeg_decode.last_info["repaired_intervals"] == 0
    assert jpeg_decode.last_info["subsequences"] == len(SH.beginnings(SH.segments(data)[0], DEFAULT))
    assert np.array_equal(got, DH.pil_decode(data))
