"""The split JPEG decode (include/gsraster_jpeg_split.h) without a GPU: the family's header and exports, the rules' statement in
tests/jpeg_split_helpers.py against itself and against the serial statement of tests/jpeg_decode_helpers.py, the core of
gscream_amd/csrc/jpeg_split.h -- the code the kernels run -- compiled into tools/jpeg_split_check.cpp with AddressSanitizer and
UndefinedBehaviorSanitizer and run as a stand-alone program over the generated corpus and the corrupt files, and the Python surface."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import jpeg_decode_helpers as DH
from tests import jpeg_split_helpers as SH
from gscream_amd import _abi, _native, jpeg_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_split_header_parses_and_the_library_exports_it(native_lib):
    main, dec, ext = _abi.header(), _abi.extension(jpeg_decode.HEADER), _abi.extension(jpeg_decode.SPLIT_HEADER)
    assert jpeg_decode.SPLIT_HEADER == "gsraster_jpeg_split.h" and ext is jpeg_decode._SPLIT_ABI
    assert list(ext.functions) == ["gsr_jpeg_split_workspace_bytes", "gsr_jpeg_decode_split"] == list(jpeg_decode.SPLIT_EXPORTED_SYMBOLS)
    for name in ext.functions:
        assert hasattr(native_lib, name), name
    # the main header and the decode header are what they were
    assert _native.EXPORTED_SYMBOLS == tuple(main.functions) and main.constants["GSR_ABI_VERSION"] == native_lib.gsr_abi_version()
    assert list(dec.functions) == ["gsr_jpeg_decode_workspace_bytes", "gsr_jpeg_decode", "gsr_jpeg_decode_status_name"] == list(jpeg_decode.EXPORTED_SYMBOLS)
    assert not set(ext.functions) & (set(main.functions) | set(dec.functions)) and not ext.constants
    # the arguments of gsr_jpeg_decode, then the family's own, the stream last
    mine = [p[1] for p in ext.functions["gsr_jpeg_decode_split"][1]]
    base = [p[1] for p in dec.functions["gsr_jpeg_decode"][1]]
    assert mine == base[:-1] + ["subsequence_bytes", "min_bytes", "trace", "info", "stream"] and base[-1] == "stream"
    assert [p[1] for p in ext.functions["gsr_jpeg_split_workspace_bytes"][1]] == ["area_bytes", "nfiles", "nintervals", "scan_bytes", "subsequence_bytes"]
    assert ext.structs == {"gsr_jpeg_split_trace": [("int32_t", f, None) for f in ("bit", "j", "k", "first_block", "blocks")]}
    lib = jpeg_decode._split_library()
    front = lib.gsr_jpeg_decode_workspace_bytes(1000, 2, 10)
    assert lib.gsr_jpeg_split_workspace_bytes(1000, 2, 10, 4096, 16) >= front + 4 * (7 * 10 + 4 * (4096 // 16 + 10))
    for bad in (0, 8, 24, 2048, -16):
        assert lib.gsr_jpeg_split_workspace_bytes(1000, 2, 10, 4096, bad) == 0
    assert lib.gsr_jpeg_split_workspace_bytes(1000, 0, 10, 4096, 16) == 0 and lib.gsr_jpeg_split_workspace_bytes(1000, 2, 10, 1 << 32, 16) == 0


def test_the_model_is_self_consistent_at_16_bytes():
    """From the model's entry state every subsequence decodes to the serial decoder's coefficients and ends in the next one's entry
    state, and the DC prefix over the stored differences gives the serial decoder's DC values."""
    B, split, shifted = 16, 0, 0
    for case in SH.corpus():
        want = DH.coefficients(case.data).astype(np.int64)
        at = 0
        for iv in SH.serial(case.data):
            rows, begins = SH.entry_rows(iv, B)
            assert len(rows) == len(SH.beginnings(iv.seg, B)) >= 1
            got = np.zeros_like(iv.diff)

            def sink(b, k, v):
                got[b, DH.ZIGZAG[k]] = v
            for i, (bit, j, k, first, blocks) in enumerate(rows):
                assert bit >= begins[i] and (i + 1 == len(rows) or bit - begins[i] < 8 * B + 27), (case.name, i)
                exit_state, begun = SH.run(iv, (bit, j, k), begins[i + 1] if i + 1 < len(rows) else None, first, sink)
                assert begun == blocks, (case.name, i)
                assert exit_state == (rows[i + 1][:3] if i + 1 < len(rows) else iv.final), (case.name, i)
            assert np.array_equal(got, iv.diff), case.name
            assert np.array_equal(SH.dc_prefix(got, iv.ny, iv.bpm), want[at:at + iv.nblocks]), case.name
            at += iv.nblocks
            split += len(rows) >= 2
        assert at == want.shape[0]
        shifted += SH.on_a_stuffed_zero(case.data, B)
    assert split > len(SH.corpus()) and shifted >= 1
    case = SH.shifted_case(B)
    assert SH.on_a_stuffed_zero(case.data, B) and any(len(r) >= 2 for r in SH.model(case.data, B).rows)


def test_the_beginnings_shift_behind_ff_and_none_is_empty():
    seg = bytes(15) + b"\xff\x00" + bytes(14) + b"\xff\x00"
    assert SH.beginnings(seg, 16) == [0, 17]  # 16 is the stuffed 00; the one that would begin at 33 = the end is none
    assert SH.beginnings(bytes(32), 16) == [0, 16] and SH.beginnings(bytes(33), 16) == [0, 16, 32] and SH.beginnings(bytes(5), 16) == [0]
    assert SH.destuffed_bit(seg, 17) == 8 * 16


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/jpeg_split_check.cpp built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tools/jpeg_split_check.cpp")
    exe = str(tmp_path_factory.mktemp("jpeg_split_check") / "jpeg_split_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "jpeg_split_check.cpp"), "-o", exe], check=True)
    return exe


def _run_checker(checker, options, cases, folder):
    paths = []
    for k, case in enumerate(cases):
        paths.append(str(folder / f"{k:05d}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(case.data)
    lines = []
    for at in range(0, len(paths), 500):
        run = subprocess.run([checker] + options + paths[at:at + 500], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]  # (a sanitizer report is on stderr and ends the program)
        lines += run.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    out = []
    for case, path, line in zip(cases, paths, lines):
        m = re.fullmatch(re.escape(path) + r" status=(\d+) serial=(\d+) digest=([0-9a-f]{8}) serial_digest=([0-9a-f]{8}) split=(\d+) repaired=(\d+) "
                         r"subsequences=(\d+)", line)
        assert m, (case.name, line)
        out.append(tuple(int(m.group(i), 16 if i in (3, 4) else 10) for i in range(1, 8)))
    return out


@pytest.mark.parametrize("options", (["-b", "16", "-s", "4"], ["-b", "64", "-s", "256"]), ids=("b16-s4", "b64-s256"))
def test_sanitized_split_core_equals_the_serial_core_on_the_valid_corpus(checker, tmp_path, options):
    cases = DH.corpus() + SH.corpus()
    split_files = 0
    for case, (code, serial, digest, serial_digest, split, repaired, subs) in zip(cases, _run_checker(checker, options, cases, tmp_path)):
        assert code == serial == DH.OK, (case.name, code, serial)
        assert digest == serial_digest == DH.digest(DH.coefficients(case.data)), case.name
        assert repaired == 0, case.name  # no hidden fallback: the chain converges on a valid stream
        want = SH.model(case.data, int(options[1])).info
        assert (split, subs) == (want[0], want[2]), case.name
        split_files += split > 0
    assert split_files > len(cases) // 5  # (a file of a few hundred bytes is one subsequence of 64)


def test_sanitized_split_core_gives_every_corrupt_file_the_serial_code(checker, tmp_path):
    cases = DH.corrupt()
    seen, split_files, repaired_files = set(), 0, 0
    for case, (code, serial, digest, serial_digest, split, repaired, _) in zip(cases, _run_checker(checker, ["-b", "16", "-s", "4"], cases, tmp_path)):
        assert code == serial == DH.status(case.data) != DH.OK and digest == serial_digest == 0, (case.name, code, serial)
        seen.add(code)
        split_files += split > 0
        repaired_files += repaired > 0
    assert {DH.TRUNCATED, DH.RESTART, DH.BAD_CODE} <= seen and split_files > 100 and repaired_files > 50


def test_split_arguments_are_checked_before_anything_runs():
    data = SH.corpus()[0].data
    for bad in ("sometimes", None, True, ""):
        with pytest.raises(ValueError, match="split"):
            jpeg_decode.decode([data], "cpu", split=bad)
        with pytest.raises(ValueError, match="split"):
            jpeg_decode.read([], "cpu", split=bad)
    for bad in (0, 8, 15, 24, 2048, -16, 16.0, "16", True):
        with pytest.raises(ValueError, match="subsequence_bytes"):
            jpeg_decode.decode([data], "cpu", split="always", subsequence_bytes=bad)
    for bad in (-1, 1 << 31, 1.5):
        with pytest.raises(ValueError, match="min_bytes"):
            jpeg_decode.decode([data], "cpu", split="auto", min_bytes=bad)
    assert jpeg_decode.SPLITS == ("never", "auto", "always") and jpeg_decode.DEFAULT_SPLIT in jpeg_decode.SPLITS
    B = jpeg_decode.DEFAULT_SUBSEQUENCE_BYTES
    assert 16 <= B <= 1024 and B & (B - 1) == 0 and jpeg_decode.DEFAULT_MIN_BYTES >= 0
    # the CPU path is what it was under every value
    for split in jpeg_decode.SPLITS:
        pictures = jpeg_decode.check(jpeg_decode.decode([data], "cpu", split=split, subsequence_bytes=16))
        assert jpeg_decode.last_path == "torch" and np.array_equal(pictures.images[0].numpy(), SH.corpus()[0].image)
        assert jpeg_decode.last_info == {"files": 1, "intervals": 1, "host_decoded": 0}  # (the counts of a split decode come from the device alone)


def test_never_calls_the_decode_entry_and_the_others_the_split_entry(monkeypatch):
    """A stub in place of the launch: `split="never"` is today's call into gsr_jpeg_decode with today's arguments; the other two call
    gsr_jpeg_decode_split.  (The stub stops the call at the launch; everything in front of it runs on host tensors.)"""
    import contextlib
    import torch

    class Launched(Exception):
        pass
    seen = []

    def run(name, device, *args):
        seen.append((name, len(args)))
        raise Launched(name)
    monkeypatch.setattr(jpeg_decode._native, "run", run)
    monkeypatch.setattr(jpeg_decode._native, "ptr", lambda t: t.data_ptr())
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(jpeg_decode, "_device_bytes", lambda n, device, what: torch.empty(n, dtype=torch.uint8))
    real_to = torch.Tensor.to
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self if a and isinstance(a[0], torch.device) and a[0].type == "cuda" else real_to(self, *a, **k))
    data = SH.corpus()[0].data
    dec = len(_abi.extension(jpeg_decode.HEADER).functions["gsr_jpeg_decode"][1]) - 1  # (run appends the stream)
    ext = len(_abi.extension(jpeg_decode.SPLIT_HEADER).functions["gsr_jpeg_decode_split"][1]) - 1
    for split, want in (("never", ("gsr_jpeg_decode", dec)), ("auto", ("gsr_jpeg_decode_split", ext)), ("always", ("gsr_jpeg_decode_split", ext))):
        del seen[:]
        with pytest.raises(Launched):
            jpeg_decode.decode([data], "cuda", split=split)
        assert seen == [want], split
    del seen[:]
    with pytest.raises(Launched):
        jpeg_decode.decode([data], "cuda")  # and the default is one of them, by its name
    assert seen == [("gsr_jpeg_decode", dec) if jpeg_decode.DEFAULT_SPLIT == "never" else ("gsr_jpeg_decode_split", ext)]
