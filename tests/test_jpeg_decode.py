"""CPU tests of gscream_amd.jpeg_decode: the rules of include/gsraster_jpeg_decode.h, stated in numpy in tests/jpeg_decode_helpers.py,
against PIL byte for byte on the whole corpus (this is what pins the rules, 4:2:2 included, to libjpeg-turbo's decoder); the host
parser on the corpus and on the rejected kinds; the family's header, its exports and their types; the entropy core of
gscream_amd/csrc/jpeg_entropy.h -- the code the kernels run -- compiled into tools/jpeg_entropy_check.cpp with AddressSanitizer and
UBSan and run as a child process over the valid and the corrupt corpus; video.MjpegReader on a file of MjpegWriter's host path.
Nothing is loaded into Python under a sanitizer."""
import ctypes
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpeg_decode_helpers as DH
from tests import jpeg_helpers as JH
from gscream_amd import _abi, _native, jpeg_decode, video

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rules_in_numpy_equal_pil_on_the_whole_corpus():
    cases = DH.corpus()
    assert len(cases) == 13 * 5 * (96 + 9)
    for case in cases:  # no case skipped, no tolerance
        got = DH.decode(case.data)
        assert got.dtype == np.uint8 and got.shape == case.image.shape, case.name
        assert np.array_equal(got, case.image), case.name
    names = " ".join(c.name for c in cases)
    for word in ("-s0", "-s1", "-s2", "-grey", "-opt", "-rb1", "-rr1", "q10-", "q100-", "own-", "ri0", "ri1", "riNone", "15x1-", "48x48-"):
        assert word in names


def test_parse_accepts_the_corpus_and_the_host_path_is_pil():
    cases = DH.corpus()
    for case in cases:
        p = jpeg_decode.parse(case.data, case.name)
        h = DH.header(case.data)
        g = DH.geometry(h)
        assert (p.H, p.W, p.C) == case.image.shape and (p.hs, p.vs, p.dri, p.scan) == (h["hs"], h["vs"], h["dri"], h["scan"]), case.name
        assert p.intervals == g["intervals"] and p.blocks == g["mcus"] * g["bpm"], case.name
        for c in range(p.C):
            assert np.array_equal(p.quant[c], h["quant"][c]) and len(p.dc[c]) == len(p.ac[c]) == 272
            bits, values = h["ac"][c]
            assert p.ac[c][:16] == bytes(bits) and p.ac[c][16:16 + len(values)] == bytes(values)
    some = cases[::97]
    pictures = jpeg_decode.check(jpeg_decode.decode([c.data for c in some], "cpu", [c.name for c in some]))
    assert jpeg_decode.last_path == "torch" and jpeg_decode.last_info == {"files": len(some), "intervals": sum(pictures.intervals), "host_decoded": 0}
    for case, image in zip(some, pictures.images):
        assert image.dtype == torch.uint8 and np.array_equal(image.numpy(), case.image)


def _pil_bytes(image, mode=None, **options):
    im = Image.fromarray(image)
    buf = io.BytesIO()
    (im.convert(mode) if mode else im).save(buf, "JPEG", **options)
    return buf.getvalue()


def _insert_before_sos(data, segment):
    at = DH.header(data)["scan"]
    sos = data.rfind(b"\xff\xda", 0, at)
    return data[:sos] + segment + data[sos:]


def rejected():
    """(name, bytes, a word of the reason)"""
    rgb = JH.picture("texture", 17, 23, 3, seed=3)
    plain = DH.pil_encode(rgb, 90, 2)
    sof = plain.find(b"\xff\xc0")
    twelve = bytearray(plain)
    twelve[sof + 4] = 12
    # one component of three in the first scan: what the first scan of a non-interleaved file looks like
    sos = plain.rfind(b"\xff\xda", 0, DH.header(plain)["scan"])
    two_scans = plain[:sos] + b"\xff\xda" + struct.pack(">H", 8) + bytes([1, 1, 0x00, 0, 63, 0]) + plain[DH.header(plain)["scan"]:]
    adobe = _insert_before_sos(plain, b"\xff\xee" + struct.pack(">H", 14) + b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 0]))
    dqt = plain.find(b"\xff\xdb")
    wide = bytearray(plain)
    wide[dqt + 4] |= 0x10
    return (("progressive", _pil_bytes(rgb, quality=90, progressive=True), "progressive"),
            ("twelve-bit", bytes(twelve), "precision 12"),
            ("two-scans", two_scans, "several scans"),
            ("adobe", adobe, "Adobe"),
            ("cmyk", _pil_bytes(rgb, "CMYK", quality=90), "CMYK"),
            ("dqt16", bytes(wide), "16-bit DQT"))


def test_rejected_kinds_name_file_and_reason():
    good = DH.corpus()[100].data
    kinds = rejected()
    assert len(kinds) == 6
    for name, data, word in kinds:
        with pytest.raises(ValueError) as e:
            jpeg_decode.parse(data, name + ".jpg")
        assert name + ".jpg" in str(e.value) and word in str(e.value), (name, str(e.value))
        with pytest.raises(ValueError):
            jpeg_decode.decode([good, data], "cpu")
    with pytest.raises(ValueError, match="no SOI"):
        jpeg_decode.parse(b"\x89PNG\r\n\x1a\n" + bytes(32))
    with pytest.raises(ValueError, match="past the end"):
        jpeg_decode.parse(good[:40])


def test_unsupported_pil_is_counted_and_never_the_default(tmp_path):
    good = DH.corpus()[200]
    name, data, _ = rejected()[0]  # progressive
    paths = [str(tmp_path / "good.jpg"), str(tmp_path / "progressive.jpg")]
    for path, blob in zip(paths, (good.data, data)):
        with open(path, "wb") as f:
            f.write(blob)
    with pytest.raises(ValueError, match="progressive"):
        jpeg_decode.read(paths, "cpu")
    images = jpeg_decode.read(paths, "cpu", unsupported="pil")
    assert jpeg_decode.last_info["host_decoded"] == 1 and jpeg_decode.last_info["files"] == 2
    assert np.array_equal(images[0].numpy(), good.image) and np.array_equal(images[1].numpy(), DH.pil_decode(data))
    with pytest.raises(ValueError, match="unsupported"):
        jpeg_decode.read(paths, "cpu", unsupported="skip")


def test_the_family_header_parses_and_types_its_exports(native_lib):
    main = _abi.header()
    ext = _abi.extension(jpeg_decode.HEADER)
    assert ext is jpeg_decode._ABI is _abi.extension(jpeg_decode.HEADER)
    assert main.constants["GSR_ABI_VERSION"] == _native.ABI_VERSION == native_lib.gsr_abi_version() == 9
    # the main header is what it was: the family adds nothing to it
    assert _abi.header() is main is _native._ABI and _native.EXPORTED_SYMBOLS == tuple(main.functions)
    assert not set(ext.functions) & set(main.functions) and not set(ext.constants) & set(main.constants)
    assert list(ext.functions) == ["gsr_jpeg_decode_workspace_bytes", "gsr_jpeg_decode", "gsr_jpeg_decode_status_name"] == list(jpeg_decode.EXPORTED_SYMBOLS)
    assert [ext.constants["GSR_JPEG_DECODE_" + n] for n in DH.STATUS_NAMES] == list(range(7)) and jpeg_decode.STATUS == DH.STATUS_NAMES
    assert ext.functions["gsr_jpeg_decode"][0] == "int" and ext.functions["gsr_jpeg_decode_workspace_bytes"][0] == "size_t"
    assert [p[1] for p in ext.functions["gsr_jpeg_decode"][1]] == ["bytes", "nbytes", "files", "nfiles", "nintervals", "quant", "nquant", "huffman",
                                                                   "nhuffman", "out", "out_bytes", "status", "workspace", "workspace_bytes", "stream"]
    lib = jpeg_decode._library()
    assert lib is native_lib
    scalars = {"int": ctypes.c_int, "size_t": ctypes.c_size_t}
    for name, (returns, params) in ext.functions.items():
        fn = getattr(lib, name)  # exported
        assert len(fn.argtypes) == len(params)
        for got, (decl, pname, is_pointer, _) in zip(fn.argtypes, params):
            assert got is (ctypes.c_void_p if is_pointer else scalars[decl]), (name, pname)
        assert fn.restype is {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}[returns]
    # the numpy mirrors come from the header's structs
    assert [(f, jpeg_decode._FILE.fields[f][0].base.str, jpeg_decode._FILE.fields[f][0].shape) for f in jpeg_decode._FILE.names] == \
        [(f, {"uint64_t": "<u8", "uint32_t": "<u4", "int32_t": "<i4"}[c], () if n is None else (n,)) for c, f, n in ext.structs["gsr_jpeg_file"]]
    assert jpeg_decode._FILE.itemsize == 104 and jpeg_decode._HUFFMAN.itemsize == 272
    assert [jpeg_decode.status_name(c) for c in (0, 1, 6, 7, -1)] == ["ok", "truncated", "table entry out of bounds", "?", "?"]
    # a struct that names a constant of the main header is read with it in scope
    assert _abi.parse("typedef struct gsr_x { double t[GSR_NUM_STAGES]; } gsr_x;", main.constants).structs == {"gsr_x": [("double", "t", 7)]}


def test_argument_rejection_before_any_launch(native_lib):
    lib = jpeg_decode._library()
    assert lib.gsr_jpeg_decode_workspace_bytes(1000, 2, 10) >= 1008 + 4 * 4 * 10
    assert lib.gsr_jpeg_decode_workspace_bytes(1000, 0, 10) == 0 and lib.gsr_jpeg_decode_workspace_bytes(1000, 2, 0) == 0
    assert lib.gsr_jpeg_decode_workspace_bytes(1 << 40, 2, 10) == 0
    raw = (ctypes.c_uint8 * 4096)()
    buf = ctypes.c_void_p((ctypes.addressof(raw) + 255) & ~255)

    def call(bytes_=buf, nbytes=64, files=buf, nfiles=1, nintervals=1, quant=buf, nquant=1, huffman=buf, nhuffman=1, out=buf, out_bytes=64, status=buf,
             workspace=buf, workspace_bytes=1024):
        return lib.gsr_jpeg_decode(bytes_, nbytes, files, nfiles, nintervals, quant, nquant, huffman, nhuffman, out, out_bytes, status, workspace,
                                   workspace_bytes, None)
    odd = ctypes.c_void_p(buf.value + 8)
    for kwargs, word in (({"bytes_": None}, b"NULL"), ({"huffman": None}, b"NULL"), ({"nfiles": 0}, b"nfiles"), ({"nintervals": -1}, b"nintervals"),
                         ({"nquant": 0}, b"nquant"), ({"nfiles": 65536}, b"nfiles"), ({"nbytes": 1 << 32}, b"2^32"), ({"out_bytes": 1 << 32}, b"2^32"),
                         ({"out": odd}, b"aligned"), ({"quant": odd}, b"aligned"), ({"workspace": odd}, b"aligned"), ({"workspace_bytes": 8}, b"tables")):
        assert call(**kwargs) == -1 and word in native_lib.gsr_last_error(), (kwargs, native_lib.gsr_last_error())


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/jpeg_entropy_check.cpp built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tools/jpeg_entropy_check.cpp")
    exe = str(tmp_path_factory.mktemp("jpeg_check") / "jpeg_entropy_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "jpeg_entropy_check.cpp"), "-o", exe], check=True)
    return exe


def _run_checker(checker, cases, folder):
    paths = []
    for k, case in enumerate(cases):
        paths.append(str(folder / f"{k:05d}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(case.data)
    lines = []
    for at in range(0, len(paths), 500):
        run = subprocess.run([checker] + paths[at:at + 500], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]  # (a sanitizer report is on stderr and ends the program)
        lines += run.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    out = []
    for case, path, line in zip(cases, paths, lines):
        m = re.fullmatch(re.escape(path) + r" status=(\d+) intervals=(\d+) digest=([0-9a-f]{8})", line)
        assert m, (case.name, line)
        out.append((int(m.group(1)), int(m.group(2)), int(m.group(3), 16)))
    return out


def test_sanitized_core_decodes_the_valid_corpus(checker, tmp_path):
    cases = DH.corpus()
    for case, (code, intervals, digest) in zip(cases, _run_checker(checker, cases, tmp_path)):
        assert code == DH.OK, (case.name, DH.STATUS_NAMES[code])
        h = DH.header(case.data)
        assert intervals == DH.geometry(h)["intervals"], case.name
        assert digest == DH.digest(DH.coefficients(case.data, h)), case.name  # the coefficients are the rules', block for block


def test_sanitized_core_ends_every_corrupt_file_in_a_code(checker, tmp_path):
    cases = DH.corrupt()
    names = " ".join(c.name for c in cases)
    for word in ("-cut", "-flip", "-rst-removed", "-rst-duplicated", "-rst-renumbered", "dri-", "plain-", "opt-"):
        assert word in names
    seen = set()
    for case, (code, _, digest) in zip(cases, _run_checker(checker, cases, tmp_path)):
        assert code != DH.OK and digest == 0, case.name
        assert code == DH.status(case.data), (case.name, DH.STATUS_NAMES[code])  # and it is the code the rules give
        seen.add(code)
        if "-cut" in case.name:
            assert code == DH.TRUNCATED, case.name
        if "-rst-" in case.name:
            assert code == DH.RESTART, case.name
    assert {DH.TRUNCATED, DH.RESTART, DH.BAD_CODE} <= seen


def test_mjpeg_reader_finds_the_frames_of_a_host_written_file(tmp_path):
    frames = torch.from_numpy(np.stack([JH.picture("texture", 32, 48, 3, seed=k) for k in range(5)]))
    path = str(tmp_path / "spiral.avi")
    with video.MjpegWriter(path, 48, 32, fps=12, quality=90) as w:
        w.add(frames[:3])
        w.add(frames[3:])
    with open(path, "rb") as f:
        want = JH.parse_avi(f.read())
    reader = video.MjpegReader(path)
    assert (reader.W, reader.H, reader.fps, len(reader)) == (48, 32, 12.0, 5)
    assert [reader.frame_bytes(i) for i in range(5)] == want["frames"]
    got = list(reader.frames("cpu", batch=2))
    assert len(got) == 5 and jpeg_decode.last_path == "torch"
    for k, image in enumerate(got):
        assert image.dtype == torch.uint8 and np.array_equal(image.numpy(), DH.pil_decode(want["frames"][k]))
    assert all(torch.equal(a, b) for a, b in zip(video.read_rgbd_video(path, "cpu"), got))
    with open(str(tmp_path / "not.avi"), "wb") as f:
        f.write(b"RIFF" + bytes(300))
    with pytest.raises(ValueError, match="not a RIFF"):
        video.MjpegReader(str(tmp_path / "not.avi"))
