"""CPU tests of gscream_amd.png_decode: the host parser on every corpus file, the rejected kinds, the host path against PIL, and the
decoder core of gscream_amd/csrc/png_inflate.h -- the code the kernels run -- compiled into tools/png_inflate_check.cpp with
AddressSanitizer and UBSan and run as a child process over the whole corpus, corrupt files included: the status codes and the pictures'
digests must be the expected ones and the sanitizers must stay silent.  Nothing is loaded into Python under a sanitizer."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import png_decode_helpers as DH
from gscream_amd import png_decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(c, l) for c in DH.COMPRESSORS for l in DH.LAYOUTS]


def _all_cases():
    cases = []
    for c, l in COMBOS:
        cases += DH.cross(c, l)
    cases += DH.edge_shapes() + DH.never_emitted() + DH.flushed("full") + DH.flushed("sync") + DH.corrupt() + tuple(DH.mixed_sizes())
    return cases


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """tools/png_inflate_check.cpp built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler for tools/png_inflate_check.cpp")
    exe = str(tmp_path_factory.mktemp("png_check") / "png_inflate_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "png_inflate_check.cpp"), "-o", exe], check=True)
    return exe


def test_sanitized_core_over_the_whole_corpus(checker, tmp_path):
    cases = _all_cases()
    paths = []
    for k, case in enumerate(cases):
        paths.append(str(tmp_path / f"{k:04d}.png"))
        with open(paths[-1], "wb") as f:
            f.write(case.data)
    lines = []
    for at in range(0, len(paths), 500):
        run = subprocess.run([checker] + paths[at:at + 500], capture_output=True, text=True)
        assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
        lines += run.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    for case, path, line in zip(cases, paths, lines):
        m = re.fullmatch(re.escape(path) + r" status=(\d+) path=(\w+) segments=(\d+) digest=([0-9a-f]{8})", line)
        assert m, line
        assert int(m.group(1)) == case.status, (case.name, line)
        if case.status == DH.OK:
            assert int(m.group(4), 16) == DH.digest(case.image), case.name
        if case.name.startswith("flush-"):
            assert (m.group(2), int(m.group(3))) == ("parallel" if case.name == "flush-full" else "serial", 15)
        if case.name.startswith("own-") and int(m.group(3)) > 1:
            assert m.group(2) == "parallel"


def test_sanitized_core_takes_own_multi_chunk_files_in_parallel(checker, tmp_path):
    from gscream_amd import png
    paths = []
    for k, image in enumerate(DH.own_pictures()):
        (data,) = png.to_bytes(png.encode(torch.from_numpy(image)))
        paths.append(str(tmp_path / f"own{k}.png"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    run = subprocess.run([checker] + paths, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]
    for image, line in zip(DH.own_pictures(), run.stdout.strip().split("\n")):
        assert " status=0 path=parallel segments=3 " in line and line.endswith("digest=%08x" % DH.digest(image)), line


@pytest.mark.parametrize("compressor,layout", COMBOS)
def test_parse_and_host_path_equal_pil(compressor, layout):
    cases = DH.cross(compressor, layout)
    for case in cases:
        p = png_decode.parse(case.data, case.name)
        assert (p.H, p.W, p.C) == case.image.shape
        idat = [x for x in p.pieces if x[2] & 1]
        assert b"".join(case.data[o:o + n] for o, n, _ in idat) == DH.idat_payload(case.data)
        assert np.array_equal(DH.pil_decode(case.data), case.image)
    some = cases[::7]
    pictures = png_decode.check(png_decode.decode([c.data for c in some], "cpu"))
    assert png_decode.last_path == "torch"
    for case, image in zip(some, pictures.images):
        assert image.dtype == torch.uint8 and np.array_equal(image.numpy(), case.image)


def test_parse_segments_and_the_other_corpus_files():
    for case in DH.edge_shapes() + DH.never_emitted() + DH.corrupt() + tuple(DH.mixed_sizes()):
        p = png_decode.parse(case.data, case.name)
        assert p.candidates == [] or case.name.startswith("own-")
    for mode in ("full", "sync"):
        (case,) = DH.flushed(mode)
        p = png_decode.parse(case.data)
        assert len(p.candidates) == 14 and (p.H, p.W, p.C) == DH.THREE_CHUNKS
        assert all(p.pieces[i][2] == 3 for i in p.candidates)
    from gscream_amd import png
    for image in DH.own_pictures():
        (data,) = png.to_bytes(png.encode(torch.from_numpy(image)))
        assert len(png_decode.parse(data).candidates) == 2


def test_rejected_kinds_name_file_and_reason():
    for name, data, word in DH.rejected():
        with pytest.raises(ValueError) as e:
            png_decode.parse(data, name + ".png")
        assert name + ".png" in str(e.value) and word in str(e.value), (name, str(e.value))
        with pytest.raises(ValueError):
            png_decode.decode([DH.mixed_sizes()[0].data, data], "cpu")


def test_unsupported_pil_is_counted_and_never_the_default(tmp_path):
    good = DH.mixed_sizes()[1]
    name, data, _ = DH.rejected()[1]  # palette
    paths = [str(tmp_path / "good.png"), str(tmp_path / "palette.png")]
    for path, blob in zip(paths, (good.data, data)):
        with open(path, "wb") as f:
            f.write(blob)
    with pytest.raises(ValueError):
        png_decode.read(paths, "cpu")
    images = png_decode.read(paths, "cpu", unsupported="pil")
    assert png_decode.last_info["host_decoded"] == 1 and png_decode.last_info["files"] == 2
    assert np.array_equal(images[0].numpy(), good.image) and np.array_equal(images[1].numpy(), DH.pil_decode(data))


def test_read_images_and_evaluate_files_on_the_host(tmp_path):
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
        png.save(torch.from_numpy(renders[k]), str(dirs["renders"] / f"{k:05d}.png"))
        png.save(torch.from_numpy(gts[k]), str(dirs["gt"] / f"{k:05d}.png"))
        png.save(torch.from_numpy(masks[k]), str(dirs["masks"] / ("out_%05d.png" % (k + 1))))
    r, g, names, m = png_decode.read_images(dirs["renders"], dirs["gt"], dirs["masks"], device="cpu")
    assert sorted(names) == [f"{k:05d}.png" for k in range(3)]
    for i, name in enumerate(names):
        k = int(name[:5])
        assert r[i].shape == g[i].shape == m[i].shape == (1, 3, H, W) and r[i].dtype == torch.float32 and m[i].dtype == torch.bool
        assert m[i].stride(1) == 0
        assert torch.equal(r[i], torch.from_numpy(renders[k]).permute(2, 0, 1)[None].float() / 255.0)
        assert torch.equal(m[i][0, 0], torch.from_numpy(masks[k][..., 0] > 0))
    full, per_view = png_decode.evaluate_files(dirs["renders"], dirs["gt"], dirs["masks"], device="cpu")
    want = metrics.evaluate_views(r, g, m, names)
    assert (full, per_view) == want


def test_abi_entries(native_lib):
    from gscream_amd import _abi, _native
    hdr = _abi.header()
    assert hdr.constants["GSR_ABI_VERSION"] == 9 and native_lib.gsr_abi_version() == 9
    assert hdr.functions["gsr_png_decode"][0] == "int" and hdr.functions["gsr_png_decode_workspace_bytes"][0] == "size_t"
    for name in ("gsr_png_decode_workspace_bytes", "gsr_png_decode"):
        assert name in _native.EXPORTED_SYMBOLS and hasattr(native_lib, name)
    for code, name in enumerate(("OK", "TRUNCATED", "BLOCK_TYPE", "STORED_LEN", "BAD_CODE", "BAD_SYMBOL", "DISTANCE", "TOO_LONG", "TOO_SHORT",
                                 "FILTER", "ADLER", "CRC", "TABLE")):
        assert getattr(DH, name) == code == hdr.constants["GSR_PNG_" + name]
    assert len(_native.PNG_STATUS) == 13 and (_native.PNG_PIECE_IDAT, _native.PNG_PIECE_START) == (1, 2)
    assert native_lib.gsr_png_decode_workspace_bytes(1000, 2, 10) >= 1000 + 120 + 8 and native_lib.gsr_png_decode_workspace_bytes(1000, 0, 10) == 0
    buf = (_native.ctypes.c_uint8 * 64)()
    assert native_lib.gsr_png_decode(buf, 64, buf, 0, buf, 1, 1, buf, 64, buf, buf, 64, None) == -1 and b"nfiles" in native_lib.gsr_last_error()
    assert native_lib.gsr_png_decode(None, 64, buf, 1, buf, 1, 1, buf, 64, buf, buf, 64, None) == -1 and b"NULL" in native_lib.gsr_last_error()
