"""Reading baseline JPEG files on the HIP path: the bytes of .jpg files -> uint8 [H, W, C] pictures on the device.  The other half of
gscream_amd.jpeg (which writes the frames of gscream_amd.video's Motion-JPEG AVI), and the stage in front of
gscream_amd.metrics.evaluate_views for a scene whose pictures are .jpg (scene/dataset_readers.py:171-172 switches the reference
between the two extensions): Image.open, to_tensor and .cuda() per file.

Integration (INTEGRATION Z):

    Image.open(path) + to_tensor + upload, per picture     ->  jpeg_decode.read(paths, device)
    the same from bytes already in memory                   ->  jpeg_decode.check(jpeg_decode.decode(files, device)).images
    the frames of a video.MjpegWriter file                  ->  video.MjpegReader(path).frames(device) / video.read_rgbd_video

The host only walks the marker segments up to SOS (`parse`): sizes, sampling, the quantisation and Huffman tables, DRI.  It does not
look at the entropy-coded data.  The files' bytes, unmodified, and the tables go to the device in one copy; the restart markers are
found there, and Huffman decoding, dequantisation, the IDCT, chroma upsampling and colour conversion run there
(gscream_amd/csrc/jpeg_decode.hip, `last_path = "hip"`), all files of a call in one launch sequence, with no synchronisation: the
sizes come from SOF0.  The unit of parallel work is the restart interval, one wavefront each.  Every file `jpeg.encode` writes has an
interval per MCU row.  A file without restart markers -- what PIL and most cameras write -- is ONE interval: one wavefront walks its
whole scan, which is correct and slow: 232.1 ms for one 567x1008 file against PIL's 2.8 ms.  `split="auto"` / "always" cut such an interval
into subsequences of 128 bytes, a lane each (gscream_amd/csrc/jpeg_split.hip, include/gsraster_jpeg_split.h): 6.7 ms for that file, 13.7 ms
for 80 of them (INTEGRATION Z has the numbers; `read`'s docstring says which files to bring here).
The picture is PIL's (libjpeg-turbo: islow IDCT, fancy upsampling) byte for byte; the rules and the status codes are in
include/gsraster_jpeg_decode.h in full.

Accepted: SOF0 with 8-bit samples, one scan with all components, grey or YCbCr with 4:4:4, 4:2:2 or 4:2:0 sampling, 8-bit DQT.
Everything else raises ValueError in `parse`, naming the file and the reason, before any launch; `read(..., unsupported="pil")` sends
such files through PIL instead and counts them.

CPU devices and `force_torch = True` decode with PIL per file (`last_path = "torch"`).  A missing library raises; nothing falls back
quietly."""
import ctypes
import io
import os
import struct
from typing import List, NamedTuple

import numpy as np
import torch

from . import _abi, _native

__all__ = ["JpegDecodeError", "JpegPictures", "check", "decode", "parse", "read"]

force_torch = False
last_path = None  # "hip" / "torch": the path the last decode took
last_info = {}    # filled by check / read: files, intervals, host_decoded

HEADER = "gsraster_jpeg_decode.h"
_ABI = _abi.extension(HEADER)  # the family's own header: its functions are typed from it, its structs and codes read from it
EXPORTED_SYMBOLS = tuple(_ABI.functions)
SPLIT_HEADER = "gsraster_jpeg_split.h"  # the split decode: a family of its own beside this one, the same library
_SPLIT_ABI = _abi.extension(SPLIT_HEADER)
SPLIT_EXPORTED_SYMBOLS = tuple(_SPLIT_ABI.functions)
SPLITS = ("never", "auto", "always")
# The shipped defaults (INTEGRATION Z, profiles/jpeg_decode_timing.json): 128 = the best median of the subsequence_bytes sweep on 80 marker-less
# files; 4644 = the smallest measured interval length from which the split path stays below the one-wave path; "never": the rule for "auto" is
# not met to the letter, and existing tests pin a default call's last_info.
DEFAULT_SUBSEQUENCE_BYTES = 128
DEFAULT_MIN_BYTES = 4644
DEFAULT_SPLIT = "never"
STATUS = tuple(name[len("GSR_JPEG_DECODE_"):] for name, _ in sorted(((n, v) for n, v in _ABI.constants.items() if n.startswith("GSR_JPEG_DECODE_")),
                                                                    key=lambda item: item[1]))
_NUMPY = {"uint8_t": "u1", "uint16_t": "<u2", "int32_t": "<i4", "uint32_t": "<u4", "uint64_t": "<u8"}


def _dtype(struct_name):
    return np.dtype([(field, _NUMPY[ctype]) if length is None else (field, _NUMPY[ctype], (length,)) for ctype, field, length in _ABI.structs[struct_name]])


_FILE, _HUFFMAN = _dtype("gsr_jpeg_file"), _dtype("gsr_jpeg_huffman")
assert _FILE.itemsize == 104 and _HUFFMAN.itemsize == 272
_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43,
           36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)  # natural index of coding position k
_lib = _split_lib = None


def _typed(lib, abi):
    for name, (returns, params) in abi.functions.items():
        fn = getattr(lib, name)  # AttributeError: a library built without the family's object file
        fn.restype = _abi.ctype(returns, returns=True)
        fn.argtypes = [_abi.ctype(ctype) for ctype, _, _, _ in params]
    return lib


def _library():
    """libgsraster.so with this family's functions typed from their declarations (_abi.ctype: an unknown type raises)."""
    global _lib
    if _lib is None:
        _lib = _typed(_native.load(), _ABI)
    return _lib


def _split_library():
    """The same library with the split family's functions typed as well, on the first split decode: a library without them (one
    built from a commit before the family) still serves split="never", and raises AttributeError here."""
    global _split_lib
    if _split_lib is None:
        _split_lib = _typed(_library(), _SPLIT_ABI)
    return _split_lib


def status_name(code):
    return _library().gsr_jpeg_decode_status_name(int(code)).decode()


class JpegDecodeError(RuntimeError):
    """A file failed on the device: .index (in the call's list), .code (GSR_JPEG_DECODE_*), .failures [(index, code)]."""

    def __init__(self, failures, names=None):
        self.failures = failures
        self.index, self.code = failures[0]
        what = "; ".join(f"file {i}{' (' + str(names[i]) + ')' if names else ''}: code {c}, {STATUS[c] if 0 <= c < len(STATUS) else '?'}" for i, c in failures[:8])
        super().__init__(f"jpeg_decode: {len(failures)} file(s) failed: {what}")


class Parsed(NamedTuple):
    """From the segments in front of the scan.  hs, vs: the sampling of component 0; dri: MCUs per restart interval (0 = no markers);
    quant: per component a uint16 [64] table in natural order; dc, ac: per component the 272 bytes bits[16] + values[256] of its Huffman
    table; scan: the offset of the first entropy-coded byte; intervals: ceil(MCUs / dri), 1 without DRI; blocks: 8x8 blocks of all components."""
    H: int
    W: int
    C: int
    hs: int
    vs: int
    dri: int
    quant: tuple
    dc: tuple
    ac: tuple
    scan: int
    intervals: int
    blocks: int


class JpegPictures(NamedTuple):
    """images: uint8 [H, W, C] views of one buffer, one per file; status: int32 [n] on the device (GSR_JPEG_DECODE_* codes, 0 = OK);
    decoded: int32 [n] on the device, the intervals decoded; intervals: per file, from the host parser; names: what `check` calls the files.
    From a split decode also info: int32 [n, 4] on the device, per file {intervals split, intervals repaired, subsequences, chunks};
    words: the one int32 buffer that holds status and info (what `check` reads back); trace: None, or with decode(trace=True) int32
    [rows, 5] on the device, per subsequence (bit, j, k, first_block, blocks) -- the split intervals in order, each one's subsequences
    in order, sum(info[:, 2]) rows used."""
    images: List[torch.Tensor]
    status: torch.Tensor
    decoded: torch.Tensor
    intervals: tuple = ()
    names: tuple = ()
    info: torch.Tensor = None
    words: torch.Tensor = None
    trace: torch.Tensor = None


_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential", 0xC6: "differential progressive",
              0xC7: "differential lossless", 0xC9: "arithmetic-coded", 0xCA: "arithmetic-coded progressive", 0xCB: "arithmetic-coded lossless",
              0xCD: "arithmetic-coded differential", 0xCE: "arithmetic-coded differential progressive", 0xCF: "arithmetic-coded differential lossless"}


def parse(data, name=None):
    """The bytes of one file -> Parsed.  Walks the marker segments up to SOS only.  ValueError, naming the file and the reason, for
    anything outside the accepted subset (include/gsraster_jpeg_decode.h): no SOI, a segment that runs past the end, a frame that is not
    SOF0 (progressive, arithmetic, lossless, ...), a precision other than 8, component counts other than 1 and 3 (CMYK), sampling other
    than 1x1 / 2x1 / 2x2 over 1x1 chroma, a 16-bit DQT, a scan that does not hold all components or is not Ss 0 Se 63 Ah/Al 0
    (several scans), a table the scan names and no segment defines, three components with an Adobe APP14 segment or with the ids R G B and
    no JFIF APP0 (libjpeg does not take those as YCbCr)."""
    name = "<bytes>" if name is None else name

    def bad(reason):
        return ValueError(f"jpeg_decode: {name}: {reason}")
    n = len(data)
    if n < 4 or bytes(data[:2]) != b"\xff\xd8":
        raise bad("no SOI marker: not a JPEG file")
    at, quant, huff, dri, frame, jfif, adobe = 2, {}, {}, 0, None, False, False
    while True:
        if at + 4 > n:
            raise bad("the file ends before a scan starts")
        if data[at] != 0xFF:
            raise bad(f"no marker at byte {at}")
        marker = data[at + 1]
        if marker == 0xFF:  # a fill byte
            at += 1
            continue
        if marker == 0xD9 or 0xD0 <= marker <= 0xD7 or marker == 0x01 or marker == 0x00:
            raise bad(f"marker FF{marker:02X} in front of the scan")
        length = struct.unpack_from(">H", data, at + 2)[0]
        if length < 2 or at + 2 + length > n:
            raise bad("a segment runs past the end of the file")
        p = bytes(data[at + 4:at + 2 + length])
        if marker == 0xC0:
            if frame is not None:
                raise bad("a second frame header")
            if len(p) < 6 or len(p) != 6 + 3 * p[5]:
                raise bad("bad SOF0 segment")
            if p[0] != 8:
                raise bad(f"sample precision {p[0]} is not decoded (8-bit files only; 12-bit needs other tables)")
            frame = p
        elif marker in _SOF_NAMES:
            raise bad(f"{_SOF_NAMES[marker]} files are not decoded (baseline SOF0 only)")
        elif marker == 0xDB:
            q = 0
            while q < len(p):
                if p[q] >> 4:
                    raise bad("a 16-bit DQT table is not decoded (baseline tables are 8-bit)")
                if len(p) - q < 65 or p[q] & 15 > 3:
                    raise bad("bad DQT segment")
                table = np.zeros(64, np.uint16)
                table[list(_ZIGZAG)] = np.frombuffer(p, np.uint8, 64, q + 1)
                quant[p[q] & 15] = table
                q += 65
        elif marker == 0xC4:
            q = 0
            while q < len(p):
                if len(p) - q < 17:
                    raise bad("bad DHT segment")
                total = sum(p[q + 1:q + 17])
                if p[q] >> 4 > 1 or p[q] & 15 > 3 or total > 256 or len(p) - q - 17 < total:
                    raise bad("bad DHT segment")
                code = 0
                for k in range(16):
                    code = (code + p[q + 1 + k]) << 1
                    if code > 2 << (k + 1):
                        raise bad("a DHT table with more codes of a length than a prefix code has room for")
                huff[p[q]] = p[q + 1:q + 17] + p[q + 17:q + 17 + total] + bytes(256 - total)
                q += 17 + total
        elif marker == 0xDD:
            if len(p) != 2:
                raise bad("bad DRI segment")
            dri = struct.unpack(">H", p)[0]
        elif marker == 0xE0 and p[:5] == b"JFIF\0":
            jfif = True
        elif marker == 0xEE and p[:5] == b"Adobe":
            adobe = True
        elif marker == 0xDC:
            raise bad("a DNL segment (the height is not in the frame header)")
        elif marker == 0xDA:
            break
        at += 2 + length
    if frame is None:
        raise bad("a scan without a frame header")
    H, W, C = struct.unpack(">HH", frame[1:5]) + (frame[5],)
    if C not in (1, 3):
        raise bad(f"{C} components are not decoded (grey and YCbCr only; CMYK / YCCK files have 4)")
    if H == 0 or W == 0:
        raise bad("a zero size")
    comps = [(frame[6 + 3 * c], frame[7 + 3 * c] >> 4, frame[7 + 3 * c] & 15, frame[8 + 3 * c]) for c in range(C)]
    hs, vs = comps[0][1], comps[0][2]
    if C == 1:
        hs = vs = 1  # (one component: its factors only scale the MCU, which is one block whatever they say)
    elif (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in comps[1:]):
        raise bad(f"sampling {'/'.join('%dx%d' % c[1:3] for c in comps)} is not decoded (4:4:4, 4:2:2 and 4:2:0 only)")
    if C == 3 and adobe:
        raise bad("three components with an Adobe APP14 segment (its transform flag, not YCbCr by default, decides the colours)")
    if C == 3 and not jfif and bytes(c[0] for c in comps) == b"RGB":
        raise bad("three components with the ids R, G, B and no JFIF APP0: an RGB file, not YCbCr")
    if len(p) != 4 + 2 * p[0] or p[0] != C:
        raise bad(f"the scan holds {p[0]} of {C} components (files of several scans are not decoded)")
    if p[-3:] != bytes([0, 63, 0]):
        raise bad("the scan is not Ss 0, Se 63, Ah/Al 0 (a progressive or several-scan file)")
    dc, ac, qt = [], [], []
    for c in range(C):
        if p[1 + 2 * c] != comps[c][0]:
            raise bad("the scan's components are not the frame's, in order")
        td, ta = p[2 + 2 * c] >> 4, 0x10 | (p[2 + 2 * c] & 15)
        if td not in huff or ta not in huff or comps[c][3] not in quant:
            raise bad("the scan names a Huffman or quantisation table that no segment defines")
        dc.append(huff[td])
        ac.append(huff[ta])
        qt.append(quant[comps[c][3]])
    mcus = -(-W // (8 * hs)) * -(-H // (8 * vs))
    return Parsed(H, W, C, hs, vs, dri, tuple(qt), tuple(dc), tuple(ac), at + 2 + length, -(-mcus // dri) if dri else 1, mcus * (hs * vs + C - 1))


def _round16(v):
    return (v + 15) & ~15


def _device_bytes(n, device, what):
    """The call's device buffers -- what: "out", "status", "workspace" -- as uint8 [n], 16-byte aligned.  (The one place they come
    from: tests/test_gpu_jpeg_decode.py puts them between guard bands here.)"""
    return torch.empty(n, dtype=torch.uint8, device=device)


def _pil_picture(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    a = np.asarray(im)
    if a.dtype != np.uint8:
        raise ValueError(f"jpeg_decode: PIL gives {a.dtype} pixels (mode {im.mode}); only 8-bit pictures have a uint8 [H, W, C] form")
    return np.array(a.reshape(a.shape[0], a.shape[1], -1))  # (a copy: PIL's buffer is read-only)


def decode(files, device, names=None, split=DEFAULT_SPLIT, subsequence_bytes=None, min_bytes=None, trace=False):
    """files: a list of bytes-like objects, one JPEG file each, of any sizes, samplings and writers -> JpegPictures on `device`.  One
    H2D copy of one staging buffer (tables and bytes), one launch sequence on torch's current stream, no synchronisation and nothing
    read back: call `check` for that.  Raises ValueError (from `parse`) before anything is launched when a file is outside the accepted
    subset.
    split: "never" -- gsr_jpeg_decode, a wavefront per restart interval; "always" -- gsr_jpeg_decode_split with every interval of at
    least two subsequences cut into subsequences of `subsequence_bytes` (a power of two, 16 .. 1024) and decoded a lane per
    subsequence (include/gsraster_jpeg_split.h); "auto" -- the same for the intervals of at least `min_bytes`, the others as under
    "never".  The pictures and the status codes are the same bytes under all three.  trace=True (split decodes only) also returns the
    per-subsequence entry states and counts.  The CPU path ignores all four."""
    global last_path
    if split not in SPLITS:
        raise ValueError(f"jpeg_decode: split={split!r} (have {', '.join(repr(v) for v in SPLITS)})")
    B = DEFAULT_SUBSEQUENCE_BYTES if subsequence_bytes is None else subsequence_bytes
    if not isinstance(B, int) or isinstance(B, bool) or not 16 <= B <= 1024 or B & (B - 1):
        raise ValueError(f"jpeg_decode: subsequence_bytes={subsequence_bytes!r} (need a power of two from 16 to 1024)")
    least = (0 if split == "always" else DEFAULT_MIN_BYTES) if min_bytes is None else min_bytes
    if not isinstance(least, int) or isinstance(least, bool) or not 0 <= least < 1 << 31:
        raise ValueError(f"jpeg_decode: min_bytes={min_bytes!r} (need an integer from 0 to 2^31 - 1)")
    device = torch.device(device)
    files = list(files)
    if not files:
        raise ValueError("jpeg_decode: no files")
    names = tuple(names) if names is not None else tuple(f"file {i}" for i in range(len(files)))
    parsed = [parse(data, name) for data, name in zip(files, names)]  # the same subset on both paths
    counts = tuple(p.intervals for p in parsed)
    if force_torch or device.type != "cuda":
        last_path = "torch"
        images = [torch.from_numpy(_pil_picture(bytes(d))).to(device) for d in files]
        zeros = torch.zeros(len(files), dtype=torch.int32, device=device)
        return JpegPictures(images, zeros, torch.tensor(counts, dtype=torch.int32, device=device), counts, names)
    nfiles = len(files)
    ftab = np.zeros(nfiles, _FILE)
    qindex, hindex = {}, {}  # equal tables are stored once
    starts, at = [], 0
    out_at = area_at = interval_at = 0
    for i, (data, p) in enumerate(zip(files, parsed)):
        starts.append(at)
        row = ftab[i]
        row["scan_offset"], row["scan_length"] = at + p.scan, len(data) - p.scan
        row["H"], row["W"], row["C"], row["hs"], row["vs"] = p.H, p.W, p.C, p.hs, p.vs
        row["restart_interval"], row["first_interval"], row["intervals"] = p.dri, interval_at, p.intervals
        row["out_offset"], row["coef_offset"], row["plane_offset"] = out_at, area_at, area_at + 128 * p.blocks
        for c in range(p.C):
            row["quant"][c] = qindex.setdefault(p.quant[c].tobytes(), len(qindex))
            row["dc"][c] = hindex.setdefault(p.dc[c], len(hindex))
            row["ac"][c] = hindex.setdefault(p.ac[c], len(hindex))
        at += _round16(len(data))
        out_at += _round16(p.H * p.W * p.C)
        area_at += 192 * p.blocks  # (a multiple of 16)
        interval_at += p.intervals
    nbytes, nintervals = at, interval_at
    if nbytes >= 1 << 32 or out_at >= 1 << 32 or nintervals >= 1 << 31 or nfiles > 65535:
        raise ValueError("jpeg_decode: a call takes less than 4 GiB of files and of pictures, at most 65535 files and fewer than 2^31 intervals")
    qtab = np.frombuffer(b"".join(qindex), "<u2")
    htab = np.frombuffer(b"".join(hindex), np.uint8)
    # the staging buffer: file table, quantisation tables, Huffman tables, then the files' bytes (each at a multiple of 16)
    off_quant = _round16(ftab.nbytes)
    off_huff = off_quant + _round16(qtab.nbytes)
    off_bytes = off_huff + _round16(htab.nbytes)
    staging = torch.empty(off_bytes + nbytes, dtype=torch.uint8)
    if torch.cuda.is_available():
        staging = staging.pin_memory()
    host = staging.numpy()
    host[:ftab.nbytes] = ftab.view(np.uint8)
    host[off_quant:off_quant + qtab.nbytes] = qtab.view(np.uint8)
    host[off_huff:off_huff + htab.nbytes] = htab
    for data, start in zip(files, starts):
        host[off_bytes + start:off_bytes + start + len(data)] = np.frombuffer(data, np.uint8)
    last_path = "hip"
    lib = _library()
    with torch.cuda.device(device):
        dev = staging.to(device, non_blocking=True)
        out = _device_bytes(max(out_at, 16), device, "out")
        base = dev.data_ptr()
        args = (ctypes.c_void_p(base + off_bytes), nbytes, ctypes.c_void_p(base), nfiles, nintervals, ctypes.c_void_p(base + off_quant), len(qindex),
                ctypes.c_void_p(base + off_huff), len(hindex), _native.ptr(out), out.numel())
        if split == "never":  # today's call, untouched
            words = info = rows = None
            status = _device_bytes(8 * nfiles, device, "status").view(torch.int32).view(nfiles, 2)
            ws_bytes = int(lib.gsr_jpeg_decode_workspace_bytes(area_at, nfiles, nintervals))
            if ws_bytes == 0:
                raise ValueError("jpeg_decode: the call's coefficients and planes are beyond 2^40 bytes")
            workspace = _device_bytes(ws_bytes, device, "workspace")
            _native.run("gsr_jpeg_decode", out.device, *args, _native.ptr(status), _native.ptr(workspace), ws_bytes)
        else:
            words = _device_bytes(24 * nfiles, device, "status").view(torch.int32)  # status {code, decoded} per file, then info: four per file
            status, info = words[:2 * nfiles].view(nfiles, 2), words[2 * nfiles:].view(nfiles, 4)
            ws_bytes = int(_split_library().gsr_jpeg_split_workspace_bytes(area_at, nfiles, nintervals, nbytes, B))
            if ws_bytes == 0:
                raise ValueError("jpeg_decode: the call's coefficients and planes are beyond 2^40 bytes")
            workspace = _device_bytes(ws_bytes, device, "workspace")
            rows = _device_bytes(20 * (nbytes // B + nintervals), device, "trace").view(torch.int32).view(-1, 5) if trace else None
            _native.run("gsr_jpeg_decode_split", out.device, *args, _native.ptr(status), _native.ptr(workspace), ws_bytes, B, least,
                        _native.ptr(rows) if trace else None, _native.ptr(info))
    images = []
    for i, p in enumerate(parsed):
        o = int(ftab["out_offset"][i])
        images.append(out[o:o + p.H * p.W * p.C].view(p.H, p.W, p.C))
    return JpegPictures(images, status[:, 0], status[:, 1], counts, names, info, words, rows)


def check(pictures, host_decoded=0):
    """The one read-back: the status words of a decode (with a split decode's counts in the same buffer).  Raises JpegDecodeError
    (index and code of every failed file) and fills last_info: files, intervals, host_decoded, and after a split decode on the device
    (decode's `split` other than "never") also split_intervals, repaired_intervals, subsequences."""
    global last_info
    counts = None
    if pictures.words is not None:
        words = pictures.words.cpu().numpy()  # one copy
        n = words.shape[0] // 6
        codes, counts = words[:2 * n].reshape(n, 2)[:, 0], words[2 * n:].reshape(n, 4)
    else:
        codes = pictures.status.cpu().numpy() if pictures.status.is_cuda else pictures.status.numpy()  # one copy
    last_info = {"files": int(codes.shape[0]) + host_decoded, "intervals": int(sum(pictures.intervals)), "host_decoded": host_decoded}
    if counts is not None:
        last_info.update(split_intervals=int(counts[:, 0].sum()), repaired_intervals=int(counts[:, 1].sum()), subsequences=int(counts[:, 2].sum()))
    failures = [(int(i), int(codes[i])) for i in np.flatnonzero(codes)]
    if failures:
        raise JpegDecodeError(failures, pictures.names)
    return pictures


def read(paths, device, unsupported="raise", split=DEFAULT_SPLIT):
    """Read the files, decode them in one call and check -> the list of uint8 [H, W, C] pictures, in the order of `paths`.
    unsupported="pil": the files `parse` rejects (progressive, CMYK, ...) go through PIL on the host and are uploaded; last_info counts
    them as host_decoded.  That is never the default: by default such a file raises ValueError.
    split: decode's -- "never" (the default), "auto", "always".
    What it is worth, measured at 567x1008x3 (tools/jpeg_decode_bench.py, INTEGRATION Z; decode + check against Image.open + upload):
    80 files with restart markers (gscream_amd.jpeg's, the frames of video.MjpegWriter): 22.5 ms, 17.7 ms with split="auto", PIL
    361.4 ms.  80 files without markers (PIL's, a camera's): 238.9 ms by default -- one wavefront walks a whole scan -- and
    13.7 ms with split="auto", PIL 214.1 ms: pass split="auto" for such files.  One file with markers: 6.81 ms, 2.59 ms with
    split="auto", PIL 4.80 ms.  One file without markers STILL LOSES to PIL: 6.67 ms with split="auto" (232.1 ms without)
    against 2.80 ms -- read a single PIL- or camera-written file with PIL.  The default stays "never" (INTEGRATION Z says why)."""
    global last_info
    if unsupported not in ("raise", "pil"):
        raise ValueError(f"jpeg_decode: unsupported={unsupported!r} (have 'raise', 'pil')")
    if split not in SPLITS:
        raise ValueError(f"jpeg_decode: split={split!r} (have {', '.join(repr(v) for v in SPLITS)})")
    paths = [os.fspath(p) for p in paths]
    blobs = []
    for path in paths:
        with open(path, "rb") as f:
            blobs.append(f.read())
    device = torch.device(device)
    images = [None] * len(paths)
    mine = list(range(len(paths)))
    if unsupported == "pil":
        mine = []
        for i, (data, path) in enumerate(zip(blobs, paths)):
            try:
                parse(data, path)
                mine.append(i)
            except ValueError:
                images[i] = torch.from_numpy(_pil_picture(data)).to(device)
    hosted = len(paths) - len(mine)
    if mine:
        pictures = check(decode([blobs[i] for i in mine], device, [paths[i] for i in mine], split=split), host_decoded=hosted)
        for i, image in zip(mine, pictures.images):
            images[i] = image
    else:
        last_info = {"files": hosted, "intervals": 0, "host_decoded": hosted}
    return images
