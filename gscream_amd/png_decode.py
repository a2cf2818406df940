"""Reading PNG files on the HIP path: the bytes of .png files -> uint8 [H, W, C] pictures on the device.  This is the stage between
gscream_amd.png (which writes render_set's files) and gscream_amd.metrics.evaluate_views: readImages in train.py:887-902, which calls
Image.open, to_tensor and .cuda() per file, and Scene's picture loading (scene/dataset_readers.py:113-207).

Integration (INTEGRATION V):

    readImages(renders_dir, gt_dir, mask_dir)              ->  png_decode.read_images(renders_dir, gt_dir, mask_dir)
    the metric loop behind it                              ->  png_decode.evaluate_files(renders_dir, gt_dir, mask_dir)
    Image.open(path) + to_tensor + upload, per picture     ->  png_decode.read(paths, device).images

The host only walks the chunk headers (`parse`): it reads IHDR, lists the chunks as pieces and marks the restart candidates -- an IDAT
whose predecessor ends in 00 00 FF FF, where the deflate stream is on a byte boundary.  The files' bytes, unmodified, and the two
tables go to the device in one copy; inflate, Adler-32, unfilter and CRC-32 run there (gscream_amd/csrc/png_decode.hip,
`last_path = "hip"`), all files of a call in one launch sequence, with no synchronisation: the sizes come from IHDR.  A file whose
segments all stand alone -- every file `png.encode` writes -- is inflated by one wavefront per segment ("parallel"); any other by one
wavefront ("serial").  The rules and the status codes are in include/gsraster.h ("PNG decoding") in full.

Accepted: bit depth 8, no interlace, colour types 0, 2, 4, 6 (C = 1, 3, 2, 4).  Everything else raises ValueError in `parse`, naming
the file and the reason, before any launch; `read(..., unsupported="pil")` sends such files through PIL instead and counts them.

CPU devices and `force_torch = True` decode with PIL per file (`last_path = "torch"`).  A missing library raises; nothing falls back
quietly."""
import ctypes
import io
import os
import struct
from typing import List, NamedTuple

import numpy as np
import torch

from . import _native

__all__ = ["PngError", "PngPictures", "check", "decode", "evaluate_files", "parse", "read", "read_images"]

force_torch = False
last_path = None  # "hip" / "torch": the path the last decode took
last_info = {}    # filled by check / read / read_images: files, segments, parallel, serial, host_decoded, masks_resized (read_images: masks_resized_hip)
use_pil_in_evaluate_files = True  # measured (tools/png_decode_bench.py, INTEGRATION V): the 80-file batch does not beat PIL's loop

_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
_MARKER = b"\x00\x00\xff\xff"
_PIECE = np.dtype([("offset", "<u8"), ("length", "<u4"), ("flags", "<u4"), ("file", "<u4"), ("reserved", "<u4")])  # gsr_png_piece
_FILE = np.dtype([("H", "<i4"), ("W", "<i4"), ("C", "<i4"), ("first_piece", "<i4"), ("piece_count", "<i4"), ("segments", "<i4"),
                  ("out_offset", "<u8"), ("stream_offset", "<u8")])  # gsr_png_file
assert _PIECE.itemsize == 24 and _FILE.itemsize == 40


class PngError(RuntimeError):
    """A file failed on the device: .index (in the call's list), .code (GSR_PNG_*), .failures [(index, code)]."""

    def __init__(self, failures, names=None):
        self.failures = failures
        self.index, self.code = failures[0]
        what = "; ".join(f"file {i}{' (' + str(names[i]) + ')' if names else ''}: code {c}, {_native.PNG_STATUS[c] if 0 <= c < len(_native.PNG_STATUS) else '?'}"
                         for i, c in failures[:8])
        super().__init__(f"png_decode: {len(failures)} file(s) failed: {what}")


class Parsed(NamedTuple):
    """H, W, C from IHDR; pieces: [(data offset, length, flags)] of every chunk in file order (flags: _native.PNG_PIECE_IDAT,
    PNG_PIECE_START on the first IDAT and on every restart candidate); candidates: the indices into `pieces` of the restart candidates."""
    H: int
    W: int
    C: int
    pieces: list
    candidates: list


class PngPictures(NamedTuple):
    """images: uint8 [H, W, C] views of one buffer, one per file; status: int32 [n] on the device (GSR_PNG_* codes, 0 = OK); paths: int32
    [n] on the device (1 = parallel, 0 = serial); segments: per file, from the host parser; names: what `check` calls the files."""
    images: List[torch.Tensor]
    status: torch.Tensor
    paths: torch.Tensor
    segments: tuple = ()
    names: tuple = ()


def parse(data, name="<bytes>"):
    """The bytes of one file -> Parsed.  Walks chunk lengths and types only.  ValueError, naming the file and the reason, for a bad
    signature, a bad IHDR, 16-bit and sub-byte depths, palette, Adam7, a chunk that runs past the end, no IDAT, no IEND, or a zlib
    header that is not deflate with a window of at most 32 KiB and no dictionary."""
    def bad(reason):
        return ValueError(f"png_decode: {name}: {reason}")
    if len(data) < 8 or bytes(data[:8]) != _SIGNATURE:
        raise bad("bad signature")
    at, n = 8, len(data)
    pieces, candidates = [], []
    H = W = C = 0
    seen_idat = seen_iend = restart = False
    head = b""
    while at < n and not seen_iend:
        if n - at < 12:
            raise bad("truncated chunk")
        length, kind = struct.unpack_from(">I4s", data, at)
        if length > n - at - 12:
            raise bad("truncated chunk")
        flags = 0
        if not pieces:
            if kind != b"IHDR" or length != 13:
                raise bad("bad IHDR: the first chunk is not a 13-byte IHDR")
            W, H, depth, colour, compression, filt, interlace = struct.unpack_from(">IIBBBBB", data, at + 8)
            if W == 0 or H == 0 or compression or filt or interlace > 1:
                raise bad("bad IHDR: a zero size or an unknown compression, filter or interlace method")
            if colour == 3:
                raise bad("palette pictures are not decoded")
            if colour not in _CHANNELS:
                raise bad(f"bad IHDR: colour type {colour}")
            if depth != 8:
                raise bad(f"bit depth {depth} is not decoded (16-bit and sub-byte depths)")
            if interlace:
                raise bad("Adam7 interlacing is not decoded")
            C = _CHANNELS[colour]
            if W * C >= 1 << 24 or H * (1 + W * C) >= 0x70000000:
                raise bad("the picture is beyond W*C < 2^24, H*(1 + W*C) < 0x70000000")
        elif kind == b"IDAT":
            flags = _native.PNG_PIECE_IDAT
            if not seen_idat or restart:
                flags |= _native.PNG_PIECE_START
                if seen_idat:
                    candidates.append(len(pieces))
            seen_idat = True
            restart = length >= 4 and bytes(data[at + 8 + length - 4:at + 8 + length]) == _MARKER
            if len(head) < 2:
                head += bytes(data[at + 8:at + 8 + min(length, 2 - len(head))])
        elif kind == b"IEND":
            seen_iend = True
        pieces.append((at + 8, length, flags))
        at += 12 + length
    if not seen_idat:
        raise bad("no IDAT chunk")
    if not seen_iend:
        raise bad("no IEND chunk")
    if len(head) < 2 or head[0] & 15 != 8 or head[0] >> 4 > 7 or head[1] & 32 or (head[0] << 8 | head[1]) % 31:
        raise bad("the zlib header is not deflate with a window of at most 32 KiB and no dictionary")
    return Parsed(H, W, C, pieces, candidates)


def _round16(v):
    return (v + 15) & ~15


def _pil_picture(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    a = np.asarray(im)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8) * 255
    if a.dtype != np.uint8:
        raise ValueError(f"png_decode: PIL gives {a.dtype} pixels (mode {im.mode}); only 8-bit pictures have a uint8 [H, W, C] form")
    return np.array(a.reshape(a.shape[0], a.shape[1], -1))  # (a copy: PIL's buffer is read-only)


def decode(files, device, verify_crc=True, names=None):
    """files: a list of bytes-like objects, one PNG file each, of any sizes and channel counts -> PngPictures on `device`.  One H2D copy
    of one staging buffer (tables and bytes), one launch sequence on torch's current stream, no synchronisation and nothing read back:
    call `check` for that.  Raises ValueError (from `parse`) before anything is launched when a file is outside the accepted subset."""
    global last_path
    device = torch.device(device)
    files = list(files)
    if not files:
        raise ValueError("png_decode: no files")
    names = tuple(names) if names is not None else tuple(f"file {i}" for i in range(len(files)))
    if force_torch or device.type != "cuda":
        last_path = "torch"
        for data, name in zip(files, names):
            parse(data, name)  # the same subset on both paths
        images = [torch.from_numpy(_pil_picture(bytes(d))).to(device) for d in files]
        zeros = torch.zeros(len(files), dtype=torch.int32, device=device)
        return PngPictures(images, zeros, zeros.clone(), tuple(1 for _ in files), names)
    parsed = [parse(data, name) for data, name in zip(files, names)]
    nfiles, npieces = len(files), sum(len(p.pieces) for p in parsed)
    ftab, ptab = np.zeros(nfiles, _FILE), np.zeros(npieces, _PIECE)
    # the staging buffer: file table, piece table, then the files' bytes (each at a multiple of 16)
    off_pieces = _round16(ftab.nbytes)
    off_bytes = off_pieces + _round16(ptab.nbytes)
    starts, at = [], 0
    for data in files:
        starts.append(at)
        at += _round16(len(data))
    nbytes = at
    out_at = stream_at = piece_at = 0
    for i, p in enumerate(parsed):
        arr = np.array(p.pieces, dtype=np.int64).reshape(-1, 3)
        k = len(p.pieces)
        ptab["offset"][piece_at:piece_at + k] = arr[:, 0] + starts[i]
        ptab["length"][piece_at:piece_at + k] = arr[:, 1]
        ptab["flags"][piece_at:piece_at + k] = arr[:, 2]
        ptab["file"][piece_at:piece_at + k] = i
        ftab[i] = (p.H, p.W, p.C, piece_at, k, 1 + len(p.candidates), out_at, stream_at)
        piece_at += k
        out_at += _round16(p.H * p.W * p.C)
        stream_at += _round16(p.H * (1 + p.W * p.C))
    if nbytes >= 1 << 32 or out_at >= 1 << 32:
        raise ValueError("png_decode: a call takes less than 4 GiB of files and of pictures")
    staging = torch.empty(off_bytes + nbytes, dtype=torch.uint8).pin_memory() if torch.cuda.is_available() else torch.empty(off_bytes + nbytes, dtype=torch.uint8)
    host = staging.numpy()
    host[:ftab.nbytes] = ftab.view(np.uint8)
    host[off_pieces:off_pieces + ptab.nbytes] = ptab.view(np.uint8)
    for data, start in zip(files, starts):
        host[off_bytes + start:off_bytes + start + len(data)] = np.frombuffer(data, np.uint8)
    last_path = "hip"
    lib = _native.load()
    with torch.cuda.device(device):
        dev = staging.to(device, non_blocking=True)
        out = torch.empty(max(out_at, 16), dtype=torch.uint8, device=device)
        status = torch.empty((nfiles, 2), dtype=torch.int32, device=device)
        ws_bytes = int(lib.gsr_png_decode_workspace_bytes(stream_at, nfiles, npieces))
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        base = dev.data_ptr()
        _native.run("gsr_png_decode", out.device, ctypes.c_void_p(base + off_bytes), nbytes, ctypes.c_void_p(base), nfiles,
                    ctypes.c_void_p(base + off_pieces), npieces, 1 if verify_crc else 0, _native.ptr(out), out.numel(), _native.ptr(status),
                    _native.ptr(workspace), ws_bytes)
    images = []
    for i, p in enumerate(parsed):
        o = int(ftab["out_offset"][i])
        images.append(out[o:o + p.H * p.W * p.C].view(p.H, p.W, p.C))
    return PngPictures(images, status[:, 0], status[:, 1], tuple(1 + len(p.candidates) for p in parsed), names)


def check(pictures, host_decoded=0, masks_resized=0):
    """The one read-back: the status words of a decode.  Raises PngError (index and code of every failed file) and fills last_info:
    files, segments, parallel, serial, host_decoded."""
    global last_info
    if pictures.status.is_cuda:
        both = torch.stack([pictures.status, pictures.paths]).cpu().numpy()  # one copy
    else:
        both = torch.stack([pictures.status, pictures.paths]).numpy()
    n = both.shape[1]
    parallel = int(both[1].sum())
    last_info = {"files": n + host_decoded, "segments": int(sum(pictures.segments)), "parallel": parallel, "serial": n - parallel,
                 "host_decoded": host_decoded, "masks_resized": masks_resized}
    failures = [(int(i), int(both[0, i])) for i in np.flatnonzero(both[0])]
    if failures:
        raise PngError(failures, pictures.names)
    return pictures


def read(paths, device, unsupported="raise", verify_crc=True):
    """Read the files, decode them in one call and check -> the list of uint8 [H, W, C] pictures, in the order of `paths`.
    unsupported="pil": the files `parse` rejects (16-bit, palette, ...) go through PIL on the host and are uploaded; last_info counts
    them as host_decoded.  That is never the default: by default such a file raises ValueError."""
    global last_info
    if unsupported not in ("raise", "pil"):
        raise ValueError(f"png_decode: unsupported={unsupported!r} (have 'raise', 'pil')")
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
        pictures = check(decode([blobs[i] for i in mine], device, verify_crc, [paths[i] for i in mine]), host_decoded=hosted)
        for i, image in zip(mine, pictures.images):
            images[i] = image
    else:
        last_info = {"files": hosted, "segments": 0, "parallel": 0, "serial": 0, "host_decoded": hosted, "masks_resized": 0}
    return images


def _to_float(image):
    """uint8 [H, W, C] -> fp32 [1, 3, H, W] as to_tensor(...).unsqueeze(0)[:, :3]: x / 255, the first three channels."""
    return (image.permute(2, 0, 1)[None, :3].to(torch.float32) / 255.0)


def read_images(renders_dir, gt_dir, mask_dir, device="cuda", reader="hip", mask_resize="pil"):
    """readImages (train.py:887-902): -> (renders, gts, image_names, masks).  renders and gts are fp32 [1, 3, H, W] (uint8 / 255, the
    first three channels), image_names the file names of renders_dir in os.listdir order, masks bool [1, 3, H, W] (> 0, the channel
    dimension an expand, not materialised).  The mask of `name` is mask_dir/out_%05d.png with the index 1 + int(stem).  All files go to
    the device in one decode.  A mask whose size differs from its render's takes the reference's own
    mask.resize((W, H), Image.LANCZOS) on the host before upload (the reference resizes every mask to 1008 x 567, its render size);
    last_info["masks_resized"] counts them.  reader="pil" reads every file with PIL instead (the reference's way).
    mask_resize="hip" resizes the mask this call has already decoded on the device instead (gscream_amd.resize, LANCZOS, the same
    bytes), when it has one or three channels; a mask with an alpha channel (PNG colour types 4 and 6: PIL premultiplies) and a
    host-decoded file keep the PIL call.  last_info["masks_resized_hip"] counts the device ones among masks_resized."""
    global last_info
    from PIL import Image
    names = list(os.listdir(renders_dir))
    if not names:
        raise ValueError(f"png_decode: no files in {renders_dir}")
    rp = [os.path.join(renders_dir, n) for n in names]
    gp = [os.path.join(gt_dir, n) for n in names]
    mp = [os.path.join(mask_dir, "out_%05d.png" % (1 + int(n.split(".")[0]))) for n in names]
    device = torch.device(device)
    if mask_resize not in ("pil", "hip"):
        raise ValueError(f"png_decode: mask_resize={mask_resize!r} (have 'pil', 'hip')")
    if reader == "pil":
        images = [torch.from_numpy(_pil_picture(open(p, "rb").read())).to(device) for p in rp + gp + mp]
        info = {"files": len(images), "segments": 0, "parallel": 0, "serial": 0, "host_decoded": len(images), "masks_resized": 0}
    elif reader == "hip":
        images = read(rp + gp + mp, device)
        info = dict(last_info)
    else:
        raise ValueError(f"png_decode: reader={reader!r} (have 'hip', 'pil')")
    k = len(names)
    renders, gts, masks = [_to_float(t) for t in images[:k]], [_to_float(t) for t in images[k:2 * k]], []
    resized = resized_hip = 0
    for i, m in enumerate(images[2 * k:]):
        H, W = renders[i].shape[2:]
        if tuple(m.shape[:2]) != (H, W):
            resized += 1
            if mask_resize == "hip" and reader == "hip" and m.is_cuda and m.shape[2] in (1, 3):
                from . import resize as _resize
                m = _resize.resize(m, (W, H), _resize.LANCZOS)
                resized_hip += _resize.last_path == "hip"
            else:
                small = np.asarray(Image.open(mp[i]).resize((W, H), Image.LANCZOS))
                m = torch.from_numpy(np.ascontiguousarray(small.reshape(H, W, -1))).to(device)
        if m.dtype != torch.uint8 or m.shape[2] != 1:
            info["masks_resized"], info["masks_resized_hip"] = resized, int(resized_hip)
            last_info = info  # (the counts up to the mask that is refused)
            raise ValueError(f"png_decode: mask {mp[i]} has {m.shape[2]} channels (readImages expands one channel to three)")
        masks.append((m.permute(2, 0, 1) > 0).expand(3, -1, -1)[None])
    info["masks_resized"] = resized
    info["masks_resized_hip"] = int(resized_hip)
    last_info = info
    return renders, gts, names, masks


def evaluate_files(renders_dir, gt_dir, mask_dir, device="cuda", reader=None, lpips=None, mask_resize=None):
    """read_images, then metrics.evaluate_views: the loop of evaluate() (train.py:905-987) -> (full, per_view); without LPIPS unless
    `lpips` is a gscream_amd.lpips.LPIPS model, which adds the keys "LPIPS" and "masked LPIPS".
    reader: "hip" or "pil"; None takes the module's measured default (INTEGRATION V).  mask_resize: "pil" or "hip" as in read_images;
    None is "pil" (INTEGRATION X has the measurement)."""
    from . import metrics
    if reader is None:
        reader = "pil" if use_pil_in_evaluate_files else "hip"
    renders, gts, names, masks = read_images(renders_dir, gt_dir, mask_dir, device, reader, "pil" if mask_resize is None else mask_resize)
    return metrics.evaluate_views(renders, gts, masks, names, lpips=lpips)
