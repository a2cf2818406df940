"""Baseline JPEG files on the HIP path: finished uint8 pictures (gscream_amd.frames) -> the bytes of their .jpg files, on the device,
ready for one D2H copy.  The lossy frames of gscream_amd.video (the spiral video of render_set, train.py:844-846; INTEGRATION Y).

The rules (include/gsraster.h has them in full, tests/jpeg_helpers.py states them in numpy): JFIF 1.01, SOF0, the typical Huffman
tables of Annex K.3 (what PIL writes with optimize=False), Annex K's quantisation tables scaled to `quality` as libjpeg does, 4:4:4 or
4:2:0, an integer colour transform, an integer 8x8 DCT in two passes, restart intervals.  Every step is integer arithmetic, so a
picture has ONE file: the device and the host path below give the same bytes.

The HIP path (gscream_amd/csrc/jpeg.hip; `last_path = "hip"`) takes uint8 tensors on a HIP device, [H, W, C] or [B, H, W, C] with C = 1
or 3, the inner two dimensions dense and the row and picture strides free -- a panel of a wider sheet is read in place -- launches four
kernels on torch's current stream, allocates its output and a workspace, reads nothing back and never synchronises.  CPU tensors and
`force_torch = True` take the host statement (`last_path = "torch"`), which also serves `restart_interval=0`: no restart markers, which
the device does not write (its unit of parallel work is the restart interval).  A missing library raises; nothing falls back quietly."""
import json
import os
import struct
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _native

__all__ = ["JpegBatch", "capacity", "encode", "save", "to_bytes"]

force_torch = False
last_path = None  # "hip" / "torch": the path the last encode took
last_info = {"reencoded": 0}  # to_bytes: pictures whose first buffer was too small

HEADER = _native.JPEG_HEADER_BYTES            # four uint32 words {file bytes, status, restart intervals, 0} in front of every file
INTERVAL_BLOCKS = _native.JPEG_INTERVAL_BLOCKS
NEED_CAPACITY = _native.JPEG_NEED_CAPACITY
MAX_PICTURES = 65535
_SUBSAMPLING = {"4:4:4": 444, "4:2:0": 420, 444: 444, 420: 420}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_tables.json")) as _f:
    TABLES = json.load(_f)  # tools/make_jpeg_tables.py
_ZIGZAG = np.array(TABLES["zigzag"])


class JpegBatch(NamedTuple):
    """data: uint8 [B, HEADER + cap] on the pictures' device, row b = the header words, then picture b's file (if it fits);
    shape = (H, W, C); batched: whether `encode` was given [B, H, W, C]; images and settings: what to_bytes encodes again from."""
    data: torch.Tensor
    shape: Tuple[int, int, int]
    batched: bool
    images: torch.Tensor
    quality: int
    subsampling: int
    restart_interval: Optional[int]


def _geometry(H, W, C, sub):
    mcu = 16 if (C == 3 and sub == 420) else 8
    bpm = 1 if C == 1 else (6 if sub == 420 else 3)
    return mcu, bpm, -(-W // mcu), -(-H // mcu)


def file_header_bytes(C):
    return 629 if C == 3 else 334


def capacity(H, W, C, subsampling="4:2:0"):
    """gsr_jpeg_capacity: no file of an [H, W, C] picture is larger (file header + 416 per block + 3 per MCU + 2)."""
    sub = _check_subsampling(subsampling, C)
    _, bpm, mx, my = _geometry(H, W, C, sub)
    return file_header_bytes(C) + 416 * mx * my * bpm + 3 * mx * my + 2


def _check_subsampling(subsampling, C):
    if subsampling not in _SUBSAMPLING:
        raise ValueError(f"jpeg: subsampling {subsampling!r} (have '4:4:4', '4:2:0')")
    sub = _SUBSAMPLING[subsampling]
    if sub == 420 and C == 1:
        raise ValueError("jpeg: subsampling '4:2:0' with a grey picture (it has no chroma; pass '4:4:4')")
    return sub


# ---- the host statement ----
def _huffman(table):
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, at = 0, 0
    for n in range(1, 17):
        for _ in range(table["bits"][n - 1]):
            code[table["values"][at]], length[table["values"][at]] = c, n
            c += 1
            at += 1
        c <<= 1
    return code, length


_HUFF = {k: _huffman(TABLES["huffman"][k]) for k in ("dc0", "dc1", "ac0", "ac1")}
_K, _N = np.mgrid[0:8, 0:8]
_DCT = np.rint(8192.0 * np.where(_K == 0, 1.0 / np.sqrt(8.0), 0.5) * np.cos((2 * _N + 1) * _K * np.pi / 16.0)).astype(np.int64)
assert _DCT.tolist() == TABLES["dct"]


def quant_tables(quality):
    """int64 [2, 64], natural order: Annex K.1 / K.2 scaled as libjpeg does."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array(TABLES["quant"], dtype=np.int64) * scale + 50) // 100, 1, 255)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def _file_header(H, W, C, quality, sub, ri):
    Q = quant_tables(quality)
    parts = [b"\xff\xd8", _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    parts += [_segment(0xDB, bytes([t]) + Q[t][_ZIGZAG].astype(np.uint8).tobytes()) for t in range(2 if C == 3 else 1)]
    comps = b"".join(bytes([c + 1, 0x22 if (c == 0 and sub == 420) else 0x11, min(c, 1)]) for c in range(C))
    parts.append(_segment(0xC0, struct.pack(">BHHB", 8, H, W, C) + comps))
    for key, ident in (("dc0", 0x00), ("ac0", 0x10), ("dc1", 0x01), ("ac1", 0x11))[:4 if C == 3 else 2]:
        parts.append(_segment(0xC4, bytes([ident]) + bytes(TABLES["huffman"][key]["bits"]) + bytes(TABLES["huffman"][key]["values"])))
    if ri:
        parts.append(_segment(0xDD, struct.pack(">H", ri)))
    parts.append(_segment(0xDA, bytes([C]) + b"".join(bytes([c + 1, 0x11 * min(c, 1)]) for c in range(C)) + b"\x00\x3f\x00"))
    return b"".join(parts)


def _coefficients(image, quality, sub):
    """uint8 numpy [H, W, C] -> int64 [blocks, 64] in scan order, zigzag order, and the blocks' component numbers."""
    H, W, C = image.shape
    mcu, bpm, mx, my = _geometry(H, W, C, sub)
    yy, xx = np.minimum(np.arange(my * mcu), H - 1), np.minimum(np.arange(mx * mcu), W - 1)  # the padding rule
    full = image[yy][:, xx].astype(np.int64)
    if C == 1:
        planes = [full[..., 0]]
    else:
        R, G, B = full[..., 0], full[..., 1], full[..., 2]
        planes = [(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
                  (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
                  (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16]
        if sub == 420:
            bias = 1 + (np.arange(mx * 8) & 1)
            planes[1:] = [(p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2 for p in planes[1:]]
    Q = quant_tables(quality)
    per = []
    for c, p in enumerate(planes):
        x = p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3) - 128  # [by, bx, m, n]
        r = (x @ _DCT.T + 512) >> 10                                                         # [.., m, k]
        c8 = (_DCT @ r + 4096) >> 13                                                         # [.., k, j]
        q = Q[min(c, 1)].reshape(8, 8)
        v = np.where(c8 < 0, -((-c8 + 4 * q) // (8 * q)), (c8 + 4 * q) // (8 * q))
        per.append(v.reshape(v.shape[0], v.shape[1], 64)[..., _ZIGZAG])
    if bpm == 6:
        Y = per[0].reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
        coef = np.concatenate([Y, per[1][:, :, None], per[2][:, :, None]], 2)
        comp = np.array([0, 0, 0, 0, 1, 2])
    else:
        coef = np.stack(per, 2)
        comp = np.arange(bpm)
    return coef.reshape(-1, 64), np.tile(comp, mx * my)


def _bit_length(a):
    out = np.zeros(a.shape, np.int64)
    for n in range(12):
        out += a >= (1 << n)
    return out


def _intervals_host(z, comp, iv0):
    """The scan bytes (unstuffed, every interval padded to a byte with 1 bits) of the blocks z [N, 64] whose interval numbers are iv0
    [N] (ascending); -> (uint8 bytes, the intervals' byte counts)."""
    N = z.shape[0]
    tab = np.minimum(comp, 1)
    diff = z[:, 0].copy()
    for c in range(int(comp.max()) + 1):
        sel = np.flatnonzero(comp == c)
        if sel.size > 1:
            same = iv0[sel][1:] == iv0[sel][:-1]
            diff[sel[1:]] -= np.where(same, z[sel[:-1], 0], 0)
    # one row of 65 slots per block: DC, the 63 AC positions, EOB; a slot is up to three ZRLs and a code with its value bits
    size = _bit_length(np.abs(diff))
    dcode = np.stack([_HUFF["dc0"][0], _HUFF["dc1"][0]])[tab, size]
    dlen = np.stack([_HUFF["dc0"][1], _HUFF["dc1"][1]])[tab, size]
    acode, alen = np.stack([_HUFF["ac0"][0], _HUFF["ac1"][0]]), np.stack([_HUFF["ac0"][1], _HUFF["ac1"][1]])
    bi, kk = np.nonzero(z[:, 1:])
    kk = kk + 1
    v = z[bi, kk]
    prev = np.where(np.concatenate([[False], bi[1:] == bi[:-1]]), np.concatenate([[0], kk[:-1]]), 0)
    run = kk - prev - 1
    vs = _bit_length(np.abs(v))
    sym = ((run & 15) << 4) | vs
    t = tab[bi]
    # every token as (order key, value, bit count); ZRLs in front of their value
    z_rep = np.repeat(np.arange(bi.size), run >> 4)
    z_sub = np.arange(z_rep.size) - np.repeat(np.cumsum(run >> 4) - (run >> 4), run >> 4)
    eob = np.flatnonzero(z[:, 63] == 0)
    key = np.concatenate([np.arange(N) * 512, bi * 512 + kk * 4 + 3, bi[z_rep] * 512 + kk[z_rep] * 4 + z_sub, eob * 512 + 511])
    val = np.concatenate([(dcode << size) | ((diff - (diff < 0)) & ((1 << size) - 1)),
                          (acode[t, sym] << vs) | ((v - (v < 0)) & ((1 << vs) - 1)), acode[t[z_rep], 0xF0], acode[tab[eob], 0x00]])
    cnt = np.concatenate([dlen + size, alen[t, sym] + vs, alen[t[z_rep], 0xF0], alen[tab[eob], 0x00]])
    order = np.argsort(key, kind="stable")
    val, cnt, tiv = val[order], cnt[order], iv0[key[order] // 512]
    # the tokens' bits, MSB first, interval by interval
    ivs, first = np.unique(tiv, return_index=True)
    ibits = np.add.reduceat(cnt, first)
    pad = -ibits % 8
    total_bits = int((ibits + pad).sum())
    bits = np.ones(total_bits, np.uint8)  # (what no token covers is an interval's padding)
    tok_start = np.cumsum(cnt) - cnt + np.repeat(np.cumsum(pad) - pad, np.diff(np.concatenate([first, [cnt.size]])))
    owner = np.repeat(np.arange(cnt.size), cnt)
    within = np.arange(owner.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    bits[tok_start[owner] + within] = (val[owner] >> (cnt[owner] - 1 - within)) & 1
    return np.packbits(bits), (ibits + pad) // 8


def _encode_host(image, quality, sub, ri):
    """uint8 numpy [H, W, C] -> (the file's bytes, its restart intervals).  ri = 0: no restart markers."""
    H, W, C = image.shape
    _, bpm, mx, my = _geometry(H, W, C, sub)
    z, comp = _coefficients(image, quality, sub)
    iv = (np.arange(z.shape[0]) // bpm) // ri if ri else np.zeros(z.shape[0], np.int64)
    nint = int(iv[-1]) + 1
    parts = [_file_header(H, W, C, quality, sub, ri)]
    per = max(1, 16384 // max(1, ri * bpm))  # intervals per slice: the bit image of a slice stays small
    for i0 in range(0, nint, per):
        sel = slice(i0 * ri * bpm, min(z.shape[0], (i0 + per) * ri * bpm)) if ri else slice(None)
        raw, sizes = _intervals_host(z[sel], comp[sel], iv[sel])
        at = 0
        for j, n in enumerate(sizes.tolist()):
            parts.append(raw[at:at + n].tobytes().replace(b"\xff", b"\xff\x00"))
            at += n
            if i0 + j < nint - 1:
                parts.append(bytes([0xFF, 0xD0 + ((i0 + j) & 7)]))
    parts.append(b"\xff\xd9")
    return b"".join(parts), nint


# ---- the calls ----
def _check_images(images):
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8:
        raise TypeError("jpeg: a uint8 tensor")
    batched = images.dim() == 4
    if images.dim() == 3:
        images = images[None]
    if images.dim() != 4 or images.shape[3] not in (1, 3) or 0 in images.shape:
        raise ValueError(f"jpeg: images are {tuple(images.shape)} (need [H, W, C] or [B, H, W, C] with C = 1 or 3, none empty)")
    B, H, W, C = images.shape
    if B > MAX_PICTURES or H > 65535 or W > 65535:
        raise ValueError(f"jpeg: images of {tuple(images.shape)} are beyond B, H, W <= 65535")
    return images, batched


def _check_settings(C, quality, subsampling, restart_interval, W):
    if not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"jpeg: quality {quality!r} (need an integer 1 .. 100)")
    sub = _check_subsampling(subsampling, C)
    bpm = 1 if C == 1 else (6 if sub == 420 else 3)
    most = INTERVAL_BLOCKS // bpm
    if restart_interval is None:
        ri = min(-(-W // (16 if bpm == 6 else 8)), most)
    elif not isinstance(restart_interval, int) or not 0 <= restart_interval <= most:
        raise ValueError(f"jpeg: restart_interval {restart_interval!r} (need None = one MCU row, 0 = no markers, or 1 .. {most} MCUs)")
    else:
        ri = restart_interval
    return sub, ri


def encode(images, quality=95, subsampling="4:2:0", restart_interval=None, out=None, cap=None):
    """uint8 [H, W, C] or [B, H, W, C] (C = 1, 3: grey, RGB) -> JpegBatch.  The inner two dimensions are dense, the row stride and the
    picture stride are free (anything else is copied first).  restart_interval: MCUs per interval; None = the MCUs of one MCU row (at
    most INTERVAL_BLOCKS blocks); 0 = no markers (host path only).  cap: the room for a file, default file header + H W C (the raw
    picture's size: photographs take a tenth of it; `capacity()` always fits); a file beyond it reports NEED_CAPACITY and to_bytes
    encodes it again.  out: a dense uint8 [B, HEADER + cap'] buffer on the pictures' device, its row length a multiple of 4; its cap'
    is used.  No synchronisation on the HIP path."""
    global last_path
    images, batched = _check_images(images)
    B, H, W, C = images.shape
    sub, ri = _check_settings(C, quality, subsampling, restart_interval, W)
    if capacity(H, W, C, sub) >= 1 << 31:
        raise ValueError(f"jpeg: images of {tuple(images.shape)} have a capacity of 2^31 bytes or more")
    least = HEADER + file_header_bytes(C)
    if out is None:
        cap = file_header_bytes(C) + H * W * C if cap is None else int(cap)
        if cap < file_header_bytes(C):
            raise ValueError(f"jpeg: cap {cap} is below the file header's {file_header_bytes(C)} bytes")
        out = torch.empty((B, (HEADER + cap + 3) & ~3), dtype=torch.uint8, device=images.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != B or out.shape[1] < least
          or out.device != images.device or not out.is_contiguous() or out.shape[1] % 4 or out.data_ptr() % 4):
        raise ValueError(f"jpeg: out is a dense uint8 [{B}, >= {least}] buffer on {images.device}, row length and address multiples of 4")
    room = out.shape[1] - HEADER
    if force_torch or not images.is_cuda:
        last_path = "torch"
        host = images.cpu().numpy()
        for b in range(B):
            data, nint = _encode_host(host[b], quality, sub, ri)
            fits = len(data) <= room
            row = struct.pack("<IIII", len(data), 0 if fits else NEED_CAPACITY, nint, 0) + (data if fits else b"")
            out[b, :len(row)] = torch.frombuffer(bytearray(row), dtype=torch.uint8).to(out.device)
        return JpegBatch(out, (H, W, C), batched, images, quality, sub, ri)
    if ri == 0:
        raise ValueError("jpeg: restart_interval=0 (no markers) is the host path's; the device codes one restart interval per workgroup")
    last_path = "hip"
    sb, sy, sx, sc = images.stride()
    if sc != 1 or sx != C or sy < W * C or (B > 1 and sb < 0):
        images = images.contiguous()
        sb, sy, sx, sc = images.stride()
    lib = _native.load()
    workspace = torch.empty(int(lib.gsr_jpeg_workspace_bytes(B, H, W, C, sub, ri)), dtype=torch.uint8, device=images.device)
    _native.run("gsr_jpeg_encode", images.device, _native.ptr(images), sy, sb, B, H, W, C, quality, sub, ri, _native.ptr(out), out.stride(0),
                _native.ptr(workspace))
    return JpegBatch(out, (H, W, C), batched, images, quality, sub, ri)


def to_bytes(batch):
    """JpegBatch -> the files as a list of bytes: ONE copy of the buffer to the host (which waits for the encode), then slices of it.
    Pictures that reported NEED_CAPACITY are encoded once more, together, into buffers of `capacity()` and read back;
    last_info["reencoded"] counts them."""
    host = batch.data.cpu().numpy()
    H, W, C = batch.shape
    files, again = [], []
    for b, row in enumerate(host):
        n, status = (int(v) for v in row[:8].view("<u4"))
        if status == NEED_CAPACITY:
            again.append(b)
            files.append(None)
            continue
        if status != 0 or not 0 < n <= row.size - HEADER:
            raise RuntimeError(f"jpeg: a header says status {status}, {n} bytes in a buffer of {row.size - HEADER}")
        files.append(row[HEADER:HEADER + n].tobytes())
    last_info["reencoded"] = len(again)
    if again:
        pictures = batch.images[torch.as_tensor(again, device=batch.images.device)] if len(again) < len(files) else batch.images
        full = encode(pictures, batch.quality, batch.subsampling, batch.restart_interval, cap=capacity(H, W, C, batch.subsampling))
        for b, row in zip(again, full.data.cpu().numpy()):
            n, status = (int(v) for v in row[:8].view("<u4"))
            if status != 0 or not 0 < n <= row.size - HEADER:
                raise RuntimeError(f"jpeg: a header says status {status}, {n} bytes in a buffer of capacity {row.size - HEADER}")
            files[b] = row[HEADER:HEADER + n].tobytes()
    return files


def save(images, paths, quality=95, subsampling="4:2:0", restart_interval=None):
    """encode, one copy, and the files: `paths` is one path for [H, W, C], a sequence of B paths for [B, H, W, C]."""
    batch = encode(images, quality, subsampling, restart_interval)
    files, paths = to_bytes(batch), (list(paths) if batch.batched else [paths])
    if len(files) != len(paths):
        raise ValueError(f"jpeg: {len(files)} pictures and {len(paths)} paths")
    for data, path in zip(files, paths):
        with open(path, "wb") as f:
            f.write(data)
