"""The baseline JPEG rules of include/gsraster.h ("JPEG encoding") stated in numpy, the strict parsers that hold files against
them, and the test pictures.  Nothing here imports the package's encoder: gscream_amd/jpeg.py's host path and jpeg.hip are both held
against `encode` byte for byte.

encode(image, quality, subsampling, ri)   uint8 [H, W, C] (C = 1, 3) -> the file's bytes.  ri: None = the default interval (the MCUs of
                                          one MCU row, at most INTERVAL_BLOCKS blocks), 0 = no restart markers (and no DRI), else MCUs.
encode(..., stats=True)                   -> (bytes, {"zrl", "no_eob", "stuffed", "ff_pairs", "dc11", "intervals"})
parse(data)                               strict marker parser -> dict; raises AssertionError on anything the rules do not allow
parse_avi(data)                           strict RIFF parser of video.MjpegWriter's container -> dict
"""
import json
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "gscream_amd", "jpeg_tables.json")) as _f:
    TABLES = json.load(_f)
ZIGZAG = np.array(TABLES["zigzag"])
INTERVAL_BLOCKS = 1024
KINDS = ("texture", "noise", "ramp", "constant", "edges")
_BITLEN = np.array([int(v).bit_length() for v in range(4096)])


def picture(kind, H, W, C=3, seed=0):
    """The five kinds of content: uint8 [H, W, C]."""
    rng = np.random.default_rng(seed + 17 * KINDS.index(kind))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "texture":
        ch = [128 + 60 * np.sin(0.21 * x + 0.13 * y + c) + 40 * np.sin(0.05 * x * (c + 1) - 0.31 * y) + 12 * rng.standard_normal((H, W)) for c in range(C)]
        img = np.stack(ch, -1)
    elif kind == "noise":
        img = rng.integers(0, 256, (H, W, C)).astype(np.float64)
    elif kind == "ramp":
        img = np.stack([7.0 + 241.0 * (x + (c + 1) * y) / max(1.0, (W - 1) + (c + 1) * (H - 1)) for c in range(C)], -1)
    elif kind == "constant":
        img = np.broadcast_to(np.array([200.0, 37.0, 99.0] if C == 3 else [201.0]), (H, W, C))
    else:  # two levels: 16-pixel cells in the left half (whole blocks flip: the largest DC steps), 5-pixel cells in the right half
        coarse = rng.integers(0, 2, (H // 16 + 1, W // 16 + 1, C))[(y // 16).astype(int), (x // 16).astype(int)]
        fine = rng.integers(0, 2, (H // 5 + 1, W // 5 + 1, C))[(y // 5).astype(int), (x // 5).astype(int)]
        img = 14.0 + 227.0 * np.where((x < W // 2)[..., None], coarse, fine)
    return np.ascontiguousarray(np.clip(np.rint(img), 0, 255).astype(np.uint8))


# ---- the rules ----
def dct_matrix():
    k, n = np.mgrid[0:8, 0:8]
    s = np.where(k == 0, 1.0 / np.sqrt(8.0), 0.5)
    return np.rint(8192.0 * s * np.cos((2 * n + 1) * k * np.pi / 16.0)).astype(np.int64)


def quant_tables(quality):
    """[2, 64] natural order."""
    assert 1 <= quality <= 100
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array(TABLES["quant"], dtype=np.int64) * s + 50) // 100, 1, 255)


def huffman_codes(table):
    """{bits, values} -> (code[256], length[256]) by Annex C."""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, at = 0, 0
    for n in range(1, 17):
        for _ in range(table["bits"][n - 1]):
            code[table["values"][at]], length[table["values"][at]] = c, n
            c += 1
            at += 1
        c <<= 1
    return code, length


def geometry(H, W, C, subsampling, ri=None):
    mcu = 16 if (C == 3 and subsampling == "4:2:0") else 8
    bpm = 1 if C == 1 else (6 if subsampling == "4:2:0" else 3)
    mcux, mcuy = -(-W // mcu), -(-H // mcu)
    if ri is None:
        ri = min(mcux, INTERVAL_BLOCKS // bpm)
    mcus = mcux * mcuy
    return dict(mcu=mcu, bpm=bpm, mcux=mcux, mcuy=mcuy, ri=ri, mcus=mcus, blocks=mcus * bpm, intervals=-(-mcus // ri) if ri else 1)


def file_header_bytes(C):
    return 629 if C == 3 else 334


def capacity(H, W, C, subsampling):
    g = geometry(H, W, C, subsampling)
    return file_header_bytes(C) + 416 * g["blocks"] + 3 * g["mcus"] + 2


def planes(image, subsampling):
    H, W, C = image.shape
    mcu = 16 if (C == 3 and subsampling == "4:2:0") else 8
    pad = lambda p: np.pad(p, ((0, -H % mcu), (0, -W % mcu)), mode="edge")
    if C == 1:
        return [pad(image[..., 0].astype(np.int64))]
    R, G, B = (image[..., c].astype(np.int64) for c in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    out = [pad(Y), pad(Cb), pad(Cr)]
    if subsampling == "4:2:0":
        for c in (1, 2):
            p = out[c]
            bias = 1 + (np.arange(p.shape[1] // 2) & 1)
            out[c] = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return out


def fdct(blocks):
    """[..., 8, 8] samples -> c8 [..., 8, 8] = 8 x the orthonormal DCT, by the two integer passes."""
    Cm = dct_matrix()
    x = blocks.astype(np.int64) - 128
    most = int(np.abs(Cm).sum(1).max())  # 23168: |a| <= 128 * 23168 < 2^22, |r| <= 2897, |b| <= 2897 * 23168 < 2^27: all int32
    a = np.einsum("kn,...mn->...mk", Cm, x)
    assert np.abs(a).max(initial=0) <= 128 * most < 1 << 22
    r = (a + 512) >> 10
    b = np.einsum("km,...mj->...kj", Cm, r)
    assert np.abs(b).max(initial=0) <= 2897 * most < 1 << 27
    return (b + 4096) >> 13


def coefficients(image, quality, subsampling):
    """-> int64 [MCUs, blocks per MCU, 64]: quantised, zigzag order, scan order."""
    H, W, C = image.shape
    g = geometry(H, W, C, subsampling)
    Q = quant_tables(quality)
    per = []
    for c, p in enumerate(planes(image, subsampling)):
        blocks = p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)
        c8 = fdct(blocks)
        q = Q[1 if c else 0].reshape(8, 8)
        v = np.sign(c8) * ((np.abs(c8) + 4 * q) // (8 * q))
        per.append(v.reshape(v.shape[0], v.shape[1], 64)[..., ZIGZAG])
    my, mx = g["mcuy"], g["mcux"]
    if g["bpm"] == 6:
        Y = per[0].reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
        out = np.concatenate([Y, per[1][:, :, None], per[2][:, :, None]], 2)
    else:
        out = np.stack(per, 2)
    return out.reshape(my * mx, g["bpm"], 64)


def _value_bits(v, size):
    return (v + (v >> 63)) & ((1 << size) - 1)


def scan(coef, ri):
    """int64 [MCUs, bpm, 64] -> (the scan's bytes with stuffing and RST markers, stats)."""
    M, bpm, _ = coef.shape
    N = M * bpm
    z = coef.reshape(N, 64)
    blk = np.arange(N)
    comp = np.array({1: [0], 3: [0, 1, 2], 6: [0, 0, 0, 0, 1, 2]}[bpm])[blk % bpm]
    tab = (comp > 0).astype(np.int64)
    interval = (blk // bpm) // ri if ri else np.zeros(N, np.int64)
    nint = int(interval[-1]) + 1
    dcc, dcl = (np.stack(t) for t in zip(huffman_codes(TABLES["huffman"]["dc0"]), huffman_codes(TABLES["huffman"]["dc1"])))
    acc, acl = (np.stack(t) for t in zip(huffman_codes(TABLES["huffman"]["ac0"]), huffman_codes(TABLES["huffman"]["ac1"])))
    # DC: the difference against the previous block of the same component, 0 at the start of an interval
    diff = z[:, 0].copy()
    for c in range(comp.max() + 1):
        sel = np.flatnonzero(comp == c)
        d, iv = z[sel, 0], interval[sel]
        prev = np.concatenate([[0], d[:-1]])
        prev[np.concatenate([[True], iv[1:] != iv[:-1]])] = 0
        diff[sel] = d - prev
    size = _BITLEN[np.abs(diff)]
    assert size.max() <= 11
    keys = [blk * 260 + 3]
    vals = [(dcc[tab, size] << size) | _value_bits(diff, size)]
    lens = [dcl[tab, size] + size]
    # AC: (run, size) symbols, a ZRL for every 16 zeros in front of a value, EOB unless coefficient 63 is non-zero
    bi, pos = np.nonzero(z[:, 1:])
    pos = pos + 1
    v = z[bi, pos]
    same = np.concatenate([[False], bi[1:] == bi[:-1]])
    run = pos - np.where(same, np.concatenate([[0], pos[:-1]]), 0) - 1
    nzrl, size = run >> 4, _BITLEN[np.abs(v)]
    assert size.max(initial=0) <= 10
    sym = ((run & 15) << 4) | size
    assert (acl[tab[bi], sym] > 0).all()
    keys.append(bi * 260 + pos * 4 + 3)
    vals.append((acc[tab[bi], sym] << size) | _value_bits(v, size))
    lens.append(acl[tab[bi], sym] + size)
    rep = np.repeat(np.arange(bi.size), nzrl)
    sub = np.arange(rep.size) - np.repeat(np.cumsum(nzrl) - nzrl, nzrl)
    keys.append(bi[rep] * 260 + pos[rep] * 4 + sub)
    vals.append(acc[tab[bi[rep]], 0xF0])
    lens.append(acl[tab[bi[rep]], 0xF0])
    eob = np.flatnonzero(z[:, 63] == 0)
    keys.append(eob * 260 + 256)
    vals.append(acc[tab[eob], 0])
    lens.append(acl[tab[eob], 0])
    keys, vals, lens = np.concatenate(keys), np.concatenate(vals), np.concatenate(lens)
    order = np.argsort(keys, kind="stable")
    keys, vals, lens = keys[order], vals[order], lens[order]
    tiv = interval[keys // 260]
    # bit positions: every interval starts on a byte; its last byte is filled with 1 bits
    ends = np.cumsum(lens)
    first = np.searchsorted(tiv, np.arange(nint))
    last = np.concatenate([first[1:], [tiv.size]]) - 1
    base_bits = (ends - lens)[first]
    ibits = ends[last] - base_bits
    ibytes = (ibits + 7) >> 3
    istart = np.cumsum(ibytes) - ibytes
    bitpos = 8 * istart[tiv] + (ends - lens) - base_bits[tiv]
    padn = 8 * ibytes - ibits
    bitpos = np.concatenate([bitpos, 8 * istart + ibits])
    vals = np.concatenate([vals, (1 << padn) - 1])
    lens = np.concatenate([lens, padn])
    total = int(ibytes.sum())
    # a token is at most 27 bits: with its offset in the first byte it lies in a window of five bytes
    assert lens.max() <= 27
    window = vals << (40 - (bitpos & 7) - lens)
    raw = np.zeros(total + 5)
    for j in range(5):
        raw += np.bincount((bitpos >> 3) + j, weights=((window >> (8 * (4 - j))) & 255).astype(np.float64), minlength=total + 5)
    raw = raw[:total].astype(np.uint8)
    # stuffing and the RST markers
    ff = raw == 255
    cum = np.concatenate([[0], np.cumsum(ff)])
    which = np.repeat(np.arange(nint), ibytes)
    out = np.zeros(total + int(ff.sum()) + 2 * (nint - 1), np.uint8)
    out[np.arange(total) + cum[:-1] + 2 * which] = raw
    starts = istart + cum[istart] + 2 * np.arange(nint)
    out[starts[1:] - 2] = 0xFF
    out[starts[1:] - 1] = 0xD0 + ((np.arange(nint - 1)) & 7)
    stats = dict(zrl=int(nzrl.sum()), no_eob=int(N - eob.size), stuffed=int(ff.sum()), ff_pairs=int((ff[1:] & ff[:-1]).sum()),
                 dc11=int((_BITLEN[np.abs(diff)] == 11).sum()), intervals=nint)
    return out.tobytes(), stats


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def file_header(H, W, C, quality, subsampling, ri):
    """SOI .. SOS."""
    Q = quant_tables(quality)
    parts = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))]
    for t in range(2 if C == 3 else 1):
        parts.append(_segment(0xDB, bytes([t]) + bytes(int(q) for q in Q[t][ZIGZAG])))
    comps = b"".join(bytes([c + 1, 0x22 if (c == 0 and subsampling == "4:2:0") else 0x11, 1 if c else 0]) for c in range(C))
    parts.append(_segment(0xC0, bytes([8]) + struct.pack(">HH", H, W) + bytes([C]) + comps))
    for key, ident in (("dc0", 0x00), ("ac0", 0x10), ("dc1", 0x01), ("ac1", 0x11))[:4 if C == 3 else 2]:
        h = TABLES["huffman"][key]
        parts.append(_segment(0xC4, bytes([ident]) + bytes(h["bits"]) + bytes(h["values"])))
    if ri:
        parts.append(_segment(0xDD, struct.pack(">H", ri)))
    parts.append(_segment(0xDA, bytes([C]) + b"".join(bytes([c + 1, 0x11 if c else 0x00]) for c in range(C)) + bytes([0, 63, 0])))
    return b"".join(parts)


def encode(image, quality=95, subsampling="4:2:0", ri=None, stats=False):
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] in (1, 3)
    H, W, C = image.shape
    if C == 1:
        subsampling = "4:4:4"
    g = geometry(H, W, C, subsampling, ri)
    assert g["ri"] == 0 or 1 <= g["ri"] <= INTERVAL_BLOCKS // g["bpm"]
    body, st = scan(coefficients(image, quality, subsampling), g["ri"])
    data = file_header(H, W, C, quality, subsampling, g["ri"]) + body + b"\xff\xd9"
    assert len(data) <= capacity(H, W, C, subsampling) or g["ri"] == 0
    return (data, st) if stats else data


# ---- the strict marker parser ----
def parse(data):
    """Segment order and lengths, the DRI value, no unstuffed 0xFF in the scan, RST numbers cycling at the right MCU counts (by
    counting intervals: their number must be ceil(MCUs / Ri)), EOI last and nothing behind it."""
    assert data[:2] == b"\xff\xd8", "SOI"
    at, seen, info = 2, [], {"dri": 0}
    while True:
        assert data[at] == 0xFF and data[at + 1] not in (0x00, 0xFF), f"marker expected at {at}"
        marker, n = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])[0]
        p = data[at + 4:at + 2 + n]
        assert len(p) == n - 2, "segment runs past the file"
        seen.append(marker)
        if marker == 0xE0:
            assert p == b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]), "APP0"
        elif marker == 0xDB:
            assert n == 67 and p[0] in (0, 1), "DQT: one 8-bit table per segment"
            info.setdefault("dqt", []).append(p[0])
        elif marker == 0xC0:
            assert p[0] == 8 and n == 8 + 3 * p[5], "SOF0"
            info["H"], info["W"], info["C"] = struct.unpack(">HH", p[1:5]) + (p[5],)
            info["sampling"] = [p[7 + 3 * c] for c in range(p[5])]
            assert [p[6 + 3 * c] for c in range(p[5])] == [1, 2, 3][:p[5]] and [p[8 + 3 * c] for c in range(p[5])] == [0, 1, 1][:p[5]]
        elif marker == 0xC4:
            assert n == 2 + 1 + 16 + sum(p[1:17]), "DHT: one table per segment"
            info.setdefault("dht", []).append(p[0])
        elif marker == 0xDD:
            assert n == 4
            info["dri"] = struct.unpack(">H", p)[0]
        elif marker == 0xDA:
            C = info["C"]
            assert n == 6 + 2 * C and p[0] == C and p[-3:] == bytes([0, 63, 0]), "SOS"
            assert [(p[1 + 2 * c], p[2 + 2 * c]) for c in range(C)] == [(1, 0x00), (2, 0x11), (3, 0x11)][:C]
            at += 2 + n
            break
        else:
            raise AssertionError(f"unexpected marker 0x{marker:02x}")
        at += 2 + n
    C = info["C"]
    want = [0xE0] + [0xDB] * (2 if C == 3 else 1) + [0xC0] + [0xC4] * (4 if C == 3 else 2) + ([0xDD] if info["dri"] else []) + [0xDA]
    assert seen == want, f"segment order {[hex(m) for m in seen]}"
    assert info["dqt"] == [0, 1][:2 if C == 3 else 1] and info["dht"] == [0x00, 0x10, 0x01, 0x11][:4 if C == 3 else 2]
    assert info["sampling"] in ([0x11], [0x11, 0x11, 0x11], [0x22, 0x11, 0x11])
    info["header_bytes"] = at
    assert data[-2:] == b"\xff\xd9", "EOI last"
    body = np.frombuffer(data, np.uint8)[at:-2]
    ffs = np.flatnonzero(body[:-1] == 0xFF) if body.size else np.zeros(0, np.int64)
    assert body.size and body[-1] != 0xFF, "a 0xFF at the end of the scan"
    follow = body[ffs + 1]
    assert np.isin(follow, [0x00] + list(range(0xD0, 0xD8))).all(), "an unstuffed 0xFF (or a foreign marker) in the scan"
    rst = follow[follow != 0]
    assert (rst == 0xD0 + (np.arange(rst.size) & 7)).all(), "RST numbers do not cycle 0 .. 7"
    mcu = 16 if info["sampling"][0] == 0x22 else 8
    mcus = -(-info["H"] // mcu) * -(-info["W"] // mcu)
    info["intervals"] = rst.size + 1
    if info["dri"]:
        assert info["intervals"] == -(-mcus // info["dri"]), "the number of RST markers does not match DRI"
    else:
        assert rst.size == 0, "RST markers without DRI"
    info["subsampling"] = "4:2:0" if info["sampling"][0] == 0x22 else "4:4:4"
    return info


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


# ---- the RIFF parser, from the statement of the container ----
def parse_avi(data):
    """RIFF 'AVI ' { LIST hdrl { avih(56), LIST strl { strh(56), strf(40) } }, LIST movi { 00dc ... }, idx1 } -> dict with the frames."""
    u32 = lambda at: struct.unpack("<I", data[at:at + 4])[0]
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and u32(4) == len(data) - 8, "RIFF header"
    at = 12
    assert data[at:at + 4] == b"LIST" and data[at + 8:at + 12] == b"hdrl"
    hdrl_end = at + 8 + u32(at + 4)
    at += 12
    assert data[at:at + 4] == b"avih" and u32(at + 4) == 56
    (us_per_frame, _, _, flags, frames, _, streams, _, width, height) = struct.unpack("<10I", data[at + 8:at + 48])
    assert streams == 1 and flags & 0x10, "one stream, AVIF_HASINDEX"
    at += 8 + 56
    assert data[at:at + 4] == b"LIST" and data[at + 8:at + 12] == b"strl" and at + 8 + u32(at + 4) == hdrl_end
    at += 12
    assert data[at:at + 4] == b"strh" and u32(at + 4) == 56 and data[at + 8:at + 16] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack("<4I", data[at + 28:at + 44])
    assert length == frames
    at += 8 + 56
    assert data[at:at + 4] == b"strf" and u32(at + 4) == 40
    bi_size, bi_w, bi_h, bi_planes, bi_bits = struct.unpack("<IiiHH", data[at + 8:at + 24])
    assert bi_size == 40 and (bi_w, bi_h) == (width, height) and bi_planes == 1 and bi_bits == 24 and data[at + 24:at + 28] == b"MJPG"
    at += 8 + 40
    assert at == hdrl_end
    assert data[at:at + 4] == b"LIST" and data[at + 8:at + 12] == b"movi"
    movi, movi_end = at + 8, at + 8 + u32(at + 4)
    at += 12
    chunks = []
    while at < movi_end:
        assert data[at:at + 4] == b"00dc"
        n = u32(at + 4)
        chunks.append((at - movi, n))
        at += 8 + n + (n & 1)
        assert at <= movi_end and (n & 1 == 0 or data[at - 1] == 0), "chunks are padded to even length with a zero"
    assert at == movi_end and len(chunks) == frames
    assert data[at:at + 4] == b"idx1" and u32(at + 4) == 16 * frames and at + 8 + 16 * frames == len(data), "idx1 closes the file"
    index = [struct.unpack("<4sIII", data[at + 8 + 16 * i:at + 24 + 16 * i]) for i in range(frames)]
    assert index == [(b"00dc", 0x10, off, n) for off, n in chunks], "idx1 entries point at the 00dc chunks, AVIIF_KEYFRAME"
    return dict(frames=[data[movi + off + 8:movi + off + 8 + n] for off, n in chunks], width=width, height=height, scale=scale, rate=rate,
                us_per_frame=us_per_frame, fps=rate / scale)
