"""The baseline JPEG decoding rules of include/gsraster_jpeg_decode.h stated in numpy -- marker walk, restart intervals, Huffman,
dequantisation, libjpeg's islow IDCT, fancy upsampling, colour -- and the corpus the decoders are held against.  Nothing here imports
the package's decoder: gscream_amd/jpeg_decode.py, jpeg_entropy.h and jpeg_decode.hip are all held against `decode` and against PIL.

decode(data)                  the file's bytes -> uint8 [H, W, C]; raises Corrupt(code) with the status code of the rules
status(data)                  -> the status code alone (0 = OK)
coefficients(data)            -> int16 [blocks, 64]: natural order, blocks in scan order (what the entropy kernel writes)
corpus()                      -> tuple of Case(name, data, image): image is PIL's decode, every file opened without a warning
corrupt()                     -> tuple of Case(name, data, None) whose status under these rules is not 0
"""
import collections
import functools
import io
import struct
import warnings
import zlib

import numpy as np
from PIL import Image

from tests import jpeg_helpers as JH

OK, TRUNCATED, BAD_CODE, BAD_SYMBOL, OVERRUN, RESTART, TABLE = range(7)
STATUS_NAMES = ("OK", "TRUNCATED", "BAD_CODE", "BAD_SYMBOL", "OVERRUN", "RESTART", "TABLE")
SIZES = ((1, 1), (8, 8), (15, 1), (15, 2), (9, 3), (18, 4), (7, 5), (19, 6), (2, 7), (3, 33), (17, 23), (33, 16), (48, 48))  # H, W
QUALITIES = (10, 50, 95, 100)
ZIGZAG = np.array(JH.ZIGZAG)  # natural index of zigzag position k

Case = collections.namedtuple("Case", "name data image")


class Corrupt(Exception):
    def __init__(self, code):
        super().__init__(STATUS_NAMES[code])
        self.code = code


# ---- the container, up to SOS ----
def header(data):
    """-> dict(H, W, C, hs, vs, quant [C][64] natural, dc / ac [C] (bits, values), dri, scan = offset of the entropy-coded bytes)."""
    assert data[:2] == b"\xff\xd8"
    at, qt, ht, dri, sof = 2, {}, {}, 0, None
    while True:
        assert data[at] == 0xFF
        marker = data[at + 1]
        if marker == 0xFF:
            at += 1
            continue
        n = struct.unpack(">H", data[at + 2:at + 4])[0]
        p = data[at + 4:at + 2 + n]
        if marker == 0xDB:
            while p:
                assert p[0] >> 4 == 0
                qt[p[0] & 15] = np.array(list(p[1:65]), np.int64)
                p = p[65:]
        elif marker == 0xC4:
            while p:
                bits = list(p[1:17])
                ht[p[0]] = (bits, list(p[17:17 + sum(bits)]))
                p = p[17 + sum(bits):]
        elif marker == 0xDD:
            dri = struct.unpack(">H", p)[0]
        elif marker == 0xC0:
            assert p[0] == 8
            sof = p
        elif marker == 0xDA:
            H, W, C = struct.unpack(">HH", sof[1:5]) + (sof[5],)
            comps = [(sof[6 + 3 * c], sof[7 + 3 * c], sof[8 + 3 * c]) for c in range(C)]
            assert p[0] == C and bytes(p[-3:]) == bytes([0, 63, 0]) and [p[1 + 2 * c] for c in range(C)] == [c[0] for c in comps]
            assert all(c[1] == 0x11 for c in comps[1:])
            quant = []
            for c in range(C):
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = qt[comps[c][2]]
                quant.append(q)
            return dict(H=H, W=W, C=C, hs=comps[0][1] >> 4, vs=comps[0][1] & 15, quant=quant, dc=[ht[p[2 + 2 * c] >> 4] for c in range(C)],
                        ac=[ht[0x10 | (p[2 + 2 * c] & 15)] for c in range(C)], dri=dri, scan=at + 2 + n)
        else:
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE, hex(marker)
        at += 2 + n


def geometry(h):
    mcux, mcuy = -(-h["W"] // (8 * h["hs"])), -(-h["H"] // (8 * h["vs"]))
    ny = h["hs"] * h["vs"]
    mcus = mcux * mcuy
    return dict(mcux=mcux, mcuy=mcuy, mcus=mcus, ny=ny, bpm=ny + h["C"] - 1, intervals=-(-mcus // h["dri"]) if h["dri"] else 1)


# ---- rule 2: the markers of the scan ----
def intervals(scan, expected):
    """The scan's bytes (everything behind SOS) -> [(start, end)] of the restart intervals.  A marker is an FF followed by a byte
    that is neither 00 nor FF.  The first marker that is not RSTm closes the scan; what lies behind it is not looked at."""
    b = np.frombuffer(scan, np.uint8)
    at = np.flatnonzero((b[:-1] == 0xFF) & (b[1:] != 0) & (b[1:] != 0xFF)) if b.size > 1 else np.zeros(0, np.int64)
    rst = (b[at + 1] & 0xF8) == 0xD0
    closing = np.flatnonzero(~rst)
    if closing.size == 0:
        raise Corrupt(TRUNCATED)
    end = int(at[closing[0]])
    at = at[:closing[0]]
    if at.size != expected - 1 or (b[at + 1] != 0xD0 + (np.arange(at.size) & 7)).any():
        raise Corrupt(RESTART)
    starts = [0] + [int(a) + 2 for a in at]
    ends = [int(a) for a in at] + [end]
    return list(zip(starts, ends))


# ---- rule 1: entropy ----
def _code_table(table):
    """(bits, values) -> (mincode[17], maxcode[17], first[17]); maxcode -1 where a length has no code."""
    bits, values = table
    mincode, maxcode, first = [0] * 17, [-1] * 17, [0] * 17
    code = at = 0
    for n in range(1, 17):
        first[n], mincode[n] = at, code
        if bits[n - 1]:
            maxcode[n] = code + bits[n - 1] - 1
        code = (code + bits[n - 1]) << 1
        at += bits[n - 1]
    return mincode, maxcode, first, values


class _Bits:
    def __init__(self, seg, ended_by_rst):
        # unstuff: FF 00 is FF; an FF followed by anything else (a fill byte, the region's end) ends the data
        out = bytearray()
        i, n = 0, len(seg)
        while i < n:
            if seg[i] != 0xFF:
                out.append(seg[i])
                i += 1
            elif i + 1 < n and seg[i + 1] == 0:
                out.append(0xFF)
                i += 2
            else:
                break
        self.n = 8 * len(out)
        self.v = int.from_bytes(bytes(out) + b"\0\0\0\0", "big")
        self.total = self.n + 32
        self.p = 0
        self.short = RESTART if ended_by_rst else TRUNCATED

    def peek16(self):
        if self.p > self.n:
            raise Corrupt(self.short)
        return (self.v >> (self.total - self.p - 16)) & 0xFFFF

    def take(self, k):
        if k == 0:
            return 0
        if self.p + k > self.n:
            raise Corrupt(self.short)
        r = (self.v >> (self.total - self.p - k)) & ((1 << k) - 1)
        self.p += k
        return r

    def symbol(self, tab):
        mincode, maxcode, first, values = tab
        w = self.peek16()
        for n in range(1, 17):
            c = w >> (16 - n)
            if c <= maxcode[n]:
                if self.p + n > self.n:
                    raise Corrupt(self.short)
                self.p += n
                return values[first[n] + c - mincode[n]]
        if self.p + 16 > self.n:
            raise Corrupt(self.short)
        raise Corrupt(BAD_CODE)


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < 1 << (s - 1) else v


def coefficients(data, h=None):
    h = h or header(data)
    g = geometry(h)
    for t in h["dc"] + h["ac"]:
        bits, values = t
        code = 0
        for n in range(16):
            code = (code + bits[n]) << 1
            if code > 2 << (n + 1):
                raise Corrupt(TABLE)  # more codes of a length than the lengths before leave room for
    dct, act = [_code_table(t) for t in h["dc"]], [_code_table(t) for t in h["ac"]]
    scan = bytes(data[h["scan"]:])
    ivs = intervals(scan, g["intervals"])
    out = np.zeros((g["mcus"] * g["bpm"], 64), np.int64)
    per = h["dri"] or g["mcus"]
    for i, (start, end) in enumerate(ivs):
        r = _Bits(scan[start:end], i + 1 < len(ivs))
        pred = [0, 0, 0]
        for m in range(i * per, min((i + 1) * per, g["mcus"])):
            for j in range(g["bpm"]):
                c = 0 if j < g["ny"] else j - g["ny"] + 1
                s = r.symbol(dct[c])
                if s > 11:
                    raise Corrupt(BAD_SYMBOL)
                pred[c] += _extend(r.take(s), s)
                blk = out[m * g["bpm"] + j]
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    rs = r.symbol(act[c])
                    run, s = rs >> 4, rs & 15
                    if s > 10 or (s == 0 and run not in (0, 15)):
                        raise Corrupt(BAD_SYMBOL)
                    if s == 0 and run == 0:
                        break
                    k += run + (s == 0)  # the run of zeros; ZRL is sixteen of them and must leave room for a value
                    if k > 63:
                        raise Corrupt(OVERRUN)
                    if s:
                        blk[ZIGZAG[k]] = _extend(r.take(s), s)
                        k += 1
        if r.n - r.p >= 8:
            raise Corrupt(RESTART)  # the interval's data goes on behind its last MCU
    return out.astype(np.int16)


# ---- rules 3 .. 6 ----
def _idct1(x, axis):
    x = np.moveaxis(x, axis, -1).astype(np.int64)
    x0, x1, x2, x3, x4, x5, x6, x7 = [x[..., i] for i in range(8)]
    z1 = (x2 + x6) * 4433
    t2, t3 = z1 - x6 * 15137, z1 + x2 * 6270
    t0, t1 = (x0 + x4) << 13, (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = x7, x5, x3, x1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], -1)
    return np.moveaxis(out, -1, axis)


def idct(blocks):
    """[..., 8 rows, 8 columns] dequantised -> samples 0 .. 255"""
    ws = (_idct1(blocks, -2) + 1024) >> 11
    return np.clip(((_idct1(ws, -1) + (1 << 17)) >> 18) + 128, 0, 255)


def upsample(p, r, n, hs, vs):
    """the used r x n part of a chroma plane -> [vs r, hs n]"""
    p = p[:r, :n].astype(np.int64)
    if hs == 1:
        return p
    if n <= 2:
        return np.repeat(np.repeat(p, vs, 0), 2, 1)
    out = np.zeros((vs * r, 2 * n), np.int64)
    if vs == 2:
        up, dn = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
        for v, nb in ((0, up), (1, dn)):
            s = 3 * p + nb
            out[v::2, 0::2] = (3 * s + np.concatenate([s[:, :1], s[:, :-1]], 1) + 8) >> 4
            out[v::2, 1::2] = (3 * s + np.concatenate([s[:, 1:], s[:, -1:]], 1) + 7) >> 4
    else:
        out[:, 0::2] = (3 * p + np.concatenate([p[:, :1], p[:, :-1]], 1) + 1) >> 2
        out[:, 1::2] = (3 * p + np.concatenate([p[:, 1:], p[:, -1:]], 1) + 2) >> 2
        out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def decode(data):
    h = header(data)
    g = geometry(h)
    H, W, C, hs, vs = h["H"], h["W"], h["C"], h["hs"], h["vs"]
    coef = coefficients(data, h).astype(np.int64).reshape(g["mcuy"], g["mcux"], g["bpm"], 8, 8)

    def plane(blocks, q):
        s = idct(blocks * q.reshape(8, 8))
        return s.transpose(0, 2, 1, 3).reshape(s.shape[0] * 8, s.shape[1] * 8)
    Yb = coef[:, :, :g["ny"]].reshape(g["mcuy"], g["mcux"], vs, hs, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(g["mcuy"] * vs, g["mcux"] * hs, 8, 8)
    Y = plane(Yb, h["quant"][0])[:H, :W]
    if C == 1:
        return Y[..., None].astype(np.uint8)
    r, n = -(-H // vs), -(-W // hs)
    cb, cr = (upsample(plane(coef[:, :, g["ny"] + c], h["quant"][1 + c]), r, n, hs, vs)[:H, :W] - 128 for c in range(2))
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], -1), 0, 255).astype(np.uint8)


def status(data):
    try:
        coefficients(data)
        return OK
    except Corrupt as e:
        return e.code


def digest(coef):
    """what tools/jpeg_entropy_check prints: CRC-32 of the int16 coefficients, little-endian"""
    return zlib.crc32(np.ascontiguousarray(coef, "<i2").tobytes())


# ---- the corpus ----
def pil_decode(data):
    """PIL's picture, uint8 [H, W, C]; a warning (a premature end, extraneous bytes) is an error."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
    a = np.asarray(im)
    assert a.dtype == np.uint8 and im.mode in ("L", "RGB"), im.mode
    return np.array(a.reshape(a.shape[0], a.shape[1], -1))


def pil_encode(image, quality, subsampling, optimize=False, **restart):
    im = Image.fromarray(image[..., 0] if image.shape[2] == 1 else image)
    buf = io.BytesIO()
    if image.shape[2] == 1:
        im.save(buf, "JPEG", quality=quality, optimize=optimize, **restart)
    else:
        im.save(buf, "JPEG", quality=quality, subsampling=subsampling, optimize=optimize, **restart)
    return buf.getvalue()


RESTARTS = (("", {}), ("-rb1", {"restart_marker_blocks": 1}), ("-rr1", {"restart_marker_rows": 1}))


@functools.lru_cache(maxsize=None)
def corpus():
    """Every size x kind x writer.  PIL: quality x (grey, 4:4:4, 4:2:2, 4:2:0) x optimize x (no markers, one per MCU, one per MCU
    row).  tests/jpeg_helpers.encode: (grey, 4:4:4, 4:2:0) x ri None, 0, 1."""
    cases = []
    for H, W in SIZES:
        for kind in JH.KINDS:
            rgb, grey = JH.picture(kind, H, W, 3, seed=H + W), JH.picture(kind, H, W, 1, seed=H + W)
            for q in QUALITIES:
                for sub in (None, 0, 1, 2):
                    for opt in (False, True):
                        for tag, restart in RESTARTS:
                            data = pil_encode(grey if sub is None else rgb, q, sub, opt, **restart)
                            cases.append((f"pil-{H}x{W}-{kind}-q{q}-{'grey' if sub is None else 's%d' % sub}{'-opt' if opt else ''}{tag}", data))
            for sub in (None, "4:4:4", "4:2:0"):
                for ri in (None, 0, 1):
                    data = JH.encode(grey if sub is None else rgb, 95, sub or "4:4:4", ri)
                    cases.append((f"own-{H}x{W}-{kind}-{sub or 'grey'}-ri{ri}", data))
    out = tuple(Case(name, data, pil_decode(data)) for name, data in cases)
    assert len(out) == len(SIZES) * len(JH.KINDS) * (len(QUALITIES) * 4 * 2 * 3 + 9)
    return out


def mixed_batches(cases, size=256):
    """The corpus in batches whose files differ in size, sampling and writer: a stride walk, so neighbours in the corpus part."""
    n = len(cases)
    stride = 389  # a prime that does not divide the corpus size
    assert n % stride
    order = [(i * stride) % n for i in range(n)]
    assert len(set(order)) == n
    return [[cases[i] for i in order[at:at + size]] for at in range(0, n, size)]


def _rst_positions(data, h):
    scan = np.frombuffer(data, np.uint8)[h["scan"]:]
    at = np.flatnonzero((scan[:-1] == 0xFF) & ((scan[1:] & 0xF8) == 0xD0))
    return [int(a) + h["scan"] for a in at]


@functools.lru_cache(maxsize=None)
def corrupt():
    """Truncations at every byte of a small file's scan, the single-bit flips of it that these rules can tell (a flipped value bit
    is another picture, not an error: the flips whose status under `status` is 0 are left out, and counted), a removed, a duplicated
    and a renumbered RST marker.  Each with and without restart markers."""
    cases = []
    rgb = JH.picture("texture", 17, 23, 3, seed=5)
    for tag, data in (("dri", JH.encode(rgb, 50, "4:2:0", 1)), ("plain", pil_encode(rgb, 50, 2)), ("opt", pil_encode(rgb, 75, 1, True, restart_marker_blocks=2))):
        h = header(data)
        assert status(data) == OK
        for cut in range(h["scan"], len(data)):
            cases.append(Case(f"{tag}-cut{cut}", data[:cut], None))
        told = 0
        for byte in range(h["scan"], len(data) - 2):  # one flip per byte of the scan, the bit walking with the byte
            bit = (byte * 3) & 7
            bad = bytearray(data)
            bad[byte] ^= 1 << bit
            if status(bytes(bad)) != OK:
                told += 1
                cases.append(Case(f"{tag}-flip{byte}.{bit}", bytes(bad), None))
        assert 5 * told > len(data) - 2 - h["scan"], "a fifth of the flips at least break a code"
        rst = _rst_positions(data, h)
        if rst:
            k = rst[len(rst) // 2]
            cases.append(Case(f"{tag}-rst-removed", data[:k] + data[k + 2:], None))
            cases.append(Case(f"{tag}-rst-duplicated", data[:k] + data[k:k + 2] + data[k:], None))
            bad = bytearray(data)
            bad[k + 1] = 0xD0 + ((bad[k + 1] + 1) & 7)
            cases.append(Case(f"{tag}-rst-renumbered", bytes(bad), None))
    out = tuple(cases)
    for c in out:
        assert status(c.data) != OK, c.name
    return out
