"""What the PNG tests share (tests/test_png.py on the CPU, tests/test_gpu_png.py on the device): the decoders of record, a chunk parser, the
zlib Z_RLE size model, and a Python statement of the rules of include/gsraster.h ("PNG encoding") that yields the file byte for byte.

Decoders of record: PIL opens the file and gives the exact pixels, mode and size; zlib inflates the concatenated IDAT payloads (which
rejects incomplete or over-subscribed codes and a wrong Adler-32) to H (1 + W C) bytes with nothing left over; the parser checks the
chunk order, every CRC, the IHDR fields and that nothing follows IEND; the filter bytes of the inflated stream equal the numpy rule."""
import heapq
import io
import struct
import zlib

import numpy as np

CHUNK = 32768
HEADER = 16
ADAPTIVE = 5
SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}
MODE = {1: "L", 3: "RGB", 4: "RGBA"}


def capacity(H, W, C):
    stream = H * (1 + W * C)
    return 8 + 25 + -(-stream // CHUNK) * (12 + 5 + 5) + stream + 2 + 4 + 12


# ---- the filter rule ----
def filter_rule(image, filter=ADAPTIVE):
    """uint8 [H, W, C] -> the filtered stream uint8 [H, 1 + W C]: type 0 .. 4 in every row, or per row the type with the smallest sum
    of |signed residual|, ties to the lowest."""
    H, W, C = image.shape
    out = np.zeros((H, 1 + W * C), np.uint8)
    prev = np.zeros(W * C, np.int64)
    for y in range(H):
        cur = image[y].reshape(-1).astype(np.int64)
        a = np.concatenate([np.zeros(C, np.int64), cur[:-C]]) if W > 1 else np.zeros(W * C, np.int64)
        b = prev
        c = np.concatenate([np.zeros(C, np.int64), prev[:-C]]) if W > 1 else np.zeros(W * C, np.int64)
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        rows = [(cur - q) % 256 for q in (0 * cur, a, b, (a + b) // 2, paeth)]
        if filter == ADAPTIVE:
            sums = [int(np.where(r < 128, r, 256 - r).sum()) for r in rows]
            t = sums.index(min(sums))
        else:
            t = filter
        out[y, 0] = t
        out[y, 1:] = rows[t]
        prev = cur
    return out


# ---- the container ----
def parse(data):
    """-> (ihdr fields, [IDAT payloads]); asserts the order signature, IHDR, IDAT+, IEND, every CRC, and that nothing follows IEND."""
    assert data[:8] == SIGNATURE
    at, kinds, idat, ihdr = 8, [], [], None
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert len(body) == n, "a chunk runs past the end of the file"
        (crc,) = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + body), f"CRC of {kind} at {at}"
        kinds.append(kind)
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        if kind == b"IDAT":
            idat.append(body)
        at += 12 + n
        if kind == b"IEND":
            assert n == 0
            break
    assert at == len(data), "bytes behind IEND"
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and len(kinds) >= 3 and set(kinds[1:-1]) == {b"IDAT"}, kinds
    return ihdr, idat


def check_file(data, image, filter=ADAPTIVE, expect_chunks=True):
    """Every decoder of record on one file of the uint8 [H, W, C] picture; -> the inflated stream."""
    from PIL import Image
    H, W, C = image.shape
    assert len(data) <= capacity(H, W, C)
    ihdr, idat = parse(data)
    assert ihdr == (W, H, 8, COLOUR_TYPE[C], 0, 0, 0)
    stream_bytes = H * (1 + W * C)
    if expect_chunks:
        assert len(idat) in (-(-stream_bytes // CHUNK), -(-stream_bytes // CHUNK) + 1)  # (+ 1: an IDAT of its own for the Adler-32)
    payload = b"".join(idat)
    assert payload[:2] == b"\x78\x01"
    d = zlib.decompressobj()
    stream = d.decompress(payload)
    assert d.eof and d.unused_data == b"" and len(stream) == stream_bytes
    want = filter_rule(image, filter)
    got = np.frombuffer(stream, np.uint8).reshape(H, 1 + W * C)
    assert np.array_equal(got[:, 0], want[:, 0]), "filter bytes"
    assert np.array_equal(got, want)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == MODE[C] and im.size == (W, H)
    assert np.array_equal(np.asarray(im).reshape(H, W, C), image)
    return stream


# ---- the size reference: zlib's Z_RLE strategy on the same filtered bytes and the same cuts ----
def rle_model_size(image, filter=ADAPTIVE):
    stream = filter_rule(image, filter).tobytes()
    total = 8 + 25 + 12 + 2 + 4
    cuts = range(0, len(stream), CHUNK)
    for k, at in enumerate(cuts):
        last = k == len(cuts) - 1
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        n = len(co.compress(stream[at:at + CHUNK]) + co.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH))
        total += 12 + min(n, 5 + len(stream[at:at + CHUNK]) + (0 if last else 5))
    return total


# ---- the rules, byte for byte ----
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def length_symbol(n):
    """match length 3 .. 258 -> (symbol, extra bits, extra value) by the table of RFC 1951 3.2.5."""
    if n == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LENGTH_BASE[i] <= n)
    return 257 + k, LENGTH_EXTRA[k], n - LENGTH_BASE[k]


def tokens(chunk):
    """bytes -> [(symbol, extra bits, extra value, is_match)] by the greedy run rule."""
    arr = np.frombuffer(chunk, np.uint8)
    heads = np.concatenate([[0], np.flatnonzero(np.diff(arr.astype(np.int16))) + 1, [len(arr)]])
    out = []
    for s, e in zip(heads[:-1], heads[1:]):
        v = int(arr[s])
        out.append((v, 0, 0, False))
        rest = int(e - s - 1)
        while rest > 0:
            piece = min(rest, 258)
            if piece >= 3:
                out.append(length_symbol(piece) + (True,))
            else:
                out += [(v, 0, 0, False)] * piece
            rest -= piece
    return out


def limited_lengths(freq, limit):
    """counts per symbol -> code lengths by the rule: two-queue merge in ascending (count, symbol) order, a leaf before an internal node
    of the same weight; fold to the limit; repair the Kraft sum; lengths to the symbols longest first."""
    order = sorted((f, s) for s, f in enumerate(freq) if f)
    m = len(order)
    lens = [0] * len(freq)
    assert m >= 2
    nodes, lpar, npar, a, b = [], [0] * m, [0] * m, 0, 0
    for k in range(m - 1):
        total = 0
        for _ in range(2):
            if a < m and (b >= k or order[a][0] <= nodes[b]):
                total += order[a][0]
                lpar[a] = k
                a += 1
            else:
                total += nodes[b]
                npar[b] = k
                b += 1
        nodes.append(total)
    depth = [0] * (m - 1)
    for k in range(m - 3, -1, -1):
        depth[k] = depth[npar[k]] + 1
    count = [0] * (limit + 2)
    for i in range(m):
        count[min(depth[lpar[i]] + 1, limit)] += 1
    total = sum(count[l] << (limit - l) for l in range(1, limit + 1))
    while total != 1 << limit:
        count[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if count[l]:
                count[l] -= 1
                count[l + 1] += 2
                break
        total -= 1
    at = 0
    for l in range(limit, 0, -1):
        for _ in range(count[l]):
            lens[order[at][1]] = l
            at += 1
    return lens


def canonical(lens):
    """code lengths -> codes (RFC 1951 3.2.2), as integers whose most significant bit goes out first."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else 0)
        nxt[l] += 1 if l else 0
    return out


class BitWriter:
    def __init__(self, prefix=b""):
        self.values, self.widths, self.prefix = [], [], prefix

    def put(self, value, width):  # least significant bit first
        self.values.append(value)
        self.widths.append(width)

    def put_code(self, code, width):  # a Huffman code: most significant bit first
        self.put(int(format(code, f"0{width}b")[::-1], 2) if width else 0, width)

    def bits(self):
        return sum(self.widths)

    def bytes(self):
        v, w = np.array(self.values, np.int64), np.array(self.widths, np.int64)
        pos = np.concatenate([[0], np.cumsum(w)])
        bits = np.zeros(int(pos[-1]) + 7 & ~7, np.uint8)
        for k in range(int(w.max()) if len(w) else 0):
            sel = w > k
            bits[pos[:-1][sel] + k] = (v[sel] >> k) & 1
        return self.prefix + np.packbits(bits, bitorder="little").tobytes()


def deflate_chunk(chunk, last):
    """One chunk of the stream -> its deflate bytes by the rules (without the zlib header)."""
    toks = tokens(chunk)
    hist = [0] * 286
    for s, _, _, _ in toks:
        hist[s] += 1
    hist[256] = 1
    matches = sum(1 for t in toks if t[3])
    lens = limited_lengths(hist, 15)
    codes = canonical(lens)
    hlit = max([257] + [s + 1 for s in range(257, 286) if lens[s]])
    seq = lens[:hlit] + [1 if matches else 0]
    cl, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v:
            cl.append((v, 0, 0))
            r -= 1
        while r >= 3:
            take = min(r, 6 if v else 138)
            cl.append((16, 2, take - 3) if v else ((17, 3, take - 3) if take <= 10 else (18, 7, take - 11)))
            r -= take
        cl += [(v, 0, 0)] * r
    clhist = [0] * 19
    for s, _, _ in cl:
        clhist[s] += 1
    if sum(1 for f in clhist if f) == 1:
        only = next(s for s in range(19) if clhist[s])
        cllens = [0] * 19
        cllens[only] = cllens[1 if only == 0 else 0] = 1
    else:
        cllens = limited_lengths(clhist, 7)
    clcodes = canonical(cllens)
    hclen = max([4] + [i + 1 for i in range(4, 19) if cllens[CL_ORDER[i]]])
    w = BitWriter()
    w.put((1 if last else 0) | 2 << 1, 3)
    w.put(hlit - 257, 5)
    w.put(0, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cllens[CL_ORDER[i]], 3)
    for s, eb, ev in cl:
        w.put_code(clcodes[s], cllens[s])
        if eb:
            w.put(ev, eb)
    for s, eb, ev, is_match in toks:
        w.put_code(codes[s], lens[s])
        if eb:
            w.put(ev, eb)
        if is_match:
            w.put(0, 1)
    w.put_code(codes[256], lens[256])
    stored_bits = 3 + 5 + 32 + 8 * len(chunk)
    if w.bits() < stored_bits:
        if not last:
            w.put(0, 3)
        data = w.bytes()
    else:
        data = bytes([1 if last else 0]) + struct.pack("<HH", len(chunk), len(chunk) ^ 0xffff) + chunk + (b"" if last else b"\x00")
    return data + (b"" if last else b"\x00\x00\xff\xff")


def _png_chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def rules_file(image, filter=ADAPTIVE):
    """uint8 [H, W, C] -> the file the rules fix, byte for byte."""
    H, W, C = image.shape
    stream = filter_rule(image, filter).tobytes()
    parts = [SIGNATURE, _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOUR_TYPE[C], 0, 0, 0))]
    cuts = range(0, len(stream), CHUNK)
    for k, at in enumerate(cuts):
        last = k == len(cuts) - 1
        body = (b"\x78\x01" if k == 0 else b"") + deflate_chunk(stream[at:at + CHUNK], last)
        parts.append(_png_chunk(b"IDAT", body + (struct.pack(">I", zlib.adler32(stream)) if last else b"")))
    parts.append(_png_chunk(b"IEND", b""))
    return b"".join(parts)


def unlimited_depth(freq):
    """The depth of Huffman's tree without a length limit (heapq; ties by order of creation)."""
    heap = [(f, i, 0) for i, f in enumerate(freq) if f]
    heapq.heapify(heap)
    tick = len(freq)
    while len(heap) > 1:
        f1, _, d1 = heapq.heappop(heap)
        f2, _, d2 = heapq.heappop(heap)
        heapq.heappush(heap, (f1 + f2, tick, max(d1, d2) + 1))
        tick += 1
    return heap[0][2]


# ---- pictures ----
SHAPES = [(1, 1, 1), (5, 7, 3), (37, 53, 4), (1, 300, 3), (300, 1, 1)]


def ladder_picture():
    """[1, W, 1] whose byte counts follow a Fibonacci-like ladder with no byte equal to its neighbour, in one chunk: with filter 0 the
    literal histogram is the ladder (plus the filter byte and the end of block), and an unlimited Huffman tree is deeper than 15."""
    fib = [1, 1]  # the end of block and the filter byte are the ladder's first two rungs, the pixel values 1, 2, ... the others
    while sum(fib) + fib[-1] + fib[-2] < CHUNK:
        fib.append(fib[-1] + fib[-2])
    values = [v for v, f in sorted(enumerate(fib[2:], start=1), key=lambda t: -t[1]) for _ in range(f)]  # most frequent first
    n = len(values)
    row = np.zeros(n, np.uint8)
    row[0::2] = values[:(n + 1) // 2]  # the most frequent value fills less than every other place: no two neighbours are equal
    row[1::2] = values[(n + 1) // 2:]
    assert not (np.diff(row.astype(np.int16)) == 0).any() and n + 1 <= CHUNK
    hist = np.bincount(np.concatenate([row, [0]]), minlength=286)
    hist[256] = 1
    return row.reshape(1, n, 1), hist
