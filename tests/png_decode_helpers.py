"""The corpus of the PNG decoder's tests (tests/test_png_decode.py on the CPU, tests/test_gpu_png_decode.py on the device), generated
at test time with zlib, PIL and a few lines of bit packing.  A case is (name, the file's bytes, the picture it holds or None, the
status code it must end in).  Every comparison the tests make is equality of bytes."""
import functools
import io
import struct
import zlib
from typing import NamedTuple, Optional

import numpy as np

from tests import png_helpers as PH
from gscream_amd import synthetic as S

# GSR_PNG_* of include/gsraster.h
(OK, TRUNCATED, BLOCK_TYPE, STORED_LEN, BAD_CODE, BAD_SYMBOL, DISTANCE, TOO_LONG, TOO_SHORT, FILTER, ADLER, CRC, TABLE) = range(13)
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
KINDS = ("texture", "mask", "noise", "colormap")
COMPRESSORS = {
    "level0": (0, zlib.Z_DEFAULT_STRATEGY), "level1": (1, zlib.Z_DEFAULT_STRATEGY), "level9": (9, zlib.Z_DEFAULT_STRATEGY),
    "fixed": (6, zlib.Z_FIXED), "huffman": (6, zlib.Z_HUFFMAN_ONLY), "rle": (6, zlib.Z_RLE),
}
LAYOUTS = {"whole": None, "seven": 7, "one": 1}
THREE_CHUNKS = (96, 250, 3)


class Case(NamedTuple):
    name: str
    data: bytes
    image: Optional[np.ndarray]
    status: int


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def container(H, W, C, idats, extra=()):
    """signature, IHDR, the `extra` ancillary chunks, the IDATs, IEND."""
    parts = [PH.SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, COLOUR_TYPE[C], 0, 0, 0))]
    parts += [chunk(k, b) for k, b in extra]
    parts += [chunk(b"IDAT", b) for b in idats]
    parts.append(chunk(b"IEND", b""))
    return b"".join(parts)


def idat_payload(data):
    """The concatenated IDAT payloads of a file, by a plain walk over its chunks."""
    at, out = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        if kind == b"IDAT":
            out.append(data[at + 8:at + 8 + n])
        at += 12 + n
    return b"".join(out)


def split(payload, piece):
    return [payload] if piece is None else [payload[i:i + piece] for i in range(0, len(payload), piece)]


def picture(kind, H, W, C, seed=0):
    """synthetic.picture, and for C = 2 a grey plus alpha pair of two of its planes."""
    if C != 2:
        return S.picture(kind, H, W, C, seed=seed)
    return np.ascontiguousarray(np.concatenate([S.picture(kind, H, W, 1, seed=seed), S.picture("texture", H, W, 1, seed=seed + 1)], -1))


def cycled_stream(image, first):
    """The filtered stream whose row y has filter type (first + y) mod 5."""
    H = image.shape[0]
    per_type = [PH.filter_rule(image, t) for t in range(5)]
    return np.stack([per_type[(first + y) % 5][y] for y in range(H)]).tobytes()


def compress(stream, compressor):
    level, strategy = COMPRESSORS[compressor]
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return co.compress(stream) + co.flush()


def pil_decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    a = np.asarray(im)
    return a.reshape(a.shape[0], a.shape[1], -1)


@functools.lru_cache(maxsize=None)
def _cross_source(kind, C, first):
    image = picture(kind, 45, 67, C, seed=C)
    image.setflags(write=False)
    return image, cycled_stream(image, first)


@functools.lru_cache(maxsize=None)
def cross(compressor, layout):
    """1: kinds x channels x the filter cycle's five starts, for one compressor and one IDAT layout."""
    cases = []
    for kind in KINDS:
        for C in (1, 2, 3, 4):
            for first in range(5):
                image, stream = _cross_source(kind, C, first)
                payload = compress(stream, compressor)
                extra = ((b"tEXt", b"Comment\x00corpus"),) if first == 0 else ()
                cases.append(Case(f"{compressor}-{layout}-{kind}-c{C}-f{first}", container(45, 67, C, split(payload, LAYOUTS[layout]), extra), image, OK))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def edge_shapes():
    """2: png_helpers.SHAPES, written by PIL and by the project's encoder (its host statement: the same container and cuts)."""
    import torch
    from PIL import Image
    from gscream_amd import png
    cases = []
    for H, W, C in PH.SHAPES:
        image = S.picture("texture", H, W, C, seed=H + W)
        buf = io.BytesIO()
        Image.fromarray(image[..., 0] if C == 1 else image).save(buf, "PNG")
        cases.append(Case(f"pil-{H}x{W}x{C}", buf.getvalue(), image, OK))
        was = png.force_torch
        png.force_torch = True
        try:
            (own,) = png.to_bytes(png.encode(torch.from_numpy(image)))
        finally:
            png.force_torch = was
        cases.append(Case(f"own-{H}x{W}x{C}", own, image, OK))
    return tuple(cases)


def fixed_code(w, sym):
    if sym < 144:
        w.put_code(0x30 + sym, 8)
    elif sym < 256:
        w.put_code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.put_code(sym - 256, 7)
    else:
        w.put_code(0xC0 + sym - 280, 8)


@functools.lru_cache(maxsize=None)
def never_emitted():
    """3: a hand-assembled fixed-Huffman stream: 32768 literals (values >= 144 among them), a match of 258 at distance 32768, one of
    258 at distance 1, one of 3 at distance 2, literals up to the end of a 3-row grey picture.  zlib.decompress is the referee."""
    H, row = 3, 11096  # 3 * 11096 = 33288 = 32768 + 258 + 258 + 3 + 1
    W = row - 1
    rng = np.random.default_rng(5)
    lits = rng.integers(0, 256, 32768, dtype=np.uint8)
    assert (lits >= 144).any() and (lits < 144).any()
    lits[[0, row, 2 * row]] = 0  # the filter bytes
    w = PH.BitWriter()
    w.put(1 | 1 << 1, 3)  # BFINAL, fixed
    for v in lits.tolist():
        fixed_code(w, v)
    for length_sym, dist_sym, extra_bits, extra in ((285, 29, 13, 32768 - 24577), (285, 0, 0, 0), (257, 1, 0, 0)):
        fixed_code(w, length_sym)
        w.put_code(dist_sym, 5)
        if extra_bits:
            w.put(extra, extra_bits)
    fixed_code(w, 77)
    fixed_code(w, 256)
    raw = w.bytes()
    stream = zlib.decompress(raw, -15)
    assert len(stream) == H * row and stream[0] == stream[row] == stream[2 * row] == 0
    payload = b"\x78\x01" + raw + struct.pack(">I", zlib.adler32(stream))
    image = np.frombuffer(stream, np.uint8).reshape(H, row)[:, 1:].reshape(H, W, 1).copy()
    return (Case("never-emitted", container(H, W, 1, [payload]), image, OK),)


def own_pictures():
    """4: what png.encode is given: all five kinds at 96 x 250 x 3 (three chunks, cuts inside rows)."""
    H, W, C = THREE_CHUNKS
    return [S.picture(kind, H, W, C, seed=3) for kind in ("texture", "colormap", "mask", "constant", "noise")]


@functools.lru_cache(maxsize=None)
def flushed(mode):
    """5: one stream at zlib level 9, an IDAT per 5000 bytes of it, each closed with Z_FULL_FLUSH (every segment stands alone) or
    Z_SYNC_FLUSH (matches reach across the cuts)."""
    H, W, C = THREE_CHUNKS
    image = S.picture("texture", H, W, C, seed=8)
    stream = PH.filter_rule(image).tobytes()
    co = zlib.compressobj(9)
    idats = []
    cuts = list(range(0, len(stream), 5000))
    for k, at in enumerate(cuts):
        last = k == len(cuts) - 1
        idats.append(co.compress(stream[at:at + 5000]) + co.flush(zlib.Z_FINISH if last else {"full": zlib.Z_FULL_FLUSH, "sync": zlib.Z_SYNC_FLUSH}[mode]))
    assert len(idats) == 15 and all(b.endswith(b"\x00\x00\xff\xff") for b in idats[:-1])
    return (Case(f"flush-{mode}", container(H, W, C, idats), image, OK),)


def _zlib(raw, stream=b""):
    return b"\x78\x01" + raw + struct.pack(">I", zlib.adler32(stream))


@functools.lru_cache(maxsize=None)
def corrupt():
    """7: every status code but OK, each from a file that is a well-formed container around a defective zlib stream."""
    H, W, C = 5, 7, 3
    image = S.picture("texture", H, W, C, seed=2)
    stream = PH.filter_rule(image).tobytes()
    row = 1 + W * C
    good = zlib.compress(stream, 9)
    cases = []

    def add(name, payload, status, idats=None):
        cases.append(Case("corrupt-" + name, container(H, W, C, idats if idats is not None else [payload]), None, status))
    add("truncated", None, TRUNCATED, [good[:10], good[10:-9]])
    add("adler", good[:-1] + bytes([good[-1] ^ 1]), ADLER)
    flipped = bytearray(container(H, W, C, [good]))
    flipped[-12 - 4] ^= 0x40  # the last byte of the IDAT's CRC (IEND is the 12 bytes behind it)
    cases.append(Case("corrupt-crc", bytes(flipped), image, CRC))
    w = PH.BitWriter()
    w.put(1 | 1 << 1, 3)
    fixed_code(w, 0)
    fixed_code(w, 257)   # length 3 ...
    w.put_code(1, 5)     # ... at distance 2, one byte into the stream
    fixed_code(w, 256)
    add("distance", _zlib(w.bytes()), DISTANCE)
    w = PH.BitWriter()
    w.put(1 | 2 << 1, 3)
    w.put(0, 5)
    w.put(0, 5)
    w.put(0, 4)          # HCLEN = 4: the lengths of 16, 17, 18, 0 ...
    for _ in range(4):
        w.put(1, 3)      # ... are all 1: four codes of one bit
    w.put(0, 16)
    add("oversubscribed", _zlib(w.bytes()), BAD_CODE)
    add("blocktype", _zlib(bytes([0x07, 0, 0, 0])), BLOCK_TYPE)
    add("storedlen", _zlib(bytes([0x01, 5, 0, 0, 0, 1, 2, 3, 4, 5])), STORED_LEN)
    longer = stream + stream[-row:]
    add("toolong", zlib.compress(longer, 9), TOO_LONG)
    add("tooshort", zlib.compress(stream[:-row], 9), TOO_SHORT)
    bad = bytearray(stream)
    bad[2 * row] = 5
    add("filter", zlib.compress(bytes(bad), 9), FILTER)
    return tuple(cases)


def mixed_sizes():
    """6: 1x1x1, 37x53x4 and 96x250x3 for one call."""
    cases = []
    for (H, W, C), compressor in (((1, 1, 1), "level9"), ((37, 53, 4), "level1"), (THREE_CHUNKS, "level9")):
        image = S.picture("texture", H, W, C, seed=H)
        cases.append(Case(f"mixed-{H}x{W}x{C}", container(H, W, C, [compress(PH.filter_rule(image).tobytes(), compressor)]), image, OK))
    return cases


def rejected():
    """10: files outside the accepted subset -> (name, bytes, a word of the reason)."""
    from PIL import Image
    out = []
    a = S.picture("texture", 9, 11, 3, seed=1)

    def pil(im):
        buf = io.BytesIO()
        im.save(buf, "PNG")
        return buf.getvalue()
    out.append(("16-bit", pil(Image.fromarray((a[..., 0].astype(np.uint16) * 257))), "bit depth"))
    out.append(("palette", pil(Image.fromarray(a).convert("P")), "palette"))
    out.append(("1-bit", pil(Image.fromarray(a[..., 0] > 100)), "bit depth"))
    good = bytearray(pil(Image.fromarray(a)))
    adam = bytearray(good)
    adam[8 + 8 + 12] = 1
    adam[8 + 8 + 13:8 + 8 + 17] = struct.pack(">I", zlib.crc32(bytes(adam[12:29])))
    out.append(("adam7", bytes(adam), "Adam7"))
    out.append(("signature", b"\x89PNX" + bytes(good[4:]), "signature"))
    out.append(("no-idat", PH.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 11, 9, 8, 2, 0, 0, 0)) + chunk(b"IEND", b""), "IDAT"))
    out.append(("no-iend", bytes(good[:-12]), "IEND"))
    out.append(("zlib-header", container(9, 11, 3, [b"\x78\x20" + zlib.compress(b"x")[2:]]), "zlib header"))
    return out


def digest(image):
    """CRC-32 of the picture's bytes, as tools/png_inflate_check.cpp prints it."""
    return zlib.crc32(image.tobytes())
