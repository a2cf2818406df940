"""The rules of include/gsraster_jpeg_split.h stated in numpy / Python from the Huffman statement of tests/jpeg_decode_helpers.py:
where the subsequences begin (rule 1, with the FF shift), the entry states read off the serial decode (rules 2 and 3), the block
counts and first_block (rule 4), the DC prefix (rule 5) -- and the small corpus the split decoders are held against.  Nothing here
imports the package's decoder.

beginnings(seg, B)            the interval's bytes -> the byte offsets at which its subsequences begin (none empty)
serial(data)                  -> per interval an Interval: the serial decoder's state in front of every unit, its final state, the
                              coefficients with the DC DIFFERENCES in place of the DC values (what the write pass stores)
model(data, B, min_bytes=0)   -> Model(rows, info): rows = per split interval, per subsequence (bit, j, k, first_block, blocks) -- the
                              trace the device must give, exactly; info = (intervals split, 0 repaired, subsequences, chunks)
run(iv, state, limit, ...)    one decoder from a state through the units that begin in front of bit `limit`
dc_prefix(diff, ny, bpm)      rule 5
corpus()                      the small corpus of the GPU tests: Case(name, data, image) with PIL's picture
"""
import collections
import functools

import numpy as np

from tests import jpeg_decode_helpers as DH
from tests import jpeg_helpers as JH

CHUNK = 256  # subsequences per chunk on the device (jpeg_split.hip JS_CHUNK)
SIZES = ((8, 8), (16, 16), (17, 23), (48, 48), (64, 40))  # H, W

Interval = collections.namedtuple("Interval", "seg ended_by_rst states final diff nblocks dct act ny bpm")
Model = collections.namedtuple("Model", "rows info")


def beginnings(seg, B):
    """Rule 1.  Subsequence i nominally begins at i B; behind an FF that byte is the stuffed 00 and it begins one byte later; a last
    one that would begin at the end does not exist."""
    n = len(seg)
    out = [0]
    for i in range(1, -(-n // B)):
        at = i * B
        if seg[at - 1] == 0xFF:
            at += 1
        if at < n:
            out.append(at)
    return out


def destuffed_bit(seg, byte):
    """the position, in the de-stuffed bit stream, of the first bit of byte `byte` (not the 00 of a pair)"""
    return 8 * (byte - bytes(seg[:byte]).count(b"\xff"))


def run(iv, state, limit, block, sink=None, states=None):
    """A decoder in `state` = (bit, j, k) goes through the units whose first bit lies in front of `limit` (None: to the interval's last
    block).  block: the number of the block the next DC unit begins.  sink(block, zigzag position, value) gets DC differences and AC
    values; states, when given, collects the state in front of every unit.  -> (exit state, blocks begun)"""
    r = DH._Bits(iv.seg, iv.ended_by_rst)
    r.p, j, k = state
    begun = 0
    while (limit is None or r.p < limit) and not (k == 0 and block + begun >= iv.nblocks):
        if states is not None:
            states.append((r.p, j, k))
        c = 0 if j < iv.ny else j - iv.ny + 1
        if k == 0:
            s = r.symbol(iv.dct[c])
            assert s <= 11
            v = DH._extend(r.take(s), s)
            if sink:
                sink(block + begun, 0, v)
            begun += 1
            k = 1
        else:
            rs = r.symbol(iv.act[c])
            zeros, s = rs >> 4, rs & 15
            assert s <= 10 and (s or zeros in (0, 15))
            if rs == 0:
                k = 64
            else:
                k += zeros + (s == 0)
                assert k <= 63
                if s:
                    v = DH._extend(r.take(s), s)
                    if sink:
                        sink(block + begun - 1, k, v)
                    k += 1
        if k == 64:
            j, k = (j + 1) % iv.bpm, 0
    return (r.p, j, k), begun


def serial(data):
    """The serial decoder over a valid file -> [Interval]."""
    h = DH.header(data)
    g = DH.geometry(h)
    dct, act = [DH._code_table(t) for t in h["dc"]], [DH._code_table(t) for t in h["ac"]]
    scan = bytes(data[h["scan"]:])
    ivs = DH.intervals(scan, g["intervals"])
    per = h["dri"] or g["mcus"]
    out = []
    for i, (start, end) in enumerate(ivs):
        nblocks = (min((i + 1) * per, g["mcus"]) - i * per) * g["bpm"]
        iv = Interval(scan[start:end], i + 1 < len(ivs), [], None, np.zeros((nblocks, 64), np.int64), nblocks, dct, act, g["ny"], g["bpm"])

        def sink(b, k, v, diff=iv.diff):
            diff[b, DH.ZIGZAG[k]] = v
        final, begun = run(iv, (0, 0, 0), None, 0, sink, iv.states)
        assert begun == nblocks and final[1:] == (0, 0)
        out.append(iv._replace(final=final))
    return out


def entry_rows(iv, B):
    """Rules 3 and 4 for one interval: per subsequence (bit, j, k, first_block, blocks)."""
    begins = [destuffed_bit(iv.seg, b) for b in beginnings(iv.seg, B)]
    bits = np.array([s[0] for s in iv.states])
    dc = np.array([s[2] == 0 for s in iv.states])
    rows, first = [], 0
    for i, at in enumerate(begins):
        lo = int(np.searchsorted(bits, at, "left"))  # the first unit whose first bit lies at or beyond the beginning
        hi = int(np.searchsorted(bits, begins[i + 1], "left")) if i + 1 < len(begins) else len(bits)
        state = iv.states[lo] if lo < len(bits) else iv.final
        blocks = int(dc[lo:hi].sum())
        rows.append(state + (first, blocks))
        first += blocks
    assert first == iv.nblocks and rows[0][:3] == (0, 0, 0)
    return rows, begins


def segments(data):
    """the bytes of the file's intervals (rule 2 of gsraster_jpeg_decode.h), without decoding them"""
    h = DH.header(data)
    scan = bytes(data[h["scan"]:])
    return [scan[start:end] for start, end in DH.intervals(scan, DH.geometry(h)["intervals"])]


@functools.lru_cache(maxsize=None)
def model(data, B, min_bytes=0):
    rows, split, subs, chunks = [], 0, 0, 0
    for iv in serial(data):
        if len(iv.seg) < min_bytes or len(beginnings(iv.seg, B)) < 2:
            continue
        r, _ = entry_rows(iv, B)
        rows.append(r)
        split += 1
        subs += len(r)
        chunks += -(-len(r) // CHUNK)
    return Model(rows, (split, 0, subs, chunks))


def dc_prefix(diff, ny, bpm):
    """Rule 5: per component the running sum of the DC differences over the blocks in scan order, wrapping at 16 bits."""
    out = diff.copy()
    comp = np.array([0 if j < ny else j - ny + 1 for j in range(bpm)])[np.arange(diff.shape[0]) % bpm]
    for c in range(3):
        out[comp == c, 0] = np.cumsum(diff[comp == c, 0])
    out[:, 0] = ((out[:, 0] + 32768) % 65536) - 32768
    return out


# ---- the corpus ----
def _files():
    for H, W in SIZES:
        for kind, q in (("ramp", 75), ("noise", 100)):  # mostly EOB, a subsequence holds many blocks / a block spans several subsequences
            rgb, grey = JH.picture(kind, H, W, 3, seed=H + W), JH.picture(kind, H, W, 1, seed=H + W)
            for sub in (None, 0, 1, 2):
                for opt in (False, True):
                    for tag, restart in (("", {}), ("-rr1", {"restart_marker_rows": 1})):
                        yield (f"pil-{H}x{W}-{kind}-q{q}-{'grey' if sub is None else 's%d' % sub}{'-opt' if opt else ''}{tag}",
                               DH.pil_encode(grey if sub is None else rgb, q, sub, opt, **restart))
            for sub in (None, "4:4:4", "4:2:0"):  # (all that tests/jpeg_helpers.encode writes: it has no 4:2:2; PIL's writer above covers it)
                yield f"own-{H}x{W}-{kind}-{sub or 'grey'}-riNone", JH.encode(grey if sub is None else rgb, q, sub or "4:4:4", None)


@functools.lru_cache(maxsize=None)
def corpus():
    out = tuple(DH.Case(name, data, DH.pil_decode(data)) for name, data in _files())
    assert len(out) == len(SIZES) * 2 * (4 * 2 * 2 + 3)
    return out


def on_a_stuffed_zero(data, B):
    """True: in some interval of the file a nominal subsequence beginning i B falls on the 00 of an FF 00 pair (rule 1's shift)."""
    for seg in segments(data):
        if any(seg[at - 1] == 0xFF and seg[at] == 0 for at in range(B, len(seg), B)):
            return True
    return False


@functools.lru_cache(maxsize=None)
def shifted_case(B=16):
    """A file of the corpus with the hand-checked property: a nominal beginning on the 00 of a pair."""
    for case in corpus():
        if "noise-q100" in case.name and on_a_stuffed_zero(case.data, B):
            return case
    raise AssertionError("no file of the corpus has a nominal beginning on a stuffed 00")


def mixed_batches(cases, size=48):
    """Batches whose files differ in size, sampling and writer: a stride walk."""
    n, stride = len(cases), 37
    assert n % stride
    order = [(i * stride) % n for i in range(n)]
    assert len(set(order)) == n
    return [[cases[i] for i in order[at:at + size]] for at in range(0, n, size)]
