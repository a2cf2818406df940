// png_inflate.h -- the core of the PNG decoder, compiled for the device (png_decode.hip) and for the host (tools/png_inflate_check.cpp,
// which runs it under AddressSanitizer and UBSan over the test corpus, corrupt files included): the bit reader that hops from one IDAT
// payload to the next, the canonical decode tables, the symbol decoder, the block loop, and the unfilter rule.
//
// The code is written for a TEAM of lanes that execute it in lockstep with identical state (the device: the 64 lanes of a one-wave
// workgroup; the host: one lane).  Every value that steers control flow comes from the input bytes or from tables behind a
// team.sync(), so it is the same in every lane.  Only lane 0 stores to the shared tables; the table fill is strided over the lanes.
// The output goes to a SINK (lit / match / pos), which counts, writes a host buffer, or is the device's LDS ring.
//
// Safety rules, which hold for any input bytes and any tables:
//   reads    a piece is clamped to [0, nbytes) when the reader enters it; a byte is read only inside the clamped piece.
//   writes   the sink refuses a byte at or beyond its limit (PNGI_TOO_LONG); the shared tables are indexed by values masked or
//            range-checked right at the access.
//   distance checked against sink.pos, the bytes produced since the start of this decode.
//   loops    every iteration of the block loop consumes >= 3 bits, of the symbol loops >= 1 bit, of the stored copy 8 bits; a
//            consume beyond the available bits ends the decode with PNGI_TRUNCATED.  The decode terminates on any input.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PNGI_HD __host__ __device__ inline
#else
#define PNGI_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PNGI_SYNC() __syncthreads()
#else
#define PNGI_SYNC() ((void)0)
#endif
#define PNGI_WINDOW 4096  // bytes of input a team stages at a time
// A value that is the same in every lane, said so: on the device it moves to a scalar register, and what is computed from it -- the bit
// accumulator, the table index, the branch conditions -- runs on the scalar unit instead of once per lane.  Only ever applied where
// all lanes are active and hold the same value (see the head of this file).
#if defined(__HIP_DEVICE_COMPILE__)
#define PNGI_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define PNGI_UNIFORM(x) ((uint32_t)(x))
#endif
#define PNGI_UNIFORM64(x) ((uint64_t)PNGI_UNIFORM((uint32_t)(x)) | (uint64_t)PNGI_UNIFORM((uint32_t)((uint64_t)(x) >> 32)) << 32)

// status codes: GSR_PNG_* of include/gsraster.h
enum {
    PNGI_OK = 0, PNGI_TRUNCATED, PNGI_BLOCK_TYPE, PNGI_STORED_LEN, PNGI_BAD_CODE, PNGI_BAD_SYMBOL, PNGI_DISTANCE, PNGI_TOO_LONG,
    PNGI_TOO_SHORT, PNGI_FILTER, PNGI_ADLER, PNGI_CRC, PNGI_TABLE,
    PNGI_MISPLACED_FINAL = 64  // BFINAL in a segment that is not the last: only ever a flag of the measuring pass
};
#define PNGI_PIECE_IDAT 1u
// what a decode covers
#define PNGI_HEAD 1  // the zlib header leads
#define PNGI_TAIL 2  // runs to BFINAL, then the Adler-32; without it: runs until the data ends on a block boundary
#define PNGI_LIT_BITS 10
#define PNGI_CL_BITS 7
#define PNGI_ADLER_MOD 65521u

struct PngiPiece {  // = gsr_png_piece
    uint64_t offset;
    uint32_t length, flags, file, reserved;
};

struct PngiCode {
    uint16_t table[1 << PNGI_LIT_BITS];  // by the low bits of the input: symbol << 4 | length, 0 = no code of <= table bits here
    uint16_t sorted[320];                // the symbols by (length, symbol)
    uint16_t count[16];                  // codes per length
    int32_t status, total;
};

struct PngiShared {
    PngiCode lit, dist, cl;
    uint8_t lens[352];  // code lengths: literal / length [0, hlit), then distance [hlit, hlit + hdist)
};

struct PngiHostTeam {
    int lane = 0, lanes = 1;
    void sync() {}
};

struct PngiReader {
    const uint8_t* bytes;
    uint64_t nbytes;
    const PngiPiece* pieces;
    int piece, piece_end;
    uint64_t p, pend;  // the unread bytes of the current piece
    uint64_t acc;      // bits [0, nb) are valid; the bits above are either zero or the bytes at p that a later refill ORs in again
    int nb;
    // The window: bytes [wbase, wbase + wlen) of the current piece, where the reader takes its bytes from.  With a staging buffer (the
    // device: PNGI_WINDOW bytes of LDS) the team copies them there, consecutive lanes on consecutive bytes, so a refill waits for
    // LDS and not for global memory; without one (the host) the window is the piece itself.
    uint8_t* stage;
    const uint8_t* win;
    uint64_t wbase, wlen;
    int lane, lanes;

    PNGI_HD void init(const uint8_t* b, uint64_t n, const PngiPiece* pc, int first, int end, uint8_t* staging = nullptr, int ln = 0, int lns = 1)
    {
        bytes = b; nbytes = n; pieces = pc; piece = first - 1; piece_end = end; p = pend = 0; acc = 0; nb = 0;
        stage = staging; win = b; wbase = wlen = 0; lane = ln; lanes = lns;
    }
    PNGI_HD void slide(uint64_t q)  // q in [p, pend): every lane takes this path together
    {
        const uint64_t n = pend - q;
#if !defined(__HIP_DEVICE_COMPILE__)
        if (!stage) { win = bytes + q; wbase = q; wlen = n; return; }
#endif
        const uint32_t take_n = n < PNGI_WINDOW ? (uint32_t)n : (uint32_t)PNGI_WINDOW;
        PNGI_SYNC();  // the window's last readers are done
        for (uint32_t i = (uint32_t)lane; i < take_n; i += (uint32_t)lanes) stage[i] = bytes[q + i];
        PNGI_SYNC();
        win = stage; wbase = q; wlen = take_n;
    }
    // where the window's bytes are: on the device always the staging buffer (a team always stages), which keeps the loads LDS loads
    PNGI_HD const uint8_t* window() const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        return stage;
#else
        return win;
#endif
    }
    PNGI_HD uint8_t byte_at(uint64_t q)
    {
        if (q - wbase >= wlen) slide(q);
        return (uint8_t)PNGI_UNIFORM(window()[q - wbase]);
    }
    PNGI_HD bool next_piece()
    {
        while (++piece < piece_end) {
            const uint32_t flags = PNGI_UNIFORM(pieces[piece].flags), length = PNGI_UNIFORM(pieces[piece].length);
            const uint64_t offset = PNGI_UNIFORM64(pieces[piece].offset);
            if (!(flags & PNGI_PIECE_IDAT) || offset >= nbytes) continue;
            const uint64_t len = length < nbytes - offset ? length : nbytes - offset;
            if (!len) continue;
            p = offset;
            pend = p + len;
            return true;
        }
        piece = piece_end;
        return false;
    }
    PNGI_HD void refill()  // -> nb >= 56, or everything that is left
    {
        if (pend - p >= 8) {
            if (p - wbase >= wlen || wlen - (p - wbase) < 8) slide(p);  // -> wlen >= 8
            uint64_t v;
            memcpy(&v, window() + (p - wbase), 8);  // (little-endian hosts and the device)
            v = PNGI_UNIFORM64(v);
            acc |= v << nb;
            p += (uint64_t)((63 - nb) >> 3);
            nb |= 56;
            return;
        }
        while (nb <= 56) {
            if (p == pend && !next_piece()) break;
            acc |= (uint64_t)byte_at(p) << nb;
            p++;
            nb += 8;
        }
    }
    PNGI_HD void drop(int n) { acc >>= n; nb -= n; }  // n <= nb, n < 64
    PNGI_HD bool take(int n, uint32_t& v)             // n <= 32
    {
        if (nb < n) refill();
        if (nb < n) return false;
        v = (uint32_t)(acc & ((1ull << n) - 1ull));
        drop(n);
        return true;
    }
    PNGI_HD bool exhausted()
    {
        refill();
        return nb == 0;
    }
};

PNGI_HD uint32_t pngi_reverse(uint32_t code, int len)
{
    uint32_t r = 0;
    for (int i = 0; i < len; i++) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// lens[0, n) (in shared memory, written by lane 0 before the call) -> code.  kind: 0 literal / length (needs symbol 256), 1 distance,
// 2 code lengths.  As zlib: an over-subscribed code is an error; an incomplete one too, unless it is a literal / length or distance
// code whose longest length is 1; a distance code without any code is allowed (a match then finds no symbol).
template <class Team>
PNGI_HD int pngi_build(Team& tm, PngiCode& code, const uint8_t* lens, int n, int tbits, int kind)
{
    tm.sync();
    if (tm.lane == 0) {
        int count[16], offs[16];
        for (int l = 0; l < 16; l++) count[l] = 0;
        for (int s = 0; s < n; s++) count[lens[s] & 15]++;
        int left = 1, maxlen = 0, status = PNGI_OK;
        for (int l = 1; l < 16; l++) {
            left = (left << 1) - count[l];
            if (left < 0) { status = PNGI_BAD_CODE; break; }
            if (count[l]) maxlen = l;
        }
        if (status == PNGI_OK && left > 0 && maxlen > 0 && (kind == 2 || maxlen != 1)) status = PNGI_BAD_CODE;
        if (status == PNGI_OK && kind == 0 && (n <= 256 || lens[256] == 0)) status = PNGI_BAD_CODE;
        offs[1] = 0;
        for (int l = 1; l < 15; l++) offs[l + 1] = offs[l] + count[l];
        if (status == PNGI_OK)
            for (int s = 0; s < n; s++) {
                const int l = lens[s] & 15;
                if (l) code.sorted[offs[l]++] = (uint16_t)s;  // < n <= 320
            }
        for (int l = 0; l < 16; l++) code.count[l] = (uint16_t)count[l];
        code.count[0] = 0;
        code.total = n - count[0];
        code.status = status;
    }
    for (int i = tm.lane; i < (1 << PNGI_LIT_BITS); i += tm.lanes) code.table[i] = 0;
    tm.sync();
    if (code.status != PNGI_OK) return code.status;
    // entry j of sorted has the canonical code first[len] + (j - index[len]); the codes of <= tbits bits fill the table
    int first = 0, index = 0, len = 1;
    for (; len <= tbits; len++) {
        const int c = code.count[len];
        for (int j = tm.lane; j < c; j += tm.lanes) {
            const uint32_t sym = code.sorted[index + j];
            const uint32_t rev = pngi_reverse((uint32_t)(first + j), len);
            for (uint32_t k = rev; k < (1u << tbits); k += 1u << len) code.table[k] = (uint16_t)(sym << 4 | (uint32_t)len);
        }
        index += c;
        first = (first + c) << 1;
    }
    tm.sync();
    return PNGI_OK;
}

// -> the symbol, or -status.  The table serves codes of <= tbits bits; longer ones are walked bit by bit through the counts.
PNGI_HD int pngi_symbol(PngiReader& r, const PngiCode& code, int tbits)
{
    if (r.nb < 15) r.refill();  // the longest code
    const uint32_t e = PNGI_UNIFORM(code.table[r.acc & ((1u << tbits) - 1u)]);
    if (e) {
        const int len = (int)(e & 15u);
        if (len > r.nb) return -PNGI_TRUNCATED;
        r.drop(len);
        return (int)(e >> 4);
    }
    int c = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; len++) {
        if (len > r.nb) return -PNGI_TRUNCATED;
        c |= (int)((r.acc >> (len - 1)) & 1ull);
        const int count = (int)PNGI_UNIFORM(code.count[len]);
        if (c - count < first) {
            const int at = index + (c - first);
            if (at < 0 || at >= 320) return -PNGI_BAD_SYMBOL;
            r.drop(len);
            return (int)PNGI_UNIFORM(code.sorted[at]);
        }
        index += count;
        first = (first + count) << 1;
        c <<= 1;
    }
    return -PNGI_BAD_SYMBOL;
}

// the symbols of one block, after its tables are built
template <class Sink>
PNGI_HD int pngi_block_body(PngiReader& r, const PngiShared& sh, Sink& sink)
{
    for (;;) {
        const int sym = pngi_symbol(r, sh.lit, PNGI_LIT_BITS);
        if (sym < 0) return -sym;
        if (sym < 256) {
            if (!sink.lit((uint8_t)sym)) return PNGI_TOO_LONG;
            continue;
        }
        if (sym == 256) return PNGI_OK;
        if (sym > 285) return PNGI_BAD_SYMBOL;
        const int k = sym - 257;
        int len, eb;
        if (k < 8) { len = 3 + k; eb = 0; }
        else if (k == 28) { len = 258; eb = 0; }
        else { eb = (k - 4) >> 2; len = 3 + ((4 + (k & 3)) << eb); }
        uint32_t extra = 0;
        if (eb && !r.take(eb, extra)) return PNGI_TRUNCATED;
        len += (int)extra;
        const int d = pngi_symbol(r, sh.dist, PNGI_LIT_BITS);
        if (d < 0) return -d;
        if (d > 29) return PNGI_BAD_SYMBOL;
        uint32_t dist;
        if (d < 4) dist = 1u + (uint32_t)d;
        else {
            const int de = (d >> 1) - 1;
            if (!r.take(de, extra)) return PNGI_TRUNCATED;
            dist = 1u + ((2u + (uint32_t)(d & 1)) << de) + extra;
        }
        if ((uint64_t)dist > sink.pos) return PNGI_DISTANCE;
        if (!sink.match(len, dist)) return PNGI_TOO_LONG;
    }
}

template <class Team>
PNGI_HD int pngi_dynamic_tables(Team& tm, PngiReader& r, PngiShared& sh)
{
    uint32_t v;
    if (!r.take(14, v)) return PNGI_TRUNCATED;
    const int hlit = 257 + (int)(v & 31u), hdist = 1 + (int)((v >> 5) & 31u), hclen = 4 + (int)(v >> 10);
    if (hlit > 286 || hdist > 30) return PNGI_BAD_CODE;
    tm.sync();  // (the previous block's readers of lens are done)
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; i++) {
        uint32_t l = 0;
        if (i < hclen && !r.take(3, l)) return PNGI_TRUNCATED;
        if (tm.lane == 0) sh.lens[order[i]] = (uint8_t)l;
    }
    int rc = pngi_build(tm, sh.cl, sh.lens, 19, PNGI_CL_BITS, 2);
    if (rc != PNGI_OK) return rc;
    const int total = hlit + hdist;  // <= 316
    int prev = -1;
    for (int i = 0; i < total;) {
        const int sym = pngi_symbol(r, sh.cl, PNGI_CL_BITS);
        if (sym < 0) return -sym;
        int value = 0, repeat = 1;
        if (sym < 16) value = sym;
        else {
            uint32_t extra;
            if (sym == 16) {
                if (prev < 0) return PNGI_BAD_CODE;
                if (!r.take(2, extra)) return PNGI_TRUNCATED;
                value = prev;
                repeat = 3 + (int)extra;
            } else if (sym == 17) {
                if (!r.take(3, extra)) return PNGI_TRUNCATED;
                repeat = 3 + (int)extra;
            } else if (sym == 18) {
                if (!r.take(7, extra)) return PNGI_TRUNCATED;
                repeat = 11 + (int)extra;
            } else return PNGI_BAD_SYMBOL;
        }
        if (repeat > total - i) return PNGI_BAD_CODE;
        if (tm.lane == 0)
            for (int k = 0; k < repeat; k++) sh.lens[i + k] = (uint8_t)value;
        i += repeat;
        prev = value;
    }
    rc = pngi_build(tm, sh.lit, sh.lens, hlit, PNGI_LIT_BITS, 0);
    if (rc != PNGI_OK) return rc;
    return pngi_build(tm, sh.dist, sh.lens + hlit, hdist, PNGI_LIT_BITS, 1);
}

template <class Team>
PNGI_HD int pngi_fixed_tables(Team& tm, PngiShared& sh)
{
    tm.sync();
    for (int i = tm.lane; i < 320; i += tm.lanes) sh.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    const int rc = pngi_build(tm, sh.lit, sh.lens, 288, PNGI_LIT_BITS, 0);
    if (rc != PNGI_OK) return rc;
    return pngi_build(tm, sh.dist, sh.lens + 288, 32, PNGI_LIT_BITS, 1);
}

// One decode: a whole zlib stream (PNGI_HEAD | PNGI_TAIL) or one segment of it.  *trailer takes the Adler-32 when PNGI_TAIL is set.
template <class Team, class Sink>
PNGI_HD int pngi_inflate(Team& tm, PngiReader& r, PngiShared& sh, Sink& sink, int cover, uint32_t* trailer)
{
    uint32_t v;
    if ((cover & PNGI_HEAD) && !r.take(16, v)) return PNGI_TRUNCATED;
    for (;;) {
        if (!(cover & PNGI_TAIL) && r.exhausted()) return PNGI_OK;
        if (!r.take(3, v)) return PNGI_TRUNCATED;
        const bool final = (v & 1u) != 0;
        const int type = (int)(v >> 1);
        if (final && !(cover & PNGI_TAIL)) return PNGI_MISPLACED_FINAL;
        int rc;
        if (type == 0) {
            r.drop(r.nb & 7);
            if (!r.take(32, v)) return PNGI_TRUNCATED;
            if ((v & 0xffffu) != ((v >> 16) ^ 0xffffu)) return PNGI_STORED_LEN;
            rc = PNGI_OK;
            for (uint32_t n = v & 0xffffu; n; n--) {
                uint32_t b;
                if (!r.take(8, b)) return PNGI_TRUNCATED;
                if (!sink.lit((uint8_t)b)) return PNGI_TOO_LONG;
            }
        } else if (type == 3) {
            return PNGI_BLOCK_TYPE;
        } else {
            rc = type == 1 ? pngi_fixed_tables(tm, sh) : pngi_dynamic_tables(tm, r, sh);
            if (rc == PNGI_OK) rc = pngi_block_body(r, sh, sink);
        }
        if (rc != PNGI_OK) return rc;
        if (final) break;
    }
    r.drop(r.nb & 7);
    if (!r.take(32, v)) return PNGI_TRUNCATED;
    *trailer = (v << 24) | ((v & 0xff00u) << 8) | ((v >> 8) & 0xff00u) | (v >> 24);
    return PNGI_OK;
}

// a sink that only counts
struct PngiCountSink {
    uint64_t pos, limit;
    PNGI_HD bool lit(uint8_t) { if (pos >= limit) return false; pos++; return true; }
    PNGI_HD bool match(int len, uint32_t) { if ((uint64_t)len > limit - pos) return false; pos += (uint64_t)len; return true; }
};

// ---- the unfilter rule: filtered byte x, a = left (bpp back), b = above, c = above a; bytes outside the picture are 0 ----
PNGI_HD int pngi_unfilter(int type, int x, int a, int b, int c)
{
    int pred = 0;
    if (type == 1) pred = a;
    else if (type == 2) pred = b;
    else if (type == 3) pred = (a + b) >> 1;  // in int: 9 bits and more
    else if (type == 4) {
        const int p = a + b - c;
        const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);  // ties: a, b, c
    }
    return (x + pred) & 255;
}
