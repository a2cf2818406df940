// jpeg_entropy.h -- the entropy half of the JPEG decoder (include/gsraster_jpeg_decode.h, rules 1 and 2): the marker classes, the check of
// the restart markers' numbering, the Huffman tables, the bit reader and the interval loop.  Host and device: jpeg_decode.hip runs it
// with a one-wave team whose 64 lanes hold identical state, tools/jpeg_entropy_check.cpp with a team of one lane under sanitizers.
//
//   Team    lane, lanes, sync()              (sync: a barrier of the team; nothing on the host)
//   Fetch   uint8_t operator()(uint32_t at)  byte `at` of the scan, at < the scan's length; every lane asks for the same byte
//   Sink    put(k, v): coefficient at zigzag position k of the current block;  flush(block): the block is complete (all other
//           coefficients are 0), store it as block number `block` of the file
// The bit reader, the symbol and the value are written once for two modes (JPGE_WAVE / JPGE_LANE below): the interval loop here reads in
// wave mode, the split decode of jpeg_split.h in lane mode; the rules of a block (component, DC size, AC step) are functions both call.
// Every loop here consumes a bit or a coefficient, or ends at a fixed count; every table index is masked or checked.
#pragma once
#include <stdint.h>

#include "jpeg_tables.h"

#if defined(__HIPCC__)
#define JPGE_HD __host__ __device__ inline
#else
#define JPGE_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define JPGE_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))  // the lanes hold the same value: keep it in a scalar register
#else
#define JPGE_UNIFORM(x) ((uint32_t)(x))
#endif

// status codes: GSR_JPEG_DECODE_* of include/gsraster_jpeg_decode.h
enum { JPGE_OK = 0, JPGE_TRUNCATED, JPGE_BAD_CODE, JPGE_BAD_SYMBOL, JPGE_OVERRUN, JPGE_RESTART, JPGE_TABLE };
#define JPGE_LOOK_BITS 9

// natural (row-major) index of zigzag position k
JPGE_HD int jpge_natural(int k)
{
    constexpr uint8_t order[64] = { JPEG_ZIGZAG_LIST };
    return order[k & 63];
}

// rule 2: what the two bytes at a position are
enum { JPGE_NO_MARKER = 0, JPGE_RST, JPGE_CLOSING };
JPGE_HD int jpge_marker_class(uint8_t a, uint8_t b)
{
    if (a != 0xFF || b == 0x00 || b == 0xFF) return JPGE_NO_MARKER;
    return (b & 0xF8) == 0xD0 ? JPGE_RST : JPGE_CLOSING;
}
// the k-th RST marker of a scan carries m = k mod 8
JPGE_HD bool jpge_marker_numbered(uint8_t b, uint32_t k) { return b == (uint8_t)(0xD0u + (k & 7u)); }

struct JpgeHuffman {  // = gsr_jpeg_huffman
    uint8_t bits[16];
    uint8_t values[256];
};
struct JpgeCode {
    uint16_t look[1 << JPGE_LOOK_BITS];  // by the next JPGE_LOOK_BITS bits: length << 8 | symbol, 0 = no code that short
    int32_t maxcode[17];                 // the last code of a length, -1 = none
    int32_t delta[17];                   // index of the length's first symbol - its first code
    uint8_t values[256];
};

// Annex C.  false: more codes of a length than a prefix code has room for, or more than 256 codes.  The team builds the table together.
template <class Team>
JPGE_HD bool jpge_build(Team& tm, JpgeCode& code, const JpgeHuffman* src)
{
    int32_t mincode[17], first[17];
    uint32_t c = 0, at = 0;
    bool ok = true;
    tm.sync();  // the table's last readers are done
    for (int n = 1; n <= 16; n++) {
        const uint32_t count = JPGE_UNIFORM(src->bits[n - 1]);
        first[n] = (int32_t)at;
        mincode[n] = (int32_t)c;
        if (c + count > (1u << n)) ok = false;
        if (tm.lane == 0) {
            code.maxcode[n] = count ? (int32_t)(c + count - 1) : -1;
            code.delta[n] = (int32_t)at - (int32_t)c;
        }
        c = (c + count) << 1;
        at += count;
        if (!ok) break;  // (c stays below 2^17)
    }
    if (!ok || at > 256) return false;
    if (tm.lane == 0) code.maxcode[0] = -1, code.delta[0] = 0;
    for (int i = tm.lane; i < (1 << JPGE_LOOK_BITS); i += tm.lanes) code.look[i] = 0;
    for (int i = tm.lane; i < 256; i += tm.lanes) code.values[i] = i < (int)at ? src->values[i] : (uint8_t)0;
    tm.sync();
    for (int i = tm.lane; i < (int)at; i += tm.lanes) {
        int n = 1;
        while (n < 16 && i >= first[n + 1]) n++;  // the length whose symbols hold index i
        if (n > JPGE_LOOK_BITS) continue;
        const uint32_t cd = (uint32_t)mincode[n] + (uint32_t)(i - first[n]), span = 1u << (JPGE_LOOK_BITS - n);
        const uint16_t entry = (uint16_t)(n << 8 | src->values[i]);
        for (uint32_t j = 0; j < span; j++) code.look[((cd << (JPGE_LOOK_BITS - n)) + j) & ((1u << JPGE_LOOK_BITS) - 1u)] = entry;
    }
    tm.sync();
    return true;
}

// rule 2's verdict from what the walk over the scan found: whether a marker closes it, the RST markers in front of that one, whether
// each carries its number, and the intervals the file's geometry asks for
JPGE_HD int jpge_marker_verdict(bool closed, uint32_t rst_found, bool numbered, uint32_t intervals)
{
    if (!closed) return JPGE_TRUNCATED;
    return (rst_found + 1u != intervals || !numbered) ? JPGE_RESTART : JPGE_OK;
}

// How a reader keeps its words.  JPGE_WAVE: the team's lanes hold one state, every fetched byte and table word goes through JPGE_UNIFORM
// (scalar registers), and the reader does not know where it stands.  JPGE_LANE: a lane has a state of its own (jpeg_split.h), nothing is
// made uniform, and the reader tracks its position in the stuffed bytes (`pairs`, where()).
enum { JPGE_WAVE = 0, JPGE_LANE = 1 };
template <int Mode>
JPGE_HD uint32_t jpge_word(uint32_t x) { return Mode == JPGE_WAVE ? JPGE_UNIFORM(x) : x; }

// The bits of the scan from byte `start` on (JPGE_LANE: from its bit `bit`, 0 = the most significant), up to the interval's end.  acc holds
// nbits bits, right-aligned, of which the last `fake` were made up behind the end of the data (zeros); consuming one of them is an
// error.  Where the data ends, `end` comes down to `pos`: nothing more is taken, and `pos` stays what where() counts from.  `pairs`
// (JPGE_LANE only; a constant 0 otherwise): bit i = the i-th last byte taken into acc was the FF of an FF 00 pair (two bytes of the scan).
template <class Fetch, int Mode>
struct JpgeReader {
    Fetch in;
    uint32_t pos, end;
    uint64_t acc;
    uint32_t pairs;
    int nbits, fake;
    JPGE_HD JpgeReader(const Fetch& f, uint32_t start, uint32_t stop, int bit = 0) : in(f), pos(start), end(stop), acc(0), pairs(0), nbits(0), fake(0)
    {
        if (Mode == JPGE_LANE) {
            refill();
            nbits -= bit & 7;  // (nbits > 56)
        }
    }
    JPGE_HD void refill()  // -> nbits > 56; every round takes a byte of the data or makes one up
    {
        while (nbits <= 56) {
            uint32_t b = 0, pair = 0;
            bool have = false;
            if (pos < end) {
                b = jpge_word<Mode>(in(pos));
                if (b != 0xFFu) { pos++; have = true; }
                else if (pos + 1 < end && jpge_word<Mode>(in(pos + 1)) == 0u) { pos += 2; have = true; pair = 1; }
                else end = pos;  // a fill byte, or the interval's last byte: the data ends here
            }
            if (!have) { b = 0; fake += 8; }
            acc = (acc << 8) | b;
            if (Mode == JPGE_LANE) pairs = (pairs << 1) | pair;
            nbits += 8;
        }
    }
    JPGE_HD uint32_t peek(int n) const { return (uint32_t)(acc >> (nbits - n)) & ((1u << n) - 1u); }  // n <= 16 <= nbits
    JPGE_HD bool drop(int n) { nbits -= n; return nbits >= fake; }                                       // false: made-up bits were used
    JPGE_HD int real() const { return nbits - fake; }
    // JPGE_LANE: where the next bit lies; meaningful while no made-up bit has been used
    JPGE_HD void where(uint32_t& byte, int& bit) const
    {
        const int held = (nbits + 7) >> 3, made = fake >> 3, live = held > made ? held - made : 0;  // bytes of acc not fully consumed; the made-up ones; the data's
        const uint32_t twice = (uint32_t)__builtin_popcount((pairs >> made) & ((1u << live) - 1u));  // (live <= 8)
        byte = pos - (uint32_t)live - twice;
        bit = (8 - (nbits & 7)) & 7;
    }
};

// the next symbol -> 0 .. 255, or -(status code): short_code where the data ended, else JPGE_BAD_CODE
template <class Fetch, int Mode>
JPGE_HD int jpge_symbol(JpgeReader<Fetch, Mode>& r, const JpgeCode& code, int short_code)
{
    if (r.nbits < 32) r.refill();
    const uint32_t w = r.peek(16);
    const uint32_t quick = jpge_word<Mode>(code.look[w >> (16 - JPGE_LOOK_BITS)]);
    int n = (int)(quick >> 8), sym = (int)(quick & 255u);
    if (!n) {
        for (n = JPGE_LOOK_BITS + 1; n <= 16; n++) {
            const int32_t c = (int32_t)(w >> (16 - n));
            if (c <= (int32_t)jpge_word<Mode>(code.maxcode[n])) {
                sym = (int)jpge_word<Mode>(code.values[(uint32_t)(c + (int32_t)jpge_word<Mode>(code.delta[n])) & 255u]);
                break;
            }
        }
        if (n > 16) return r.real() < 16 ? -short_code : -JPGE_BAD_CODE;
    }
    return r.drop(n) ? sym : -short_code;
}

// `size` value bits -> the coefficient (size <= 11; at most 27 bits since the refill in jpge_symbol); false: the data ended
template <class Fetch, int Mode>
JPGE_HD bool jpge_value(JpgeReader<Fetch, Mode>& r, int size, int32_t& v)
{
    v = 0;
    if (!size) return true;
    const int32_t bits = (int32_t)r.peek(size);
    v = bits < (1 << (size - 1)) ? bits - (1 << size) + 1 : bits;
    return r.drop(size);
}

// ---- the rules of a block, for the interval loop below and for jps_unit (jpeg_split.h) ----
// the component of block j of an MCU whose first ny blocks are component 0's
JPGE_HD int jpge_component(int j, int ny) { return j < ny ? 0 : (j - ny + 1 > 2 ? 2 : j - ny + 1); }
// a DC symbol is the size of the difference
JPGE_HD bool jpge_dc_sound(int s) { return s <= 11; }
// The AC symbol rs with the block at zigzag position k -> status code.  JPGE_OK: k is where the value goes and `size` its bits; size 0:
// no value follows, and k is 64 after the end-of-block symbol, 16 further after ZRL.
JPGE_HD int jpge_ac_step(int rs, int& k, int& size)
{
    const int run = rs >> 4;
    size = rs & 15;
    if (size > 10 || (size == 0 && run != 0 && run != 15)) return JPGE_BAD_SYMBOL;
    if (rs == 0) { k = 64; return JPGE_OK; }
    k += run + (size == 0);  // the zeros; ZRL is sixteen of them and must leave room for a value
    return k > 63 ? JPGE_OVERRUN : JPGE_OK;
}

// One restart interval: the MCUs [first_mcu, first_mcu + mcus) of a file from the bytes [start, end) of its scan.  codes[2c], codes[2c + 1]:
// component c's DC and AC tables.  ny = component 0's blocks per MCU, bpm = all blocks per MCU.  -> status code
template <class Fetch, class Sink>
JPGE_HD int jpge_interval(const Fetch& in, uint32_t start, uint32_t end, bool ended_by_rst, const JpgeCode* const* codes, int ny, int bpm,
                          uint32_t first_mcu, uint32_t mcus, Sink& sink)
{
    const int short_code = ended_by_rst ? JPGE_RESTART : JPGE_TRUNCATED;
    JpgeReader<Fetch, JPGE_WAVE> r(in, start, end);
    uint32_t pred[3] = { 0u, 0u, 0u };  // (unsigned: a crafted file may wrap it)
    for (uint32_t m = 0; m < mcus; m++)
        for (int j = 0; j < bpm; j++) {
            const int c = jpge_component(j, ny);
            const JpgeCode& ac_code = *codes[2 * c + 1];  // (read once per block, not once per symbol)
            int s = jpge_symbol(r, *codes[2 * c], short_code);
            if (s < 0) return -s;
            if (!jpge_dc_sound(s)) return JPGE_BAD_SYMBOL;
            int32_t v;
            if (!jpge_value(r, s, v)) return short_code;
            pred[c] += (uint32_t)v;
            sink.put(0, (int16_t)(uint16_t)pred[c]);
            for (int k = 1; k < 64;) {
                const int rs = jpge_symbol(r, ac_code, short_code);
                if (rs < 0) return -rs;
                const int rc = jpge_ac_step(rs, k, s);
                if (rc != JPGE_OK) return rc;
                if (s) {
                    if (!jpge_value(r, s, v)) return short_code;
                    sink.put(k, (int16_t)v);
                    k++;
                }
            }
            sink.flush((size_t)(first_mcu + m) * (size_t)bpm + (size_t)j);
        }
    r.refill();
    return r.real() >= 8 ? JPGE_RESTART : JPGE_OK;  // a whole byte behind the last MCU
}
