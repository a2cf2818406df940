// jpeg_split.h -- the core of the split JPEG decode (include/gsraster_jpeg_split.h, rules 1 to 4 and 6): where a subsequence begins,
// the decoder's state and its packed form, one decoding unit, and the run of a decoder through one subsequence.  Host and device:
// jpeg_split.hip gives every lane a decoder of its own, tools/jpeg_split_check.cpp emulates the lanes one after another under
// sanitizers.  The tables (JpgeCode, jpge_build), the marker classes, the status codes, the bit reader, the symbol, the value and the
// rules of a block are jpeg_entropy.h's; the reader runs here in its lane mode (JPGE_LANE): nothing made uniform, and it knows where it
// stands in the stuffed bytes.
//
//   Fetch   uint8_t operator()(uint32_t at)  byte `at` of the scan, at < the scan's length; every lane asks for a byte of its own
//   Sink    bool full(int k)                  true: decode no further unit (k = the state's: the interval's last block is complete)
//           void dc(int32_t diff)             a block begins: its DC difference
//           void ac(int k, int32_t v)         coefficient at zigzag position k of the current block
// Every loop consumes a bit of the data or ends at a count fixed before it starts; every table index is masked or checked.
#pragma once
#include <stdint.h>

#include "jpeg_entropy.h"

#define JPS_MIN_BYTES 16
#define JPS_MAX_BYTES 1024
#define JPS_NO_STATE 0xffffffffu  // the packed form of "no state": a decoder that failed

JPGE_HD bool jps_bytes_allowed(int b) { return b >= JPS_MIN_BYTES && b <= JPS_MAX_BYTES && (b & (b - 1)) == 0; }

// rule 1: an interval [start, end) of the scan cut into subsequences of B bytes
struct JpsCut {
    uint32_t start, end, B, count;  // count = ceil((end - start) / B), less one that would be empty
};
template <class Fetch>
JPGE_HD JpsCut jps_cut(Fetch& in, uint32_t start, uint32_t end, uint32_t B)
{
    JpsCut c = {start, end, B, 0u};
    if (end > start) c.count = (end - start - 1u) / B + 1u;  // (< 2^28: B >= 16)
    // the last one would begin on the interval's last byte, and that byte is the 00 of a pair: it would begin at the end, and is none
    if (c.count > 1u && start + (c.count - 1u) * B == end - 1u && in(end - 2u) == 0xFFu) c.count--;
    return c;
}
// the byte at which subsequence i begins, i <= count; i = count: the interval's end
template <class Fetch>
JPGE_HD uint32_t jps_begin(Fetch& in, const JpsCut& c, uint32_t i)
{
    if (i == 0) return c.start;
    if (i >= c.count) return c.end;
    uint32_t at = c.start + i * c.B;  // < end
    if (in(at - 1u) == 0xFFu) at++;  // the nominal byte is the stuffed 00
    return at;  // < end (jps_cut)
}

// rule 2, in the stuffed bytes: the next bit to read is bit `bit` (0 = the most significant) of byte `byte` of the scan; never the 00 of
// a pair.  Equal positions here are equal positions in the de-stuffed stream.
struct JpsState {
    uint32_t byte;
    int bit, j, k;
    bool ok;
};
// A state between subsequence x and x + 1, relative to `begin` = where x + 1 begins: the unit in front of it started before `begin` and
// is at most 27 bits, so the distance is small.  bits 0 .. 11 the distance in bits, 12 .. 15 j, 16 .. 21 k.
JPGE_HD uint32_t jps_pack(const JpsState& s, uint32_t begin)
{
    if (!s.ok || s.byte < begin || s.byte - begin >= 256u) return JPS_NO_STATE;
    return ((s.byte - begin) << 3 | (uint32_t)s.bit) | (uint32_t)s.j << 12 | (uint32_t)s.k << 16;
}
JPGE_HD JpsState jps_unpack(uint32_t w, uint32_t begin, int bpm)
{
    JpsState s = {begin + ((w & 0xfffu) >> 3), (int)(w & 7u), (int)(w >> 12 & 15u), (int)(w >> 16 & 63u), true};
    if (w == JPS_NO_STATE || (w >> 22) != 0u || s.j >= bpm) s.ok = false;
    return s;
}

template <class Fetch>
using JpsReader = JpgeReader<Fetch, JPGE_LANE>;  // from (byte, bit) of a state on: JpsReader(in, s.byte, stop, s.bit)

// The file's lookup tables: entry 2c is component c's DC table, 2c + 1 its AC table; slot e of `slots` (four bits each) is the entry's
// place in `base`, so a table two components share is stored once and a lane finds its table by arithmetic, not through an array of
// pointers (which a lane that indexes it by its own j keeps in private memory).
struct JpsTables {
    const JpgeCode* base;  // at most 6 tables
    uint32_t slots;        // each below 6
    JPGE_HD const JpgeCode& at(int e) const { return base[(slots >> (4 * e)) & 7u]; }
};

// One decoding unit in state (j, k) -> the next (j, k); false: the unit fails under rule 1 of gsraster_jpeg_decode.h (any of its codes).
template <class Fetch, class Sink>
JPGE_HD bool jps_unit(JpsReader<Fetch>& r, const JpsTables& codes, int ny, int bpm, int& j, int& k, Sink& sink)
{
    const int c = jpge_component(j, ny);
    int32_t v;
    int s;
    if (k == 0) {
        s = jpge_symbol(r, codes.at(2 * c), JPGE_TRUNCATED);  // (which code it fails with does not matter here: any negative result fails)
        if (s < 0 || !jpge_dc_sound(s) || !jpge_value(r, s, v)) return false;
        sink.dc(v);
        k = 1;
        return true;
    }
    const int rs = jpge_symbol(r, codes.at(2 * c + 1), JPGE_TRUNCATED);
    if (rs < 0 || jpge_ac_step(rs, k, s) != JPGE_OK) return false;
    if (s) {
        if (!jpge_value(r, s, v)) return false;
        sink.ac(k, v);
        k++;
    }
    if (k == 64) { k = 0; j = j + 1 < bpm ? j + 1 : 0; }
    return true;
}

// A decoder in state `s` runs through the units whose first bit lies in front of byte `limit` (where the next subsequence begins;
// limit <= stop = the interval's end).  -> the state in front of the first unit at or beyond `limit` (rule 3), s.ok = false when a
// unit failed.  At most 8 (limit - s.byte) units: each takes a bit at least.
template <class Fetch, class Sink>
JPGE_HD void jps_run(const Fetch& in, JpsState& s, uint32_t limit, uint32_t stop, const JpsTables& codes, int ny, int bpm, Sink& sink)
{
    if (!s.ok || s.byte >= limit) return;
    JpsReader<Fetch> r(in, s.byte, stop, s.bit);
    const uint32_t most = 8u * (limit - s.byte);  // (limit - s.byte: a subsequence and the tail of a unit, far below 2^29)
    for (uint32_t n = 0; n < most; n++) {
        if (s.byte >= limit || sink.full(s.k)) return;
        if (!jps_unit(r, codes, ny, bpm, s.j, s.k, sink)) { s.ok = false; return; }
        r.where(s.byte, s.bit);
    }
}

// what the synchronisation passes listen for: the blocks begun
struct JpsCount {
    uint32_t blocks;
    JPGE_HD bool full(int) const { return false; }
    JPGE_HD void dc(int32_t) { blocks++; }
    JPGE_HD void ac(int, int32_t) {}
};

// ---- the passes, one lane's part each; `entry`, `blocks`, `first` are the interval's own words, one per subsequence ----
// entry[x]: the packed state between subsequence x and x + 1 (the entry state of x + 1); blocks[x], first[x]: rule 4.
struct JpsInterval {
    JpsCut cut;
    JpsTables codes;
    int ny, bpm;
    uint32_t total;  // the interval's blocks, MCUs bpm
};

// A decoder in state s goes through subsequence x: it leaves the blocks it began there, and its state at the end unless that is the
// state already stored (cold = round 0: nothing is stored yet).  -> true: it goes on into x + 1; false: it matched, failed, or x is the last.
template <class Fetch>
JPGE_HD bool jps_through(Fetch& in, const JpsInterval& iv, uint32_t x, JpsState& s, bool cold, uint32_t* entry, uint32_t* blocks)
{
    const uint32_t limit = jps_begin(in, iv.cut, x + 1u);
    JpsCount count = {0u};
    jps_run(in, s, limit, iv.cut.end, iv.codes, iv.ny, iv.bpm, count);
    blocks[x] = count.blocks;
    if (x + 1u >= iv.cut.count) return false;
    const uint32_t w = jps_pack(s, limit);
    if (!cold && w != JPS_NO_STATE && w == entry[x]) return false;
    entry[x] = w;
    return w != JPS_NO_STATE;
}
// round 0 of the sync within a chunk: subsequence x cold
template <class Fetch>
JPGE_HD bool jps_cold(Fetch& in, const JpsInterval& iv, uint32_t x, JpsState& s, uint32_t* entry, uint32_t* blocks)
{
    s.byte = jps_begin(in, iv.cut, x);
    s.bit = s.j = s.k = 0;
    s.ok = true;
    return jps_through(in, iv, x, s, true, entry, blocks);
}
// the sync across chunks of `chunk` subsequences: from the verified exit of chunk c - 1 into chunk c until the stored state is met
template <class Fetch>
JPGE_HD void jps_walk(Fetch& in, const JpsInterval& iv, uint32_t chunk, uint32_t* entry, uint32_t* blocks)
{
    for (uint32_t x0 = chunk; x0 < iv.cut.count; x0 += chunk) {
        JpsState s = jps_unpack(entry[x0 - 1u], jps_begin(in, iv.cut, x0), iv.bpm);
        const uint32_t x1 = iv.cut.count - x0 < chunk ? iv.cut.count : x0 + chunk;
        for (uint32_t x = x0; x < x1 && s.ok; x++)
            if (!jps_through(in, iv, x, s, false, entry, blocks)) break;
    }
}

// the write pass's sink: store(block, k, v) gets the block's number within the interval (below total) and the zigzag position
template <class Store>
struct JpsPlace {
    Store& store;
    uint32_t cur, next, total, begun;
    bool bad;
    JPGE_HD bool full(int k) const { return k == 0 && next >= total; }
    JPGE_HD void dc(int32_t v)
    {
        if (next >= total) { bad = true; return; }
        cur = next++;
        begun++;
        store(cur, 0, v);
    }
    JPGE_HD void ac(int k, int32_t v)
    {
        if (cur >= total) { bad = true; return; }
        store(cur, k, v);
    }
};
// Subsequence x from its final entry state: the DC differences and AC values to `store`, and the checks of rule 6.  -> false: repair.
template <class Fetch, class Store>
JPGE_HD bool jps_write(Fetch& in, const JpsInterval& iv, uint32_t x, const uint32_t* entry, const uint32_t* blocks, const uint32_t* first, Store& store)
{
    const uint32_t begin = jps_begin(in, iv.cut, x), limit = jps_begin(in, iv.cut, x + 1u), fb = first[x];
    JpsState s = {begin, 0, 0, 0, true};
    if (x) s = jps_unpack(entry[x - 1u], begin, iv.bpm);
    if (!s.ok || fb > iv.total) return false;
    JpsPlace<Store> place = {store, fb, fb, iv.total, 0u, false};
    if (s.k) {  // in the middle of the block begun before
        if (!fb) return false;
        place.cur = fb - 1u;
    }
    if (place.cur % (uint32_t)iv.bpm != (uint32_t)s.j) return false;
    jps_run(in, s, limit, iv.cut.end, iv.codes, iv.ny, iv.bpm, place);
    if (!s.ok || place.bad || place.begun != blocks[x]) return false;
    if (x + 1u < iv.cut.count) {
        const uint32_t w = jps_pack(s, limit);
        return w != JPS_NO_STATE && w == entry[x];
    }
    if (fb + place.begun != iv.total || s.k) return false;
    JpsReader<Fetch> rest(in, s.byte, iv.cut.end, s.bit);
    return rest.real() < 8;  // a whole byte behind the last MCU is the serial decoder's RESTART
}
