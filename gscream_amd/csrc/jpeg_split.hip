// jpeg_split.hip -- baseline JPEG decoding with an interval's scan split at self-synchronisation points: the rules, the launches and
// the repair are in include/gsraster_jpeg_split.h in full; the core (where a subsequence begins, the state, one lane's part of every pass, over
// jpeg_entropy.h's bit reader in its lane mode) is jpeg_split.h, which tools/jpeg_split_check.cpp runs on the host under sanitizers over the same corpus.
// Here one lane decodes one subsequence with a state of its own (in jpeg_decode.hip's entropy kernel 64 lanes hold one state); the
// file's six lookup tables sit in LDS (8.5 KB) and are read divergently; a lane's bytes come through one aligned dword it keeps in a
// register.  The launches run inside jpeg_decode.hip's own sequence (jpeg_decode_launch.h), between its markers and entropy kernels:
//   classify : one workgroup of 1024, a thread per run of intervals: which intervals are split (at least min_bytes, at least two
//              subsequences, room in the tables), and by two scans where their subsequences and chunks lie
//   sync     : a workgroup of JS_CHUNK lanes per chunk of JS_CHUNK subsequences: round 0 cold, round r through subsequence i + r until
//              the state stored there by the round before is met; one barrier a round, at most JS_CHUNK rounds
//   walk     : a lane per split interval of more than one chunk: from chunk c - 1's verified exit into chunk c until the stored state is met
//   pairs    : (only with a trace) a lane per subsequence: its FF 00 pairs, for the de-stuffed bit position the trace reports
//   scan     : a workgroup per split interval: first_block = the exclusive sum of blocks (gsr_scan.h)
//   clear    : zeros in the coefficients of the split intervals' blocks (the write pass stores what is coded, nothing else)
//   write    : a lane per subsequence from its final entry state: DC differences and AC values, and rule 6's checks; a failed check
//              stores 1 into the interval's word of `only` (every writer stores the same value)
//   dc       : a workgroup per split interval that needs no repair: per component the ordered prefix sum of the DC differences
//   info     : a thread per file
// and then jpeg_decode.hip's entropy kernel decodes exactly the intervals whose word of `only` is set.  No workgroup waits for another,
// nothing spins, no global atomics; a slot of `entry` / `blocks` is written by one lane per round and launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsraster_jpeg_split.h"
#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_scan.h"
#include "jpeg_decode_launch.h"
#include "jpeg_split.h"

#define JS_CHUNK 256  // subsequences per chunk = lanes per workgroup of sync and write

static_assert(sizeof(gsr_jpeg_split_trace) == 20, "the trace's layout");

struct JsTables {
    unsigned long long *sub_first, *chunk_first;  // per interval: its first subsequence and chunk among the call's
    uint32_t* count;                               // per interval: its subsequences (0: not split)
    int32_t *split, *only;                         // per interval: takes the split path; is the entropy kernel's (not split, or repair)
    uint32_t *entry, *blocks, *first, *pairs;      // per subsequence (jpeg_split.h); pairs: the FF 00 pairs in front of it in its interval
    unsigned long long max_subs, max_chunks;
};
struct JsCarve {
    JsTables t;
    size_t bytes;
};
// scan_bytes / B + nintervals subsequences at most: an interval holds ceil(n / B) of them and the intervals of sound tables do not overlap
static JsCarve js_carve(void* base, int nintervals, size_t scan_bytes, int B)
{
    JsCarve r{};
    GsrCarver c(base);
    const size_t subs = scan_bytes / (size_t)B + (size_t)nintervals;
    r.t.max_subs = subs;
    r.t.max_chunks = subs / JS_CHUNK + (size_t)nintervals;
    r.t.sub_first = c.take<unsigned long long>((size_t)nintervals, 16);
    r.t.chunk_first = c.take<unsigned long long>((size_t)nintervals, 16);
    r.t.count = c.take<uint32_t>((size_t)nintervals, 16);
    r.t.split = c.take<int32_t>((size_t)nintervals, 16);
    r.t.only = c.take<int32_t>((size_t)nintervals, 16);
    r.t.entry = c.take<uint32_t>(subs, 16);
    r.t.blocks = c.take<uint32_t>(subs, 16);
    r.t.first = c.take<uint32_t>(subs, 16);
    r.t.pairs = c.take<uint32_t>(subs, 16);
    r.bytes = c.total();
    return r;
}

// byte `at` of a file's scan through the aligned dword that holds it, kept in a register; a dword that reaches over the scan's end is
// read byte by byte
struct JsFetch {
    JdScan scan;
    uint32_t base, word;  // base 0xffffffff = nothing loaded
    __device__ uint8_t operator()(uint32_t at)
    {
        const uint32_t q = at + scan.shift;
        if ((q & ~3u) != base) {
            base = q & ~3u;
            word = scan.dword(base);
        }
        return (uint8_t)(word >> (8u * (q & 3u)));
    }
};
__device__ __forceinline__ JsFetch js_fetch(const uint8_t* bytes, const gsr_jpeg_file& fl) { return JsFetch{jd_scan(bytes, fl), 0xffffffffu, 0u}; }

// interval i of file fl: its bytes cut by B, its blocks
struct JsPiece {
    JpsCut cut;
    uint32_t first_mcu, total;
    int ny, bpm;
};
__device__ __forceinline__ JsPiece js_piece(JsFetch& in, const gsr_jpeg_file& fl, int i, const JdWorkspace& ws, uint32_t B)
{
    const JdGeometry g = jd_geometry(fl);
    const JdPiece q = jd_piece(fl, g, i, ws);
    return JsPiece{jps_cut(in, q.start, max(q.start, q.end), B), q.first_mcu, q.mcus * (uint32_t)g.bpm, g.ny, g.bpm};
}

// ---- classify ----
__global__ void __launch_bounds__(1024) jpeg_split_classify_kernel(const uint8_t* __restrict__ bytes, const gsr_jpeg_file* __restrict__ files, int nfiles,
                                                                   int nintervals, JdWorkspace ws, const int32_t* status, JsTables t, uint32_t B,
                                                                   uint32_t min_bytes)
{
    const int per = (nintervals + 1023) / 1024, i0 = (int)threadIdx.x * per;
    for (int i = i0; i < i0 + per && i < nintervals; i++) {
        uint32_t count = 0;
        const int f = jd_owner(i, files, nfiles, ws, status);
        if (f >= 0) {
            const gsr_jpeg_file fl = files[f];
            JsFetch in = js_fetch(bytes, fl);
            const JpsCut cut = js_piece(in, fl, i, ws, B).cut;
            if (cut.end - cut.start >= min_bytes && cut.count >= 2u && cut.count <= t.max_subs) count = cut.count;
        }
        t.count[i] = count;
        t.sub_first[i] = count;
        t.chunk_first[i] = (count + JS_CHUNK - 1u) / JS_CHUNK;
    }
    __syncthreads();
    unsigned long long* const both[2] = {t.sub_first, t.chunk_first};
    unsigned long long totals[2];
    gsr_top_scan(nintervals, both, totals);
    for (int i = i0; i < i0 + per && i < nintervals; i++) {  // (this thread's own entries)
        const uint32_t count = t.count[i];
        const bool room = t.sub_first[i] + count <= t.max_subs && t.chunk_first[i] + (count + JS_CHUNK - 1u) / JS_CHUNK <= t.max_chunks;
        const int split = count && room;
        if (!split) t.count[i] = 0u;
        t.split[i] = split;
        t.only[i] = !split;
    }
}

// the interval that holds chunk `chunk` of the call and takes the split path, or -1; *c = the chunk's number within it
__device__ __forceinline__ int js_chunk_interval(unsigned long long chunk, int nintervals, const JsTables& t, uint32_t* c)
{
    int lo = 0, hi = nintervals;  // the last interval whose first chunk is <= chunk
    while (hi - lo > 1) {         // (log2 nintervals rounds)
        const int mid = lo + (hi - lo) / 2;
        if (t.chunk_first[mid] <= chunk) lo = mid;
        else hi = mid;
    }
    const unsigned long long at = chunk - t.chunk_first[lo];
    if (t.chunk_first[lo] > chunk || !t.split[lo] || at >= (t.count[lo] + JS_CHUNK - 1u) / JS_CHUNK) return -1;
    *c = (uint32_t)at;
    return lo;
}

// the file's lookup tables, built by the workgroup together (all its threads call); false: a table is unsound
__device__ __forceinline__ bool js_build(JdTeam tm, JpgeCode* codes, JpsTables& use, const gsr_jpeg_file& fl, const JpgeHuffman* huffman)
{
    uint32_t slots;
    const bool sound = jd_build(tm, codes, fl, huffman, slots);
    if (fl.C == 1) slots |= slots << 8 | slots << 16;  // (j is 0 in a grey file: never followed)
    use.base = codes;
    use.slots = slots;
    return sound;
}

// ---- sync within a chunk ----
__global__ void __launch_bounds__(JS_CHUNK) jpeg_split_sync_kernel(const uint8_t* __restrict__ bytes, const gsr_jpeg_file* __restrict__ files, int nfiles,
                                                                   int nintervals, const JpgeHuffman* __restrict__ huffman, JdWorkspace ws,
                                                                   const int32_t* status, JsTables t, uint32_t B)
{
    __shared__ JpgeCode codes[6];
    const int tid = (int)threadIdx.x;
    uint32_t c = 0;
    const int i = js_chunk_interval(blockIdx.x, nintervals, t, &c);
    if (i < 0) return;
    const int f = jd_owner(i, files, nfiles, ws, status);
    if (f < 0) return;
    const gsr_jpeg_file fl = files[f];
    JpsTables use;
    if (!js_build(JdTeam{tid, JS_CHUNK}, codes, use, fl, huffman)) return;  // (the write pass finds the same and hands the interval over)
    JsFetch in = js_fetch(bytes, fl);
    const JsPiece p = js_piece(in, fl, i, ws, B);
    const JpsInterval iv = {p.cut, use, p.ny, p.bpm, p.total};
    uint32_t* entry = t.entry + t.sub_first[i];
    uint32_t* blocks = t.blocks + t.sub_first[i];
    const uint32_t x = c * JS_CHUNK + (uint32_t)tid;
    JpsState s = {};
    bool active = x < iv.cut.count && jps_cold(in, iv, x, s, entry, blocks);
    for (uint32_t r = 1; r < JS_CHUNK; r++) {
        if (!__syncthreads_or(active)) break;  // (the barrier between rounds: round r reads what round r - 1 stored)
        if (!active) continue;
        if ((uint32_t)tid + r >= JS_CHUNK || x + r >= iv.cut.count) { active = false; continue; }
        active = jps_through(in, iv, x + r, s, false, entry, blocks);
    }
}

// ---- sync across chunks ----
__global__ void __launch_bounds__(64) jpeg_split_walk_kernel(const uint8_t* __restrict__ bytes, const gsr_jpeg_file* __restrict__ files, int nfiles,
                                                             const JpgeHuffman* __restrict__ huffman, JdWorkspace ws, const int32_t* status, JsTables t,
                                                             uint32_t B)
{
    __shared__ JpgeCode codes[6];
    const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (!t.split[i] || t.count[i] <= JS_CHUNK) return;  // (one chunk: subsequence 0 started from the true state)
    const int f = jd_owner(i, files, nfiles, ws, status);
    if (f < 0) return;
    const gsr_jpeg_file fl = files[f];
    JpsTables use;
    if (!js_build(JdTeam{lane, 64}, codes, use, fl, huffman) || lane) return;
    JsFetch in = js_fetch(bytes, fl);
    const JsPiece p = js_piece(in, fl, i, ws, B);
    const JpsInterval iv = {p.cut, use, p.ny, p.bpm, p.total};
    jps_walk(in, iv, JS_CHUNK, t.entry + t.sub_first[i], t.blocks + t.sub_first[i]);  // (at most the interval's units: the serial decode)
}

// ---- pairs (trace only) ----
__global__ void __launch_bounds__(JS_CHUNK) jpeg_split_pairs_kernel(const uint8_t* __restrict__ bytes, const gsr_jpeg_file* __restrict__ files, int nfiles,
                                                                    int nintervals, JdWorkspace ws, const int32_t* status, JsTables t, uint32_t B)
{
    uint32_t c = 0;
    const int i = js_chunk_interval(blockIdx.x, nintervals, t, &c);
    if (i < 0) return;
    const int f = jd_owner(i, files, nfiles, ws, status);
    if (f < 0) return;
    const gsr_jpeg_file fl = files[f];
    JsFetch in = js_fetch(bytes, fl);
    const JpsCut cut = js_piece(in, fl, i, ws, B).cut;
    const uint32_t x = c * JS_CHUNK + threadIdx.x;
    if (x >= cut.count) return;
    const uint32_t a = jps_begin(in, cut, x), b = jps_begin(in, cut, x + 1u);
    uint32_t n = 0;
    for (uint32_t at = a; at < b; at++) n += in(at) == 0xFFu;  // (b - a <= B + 1)
    t.pairs[t.sub_first[i] + x] = n;
}

// ---- scan ----
__global__ void __launch_bounds__(256) jpeg_split_scan_kernel(JsTables t, int with_pairs)
{
    const int i = (int)blockIdx.x;
    if (!t.split[i]) return;
    const uint32_t* blocks = t.blocks + t.sub_first[i];
    uint32_t* first = t.first + t.sub_first[i];
    gsr_block_scan_runs<256, 0>((int)t.count[i], [&](int x) { return blocks[x]; }, [&](int x, uint32_t start, uint32_t) { first[x] = start; });
    if (!with_pairs) return;
    __syncthreads();  // (gsr_scan.h: one barrier between two calls of the same form)
    uint32_t* pairs = t.pairs + t.sub_first[i];
    gsr_block_scan_runs<256, 0>((int)t.count[i], [&](int x) { return pairs[x]; }, [&](int x, uint32_t start, uint32_t) { pairs[x] = start; });
}

// ---- clear ----
__global__ void __launch_bounds__(256) jpeg_split_clear_kernel(const gsr_jpeg_file* __restrict__ files, JdWorkspace ws, const int32_t* __restrict__ status,
                                                               JsTables t)
{
    const int f = (int)blockIdx.y;
    if (status[2 * f] != GSR_JPEG_DECODE_OK) return;
    const gsr_jpeg_file fl = files[f];
    const JdGeometry g = jd_geometry(fl);
    uint4* coef = (uint4*)(ws.area + fl.coef_offset);  // (16-byte aligned, 128 bytes a block: validate)
    const uint32_t per_interval = g.per * (uint32_t)g.bpm;  // blocks
    for (unsigned long long q = (unsigned long long)blockIdx.x * 256u + threadIdx.x; q < 8ull * g.blocks; q += (unsigned long long)gridDim.x * 256u) {
        const uint32_t k = (uint32_t)(q >> 3) / per_interval;  // < fl.intervals
        if (t.split[fl.first_interval + (int)k]) coef[q] = make_uint4(0u, 0u, 0u, 0u);
    }
}

// ---- write ----
struct JsStore {
    int16_t* out;  // the interval's first block
    __device__ void operator()(uint32_t block, int k, int32_t v) { out[(size_t)block * 64 + (size_t)jpge_natural(k)] = (int16_t)v; }  // block < the interval's blocks, k < 64
};

__global__ void __launch_bounds__(JS_CHUNK) jpeg_split_write_kernel(const uint8_t* __restrict__ bytes, const gsr_jpeg_file* __restrict__ files, int nfiles,
                                                                    int nintervals, const JpgeHuffman* __restrict__ huffman, JdWorkspace ws,
                                                                    const int32_t* status, JsTables t, uint32_t B, gsr_jpeg_split_trace* trace)
{
    __shared__ JpgeCode codes[6];
    const int tid = (int)threadIdx.x;
    uint32_t c = 0;
    const int i = js_chunk_interval(blockIdx.x, nintervals, t, &c);
    if (i < 0) return;
    const int f = jd_owner(i, files, nfiles, ws, status);
    if (f < 0) return;
    const gsr_jpeg_file fl = files[f];
    JpsTables use;
    if (!js_build(JdTeam{tid, JS_CHUNK}, codes, use, fl, huffman)) {
        if (tid == 0) t.only[i] = 1;  // the entropy kernel reports the table
        return;
    }
    JsFetch in = js_fetch(bytes, fl);
    const JsPiece p = js_piece(in, fl, i, ws, B);
    const JpsInterval iv = {p.cut, use, p.ny, p.bpm, p.total};
    const uint32_t x = c * JS_CHUNK + (uint32_t)tid;
    if (x >= iv.cut.count) return;
    const uint32_t* entry = t.entry + t.sub_first[i];
    const uint32_t* blocks = t.blocks + t.sub_first[i];
    const uint32_t* first = t.first + t.sub_first[i];
    JsStore store = {(int16_t*)(ws.area + fl.coef_offset) + (size_t)p.first_mcu * (size_t)p.bpm * 64};
    if (!jps_write(in, iv, x, entry, blocks, first, store)) t.only[i] = 1;
    if (trace) {
        const uint32_t begin = jps_begin(in, iv.cut, x);
        JpsState s = {begin, 0, 0, 0, true};
        if (x) s = jps_unpack(entry[x - 1u], begin, iv.bpm);
        gsr_jpeg_split_trace row = {-1, -1, -1, (int32_t)first[x], (int32_t)blocks[x]};
        if (s.ok) {
            uint32_t pairs = t.pairs[t.sub_first[i] + x];
            for (uint32_t at = begin; at < s.byte && at < iv.cut.end; at++) pairs += in(at) == 0xFFu;  // (s.byte - begin < 256)
            row.bit = (int32_t)(8u * (s.byte - iv.cut.start - pairs) + (uint32_t)s.bit);
            row.j = s.j;
            row.k = s.k;
        }
        trace[t.sub_first[i] + x] = row;
    }
}

// ---- dc ----
__global__ void __launch_bounds__(256) jpeg_split_dc_kernel(const gsr_jpeg_file* __restrict__ files, int nfiles, JdWorkspace ws, const int32_t* status, JsTables t)
{
    const int i = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (!t.split[i] || t.only[i]) return;
    const int f = jd_owner(i, files, nfiles, ws, status);
    if (f < 0) return;
    const gsr_jpeg_file fl = files[f];
    const JdGeometry g = jd_geometry(fl);
    const uint32_t first_mcu = jd_piece(fl, g, i, ws).first_mcu, mcus = jd_piece(fl, g, i, ws).mcus;
    int16_t* coef = (int16_t*)(ws.area + fl.coef_offset) + (size_t)first_mcu * (size_t)g.bpm * 64;
    const uint32_t per = (mcus + 255u) / 256u, m0 = (uint32_t)tid * per, m1 = min(mcus, m0 + per);
    uint32_t sum[3] = {0u, 0u, 0u};
    for (uint32_t m = m0; m < m1; m++)
        for (int j = 0; j < g.bpm; j++) sum[jpge_component(j, g.ny)] += (uint32_t)(int32_t)coef[((size_t)m * g.bpm + j) * 64];
    gsr_block_scan_excl<256>(sum);  // (integer sums modulo 2^32: the order of the additions does not show)
    for (uint32_t m = m0; m < m1; m++)
        for (int j = 0; j < g.bpm; j++) {
            int16_t* dc = coef + ((size_t)m * g.bpm + j) * 64;
            uint32_t& pred = sum[jpge_component(j, g.ny)];
            pred += (uint32_t)(int32_t)*dc;
            *dc = (int16_t)(uint16_t)pred;
        }
}

// ---- info ----
__global__ void __launch_bounds__(64) jpeg_split_info_kernel(const gsr_jpeg_file* __restrict__ files, int nfiles, const int32_t* status, JsTables t,
                                                             int32_t* __restrict__ info)
{
    const int f = (int)(blockIdx.x * 64 + threadIdx.x);
    if (f >= nfiles) return;
    int32_t split = 0, repaired = 0, subs = 0, chunks = 0;
    if (status[2 * f] != GSR_JPEG_DECODE_TABLE) {  // (its table entries are sound: validate)
        const gsr_jpeg_file fl = files[f];
        for (int i = fl.first_interval; i < fl.first_interval + fl.intervals; i++)
            if (status[2 * f] == GSR_JPEG_DECODE_OK && t.split[i]) {
                split++;
                repaired += t.only[i] != 0;
                subs += (int32_t)t.count[i];
                chunks += (int32_t)((t.count[i] + JS_CHUNK - 1u) / JS_CHUNK);
            }
    }
    info[4 * f] = split;
    info[4 * f + 1] = repaired;
    info[4 * f + 2] = subs;
    info[4 * f + 3] = chunks;
}

struct JsCall {
    const uint8_t* bytes;
    const gsr_jpeg_file* files;
    int nfiles, nintervals;
    const JpgeHuffman* huffman;
    const int32_t* status;
    JsTables t;
    uint32_t B, min_bytes;
    gsr_jpeg_split_trace* trace;
    int32_t* info;
};
static hipError_t js_launch(void* self, const JdWorkspace& ws, hipStream_t stream)
{
    const JsCall& a = *(const JsCall*)self;
    const uint32_t chunks = (uint32_t)a.t.max_chunks, nint = (uint32_t)a.nintervals, nf = (uint32_t)a.nfiles;
    hipError_t e;
    hipLaunchKernelGGL(jpeg_split_classify_kernel, dim3(1), dim3(1024), 0, stream, a.bytes, a.files, a.nfiles, a.nintervals, ws, a.status, a.t, a.B, a.min_bytes);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_split_sync_kernel, dim3(chunks), dim3(JS_CHUNK), 0, stream, a.bytes, a.files, a.nfiles, a.nintervals, a.huffman, ws, a.status, a.t, a.B);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_split_walk_kernel, dim3(nint), dim3(64), 0, stream, a.bytes, a.files, a.nfiles, a.huffman, ws, a.status, a.t, a.B);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.trace) {
        hipLaunchKernelGGL(jpeg_split_pairs_kernel, dim3(chunks), dim3(JS_CHUNK), 0, stream, a.bytes, a.files, a.nfiles, a.nintervals, ws, a.status, a.t, a.B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(jpeg_split_scan_kernel, dim3(nint), dim3(256), 0, stream, a.t, a.trace ? 1 : 0);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const size_t blocks_each = ws.area_bytes / 192 / (size_t)a.nfiles;  // a file's share of the call, as the idct launch counts it
    hipLaunchKernelGGL(jpeg_split_clear_kernel, dim3((uint32_t)min((size_t)1024, blocks_each / 32 + 1), nf), dim3(256), 0, stream, a.files, ws, a.status, a.t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_split_write_kernel, dim3(chunks), dim3(JS_CHUNK), 0, stream, a.bytes, a.files, a.nfiles, a.nintervals, a.huffman, ws, a.status, a.t, a.B,
                       a.trace);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_split_dc_kernel, dim3(nint), dim3(256), 0, stream, a.files, a.nfiles, ws, a.status, a.t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_split_info_kernel, dim3((nf + 63u) / 64u), dim3(64), 0, stream, a.files, a.nfiles, a.status, a.t, a.info);
    return hipGetLastError();
}

// ---- C entry points (include/gsraster_jpeg_split.h): check the arguments, launch ----
extern "C" size_t gsr_jpeg_split_workspace_bytes(size_t area_bytes, int nfiles, int nintervals, size_t scan_bytes, int subsequence_bytes)
{
    if (scan_bytes >= ((size_t)1 << 32) || !jps_bytes_allowed(subsequence_bytes)) return 0;
    const size_t front = gsr_jpeg_decode_workspace_bytes(area_bytes, nfiles, nintervals);  // (0 for its own reasons)
    return front ? front + js_carve(nullptr, nintervals, scan_bytes, subsequence_bytes).bytes : 0;
}

extern "C" int gsr_jpeg_decode_split(const uint8_t* bytes, size_t nbytes, const gsr_jpeg_file* files, int nfiles, int nintervals, const uint16_t* quant,
                                     int nquant, const gsr_jpeg_huffman* huffman, int nhuffman, uint8_t* out, size_t out_bytes, int32_t* status,
                                     void* workspace, size_t workspace_bytes, int subsequence_bytes, int min_bytes, gsr_jpeg_split_trace* trace,
                                     int32_t* info, void* stream)
{
    if (!bytes || !files || !quant || !huffman || !out || !status || !workspace || !info)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode split: bytes, files, quant, huffman, out, status, workspace or info is NULL");
    if (nfiles <= 0 || nintervals <= 0 || nquant <= 0 || nhuffman <= 0 || nfiles > 65535)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode split: nfiles=%d nintervals=%d nquant=%d nhuffman=%d (need all > 0, nfiles <= 65535)", nfiles,
                        nintervals, nquant, nhuffman);
    if (nbytes >= ((size_t)1 << 32) || out_bytes >= ((size_t)1 << 32))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode split: nbytes=%zu out_bytes=%zu (need both < 2^32)", nbytes, out_bytes);
    if (((uintptr_t)bytes & 15) || ((uintptr_t)out & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)quant & 15) || ((uintptr_t)files & 7) ||
        ((uintptr_t)status & 3) || ((uintptr_t)trace & 3) || ((uintptr_t)info & 3))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode split: bytes, out, workspace and quant are 16-byte aligned, files 8, status, trace and info 4");
    if (!jps_bytes_allowed(subsequence_bytes) || min_bytes < 0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode split: subsequence_bytes=%d min_bytes=%d (need a power of two in 16 .. 1024, min_bytes >= 0)",
                        subsequence_bytes, min_bytes);
    const size_t mine = js_carve(nullptr, nintervals, nbytes, subsequence_bytes).bytes;
    if (workspace_bytes < mine || workspace_bytes - mine < jd_tables_bytes(nintervals))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode split: workspace_bytes=%zu is below the tables' part alone", workspace_bytes);
    // this family's tables at the END of what the caller gave; gsr_jpeg_decode's launcher gets what lies in front of them
    const size_t front = (workspace_bytes - mine) & ~(size_t)15;
    JsCall call = {bytes, files, nfiles, nintervals, (const JpgeHuffman*)huffman, status, js_carve((char*)workspace + front, nintervals, nbytes, subsequence_bytes).t,
                   (uint32_t)subsequence_bytes, (uint32_t)min_bytes, trace, info};
    const JdBetween between = {js_launch, &call, call.t.only};
    GSR_HIP(jpeg_launch_decode(bytes, nbytes, files, nfiles, nintervals, quant, nquant, huffman, nhuffman, out, out_bytes, status, workspace, front,
                               (hipStream_t)stream, &between),
            "jpeg decode split");
    return GSR_OK;
}
