// png_decode.hip -- the bytes of PNG files -> uint8 [H, W, C] pictures on the device.  The accepted subset, the tables, the segment rule and
// the status codes are in include/gsraster.h ("PNG decoding") in full; the decoder core (bit reader, decode tables, block loop, unfilter
// rule) is png_inflate.h, which the host check program runs under sanitizers over the same corpus.  Seven launches per batch, nothing
// read back, no host decision:
//   validate : a workgroup per file.  Every table entry the later kernels follow is checked against nbytes, out_bytes and the
//              workspace; a file with a bad entry gets GSR_PNG_TABLE and is skipped by everything below.
//   measure  : a one-wave workgroup per piece; those that start a segment of a file of SEVERAL segments decode the segment for its
//              size only (no output, no window) and flag it if it does not stand alone.
//   plan     : a thread per file: no flag -> exclusive scan of the sizes, path "parallel"; a flag -> path "serial".
//   inflate  : a one-wave workgroup per piece.  Parallel path: every segment start decodes its segment to its scanned offset.
//              Serial path (and files of one segment): the file's first segment start decodes the file with all IDATs joined.
//              The 64 lanes run the decoder in lockstep with identical state; literals are stored by lane 0, a match is copied by
//              all lanes, the table fill is strided over the lanes.  The last 32 KiB of output live in LDS: a ring of 64 KiB that is
//              flushed to the stream in dwords every 16 KiB, so a match never reads global memory that the wave wrote.
//   adler    : a workgroup per file: sum d and sum (n - i) d over the stream, coalesced, against the trailer.
//   unfilter : a one-wave workgroup per file.  Lane l owns row r0 + l of a group of 64 rows and runs one pixel behind lane l - 1: the
//              byte above comes from that lane's previous step through one shuffle, the byte above-left is the one before that, the
//              byte to the left is the lane's own last output.  A group is walked in column tiles that are staged into LDS and
//              written back from it with consecutive lanes on consecutive bytes.  Lane 0's row above is the picture's row r0 - 1,
//              which this workgroup wrote one group earlier: it is read after a __syncthreads(), whose workgroup-scope release /
//              acquire fences order the workgroup's global stores before the loads behind the barrier (HIP memory model).
//   crc      : a workgroup per chunk (verify_crc), the slice-combining CRC-32 of png_crc.h against the stored word.
// Integer arithmetic only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_reduce.h"
#include "png_crc.h"
#include "png_inflate.h"

static_assert(sizeof(PngiPiece) == sizeof(gsr_png_piece) && sizeof(gsr_png_piece) == 24, "the piece table is read as PngiPiece");
static_assert(sizeof(gsr_png_file) == 40, "the file table's layout");
static_assert(PNGI_TABLE == GSR_PNG_TABLE && PNGI_CRC == GSR_PNG_CRC && PNGI_TRUNCATED == GSR_PNG_TRUNCATED, "one set of status codes");

#define PD_RING 65536u   // >= the 32 KiB window + PD_FLUSH + one match
#define PD_FLUSH 16384u
#define PD_TB 768        // bytes of a row in an unfilter tile: a multiple of every C
#define PD_ADLER_THREADS 1024
#define PD_CRC_THREADS 256
#define PD_SEG (GSR_PNG_PIECE_IDAT | GSR_PNG_PIECE_START)

struct PdWorkspace {
    uint8_t* streams;
    unsigned long long stream_area;
    uint32_t *seg_size, *seg_flag, *seg_off, *trailer;
};

// The streams' area of `stream_bytes` (rounded up to 16), then the tables: per piece {size, flag, offset} as three arrays in one
// piece, per file the trailer's Adler-32.  The launcher puts the tables at the END of what the caller gave: its stream area is
// whatever lies in front of them.
struct PdCarve {
    PdWorkspace ws;
    size_t bytes;
};
static PdCarve pd_carve(void* base, size_t stream_bytes, int nfiles, int npieces)
{
    PdCarve r{};
    GsrCarver c(base);
    r.ws.streams = c.take<uint8_t>(stream_bytes, 16);
    r.ws.stream_area = c.bytes();
    r.ws.seg_size = c.take<uint32_t>((size_t)npieces * 3, 16);
    r.ws.seg_flag = r.ws.seg_size ? r.ws.seg_size + npieces : nullptr;
    r.ws.seg_off = r.ws.seg_size ? r.ws.seg_flag + npieces : nullptr;
    r.ws.trailer = c.take<uint32_t>((size_t)nfiles, 16);
    r.bytes = c.total();
    return r;
}
static size_t pd_tables_bytes(int nfiles, int npieces) { return pd_carve(nullptr, 0, nfiles, npieces).bytes; }  // the tables' part alone: the least workspace a call is taken with

struct PdTeam {
    int lane, lanes;
    __device__ void sync() { __syncthreads(); }
};

__device__ __forceinline__ unsigned long long pd_stream_bytes(const gsr_png_file& f)
{
    return (unsigned long long)f.H * (1ull + (unsigned long long)f.W * (unsigned long long)f.C);
}
__device__ __forceinline__ void pd_fail(int32_t* status, int f, int code)
{
    atomicCAS((int*)&status[2 * f], 0, code);  // the first code stays
}

// ---- validate ----
__global__ void __launch_bounds__(256) png_validate_kernel(const gsr_png_file* __restrict__ files, int nfiles, const PngiPiece* __restrict__ pieces,
                                                           int npieces, unsigned long long nbytes, unsigned long long out_bytes, PdWorkspace ws,
                                                           int32_t* __restrict__ status)
{
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
    const gsr_png_file fl = files[f];
    bool ok = fl.H > 0 && fl.W > 0 && fl.C >= 1 && fl.C <= 4 && (long long)fl.W * fl.C < (1 << 24) && fl.first_piece >= 0 && fl.piece_count > 0 &&
              (long long)fl.first_piece + fl.piece_count <= (long long)npieces;
    if (ok) {
        const unsigned long long stream = pd_stream_bytes(fl), picture = (unsigned long long)fl.H * fl.W * fl.C;
        ok = stream < 0x70000000ull && (fl.out_offset & 15) == 0 && (fl.stream_offset & 15) == 0 && fl.out_offset <= out_bytes &&
             picture <= out_bytes - fl.out_offset && fl.stream_offset <= ws.stream_area && stream <= ws.stream_area - fl.stream_offset;
    }
    int bad = 0;
    if (ok)
        for (int p = fl.first_piece + tid; p < fl.first_piece + fl.piece_count; p += 256) {
            const PngiPiece pc = pieces[p];
            // the type in front and the CRC behind the data are read too
            if (pc.file != (uint32_t)f || pc.offset < 4 || pc.offset > nbytes || (unsigned long long)pc.length + 4ull > nbytes - pc.offset) bad = 1;
            ws.seg_size[p] = 0u;
            ws.seg_flag[p] = 0u;
            ws.seg_off[p] = 0u;
        }
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        status[2 * f] = (ok && !bad) ? GSR_PNG_OK : GSR_PNG_TABLE;
        status[2 * f + 1] = 0;
        ws.trailer[f] = 0u;
    }
}

// What a one-wave workgroup per piece does first: is piece p the start of a segment of a file that is still sound?  -> the file, the
// segment's pieces [p, end), whether it is the file's first / last segment.
struct PdSegment {
    int f, end, fend;
    bool first, last;
    gsr_png_file file;
};
__device__ __forceinline__ bool pd_segment(const gsr_png_file* files, int nfiles, const PngiPiece* pieces, const int32_t* status, int p, PdSegment& s)
{
    const PngiPiece pc = pieces[p];
    if ((pc.flags & PD_SEG) != PD_SEG || pc.file >= (uint32_t)nfiles) return false;
    s.f = (int)pc.file;
    if (status[2 * s.f] != GSR_PNG_OK) return false;
    s.file = files[s.f];
    s.fend = s.file.first_piece + s.file.piece_count;
    if (p < s.file.first_piece || p >= s.fend) return false;
    s.first = true;
    for (int q = p - 1; q >= s.file.first_piece && s.first; q--) s.first = !(pieces[q].flags & GSR_PNG_PIECE_IDAT);
    s.end = p + 1;
    while (s.end < s.fend && (pieces[s.end].flags & PD_SEG) != PD_SEG) s.end++;
    s.last = s.end == s.fend;
    return true;
}

// ---- measure ----
__global__ void __launch_bounds__(64) png_measure_kernel(const uint8_t* __restrict__ bytes, unsigned long long nbytes, const gsr_png_file* __restrict__ files,
                                                         int nfiles, const PngiPiece* __restrict__ pieces, PdWorkspace ws, const int32_t* status)
{
    __shared__ PngiShared sh;
    __shared__ __attribute__((aligned(16))) uint8_t window[PNGI_WINDOW];  // the reader's staged input
    const int p = (int)blockIdx.x;
    PdSegment s;
    if (!pd_segment(files, nfiles, pieces, status, p, s) || s.file.segments <= 1) return;
    PdTeam tm = {(int)threadIdx.x, 64};
    PngiReader r;
    r.init(bytes, nbytes, pieces, p, s.end, window, (int)threadIdx.x, 64);
    PngiCountSink sink = {0ull, PNGI_UNIFORM64(pd_stream_bytes(s.file))};
    uint32_t trailer = 0;
    const int rc = pngi_inflate(tm, r, sh, sink, (s.first ? PNGI_HEAD : 0) | (s.last ? PNGI_TAIL : 0), &trailer);
    if (threadIdx.x == 0) {
        ws.seg_size[p] = (uint32_t)sink.pos;  // <= the stream's bytes < 2^31
        ws.seg_flag[p] = rc != PNGI_OK ? 1u : 0u;
        if (s.last && rc == PNGI_OK) ws.trailer[s.f] = trailer;
    }
}

// ---- plan ----
__global__ void __launch_bounds__(64) png_plan_kernel(const gsr_png_file* __restrict__ files, int nfiles, const PngiPiece* __restrict__ pieces, PdWorkspace ws,
                                                      int32_t* __restrict__ status)
{
    const int f = (int)(blockIdx.x * 64 + threadIdx.x);
    if (f >= nfiles || status[2 * f] != GSR_PNG_OK) return;
    const gsr_png_file fl = files[f];
    if (fl.segments <= 1) return;  // path 0
    unsigned long long total = 0;
    uint32_t flag = 0;
    for (int p = fl.first_piece; p < fl.first_piece + fl.piece_count; p++) {
        if ((pieces[p].flags & PD_SEG) != PD_SEG) continue;
        flag |= ws.seg_flag[p];
        ws.seg_off[p] = (uint32_t)total;  // used only when total ends equal to the stream's bytes
        total += ws.seg_size[p];
    }
    if (flag) return;  // path 0: the serial decode also names the error, if there is one
    const unsigned long long stream = pd_stream_bytes(fl);
    status[2 * f + 1] = 1;
    if (total != stream) status[2 * f] = total > stream ? GSR_PNG_TOO_LONG : GSR_PNG_TOO_SHORT;
}

// ---- inflate ----
struct PdRingSink {
    uint8_t* ring;  // LDS, PD_RING bytes
    uint8_t* out;   // this decode's first byte in the stream
    uint64_t pos, limit;
    uint32_t flushed;
    int lane;
    __device__ void flush()
    {
        __syncthreads();
        const uint32_t n = (uint32_t)pos - flushed;  // every byte below pos is below limit
        uint8_t* dst = out + flushed;
        const uint32_t head = min(n, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
        if ((uint32_t)lane < head) dst[lane] = ring[(flushed + lane) & (PD_RING - 1u)];
        const uint32_t words = (n - head) >> 2;
        uint32_t* d32 = (uint32_t*)(dst + head);
        for (uint32_t w = (uint32_t)lane; w < words; w += 64u) {
            const uint32_t at = flushed + head + 4u * w;
            d32[w] = (uint32_t)ring[at & (PD_RING - 1u)] | (uint32_t)ring[(at + 1u) & (PD_RING - 1u)] << 8 |
                     (uint32_t)ring[(at + 2u) & (PD_RING - 1u)] << 16 | (uint32_t)ring[(at + 3u) & (PD_RING - 1u)] << 24;
        }
        const uint32_t done = head + 4u * words;
        if ((uint32_t)lane < n - done) dst[done + lane] = ring[(flushed + done + lane) & (PD_RING - 1u)];
        flushed = (uint32_t)pos;
    }
    __device__ bool lit(uint8_t b)
    {
        if (pos >= limit) return false;
        if ((uint32_t)pos - flushed >= PD_FLUSH) flush();
        if (lane == 0) ring[(uint32_t)pos & (PD_RING - 1u)] = b;
        pos++;
        return true;
    }
    // dist <= pos (checked by the caller) and dist <= 32768: the source lies in the ring.  Byte i of the copy is source byte i mod dist,
    // which was written before this match: no lane reads what another writes here.
    __device__ bool match(int len, uint32_t dist)
    {
        if ((uint64_t)len > limit - pos) return false;
        if ((uint32_t)pos - flushed >= PD_FLUSH) flush();
        __syncthreads();  // the bytes before pos are in the ring for every lane
        const uint32_t at = (uint32_t)pos;
        for (uint32_t i = (uint32_t)lane; i < (uint32_t)len; i += 64u) {
            const uint32_t from = dist >= (uint32_t)len ? i : i % dist;
            ring[(at + i) & (PD_RING - 1u)] = ring[(at - dist + from) & (PD_RING - 1u)];
        }
        pos += (uint64_t)len;
        return true;
    }
};

__global__ void __launch_bounds__(64) png_inflate_kernel(const uint8_t* __restrict__ bytes, unsigned long long nbytes, const gsr_png_file* __restrict__ files,
                                                         int nfiles, const PngiPiece* __restrict__ pieces, PdWorkspace ws, int32_t* status)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t pd_ring[];
    __shared__ PngiShared sh;
    __shared__ __attribute__((aligned(16))) uint8_t window[PNGI_WINDOW];  // the reader's staged input
    const int p = (int)blockIdx.x;
    PdSegment s;
    if (!pd_segment(files, nfiles, pieces, status, p, s)) return;
    const bool parallel = s.file.segments > 1 && status[2 * s.f + 1] == 1;
    if (!parallel && !s.first) return;
    PdTeam tm = {(int)threadIdx.x, 64};
    const unsigned long long stream = pd_stream_bytes(s.file);
    PngiReader r;
    PdRingSink sink;
    sink.ring = pd_ring;
    sink.pos = 0;
    sink.flushed = 0;
    sink.lane = (int)threadIdx.x;
    int cover;
    if (parallel) {  // (plan: the offsets and sizes add up to the stream's bytes exactly)
        r.init(bytes, nbytes, pieces, p, s.end, window, (int)threadIdx.x, 64);
        sink.out = ws.streams + PNGI_UNIFORM64(s.file.stream_offset) + PNGI_UNIFORM(ws.seg_off[p]);
        sink.limit = PNGI_UNIFORM(ws.seg_size[p]);
        cover = (s.first ? PNGI_HEAD : 0) | (s.last ? PNGI_TAIL : 0);
    } else {
        r.init(bytes, nbytes, pieces, s.file.first_piece, s.fend, window, (int)threadIdx.x, 64);
        sink.out = ws.streams + PNGI_UNIFORM64(s.file.stream_offset);
        sink.limit = PNGI_UNIFORM64(stream);
        cover = PNGI_HEAD | PNGI_TAIL;
    }
    uint32_t trailer = 0;
    int rc = pngi_inflate(tm, r, sh, sink, cover, &trailer);
    sink.flush();
    if (rc == PNGI_OK && sink.pos < sink.limit) rc = PNGI_TOO_SHORT;
    if (threadIdx.x == 0) {
        if (rc != PNGI_OK) pd_fail(status, s.f, rc > PNGI_TABLE ? PNGI_BAD_SYMBOL : rc);
        else if (!parallel) ws.trailer[s.f] = trailer;
    }
}

// ---- adler ----
__global__ void __launch_bounds__(PD_ADLER_THREADS) png_adler_kernel(const gsr_png_file* __restrict__ files, PdWorkspace ws, int32_t* status)
{
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (status[2 * f] != GSR_PNG_OK) return;  // (written in this kernel only by this workgroup, behind its barrier)
    const gsr_png_file fl = files[f];
    const uint32_t n = (uint32_t)pd_stream_bytes(fl);
    const uint8_t* S = ws.streams + fl.stream_offset;  // 16-byte aligned
    const uint32_t* S32 = (const uint32_t*)S;
    // Adler-32 = (n + sum (n - i) d_i) mod 65521 << 16 | (1 + sum d_i) mod 65521.  A thread's sums: < 2^21 terms of < 2^39.
    unsigned long long A = 0, B = 0;
    for (uint32_t w = (uint32_t)tid; w < n / 4u; w += PD_ADLER_THREADS) {
        const uint32_t v = S32[w], i = 4u * w;
        const uint32_t d0 = v & 255u, d1 = (v >> 8) & 255u, d2 = (v >> 16) & 255u, d3 = v >> 24;
        A += d0 + d1 + d2 + d3;
        B += (unsigned long long)(n - i) * (d0 + d1 + d2 + d3) - (d1 + 2u * d2 + 3u * d3);
    }
    {
        const uint32_t i = (n & ~3u) + (uint32_t)tid;
        if (i < n) { A += S[i]; B += (unsigned long long)(n - i) * S[i]; }
    }
    unsigned long long ab[2] = { A % PNGI_ADLER_MOD, B % PNGI_ADLER_MOD };
    gsr_block_reduce<PD_ADLER_THREADS>(ab, gsr_add());
    if (tid == 0) {
        const uint32_t adler = (uint32_t)((n + ab[1]) % PNGI_ADLER_MOD) << 16 | (uint32_t)((1 + ab[0]) % PNGI_ADLER_MOD);
        if (adler != ws.trailer[f]) pd_fail(status, f, GSR_PNG_ADLER);
    }
}

// ---- unfilter ----
__global__ void __launch_bounds__(64) png_unfilter_kernel(const gsr_png_file* __restrict__ files, PdWorkspace ws, uint8_t* out, int32_t* status)
{
    __shared__ uint8_t tile[64][PD_TB];
    __shared__ uint8_t uprow[PD_TB + 4];
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (status[2 * f] != GSR_PNG_OK) return;  // (one wave: the same value in every lane)
    const gsr_png_file fl = files[f];
    const int H = fl.H, W = fl.W, C = fl.C, tpix = PD_TB / C;
    const size_t wc = (size_t)W * (size_t)C, rowb = wc + 1;
    const uint8_t* S = ws.streams + fl.stream_offset;
    uint8_t* P = out + fl.out_offset;
    for (int r0 = 0; r0 < H; r0 += 64) {
        const int rows = min(64, H - r0);
        const bool have = lane < rows;
        const int type = have ? (int)S[(size_t)(r0 + lane) * rowb] : 0;
        if (__syncthreads_or(type > 4 ? 1 : 0)) {
            if (lane == 0) pd_fail(status, f, GSR_PNG_FILTER);
            return;
        }
        uint32_t left = 0;  // the lane's pixel in front of the tile, a byte per channel
        for (int x0 = 0; x0 < W; x0 += tpix) {
            const int npx = min(tpix, W - x0), nb = npx * C;
            const size_t b0 = (size_t)x0 * (size_t)C;
            __syncthreads();  // the tile's last readers are done; the picture rows this workgroup wrote are visible to its loads
            for (int rr = 0; rr < rows; rr++) {
                const uint8_t* src = S + (size_t)(r0 + rr) * rowb + 1 + b0;
                for (int j = lane; j < nb; j += 64) tile[rr][j] = src[j];
            }
            for (int j = lane; j < nb + C; j += 64)  // the row above the group, from one pixel in front of the tile
                uprow[j] = (r0 > 0 && b0 + (size_t)j >= (size_t)C) ? P[(size_t)(r0 - 1) * wc + b0 + (size_t)j - (size_t)C] : (uint8_t)0;
            __syncthreads();
            uint32_t a = left, prev = 0;
            uint32_t c = (uint32_t)__shfl_up((int)left, 1, 64);
            if (lane == 0) {
                c = 0;
                for (int k = 0; k < C; k++) c |= (uint32_t)uprow[k] << (8 * k);
            }
            for (int t = 0; t < npx + 63; t++) {
                uint32_t b = (uint32_t)__shfl_up((int)prev, 1, 64);
                const int x = t - lane;
                if (have && x >= 0 && x < npx) {
                    uint8_t* px = &tile[lane][x * C];
                    if (lane == 0) {
                        b = 0;
                        for (int k = 0; k < C; k++) b |= (uint32_t)uprow[C + x * C + k] << (8 * k);
                    }
                    uint32_t o = 0;
                    for (int k = 0; k < C; k++) {
                        const int v = pngi_unfilter(type, px[k], (int)((a >> (8 * k)) & 255u), (int)((b >> (8 * k)) & 255u), (int)((c >> (8 * k)) & 255u));
                        px[k] = (uint8_t)v;
                        o |= (uint32_t)v << (8 * k);
                    }
                    c = b;
                    a = o;
                    prev = o;
                }
            }
            left = a;
            __syncthreads();
            for (int rr = 0; rr < rows; rr++) {
                uint8_t* dst = P + (size_t)(r0 + rr) * wc + b0;
                for (int j = lane; j < nb; j += 64) dst[j] = tile[rr][j];
            }
        }
    }
}

// ---- crc ----
__global__ void __launch_bounds__(PD_CRC_THREADS) png_crc_kernel(const uint8_t* __restrict__ bytes, const gsr_png_file* __restrict__ files, int nfiles,
                                                                 const PngiPiece* __restrict__ pieces, int32_t* status)
{
    __shared__ uint32_t tab[256];
    const int p = (int)blockIdx.x, tid = (int)threadIdx.x;
    const PngiPiece pc = pieces[p];
    if (pc.file >= (uint32_t)nfiles) return;
    const gsr_png_file fl = files[pc.file];
    // (GSR_PNG_TABLE is final since the validate kernel: a file that has it keeps it, and only then may this piece be unchecked)
    if (status[2 * pc.file] == GSR_PNG_TABLE || p < fl.first_piece || p >= fl.first_piece + fl.piece_count) return;
    tab[tid] = png_crc_table_entry((uint32_t)tid);
    __syncthreads();
    const uint8_t* src = bytes + pc.offset - 4;  // type, data
    const uint32_t N = 4u + pc.length, per = (N + PD_CRC_THREADS - 1) / PD_CRC_THREADS;
    const uint32_t lo = min(N, (uint32_t)tid * per), hi = min(N, lo + per);
    uint32_t r = 0;
    for (uint32_t i = lo; i < hi; i++) r = tab[(r ^ src[i]) & 0xffu] ^ (r >> 8);
    uint32_t crc = hi > lo ? png_gf2_mul(r, png_x8n(N - hi)) : 0u;
    if (tid == 0) crc ^= png_gf2_mul(0xffffffffu, png_x8n(N));
    crc = gsr_block_reduce<PD_CRC_THREADS>(crc, gsr_xor());
    if (tid == 0) {
        crc ^= 0xffffffffu;
        const uint8_t* q = src + N;
        const uint32_t stored = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | (uint32_t)q[3];
        if (crc != stored) pd_fail(status, (int)pc.file, GSR_PNG_CRC);
    }
}

static hipError_t png_launch_decode(const uint8_t* bytes, size_t nbytes, const gsr_png_file* files, int nfiles, const gsr_png_piece* pieces, int npieces,
                                    int verify_crc, uint8_t* out, size_t out_bytes, int32_t* status, void* workspace, size_t workspace_bytes,
                                    hipStream_t stream)
{
    const size_t tables = pd_tables_bytes(nfiles, npieces);
    if (workspace_bytes < tables) return hipErrorInvalidValue;
    const PdWorkspace ws = pd_carve(workspace, (workspace_bytes - tables) & ~(size_t)15, nfiles, npieces).ws;
    static thread_local uint64_t done_mask = 0;  // the ring and the tables are beyond 64 KiB of LDS: a one-time opt-in per device
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!(dev >= 0 && dev < 64 && ((done_mask >> dev) & 1))) {
        e = hipFuncSetAttribute((const void*)png_inflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PD_RING);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) done_mask |= 1ull << dev;
    }
    const PngiPiece* pc = (const PngiPiece*)pieces;
    hipLaunchKernelGGL(png_validate_kernel, dim3((uint32_t)nfiles), dim3(256), 0, stream, files, nfiles, pc, npieces, (unsigned long long)nbytes,
                       (unsigned long long)out_bytes, ws, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(png_measure_kernel, dim3((uint32_t)npieces), dim3(64), 0, stream, bytes, (unsigned long long)nbytes, files, nfiles, pc, ws,
                       (const int32_t*)status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(png_plan_kernel, dim3((uint32_t)((nfiles + 63) / 64)), dim3(64), 0, stream, files, nfiles, pc, ws, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(png_inflate_kernel, dim3((uint32_t)npieces), dim3(64), PD_RING, stream, bytes, (unsigned long long)nbytes, files, nfiles, pc, ws,
                       status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(png_adler_kernel, dim3((uint32_t)nfiles), dim3(PD_ADLER_THREADS), 0, stream, files, ws, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((uint32_t)nfiles), dim3(64), 0, stream, files, ws, out, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (verify_crc) {
        hipLaunchKernelGGL(png_crc_kernel, dim3((uint32_t)npieces), dim3(PD_CRC_THREADS), 0, stream, bytes, files, nfiles, pc, status);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
extern "C" size_t gsr_png_decode_workspace_bytes(size_t stream_bytes, int nfiles, int npieces)
{
    if (nfiles <= 0 || npieces <= 0 || stream_bytes >= ((size_t)1 << 40)) return 0;  // (no accepted size wraps the carve: 2^40 + 2^31 * 12 + 2^31 * 4)
    return pd_carve(nullptr, stream_bytes, nfiles, npieces).bytes;
}

extern "C" int gsr_png_decode(const uint8_t* bytes, size_t nbytes, const gsr_png_file* files, int nfiles, const gsr_png_piece* pieces, int npieces,
                              int verify_crc, uint8_t* out, size_t out_bytes, int32_t* status, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!bytes || !files || !pieces || !out || !status || !workspace)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png decode: bytes, files, pieces, out, status or workspace is NULL");
    if (nfiles <= 0 || npieces <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png decode: nfiles=%d npieces=%d (need both > 0)", nfiles, npieces);
    if (nbytes >= ((size_t)1 << 32) || out_bytes >= ((size_t)1 << 32))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png decode: nbytes=%zu out_bytes=%zu (need both < 2^32)", nbytes, out_bytes);
    if (((uintptr_t)bytes & 15) || ((uintptr_t)out & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)files & 7) || ((uintptr_t)pieces & 7) ||
        ((uintptr_t)status & 3))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png decode: bytes, out and workspace are 16-byte aligned, the tables 8, status 4");
    if (workspace_bytes < pd_tables_bytes(nfiles, npieces))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png decode: workspace_bytes=%zu is below the tables' part alone", workspace_bytes);
    GSR_HIP(png_launch_decode(bytes, nbytes, files, nfiles, pieces, npieces, verify_crc, out, out_bytes, status, workspace, workspace_bytes,
                              (hipStream_t)stream),
            "png decode");
    return GSR_OK;
}
