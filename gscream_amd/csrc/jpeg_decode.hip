// jpeg_decode.hip -- the bytes of baseline JPEG files -> uint8 [H, W, C] pictures on the device.  The accepted subset, the tables, the six
// rules and the status codes are in include/gsraster_jpeg_decode.h in full; the entropy core (marker classes, Huffman tables, bit reader,
// interval loop) is jpeg_entropy.h, which the host check program runs under sanitizers over the same corpus.  Six launches per batch,
// nothing read back, no host decision, no global atomics:
//   validate : a one-wave workgroup per file.  Every table entry the later kernels follow is checked against nbytes, out_bytes, the
//              table counts and the workspace, the sizes and sampling against the accepted set, the interval count against the
//              geometry; a file with a bad entry gets GSR_JPEG_DECODE_TABLE and is skipped by everything below.  The file's entries of
//              the interval tables are claimed (owner) and cleared.
//   markers  : a workgroup of 1024 per file walks the scan in pieces of 64 KiB, a thread per run of 64 bytes: the run's RST markers as a
//              bit mask, the first closing marker by an LDS minimum, the markers in front of it compacted in order (gsr_scan.h) into
//              the intervals' [start, end); then count and numbering are checked (jpge_marker_verdict).
//   entropy  : a one-wave workgroup per restart interval.  The wave builds its file's lookup tables in LDS together, then the 64
//              lanes run jpge_interval in lockstep with identical state (the reader's words live in scalar registers); the scan's bytes
//              come through a window of 256 bytes held in registers, a dword per lane, read with v_readlane.  Lane k keeps coefficient k
//              (zigzag) of the block in a register; a finished block is one 128-byte store, natural order.
//   status   : a thread per file: the first failing interval in scan order decides.
//   idct     : 256 threads take 32 blocks: dequantise on load (a row of 8 coefficients per thread, 16 bytes), column pass, LDS, row pass,
//              range limit, 8 samples per thread as one 8-byte store into the component's plane.  Mirrors jpeg.hip's `transform`.
//   colour   : a thread per four pixels of a row: chroma upsampling (rule 5) from the planes, conversion (rule 6), the HWC store, in
//              dwords where the four pixels are whole and aligned.
// The entropy kernel has a second entry behind a per-interval predicate (`only`): gsr_jpeg_decode launches the plain one, all intervals; the split decode
// of jpeg_split.hip runs this file's launcher (jpeg_decode_launch.h) with its own launches between markers and entropy and names the intervals left here.
// idct and colour run a grid of (G, nfiles) with a stride loop inside the file; G comes from the call's averages (the host knows no
// file's size: the tables are device memory).  Integer arithmetic only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_scan.h"
#include "jpeg_decode_launch.h"
#include "jpeg_entropy.h"

static_assert(sizeof(gsr_jpeg_file) == 104, "the file table's layout");
static_assert(sizeof(JpgeHuffman) == sizeof(gsr_jpeg_huffman) && sizeof(gsr_jpeg_huffman) == 272, "the Huffman tables are read as JpgeHuffman");
static_assert(JPGE_OK == GSR_JPEG_DECODE_OK && JPGE_TRUNCATED == GSR_JPEG_DECODE_TRUNCATED && JPGE_RESTART == GSR_JPEG_DECODE_RESTART &&
              JPGE_TABLE == GSR_JPEG_DECODE_TABLE, "one set of status codes");

#define JD_MARK_THREADS 1024
#define JD_RUN 64u         // bytes of the scan per thread and round of the marker walk
#define JD_WINDOW 256u     // bytes of the scan the entropy kernel's wave holds in registers, a dword per lane
#define JD_IDCT_BLOCKS 32  // blocks per round of a 256-thread idct workgroup
#define JD_LDS_ROW 72      // dwords between two blocks in the idct's LDS tiles

// The caller's area of `area_bytes` (rounded up to 16), then per interval {start, end, status, owner}.  The launcher puts the tables at
// the END of what the caller gave: its area is whatever lies in front of them.
struct JdCarve {
    JdWorkspace ws;
    size_t bytes;
};
static JdCarve jd_carve(void* base, size_t area_bytes, int nintervals)
{
    JdCarve r{};
    GsrCarver c(base);
    r.ws.area = c.take<uint8_t>(area_bytes, 16);
    r.ws.area_bytes = c.bytes();
    r.ws.ivl_start = c.take<uint32_t>((size_t)nintervals, 16);
    r.ws.ivl_end = c.take<uint32_t>((size_t)nintervals, 16);
    r.ws.ivl_status = c.take<int32_t>((size_t)nintervals, 16);
    r.ws.ivl_owner = c.take<int32_t>((size_t)nintervals, 16);
    r.bytes = c.total();
    return r;
}
size_t jd_tables_bytes(int nintervals) { return jd_carve(nullptr, 0, nintervals).bytes; }  // the tables' part alone: the least workspace a call is taken with

// ---- validate ----
__global__ void __launch_bounds__(64) jpeg_decode_validate_kernel(const gsr_jpeg_file* __restrict__ files, int nintervals, unsigned long long nbytes,
                                                                  unsigned long long out_bytes, int nquant, int nhuffman, JdWorkspace ws,
                                                                  int32_t* __restrict__ status)
{
    const int f = (int)blockIdx.x, lane = (int)threadIdx.x;
    const gsr_jpeg_file fl = files[f];
    bool ok = fl.H > 0 && fl.W > 0 && fl.H <= 65535 && fl.W <= 65535 && fl.restart_interval >= 0 && fl.restart_interval <= 65535 &&
              ((fl.C == 1 && fl.hs == 1 && fl.vs == 1) || (fl.C == 3 && (fl.hs == 1 || fl.hs == 2) && (fl.vs == 1 || fl.vs == 2) && !(fl.hs == 1 && fl.vs == 2)));
    if (ok) {
        const JdGeometry g = jd_geometry(fl);
        const uint32_t expected = (g.mcus + g.per - 1u) / g.per;
        const unsigned long long picture = (unsigned long long)fl.H * fl.W * fl.C, coef = 128ull * g.blocks, planes = 64ull * g.blocks;
        ok = fl.intervals > 0 && (uint32_t)fl.intervals == expected && fl.first_interval >= 0 &&
             (long long)fl.first_interval + fl.intervals <= (long long)nintervals && fl.scan_offset <= nbytes &&
             (unsigned long long)fl.scan_length <= nbytes - fl.scan_offset && fl.out_offset <= out_bytes && picture <= out_bytes - fl.out_offset &&
             (fl.coef_offset & 15) == 0 && (fl.plane_offset & 15) == 0 && fl.coef_offset <= ws.area_bytes && coef <= ws.area_bytes - fl.coef_offset &&
             fl.plane_offset <= ws.area_bytes && planes <= ws.area_bytes - fl.plane_offset;
        for (int c = 0; c < fl.C; c++)
            ok = ok && fl.quant[c] >= 0 && fl.quant[c] < nquant && fl.dc[c] >= 0 && fl.dc[c] < nhuffman && fl.ac[c] >= 0 && fl.ac[c] < nhuffman;
    }
    if (ok)
        for (int i = lane; i < fl.intervals; i += 64) {
            ws.ivl_owner[fl.first_interval + i] = f;
            ws.ivl_status[fl.first_interval + i] = JPGE_OK;
            ws.ivl_start[fl.first_interval + i] = 0u;
            ws.ivl_end[fl.first_interval + i] = 0u;
        }
    if (lane == 0) {
        status[2 * f] = ok ? GSR_JPEG_DECODE_OK : GSR_JPEG_DECODE_TABLE;
        status[2 * f + 1] = 0;
    }
}

// ---- markers ----
__global__ void __launch_bounds__(JD_MARK_THREADS) jpeg_decode_markers_kernel(const uint8_t* __restrict__ bytes, const gsr_jpeg_file* __restrict__ files,
                                                                              JdWorkspace ws, int32_t* status)
{
    __shared__ uint32_t closing;
    const int f = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (status[2 * f] != GSR_JPEG_DECODE_OK) return;  // (written by the launch before this one: the same value in every thread)
    const gsr_jpeg_file fl = files[f];
    const uint8_t* S = bytes + fl.scan_offset;
    const uint32_t L = fl.scan_length, want = (uint32_t)fl.intervals - 1u;
    uint32_t* starts = ws.ivl_start + fl.first_interval;
    uint32_t* ends = ws.ivl_end + fl.first_interval;
    if (tid == 0) closing = 0xffffffffu;
    __syncthreads();
    uint32_t found = 0;
    int misnumbered = 0;
    for (unsigned long long piece = 0; piece < L; piece += (unsigned long long)JD_MARK_THREADS * JD_RUN) {
        const unsigned long long a = piece + (unsigned long long)tid * JD_RUN;
        // the run's markers: bit i = an RST marker at a + i; the first closing marker goes to the LDS minimum
        unsigned long long rst = 0;
        if (a < L) {
            const uint32_t n = (uint32_t)min((unsigned long long)JD_RUN, (unsigned long long)L - a);
            uint8_t cur = S[a];
            uint32_t mine = 0xffffffffu;
            for (uint32_t i = 0; i < n && a + i + 1 < L; i++) {
                const uint8_t next = S[a + i + 1];
                const int cls = jpge_marker_class(cur, next);
                if (cls == JPGE_RST) rst |= 1ull << i;
                else if (cls == JPGE_CLOSING && mine == 0xffffffffu) mine = (uint32_t)a + i;
                cur = next;
            }
            if (mine != 0xffffffffu) atomicMin(&closing, mine);  // (LDS; a minimum does not depend on the order)
        }
        __syncthreads();
        const uint32_t close = closing;
        if (close != 0xffffffffu) {  // only what lies in front of the closing marker counts
            if (a >= close) rst = 0;
            else if (close - a < 64u) rst &= (1ull << (uint32_t)(close - a)) - 1ull;
        }
        uint32_t total = 0;
        uint32_t k = found + gsr_block_scan_excl<JD_MARK_THREADS>((uint32_t)__popcll(rst), &total);
        for (; rst; rst &= rst - 1ull, k++) {
            const uint32_t at = (uint32_t)a + (uint32_t)__builtin_ctzll(rst);
            if (!jpge_marker_numbered(S[at + 1], k)) misnumbered = 1;
            if (k < want) { ends[k] = at; starts[k + 1] = at + 2u; }
        }
        found += total;
        if (close != 0xffffffffu) break;  // (the same in every thread)
        __syncthreads();  // the scan's LDS words are free again
    }
    misnumbered = __syncthreads_or(misnumbered);
    if (tid == 0) {
        const uint32_t close = closing;
        const int verdict = jpge_marker_verdict(close != 0xffffffffu, found, !misnumbered, (uint32_t)fl.intervals);
        if (verdict == JPGE_OK) ends[want] = close;
        else status[2 * f] = verdict;
    }
}

// ---- entropy ----
// byte `at` of the scan; every lane asks for the same byte.  The wave holds a window of JD_WINDOW bytes in one register per lane (lane l:
// the dword at aligned + base + 4 l), filled by one coalesced load, and a byte comes out of it with v_readlane: no LDS word, no barrier.
// (Measured against a 512-byte LDS window behind two barriers: the entropy launch 2 to 4 % shorter, 6.39 -> 6.25 ms for one 567x1008
// file of 71 intervals.  The bytes are not what the wave waits for: it is one instruction stream per interval, a few hundred dependent
// scalar instructions a symbol.)
struct JdFetch {
    JdScan scan;
    uint32_t base;  // 0xffffffff = nothing loaded
    uint32_t mine;
    int lane;
    __device__ uint8_t operator()(uint32_t at)
    {
        const uint32_t q = at + scan.shift;
        if (base == 0xffffffffu || q - base >= JD_WINDOW) {
            base = q & ~3u;
            mine = scan.dword(base + 4u * (uint32_t)lane);
        }
        const uint32_t d = JPGE_UNIFORM(q - base);  // < JD_WINDOW
        return (uint8_t)((uint32_t)__builtin_amdgcn_readlane((int)mine, (int)(d >> 2)) >> (8u * (d & 3u)));
    }
};
struct JdSink {
    int16_t* out;  // the file's coefficients
    int lane, natural;
    int32_t mine;  // coefficient `lane` (zigzag) of the block being decoded
    __device__ void put(int k, int16_t v) { if (lane == k) mine = v; }
    __device__ void flush(size_t block)
    {
        out[block * 64 + (size_t)natural] = (int16_t)mine;
        mine = 0;
    }
};

__device__ __forceinline__ void jd_entropy_interval(const uint8_t* __restrict__ bytes, const gsr_jpeg_file* __restrict__ files, int nfiles,
                                                    const JpgeHuffman* __restrict__ huffman, JdWorkspace ws, const int32_t* status)
{
    __shared__ JpgeCode codes[6];
    const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int f = (int)JPGE_UNIFORM(jd_owner(i, files, nfiles, ws, status));  // (the lanes hold one state: the scalar registers' from here on)
    if (f < 0) return;
    const gsr_jpeg_file fl = files[f];
    const JdGeometry g = jd_geometry(fl);
    uint32_t slots;
    int rc = JPGE_TABLE;
    if (jd_build(JdTeam{lane, 64}, codes, fl, huffman, slots)) {
        const JpgeCode* use[6];
        for (int e = 0; e < 6; e++) use[e] = &codes[(slots >> (4 * e)) & 7u];
        JdFetch in = {jd_scan(bytes, fl), 0xffffffffu, 0u, lane};
        JdSink sink = {(int16_t*)(ws.area + fl.coef_offset), lane, jpge_natural(lane), 0};
        const JdPiece p = jd_piece(fl, g, i, ws);
        rc = jpge_interval(in, JPGE_UNIFORM(p.start), JPGE_UNIFORM(p.end), !p.last, use, g.ny, g.bpm, p.first_mcu, p.mcus, sink);
    }
    if (lane == 0) ws.ivl_status[i] = rc;
}
__global__ void __launch_bounds__(64) jpeg_decode_entropy_kernel(const uint8_t* __restrict__ bytes, const gsr_jpeg_file* __restrict__ files, int nfiles,
                                                                 const JpgeHuffman* __restrict__ huffman, JdWorkspace ws, const int32_t* status)
{
    jd_entropy_interval(bytes, files, nfiles, huffman, ws, status);
}
// The same kernel behind a per-interval predicate, for the split decode (jpeg_split.hip): only[i] != 0: interval i is this kernel's; the
// workgroup of any other interval reads the word and leaves.  (A kernel of its own: the one above is compiled as it was.)
__global__ void __launch_bounds__(64) jpeg_decode_entropy_only_kernel(const uint8_t* __restrict__ bytes, const gsr_jpeg_file* __restrict__ files, int nfiles,
                                                                      const JpgeHuffman* __restrict__ huffman, JdWorkspace ws, const int32_t* status,
                                                                      const int32_t* __restrict__ only)
{
    if (!only[blockIdx.x]) return;
    jd_entropy_interval(bytes, files, nfiles, huffman, ws, status);
}

// ---- status ----
__global__ void __launch_bounds__(64) jpeg_decode_status_kernel(const gsr_jpeg_file* __restrict__ files, int nfiles, JdWorkspace ws, int32_t* status)
{
    const int f = (int)(blockIdx.x * 64 + threadIdx.x);
    if (f >= nfiles || status[2 * f] != GSR_JPEG_DECODE_OK) return;
    const gsr_jpeg_file fl = files[f];
    int done = 0, rc = JPGE_OK;
    for (; done < fl.intervals && rc == JPGE_OK; done++) rc = ws.ivl_status[fl.first_interval + done];
    status[2 * f] = rc;
    status[2 * f + 1] = rc == JPGE_OK ? done : done - 1;
}

// ---- idct ----
// rule 4's pass over eight values, in place
__device__ __forceinline__ void jd_idct8(int32_t (&x)[8])
{
    int32_t z1 = (x[2] + x[6]) * 4433;
    const int32_t t2 = z1 - x[6] * 15137, t3 = z1 + x[2] * 6270;
    const int32_t t0 = (x[0] + x[4]) * 8192, t1 = (x[0] - x[4]) * 8192;
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int32_t a0 = x[7], a1 = x[5], a2 = x[3], a3 = x[1];
    z1 = a0 + a3;
    int32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
    const int32_t z5 = (z3 + z4) * 9633;
    a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
    x[0] = t10 + a3; x[7] = t10 - a3;
    x[1] = t11 + a2; x[6] = t11 - a2;
    x[2] = t12 + a1; x[5] = t12 - a1;
    x[3] = t13 + a0; x[4] = t13 - a0;
}

// where block b (scan order) of a file lies: its component, and the byte offset of its top left sample among the file's planes, whose
// rows are `pitch` bytes apart
struct JdPlace {
    int comp;
    uint32_t pitch;
    size_t offset;
};
__device__ __forceinline__ JdPlace jd_place(const gsr_jpeg_file& fl, const JdGeometry& g, uint32_t b)
{
    const uint32_t mcu = b / (uint32_t)g.bpm, j = b % (uint32_t)g.bpm, my = mcu / g.mcux, mx = mcu % g.mcux;
    JdPlace p;
    if (j < (uint32_t)g.ny) {
        p.comp = 0;
        p.pitch = g.mcux * 8u * (uint32_t)fl.hs;
        p.offset = (size_t)((my * (uint32_t)fl.vs + j / (uint32_t)fl.hs) * 8u) * p.pitch + (size_t)(mx * (uint32_t)fl.hs + j % (uint32_t)fl.hs) * 8u;
    } else {
        p.comp = (int)j - g.ny + 1;
        p.pitch = g.mcux * 8u;
        p.offset = (size_t)g.mcus * 64u * (size_t)(g.ny + p.comp - 1) + (size_t)(my * 8u) * p.pitch + (size_t)mx * 8u;
    }
    return p;
}

__global__ void __launch_bounds__(256) jpeg_decode_idct_kernel(const gsr_jpeg_file* __restrict__ files, const uint16_t* __restrict__ quant, JdWorkspace ws,
                                                               const int32_t* __restrict__ status)
{
    __shared__ int32_t tile[JD_IDCT_BLOCKS * JD_LDS_ROW];
    const int f = (int)blockIdx.y, tid = (int)threadIdx.x, slot = tid >> 3, line = tid & 7;
    if (status[2 * f] != GSR_JPEG_DECODE_OK) return;
    const gsr_jpeg_file fl = files[f];
    const JdGeometry g = jd_geometry(fl);
    const int16_t* coef = (const int16_t*)(ws.area + fl.coef_offset);
    uint8_t* planes = ws.area + fl.plane_offset;
    int32_t* mine = tile + slot * JD_LDS_ROW;
    for (uint32_t b0 = blockIdx.x * JD_IDCT_BLOCKS; b0 < g.blocks; b0 += gridDim.x * JD_IDCT_BLOCKS) {  // (the same trip count in every thread)
        const uint32_t b = b0 + (uint32_t)slot;
        const bool have = b < g.blocks;
        JdPlace at = {};
        if (have) {
            at = jd_place(fl, g, b);
            // rule 3 on load: row `line` of the block, eight coefficients in 16 bytes, times the table's row
            const uint4 raw = *(const uint4*)(coef + (size_t)b * 64 + (size_t)line * 8);
            const uint4 q = *(const uint4*)(quant + (size_t)fl.quant[at.comp] * 64 + (size_t)line * 8);
            const uint32_t rw[4] = {raw.x, raw.y, raw.z, raw.w}, qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                mine[line * 8 + 2 * i] = (int32_t)(int16_t)(rw[i] & 0xffffu) * (int32_t)(qw[i] & 0xffffu);
                mine[line * 8 + 2 * i + 1] = (int32_t)(int16_t)(rw[i] >> 16) * (int32_t)(qw[i] >> 16);
            }
        }
        __syncthreads();
        int32_t x[8];
        if (have) {  // column `line`
#pragma unroll
            for (int r = 0; r < 8; r++) x[r] = mine[r * 8 + line];
            jd_idct8(x);
        }
        __syncthreads();
        if (have)
#pragma unroll
            for (int r = 0; r < 8; r++) mine[r * 8 + line] = (x[r] + 1024) >> 11;
        __syncthreads();
        if (have) {  // row `line`
#pragma unroll
            for (int c = 0; c < 8; c++) x[c] = mine[line * 8 + c];
            jd_idct8(x);
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                lo |= (uint32_t)min(max(((x[c] + (1 << 17)) >> 18) + 128, 0), 255) << (8 * c);
                hi |= (uint32_t)min(max(((x[c + 4] + (1 << 17)) >> 18) + 128, 0), 255) << (8 * c);
            }
            *(uint2*)(planes + at.offset + (size_t)line * at.pitch) = make_uint2(lo, hi);  // inside the block's 8 x 8 of its plane
        }
        __syncthreads();  // the tile is free again
    }
}

// ---- colour ----
// rule 5: the chroma sample of picture position (y, x) from the used r x n part of a plane
__device__ __forceinline__ int jd_chroma(const uint8_t* __restrict__ p, uint32_t pitch, int hs, int vs, int r, int n, int y, int x)
{
    if (hs == 1) return p[(size_t)y * pitch + x];
    const int i = x >> 1, k = vs == 2 ? y >> 1 : y;
    const uint8_t* row = p + (size_t)k * pitch;
    if (n <= 2) return row[i];
    const int side = (x & 1) ? min(i + 1, n - 1) : max(i - 1, 0);
    if (vs == 2) {
        const uint8_t* other = p + (size_t)((y & 1) ? min(k + 1, r - 1) : max(k - 1, 0)) * pitch;
        const int s = 3 * row[i] + other[i], t = 3 * row[side] + other[side];
        return (3 * s + t + ((x & 1) ? 7 : 8)) >> 4;
    }
    if (x == 0 || x == 2 * n - 1) return row[i];
    return (3 * row[i] + row[side] + ((x & 1) ? 2 : 1)) >> 2;
}

__global__ void __launch_bounds__(256) jpeg_decode_colour_kernel(const gsr_jpeg_file* __restrict__ files, JdWorkspace ws, uint8_t* __restrict__ out,
                                                                 const int32_t* __restrict__ status)
{
    const int f = (int)blockIdx.y;
    if (status[2 * f] != GSR_JPEG_DECODE_OK) return;
    const gsr_jpeg_file fl = files[f];
    const JdGeometry g = jd_geometry(fl);
    const int H = fl.H, W = fl.W, C = fl.C, hs = fl.hs, vs = fl.vs;
    const uint32_t pitch0 = g.mcux * 8u * (uint32_t)hs, pitch1 = g.mcux * 8u;
    const uint8_t* Y = ws.area + fl.plane_offset;
    const uint8_t* Cb = Y + (size_t)g.mcus * 64u * (size_t)g.ny;
    const uint8_t* Cr = Cb + (size_t)g.mcus * 64u;
    uint8_t* P = out + fl.out_offset;
    const int r = (H + vs - 1) / vs, n = (W + hs - 1) / hs;
    const uint32_t groups = ((uint32_t)W + 3u) / 4u, items = groups * (uint32_t)H;  // < 2^30
    for (uint32_t it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const int y = (int)(it / groups), x0 = (int)(it % groups) * 4, count = min(4, W - x0);
        uint8_t px[12] = {};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j >= count) break;
            const int x = x0 + j, luma = Y[(size_t)y * pitch0 + x];
            if (C == 1) { px[j] = (uint8_t)luma; continue; }
            const int cb = jd_chroma(Cb, pitch1, hs, vs, r, n, y, x) - 128, cr = jd_chroma(Cr, pitch1, hs, vs, r, n, y, x) - 128;
            px[3 * j] = (uint8_t)min(max(luma + ((91881 * cr + 32768) >> 16), 0), 255);
            px[3 * j + 1] = (uint8_t)min(max(luma + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
            px[3 * j + 2] = (uint8_t)min(max(luma + ((116130 * cb + 32768) >> 16), 0), 255);
        }
        uint8_t* dst = P + ((size_t)y * W + x0) * C;  // count * C bytes of row y: inside the picture
        if (count == 4 && ((uintptr_t)dst & 3u) == 0) {
            for (int w = 0; w < C; w++)
                ((uint32_t*)dst)[w] = (uint32_t)px[4 * w] | (uint32_t)px[4 * w + 1] << 8 | (uint32_t)px[4 * w + 2] << 16 | (uint32_t)px[4 * w + 3] << 24;
        } else {
            for (int j = 0; j < count * C; j++) dst[j] = px[j];
        }
    }
}

hipError_t jpeg_launch_decode(const uint8_t* bytes, size_t nbytes, const gsr_jpeg_file* files, int nfiles, int nintervals, const uint16_t* quant, int nquant,
                              const gsr_jpeg_huffman* huffman, int nhuffman, uint8_t* out, size_t out_bytes, int32_t* status, void* workspace,
                              size_t workspace_bytes, hipStream_t stream, const JdBetween* between)
{
    const size_t tables = jd_tables_bytes(nintervals);
    if (workspace_bytes < tables) return hipErrorInvalidValue;
    const JdWorkspace ws = jd_carve(workspace, (workspace_bytes - tables) & ~(size_t)15, nintervals).ws;
    hipError_t e;
    hipLaunchKernelGGL(jpeg_decode_validate_kernel, dim3((uint32_t)nfiles), dim3(64), 0, stream, files, nintervals, (unsigned long long)nbytes,
                       (unsigned long long)out_bytes, nquant, nhuffman, ws, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_decode_markers_kernel, dim3((uint32_t)nfiles), dim3(JD_MARK_THREADS), 0, stream, bytes, files, ws, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (between && (e = between->launch(between->self, ws, stream)) != hipSuccess) return e;
    if (between)
        hipLaunchKernelGGL(jpeg_decode_entropy_only_kernel, dim3((uint32_t)nintervals), dim3(64), 0, stream, bytes, files, nfiles, (const JpgeHuffman*)huffman,
                           ws, (const int32_t*)status, between->only);
    else
        hipLaunchKernelGGL(jpeg_decode_entropy_kernel, dim3((uint32_t)nintervals), dim3(64), 0, stream, bytes, files, nfiles, (const JpgeHuffman*)huffman, ws,
                           (const int32_t*)status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_decode_status_kernel, dim3((uint32_t)((nfiles + 63) / 64)), dim3(64), 0, stream, files, nfiles, ws, status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // a file's share of the call: 192 bytes of the area per block, C bytes of `out` per pixel
    const size_t blocks_each = ws.area_bytes / 192 / (size_t)nfiles, bytes_each = out_bytes / (size_t)nfiles;
    const uint32_t g_idct = (uint32_t)min((size_t)4096, blocks_each / JD_IDCT_BLOCKS + 1), g_colour = (uint32_t)min((size_t)4096, bytes_each / 3072 + 1);
    hipLaunchKernelGGL(jpeg_decode_idct_kernel, dim3(g_idct, (uint32_t)nfiles), dim3(256), 0, stream, files, quant, ws, (const int32_t*)status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_decode_colour_kernel, dim3(g_colour, (uint32_t)nfiles), dim3(256), 0, stream, files, (JdWorkspace)ws, out, (const int32_t*)status);
    return hipGetLastError();
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
extern "C" size_t gsr_jpeg_decode_workspace_bytes(size_t area_bytes, int nfiles, int nintervals)
{
    if (nfiles <= 0 || nintervals <= 0 || area_bytes >= ((size_t)1 << 40)) return 0;  // (no accepted size wraps the carve: 2^40 + 2^31 * 16)
    return jd_carve(nullptr, area_bytes, nintervals).bytes;
}

extern "C" int gsr_jpeg_decode(const uint8_t* bytes, size_t nbytes, const gsr_jpeg_file* files, int nfiles, int nintervals, const uint16_t* quant,
                               int nquant, const gsr_jpeg_huffman* huffman, int nhuffman, uint8_t* out, size_t out_bytes, int32_t* status,
                               void* workspace, size_t workspace_bytes, void* stream)
{
    if (!bytes || !files || !quant || !huffman || !out || !status || !workspace)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode: bytes, files, quant, huffman, out, status or workspace is NULL");
    if (nfiles <= 0 || nintervals <= 0 || nquant <= 0 || nhuffman <= 0 || nfiles > 65535)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode: nfiles=%d nintervals=%d nquant=%d nhuffman=%d (need all > 0, nfiles <= 65535)", nfiles,
                        nintervals, nquant, nhuffman);
    if (nbytes >= ((size_t)1 << 32) || out_bytes >= ((size_t)1 << 32))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode: nbytes=%zu out_bytes=%zu (need both < 2^32)", nbytes, out_bytes);
    if (((uintptr_t)bytes & 15) || ((uintptr_t)out & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)quant & 15) || ((uintptr_t)files & 7) ||
        ((uintptr_t)status & 3))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode: bytes, out, workspace and quant are 16-byte aligned, files 8, status 4");
    if (workspace_bytes < jd_tables_bytes(nintervals))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode: workspace_bytes=%zu is below the tables' part alone", workspace_bytes);
    GSR_HIP(jpeg_launch_decode(bytes, nbytes, files, nfiles, nintervals, quant, nquant, huffman, nhuffman, out, out_bytes, status, workspace,
                               workspace_bytes, (hipStream_t)stream, nullptr),
            "jpeg decode");
    return GSR_OK;
}

extern "C" const char* gsr_jpeg_decode_status_name(int code)
{
    static const char* const names[] = {"ok", "truncated", "bit pattern with no symbol", "invalid symbol", "run past coefficient 63",
                                        "restart markers miscounted, misnumbered or misplaced", "table entry out of bounds"};
    return code >= GSR_JPEG_DECODE_OK && code <= GSR_JPEG_DECODE_TABLE ? names[code] : "?";
}
