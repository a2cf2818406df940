// png.hip -- the last stage of render_set on the device: finished uint8 pictures -> PNG files, byte for byte what goes to disk.  The
// format rules are in include/gsraster.h ("PNG encoding") in full.  Three launches per batch, nothing read back, no host stop, no
// dependency between workgroups, every loop bounded by a compile-time constant or an argument:
//   filter   : one workgroup per row.  Pass 1 (adaptive only) sums |signed residual| of the five filter types and takes the smallest
//              (ties: the lowest type); pass 2 writes the filter byte and the residuals to the filtered stream S and the row's Adler-32
//              partial {sum d, sum (n - i) d} mod 65521.  The picture is read through its row stride: a panel of a wider sheet is
//              read in place.
//   deflate  : one workgroup of 1024 per GSR_PNG_CHUNK bytes of S, staged in LDS.  A thread owns 32 consecutive bytes: it finds its run
//              heads as a bit mask, two block-wide max scans hand it the run that reaches into its span and the first head behind it,
//              and a walk over its (at most 32) run segments yields the tokens of the greedy rule -- first in the histogram, then
//              as bit lengths (block scan -> bit offsets), then as bits ORed into an LDS image of the block.  Between the first and
//              the second walk the 286 used symbols are ranked by frequency by all threads, and thread 0 runs the two-queue Huffman
//              merge, the length limit (fold to 15, then move codes down until the Kraft sum is exactly 1), the canonical codes, the
//              code-length sequence with its repeat symbols, the 19-symbol code (limit 7) and the block header, and counts the
//              block's bits exactly: dynamic or stored, whichever is shorter.  The chunk's bytes go to its slot of the workspace.
//   assemble : one workgroup per IDAT.  File offset = 33 + the sizes of the chunks before it; length, type and data are written with
//              whole dwords where the destination allows; the CRC-32 is lane-parallel (a slice per thread through an LDS table from
//              a zero state, times x^(8 * bytes behind the slice) mod P, XORed over the workgroup, plus the initial state's term).
//              The first workgroup also writes the signature and IHDR, the last one the Adler-32 (row partials combined in order),
//              IEND and the header words.
// Integer arithmetic only; the same input gives the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_scan.h"
#include "png_crc.h"

#define PNG_CHUNK GSR_PNG_CHUNK
#define PNG_FLT_THREADS 256
#define PNG_DEF_THREADS 1024
#define PNG_ASM_THREADS 256
#define PNG_PER (PNG_CHUNK / PNG_DEF_THREADS)  // bytes of a chunk a deflate thread owns
#define PNG_ADLER 65521u
#define PNG_LITLEN 286
#define PNG_SLOT_BYTES (GSR_PNG_CHUNK + 32)
static_assert(PNG_PER == 32, "a thread's run heads are one 32-bit mask, and at most one 258-byte match starts in its span");
static_assert(PNG_SLOT_BYTES >= PNG_CHUNK + 2 + 5 + 5 + 4 && PNG_SLOT_BYTES % 16 == 0, "zlib header, stored header, marker, one dword of slack");

// ---- layout of the workspace (per picture; every part a multiple of 16 bytes) ----
// The workspace holds, per picture, the filtered stream, the rows' Adler-32 partials (two words each), the chunks' byte counts and one
// slot of PNG_SLOT_BYTES per chunk (the chunk's deflate bytes).
struct PngLayout {
    size_t row_bytes, stream_bytes, chunks;             // 1 + W*C, H * row_bytes, ceil(stream_bytes / GSR_PNG_CHUNK)
    size_t adler_off, sizes_off, slots_off, per_picture;  // byte offsets inside a picture's part of the workspace, and its size
    size_t capacity;                                    // what a file can take at most (every chunk stored)
};
static PngLayout png_layout(int H, int W, int C)
{
    PngLayout l;
    l.row_bytes = 1 + (size_t)W * (size_t)C;
    l.stream_bytes = (size_t)H * l.row_bytes;
    l.chunks = (l.stream_bytes + PNG_CHUNK - 1) / PNG_CHUNK;
    GsrCarver c(nullptr);  // offsets only: the kernels add them to the start of the picture's part
    c.skip(l.stream_bytes, 16);
    l.adler_off = c.bytes(); c.skip((size_t)H * 8, 16);
    l.sizes_off = c.bytes(); c.skip(l.chunks * 4, 16);
    l.slots_off = c.bytes(); c.skip(l.chunks * PNG_SLOT_BYTES, 16);
    l.per_picture = c.total();
    // signature, IHDR, per chunk {length, type, CRC, stored header, marker}, the stream, zlib header, Adler-32, IEND
    l.capacity = 8 + 25 + l.chunks * (12 + 5 + 5) + l.stream_bytes + 2 + 4 + 12;
    return l;
}

// ---- filter ----
__device__ __forceinline__ int png_predict(int type, int a, int b, int c)
{
    if (type == 0) return 0;
    if (type == 1) return a;
    if (type == 2) return b;
    if (type == 3) return (a + b) >> 1;
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__global__ void __launch_bounds__(PNG_FLT_THREADS) png_filter_kernel(const uint8_t* __restrict__ images, long long row_stride, long long image_stride,
                                                                     int WC, int C, int filter, uint8_t* __restrict__ ws, PngLayout lay)
{
    __shared__ uint32_t red[5][PNG_FLT_THREADS / 64];
    __shared__ unsigned long long red64[2][PNG_FLT_THREADS / 64];
    const int y = (int)blockIdx.x, b = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* row = images + (long long)b * image_stride + (long long)y * row_stride;
    const uint8_t* up = row - row_stride;  // read only when y > 0
    int type = filter;
    if (filter == GSR_PNG_FILTER_ADAPTIVE) {
        uint32_t s[5] = {0u, 0u, 0u, 0u, 0u};
        for (int x = tid; x < WC; x += PNG_FLT_THREADS) {
            const int cur = row[x], a = x >= C ? row[x - C] : 0, bb = y > 0 ? up[x] : 0, c = (x >= C && y > 0) ? up[x - C] : 0;
#pragma unroll
            for (int t = 0; t < 5; t++) {
                const int r = (cur - png_predict(t, a, bb, c)) & 255;
                s[t] += (uint32_t)(r < 128 ? r : 256 - r);
            }
        }
#pragma unroll
        for (int t = 0; t < 5; t++) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s[t] += (uint32_t)__shfl_xor((int)s[t], d, 64);
            if (lane == 0) red[t][wave] = s[t];
        }
        __syncthreads();
        uint32_t best = 0xffffffffu;
        type = 0;
#pragma unroll
        for (int t = 0; t < 5; t++) {
            uint32_t tot = 0;
#pragma unroll
            for (int w = 0; w < PNG_FLT_THREADS / 64; w++) tot += red[t][w];
            if (tot < best) { best = tot; type = t; }  // ties: the lowest type
        }
    }
    const unsigned long long n = lay.row_bytes;
    uint8_t* S = ws + (size_t)b * lay.per_picture + (size_t)y * lay.row_bytes;
    unsigned long long A = 0, Bs = 0;
    if (tid == 0) {
        S[0] = (uint8_t)type;
        A = (unsigned long long)type;
        Bs = n * (unsigned long long)type;
    }
    for (int x = tid; x < WC; x += PNG_FLT_THREADS) {
        const int cur = row[x], a = x >= C ? row[x - C] : 0, bb = y > 0 ? up[x] : 0, c = (x >= C && y > 0) ? up[x - C] : 0;
        const uint32_t r = (uint32_t)((cur - png_predict(type, a, bb, c)) & 255);
        S[1 + x] = (uint8_t)r;
        A += r;
        Bs += (n - 1ull - (unsigned long long)x) * r;  // n < 2^25: a thread's sum stays below 2^58
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        A += __shfl_xor(A, d, 64);
        Bs += __shfl_xor(Bs, d, 64);
    }
    if (lane == 0) { red64[0][wave] = A; red64[1][wave] = Bs; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long ta = 0, tb = 0;
        for (int w = 0; w < PNG_FLT_THREADS / 64; w++) { ta += red64[0][w]; tb += red64[1][w] % PNG_ADLER; }
        uint32_t* adler = (uint32_t*)(ws + (size_t)b * lay.per_picture + lay.adler_off);
        adler[2 * y] = (uint32_t)(ta % PNG_ADLER);
        adler[2 * y + 1] = (uint32_t)(tb % PNG_ADLER);
    }
}

// ---- deflate ----
// length 3 .. 258 -> (symbol 257 .. 285, number of extra bits, their value)
__device__ __forceinline__ void png_length_code(int len, int& sym, int& ebits, uint32_t& evalue)
{
    const int l = len - 3;
    if (len == 258) { sym = 285; ebits = 0; evalue = 0u; return; }
    if (l < 8) { sym = 257 + l; ebits = 0; evalue = 0u; return; }
    const int e = 29 - __clz(l);  // floor(log2 l) - 2
    sym = 261 + 4 * e + ((l >> e) & 3);
    ebits = e;
    evalue = (uint32_t)l & ((1u << e) - 1u);
}
// extra bits of a length symbol
__device__ __forceinline__ int png_symbol_extra(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

// The tokens that START in a thread's span [s0, s0 + cnt) of the chunk, in order.  heads: bit j = byte s0 + j differs from its
// predecessor (or is the chunk's first); carried: the head of the run that reaches into the span; after: the first head behind the
// span (the chunk's length when there is none).  A segment [a, b) of the span lies in one run [rs, re) of value v: the run's first
// byte is a literal, its R = re - rs - 1 repeats are cut into blocks of 258; a block of >= 3 is one match, a shorter one literals.
// At most one block starts in a segment (258 > 32), and a segment with a match has no short block.
template <typename Lit, typename Match>
__device__ __forceinline__ void png_walk(const uint8_t* data, int s0, int cnt, uint32_t heads, int carried, int after, Lit lit, Match match)
{
    int rs = carried;
    for (int j = 0; j < cnt;) {  // at most PNG_PER segments
        if ((heads >> j) & 1u) rs = s0 + j;
        const uint32_t above = j < 31 ? heads >> (j + 1) : 0u;
        const int nxt = above ? j + __ffs((int)above) : cnt;
        const int re = above ? s0 + nxt : after;
        const int a = s0 + j, b = s0 + nxt;
        const uint32_t v = data[rs];
        if (a == rs) lit(v, 1);
        const int R = re - rs - 1;
        const int k0 = max(a, rs + 1) - rs - 1, k1 = b - rs - 1;  // the repeats [k0, k1) of the run lie in the segment
        if (k1 > k0) {
            const int ks = ((k0 + 257) / 258) * 258;  // the first block start at or behind k0
            if (ks < k1 && R - ks >= 3) match(min(258, R - ks));
            else {
                const int tail = (R / 258) * 258;
                const int lo = max(k0, tail), hi = min(k1, R);
                if (R - tail < 3 && hi > lo) lit(v, hi - lo);
            }
        }
        j = nxt;
    }
}

struct PngBits {  // a thread's contiguous bits, ORed into the LDS image a dword at a time
    uint32_t* out;
    unsigned long long acc;
    uint32_t word;
    int nb;
    __device__ __forceinline__ PngBits(uint32_t* o, uint32_t pos) : out(o), acc(0ull), word(pos >> 5), nb((int)(pos & 31u)) {}
    __device__ __forceinline__ void put(uint32_t v, int n)  // n <= 32
    {
        acc |= (unsigned long long)v << nb;
        nb += n;
        if (nb >= 32) {
            atomicOr(&out[word], (uint32_t)acc);
            acc >>= 32;
            nb -= 32;
            word++;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (acc) atomicOr(&out[word], (uint32_t)acc);
    }
    __device__ __forceinline__ uint32_t pos() const { return word * 32u + (uint32_t)nb; }
};

struct PngShared {
    uint32_t hist[288];    // literal / length frequencies
    uint32_t code[288];    // bit-reversed code | length << 16
    uint32_t nf[288];      // weights of the merge's internal nodes
    uint16_t order[288];   // used symbols, ascending (frequency, symbol)
    uint16_t lpar[288];    // parent of the leaf order[i]
    uint16_t npar[288];    // parent of an internal node
    uint16_t ndepth[288];  // depth of an internal node
    uint16_t cltok[320];   // the code-length sequence: symbol | extra value << 8
    uint8_t lens[320];     // code lengths: literal / length [0, hlit), then the distance code's
    uint32_t clhist[19], clcode[19];
    uint16_t clorder[19];
    uint8_t cllen[19];
    uint32_t cnt[16], next[16];
    uint32_t wtot[2][PNG_DEF_THREADS / 64];
    uint32_t used, matches, ncl, dynamic, bitpos;
};

// Thread 0.  order[0, m): the used symbols ascending by (freq, symbol), m >= 2 -> lens[sym] <= maxlen with a Kraft sum of exactly 1.
__device__ void png_huffman_lengths(PngShared& sh, const uint16_t* order, int m, const uint32_t* freq, int maxlen, uint8_t* lens)
{
    int a = 0, b = 0;
    for (int k = 0; k < m - 1; k++) {  // two-queue merge: leaves in order, internal nodes in the order they were made
        uint32_t sum = 0;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const bool leaf = a < m && (b >= k || freq[order[a]] <= sh.nf[b]);
            if (leaf) { sum += freq[order[a]]; sh.lpar[a++] = (uint16_t)k; }
            else { sum += sh.nf[b]; sh.npar[b++] = (uint16_t)k; }
        }
        sh.nf[k] = sum;
    }
    sh.ndepth[m - 2] = 0;
    for (int k = m - 3; k >= 0; k--) sh.ndepth[k] = (uint16_t)(sh.ndepth[sh.npar[k]] + 1);
    for (int i = 0; i < 16; i++) sh.cnt[i] = 0;
    for (int i = 0; i < m; i++) sh.cnt[min((int)sh.ndepth[sh.lpar[i]] + 1, maxlen)]++;
    // the limit: deeper leaves were folded to maxlen, which over-subscribes the code by < m units of 2^-maxlen; each step takes one
    // unit back by lengthening one code of the deepest length below maxlen and pairing a maxlen code with it
    uint32_t total = 0;
    for (int i = 1; i <= maxlen; i++) total += sh.cnt[i] << (maxlen - i);
    for (int it = 0; it < 288 && total != (1u << maxlen); it++) {
        sh.cnt[maxlen]--;
        for (int i = maxlen - 1; i > 0; i--)
            if (sh.cnt[i]) { sh.cnt[i]--; sh.cnt[i + 1] += 2; break; }
        total--;
    }
    int at = 0;
    for (int l = maxlen; l >= 1; l--)  // the rarest symbols take the longest codes
        for (uint32_t c = 0; c < sh.cnt[l]; c++) lens[order[at++]] = (uint8_t)l;
}

// Thread 0.  Canonical codes (RFC 1951 3.2.2) of lens[0, n), bit-reversed for an LSB-first writer -> code[sym] = rev | len << 16.
__device__ void png_canonical(PngShared& sh, const uint8_t* lens, int n, int maxlen, uint32_t* code)
{
    for (int i = 0; i < 16; i++) sh.cnt[i] = 0;
    for (int s = 0; s < n; s++) sh.cnt[lens[s]]++;
    sh.cnt[0] = 0;
    uint32_t c = 0;
    for (int l = 1; l <= maxlen; l++) { c = (c + sh.cnt[l - 1]) << 1; sh.next[l] = c; }
    for (int s = 0; s < n; s++) {
        const uint32_t l = lens[s];
        code[s] = l ? ((__brev(sh.next[l]++) >> (32 - l)) | (l << 16)) : 0u;
    }
}

__device__ __forceinline__ void png_block_scan_max2(uint32_t& a, uint32_t& b, uint32_t (&wtot)[2][PNG_DEF_THREADS / 64])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = gsr_wave_scan_max(a);
    b = gsr_wave_scan_max(b);
    if (lane == 63) { wtot[0][wave] = a; wtot[1][wave] = b; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < PNG_DEF_THREADS / 64; w++) {
        a = max(a, w < wave ? wtot[0][w] : 0u);
        b = max(b, w < wave ? wtot[1][w] : 0u);
    }
}

__constant__ uint8_t png_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__global__ void __launch_bounds__(PNG_DEF_THREADS) png_deflate_kernel(uint8_t* __restrict__ ws, PngLayout lay)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t png_lds[];
    __shared__ PngShared sh;
    uint8_t* data = png_lds;                                   // [PNG_CHUNK]
    uint32_t* out = (uint32_t*)(png_lds + PNG_CHUNK);          // [PNG_SLOT_BYTES / 4]: the chunk's bytes as they leave
    const int k = (int)blockIdx.x, b = (int)blockIdx.y, tid = (int)threadIdx.x;
    uint8_t* base = ws + (size_t)b * lay.per_picture;
    const size_t start = (size_t)k * PNG_CHUNK;
    const int n = lay.stream_bytes - start < (size_t)PNG_CHUNK ? (int)(lay.stream_bytes - start) : PNG_CHUNK;  // >= 1
    const bool final = k == (int)lay.chunks - 1;
    const int pre = k == 0 ? 2 : 0;  // the zlib header 78 01 leads the first chunk

    // stage the chunk (whole 16-byte pieces: the stream's part of the workspace is rounded up to 16), clear the image and the tables
    for (int i = tid; i * 16 < n; i += PNG_DEF_THREADS) ((uint4*)data)[i] = ((const uint4*)(base + start))[i];
    for (int i = tid; i < PNG_SLOT_BYTES / 4; i += PNG_DEF_THREADS) out[i] = 0u;
    for (int i = tid; i < 288; i += PNG_DEF_THREADS) { sh.hist[i] = 0u; sh.code[i] = 0u; }
    for (int i = tid; i < 320; i += PNG_DEF_THREADS) sh.lens[i] = 0;
    if (tid < 19) { sh.clhist[tid] = 0u; sh.cllen[tid] = 0; }
    if (tid == 0) { sh.used = 0u; sh.matches = 0u; }
    __syncthreads();

    // run heads of the thread's span
    const int s0 = tid * PNG_PER, cnt = min(PNG_PER, n - s0);
    uint32_t heads = 0u;
    if (cnt > 0) {
        const uint4 q0 = ((const uint4*)data)[2 * tid], q1 = ((const uint4*)data)[2 * tid + 1];
        const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        uint32_t prev = tid > 0 ? (uint32_t)data[s0 - 1] << 24 : 0u;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t diff = w[j] ^ ((w[j] << 8) | (prev >> 24));
#pragma unroll
            for (int i = 0; i < 4; i++) heads |= ((diff >> (8 * i)) & 0xffu) ? 1u << (4 * j + i) : 0u;
            prev = w[j];
        }
        if (tid == 0) heads |= 1u;
        if (cnt < 32) heads &= (1u << cnt) - 1u;
    }
    // the last head at or before each thread's span (+ 1; 0 = none), and, scanning the threads in reverse, the first head behind it
    // (as n - position; 0 = none)
    uint32_t* rev = out;  // [PNG_DEF_THREADS], cleared again below
    if (heads) rev[PNG_DEF_THREADS - 1 - tid] = (uint32_t)(n - (s0 + __ffs((int)heads) - 1));
    __syncthreads();
    uint32_t lastp = heads ? (uint32_t)(s0 + 32 - __clz((int)heads)) : 0u, firstp = rev[tid];
    png_block_scan_max2(lastp, firstp, sh.wtot);
    uint32_t* fwd = out + PNG_DEF_THREADS;
    __syncthreads();
    fwd[tid] = lastp;
    rev[tid] = firstp;
    __syncthreads();
    const int carried = tid > 0 ? (int)fwd[tid - 1] - 1 : 0;
    const int after = n - (tid < PNG_DEF_THREADS - 1 ? (int)rev[PNG_DEF_THREADS - 2 - tid] : 0);
    __syncthreads();
    fwd[tid] = 0u;
    rev[tid] = 0u;

    // walk 1: the histogram
    png_walk(data, s0, cnt, heads, carried, after,
             [&](uint32_t v, int c) { atomicAdd(&sh.hist[v], (uint32_t)c); },
             [&](int len) {
                 int sym, eb;
                 uint32_t ev;
                 png_length_code(len, sym, eb, ev);
                 atomicAdd(&sh.hist[sym], 1u);
                 atomicAdd(&sh.matches, 1u);
             });
    if (tid == 0) sh.hist[256] = 1u;
    __syncthreads();

    // rank the used symbols by (frequency, symbol)
    if (tid < PNG_LITLEN) {
        const uint32_t f = sh.hist[tid];
        if (f) {
            int rank = 0;
            for (int j = 0; j < PNG_LITLEN; j++) {
                const uint32_t g = sh.hist[j];
                rank += (g && (g < f || (g == f && j < tid))) ? 1 : 0;
            }
            sh.order[rank] = (uint16_t)tid;
            atomicAdd(&sh.used, 1u);
        }
    }
    __syncthreads();

    if (tid == 0) {
        const int m = (int)sh.used;  // >= 2: a literal and the end of block
        png_huffman_lengths(sh, sh.order, m, sh.hist, 15, sh.lens);
        png_canonical(sh, sh.lens, PNG_LITLEN, 15, sh.code);
        int hlit = 257;
        for (int s = 257; s < PNG_LITLEN; s++) hlit = sh.lens[s] ? s + 1 : hlit;
        // one distance code: length 1 when the chunk has a match (RFC 1951 3.2.7), else length 0
        const uint32_t dlen = sh.matches ? 1u : 0u;
        sh.lens[hlit] = (uint8_t)dlen;
        const int nseq = hlit + 1;
        uint32_t body = sh.matches * dlen;
        for (int s = 0; s < PNG_LITLEN; s++) body += sh.hist[s] * ((uint32_t)sh.lens[s] + (uint32_t)(s > 256 ? png_symbol_extra(s) : 0));
        // the code-length sequence: runs of zeros as 17 / 18, repeats of a length as 16 (runs cross from the literal / length code
        // into the distance code, which RFC 1951 allows)
        int ncl = 0;
        for (int i = 0; i < nseq;) {
            const int v = sh.lens[i];
            int r = 1;
            while (i + r < nseq && sh.lens[i + r] == v) r++;
            i += r;
            if (v) { sh.cltok[ncl++] = (uint16_t)v; sh.clhist[v]++; r--; }
            while (r >= 3) {
                const int take = min(r, v ? 6 : 138);
                const int sym = v ? 16 : (take <= 10 ? 17 : 18);
                sh.cltok[ncl++] = (uint16_t)(sym | ((take - (sym == 18 ? 11 : 3)) << 8));
                sh.clhist[sym]++;
                r -= take;
            }
            for (; r > 0; r--) { sh.cltok[ncl++] = (uint16_t)v; sh.clhist[v]++; }
        }
        int cm = 0;
        for (int s = 0; s < 19; s++) {
            if (!sh.clhist[s]) continue;
            int at = cm++;
            for (; at > 0 && sh.clhist[sh.clorder[at - 1]] > sh.clhist[s]; at--) sh.clorder[at] = sh.clorder[at - 1];
            sh.clorder[at] = (uint16_t)s;
        }
        if (cm == 1) {  // a complete code needs two symbols: an unused one takes the other 1-bit code
            sh.cllen[sh.clorder[0]] = 1;
            sh.cllen[sh.clorder[0] == 0 ? 1 : 0] = 1;
        } else {
            png_huffman_lengths(sh, sh.clorder, cm, sh.clhist, 7, sh.cllen);
        }
        png_canonical(sh, sh.cllen, 19, 7, sh.clcode);
        int hclen = 4;
        for (int i = 4; i < 19; i++) hclen = sh.cllen[png_cl_order[i]] ? i + 1 : hclen;
        uint32_t head = 3 + 5 + 5 + 4 + 3 * (uint32_t)hclen;
        for (int i = 0; i < ncl; i++) {
            const int sym = sh.cltok[i] & 0xff;
            head += (uint32_t)sh.cllen[sym] + (sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u);
        }
        const uint32_t stored = 3 + 5 + 32 + 8 * (uint32_t)n;  // header bits, padding to the byte, LEN / NLEN, the bytes
        sh.dynamic = head + body < stored ? 1u : 0u;
        if (sh.dynamic) {
            if (pre) out[0] = 0x0178u;
            PngBits w(out, 8u * (uint32_t)pre);
            w.put((final ? 1u : 0u) | (2u << 1), 3);
            w.put((uint32_t)(hlit - 257), 5);
            w.put(0u, 5);
            w.put((uint32_t)(hclen - 4), 4);
            for (int i = 0; i < hclen; i++) w.put(sh.cllen[png_cl_order[i]], 3);
            for (int i = 0; i < ncl; i++) {
                const int sym = sh.cltok[i] & 0xff;
                const uint32_t c = sh.clcode[sym];
                w.put(c & 0xffffu, (int)(c >> 16));
                if (sym >= 16) w.put((uint32_t)(sh.cltok[i] >> 8), sym == 16 ? 2 : sym == 17 ? 3 : 7);
            }
            w.flush();
            sh.bitpos = w.pos();
        }
    }
    __syncthreads();

    uint32_t nbytes;
    if (sh.dynamic) {
        // walk 2: the bit lengths of the thread's tokens -> bit offsets; walk 3: the bits
        uint32_t bits = 0;
        png_walk(data, s0, cnt, heads, carried, after,
                 [&](uint32_t v, int c) { bits += (uint32_t)c * (sh.code[v] >> 16); },
                 [&](int len) {
                     int sym, eb;
                     uint32_t ev;
                     png_length_code(len, sym, eb, ev);
                     bits += (sh.code[sym] >> 16) + (uint32_t)eb + 1u;
                 });
        uint32_t total;
        const uint32_t at = sh.bitpos + gsr_block_scan_excl<PNG_DEF_THREADS>(bits, &total);
        PngBits w(out, at);
        png_walk(data, s0, cnt, heads, carried, after,
                 [&](uint32_t v, int c) {
                     const uint32_t cd = sh.code[v];
                     for (int i = 0; i < c; i++) w.put(cd & 0xffffu, (int)(cd >> 16));  // c <= 2
                 },
                 [&](int len) {
                     int sym, eb;
                     uint32_t ev;
                     png_length_code(len, sym, eb, ev);
                     const uint32_t cd = sh.code[sym], l = cd >> 16;
                     w.put((cd & 0xffffu) | (ev << l), (int)l + eb + 1);  // ... and the distance code: one 0 bit
                 });
        w.flush();
        uint32_t end = sh.bitpos + total;
        if (tid == 0) {
            const uint32_t eob = sh.code[256];
            PngBits e(out, end);
            e.put(eob & 0xffffu, (int)(eob >> 16));
            e.flush();
        }
        end += sh.code[256] >> 16;
        nbytes = (end + 7u) >> 3;
        if (!final) {  // an empty stored block: 000, padding to the byte, 00 00 FF FF
            nbytes = ((end + 3u + 7u) >> 3) + 4u;
            if (tid == 0) {  // (ORed like the tokens: the dwords may hold the block's last bits)
                atomicOr(&out[(nbytes - 2u) >> 2], 0xffu << (8u * ((nbytes - 2u) & 3u)));
                atomicOr(&out[(nbytes - 1u) >> 2], 0xffu << (8u * ((nbytes - 1u) & 3u)));
            }
        }
    } else {
        uint8_t* o8 = (uint8_t*)out;
        if (tid == 0) {
            if (pre) { o8[0] = 0x78; o8[1] = 0x01; }
            o8[pre] = final ? 1 : 0;
            o8[pre + 1] = (uint8_t)(n & 0xff);
            o8[pre + 2] = (uint8_t)(n >> 8);
            o8[pre + 3] = (uint8_t)(~n & 0xff);
            o8[pre + 4] = (uint8_t)((~n >> 8) & 0xff);
            if (!final) { o8[pre + 5 + n + 3] = 0xff; o8[pre + 5 + n + 4] = 0xff; }
        }
        for (int i = tid; i < n; i += PNG_DEF_THREADS) o8[pre + 5 + i] = data[i];
        nbytes = (uint32_t)(pre + 5 + n + (final ? 0 : 5));
    }
    __syncthreads();
    uint32_t* slot = (uint32_t*)(base + lay.slots_off + (size_t)k * PNG_SLOT_BYTES);
    for (uint32_t i = tid; i < (nbytes + 3u) / 4u; i += PNG_DEF_THREADS) slot[i] = out[i];
    if (tid == 0) ((uint32_t*)(base + lay.sizes_off))[k] = nbytes;
}

// ---- assemble ---- (the CRC's slice arithmetic: png_crc.h)
__device__ __forceinline__ void png_put_be32(uint8_t* p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

__global__ void __launch_bounds__(PNG_ASM_THREADS) png_assemble_kernel(int H, int W, int C, const uint8_t* __restrict__ ws, PngLayout lay,
                                                                       uint8_t* __restrict__ out, size_t out_stride)
{
    __shared__ uint32_t tab[256];
    __shared__ uint32_t red[PNG_ASM_THREADS / 64];
    __shared__ uint32_t seg[2][PNG_ASM_THREADS];
    __shared__ uint8_t tail[4];  // the Adler-32, big-endian (last chunk only)
    const int k = (int)blockIdx.x, b = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunks = (int)lay.chunks;
    const bool last = k == chunks - 1;
    const uint8_t* base = ws + (size_t)b * lay.per_picture;
    const uint32_t* sizes = (const uint32_t*)(base + lay.sizes_off);
    const uint8_t* slot = base + lay.slots_off + (size_t)k * PNG_SLOT_BYTES;
    uint8_t* head = out + (size_t)b * out_stride;
    uint8_t* file = head + GSR_PNG_HEADER_BYTES;

    {  // the CRC table
        uint32_t c = (uint32_t)tid;
#pragma unroll
        for (int i = 0; i < 8; i++) c = (c & 1u) ? (c >> 1) ^ PNG_POLY : c >> 1;
        tab[tid] = c;
    }
    // the file offset of this IDAT: signature and IHDR, then the chunks before it
    uint32_t sum = 0;
    for (int j = tid; j < k; j += PNG_ASM_THREADS) sum += 12u + sizes[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, 64);
    if (lane == 0) red[wave] = sum;
    if (last) {  // Adler-32: a thread combines a run of rows, thread 0 the runs (below)
        const uint32_t* adler = (const uint32_t*)(base + lay.adler_off);
        const int per = (H + PNG_ASM_THREADS - 1) / PNG_ASM_THREADS;
        const unsigned long long n = lay.row_bytes % PNG_ADLER;
        unsigned long long A = 0, Bs = 0;
        for (int y = tid * per; y < min(H, (tid + 1) * per); y++) {
            Bs = (Bs + n * A + adler[2 * y + 1]) % PNG_ADLER;
            A = (A + adler[2 * y]) % PNG_ADLER;
        }
        seg[0][tid] = (uint32_t)A;
        seg[1][tid] = (uint32_t)Bs;
    }
    __syncthreads();
    uint32_t off = 33u;
#pragma unroll
    for (int w = 0; w < PNG_ASM_THREADS / 64; w++) off += red[w];
    const uint32_t size = sizes[k], len = size + (last ? 4u : 0u);
    if (last && tid == 0) {
        const int per = (H + PNG_ASM_THREADS - 1) / PNG_ASM_THREADS;
        unsigned long long a = 1, bb = 0;
        for (int t = 0; t < PNG_ASM_THREADS; t++) {
            const long long rows = min(H, (t + 1) * per) - min(H, t * per);
            const unsigned long long bytes = ((unsigned long long)rows * lay.row_bytes) % PNG_ADLER;
            bb = (bb + bytes * a + seg[1][t]) % PNG_ADLER;
            a = (a + seg[0][t]) % PNG_ADLER;
        }
        tail[0] = (uint8_t)(bb >> 8);
        tail[1] = (uint8_t)bb;
        tail[2] = (uint8_t)(a >> 8);
        tail[3] = (uint8_t)a;
    }
    __syncthreads();

    uint8_t* dst = file + off;
    if (tid == 0) {
        png_put_be32(dst, len);
        dst[4] = 'I'; dst[5] = 'D'; dst[6] = 'A'; dst[7] = 'T';
        if (last)
            for (int i = 0; i < 4; i++) dst[8 + size + i] = tail[i];
    }
    {  // the data: bytes up to the destination's first dword boundary, whole dwords (two source dwords each), the last bytes
        uint8_t* d = dst + 8;
        const uint32_t lead = min((uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u), size);
        const uint32_t words = (size - lead) / 4u;
        const uint32_t* s32 = (const uint32_t*)slot;
        uint32_t* d32 = (uint32_t*)(d + lead);
        if ((uint32_t)tid < lead) d[tid] = slot[tid];
        for (uint32_t i = tid; i < words; i += PNG_ASM_THREADS) {
            const uint32_t lo = s32[i];
            d32[i] = lead ? (lo >> (8u * lead)) | (s32[i + 1] << (32u - 8u * lead)) : lo;  // (s32[i + 1]: inside the slot's slack at the end)
        }
        const uint32_t done = lead + 4u * words;
        if ((uint32_t)tid < size - done) d[done + tid] = slot[done + tid];
    }
    // CRC-32 over type, data (and the Adler-32): N bytes in PNG_ASM_THREADS slices
    const uint32_t N = 4u + len, per = (N + PNG_ASM_THREADS - 1) / PNG_ASM_THREADS;
    const uint32_t lo = min(N, (uint32_t)tid * per), hi = min(N, lo + per);
    uint32_t r = 0;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t byte = i < 4u ? (0x54414449u >> (8u * i)) & 0xffu /* "IDAT" */ : (i - 4u < size ? slot[i - 4u] : tail[i - 4u - size]);
        r = tab[(r ^ byte) & 0xffu] ^ (r >> 8);
    }
    uint32_t crc = hi > lo ? png_gf2_mul(r, png_x8n(N - hi)) : 0u;
    if (tid == 0) crc ^= png_gf2_mul(0xffffffffu, png_x8n(N));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) crc ^= (uint32_t)__shfl_xor((int)crc, d, 64);
    __syncthreads();  // (red is read above)
    if (lane == 0) red[wave] = crc;
    __syncthreads();
    if (tid == 0) {
        crc = 0xffffffffu;
        for (int w = 0; w < PNG_ASM_THREADS / 64; w++) crc ^= red[w];
        png_put_be32(dst + 8 + len, crc);
        if (k == 0) {
            const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
            for (int i = 0; i < 8; i++) file[i] = sig[i];
            uint8_t* h = file + 8;
            png_put_be32(h, 13u);
            h[4] = 'I'; h[5] = 'H'; h[6] = 'D'; h[7] = 'R';
            png_put_be32(h + 8, (uint32_t)W);
            png_put_be32(h + 12, (uint32_t)H);
            h[16] = 8;
            h[17] = C == 1 ? 0 : (C == 3 ? 2 : 6);
            h[18] = h[19] = h[20] = 0;
            uint32_t c = 0xffffffffu;
            for (int i = 4; i < 21; i++) c = tab[(c ^ h[i]) & 0xffu] ^ (c >> 8);
            png_put_be32(h + 21, c ^ 0xffffffffu);
        }
        if (last) {
            uint8_t* e = dst + 12 + len;
            const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
            for (int i = 0; i < 12; i++) e[i] = iend[i];
            uint32_t* hw = (uint32_t*)head;
            hw[0] = off + 12u + len + 12u;  // the file's bytes
            hw[1] = (uint32_t)chunks;       // its IDAT chunks
            hw[2] = 0u;
            hw[3] = 0u;
        }
    }
}

static hipError_t png_launch_encode(const uint8_t* images, long long row_stride, long long image_stride, int B, int H, int W, int C, int filter,
                                    uint8_t* out, size_t out_stride, void* workspace, hipStream_t stream)
{
    const PngLayout lay = png_layout(H, W, C);
    const size_t lds = PNG_CHUNK + PNG_SLOT_BYTES;  // beyond 64 KiB: a one-time opt-in per device
    static thread_local uint64_t done_mask = 0;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (!(dev >= 0 && dev < 64 && ((done_mask >> dev) & 1))) {
        e = hipFuncSetAttribute((const void*)png_deflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64) done_mask |= 1ull << dev;
    }
    uint8_t* ws = (uint8_t*)workspace;
    hipLaunchKernelGGL(png_filter_kernel, dim3((uint32_t)H, (uint32_t)B), dim3(PNG_FLT_THREADS), 0, stream, images, row_stride, image_stride, W * C, C,
                       filter, ws, lay);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(png_deflate_kernel, dim3((uint32_t)lay.chunks, (uint32_t)B), dim3(PNG_DEF_THREADS), lds, stream, ws, lay);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(png_assemble_kernel, dim3((uint32_t)lay.chunks, (uint32_t)B), dim3(PNG_ASM_THREADS), 0, stream, H, W, C, (const uint8_t*)ws, lay, out,
                       out_stride);
    return hipGetLastError();
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
static int png_check_sizes(int B, int H, int W, int C)
{
    if (B <= 0 || H <= 0 || W <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: B=%d H=%d W=%d (need all > 0)", B, H, W);
    if (C != 1 && C != 3 && C != 4) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: C=%d (need 1, 3 or 4)", C);
    if (B > 65535) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: B=%d has too many pictures (need B <= 65535)", B);
    if ((int64_t)W * C >= (1 << 24)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: W=%d C=%d has too long a row (need W*C < 2^24)", W, C);
    if ((int64_t)H * ((int64_t)W * C + 1) >= 0x70000000LL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: H=%d W=%d C=%d has too many bytes (need H*(1 + W*C) < 0x70000000)", H, W, C);
    // (no accepted size wraps the layout: a picture's part is below 2^32 bytes, B below 2^16)
    return GSR_OK;
}

extern "C" size_t gsr_png_capacity(int H, int W, int C) { return png_check_sizes(1, H, W, C) ? 0 : png_layout(H, W, C).capacity; }

extern "C" size_t gsr_png_workspace_bytes(int B, int H, int W, int C)
{
    return png_check_sizes(B, H, W, C) ? 0 : (size_t)B * png_layout(H, W, C).per_picture;
}

extern "C" int gsr_png_encode(const uint8_t* images, long long row_stride, long long image_stride, int B, int H, int W, int C, int filter,
                              uint8_t* out, size_t out_stride, void* workspace, void* stream)
{
    if (int rc = png_check_sizes(B, H, W, C)) return rc;
    if (!images || !out || !workspace) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: images, out or workspace is NULL");
    if (filter < 0 || filter > GSR_PNG_FILTER_ADAPTIVE)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: filter=%d (need 0 .. 4 or GSR_PNG_FILTER_ADAPTIVE)", filter);
    if (row_stride < (long long)W * C) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: row_stride=%lld is below W*C=%lld", row_stride, (long long)W * C);
    if (B > 1 && image_stride < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: image_stride=%lld is negative", image_stride);
    const size_t need = GSR_PNG_HEADER_BYTES + png_layout(H, W, C).capacity;
    if (out_stride < need || out_stride % 4 || ((uintptr_t)out & 3))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: out_stride=%zu (need >= %zu = header + capacity, a multiple of 4) or out is not 4-byte aligned",
                        out_stride, need);
    if ((uintptr_t)workspace & 15) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: workspace is not 16-byte aligned");
    GSR_HIP(png_launch_encode(images, row_stride, image_stride, B, H, W, C, filter, out, out_stride, workspace, (hipStream_t)stream), "png encode");
    return GSR_OK;
}
