// jpeg.hip -- uint8 pictures -> baseline JPEG files on the device, byte for byte by the rules of include/gsraster.h ("JPEG encoding").
// Four launches per batch, nothing read back, no host stop, no global atomics, no dependency between workgroups of a launch, every
// loop bounded by a compile-time constant or an argument:
//   transform : a thread per row of an 8x8 block, 32 blocks a workgroup.  The thread reads its eight samples through the picture's
//               strides (clamped coordinates are the padding rule; a 4:2:0 chroma sample converts its four pixels), does the row
//               pass, hands it over through LDS, does the column pass of column (its row number), quantises, and places the values
//               in zigzag order in LDS, from where the block's 128 bytes leave in whole dwords: int16 [blocks][64], scan order.
//   entropy   : a workgroup per restart interval, a thread per block, run twice.  The thread keeps its 64 coefficients in registers;
//               the DC predictor is the previous block of its component in the coefficient array, so nothing is serial.  Walk 1
//               counts the block's bits, a block scan gives its bit offset, walk 2 ORs the bits into an LDS image MSB first -- in
//               pieces of JPEG_PIECE_BYTES, a thread taking part in the pieces its bits touch -- and a second scan over the 0xFF
//               bytes of a piece's words gives every thread the stuffed position of its words.  The first run (measure) only adds
//               the counts up: the interval's byte count.  The second (write) stores the bytes, each 0xFF followed by 0x00, at the
//               interval's file offset, and the RST marker behind it.
//   offsets   : between the two, a workgroup per picture: exclusive scan of the interval sizes in place, the file header (built on
//               the host, carried in the kernel arguments), EOI, the four header words and the "fits" word the write run reads.
// Measuring and writing in two runs instead of keeping a slot per interval (png.hip's shape) saves a workspace of 416 bytes a block,
// three times the picture, and the copy out of it; the price is coding every block twice.
// Integer arithmetic only; the same input gives the same bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_scan.h"
#include "jpeg_tables.h"

#define JPEG_TR_THREADS 256
#define JPEG_TR_BLOCKS (JPEG_TR_THREADS / 8)
#define JPEG_PIECE_BYTES 32768
#define JPEG_PIECE_WORDS (JPEG_PIECE_BYTES / 4)
#define JPEG_OFF_THREADS 256
#define JPEG_BLOCK_BYTES 416  // 22 + 63 * 26 bits = 208 bytes, doubled by stuffing
static_assert(GSR_JPEG_INTERVAL_BLOCKS == 1024, "the entropy kernel has at most 1024 threads, one per block of an interval");

#define JPEG_FILE_HEADER_MAX 640
struct JpegLayout {
    int comps, mcu, bpm;                  // components; MCU edge in pixels (8 or 16); blocks per MCU (1, 3, 6)
    int mcux, mcuy;                       // MCUs per row and per column
    int ri;                               // MCUs per restart interval (the resolved value)
    size_t mcus, blocks, intervals;       // per picture
    size_t file_header;                   // bytes in front of the scan: 629 (C = 3) or 334 (C = 1)
    size_t sizes_off, fits_off, per_picture;  // byte offsets inside a picture's part of the workspace, and its size
    size_t capacity;                      // file_header + 416 blocks + 3 mcus + 2
};
struct JpegTables {                       // travels in the kernel arguments
    uint8_t quant[2][64];                 // natural order, scaled to the quality
    uint8_t header[JPEG_FILE_HEADER_MAX]; // SOI .. SOS
};

__constant__ int jpeg_dct[64] = { JPEG_DCT_ROWS };
__constant__ uint8_t jpeg_zigzag[64] = { JPEG_ZIGZAG_LIST };
__constant__ uint32_t jpeg_dc_codes[2][12] = { { JPEG_DC0_CODES }, { JPEG_DC1_CODES } };     // code | length << 16
__constant__ uint32_t jpeg_ac_codes[2][256] = { { JPEG_AC0_CODES }, { JPEG_AC1_CODES } };

// ---- layout, tables and the file header (host) ----
// The workspace holds, per picture, the quantised coefficients (int16 [blocks][64], zigzag order, blocks in scan order), then the
// intervals' byte counts / file offsets, then one word that says whether the file fits.
static JpegLayout jpeg_layout(int H, int W, int C, int subsampling, int restart_interval)
{
    JpegLayout l;
    l.comps = C;
    l.mcu = (C == 3 && subsampling == 420) ? 16 : 8;
    l.bpm = C == 1 ? 1 : (subsampling == 420 ? 6 : 3);
    l.mcux = (W + l.mcu - 1) / l.mcu;
    l.mcuy = (H + l.mcu - 1) / l.mcu;
    const int most = GSR_JPEG_INTERVAL_BLOCKS / l.bpm;
    l.ri = restart_interval > 0 ? restart_interval : (l.mcux < most ? l.mcux : most);
    l.mcus = (size_t)l.mcux * (size_t)l.mcuy;
    l.blocks = l.mcus * (size_t)l.bpm;
    l.intervals = (l.mcus + (size_t)l.ri - 1) / (size_t)l.ri;
    l.file_header = C == 3 ? 629 : 334;
    GsrCarver c(nullptr);  // offsets only: the kernels add them to the start of the picture's part
    c.skip(l.blocks * 128, 16);
    l.sizes_off = c.bytes(); c.skip(l.intervals * 4, 16);
    l.fits_off = c.bytes(); c.skip(16, 16);
    l.per_picture = c.total();
    l.capacity = l.file_header + l.blocks * JPEG_BLOCK_BYTES + l.mcus * 3 + 2;
    return l;
}

static uint8_t* jpeg_put16(uint8_t* p, int v)
{
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
    return p + 2;
}
static uint8_t* jpeg_put_dht(uint8_t* p, int id, const uint8_t* bits, const uint8_t* values, int n)
{
    *p++ = 0xff; *p++ = 0xc4;
    p = jpeg_put16(p, 2 + 1 + 16 + n);
    *p++ = (uint8_t)id;
    memcpy(p, bits, 16);
    memcpy(p + 16, values, (size_t)n);
    return p + 16 + n;
}
static void jpeg_fill_tables(JpegTables* t, int H, int W, int C, int quality, int subsampling, const JpegLayout& lay)
{
    memset(t, 0, sizeof(*t));
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const uint8_t* base[2] = { JPEG_QUANT_BASE_0, JPEG_QUANT_BASE_1 };
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < 64; i++) {
            const int v = (base[k][i] * scale + 50) / 100;
            t->quant[k][i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    uint8_t* p = t->header;
    *p++ = 0xff; *p++ = 0xd8;
    *p++ = 0xff; *p++ = 0xe0;
    p = jpeg_put16(p, 16);
    memcpy(p, "JFIF", 5); p += 5;
    *p++ = 1; *p++ = 1; *p++ = 0;
    p = jpeg_put16(p, 1);
    p = jpeg_put16(p, 1);
    *p++ = 0; *p++ = 0;
    for (int k = 0; k < (C == 3 ? 2 : 1); k++) {
        *p++ = 0xff; *p++ = 0xdb;
        p = jpeg_put16(p, 67);
        *p++ = (uint8_t)k;
        for (int i = 0; i < 64; i++) *p++ = t->quant[k][JPEG_ZIGZAG[i]];
    }
    *p++ = 0xff; *p++ = 0xc0;
    p = jpeg_put16(p, 8 + 3 * C);
    *p++ = 8;
    p = jpeg_put16(p, H);
    p = jpeg_put16(p, W);
    *p++ = (uint8_t)C;
    for (int c = 0; c < C; c++) {
        *p++ = (uint8_t)(c + 1);
        *p++ = (c == 0 && subsampling == 420) ? 0x22 : 0x11;
        *p++ = c ? 1 : 0;
    }
    p = jpeg_put_dht(p, 0x00, JPEG_DC0_BITS, JPEG_DC0_VALUES, (int)sizeof(JPEG_DC0_VALUES));
    p = jpeg_put_dht(p, 0x10, JPEG_AC0_BITS, JPEG_AC0_VALUES, (int)sizeof(JPEG_AC0_VALUES));
    if (C == 3) {
        p = jpeg_put_dht(p, 0x01, JPEG_DC1_BITS, JPEG_DC1_VALUES, (int)sizeof(JPEG_DC1_VALUES));
        p = jpeg_put_dht(p, 0x11, JPEG_AC1_BITS, JPEG_AC1_VALUES, (int)sizeof(JPEG_AC1_VALUES));
    }
    *p++ = 0xff; *p++ = 0xdd;
    p = jpeg_put16(p, 4);
    p = jpeg_put16(p, lay.ri);
    *p++ = 0xff; *p++ = 0xda;
    p = jpeg_put16(p, 6 + 2 * C);
    *p++ = (uint8_t)C;
    for (int c = 0; c < C; c++) {
        *p++ = (uint8_t)(c + 1);
        *p++ = c ? 0x11 : 0x00;
    }
    *p++ = 0; *p++ = 63; *p++ = 0;
    // (p - t->header == lay.file_header: 629 or 334, checked by the caller's tests against the file)
}

// ---- transform ----
// component `comp` of the full-resolution pixel (y, x); coordinates beyond the picture repeat its last column and row
__device__ __forceinline__ int jpeg_sample(const uint8_t* __restrict__ img, long long row_stride, int H, int W, int C, int comp, int y, int x)
{
    y = min(y, H - 1);
    x = min(x, W - 1);
    const uint8_t* p = img + (long long)y * row_stride + (long long)x * C;
    if (C == 1) return p[0];
    const int R = p[0], G = p[1], B = p[2];
    if (comp == 0) return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    if (comp == 1) return (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    return (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}

__global__ void __launch_bounds__(JPEG_TR_THREADS) jpeg_transform_kernel(const uint8_t* __restrict__ images, long long row_stride, long long image_stride,
                                                                         int H, int W, int C, JpegTables tables, JpegLayout lay,
                                                                         uint8_t* __restrict__ ws)
{
    __shared__ int rows[JPEG_TR_BLOCKS][8][9];  // the row pass: [block][m][k] (a row of 9: the column pass reads down a column)
    __shared__ __attribute__((aligned(16))) int16_t zz[JPEG_TR_BLOCKS][64];
    __shared__ uint8_t place[64];  // natural index -> coding position
    __shared__ uint8_t quant[2][64];
    const int tid = (int)threadIdx.x, lb = tid >> 3, m = tid & 7, b = (int)blockIdx.y;
    if (tid < 64) place[jpeg_zigzag[tid]] = (uint8_t)tid;
    if (tid < 128) quant[tid >> 6][tid & 63] = tables.quant[tid >> 6][tid & 63];
    const size_t first = (size_t)blockIdx.x * JPEG_TR_BLOCKS, g = first + (size_t)lb;
    const bool valid = g < lay.blocks;
    const uint8_t* img = images + (long long)b * image_stride;
    int comp = 0;
    if (valid) {
        const size_t mcu = g / (size_t)lay.bpm;
        const int i = (int)(g - mcu * (size_t)lay.bpm), my = (int)(mcu / (size_t)lay.mcux), mx = (int)(mcu - (size_t)my * (size_t)lay.mcux);
        int x[8];
        if (lay.bpm == 6 && i >= 4) {  // a 4:2:0 chroma block: sample (cy, cx) is the mean of the 2x2 pixels at (2 cy, 2 cx)
            comp = i - 3;
            const int yy = 2 * (my * 8 + m);
#pragma unroll
            for (int n = 0; n < 8; n++) {
                const int xx = 2 * (mx * 8 + n);
                const int s = jpeg_sample(img, row_stride, H, W, C, comp, yy, xx) + jpeg_sample(img, row_stride, H, W, C, comp, yy, xx + 1)
                            + jpeg_sample(img, row_stride, H, W, C, comp, yy + 1, xx) + jpeg_sample(img, row_stride, H, W, C, comp, yy + 1, xx + 1);
                x[n] = ((s + 1 + (n & 1)) >> 2) - 128;
            }
        } else {
            int y0, x0;
            if (lay.bpm == 6) { comp = 0; y0 = my * 16 + (i >> 1) * 8; x0 = mx * 16 + (i & 1) * 8; }
            else { comp = i; y0 = my * 8; x0 = mx * 8; }
#pragma unroll
            for (int n = 0; n < 8; n++) x[n] = jpeg_sample(img, row_stride, H, W, C, comp, y0 + m, x0 + n) - 128;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            int s = 512;
#pragma unroll
            for (int n = 0; n < 8; n++) s += jpeg_dct[k * 8 + n] * x[n];
            rows[lb][m][k] = s >> 10;
        }
    }
    __syncthreads();
    if (valid) {
        const int j = m;  // the column this thread finishes
        int r[8];
#pragma unroll
        for (int n = 0; n < 8; n++) r[n] = rows[lb][n][j];
        const uint8_t* Q = quant[comp ? 1 : 0];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            int s = 4096;
#pragma unroll
            for (int n = 0; n < 8; n++) s += jpeg_dct[k * 8 + n] * r[n];
            const int c8 = s >> 13, q = (int)Q[k * 8 + j];
            const int a = (abs(c8) + 4 * q) / (8 * q);
            zz[lb][place[k * 8 + j]] = (int16_t)(c8 < 0 ? -a : a);
        }
    }
    __syncthreads();
    uint32_t* dst = (uint32_t*)(ws + (size_t)b * lay.per_picture + first * 128);
    const uint32_t* src = (const uint32_t*)&zz[0][0];
    for (int w = tid; w < JPEG_TR_BLOCKS * 32; w += JPEG_TR_THREADS)
        if (first + (size_t)(w >> 5) < lay.blocks) dst[w] = src[w];
}

// ---- entropy ----
struct JpegBits {  // a thread's contiguous bits, MSB first, ORed into the words [lo, hi) of the interval that the LDS image holds
    uint32_t* out;
    unsigned long long acc;  // the low nb bits are pending
    uint32_t word, lo, hi;
    int nb;
    __device__ __forceinline__ JpegBits(uint32_t* o, uint32_t pos, uint32_t l, uint32_t h) : out(o), acc(0ull), word(pos >> 5), lo(l), hi(h), nb((int)(pos & 31u)) {}
    __device__ __forceinline__ void put(uint32_t v, int n)  // n <= 26, v < 2^n
    {
        acc = (acc << n) | v;
        nb += n;
        if (nb >= 32) {
            nb -= 32;
            const uint32_t x = (uint32_t)(acc >> nb);
            if (word >= lo && word < hi && x) atomicOr(&out[word - lo], x);
            word++;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (nb > 0) {
            const uint32_t x = (uint32_t)(acc << (32 - nb));
            if (word >= lo && word < hi && x) atomicOr(&out[word - lo], x);
        }
    }
};

// The tokens of one block, in order: emit(bits, count).  q: its 64 coefficients in coding order; pred: the DC predictor.
template <typename Emit>
__device__ __forceinline__ void jpeg_block_tokens(const uint4 (&q)[8], int pred, const uint32_t* dc, const uint32_t* ac, Emit emit)
{
    int run = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t w[4] = { q[i].x, q[i].y, q[i].z, q[i].w };
#pragma unroll
        for (int h = 0; h < 8; h++) {
            int v = (int)(int16_t)(w[h >> 1] >> (16 * (h & 1)));
            if (i == 0 && h == 0) {
                v -= pred;
                const int size = v ? 32 - __clz(abs(v)) : 0;
                const uint32_t code = dc[size];
                emit(((code & 0xffffu) << size) | ((uint32_t)(v + (v >> 31)) & ((1u << size) - 1u)), (int)(code >> 16) + size);
            } else if (v == 0) {
                run++;
            } else {
                for (; run >= 16; run -= 16) emit(ac[0xf0] & 0xffffu, (int)(ac[0xf0] >> 16));  // at most three
                const int size = 32 - __clz(abs(v));
                const uint32_t code = ac[(run << 4) | size];
                emit(((code & 0xffffu) << size) | ((uint32_t)(v + (v >> 31)) & ((1u << size) - 1u)), (int)(code >> 16) + size);
                run = 0;
            }
        }
    }
    if (run) emit(ac[0] & 0xffffu, (int)(ac[0] >> 16));
}

template <int NT, bool WRITE>
__global__ void __launch_bounds__(NT) jpeg_entropy_kernel(uint8_t* __restrict__ ws, JpegLayout lay, uint8_t* __restrict__ out, size_t out_stride)
{
    __shared__ uint32_t image[JPEG_PIECE_WORDS];
    __shared__ uint32_t dc[2][12], ac[2][256];
    const int iv = (int)blockIdx.x, b = (int)blockIdx.y, tid = (int)threadIdx.x;
    uint8_t* base = ws + (size_t)b * lay.per_picture;
    uint32_t* sizes = (uint32_t*)(base + lay.sizes_off);
    if (WRITE && *(const uint32_t*)(base + lay.fits_off) == 0u) return;  // the whole workgroup: the file needs more room
    for (int i = tid; i < 24; i += NT) dc[i / 12][i % 12] = jpeg_dc_codes[i / 12][i % 12];
    for (int i = tid; i < 512; i += NT) ac[i >> 8][i & 255] = jpeg_ac_codes[i >> 8][i & 255];

    const size_t mcu0 = (size_t)iv * (size_t)lay.ri;
    const int nmcu = lay.mcus - mcu0 < (size_t)lay.ri ? (int)(lay.mcus - mcu0) : lay.ri, nblk = nmcu * lay.bpm;  // >= 1, <= NT
    const bool valid = tid < nblk;
    uint4 q[8];
    int pred = 0, tab = 0;
    if (valid) {
        const size_t g = mcu0 * (size_t)lay.bpm + (size_t)tid;
        const uint8_t* coef = base + g * 128;
#pragma unroll
        for (int i = 0; i < 8; i++) q[i] = ((const uint4*)coef)[i];
        const int i = tid % lay.bpm, lm = tid / lay.bpm;
        int back = 0;  // blocks back to the previous block of the component (0: none in this interval)
        if (lay.bpm == 1) back = tid > 0 ? 1 : 0;
        else if (lay.bpm == 3) back = lm > 0 ? 3 : 0;
        else if (i >= 4) back = lm > 0 ? 6 : 0;
        else if (i >= 1) back = 1;
        else back = lm > 0 ? 3 : 0;
        if (back) pred = (int)*(const int16_t*)(coef - (size_t)back * 128);
        tab = (lay.bpm == 3 && i >= 1) || (lay.bpm == 6 && i >= 4) ? 1 : 0;
    }
    __syncthreads();

    uint32_t bits = 0;
    if (valid) jpeg_block_tokens(q, pred, dc[tab], ac[tab], [&](uint32_t, int n) { bits += (uint32_t)n; });
    uint32_t total;
    const uint32_t start = gsr_block_scan_excl<NT>(bits, &total);
    const uint32_t padded = (total + 7u) & ~7u, nbytes = padded >> 3;  // the last byte is filled with 1 bits by the last block's thread
    const bool closes = tid == nblk - 1;
    const uint32_t end = closes ? padded : start + bits;
    const uint32_t at = WRITE ? sizes[iv] : 0u;  // the interval's file offset (the offsets kernel's scan)
    uint8_t* file = out + (size_t)b * out_stride + GSR_JPEG_HEADER_BYTES;
    uint32_t stuffed = 0;  // 0xFF bytes of the pieces done
    const uint32_t pieces = (nbytes + JPEG_PIECE_BYTES - 1) / JPEG_PIECE_BYTES;  // <= ceil(1024 * 208 / 32768) = 7
    for (uint32_t p = 0; p < pieces; p++) {
        const uint32_t lo = p * JPEG_PIECE_WORDS, hi = lo + JPEG_PIECE_WORDS;
        const uint32_t pbytes = min((uint32_t)JPEG_PIECE_BYTES, nbytes - p * JPEG_PIECE_BYTES), pwords = (pbytes + 3u) >> 2;
        __syncthreads();  // (the scan's totals and the image of the piece before are read)
        for (uint32_t i = tid; i < pwords; i += NT) image[i] = 0u;
        __syncthreads();
        if (valid && end > lo * 32u && start < hi * 32u) {
            JpegBits w(image, start, lo, hi);
            jpeg_block_tokens(q, pred, dc[tab], ac[tab], [&](uint32_t v, int n) { w.put(v, n); });
            if (closes && padded > total) w.put((1u << (padded - total)) - 1u, (int)(padded - total));
            w.flush();
        }
        __syncthreads();
        // a thread owns a run of the piece's words: its 0xFF bytes, then (write) its bytes at their stuffed position
        const uint32_t per = (pwords + NT - 1) / NT, w0 = min((uint32_t)tid * per, pwords), w1 = min(w0 + per, pwords);
        uint32_t ff = 0;
        for (uint32_t w = w0; w < w1; w++) {
            const uint32_t x = image[w];
#pragma unroll
            for (int k = 0; k < 4; k++) ff += (w * 4u + k < pbytes && ((x >> (24 - 8 * k)) & 0xffu) == 0xffu) ? 1u : 0u;
        }
        uint32_t fftotal;
        const uint32_t before = gsr_block_scan_excl<NT>(ff, &fftotal);
        if (WRITE) {
            uint8_t* d = file + at + p * JPEG_PIECE_BYTES + stuffed + before + w0 * 4u;
            for (uint32_t w = w0; w < w1; w++) {
                const uint32_t x = image[w];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t byte = (x >> (24 - 8 * k)) & 0xffu;
                    if (w * 4u + k < pbytes) {
                        *d++ = (uint8_t)byte;
                        if (byte == 0xffu) *d++ = 0;
                    }
                }
            }
        }
        stuffed += fftotal;
    }
    const bool last = (size_t)iv == lay.intervals - 1;
    if (tid == 0) {
        if (!WRITE) sizes[iv] = nbytes + stuffed + (last ? 0u : 2u);
        else if (!last) {
            uint8_t* d = file + at + nbytes + stuffed;
            d[0] = 0xff;
            d[1] = (uint8_t)(0xd0 + (iv & 7));
        }
    }
}

// ---- offsets ----
__global__ void __launch_bounds__(JPEG_OFF_THREADS) jpeg_offsets_kernel(uint8_t* __restrict__ ws, JpegLayout lay, JpegTables tables, uint8_t* __restrict__ out,
                                                                        size_t out_stride)
{
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    uint8_t* base = ws + (size_t)b * lay.per_picture;
    uint32_t* sizes = (uint32_t*)(base + lay.sizes_off);
    const uint32_t fh = (uint32_t)lay.file_header;
    uint32_t total;
    gsr_block_scan_runs<JPEG_OFF_THREADS, 0>((int)lay.intervals, [&](int j) { return sizes[j]; },
                                             [&](int j, uint32_t start, uint32_t) { sizes[j] = fh + start; }, &total);
    const uint32_t nfile = fh + total + 2u;  // < 2^31: the capacity is
    const bool fits = (size_t)nfile + GSR_JPEG_HEADER_BYTES <= out_stride;
    uint8_t* head = out + (size_t)b * out_stride;
    uint8_t* file = head + GSR_JPEG_HEADER_BYTES;
    if (fits) {
        for (uint32_t i = tid; i < fh; i += JPEG_OFF_THREADS) file[i] = tables.header[i];
        if (tid == 0) { file[nfile - 2] = 0xff; file[nfile - 1] = 0xd9; }
    }
    if (tid == 0) {
        uint32_t* hw = (uint32_t*)head;
        hw[0] = nfile;  // the file's bytes, or what it needs
        hw[1] = fits ? GSR_JPEG_OK : GSR_JPEG_NEED_CAPACITY;
        hw[2] = (uint32_t)lay.intervals;
        hw[3] = 0u;
        *(uint32_t*)(base + lay.fits_off) = fits ? 1u : 0u;
    }
}

template <int NT>
static hipError_t jpeg_launch_entropy(uint8_t* ws, const JpegLayout& lay, int B, uint8_t* out, size_t out_stride, const JpegTables& tables,
                                      hipStream_t stream)
{
    const dim3 grid((uint32_t)lay.intervals, (uint32_t)B);
    hipLaunchKernelGGL((jpeg_entropy_kernel<NT, false>), grid, dim3(NT), 0, stream, ws, lay, out, out_stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3((uint32_t)B), dim3(JPEG_OFF_THREADS), 0, stream, ws, lay, tables, out, out_stride);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((jpeg_entropy_kernel<NT, true>), grid, dim3(NT), 0, stream, ws, lay, out, out_stride);
    return hipGetLastError();
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
static int jpeg_check_sizes(int B, int H, int W, int C, int subsampling)
{
    if (B <= 0 || H <= 0 || W <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: B=%d H=%d W=%d (need all > 0)", B, H, W);
    if (C != 1 && C != 3) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: C=%d (need 1 or 3)", C);
    if (B > 65535 || H > 65535 || W > 65535) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: B=%d H=%d W=%d (need all <= 65535)", B, H, W);
    if (subsampling != 444 && subsampling != 420) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: subsampling=%d (need 444 or 420)", subsampling);
    if (subsampling == 420 && C == 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: subsampling 420 with C=1 (a grey picture has no chroma)");
    if (jpeg_layout(H, W, C, subsampling, 0).capacity >= ((size_t)1 << 31))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: H=%d W=%d C=%d has a capacity of 2^31 bytes or more", H, W, C);
    // (no accepted size wraps the layout: a picture's part is below 2^32 bytes, B below 2^16)
    return GSR_OK;
}

static int jpeg_check_interval(int C, int subsampling, int restart_interval)
{
    const int most = GSR_JPEG_INTERVAL_BLOCKS / (C == 1 ? 1 : (subsampling == 420 ? 6 : 3));
    if (restart_interval < 0 || restart_interval > most)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: restart_interval=%d (need 0 = the default, or 1 .. %d MCUs)", restart_interval, most);
    return GSR_OK;
}

// a pointer the kernels may use: device memory of this process
static bool jpeg_on_device(const void* p)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();  // (an unregistered host pointer: the error is ours to clear)
        return false;
    }
    return attr.type == hipMemoryTypeDevice;
}

extern "C" size_t gsr_jpeg_capacity(int H, int W, int C, int subsampling)
{
    return jpeg_check_sizes(1, H, W, C, subsampling) ? 0 : jpeg_layout(H, W, C, subsampling, 0).capacity;
}

extern "C" size_t gsr_jpeg_workspace_bytes(int B, int H, int W, int C, int subsampling, int restart_interval)
{
    if (jpeg_check_sizes(B, H, W, C, subsampling) || jpeg_check_interval(C, subsampling, restart_interval)) return 0;
    return (size_t)B * jpeg_layout(H, W, C, subsampling, restart_interval).per_picture;
}

extern "C" int gsr_jpeg_encode(const uint8_t* images, long long row_stride, long long image_stride, int B, int H, int W, int C, int quality,
                               int subsampling, int restart_interval, uint8_t* out, size_t out_stride, void* workspace, void* stream_)
{
    if (int rc = jpeg_check_sizes(B, H, W, C, subsampling)) return rc;
    if (int rc = jpeg_check_interval(C, subsampling, restart_interval)) return rc;
    if (!images || !out || !workspace) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: images, out or workspace is NULL");
    if (quality < 1 || quality > 100) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: quality=%d (need 1 .. 100)", quality);
    if (row_stride < (long long)W * C) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: row_stride=%lld is below W*C=%lld", row_stride, (long long)W * C);
    if (B > 1 && image_stride < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: image_stride=%lld is negative", image_stride);
    const JpegLayout lay = jpeg_layout(H, W, C, subsampling, restart_interval);
    const size_t need = GSR_JPEG_HEADER_BYTES + lay.file_header;
    if (out_stride < need || out_stride % 4 || ((uintptr_t)out & 3))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: out_stride=%zu (need >= %zu = the four words + the file header, a multiple of 4) or out is not 4-byte aligned",
                        out_stride, need);
    if ((uintptr_t)workspace & 15) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: workspace is not 16-byte aligned");
    if (!jpeg_on_device(images) || !jpeg_on_device(out) || !jpeg_on_device(workspace))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: images, out or workspace is not device memory");
    JpegTables tables;
    jpeg_fill_tables(&tables, H, W, C, quality, subsampling, lay);
    hipStream_t stream = (hipStream_t)stream_;
    uint8_t* ws = (uint8_t*)workspace;
    const size_t groups = (lay.blocks + JPEG_TR_BLOCKS - 1) / JPEG_TR_BLOCKS;
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((uint32_t)groups, (uint32_t)B), dim3(JPEG_TR_THREADS), 0, stream, images, row_stride, image_stride, H, W,
                       C, tables, lay, ws);
    GSR_HIP(hipGetLastError(), "jpeg encode");
    const int most = lay.ri * lay.bpm;  // blocks of a full interval: the workgroup's size
    if (most <= 64) GSR_HIP(jpeg_launch_entropy<64>(ws, lay, B, out, out_stride, tables, stream), "jpeg encode");
    else if (most <= 256) GSR_HIP(jpeg_launch_entropy<256>(ws, lay, B, out, out_stride, tables, stream), "jpeg encode");
    else GSR_HIP(jpeg_launch_entropy<1024>(ws, lay, B, out, out_stride, tables, stream), "jpeg encode");
    return GSR_OK;
}
