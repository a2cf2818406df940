// lpips.hip -- LPIPS v0.1 (net = 'vgg', lpips = True, eval mode), the third metric evaluate() (train.py:905-987) reports: thirteen
// 3x3 convolutions of VGG-16 in fp32 on the exact f32 matrix cores, the unit-normalised squared feature distance under the 1x1 `lin`
// weights at five taps, and the plain, per-layer, spatial and masked values.  The rule is in include/gsraster.h in full.
//
//   conv   : conv3x3 + bias + ReLU as an implicit GEMM on v_mfma_f32_32x32x2_f32, NCHW in and out.  M = 64 output channels (the A
//            operand, from the packed weights), N = an LPC_TH x LPC_TW = 8 x 32 tile of output pixels (the B operand, from the input
//            halo tile), K = 9 Cin walked in chunks of LPC_KC = 8 input channels.  A workgroup of four waves stages, per chunk, the
//            10 x 34 halo of the 8 channels ([c][y][x], 2720 floats) and the chunk's weights ([tap][c][64], 4608 floats, one
//            contiguous piece of the packed blob) in LDS, through registers: the next chunk's loads are issued before the MFMA loop
//            of the current one; wave w owns tile rows 2w and 2w + 1 and all 64 channels: four 32 x 32
//            accumulators, four MFMAs per two A and two B reads.  Lane l = (j = l & 31, h = l >> 5) supplies A[channel j][k = h] and
//            B[k = h][pixel j] and holds D[channel (r & 3) + 8 (r >> 2) + 4 h][pixel j] in register r, so the lanes of a half read 32
//            consecutive dwords of LDS in both operands (every bank once) and store 32 consecutive pixels of one channel row.
//            The accumulator starts at the bias; the k order of an output element is: chunks ascending, within a chunk the taps
//            (ky, kx) row-major, within a tap the chunk's channels ascending -- the same for every element, so the same inputs give
//            the same bits.  Channels beyond Cin in the last chunk carry zero weights and zero inputs: fma(0, 0, acc) = acc.
//            With Cin = 3 the loader applies the normalise and scaling steps to the pixels inside the image; the padding stays 0.
//   pool   : 2x2 stride-2 max, floor, one thread per output element.
//   head   : one thread per pixel of a tap and view: n = sqrt(sum_c f^2) for both images, then m = sum_c lin[c] (f0/(n0+1e-10) -
//            f1/(n1+1e-10))^2, channels ascending, all in fp64 (contraction off); m is stored rounded to fp32 and its fp64 value is
//            summed over the workgroup in a fixed order (xor-butterfly, then the waves in order) into a partial.
//   spatial: one thread per image pixel: the five maps sampled by torch's bilinear rule in fp32 and added in tap order; the value
//            under the mask and the count are summed per workgroup in fp64.
//   finish : one workgroup per view adds the partials in a fixed order and divides.
// No atomics anywhere.  Index arithmetic into the activations is 64-bit: 2B * 64 * H * W passes 2^31 at two views of 567 x 1008.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_reduce.h"

#pragma clang fp contract(off)

typedef float lp_v16 __attribute__((ext_vector_type(16)));
typedef float lp_v4 __attribute__((ext_vector_type(4)));
#define LP_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_32x32x2f32((A), (B), (C), 0, 0, 0)

#define LPC_THREADS 256
#define LPC_TW 32
#define LPC_TH 8
// The packed weights of a layer are [Cout / LPIPS_CONV_NB][ceil(Cin / LPIPS_CONV_KC)][9][LPIPS_CONV_KC][LPIPS_CONV_NB] floats, zero where
// the channel is beyond Cin.
#define LPIPS_CONV_KC 8
#define LPIPS_CONV_NB 64
#define LPC_KC LPIPS_CONV_KC            // input channels per staged chunk
#define LPC_NB LPIPS_CONV_NB            // output channels per workgroup
#define LPC_HW (LPC_TW + 2)             // 34 staged columns
#define LPC_HH (LPC_TH + 2)             // 10 staged rows
#define LPC_CP (LPC_HW * LPC_HH)        // 340 floats per staged channel
#define LPC_WCHUNK (9 * LPC_KC * LPC_NB)  // 4608 floats of weights per chunk
static_assert(LPC_KC == 8 && LPC_NB == 64 && LPC_THREADS == 256, "the wave / tile maps below are written for these");
static_assert(LPC_WCHUNK % 4 == 0, "the weight chunk is copied as float4");
#define LPC_XN ((LPC_KC * LPC_CP + LPC_THREADS - 1) / LPC_THREADS)   // 11 halo elements per thread and chunk
#define LPC_WN ((LPC_WCHUNK / 4 + LPC_THREADS - 1) / LPC_THREADS)    // 5 float4 of weights per thread and chunk

#define LP_THREADS 256

__device__ __constant__ float lp_shift[3] = {-0.030f, -0.088f, -0.188f};
__device__ __constant__ float lp_scale[3] = {0.458f, 0.448f, 0.450f};

__global__ void __launch_bounds__(LPC_THREADS) lpips_conv_kernel(int Cin, int Cout, int H, int W, int tiles_x, const float* __restrict__ in,
                                                                const float* __restrict__ wpack, const float* __restrict__ bias,
                                                                float* __restrict__ out, int flags)
{
    __shared__ __attribute__((aligned(16))) float ws[LPC_WCHUNK];
    __shared__ float xs[LPC_KC * LPC_CP];
    const int tile = (int)blockIdx.x, cb = (int)blockIdx.y, n = (int)blockIdx.z;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int x0 = tile_x * LPC_TW, y0 = tile_y * LPC_TH;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int chunks = (Cin + LPC_KC - 1) / LPC_KC;
    const size_t hw = (size_t)H * (size_t)W;
    const float* img = in + (size_t)n * (size_t)Cin * hw;
    const float* wblock = wpack + (size_t)cb * (size_t)chunks * LPC_WCHUNK;
    const int co0 = cb * LPC_NB;

    lp_v16 acc[2][2];  // [channel tile][pixel row]
#pragma unroll
    for (int ct = 0; ct < 2; ct++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float b = bias[co0 + ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * h];
            acc[ct][0][r] = b;
            acc[ct][1][r] = b;
        }

    // what this thread stages of every chunk: LPC_XN halo elements (their place in the image is the same for every chunk, so the
    // offsets are formed once) and LPC_WN float4 of weights.  The next chunk's values are loaded into registers before the MFMA
    // loop of the current one and stored to LDS after it, so the loads are in flight while the matrix cores work.
    int xoff[LPC_XN];  // gy * W + gx, or -1 outside the image (and beyond the staged tile)
#pragma unroll
    for (int i = 0; i < LPC_XN; i++) {
        const int e = tid + i * LPC_THREADS, rem = e % LPC_CP;
        const int hy = rem / LPC_HW, hx = rem - hy * LPC_HW;
        const int gy = y0 + hy - 1, gx = x0 + hx - 1;
        xoff[i] = (e < LPC_KC * LPC_CP && gy >= 0 && gy < H && gx >= 0 && gx < W) ? gy * W + gx : -1;  // H * W < 2^31
    }
    float xr[LPC_XN];
    lp_v4 wr[LPC_WN];
    auto fetch = [&](int chunk) {
        const lp_v4* wsrc = reinterpret_cast<const lp_v4*>(wblock + (size_t)chunk * LPC_WCHUNK);
#pragma unroll
        for (int i = 0; i < LPC_WN; i++) {
            const int e = tid + i * LPC_THREADS;
            if (e < LPC_WCHUNK / 4) wr[i] = wsrc[e];
        }
#pragma unroll
        for (int i = 0; i < LPC_XN; i++) {
            const int ci = chunk * LPC_KC + (tid + i * LPC_THREADS) / LPC_CP;
            float v = 0.0f;
            if (xoff[i] >= 0 && ci < Cin) {
                v = img[(size_t)ci * hw + (size_t)xoff[i]];
                if (flags & GSR_LPIPS_NORMALIZE) v = __fsub_rn(__fmul_rn(2.0f, v), 1.0f);
                if (flags & GSR_LPIPS_SCALING) v = __fdiv_rn(__fsub_rn(v, lp_shift[ci]), lp_scale[ci]);  // (Cin == 3, checked by the caller)
            }
            xr[i] = v;
        }
    };
    fetch(0);
    for (int chunk = 0; chunk < chunks; chunk++) {
        __syncthreads();  // the previous chunk's reads are done
#pragma unroll
        for (int i = 0; i < LPC_WN; i++) {
            const int e = tid + i * LPC_THREADS;
            if (e < LPC_WCHUNK / 4) reinterpret_cast<lp_v4*>(ws)[e] = wr[i];
        }
#pragma unroll
        for (int i = 0; i < LPC_XN; i++) {
            const int e = tid + i * LPC_THREADS;
            if (e < LPC_KC * LPC_CP) xs[e] = xr[i];
        }
        __syncthreads();
        if (chunk + 1 < chunks) fetch(chunk + 1);
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int dy = tap / 3, dx = tap - 3 * dy;
            const float* wp = ws + tap * (LPC_KC * LPC_NB) + h * LPC_NB + j;
            const float* xp = xs + h * LPC_CP + (2 * wave + dy) * LPC_HW + j + dx;
#pragma unroll
            for (int s = 0; s < LPC_KC / 2; s++) {
                const float a0 = wp[2 * s * LPC_NB], a1 = wp[2 * s * LPC_NB + 32];
                const float b0 = xp[2 * s * LPC_CP], b1 = xp[2 * s * LPC_CP + LPC_HW];
                acc[0][0] = LP_MFMA(a0, b0, acc[0][0]);
                acc[0][1] = LP_MFMA(a0, b1, acc[0][1]);
                acc[1][0] = LP_MFMA(a1, b0, acc[1][0]);
                acc[1][1] = LP_MFMA(a1, b1, acc[1][1]);
            }
        }
    }

    const int px = x0 + j;
    if (px >= W) return;
    float* oimg = out + (size_t)n * (size_t)Cout * hw;
#pragma unroll
    for (int pr = 0; pr < 2; pr++) {
        const int py = y0 + 2 * wave + pr;
        if (py >= H) continue;
#pragma unroll
        for (int ct = 0; ct < 2; ct++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int co = co0 + ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const float v = acc[ct][pr][r];
                oimg[(size_t)co * hw + (size_t)py * (size_t)W + (size_t)px] = v < 0.0f ? 0.0f : v;  // (a NaN stays a NaN)
            }
    }
}

__global__ void __launch_bounds__(LP_THREADS) lpips_pool_kernel(long long total /* planes * Ho * Wo */, int H, int W, int Ho, int Wo,
                                                               const float* __restrict__ in, float* __restrict__ out)
{
    const long long e = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (e >= total) return;
    const long long row = e / Wo, plane = row / Ho;
    const int x = (int)(e - row * Wo), y = (int)(row - plane * Ho);
    const float* p = in + ((size_t)plane * (size_t)H + (size_t)(2 * y)) * (size_t)W + (size_t)(2 * x);
    out[e] = fmaxf(fmaxf(p[0], p[1]), fmaxf(p[W], p[W + 1]));
}

__global__ void __launch_bounds__(LP_THREADS) lpips_head_kernel(int B, int C, long long hw, const float* __restrict__ feat /* [2B,C,hw] */,
                                                               const float* __restrict__ lin, float* __restrict__ map /* [B,hw] */,
                                                               double* __restrict__ partials /* [B,gridDim.x] */)
{
    const int b = (int)blockIdx.y;
    const long long p = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
    double m = 0.0;
    if (p < hw) {
        const float* f0 = feat + (size_t)b * (size_t)C * (size_t)hw + (size_t)p;
        const float* f1 = feat + (size_t)(B + b) * (size_t)C * (size_t)hw + (size_t)p;
        double n0 = 0.0, n1 = 0.0;
        for (int c = 0; c < C; c++) {
            const double a = (double)f0[(size_t)c * (size_t)hw], e = (double)f1[(size_t)c * (size_t)hw];
            n0 += a * a;
            n1 += e * e;
        }
        n0 = sqrt(n0) + 1e-10;
        n1 = sqrt(n1) + 1e-10;
        for (int c = 0; c < C; c++) {
            const double d = (double)f0[(size_t)c * (size_t)hw] / n0 - (double)f1[(size_t)c * (size_t)hw] / n1;
            m += (double)lin[c] * (d * d);
        }
        map[(size_t)b * (size_t)hw + (size_t)p] = (float)m;
    }
    const double s = gsr_block_reduce_all<LP_THREADS>(m, gsr_add());
    if (threadIdx.x == 0) partials[(size_t)b * gridDim.x + blockIdx.x] = s;
}

struct lp_levels {
    const float* map[5];  // [B, h*w]
    int h[5], w[5];
};

// torch's upsample_bilinear2d, align_corners = False, in fp32
__device__ __forceinline__ void lp_source(int dst, int in, int out, int& i0, int& i1, float& l0, float& l1)
{
    const float scale = __fdiv_rn((float)in, (float)out);
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    src = src < 0.0f ? 0.0f : src;
    i0 = (int)src;
    i0 = i0 > in - 1 ? in - 1 : i0;
    i1 = i0 < in - 1 ? i0 + 1 : i0;
    l1 = __fsub_rn(src, (float)i0);
    l0 = __fsub_rn(1.0f, l1);
}

__global__ void __launch_bounds__(LP_THREADS) lpips_spatial_kernel(int H, int W, lp_levels lv, const uint8_t* __restrict__ mask,
                                                                  long long mask_stride_b, float* __restrict__ spatial /* [B,H,W] or NULL */,
                                                                  double* __restrict__ partials /* [B,gridDim.x,2] */)
{
    const int b = (int)blockIdx.y;
    const long long hw = (long long)H * W, p = (long long)blockIdx.x * LP_THREADS + threadIdx.x;
    double value = 0.0, count = 0.0;
    if (p < hw) {
        const int y = (int)(p / W), x = (int)(p - (long long)y * W);
        float s = 0.0f;
#pragma unroll
        for (int l = 0; l < 5; l++) {
            int y0, y1, x0, x1;
            float ly0, ly1, lx0, lx1;
            lp_source(y, lv.h[l], H, y0, y1, ly0, ly1);
            lp_source(x, lv.w[l], W, x0, x1, lx0, lx1);
            const float* m = lv.map[l] + (size_t)b * (size_t)lv.h[l] * (size_t)lv.w[l];
            const size_t r0 = (size_t)y0 * (size_t)lv.w[l], r1 = (size_t)y1 * (size_t)lv.w[l];
            const float top = __fadd_rn(__fmul_rn(lx0, m[r0 + x0]), __fmul_rn(lx1, m[r0 + x1]));
            const float bot = __fadd_rn(__fmul_rn(lx0, m[r1 + x0]), __fmul_rn(lx1, m[r1 + x1]));
            const float v = __fadd_rn(__fmul_rn(ly0, top), __fmul_rn(ly1, bot));
            s = l == 0 ? v : __fadd_rn(s, v);
        }
        if (spatial) spatial[(size_t)b * (size_t)hw + (size_t)p] = s;
        if (!mask || mask[(size_t)b * (size_t)mask_stride_b + (size_t)p] != 0) {  // selected, not multiplied
            value = (double)s;
            count = 1.0;
        }
    }
    const double vs = gsr_block_reduce_all<LP_THREADS>(value, gsr_add());
    __syncthreads();
    const double cs = gsr_block_reduce_all<LP_THREADS>(count, gsr_add());
    if (threadIdx.x == 0) {
        double* o = partials + ((size_t)b * gridDim.x + blockIdx.x) * 2;
        o[0] = vs;
        o[1] = cs;
    }
}

struct lp_finish_args {
    const double* head[5];  // [B, blocks[l]]
    int blocks[5];
    double pixels[5];       // h*w of the tap
    const double* spatial;  // [B, sblocks, 2]
    int sblocks;
};

__global__ void __launch_bounds__(LP_THREADS) lpips_finish_kernel(lp_finish_args a, float* __restrict__ out_plain, float* __restrict__ out_layers,
                                                                 float* __restrict__ out_masked)
{
    const int b = (int)blockIdx.x;
    double total = 0.0;
    for (int l = 0; l < 5; l++) {
        const double* in = a.head[l] + (size_t)b * (size_t)a.blocks[l];
        double v = 0.0;
        for (int i = threadIdx.x; i < a.blocks[l]; i += LP_THREADS) v += in[i];
        const double mean = gsr_block_reduce_all<LP_THREADS>(v, gsr_add()) / a.pixels[l];
        __syncthreads();  // (before the next sum: gsr_reduce.h)
        if (threadIdx.x == 0 && out_layers) out_layers[(size_t)b * 5 + l] = (float)mean;
        total = l == 0 ? mean : total + mean;
    }
    const double* in = a.spatial + (size_t)b * (size_t)a.sblocks * 2;
    double v = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < a.sblocks; i += LP_THREADS) {
        v += in[2 * (size_t)i];
        c += in[2 * (size_t)i + 1];
    }
    const double vs = gsr_block_reduce_all<LP_THREADS>(v, gsr_add());
    __syncthreads();
    const double cs = gsr_block_reduce_all<LP_THREADS>(c, gsr_add());
    if (threadIdx.x == 0) {
        out_plain[b] = (float)total;
        if (out_masked) out_masked[b] = (float)(vs / cs);  // an empty mask: 0/0 = NaN
    }
}

// ---- host side ----
static const int lp_widths[13][2] = {{3, 64}, {64, 64}, {64, 128}, {128, 128}, {128, 256}, {256, 256}, {256, 256},
                                     {256, 512}, {512, 512}, {512, 512}, {512, 512}, {512, 512}, {512, 512}};
static const int lp_group_end[5] = {1, 3, 6, 9, 12};  // the layer whose ReLU output is tap l
static const int lp_tap_channels[5] = {64, 128, 256, 512, 512};

static size_t lp_packed_floats(int Cin, int Cout) { return (size_t)(Cout / LPC_NB) * (size_t)((Cin + LPC_KC - 1) / LPC_KC) * LPC_WCHUNK; }
static int lp_blocks(long long hw) { return (int)((hw + LP_THREADS - 1) / LP_THREADS); }

static hipError_t lpips_launch_conv(int N, int Cin, int Cout, int H, int W, const float* in, const float* wpack, const float* bias, float* out, int flags,
                                    hipStream_t stream)
{
    const int tiles_x = (W + LPC_TW - 1) / LPC_TW, tiles_y = (H + LPC_TH - 1) / LPC_TH;
    hipLaunchKernelGGL(lpips_conv_kernel, dim3((uint32_t)(tiles_x * tiles_y), (uint32_t)(Cout / LPC_NB), (uint32_t)N), dim3(LPC_THREADS), 0, stream,
                       Cin, Cout, H, W, tiles_x, in, wpack, bias, out, flags);
    return hipGetLastError();
}

// the carve of the workspace: two activation buffers of 2B*64*H*W floats (the largest stage), the five maps, the head partials, the
// spatial partials; every piece on a 512-byte boundary
struct lp_carve {
    float *buf[2], *map[5];
    double *head[5], *spatial;
    size_t total;
    int h[5], w[5], blocks[5], sblocks;
};

static lp_carve lp_plan(void* base, int B, int H, int W)
{
    lp_carve p;
    GsrCarver c(base);
    for (int k = 0; k < 2; k++) p.buf[k] = c.take<float>((size_t)2 * (size_t)B * 64 * (size_t)H * (size_t)W, 512);
    int h = H, w = W;
    for (int l = 0; l < 5; l++) {
        p.h[l] = h;
        p.w[l] = w;
        p.blocks[l] = lp_blocks((long long)h * w);
        p.map[l] = c.take<float>((size_t)B * (size_t)h * (size_t)w, 512);
        p.head[l] = c.take<double>((size_t)B * (size_t)p.blocks[l], 512);
        h /= 2;
        w /= 2;
    }
    p.sblocks = lp_blocks((long long)H * W);
    p.spatial = c.take<double>((size_t)B * (size_t)p.sblocks * 2, 512);
    p.total = c.total();
    return p;
}

static hipError_t lpips_launch(int B, int H, int W, const float* in0, const float* in1, int flags, const float* conv_weights, const float* conv_bias,
                               const float* lin_weights, const uint8_t* mask, long long mask_stride_b, void* workspace, float* out_plain,
                               float* out_layers, float* out_masked, float* out_spatial, hipStream_t stream)
{
    const lp_carve c = lp_plan(workspace, B, H, W);
    float* cur = c.buf[0];  // holds the newest activations
    float* other = c.buf[1];
    hipError_t e;
    lp_levels lv;
    lp_finish_args fa;
    const float* wp = conv_weights;
    const float* bp = conv_bias;
    const float* lp = lin_weights;
    int h = H, w = W, layer = 0;
    for (int l = 0; l < 5; l++) {
        if (l > 0) {  // pool cur -> other
            const int ho = h / 2, wo = w / 2, C = lp_tap_channels[l - 1];
            const long long total = (long long)2 * B * C * ho * wo;
            hipLaunchKernelGGL(lpips_pool_kernel, dim3((uint32_t)((total + LP_THREADS - 1) / LP_THREADS)), dim3(LP_THREADS), 0, stream, total, h, w, ho,
                               wo, (const float*)cur, other);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            float* t = cur; cur = other; other = t;
            h = ho;
            w = wo;
        }
        for (; layer <= lp_group_end[l]; layer++) {
            const int Cin = lp_widths[layer][0], Cout = lp_widths[layer][1];
            if (layer == 0) {  // the two inputs become one batch of 2B images
                const int f = (flags & GSR_LPIPS_NORMALIZE) | GSR_LPIPS_SCALING;
                if ((e = lpips_launch_conv(B, Cin, Cout, h, w, in0, wp, bp, cur, f, stream)) != hipSuccess) return e;
                if ((e = lpips_launch_conv(B, Cin, Cout, h, w, in1, wp, bp, cur + (size_t)B * 64 * (size_t)h * (size_t)w, f, stream)) != hipSuccess) return e;
            } else {
                if ((e = lpips_launch_conv(2 * B, Cin, Cout, h, w, cur, wp, bp, other, 0, stream)) != hipSuccess) return e;
                float* t = cur; cur = other; other = t;
            }
            wp += lp_packed_floats(Cin, Cout);
            bp += Cout;
        }
        float* map = c.map[l];
        double* part = c.head[l];
        const long long hw = (long long)h * w;
        hipLaunchKernelGGL(lpips_head_kernel, dim3((uint32_t)c.blocks[l], (uint32_t)B), dim3(LP_THREADS), 0, stream, B, lp_tap_channels[l], hw,
                           (const float*)cur, lp, map, part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        lp += lp_tap_channels[l];
        lv.map[l] = map;
        lv.h[l] = h;
        lv.w[l] = w;
        fa.head[l] = part;
        fa.blocks[l] = c.blocks[l];
        fa.pixels[l] = (double)hw;
    }
    double* sp = c.spatial;
    hipLaunchKernelGGL(lpips_spatial_kernel, dim3((uint32_t)c.sblocks, (uint32_t)B), dim3(LP_THREADS), 0, stream, H, W, lv, mask, mask_stride_b,
                       out_spatial, sp);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    fa.spatial = sp;
    fa.sblocks = c.sblocks;
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((uint32_t)B), dim3(LP_THREADS), 0, stream, fa, out_plain, out_layers, out_masked);
    return hipGetLastError();
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
static int lpips_check_sizes(int B, int H, int W)
{
    if (B <= 0 || B > 32767) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: B=%d (need 1 .. 32767 views: 2B images are one batch)", B);
    if (H < 16 || W < 16) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: H=%d W=%d (need both >= 16: four 2x2 pools)", H, W);
    if ((int64_t)H * (int64_t)W >= 0x7fffff00LL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: H=%d W=%d has too many pixels (need H*W < 2^31 - 256)", H, W);
    // (no accepted size wraps the carve: an activation buffer is 2 B * 64 * H*W floats < 2^15 * 2^9 * 2^31 = 2^55 bytes)
    return GSR_OK;
}

extern "C" size_t gsr_lpips_workspace_bytes(int B, int H, int W)
{
    if (lpips_check_sizes(B, H, W)) return 0;
    return lp_plan(nullptr, B, H, W).total;
}

extern "C" int gsr_lpips(int B, int H, int W, const float* in0, const float* in1, int flags, const float* conv_weights, const float* conv_bias,
                         const float* lin_weights, const uint8_t* mask, long long mask_stride_b, void* workspace, float* out_plain,
                         float* out_layers, float* out_masked, float* out_spatial, void* stream)
{
    if (int rc = lpips_check_sizes(B, H, W)) return rc;
    if (!in0 || !in1 || !conv_weights || !conv_bias || !lin_weights || !workspace || !out_plain)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: in0, in1, conv_weights, conv_bias, lin_weights, workspace or out_plain is NULL");
    if (flags & ~GSR_LPIPS_NORMALIZE) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: unknown flag bits in %d", flags);
    if (mask_stride_b < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: negative mask stride %lld", mask_stride_b);
    GSR_HIP(lpips_launch(B, H, W, in0, in1, flags, conv_weights, conv_bias, lin_weights, mask, mask_stride_b, workspace, out_plain, out_layers,
                         out_masked, out_spatial, (hipStream_t)stream),
            "lpips");
    return GSR_OK;
}

extern "C" int gsr_conv3x3_relu(int B, int Cin, int Cout, int H, int W, const float* in, const float* weights_packed, const float* bias,
                                float* out, int flags, void* stream)
{
    if (B <= 0 || B > 65535) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: B=%d (need 1 .. 65535 images)", B);
    if (Cin <= 0 || Cout <= 0 || Cout % LPIPS_CONV_NB != 0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: Cin=%d Cout=%d (need Cin > 0 and Cout a positive multiple of %d)", Cin, Cout, LPIPS_CONV_NB);
    if (Cin > 65536 || Cout > 65536) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: Cin=%d Cout=%d is too wide", Cin, Cout);
    if (H <= 0 || W <= 0 || (int64_t)H * (int64_t)W >= 0x7fffff00LL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: H=%d W=%d (need both > 0 and H*W < 2^31 - 256)", H, W);
    if (!in || !weights_packed || !bias || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: in, weights_packed, bias or out is NULL");
    if (flags & ~(GSR_LPIPS_NORMALIZE | GSR_LPIPS_SCALING)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: unknown flag bits in %d", flags);
    if (flags && Cin != 3) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: the input transforms are for Cin = 3 (got %d)", Cin);
    GSR_HIP(lpips_launch_conv(B, Cin, Cout, H, W, in, weights_packed, bias, out, flags, (hipStream_t)stream), "conv3x3");
    return GSR_OK;
}
