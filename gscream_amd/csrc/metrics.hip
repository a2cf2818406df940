// metrics.hip -- the test-view metrics evaluate() (train.py:905-990) and training_report (:655-708) log: L1, MSE, PSNR
// (utils/image_utils.py:22-32) and the 5x5 reflect-padded SSIM of my_ssim (utils/loss_utils.py:123-128, kornia 0.6.12's
// metrics.ssim), each over the whole image and over a boolean mask, for a batch of images in one launch.  The rules are in
// include/gsraster.h in full.
//
// The reference runs, per view, five 5x5 conv2d over padded copies, ~15 elementwise passes, a boolean-mask gather (a nonzero and a
// host stop) per masked value and one .item() per value.  The algorithm needs both images read once:
//   tile   : one workgroup per MET_TH x MET_TW = 16 x 32 pixel tile of one (b, c) plane.  It stages the tile plus the 2-pixel halo of
//            both images as fp32 in LDS (reflected indices, input transform applied on the way in), filters horizontally into five
//            fp64 planes in LDS (mu1, mu2, e11, e22, e12 of the 20 staged rows), then vertically per pixel -- two pixels per
//            thread, rows ly and ly + 8 -- forms dssim, reads the mask byte, and reduces its eight sums over the workgroup in a
//            fixed order (own pixels, xor-butterfly over the wave, the four waves in order) into workspace[(b*C + c)*tiles + tile].
//   finish : one workgroup per image sums that image's C*tiles partials in a fixed order and writes sums[b] and metrics[b].
// No atomics, no intermediate image in HBM: 8 bytes per element plus its mask byte (a channel-broadcast mask is read once per channel
// plane).  The same inputs give the same bits.
//
// LDS layout and banks.  The fp64 planes are read with ds_read_b64, bank = (a/4) % 64, conflicts within a 32-lane half.  A half
// is one tile row (lx = 0 .. 31) in both passes, so it reads or writes 32 consecutive doubles = 256 contiguous bytes = every one of
// the 64 banks once, whatever row it is: the pitch is MET_TW = 32 doubles with no padding, and this is why the tile is 32 wide.
// The fp32 planes are read with ds_read_b32, bank = (a/4) % 32; a half reads 32 consecutive dwords at column offset k = 0 .. 4, again
// every bank once at any pitch, so the pitch is the staged width MET_TW + 4 = 36 and the staging loop writes consecutive dwords.
// 2 * 20*36*4 + 5 * 20*32*8 + 256 for the reduction = 31 616 bytes per workgroup, five workgroups per CU.
//
// Arithmetic.  The input transform and d = x - y are fp32 with one rounding per operation (contraction is off below; min / max are
// written as comparisons so that a NaN stays a NaN).  Everything after is fp64: a product of two fp32 values is exact there, so
// each filtered value carries one rounding per tap and pass, and s = e - mu^2 keeps ~1e-16 where the reference's fp32 form keeps
// ~1e-7 against C2 = 9e-4 (INTEGRATION R).  Timing: profiles/metrics_timing.json; the kernel is bound by the fp64 window arithmetic
// and its LDS reads, not by HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_reduce.h"

#pragma clang fp contract(off)

#define MET_THREADS 256
#define MET_TW 32
#define MET_TH 16
#define MET_R 2                       // halo of the 5-tap window
#define MET_SW (MET_TW + 2 * MET_R)   // 36 staged columns = the fp32 pitch
#define MET_SH (MET_TH + 2 * MET_R)   // 20 staged rows
static_assert(MET_TW == 32, "a 32-lane half is one tile row: 32 consecutive doubles cover the 64 banks once");
static_assert(MET_THREADS == MET_TW * MET_TH / 2, "two pixels per thread");

__device__ __forceinline__ float met_transform(float x, int flags)
{
    if (flags & GSR_METRICS_CLAMP) x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);  // NaN fails both comparisons and stays
    if (flags & GSR_METRICS_QUANTIZE) {
        float q = x * 255.0f;
        q = q + 0.5f;
        q = q < 0.0f ? 0.0f : (q > 255.0f ? 255.0f : q);
        x = truncf(q) / 255.0f;
    }
    return x;
}

// reflect without repeating the edge; the clamp behind it only serves staged positions that no pixel of the image reads (a partial
// tile's far side), where the reflection itself can leave the image
__device__ __forceinline__ int met_reflect(int g, int n)
{
    g = g < 0 ? -g : g;
    g = g >= n ? 2 * (n - 1) - g : g;
    return min(max(g, 0), n - 1);
}

struct met_taps { double g0, g1, g2; };  // g_k = g_{4-k}

__global__ void __launch_bounds__(MET_THREADS) metrics_tile_kernel(int H, int W, int C, int tiles_x, const float* __restrict__ pred,
                                                                   const float* __restrict__ gt, const uint8_t* __restrict__ mask,
                                                                   long long mask_stride_b, long long mask_stride_c, int flags, met_taps taps,
                                                                   double* __restrict__ partials)
{
    __shared__ float xs[MET_SH * MET_SW], ys[MET_SH * MET_SW];
    __shared__ double hp[5][MET_SH * MET_TW];
    const int tile = (int)blockIdx.x, plane = (int)blockIdx.y;  // plane = b*C + c
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int x0 = tile_x * MET_TW, y0 = tile_y * MET_TH;
    const size_t hw = (size_t)H * (size_t)W, base = (size_t)plane * hw;
    const double g[5] = {taps.g0, taps.g1, taps.g2, taps.g1, taps.g0};

    for (int e = threadIdx.x; e < MET_SH * MET_SW; e += MET_THREADS) {
        const int ty = e / MET_SW, tx = e - ty * MET_SW;
        const int gy = met_reflect(y0 + ty - MET_R, H), gx = met_reflect(x0 + tx - MET_R, W);
        const size_t a = base + (size_t)gy * (size_t)W + (size_t)gx;  // < B*C*H*W
        xs[e] = met_transform(pred[a], flags);
        ys[e] = met_transform(gt[a], flags);
    }
    __syncthreads();

    for (int e = threadIdx.x; e < MET_SH * MET_TW; e += MET_THREADS) {
        const int row = e >> 5, col = e & (MET_TW - 1);
        double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const double x = (double)xs[row * MET_SW + col + k], y = (double)ys[row * MET_SW + col + k];
            m1 = fma(g[k], x, m1);
            m2 = fma(g[k], y, m2);
            e11 = fma(g[k], x * x, e11);  // (x*x, y*y, x*y are exact)
            e22 = fma(g[k], y * y, e22);
            e12 = fma(g[k], x * y, e12);
        }
        hp[0][e] = m1;
        hp[1][e] = m2;
        hp[2][e] = e11;
        hp[3][e] = e22;
        hp[4][e] = e12;
    }
    __syncthreads();

    const int b = plane / C, c = plane - b * C;
    const uint8_t* mrow = mask ? mask + (size_t)b * (size_t)mask_stride_b + (size_t)c * (size_t)mask_stride_c : nullptr;
    const int lx = threadIdx.x & (MET_TW - 1);
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // n, |d|, d^2, dssim, then the same under the mask
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int ly = (int)(threadIdx.x >> 5) + p * (MET_TH / 2);
        const int px = x0 + lx, py = y0 + ly;
        if (px >= W || py >= H) continue;
        double m1 = 0.0, m2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int l = (ly + k) * MET_TW + lx;
            m1 = fma(g[k], hp[0][l], m1);
            m2 = fma(g[k], hp[1][l], m2);
            e11 = fma(g[k], hp[2][l], e11);
            e22 = fma(g[k], hp[3][l], e22);
            e12 = fma(g[k], hp[4][l], e12);
        }
        const double m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        const double s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
        const double num = (2.0 * m12 + 1e-4) * (2.0 * s12 + 9e-4);
        const double den = ((m11 + m22) + 1e-4) * ((s1 + s2) + 9e-4) + 1e-12;
        double ds = (1.0 - num / den) / 2.0;
        ds = ds < 0.0 ? 0.0 : (ds > 1.0 ? 1.0 : ds);  // NaN stays
        const int l = (ly + MET_R) * MET_SW + lx + MET_R;
        const float d = xs[l] - ys[l];
        const double ad = (double)fabsf(d), dd = (double)d * (double)d;
        const bool in_mask = mrow ? mrow[(size_t)py * (size_t)W + (size_t)px] != 0 : true;
        acc[0] += 1.0;
        acc[1] += ad;
        acc[2] += dd;
        acc[3] += ds;
        if (in_mask) {  // selected, not multiplied: a NaN outside the mask stays outside
            acc[4] += 1.0;
            acc[5] += ad;
            acc[6] += dd;
            acc[7] += ds;
        }
    }
    gsr_block_reduce<MET_THREADS>(acc, gsr_add());
    if (threadIdx.x == 0) {
        double* out = partials + ((size_t)plane * (size_t)gridDim.x + (size_t)tile) * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) out[q] = acc[q];
    }
}

__global__ void __launch_bounds__(MET_THREADS) metrics_finish_kernel(int per_image /* C * tiles */, const double* __restrict__ partials,
                                                                     double* __restrict__ sums, float* __restrict__ metrics)
{
    const int b = (int)blockIdx.x;
    const double* in = partials + (size_t)b * (size_t)per_image * 8;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < per_image; i += MET_THREADS)
#pragma unroll
        for (int q = 0; q < 8; q++) acc[q] += in[(size_t)i * 8 + q];
    gsr_block_reduce<MET_THREADS>(acc, gsr_add());
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int q = 0; q < 8; q++) sums[(size_t)b * 8 + q] = acc[q];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const double n = acc[4 * h], l1 = acc[4 * h + 1] / n, mse = acc[4 * h + 2] / n;  // n == 0: 0/0 = NaN
        float* m = metrics + (size_t)b * 8 + 4 * h;
        m[0] = (float)l1;
        m[1] = (float)mse;
        m[2] = (float)(-10.0 * log10(mse));  // mse == 0: +inf
        m[3] = (float)(1.0 - 2.0 * (acc[4 * h + 3] / n));
    }
}

// workspace[(b*C + c)*tiles + tile]: the eight sums of each tile, nothing between them
struct MetWork { double* partials; int tiles_x, tiles; size_t bytes; };
static MetWork met_carve(void* base, int B, int C, int H, int W)
{
    GsrCarver c(base);
    const int tiles_x = (W + MET_TW - 1) / MET_TW, tiles_y = (H + MET_TH - 1) / MET_TH;  // tiles_x * tiles_y < 2^31 / 3: C*H*W < 2^31
    double* partials = c.take<double>((size_t)B * (size_t)C * (size_t)tiles_x * (size_t)tiles_y * 8, sizeof(double));
    return { partials, tiles_x, tiles_x * tiles_y, c.total() };
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
static int metrics_check_sizes(int B, int C, int H, int W)
{
    if (B <= 0 || C <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: B=%d C=%d (need both > 0)", B, C);
    if ((int64_t)B * (int64_t)C > 65535)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: B=%d C=%d has too many planes (need B*C <= 65535)", B, C);
    if (H < 3 || W < 3) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: H=%d W=%d (need both >= 3: reflect padding of 2)", H, W);
    if ((double)C * (double)H * (double)W >= 2147483392.0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: C=%d H=%d W=%d has too many elements (need C*H*W < 2^31 - 256)", C, H, W);
    // (no accepted size wraps the carve: 65535 planes of fewer than 2^22 tiles, 64 bytes each)
    return GSR_OK;
}

extern "C" size_t gsr_image_metrics_workspace_bytes(int B, int C, int H, int W)
{
    if (metrics_check_sizes(B, C, H, W)) return 0;
    return met_carve(nullptr, B, C, H, W).bytes;
}

extern "C" int gsr_image_metrics(int B, int C, int H, int W, const float* pred, const float* gt, const uint8_t* mask, long long mask_stride_b,
                                 long long mask_stride_c, int flags, void* workspace, double* sums, float* metrics, void* stream_)
{
    if (int rc = metrics_check_sizes(B, C, H, W)) return rc;
    if (!pred || !gt || !workspace || !sums || !metrics)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: pred, gt, workspace, sums or metrics is NULL");
    if (flags & ~(GSR_METRICS_CLAMP | GSR_METRICS_QUANTIZE)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: unknown flag bits in %d", flags);
    if (mask_stride_b < 0 || mask_stride_c < 0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: negative mask stride (%lld, %lld)", mask_stride_b, mask_stride_c);
    double taps[3], total = 0.0;  // g_k = exp(-(k-2)^2 / 4.5) / sum, k = 0 .. 4 (sigma 1.5), in fp64
    for (int k = 0; k < 3; k++) taps[k] = exp(-(double)((k - 2) * (k - 2)) / 4.5);
    total = ((taps[0] + taps[1]) + taps[2]) + (taps[1] + taps[0]);
    for (int k = 0; k < 3; k++) taps[k] /= total;
    hipStream_t stream = (hipStream_t)stream_;
    const MetWork w = met_carve(workspace, B, C, H, W);
    const int tiles_x = w.tiles_x, tiles = w.tiles;
    met_taps t = {taps[0], taps[1], taps[2]};
    hipLaunchKernelGGL(metrics_tile_kernel, dim3((uint32_t)tiles, (uint32_t)(B * C)), dim3(MET_THREADS), 0, stream, H, W, C, tiles_x, pred, gt,
                       mask, mask_stride_b, mask_stride_c, flags, t, w.partials);
    GSR_HIP(hipGetLastError(), "image metrics");
    hipLaunchKernelGGL(metrics_finish_kernel, dim3((uint32_t)B), dim3(MET_THREADS), 0, stream, C * tiles, (const double*)w.partials, sums, metrics);
    GSR_HIP(hipGetLastError(), "image metrics");
    return GSR_OK;
}
