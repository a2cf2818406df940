// frames.hip -- what render_set (train.py:710-848) does between the render and the PNG encoder, as finished uint8 pictures on the
// device: save_image's quantisation, the error map, the normal picture's second normalisation, compute_scale_and_shift (:198-218),
// the two colour maps (cv2.applyColorMap, plt.imsave), the flips, the one-channel expand and the concat.  The rules are in
// include/gsraster.h in full.
//
// The reference does this per frame in eager torch and on the host: a min, a max, four fp32 .cpu() copies (22.9 MB at 567 x 1008 for a
// 6.9 MB file), numpy and cv2 on the CPU, five masked sums with a nonzero (a host stop) and matplotlib for the depth panel.  Here:
//   stats    : partial -- one workgroup per FRAME_STATS_CHUNK = 4096 elements of a frame reads depth (and target, mask) once and
//              writes eight doubles {a00, a01, a11, b0, b1, lo, hi, NaN count}, reduced in a fixed order (a thread's elements in
//              order, xor-butterfly over the wave, the four waves in order); finish -- one workgroup per frame reduces the frame's
//              partials the same way and writes stats[b] and params[b].  With a target both run a second time for lo2 / hi2 of the
//              [aligned | target] panel, reading scale and shift from params[b] on the device.
//   compose  : one thread makes four consecutive output pixels of one row.  The panel table travels in the kernel arguments; the
//              loop over panels is uniform (scalar loads of the table), a lane takes part in the panels its pixels lie in, so a wave
//              diverges only where it straddles a panel edge.  Sources are read through signed strides (flip, expand, interleaved
//              normals); stores are whole dwords (three for 4 RGB pixels, one per RGBA pixel) or bytes, a template argument.
// No atomics, nothing read back, the same bits for the same inputs.  Both are bound by memory traffic: 4 .. 12 bytes read and 3 .. 4
// written per output pixel.
//
// Arithmetic: every fp32 operation below rounds once (contraction is off from the pragma on; min / max are comparisons, so a NaN
// stays where the rules keep it), `/` is the IEEE division and sqrtf the correctly rounded root, as in adam.hip.  fp32 denormals are
// kept (the default kernel mode).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_reduce.h"

#pragma clang fp contract(off)

#define FRM_THREADS 256
// Stats: one workgroup per FRAME_STATS_CHUNK elements of a frame writes eight doubles {a00, a01, a11, b0, b1, lo, hi, NaN count}: the
// workspace is B*chunks*8 doubles, used again by the second pass (lo2 / hi2).
#define FRAME_STATS_CHUNK 4096
static_assert(FRAME_STATS_CHUNK % FRM_THREADS == 0, "every thread of a full chunk reads the same number of elements");
static_assert(sizeof(gsr_frame_panel) == 72, "gsr_frame_panel is 3 pointers, 4 strides and 3 ints (padded to 8 bytes)");

struct FrmTable {
    gsr_frame_panel p[GSR_FRAME_MAX_PANELS];
    int32_t n;
};
static_assert(sizeof(FrmTable) <= 1024, "the table travels in the kernel arguments");

// ---- stats ----
// slots 0 .. 4 and 7 add, 5 takes the minimum, 6 the maximum (never NaN: the comparisons that fill them reject it)
struct frm_join {
    __device__ __forceinline__ double operator()(int q, double a, double b) const
    {
        if (q == 5) return b < a ? b : a;
        if (q == 6) return b > a ? b : a;
        return a + b;
    }
};

__device__ __forceinline__ void frm_extrema(float x, double (&acc)[8])
{
    const double v = (double)x;
    acc[5] = v < acc[5] ? v : acc[5];
    acc[6] = v > acc[6] ? v : acc[6];
    acc[7] += x != x ? 1.0 : 0.0;
}

#define FRM_ACC_INIT {0.0, 0.0, 0.0, 0.0, 0.0, __builtin_huge_val(), -__builtin_huge_val(), 0.0}

// PASS 1: the five sums and the extrema of depth.  PASS 2: the extrema of [depth*scale + shift | target], scale / shift from params.
template <int PASS>
__global__ void __launch_bounds__(FRM_THREADS) frame_stats_partial_kernel(int HW, const float* __restrict__ depth, const float* __restrict__ target,
                                                                          const float* __restrict__ mask, const float* __restrict__ params,
                                                                          double* __restrict__ partials)
{
    const int b = (int)blockIdx.y;
    const size_t base = (size_t)b * (size_t)HW;
    const int start = (int)blockIdx.x * FRAME_STATS_CHUNK;  // < HW < 2^29
    const int end = min(start + FRAME_STATS_CHUNK, HW);
    float scale = 0.0f, shift = 0.0f;
    if (PASS == 2) {
        scale = params[(size_t)b * 8 + 2];
        shift = params[(size_t)b * 8 + 3];
    }
    double acc[8] = FRM_ACC_INIT;
    for (int i = start + (int)threadIdx.x; i < end; i += FRM_THREADS) {
        const float d = depth[base + (size_t)i];
        if (PASS == 1) {
            frm_extrema(d, acc);
            if (target) {
                const float y = target[base + (size_t)i];
                const float m = mask ? mask[base + (size_t)i] : 1.0f;
                const double dd = (double)d, md = (double)m * dd;  // (exact)
                acc[0] += md * dd;
                acc[1] += md;
                acc[2] += (double)m;
                acc[3] += md * (double)y;
                acc[4] += (double)m * (double)y;
            }
        } else {
            float a = d * scale;
            a = a + shift;
            frm_extrema(a, acc);
            frm_extrema(target[base + (size_t)i], acc);
        }
    }
    gsr_block_reduce<FRM_THREADS>(acc, frm_join());
    if (threadIdx.x == 0) {
        double* out = partials + ((size_t)b * (size_t)gridDim.x + (size_t)blockIdx.x) * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) out[q] = acc[q];
    }
}

template <int PASS>
__global__ void __launch_bounds__(FRM_THREADS) frame_stats_finish_kernel(int chunks, const double* __restrict__ partials, double* __restrict__ stats,
                                                                         float* __restrict__ params)
{
    const int b = (int)blockIdx.x;
    const double* in = partials + (size_t)b * (size_t)chunks * 8;
    double acc[8] = FRM_ACC_INIT;
    for (int i = threadIdx.x; i < chunks; i += FRM_THREADS)
#pragma unroll
        for (int q = 0; q < 8; q++) acc[q] = frm_join()(q, acc[q], in[(size_t)i * 8 + q]);
    gsr_block_reduce<FRM_THREADS>(acc, frm_join());
    if (threadIdx.x != 0) return;
    const float nan = __builtin_nanf("");
    const float lo = acc[7] > 0.0 ? nan : (float)acc[5], hi = acc[7] > 0.0 ? nan : (float)acc[6];  // (fp32 values: the casts are exact)
    float* p = params + (size_t)b * 8;
    if (PASS == 2) {
        p[4] = lo;
        p[5] = hi;
        return;
    }
    const double a00 = acc[0], a01 = acc[1], a11 = acc[2], b0 = acc[3], b1 = acc[4];
    const double det = a00 * a11 - a01 * a01;
    double x0 = 0.0, x1 = 0.0;
    if (det != 0.0) {  // (a NaN determinant is "nonzero", as in the reference: the quotients are NaN)
        x0 = (a11 * b0 - a01 * b1) / det;
        x1 = (-a01 * b0 + a00 * b1) / det;
    }
    double* s = stats + (size_t)b * 8;
    s[0] = a00;
    s[1] = a01;
    s[2] = a11;
    s[3] = b0;
    s[4] = b1;
    s[5] = det;
    s[6] = x0;
    s[7] = x1;
    p[0] = lo;
    p[1] = hi;
    p[2] = fabsf((float)x0);
    p[3] = (float)x1;
    p[4] = p[5] = p[6] = p[7] = 0.0f;
}

// partials[(b*chunks + chunk)*8]: the eight doubles of each chunk, nothing between them
struct FrmStatsWork { double* partials; int chunks; size_t bytes; };
static FrmStatsWork frm_stats_carve(void* base, int B, int H, int W)
{
    GsrCarver c(base);
    const int chunks = (int)(((size_t)H * (size_t)W + FRAME_STATS_CHUNK - 1) / FRAME_STATS_CHUNK);
    double* partials = c.take<double>((size_t)B * (size_t)chunks * 8, sizeof(double));
    return { partials, chunks, c.total() };
}

// ---- compose ----
__device__ __forceinline__ float frm_clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }  // NaN fails both comparisons and stays

// trunc(min(max(v, 0), 255)) as an integer, NaN -> 0
__device__ __forceinline__ uint32_t frm_byte(float v)
{
    v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    return v == v ? (uint32_t)(int)v : 0u;
}

__device__ __forceinline__ uint32_t frm_quantise(float x)
{
    float v = x * 255.0f;
    v = v + 0.5f;
    return frm_byte(v);
}

__device__ __forceinline__ uint32_t frm_rgba(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return r | (g << 8) | (b << 16) | (a << 24); }

__device__ __forceinline__ uint32_t frm_lut(const uint8_t* __restrict__ lut, uint32_t i)
{
    return frm_rgba(lut[i * 3], lut[i * 3 + 1], lut[i * 3 + 2], 255u);
}

__device__ __forceinline__ uint32_t frm_map_mpl(float v, float lo, float hi, const uint8_t* __restrict__ lut)
{
    if (lo != lo || hi != hi) return 0u;
    if (hi == lo) return frm_lut(lut, 0u);
    const float den = (float)((double)hi - (double)lo);
    float t = (v - lo) / den;
    t = t * 256.0f;
    if (t != t) return 0u;
    t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);  // (int) trunc(t) clipped to 0 .. 255
    return frm_lut(lut, (uint32_t)(int)t);
}

// one output pixel as r | g << 8 | b << 16 | a << 24.  p is uniform over the wave; lx is the column inside the panel.
__device__ __forceinline__ uint32_t frm_pixel(const gsr_frame_panel& p, const float* __restrict__ pr, int b, int y, int lx)
{
    const long long at = (long long)b * p.stride_b + (long long)y * p.stride_y + (long long)lx * p.stride_x;
    const float* s = p.src + at;
    const long long sc = p.stride_c;
    switch (p.mode) {
    case GSR_FRAME_QUANT:
        return frm_rgba(frm_quantise(s[0]), frm_quantise(s[sc]), frm_quantise(s[2 * sc]), 255u);
    case GSR_FRAME_QUANT_CLAMP:
        return frm_rgba(frm_quantise(frm_clamp01(s[0])), frm_quantise(frm_clamp01(s[sc])), frm_quantise(frm_clamp01(s[2 * sc])), 255u);
    case GSR_FRAME_ABSDIFF: {
        const float* s2 = p.src2 + at;
        return frm_rgba(frm_quantise(fabsf(frm_clamp01(s[0]) - s2[0])), frm_quantise(fabsf(frm_clamp01(s[sc]) - s2[sc])),
                        frm_quantise(fabsf(frm_clamp01(s[2 * sc]) - s2[2 * sc])), 255u);
    }
    case GSR_FRAME_NORMAL: {
        const float x = s[0], yv = s[sc], z = s[2 * sc];
        float q = x * x;
        const float yy = yv * yv, zz = z * z;
        q = q + yy;
        q = q + zz;
        float r = sqrtf(q);
        r = r < 1e-12f ? 1e-12f : r;  // max(r, 1e-12) that keeps a NaN
        float c[3] = {x / r, yv / r, z / r};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            c[k] = c[k] + 1.0f;
            c[k] = c[k] / 2.0f;
        }
        return frm_rgba(frm_quantise(c[0]), frm_quantise(c[1]), frm_quantise(c[2]), 255u);
    }
    case GSR_FRAME_CMAP_CV: {
        const float lo = pr[0], hi = pr[1];
        uint32_t i = 0u;
        if (hi != lo && fabsf(lo) <= 3.402823466e38f && fabsf(hi) <= 3.402823466e38f) {  // both finite (a NaN fails the comparison)
            const float num = s[0] - lo, den = hi - lo;
            float t = num / den;
            t = 255.0f * t;
            i = frm_byte(t);
        }
        return frm_lut(p.lut, i);
    }
    case GSR_FRAME_CMAP_MPL_ALIGNED: {
        float v = s[0] * pr[2];
        v = v + pr[3];
        return frm_map_mpl(v, pr[4], pr[5], p.lut);
    }
    default:  // GSR_FRAME_CMAP_MPL (the caller has rejected every other value)
        return frm_map_mpl(s[0], pr[4], pr[5], p.lut);
    }
}

template <int CH, bool DWORDS>
__global__ void __launch_bounds__(FRM_THREADS) frame_compose_kernel(int H, int W_out, int quads /* ceil(W_out / 4) */, FrmTable tab,
                                                                    const float* __restrict__ params, uint8_t* __restrict__ out)
{
    const int t = (int)blockIdx.x * FRM_THREADS + (int)threadIdx.x;  // H * quads <= H * W_out < 2^29
    if (t >= H * quads) return;
    const int b = (int)blockIdx.y;
    const int y = t / quads, x = (t - y * quads) * 4;
    const int count = min(4, W_out - x);
    const float* pr = params ? params + (size_t)b * 8 : nullptr;  // (NULL only when no panel reads it)
    uint32_t px[4] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < tab.n; j++) {  // uniform: the table is read with scalar loads (checked in the gfx950 ISA: s_load from the kernel
                                       // arguments at a runtime offset, no scratch)
        const gsr_frame_panel& p = tab.p[j];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int lx = x + k - p.x0;
            if (k < count && lx >= 0 && lx < p.width) px[k] = frm_pixel(p, pr, b, y, lx);
        }
    }
    uint8_t* o = out + (((size_t)b * (size_t)H + (size_t)y) * (size_t)W_out + (size_t)x) * CH;
    if (DWORDS && CH == 4) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < count) ((uint32_t*)o)[k] = px[k];
    } else if (DWORDS) {  // CH == 3 and W_out % 4 == 0: count == 4, and o is a multiple of 12 bytes past the aligned base
        uint32_t* o32 = (uint32_t*)o;
        o32[0] = (px[0] & 0xffffffu) | (px[1] << 24);
        o32[1] = ((px[1] >> 8) & 0xffffu) | (px[2] << 16);
        o32[2] = ((px[2] >> 16) & 0xffu) | (px[3] << 8);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < count)
#pragma unroll
                for (int c = 0; c < CH; c++) o[k * CH + c] = (uint8_t)(px[k] >> (8 * c));
    }
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
static int frames_check_sizes(const char* what, int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: B=%d H=%d W=%d (need all > 0)", what, B, H, W);
    if (B > 65535) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: B=%d has too many frames (need B <= 65535)", what, B);
    if ((int64_t)H * (int64_t)W >= 0x7fffff00LL / 4)  // (H*W*4 itself can pass 2^63)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: H=%d W=%d has too many pixels (need H*W*4 < 2^31 - 256)", what, H, W);
    // (no accepted size wraps the carve: 65535 frames of fewer than 2^17 chunks, 64 bytes each)
    return GSR_OK;
}

extern "C" size_t gsr_frame_stats_workspace_bytes(int B, int H, int W)
{
    if (frames_check_sizes("frame stats", B, H, W)) return 0;
    return frm_stats_carve(nullptr, B, H, W).bytes;
}

extern "C" int gsr_frame_stats(int B, int H, int W, const float* depth, const float* target, const float* lsq_mask, void* workspace,
                               double* stats, float* params, void* stream_)
{
    if (int rc = frames_check_sizes("frame stats", B, H, W)) return rc;
    if (!depth || !workspace || !stats || !params)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame stats: depth, workspace, stats or params is NULL");
    if (lsq_mask && !target) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame stats: an lsq_mask needs a target, which is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    const int HW = H * W;  // < 2^29
    const FrmStatsWork w = frm_stats_carve(workspace, B, H, W);
    const int chunks = w.chunks;
    double* const partials = w.partials;
    const dim3 grid((uint32_t)chunks, (uint32_t)B);
    hipLaunchKernelGGL(frame_stats_partial_kernel<1>, grid, dim3(FRM_THREADS), 0, stream, HW, depth, target, lsq_mask, (const float*)nullptr, partials);
    GSR_HIP(hipGetLastError(), "frame stats");
    hipLaunchKernelGGL(frame_stats_finish_kernel<1>, dim3((uint32_t)B), dim3(FRM_THREADS), 0, stream, chunks, (const double*)partials, stats, params);
    GSR_HIP(hipGetLastError(), "frame stats");
    if (!target) return GSR_OK;
    hipLaunchKernelGGL(frame_stats_partial_kernel<2>, grid, dim3(FRM_THREADS), 0, stream, HW, depth, target, (const float*)nullptr, (const float*)params,
                       partials);
    GSR_HIP(hipGetLastError(), "frame stats");
    hipLaunchKernelGGL(frame_stats_finish_kernel<2>, dim3((uint32_t)B), dim3(FRM_THREADS), 0, stream, chunks, (const double*)partials, stats, params);
    GSR_HIP(hipGetLastError(), "frame stats");
    return GSR_OK;
}

extern "C" int gsr_frame_compose(int B, int H, int W_out, int channels_out, int n, const gsr_frame_panel* panels, const float* params,
                                 uint8_t* out, void* stream_)
{
    if (int rc = frames_check_sizes("frame compose", B, H, W_out)) return rc;
    if (channels_out != 3 && channels_out != 4)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: channels_out=%d (need 3 or 4)", channels_out);
    if (n < 1 || n > GSR_FRAME_MAX_PANELS)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: n=%d panels (need 1 .. %d)", n, GSR_FRAME_MAX_PANELS);
    if (!panels || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panels or out is NULL");
    int order[GSR_FRAME_MAX_PANELS];
    for (int j = 0; j < n; j++) {
        const gsr_frame_panel& p = panels[j];
        if (p.mode < GSR_FRAME_QUANT || p.mode > GSR_FRAME_CMAP_MPL)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d has the unknown mode %d", j, p.mode);
        if (!p.src) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d has a NULL src", j);
        if (p.mode == GSR_FRAME_ABSDIFF && !p.src2) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d is ABSDIFF with a NULL src2", j);
        if (p.mode >= GSR_FRAME_CMAP_CV && (!p.lut || !params))
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d has a CMAP mode with a NULL lut or params", j);
        if (p.width <= 0 || p.x0 < 0 || (int64_t)p.x0 + (int64_t)p.width > (int64_t)W_out)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d covers columns [%d, %lld), outside [0, %d) or empty", j, p.x0,
                            (long long)p.x0 + (long long)p.width, W_out);
        int k = j;  // insertion by x0
        for (; k > 0 && panels[order[k - 1]].x0 > p.x0; k--) order[k] = order[k - 1];
        order[k] = j;
    }
    int next = 0;
    for (int k = 0; k < n; k++) {
        const gsr_frame_panel& p = panels[order[k]];
        if (p.x0 != next)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d starts at column %d where %d is next (the panels %s)", order[k], p.x0,
                            next, p.x0 < next ? "overlap" : "leave a gap");
        next = p.x0 + p.width;
    }
    if (next != W_out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: the panels end at column %d of %d (they leave a gap)", next, W_out);
    const bool dwords = ((uintptr_t)out & 3) == 0 && (channels_out == 4 || W_out % 4 == 0);
    hipStream_t stream = (hipStream_t)stream_;
    FrmTable tab = {};
    for (int j = 0; j < n; j++) tab.p[j] = panels[j];
    tab.n = n;
    const int quads = (W_out + 3) / 4;
    const dim3 grid((uint32_t)(((long long)H * quads + FRM_THREADS - 1) / FRM_THREADS), (uint32_t)B), block(FRM_THREADS);
    if (channels_out == 4) {
        if (dwords) hipLaunchKernelGGL((frame_compose_kernel<4, true>), grid, block, 0, stream, H, W_out, quads, tab, params, out);
        else hipLaunchKernelGGL((frame_compose_kernel<4, false>), grid, block, 0, stream, H, W_out, quads, tab, params, out);
    } else {
        if (dwords) hipLaunchKernelGGL((frame_compose_kernel<3, true>), grid, block, 0, stream, H, W_out, quads, tab, params, out);
        else hipLaunchKernelGGL((frame_compose_kernel<3, false>), grid, block, 0, stream, H, W_out, quads, tab, params, out);
    }
    GSR_HIP(hipGetLastError(), "frame compose");
    return GSR_OK;
}
