// anchor_adjust.hip -- the pruning half of GScream's densification: GaussianModel.adjust_anchor around its anchor_growing call, with
// prune_anchor / _prune_anchor_optimizer (scene/gaussian_model.py:914-973, :762-805).
//
// The reference compacts about 1 KB per anchor with ~26 boolean-mask gathers (7 parameters and their 2 Adam moments each, 5
// accumulators), every one a nonzero and a size read-back.  Here:
//   gaa_offsets_kernel   :916-919  grads_norm = |accum / denom| (NaN -> 0), offset_mask = denom > threshold       over the N0 K offset rows
//   gaa_flag_kernel      :937-939  prune / reset per anchor, keep flags, block counts                           over the N1 anchors after growth
//   gaa_top_scan_kernel            exclusive scan of the block counts, info = {n_keep, n_prune, n_reset, 0}
//   gaa_place_kernel               keep_rows[position among the kept] = anchor (ascending)
//   gaa_gather_kernel    :942-968, :770-788  every tensor's kept rows in ONE launch, driven by a table of copies passed by value, rows in
//                        16-, 8- or 4-byte units (whichever the row width and the pointers allow); the offset resets and zero padding
//                        (:924-934), the anchor resets (:953-956) and the scaling clamp (:776-780) ride on it
// Scans and ranks are gsr_scan.h's.  No atomics, one fixed association order: repeated calls give identical bits.
//
// Exactness.  accum / denom is the IEEE division (__fdiv_rn); min_opacity * anchor_demon is one fp32 product (__fmul_rn) of the
// scalar rounded to fp32, as torch multiplies a float tensor by a Python scalar; the thresholds arrive rounded to fp32, as torch
// compares a float tensor with a Python scalar.  Nothing here can contract into an FMA.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_scan.h"

#define GAA_THREADS 256                      // anchors per block of the flag / place kernels (one per thread)
#define GAA_PER_THREAD 8                     // stream units (4, 2 or 1 floats) per thread of the gather
#define GAA_CHUNK (GAA_THREADS * GAA_PER_THREAD)

static inline int gaa_blocks(long long n, int per) { return (int)((n + per - 1) / per); }

// ---- :916-919 ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GAA_THREADS) gaa_offsets_kernel(int L0, const float* __restrict__ accum, const float* __restrict__ denom,
                                                                  float thr_half, float* __restrict__ grads_norm,
                                                                  uint8_t* __restrict__ offset_mask)
{
    const int i = blockIdx.x * GAA_THREADS + threadIdx.x;
    if (i >= L0) return;
    const float d = denom[i];
    float g = __fdiv_rn(accum[i], d);
    if (g != g) g = 0.0f;
    grads_norm[i] = fabsf(g);
    offset_mask[i] = (uint8_t)(d > thr_half);
}

// ---- plan: flags, top scan, place ------------------------------------------------------------------------------------------
// one 64-bit value per anchor: low word = kept, high word = reset (counts <= N < 2^31 each)
__global__ void __launch_bounds__(GAA_THREADS) gaa_flag_kernel(int N, const float* __restrict__ opacity_accum, const float* __restrict__ anchor_demon,
                                                               const uint8_t* __restrict__ prune_mask, float min_opacity, float thr,
                                                               uint8_t* __restrict__ keep, uint8_t* __restrict__ reset,
                                                               unsigned long long* __restrict__ block_sum)
{
    const long long i = (long long)blockIdx.x * GAA_THREADS + threadIdx.x;
    bool k = false, r = false;
    if (i < N) {
        if (prune_mask) {
            k = prune_mask[i] == 0;
        } else {
            const float demon = anchor_demon[i];
            r = demon > thr;
            k = !(opacity_accum[i] < __fmul_rn(demon, min_opacity) && r);
        }
        keep[i] = (uint8_t)k;
        reset[i] = (uint8_t)r;
    }
    unsigned long long tot;
    (void)gsr_block_scan_excl<GAA_THREADS>((unsigned long long)k | ((unsigned long long)r << 32), &tot);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(1024) gaa_top_scan_kernel(int N, int nb, unsigned long long* __restrict__ block_sum, int32_t* __restrict__ info)
{
    const unsigned long long tot = gsr_top_scan(nb, block_sum);
    if (threadIdx.x == 0) {
        const int32_t n_keep = (int32_t)(uint32_t)tot;
        info[0] = n_keep;
        info[1] = N - n_keep;
        info[2] = (int32_t)(uint32_t)(tot >> 32);
        info[3] = 0;
    }
}

__global__ void __launch_bounds__(GAA_THREADS) gaa_place_kernel(int N, const uint8_t* __restrict__ keep,
                                                                const unsigned long long* __restrict__ block_base, int32_t* __restrict__ keep_rows)
{
    const long long i = (long long)blockIdx.x * GAA_THREADS + threadIdx.x;
    const bool k = i < N && keep[i] != 0;
    const uint32_t pos = (uint32_t)block_base[blockIdx.x] + gsr_block_rank<GAA_THREADS>(k);  // low word: the kept anchors before this block
    if (k) keep_rows[pos] = (int32_t)i;  // pos < n_keep <= N
}

struct GaaWork {
    unsigned long long* block_sum;  // [blocks(N) + 1]
    uint8_t* keep;                  // [N]
    size_t bytes;
};

static GaaWork gaa_carve(void* base, int N)
{
    GaaWork w{};
    GsrCarver c(base);
    w.block_sum = c.take<unsigned long long>((size_t)gaa_blocks(N, GAA_THREADS) + 1);
    w.keep = c.take<uint8_t>((size_t)N);
    w.bytes = c.total();
    return w;
}

// ---- gather ----------------------------------------------------------------------------------------------------------------
// The table travels in the kernel arguments.  Copy c owns the blocks [first[c], first[c + 1]); a block moves GAA_CHUNK consecutive
// units of its copy's destination stream, thread t the units t, t + 256, ...: every store instruction is contiguous over the wave.
// A unit is vec[c] = 4, 2 or 1 floats: the widest that divides the row width with both base pointers aligned to it (the host
// checks; a row then starts on a unit boundary in the source and in the destination).  The two statistics modes move single floats.
struct GaaTable {
    gsr_adjust_copy copy[GSR_ADJUST_MAX_COPIES];
    uint32_t first[GSR_ADJUST_MAX_COPIES + 1];
    uint8_t vec[GSR_ADJUST_MAX_COPIES];
    int32_t n;
};

// COPY / CLAMP_TAIL in units of V floats.  A unit beyond the stream reads unit 0 instead (the stream is not empty), so that no load
// sits behind a branch and all of a thread's loads are in flight together.
template <int V>
__device__ __forceinline__ void gaa_move_rows(const float* __restrict__ src_f, float* __restrict__ dst_f, uint32_t width_f, bool clamp_tail,
                                              uint32_t block, int n_keep, const int32_t* __restrict__ keep_rows)
{
    typedef float unit_t __attribute__((ext_vector_type(V)));
    const unit_t* __restrict__ src = (const unit_t*)src_f;
    unit_t* __restrict__ dst = (unit_t*)dst_f;
    const uint32_t width = width_f / V, total = (uint32_t)n_keep * width;  // in units
    const uint32_t e0 = block * (uint32_t)GAA_CHUNK + threadIdx.x;
    uint32_t col[GAA_PER_THREAD], s[GAA_PER_THREAD];
    unit_t v[GAA_PER_THREAD];
#pragma unroll
    for (int j = 0; j < GAA_PER_THREAD; j++) {
        const uint32_t e = e0 + (uint32_t)j * GAA_THREADS, ec = e < total ? e : 0u;
        const uint32_t row = ec / width;
        col[j] = ec - row * width;
        s[j] = (uint32_t)keep_rows[row] * width + col[j];  // keep_rows[] < N and N * width_f < 2^31 (checked by the caller)
    }
#pragma unroll
    for (int j = 0; j < GAA_PER_THREAD; j++) v[j] = src[s[j]];
    if (clamp_tail) {
#pragma unroll
        for (int j = 0; j < GAA_PER_THREAD; j++)
#pragma unroll
            for (int k = 0; k < V; k++) v[j][k] = (col[j] * V + k >= 3u && v[j][k] > 0.05f) ? 0.05f : v[j][k];
    }
#pragma unroll
    for (int j = 0; j < GAA_PER_THREAD; j++) {
        const uint32_t e = e0 + (uint32_t)j * GAA_THREADS;
        if (e < total) dst[e] = v[j];
    }
}

// OFFSET_STAT / ANCHOR_STAT, single floats (a tenth of the traffic)
__device__ __forceinline__ void gaa_move_stats(const float* __restrict__ src, float* __restrict__ dst, uint32_t width, bool per_offset,
                                               uint32_t block, int n_keep, const int32_t* __restrict__ keep_rows,
                                               const uint8_t* __restrict__ offset_mask, int L0, const uint8_t* __restrict__ reset)
{
    const uint32_t total = (uint32_t)n_keep * width;
    const uint32_t e0 = block * (uint32_t)GAA_CHUNK + threadIdx.x;
#pragma unroll
    for (int j = 0; j < GAA_PER_THREAD; j++) {
        const uint32_t e = e0 + (uint32_t)j * GAA_THREADS;
        if (e >= total) break;
        const uint32_t row = e / width, col = e - row * width;
        const uint32_t a = (uint32_t)keep_rows[row], s = a * width + col;
        float v = 0.0f;
        if (per_offset) {
            if (s < (uint32_t)L0 && !offset_mask[s]) v = src[s];
        } else if (!reset[a]) {
            v = src[s];
        }
        dst[e] = v;
    }
}

__global__ void __launch_bounds__(GAA_THREADS) gaa_gather_kernel(const GaaTable tab, int n_keep, const int32_t* __restrict__ keep_rows,
                                                                 const uint8_t* __restrict__ offset_mask, int L0, const uint8_t* __restrict__ reset)
{
    int c = 0;
    while (c + 1 < tab.n && blockIdx.x >= tab.first[c + 1]) c++;  // (uniform: at most 31 scalar steps)
    const uint32_t block = blockIdx.x - tab.first[c];
    const float* src = tab.copy[c].src;
    float* dst = tab.copy[c].dst;
    const uint32_t width = (uint32_t)tab.copy[c].width;
    const int mode = tab.copy[c].mode, vec = tab.vec[c];
    if (mode >= GSR_ADJUST_OFFSET_STAT) gaa_move_stats(src, dst, width, mode == GSR_ADJUST_OFFSET_STAT, block, n_keep, keep_rows, offset_mask, L0, reset);
    else if (vec == 4) gaa_move_rows<4>(src, dst, width, mode == GSR_ADJUST_CLAMP_TAIL, block, n_keep, keep_rows);
    else if (vec == 2) gaa_move_rows<2>(src, dst, width, mode == GSR_ADJUST_CLAMP_TAIL, block, n_keep, keep_rows);
    else gaa_move_rows<1>(src, dst, width, mode == GSR_ADJUST_CLAMP_TAIL, block, n_keep, keep_rows);
}

static int gaa_unit(const gsr_adjust_copy& d)
{
    if (d.mode != GSR_ADJUST_COPY && d.mode != GSR_ADJUST_CLAMP_TAIL) return 1;
    const uintptr_t bits = (uintptr_t)d.src | (uintptr_t)d.dst;
    if (d.width % 4 == 0 && bits % 16 == 0) return 4;
    if (d.width % 2 == 0 && bits % 8 == 0) return 2;
    return 1;
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
extern "C" size_t gsr_anchor_adjust_workspace_bytes(int N)
{
    if (N < 0 || N > 0x7fffff00) return 0;  // (no accepted N wraps the carve: N bytes + N / 256 sums)
    return gaa_carve(nullptr, N).bytes;
}

extern "C" int gsr_anchor_adjust_offsets(int L0, const float* offset_gradient_accum, const float* offset_denom, float denom_threshold,
                                         float* grads_norm, uint8_t* offset_mask, void* stream)
{
    if (L0 < 0 || L0 > 0x7fffff00) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust offsets: bad size L0=%d", L0);
    if (L0 > 0 && (!offset_gradient_accum || !offset_denom || !grads_norm || !offset_mask))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust offsets: a required pointer is NULL");
    if (L0 == 0) return GSR_OK;
    hipLaunchKernelGGL(gaa_offsets_kernel, dim3(gaa_blocks(L0, GAA_THREADS)), dim3(GAA_THREADS), 0, (hipStream_t)stream, L0, offset_gradient_accum,
                       offset_denom, denom_threshold, grads_norm, offset_mask);
    GSR_HIP(hipGetLastError(), "anchor adjust offsets");
    return GSR_OK;
}

extern "C" int gsr_anchor_adjust_plan(int N, const float* opacity_accum, const float* anchor_demon, const uint8_t* prune_mask,
                                      float min_opacity, float demon_threshold, void* workspace, int32_t* keep_rows, uint8_t* reset,
                                      int32_t* info, void* stream_)
{
    if (N < 0 || N > 0x7fffff00) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust plan: bad size N=%d", N);
    if (!info || (N > 0 && (!workspace || !keep_rows || !reset || (!prune_mask && (!opacity_accum || !anchor_demon)))))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust plan: a required pointer is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    if (N == 0) { GSR_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int32_t), stream), "anchor adjust plan"); return GSR_OK; }
    const GaaWork w = gaa_carve(workspace, N);
    const int nb = gaa_blocks(N, GAA_THREADS);
    hipLaunchKernelGGL(gaa_flag_kernel, dim3(nb), dim3(GAA_THREADS), 0, stream, N, opacity_accum, anchor_demon, prune_mask, min_opacity, demon_threshold,
                       w.keep, reset, w.block_sum);
    hipLaunchKernelGGL(gaa_top_scan_kernel, dim3(1), dim3(1024), 0, stream, N, nb, w.block_sum, info);
    hipLaunchKernelGGL(gaa_place_kernel, dim3(nb), dim3(GAA_THREADS), 0, stream, N, w.keep, w.block_sum, keep_rows);
    GSR_HIP(hipGetLastError(), "anchor adjust plan");
    return GSR_OK;
}

extern "C" int gsr_anchor_adjust_gather(int N, int n_keep, int n_copies, const gsr_adjust_copy* copies, const int32_t* keep_rows,
                                        const uint8_t* offset_mask, int L0, const uint8_t* reset, void* stream)
{
    if (N < 0 || n_keep < 0 || n_keep > N || n_copies < 0 || n_copies > GSR_ADJUST_MAX_COPIES || L0 < 0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: bad sizes N=%d n_keep=%d n_copies=%d L0=%d", N, n_keep, n_copies, L0);
    if (n_keep == 0 || n_copies == 0) return GSR_OK;
    if (!copies || !keep_rows) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: copies / keep_rows is NULL");
    for (int c = 0; c < n_copies; c++) {
        const gsr_adjust_copy& d = copies[c];
        if (d.width < 1 || (long long)N * d.width > 0x7fffffffLL || d.mode < GSR_ADJUST_COPY || d.mode > GSR_ADJUST_ANCHOR_STAT)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: copy %d has width %d, mode %d (need 1 <= width, N*width < 2^31)", c,
                            d.width, d.mode);
        if (!d.dst || (!d.src && !(d.mode == GSR_ADJUST_OFFSET_STAT && L0 == 0)))
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: copy %d has a NULL pointer", c);
        if (d.mode == GSR_ADJUST_OFFSET_STAT && L0 > 0 && !offset_mask)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: copy %d is OFFSET_STAT but offset_mask is NULL", c);
        if (d.mode == GSR_ADJUST_OFFSET_STAT && (long long)L0 > (long long)N * d.width)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: L0=%d exceeds N*K=%lld", L0, (long long)N * d.width);
        if (d.mode == GSR_ADJUST_ANCHOR_STAT && (d.width != 1 || !reset))
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: copy %d is ANCHOR_STAT: width must be 1 and reset given", c);
    }
    GaaTable tab{};
    tab.n = n_copies;
    uint32_t blocks = 0;
    for (int c = 0; c < n_copies; c++) {
        tab.copy[c] = copies[c];
        tab.vec[c] = (uint8_t)gaa_unit(copies[c]);
        tab.first[c] = blocks;
        blocks += (uint32_t)gaa_blocks((long long)n_keep * (copies[c].width / tab.vec[c]), GAA_CHUNK);
    }
    tab.first[n_copies] = blocks;
    hipLaunchKernelGGL(gaa_gather_kernel, dim3(blocks), dim3(GAA_THREADS), 0, (hipStream_t)stream, tab, n_keep, keep_rows, offset_mask, L0, reset);
    GSR_HIP(hipGetLastError(), "anchor adjust gather");
    return GSR_OK;
}
