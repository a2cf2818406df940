// anchor_sample.hip -- the anchor sampler of GScream's cross-attention step, on the device and without a host stop.
//
// Replaces the tensor math of train.py:436-511: classify every anchor by where it projects, count the classes, and draw the two
// equally sized random subsets (foreground = src, background = dst) that GaussianModel.run_crossattn pairs up.  For anchor a with
// x = px[a], y = py[a] (fp32), image H x W, rectangle (min_y, max_y, min_x, max_x):
//   valid    visible[a] and 0 < x < W and 0 < y < H          strict, in floating point; NaN is invalid
//   pixel    iy = (int)y, ix = (int)x                        truncation (.long())
//   sampled  valid and min_y <= iy < max_y and min_x <= ix < max_x
//   label    (long)gt_mask[iy, ix]                           truncation: label > 0 <=> m >= 1, label == 0 <=> -1 < m < 1
//   fg       sampled and label > 0;   bg  sampled and label == 0;   a negative label (m <= -1) or a NaN is in neither class
//   ok       n_fg > 11 and n_bg > 11  (the reference's four exit() guards reduce to this)
//   min_num  min(n_fg, n_bg, max_pairs)
//   src      the min_num members of fg with the smallest (key, index);  dst the same of bg;  both empty when not ok
//
// The key function (part of the contract: gscream_amd/anchor_sampler.py and the tests restate it).  All arithmetic is modulo 2^32,
// s_lo / s_hi are the low / high 32 bits of the 64-bit seed, i is the anchor index:
//   mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
//   key(i) = mix(((mix((i ^ s_lo) + s_hi)) + s_lo) ^ s_hi)
// Every step is a bijection of uint32, so two anchors never share a key and the index tie-break below is never taken; it is kept.
// The reference draws with randperm and keeps only the set, so a keyed order statistic has the same distribution.
//
// Passes (all on the caller's stream, a fixed number of launches, no read-back):
//   gas_classify   class byte per anchor, the three counts, and the level-0 histogram of the keys' top 11 bits per class
//   gas_pick  x 3  one block: find the digit in which the min_num-th smallest key of each class lies (level 0 also writes info[])
//   gas_hist  x 2  histograms of the next 11 / the last 10 key bits among the anchors that match the prefix found so far
//   gas_flag       per anchor: key < threshold / key == threshold; block sums of both, per class
//   gas_top_scan   exclusive scan of the block sums (one block, each thread a contiguous run)
//   gas_place      masks for every anchor, ascending row lists (position = selected anchors of the class before it)
// Histograms are LDS integer counters flushed with integer atomics: the result does not depend on the order of arrival.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_scan.h"

#define GAS_THREADS 256
#define GAS_ITEMS 8                          // anchors per thread in the histogram sweeps
#define GAS_TILE (GAS_THREADS * GAS_ITEMS)   // anchors per block there
#define GAS_BINS 2048                        // 11 bits (levels 0 and 1); level 2 uses the first 1024
#define GAS_NONE 0
#define GAS_FG 1
#define GAS_BG 2
#define GAS_OTHER 3                          // sampled, in neither class
#define GAS_LT 4                             // flag byte: key below the class's threshold
#define GAS_EQ 8                             // flag byte: key equal to it

// workspace head (uint32 words): [0] n_sampled [1] n_fg [2] n_bg [3] -, [4] prefix fg [5] prefix bg [6] take fg [7] take bg,
// then from word GAS_HIST0 the histograms [level][class][GAS_BINS]
#define GAS_HIST0 64
#define GAS_HEAD_WORDS (GAS_HIST0 + 3 * 2 * GAS_BINS)

__host__ __device__ __forceinline__ uint32_t gas_mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__host__ __device__ __forceinline__ uint32_t gas_key(uint32_t i, uint32_t s_lo, uint32_t s_hi)
{
    return gas_mix((gas_mix((i ^ s_lo) + s_hi) + s_lo) ^ s_hi);
}

static __host__ __device__ inline int gas_shift(int level) { return level == 0 ? 21 : level == 1 ? 10 : 0; }
static __host__ __device__ inline int gas_bins(int level) { return level == 2 ? 1024 : GAS_BINS; }
static inline int gas_blocks(long long n, int per) { return (int)((n + per - 1) / per); }

__device__ __forceinline__ int gas_class(int i, int H, int W, const uint8_t* __restrict__ visible, const float* __restrict__ px,
                                         const float* __restrict__ py, const float* __restrict__ gt_mask, int min_y, int max_y, int min_x,
                                         int max_x)
{
    if (!visible[i]) return GAS_NONE;
    const float x = px[i], y = py[i];
    if (!(x > 0.0f && x < (float)W && y > 0.0f && y < (float)H)) return GAS_NONE;  // false for NaN
    const int ix = min((int)x, W - 1), iy = min((int)y, H - 1);                     // (the min never binds for H, W <= 2^24)
    if (!(iy >= min_y && iy < max_y && ix >= min_x && ix < max_x)) return GAS_NONE;
    const float m = gt_mask[(size_t)iy * W + ix];
    if (m >= 1.0f) return GAS_FG;
    if (m > -1.0f && m < 1.0f) return GAS_BG;
    return GAS_OTHER;
}

__device__ __forceinline__ void gas_flush(const uint32_t* lds, uint32_t* __restrict__ hist)
{
    for (int b = threadIdx.x; b < 2 * GAS_BINS; b += GAS_THREADS) {
        const uint32_t c = lds[b];
        if (c) atomicAdd(&hist[b], c);
    }
}

__global__ void __launch_bounds__(GAS_THREADS) gas_classify_kernel(int N, int H, int W, const uint8_t* __restrict__ visible,
                                                                   const float* __restrict__ px, const float* __restrict__ py,
                                                                   const float* __restrict__ gt_mask, int min_y, int max_y, int min_x, int max_x,
                                                                   uint32_t s_lo, uint32_t s_hi, uint8_t* __restrict__ cls,
                                                                   uint32_t* __restrict__ head)
{
    __shared__ uint32_t lh[2 * GAS_BINS];
    __shared__ uint32_t cnt[3];
    for (int b = threadIdx.x; b < 2 * GAS_BINS; b += GAS_THREADS) lh[b] = 0u;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const long long base = (long long)blockIdx.x * GAS_TILE;
#pragma unroll
    for (int j = 0; j < GAS_ITEMS; j++) {
        const long long i = base + j * GAS_THREADS + threadIdx.x;
        if (i >= N) break;
        const int c = gas_class((int)i, H, W, visible, px, py, gt_mask, min_y, max_y, min_x, max_x);
        cls[i] = (uint8_t)c;
        if (c == GAS_NONE) continue;
        atomicAdd(&cnt[0], 1u);
        if (c == GAS_OTHER) continue;
        atomicAdd(&cnt[c], 1u);
        atomicAdd(&lh[(c - 1) * GAS_BINS + (gas_key((uint32_t)i, s_lo, s_hi) >> 21)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&head[threadIdx.x], cnt[threadIdx.x]);
    if (cnt[1] | cnt[2]) gas_flush(lh, head + GAS_HIST0);
}

// level 1 / 2: among the anchors of a class whose key agrees with the class's prefix above this level's digit
__global__ void __launch_bounds__(GAS_THREADS) gas_hist_kernel(int N, int level, uint32_t s_lo, uint32_t s_hi, const uint8_t* __restrict__ cls,
                                                               uint32_t* __restrict__ head)
{
    __shared__ uint32_t lh[2 * GAS_BINS];
    __shared__ uint32_t any;
    for (int b = threadIdx.x; b < 2 * GAS_BINS; b += GAS_THREADS) lh[b] = 0u;
    if (threadIdx.x == 0) any = 0u;
    __syncthreads();
    const int shift = gas_shift(level), up = gas_shift(level - 1);
    const uint32_t dmask = (uint32_t)gas_bins(level) - 1u;
    const uint32_t pre[2] = { head[4] >> up, head[5] >> up };
    const uint32_t take[2] = { head[6], head[7] };
    const long long base = (long long)blockIdx.x * GAS_TILE;
#pragma unroll
    for (int j = 0; j < GAS_ITEMS; j++) {
        const long long i = base + j * GAS_THREADS + threadIdx.x;
        if (i >= N) break;
        const int c = cls[i];
        if (c != GAS_FG && c != GAS_BG) continue;
        if (take[c - 1] == 0u) continue;
        const uint32_t k = gas_key((uint32_t)i, s_lo, s_hi);
        if ((k >> up) != pre[c - 1]) continue;
        atomicAdd(&lh[(c - 1) * GAS_BINS + ((k >> shift) & dmask)], 1u);
        any = 1u;
    }
    __syncthreads();
    if (any) gas_flush(lh, head + GAS_HIST0 + level * 2 * GAS_BINS);
}

// One block of 1024: thread t owns bins 2t and 2t + 1 of each class.  The digit d of a class is the first whose inclusive count
// reaches `take`; the anchors below it are all taken, `take` becomes what is still to be taken inside d.
__global__ void __launch_bounds__(1024) gas_pick_kernel(int level, int max_pairs, uint32_t* __restrict__ head, int32_t* __restrict__ info)
{
    uint32_t take[2];
    if (level == 0) {
        const uint32_t n_fg = head[1], n_bg = head[2];
        const bool ok = n_fg > 11u && n_bg > 11u;
        const uint32_t min_num = min(min(n_fg, n_bg), (uint32_t)max_pairs);
        take[0] = take[1] = ok ? min_num : 0u;
        if (threadIdx.x == 0) {
            info[0] = (int32_t)head[0];
            info[1] = (int32_t)n_fg;
            info[2] = (int32_t)n_bg;
            info[3] = (int32_t)min_num;
            info[4] = ok ? 1 : 0;
            info[5] = info[6] = info[7] = 0;
        }
    } else {
        take[0] = head[6];
        take[1] = head[7];
    }
    const uint32_t prefix[2] = { level == 0 ? 0u : head[4], level == 0 ? 0u : head[5] };
    const int bins = gas_bins(level), shift = gas_shift(level);
    const uint32_t* hist = head + GAS_HIST0 + level * 2 * GAS_BINS;
    const int b0 = 2 * threadIdx.x;
    uint32_t h0[2], h1[2], ex[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        h0[c] = b0 < bins ? hist[c * GAS_BINS + b0] : 0u;
        h1[c] = b0 + 1 < bins ? hist[c * GAS_BINS + b0 + 1] : 0u;
        ex[c] = h0[c] + h1[c];
    }
    gsr_block_scan_excl<1024>(ex);  // (its barrier also: every thread has read head[4..7] before any thread writes them below)
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const uint32_t in = ex[c] + h0[c] + h1[c];
        if (level == 0 && threadIdx.x == 0 && take[c] == 0u) {
            head[4 + c] = 0u;
            head[6 + c] = 0u;
        }
        if (take[c] > 0u && ex[c] < take[c] && take[c] <= in) {
            const bool first = ex[c] + h0[c] >= take[c];
            head[4 + c] = prefix[c] | ((uint32_t)(first ? b0 : b0 + 1) << shift);
            head[6 + c] = first ? take[c] - ex[c] : take[c] - ex[c] - h0[c];
        }
    }
}

// ---- ordered compaction --------------------------------------------------------------------------------------------------------
// per class one 64-bit value: low word = keys below the threshold, high word = keys equal to it (counts <= N < 2^31 each)
__device__ __forceinline__ void gas_flag_values(uint8_t f, unsigned long long (&v)[2] /* fg, bg */)
{
    const unsigned long long x = (f & GAS_LT) ? 1ull : (f & GAS_EQ) ? (1ull << 32) : 0ull;
    v[0] = (f & 3) == GAS_FG ? x : 0ull;
    v[1] = (f & 3) == GAS_BG ? x : 0ull;
}

__global__ void __launch_bounds__(GAS_THREADS) gas_flag_kernel(int N, uint32_t s_lo, uint32_t s_hi, const uint8_t* __restrict__ cls,
                                                               const uint32_t* __restrict__ head, uint8_t* __restrict__ flag,
                                                               unsigned long long* __restrict__ sum_fg, unsigned long long* __restrict__ sum_bg)
{
    const long long i = (long long)blockIdx.x * GAS_THREADS + threadIdx.x;
    uint8_t f = 0;
    if (i < N) {
        const int c = cls[i];
        if ((c == GAS_FG || c == GAS_BG) && head[6 + c - 1] > 0u) {
            const uint32_t k = gas_key((uint32_t)i, s_lo, s_hi), t = head[4 + c - 1];
            f = (uint8_t)(c | (k < t ? GAS_LT : 0) | (k == t ? GAS_EQ : 0));
        }
        flag[i] = f;
    }
    unsigned long long v[2], tot[2];
    gas_flag_values(f, v);
    gsr_block_scan_excl<GAS_THREADS>(v, tot);
    if (threadIdx.x == 0) {
        sum_fg[blockIdx.x] = tot[0];
        sum_bg[blockIdx.x] = tot[1];
    }
}

__global__ void __launch_bounds__(1024) gas_top_scan_kernel(int nb, unsigned long long* __restrict__ sum_fg, unsigned long long* __restrict__ sum_bg)
{
    unsigned long long* const arr[2] = { sum_fg, sum_bg };
    unsigned long long total[2];
    gsr_top_scan(nb, arr, total);
}

// An anchor is selected when its key is below the threshold, or equal to it and fewer than `take` equal keys of its class come
// before it (smallest index first).  Its row-list position = the selected anchors of its class before it.
__global__ void __launch_bounds__(GAS_THREADS) gas_place_kernel(int N, int max_pairs, const uint8_t* __restrict__ flag,
                                                                const uint32_t* __restrict__ head, const unsigned long long* __restrict__ base_fg,
                                                                const unsigned long long* __restrict__ base_bg, uint8_t* __restrict__ src_mask,
                                                                uint8_t* __restrict__ dst_mask, int64_t* __restrict__ src_rows,
                                                                int64_t* __restrict__ dst_rows)
{
    const long long i = (long long)blockIdx.x * GAS_THREADS + threadIdx.x;
    const uint8_t f = i < N ? flag[i] : (uint8_t)0;
    unsigned long long v[2];
    gas_flag_values(f, v);
    gsr_block_scan_excl<GAS_THREADS>(v);
    if (i >= N) return;
    const int c = f & 3;
    bool sel = false;
    if (f & (GAS_LT | GAS_EQ)) {
        const unsigned long long e = (c == GAS_FG ? base_fg[blockIdx.x] + v[0] : base_bg[blockIdx.x] + v[1]);
        const uint32_t lt = (uint32_t)e, eq = (uint32_t)(e >> 32), take = head[6 + c - 1];
        sel = (f & GAS_LT) || eq < take;
        const uint32_t pos = lt + min(eq, take);
        if (sel && pos < (uint32_t)max_pairs) (c == GAS_FG ? src_rows : dst_rows)[pos] = (int64_t)i;
    }
    src_mask[i] = (uint8_t)(sel && c == GAS_FG);
    dst_mask[i] = (uint8_t)(sel && c == GAS_BG);
}

// ---- workspace --------------------------------------------------------------------------------------------------------------
struct GasWork {
    uint32_t* head;              // [GAS_HEAD_WORDS]
    unsigned long long* sum_fg;  // [blocks(N) + 1]
    unsigned long long* sum_bg;  // [blocks(N) + 1]
    uint8_t* cls;                // [N]
    uint8_t* flag;               // [N]
    size_t bytes;
};

static GasWork gas_carve(void* base, int N)
{
    GasWork w{};
    GsrCarver c(base);
    const size_t nb = (size_t)gas_blocks(N, GAS_THREADS) + 1;
    w.head = c.take<uint32_t>(GAS_HEAD_WORDS);
    w.sum_fg = c.take<unsigned long long>(nb);
    w.sum_bg = c.take<unsigned long long>(nb);
    w.cls = c.take<uint8_t>((size_t)N);
    w.flag = c.take<uint8_t>((size_t)N);
    w.bytes = c.total();
    return w;
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
static int gas_check_sizes(int N, int H, int W, int max_pairs)
{
    if (N < 0 || N > 0x7fffff00 || max_pairs < 0 || H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24) || (long long)H * W > 0x7fffffffLL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor sample: bad sizes N=%d H=%d W=%d max_pairs=%d", N, H, W, max_pairs);
    // (no accepted size wraps the carve: N < 2^31 bytes per array)
    return GSR_OK;
}

extern "C" size_t gsr_anchor_sample_workspace_bytes(int N, int max_pairs)
{
    if (N < 0 || N > 0x7fffff00 || max_pairs < 0) return 0;
    return gas_carve(nullptr, N).bytes;  // (the row lists are the caller's; max_pairs keeps the size query's signature in step with the call's)
}

extern "C" int gsr_anchor_sample(int N, int H, int W, const uint8_t* visible, const float* px, const float* py, const float* gt_mask,
                                 int min_y, int max_y, int min_x, int max_x, int max_pairs, uint64_t seed, void* workspace,
                                 uint8_t* src_mask, uint8_t* dst_mask, int64_t* src_rows, int64_t* dst_rows, int32_t* info, void* stream_)
{
    if (int rc = gas_check_sizes(N, H, W, max_pairs)) return rc;
    if (!info || (N > 0 && (!workspace || !visible || !px || !py || !gt_mask || !src_mask || !dst_mask))
        || (N > 0 && max_pairs > 0 && (!src_rows || !dst_rows)))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor sample: a required pointer is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    if (N == 0) { GSR_HIP(hipMemsetAsync(info, 0, 8 * sizeof(int32_t), stream), "anchor sample"); return GSR_OK; }
    const GasWork w = gas_carve(workspace, N);
    const uint32_t s_lo = (uint32_t)seed, s_hi = (uint32_t)(seed >> 32);
    const int nt = gas_blocks(N, GAS_TILE), nb = gas_blocks(N, GAS_THREADS);
    GSR_HIP(hipMemsetAsync(w.head, 0, (size_t)GAS_HEAD_WORDS * 4, stream), "anchor sample");
    hipLaunchKernelGGL(gas_classify_kernel, dim3(nt), dim3(GAS_THREADS), 0, stream, N, H, W, visible, px, py, gt_mask, min_y, max_y, min_x,
                       max_x, s_lo, s_hi, w.cls, w.head);
    hipLaunchKernelGGL(gas_pick_kernel, dim3(1), dim3(1024), 0, stream, 0, max_pairs, w.head, info);
    for (int level = 1; level <= 2; level++) {
        hipLaunchKernelGGL(gas_hist_kernel, dim3(nt), dim3(GAS_THREADS), 0, stream, N, level, s_lo, s_hi, w.cls, w.head);
        hipLaunchKernelGGL(gas_pick_kernel, dim3(1), dim3(1024), 0, stream, level, max_pairs, w.head, info);
    }
    hipLaunchKernelGGL(gas_flag_kernel, dim3(nb), dim3(GAS_THREADS), 0, stream, N, s_lo, s_hi, w.cls, w.head, w.flag, w.sum_fg, w.sum_bg);
    hipLaunchKernelGGL(gas_top_scan_kernel, dim3(1), dim3(1024), 0, stream, nb, w.sum_fg, w.sum_bg);
    hipLaunchKernelGGL(gas_place_kernel, dim3(nb), dim3(GAS_THREADS), 0, stream, N, max_pairs, w.flag, w.head, w.sum_fg, w.sum_bg, src_mask,
                       dst_mask, src_rows, dst_rows);
    GSR_HIP(hipGetLastError(), "anchor sample");
    return GSR_OK;
}
