// scene_init.hip -- the first stage of a run on the device: point cloud -> anchors -> initial parameters
// (GaussianModel.voxelize_sample and create_from_pcd, scene/gaussian_model.py:295-345), and the sort it needs.
//
// 1. gsi_sort_launch: stable ascending LSD radix sort of N unsigned 64-bit keys, 8-bit digits, all 64 bits significant.
//      prepass   copies in -> out and counts all eight digits of every key (the multiset of a digit does not change with the order)
//      plan      one block: pass p is SKIPPED when one bin of its digit holds all N keys (decided here, on the device); the buffer
//                (out / tmp) each remaining pass reads follows from the skips before it, and so does where the result ends up
//      per pass  hist (digit counts per workgroup of GSR_SORT_BLOCK_KEYS keys, digit-major), a two-level exclusive scan of the
//                256 x workgroups counts, scatter
//      finish    copies tmp -> out when the number of passes that ran is odd
//    Ranks inside a workgroup are stable: wave w owns the w-th quarter of the workgroup's keys and walks it 64 keys at a time; the
//    lanes of a round are matched on the digit with eight ballots, a key's rank is the wave's running count of its digit plus
//    the matching lanes below it, and the waves are combined in order through LDS.  Integer counters and scans only.
// 2. gsi_voxelize_launch: cell = round_half_even(p / v) per component in the input's own precision (one IEEE division, rint),
//    per-axis minima / maxima of the integer cells, key = (x - xmin, y - ymin, z - zmin) packed x-major with field widths from
//    the ranges, sort, heads (key differs from its predecessor), ordered compaction, row = (T)cell * (T)v as one rounded product.
//    Ascending keys are lexicographic (x, y, z) rows: the row order of np.unique(axis=0).  -0.0 and +0.0 are the cell 0.
// 3. gsi_kth_launch: radix select (four levels of eight bits) on an order-preserving image of the fp32 bit patterns.
// 4. gsi_fill_launch: one launch for the state create_from_pcd leaves.
// Every fp operation that has to match is written with its rounding explicit; contraction is off for the whole file.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_reduce.h"
#include "gsr_scan.h"

#pragma clang fp contract(off)

typedef unsigned long long gsi_u64;

#define GSI_THREADS 256
#define GSI_WAVES (GSI_THREADS / 64)
#define GSI_ROUNDS (GSR_SORT_BLOCK_KEYS / GSI_THREADS)  // keys per thread = 64-key rounds per wave
#define GSI_PASSES 8
#define GSI_SCAN_TILE 4096                               // entries per workgroup of the count scan (1024 threads x 4)
// control words of a sort (written by the plan kernel)
#define GSI_CTL_SKIP 0    // [8] 1 = the pass does nothing
#define GSI_CTL_SRC 8     // [8] 1 = the pass reads tmp and writes out, 0 = the other way round
#define GSI_CTL_FINAL 16  // 1 = the sorted keys are in tmp
#define GSI_CTL_WORDS 32
static_assert(GSR_SORT_BLOCK_KEYS == GSI_THREADS * GSI_ROUNDS && GSI_ROUNDS * 64 * GSI_WAVES == GSR_SORT_BLOCK_KEYS, "sort tile");

static inline int gsi_blocks(long long n, int per) { return (int)((n + per - 1) / per); }

// ---- sort ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(GSI_THREADS) gsi_sort_prepass_kernel(int N, const gsi_u64* in, gsi_u64* out, uint32_t* __restrict__ ghist)
{
    __shared__ uint32_t lh[GSI_PASSES * 256];
    for (int b = threadIdx.x; b < GSI_PASSES * 256; b += GSI_THREADS) lh[b] = 0u;
    __syncthreads();
    const long long base = (long long)blockIdx.x * GSR_SORT_BLOCK_KEYS;
#pragma unroll
    for (int r = 0; r < GSI_ROUNDS; r++) {
        const long long i = base + r * GSI_THREADS + threadIdx.x;
        if (i < N) {
            const gsi_u64 k = in[i];
            out[i] = k;
#pragma unroll
            for (int p = 0; p < GSI_PASSES; p++) atomicAdd(&lh[p * 256 + (int)((k >> (8 * p)) & 255u)], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < GSI_PASSES * 256; b += GSI_THREADS) {
        const uint32_t c = lh[b];
        if (c) atomicAdd(&ghist[b], c);
    }
}

__global__ void __launch_bounds__(256) gsi_sort_plan_kernel(int N, const uint32_t* __restrict__ ghist, uint32_t* __restrict__ ctl)
{
    uint32_t src = 0u;
    for (int p = 0; p < GSI_PASSES; p++) {
        const int constant = __syncthreads_or(ghist[p * 256 + threadIdx.x] == (uint32_t)N);
        if (threadIdx.x == 0) {
            ctl[GSI_CTL_SKIP + p] = constant ? 1u : 0u;
            ctl[GSI_CTL_SRC + p] = src;
        }
        if (!constant) src ^= 1u;
    }
    if (threadIdx.x == 0) ctl[GSI_CTL_FINAL] = src;
}

__global__ void __launch_bounds__(GSI_THREADS) gsi_sort_hist_kernel(int N, int pass, int nb, const gsi_u64* out, const gsi_u64* tmp,
                                                                    const uint32_t* __restrict__ ctl, uint32_t* __restrict__ bhist)
{
    if (ctl[GSI_CTL_SKIP + pass]) return;
    const gsi_u64* src = ctl[GSI_CTL_SRC + pass] ? tmp : out;
    __shared__ uint32_t lh[256];
    lh[threadIdx.x] = 0u;
    __syncthreads();
    const long long base = (long long)blockIdx.x * GSR_SORT_BLOCK_KEYS;
#pragma unroll
    for (int r = 0; r < GSI_ROUNDS; r++) {
        const long long i = base + r * GSI_THREADS + threadIdx.x;
        if (i < N) atomicAdd(&lh[(int)((src[i] >> (8 * pass)) & 255u)], 1u);
    }
    __syncthreads();
    bhist[(size_t)threadIdx.x * nb + blockIdx.x] = lh[threadIdx.x];
}

// exclusive scan of n counts: inside tiles of GSI_SCAN_TILE (tile totals to tsum), then the tile totals by one block; a reader adds
// a[e] + tsum[e / GSI_SCAN_TILE].  ctl == NULL: not part of a sort, always runs.
__global__ void __launch_bounds__(1024) gsi_scan_tiles_kernel(int n, int pass, const uint32_t* __restrict__ ctl, uint32_t* __restrict__ a,
                                                              uint32_t* __restrict__ tsum)
{
    if (ctl && ctl[GSI_CTL_SKIP + pass]) return;
    const long long i0 = ((long long)blockIdx.x * 1024 + threadIdx.x) * 4;
    uint32_t v[4], sum = 0u;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        v[j] = i0 + j < n ? a[i0 + j] : 0u;
        sum += v[j];
    }
    uint32_t total;
    uint32_t run = gsr_block_scan_excl<1024>(sum, &total);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (i0 + j < n) a[i0 + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(1024) gsi_scan_top_kernel(int nt, int pass, const uint32_t* __restrict__ ctl, uint32_t* __restrict__ tsum)
{
    if (ctl && ctl[GSI_CTL_SKIP + pass]) return;
    (void)gsr_top_scan(nt, tsum);
}

__global__ void __launch_bounds__(GSI_THREADS) gsi_sort_scatter_kernel(int N, int pass, int nb, gsi_u64* out, gsi_u64* tmp,
                                                                       const uint32_t* __restrict__ ctl, const uint32_t* __restrict__ bhist,
                                                                       const uint32_t* __restrict__ tsum)
{
    if (ctl[GSI_CTL_SKIP + pass]) return;
    const bool from_tmp = ctl[GSI_CTL_SRC + pass] != 0u;
    const gsi_u64* src = from_tmp ? tmp : out;
    gsi_u64* dst = from_tmp ? out : tmp;
    __shared__ uint32_t wcnt[GSI_WAVES][256];
    for (int b = threadIdx.x; b < GSI_WAVES * 256; b += GSI_THREADS) (&wcnt[0][0])[b] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * GSR_SORT_BLOCK_KEYS + (long long)wave * (GSI_ROUNDS * 64);
    gsi_u64 key[GSI_ROUNDS];
    uint32_t rank[GSI_ROUNDS];
#pragma unroll
    for (int r = 0; r < GSI_ROUNDS; r++) {
        const long long i = base + r * 64 + lane;
        const bool valid = i < N;
        key[r] = valid ? src[i] : 0ull;
        const uint32_t d = (uint32_t)(key[r] >> (8 * pass)) & 255u;
        gsi_u64 same = __ballot(valid);  // the lanes of this round with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const gsi_u64 set = __ballot((d >> b) & 1u);
            same &= ((d >> b) & 1u) ? set : ~set;
        }
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(same >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)same, 0u));
        uint32_t prior = 0u;
        if (valid && below == 0u) prior = atomicAdd(&wcnt[wave][d], (uint32_t)__popcll(same));  // one lane per digit: the wave's running count
        prior = (uint32_t)__shfl((int)prior, valid ? __ffsll((long long)same) - 1 : lane, 64);
        rank[r] = prior + below;
    }
    __syncthreads();
    {   // thread t = digit t: where each wave's keys of that digit start in dst
        const size_t e = (size_t)threadIdx.x * nb + blockIdx.x;
        uint32_t run = bhist[e] + tsum[e / GSI_SCAN_TILE];
#pragma unroll
        for (int w = 0; w < GSI_WAVES; w++) {
            const uint32_t c = wcnt[w][threadIdx.x];
            wcnt[w][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < GSI_ROUNDS; r++) {
        const long long i = base + r * 64 + lane;
        if (i < N) {
            const uint32_t pos = wcnt[wave][(uint32_t)(key[r] >> (8 * pass)) & 255u] + rank[r];
            if (pos < (uint32_t)N) dst[pos] = key[r];  // (always: the counts sum to N)
        }
    }
}

__global__ void __launch_bounds__(GSI_THREADS) gsi_sort_finish_kernel(int N, const uint32_t* __restrict__ ctl, const gsi_u64* __restrict__ tmp,
                                                                      gsi_u64* __restrict__ out)
{
    if (!ctl[GSI_CTL_FINAL]) return;
    const long long i = (long long)blockIdx.x * GSI_THREADS + threadIdx.x;
    if (i < N) out[i] = tmp[i];
}

struct GsiSortWork {
    uint32_t* ctl;    // [GSI_CTL_WORDS]
    uint32_t* ghist;  // [8][256] digit counts of the whole array
    uint32_t* bhist;  // [256][nb] digit counts per workgroup, scanned in place
    uint32_t* tsum;   // [tiles of bhist + 1]
    gsi_u64* tmp;     // [N]
    int nb, nt;
    size_t bytes;
};

static GsiSortWork gsi_sort_carve(void* base, int N)
{
    GsiSortWork w{};
    GsrCarver c(base);
    const size_t n = (size_t)(N > 0 ? N : 1);
    w.nb = gsi_blocks((long long)n, GSR_SORT_BLOCK_KEYS);
    w.nt = gsi_blocks(256LL * w.nb, GSI_SCAN_TILE);
    w.ctl = c.take<uint32_t>(GSI_CTL_WORDS);
    w.ghist = c.take<uint32_t>((size_t)GSI_PASSES * 256);
    w.bhist = c.take<uint32_t>((size_t)256 * w.nb);
    w.tsum = c.take<uint32_t>((size_t)w.nt + 1);
    w.tmp = c.take<gsi_u64>(n);
    w.bytes = c.total();
    return w;
}

static size_t gsi_sort_workspace_bytes(int N) { return gsi_sort_carve(nullptr, N).bytes; }

static hipError_t gsi_sort_launch(int N, const uint64_t* keys_in, uint64_t* keys_out, void* workspace, hipStream_t stream)
{
    if (N == 0) return hipSuccess;
    hipError_t e;
    const GsiSortWork w = gsi_sort_carve(workspace, N);
    const gsi_u64* in = (const gsi_u64*)keys_in;
    gsi_u64* out = (gsi_u64*)keys_out;
    if ((e = hipMemsetAsync(w.ghist, 0, (size_t)GSI_PASSES * 256 * 4, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(gsi_sort_prepass_kernel, dim3(w.nb), dim3(GSI_THREADS), 0, stream, N, in, out, w.ghist);
    hipLaunchKernelGGL(gsi_sort_plan_kernel, dim3(1), dim3(256), 0, stream, N, w.ghist, w.ctl);
    for (int pass = 0; pass < GSI_PASSES; pass++) {
        hipLaunchKernelGGL(gsi_sort_hist_kernel, dim3(w.nb), dim3(GSI_THREADS), 0, stream, N, pass, w.nb, out, w.tmp, w.ctl, w.bhist);
        hipLaunchKernelGGL(gsi_scan_tiles_kernel, dim3(w.nt), dim3(1024), 0, stream, 256 * w.nb, pass, w.ctl, w.bhist, w.tsum);
        hipLaunchKernelGGL(gsi_scan_top_kernel, dim3(1), dim3(1024), 0, stream, w.nt, pass, w.ctl, w.tsum);
        hipLaunchKernelGGL(gsi_sort_scatter_kernel, dim3(w.nb), dim3(GSI_THREADS), 0, stream, N, pass, w.nb, out, w.tmp, w.ctl, w.bhist, w.tsum);
    }
    hipLaunchKernelGGL(gsi_sort_finish_kernel, dim3(gsi_blocks(N, GSI_THREADS)), dim3(GSI_THREADS), 0, stream, N, w.ctl, w.tmp, out);
    return hipGetLastError();
}

// ---- voxelize -----------------------------------------------------------------------------------------------------------------
// head words (int32): [0..2] per-axis minimum cell, [3..5] maximum, [6] GSR_VOXELIZE_* flags
#define GSI_HEAD_WORDS 8

__device__ __forceinline__ float gsi_quot(float p, float v) { return rintf(__fdiv_rn(p, v)); }
__device__ __forceinline__ double gsi_quot(double p, double v) { return rint(__ddiv_rn(p, v)); }
__device__ __forceinline__ float gsi_prod(float c, float v) { return __fmul_rn(c, v); }
__device__ __forceinline__ double gsi_prod(double c, double v) { return __dmul_rn(c, v); }

// the voxel size in the input's precision: the host double, or the fp32 word on the device when given
template <typename T>
__device__ __forceinline__ T gsi_voxel(double v_host, const float* __restrict__ v_dev)
{
    return v_dev ? (T)*v_dev : (T)v_host;
}

// one component's cell; false (and a flag) when it has none
template <typename T>
__device__ __forceinline__ bool gsi_cell(T p, T v, int32_t& cell, uint32_t& flags)
{
    const T r = gsi_quot(p, v);
    cell = 0;
    if (!(r - r == (T)0)) {  // NaN or an infinity
        flags |= GSR_VOXELIZE_NONFINITE;
        return false;
    }
    if (!(r > (T)-2147483648.0 && r < (T)2147483648.0)) {
        flags |= GSR_VOXELIZE_CELL_RANGE;
        return false;
    }
    cell = (int32_t)r;  // exact: r is an integer of magnitude below 2^31 (so -0.0 and +0.0 are the cell 0)
    return true;
}

__global__ void gsi_vox_init_kernel(int32_t* __restrict__ head)
{
    if (threadIdx.x < 3) head[threadIdx.x] = INT_MAX;
    else if (threadIdx.x < 6) head[threadIdx.x] = INT_MIN;
    else if (threadIdx.x < GSI_HEAD_WORDS) head[threadIdx.x] = 0;
}

template <typename T>
__global__ void __launch_bounds__(GSI_THREADS) gsi_vox_range_kernel(int N, const T* __restrict__ pts, double v_host, const float* __restrict__ v_dev,
                                                                    int32_t* __restrict__ head)
{
    __shared__ int32_t lmin[3], lmax[3];
    __shared__ uint32_t lflags;
    if (threadIdx.x < 3) {
        lmin[threadIdx.x] = INT_MAX;
        lmax[threadIdx.x] = INT_MIN;
    }
    if (threadIdx.x == 3) lflags = 0u;
    __syncthreads();
    const T v = gsi_voxel<T>(v_host, v_dev);
    const long long i = (long long)blockIdx.x * GSI_THREADS + threadIdx.x;
    int32_t mn[3] = { INT_MAX, INT_MAX, INT_MAX }, mx[3] = { INT_MIN, INT_MIN, INT_MIN };
    uint32_t flags = 0u;
    if (i < N) {
        int32_t c[3];
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; a++) ok = gsi_cell(pts[(size_t)i * 3 + a], v, c[a], flags) && ok;
        if (ok) {
#pragma unroll
            for (int a = 0; a < 3; a++) mn[a] = mx[a] = c[a];
        }
    }
    gsr_wave_reduce(mn, gsr_min());
    gsr_wave_reduce(mx, gsr_max());
    flags = gsr_wave_reduce(flags, gsr_or());
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            atomicMin(&lmin[a], mn[a]);
            atomicMax(&lmax[a], mx[a]);
        }
        if (flags) atomicOr(&lflags, flags);
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        atomicMin(&head[threadIdx.x], lmin[threadIdx.x]);
        atomicMax(&head[3 + threadIdx.x], lmax[threadIdx.x]);
    }
    if (threadIdx.x == 3 && lflags) atomicOr((uint32_t*)&head[6], lflags);
}

// key layout from the ranges: x in the top field, z in the bottom one; a field is as wide as its range needs (0 bits for a constant axis)
struct GsiLayout {
    int32_t lo[3];
    int bits[3];
};
__device__ __forceinline__ GsiLayout gsi_layout(const int32_t* __restrict__ head)
{
    GsiLayout L;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int32_t lo = head[a], hi = head[3 + a];
        const gsi_u64 range = hi >= lo ? (gsi_u64)((long long)hi - (long long)lo) : 0ull;  // (hi < lo: no point had a cell)
        L.lo[a] = hi >= lo ? lo : 0;
        L.bits[a] = range ? 64 - __clzll((long long)range) : 0;  // <= 32
    }
    return L;
}
__device__ __forceinline__ gsi_u64 gsi_shl(gsi_u64 v, int s) { return s >= 64 ? 0ull : v << s; }
__device__ __forceinline__ gsi_u64 gsi_shr(gsi_u64 v, int s) { return s >= 64 ? 0ull : v >> s; }
__device__ __forceinline__ gsi_u64 gsi_low(gsi_u64 v, int bits) { return bits >= 64 ? v : v & ((1ull << bits) - 1ull); }

template <typename T>
__global__ void __launch_bounds__(GSI_THREADS) gsi_vox_keys_kernel(int N, const T* __restrict__ pts, double v_host, const float* __restrict__ v_dev,
                                                                   int32_t* __restrict__ head, gsi_u64* __restrict__ keys)
{
    const GsiLayout L = gsi_layout(head);
    const long long i = (long long)blockIdx.x * GSI_THREADS + threadIdx.x;
    if (i == 0 && L.bits[0] + L.bits[1] + L.bits[2] > 64) atomicOr((uint32_t*)&head[6], (uint32_t)GSR_VOXELIZE_KEY_WIDTH);
    if (i >= N) return;
    const T v = gsi_voxel<T>(v_host, v_dev);
    uint32_t flags = 0u;
    gsi_u64 d[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        int32_t c;
        (void)gsi_cell(pts[(size_t)i * 3 + a], v, c, flags);
        d[a] = (gsi_u64)((long long)c - (long long)L.lo[a]);  // (a flagged cloud: any 64 bits; the caller discards the result)
    }
    keys[i] = gsi_shl(d[0], L.bits[1] + L.bits[2]) | gsi_shl(d[1], L.bits[2]) | d[2];
}

__global__ void __launch_bounds__(GSI_THREADS) gsi_vox_heads_kernel(int N, const gsi_u64* __restrict__ keys, uint32_t* __restrict__ bsum)
{
    const long long i = (long long)blockIdx.x * GSI_THREADS + threadIdx.x;
    const bool head = i < N && (i == 0 || keys[i] != keys[i - 1]);
    uint32_t count;
    (void)gsr_block_rank<GSI_THREADS>(head, &count);
    if (threadIdx.x == 0) bsum[blockIdx.x] = count;
}

__global__ void __launch_bounds__(1024) gsi_vox_top_kernel(int nb, uint32_t* __restrict__ bsum, const int32_t* __restrict__ head, double v_host,
                                                           const float* __restrict__ v_dev, int32_t* __restrict__ info)
{
    const uint32_t total = gsr_top_scan(nb, bsum);
    if (threadIdx.x == 0) {
        info[0] = (int32_t)total;
        info[1] = head[6];
        info[2] = __float_as_int(gsi_voxel<float>(v_host, v_dev));
        info[3] = 0;
    }
}

template <typename T>
__global__ void __launch_bounds__(GSI_THREADS) gsi_vox_place_kernel(int N, const gsi_u64* __restrict__ keys, const uint32_t* __restrict__ bbase,
                                                                    const int32_t* __restrict__ head, double v_host,
                                                                    const float* __restrict__ v_dev, T* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * GSI_THREADS + threadIdx.x;
    const gsi_u64 key = i < N ? keys[i] : 0ull;
    const bool is_head = i < N && (i == 0 || key != keys[i - 1]);
    const uint32_t pos = bbase[blockIdx.x] + gsr_block_rank<GSI_THREADS>(is_head);
    if (!is_head || pos >= (uint32_t)N) return;
    const GsiLayout L = gsi_layout(head);
    const T v = gsi_voxel<T>(v_host, v_dev);
    const gsi_u64 d[3] = { gsi_shr(key, L.bits[1] + L.bits[2]), gsi_low(gsi_shr(key, L.bits[2]), L.bits[1]), gsi_low(key, L.bits[2]) };
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const int32_t cell = (int32_t)((long long)L.lo[a] + (long long)d[a]);
        out[(size_t)pos * 3 + a] = gsi_prod((T)cell, v);
    }
}

struct GsiVoxWork {
    int32_t* head;   // [GSI_HEAD_WORDS]
    gsi_u64* keys;   // [N]
    uint32_t* bsum;  // [blocks(N) + 1] heads per workgroup, scanned in place
    void* sort;      // gsi_sort_workspace_bytes(N)
    size_t bytes;
};

static GsiVoxWork gsi_vox_carve(void* base, int N)
{
    GsiVoxWork w{};
    GsrCarver c(base);
    const size_t n = (size_t)(N > 0 ? N : 1);
    w.head = c.take<int32_t>(GSI_HEAD_WORDS);
    w.keys = c.take<gsi_u64>(n);
    w.bsum = c.take<uint32_t>((size_t)gsi_blocks((long long)n, GSI_THREADS) + 1);
    w.sort = c.take<uint8_t>(gsi_sort_workspace_bytes(N));
    w.bytes = c.total();
    return w;
}

template <typename T>
static hipError_t gsi_voxelize_typed(int N, const T* pts, double v_host, const float* v_dev, void* workspace, T* out, int32_t* info,
                                     hipStream_t stream)
{
    const GsiVoxWork w = gsi_vox_carve(workspace, N);
    const int nb = gsi_blocks(N, GSI_THREADS);
    hipLaunchKernelGGL(gsi_vox_init_kernel, dim3(1), dim3(64), 0, stream, w.head);
    hipLaunchKernelGGL(gsi_vox_range_kernel<T>, dim3(nb), dim3(GSI_THREADS), 0, stream, N, pts, v_host, v_dev, w.head);
    hipLaunchKernelGGL(gsi_vox_keys_kernel<T>, dim3(nb), dim3(GSI_THREADS), 0, stream, N, pts, v_host, v_dev, w.head, w.keys);
    hipError_t e = gsi_sort_launch(N, (const uint64_t*)w.keys, (uint64_t*)w.keys, w.sort, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gsi_vox_heads_kernel, dim3(nb), dim3(GSI_THREADS), 0, stream, N, w.keys, w.bsum);
    hipLaunchKernelGGL(gsi_vox_top_kernel, dim3(1), dim3(1024), 0, stream, nb, w.bsum, w.head, v_host, v_dev, info);
    hipLaunchKernelGGL(gsi_vox_place_kernel<T>, dim3(nb), dim3(GSI_THREADS), 0, stream, N, w.keys, w.bsum, w.head, v_host, v_dev, out);
    return hipGetLastError();
}

// ---- k-th smallest ------------------------------------------------------------------------------------------------------------
// workspace (uint32 words): [0] the digits found so far, [1] the rank still to find inside them, then from word 8 hist[4][256]
#define GSI_KTH_HIST0 8
#define GSI_KTH_WORDS (GSI_KTH_HIST0 + 4 * 256)
#define GSI_KTH_TILE (GSI_THREADS * 8)

// order-preserving image of an fp32 value in uint32 (negative values below the positive ones, every NaN last, as torch orders them)
__device__ __forceinline__ uint32_t gsi_fkey(float x)
{
    if (x != x) return 0xffffffffu;
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float gsi_fkey_value(uint32_t k)
{
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ void __launch_bounds__(GSI_THREADS) gsi_kth_hist_kernel(int N, int level, const float* __restrict__ values, uint32_t* __restrict__ ws)
{
    __shared__ uint32_t lh[256];
    lh[threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 24 - 8 * level;
    const uint32_t prefix = level ? ws[0] : 0u;
    const long long base = (long long)blockIdx.x * GSI_KTH_TILE;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const long long i = base + j * GSI_THREADS + threadIdx.x;
        if (i < N) {
            const uint32_t k = gsi_fkey(values[i]);
            if (level == 0 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&lh[(k >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    const uint32_t c = lh[threadIdx.x];
    if (c) atomicAdd(&ws[GSI_KTH_HIST0 + level * 256 + threadIdx.x], c);
}

// one block, thread t = digit t: the digit whose inclusive count first reaches the rank
__global__ void __launch_bounds__(256) gsi_kth_pick_kernel(int level, int k_arg, uint32_t* __restrict__ ws, float* __restrict__ out)
{
    const uint32_t k = level ? ws[1] : (uint32_t)k_arg, prefix = level ? ws[0] : 0u;
    const uint32_t h = ws[GSI_KTH_HIST0 + level * 256 + threadIdx.x];
    const uint32_t ex = gsr_block_scan_excl<256>(h);  // (its barrier: every thread has read ws[0..1] before one writes them)
    if (ex < k && k <= ex + h) {
        const uint32_t found = prefix | ((uint32_t)threadIdx.x << (24 - 8 * level));
        ws[0] = found;
        ws[1] = k - ex;
        if (level == 3) *out = gsi_fkey_value(found);
    }
}

struct GsiKthWork { uint32_t* ws; size_t bytes; };  // [GSI_KTH_WORDS], whatever N
static GsiKthWork gsi_kth_carve(void* base)
{
    GsrCarver c(base);
    uint32_t* ws = c.take<uint32_t>(GSI_KTH_WORDS);
    return { ws, c.total() };
}

// ---- the state create_from_pcd leaves -----------------------------------------------------------------------------------------
// max of fp32 values through integer atomics (the word starts at -inf): the result does not depend on the order of arrival
__device__ __forceinline__ void gsi_atomic_max_f32(float* addr, float v)
{
    v = v + 0.0f;  // -0.0 -> +0.0
    if (v >= 0.0f) atomicMax((int*)addr, __float_as_int(v));
    else atomicMin((unsigned int*)addr, __float_as_uint(v));
}

__global__ void __launch_bounds__(GSI_THREADS) gsi_fill_kernel(int M, int K, int F, const float* __restrict__ anchors, const float* __restrict__ dist2,
                                                               float opacity, float* __restrict__ scaling, float* __restrict__ offset,
                                                               float* __restrict__ feat, float* __restrict__ rotation, float* __restrict__ opac,
                                                               float* __restrict__ unc, float* __restrict__ radii, float* __restrict__ xyz_max)
{
    const size_t i = (size_t)blockIdx.x * GSI_THREADS + threadIdx.x, m = (size_t)M;
    if (i < m * K * 3) offset[i] = 0.0f;
    if (i < m * F) feat[i] = 0.0f;
    if (i < m * 6) scaling[i] = logf(__fsqrt_rn(fmaxf(dist2[i / 6], 1e-7f)));
    if (i < m * 4) rotation[i] = (i & 3) == 0 ? 1.0f : 0.0f;
    if ((size_t)blockIdx.x * GSI_THREADS >= m) return;  // (the whole block)
    float mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    if (i < m) {
        opac[i] = opacity;
        unc[i] = opacity;
        radii[i] = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; a++) mx[a] = anchors[i * 3 + a];
    }
    gsr_wave_reduce(mx, gsr_max());
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) gsi_atomic_max_f32(&xyz_max[a], mx[a]);
    }
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
#define GSI_MAX_N (1 << 30)  // (no accepted N wraps a carve: the largest piece is N keys of 8 bytes = 2^33)
extern "C" int gsr_sort_block_keys(void) { return GSR_SORT_BLOCK_KEYS; }

extern "C" size_t gsr_sort_keys_workspace_bytes(int N) { return N < 0 || N > GSI_MAX_N ? 0 : gsi_sort_workspace_bytes(N); }

extern "C" int gsr_sort_keys_u64(int N, const uint64_t* keys_in, uint64_t* keys_out, void* workspace, void* stream)
{
    if (N < 0 || N > GSI_MAX_N) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "sort keys: N=%d (need 0 <= N <= 2^30)", N);
    if (N == 0) return GSR_OK;
    if (!keys_in || !keys_out || !workspace) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "sort keys: keys_in, keys_out or workspace is NULL");
    GSR_HIP(gsi_sort_launch(N, keys_in, keys_out, workspace, (hipStream_t)stream), "sort keys");
    return GSR_OK;
}

extern "C" size_t gsr_voxelize_workspace_bytes(int N) { return N < 0 || N > GSI_MAX_N ? 0 : gsi_vox_carve(nullptr, N).bytes; }

extern "C" int gsr_voxelize(int N, int fp64, const void* points, double voxel_size, const float* voxel_size_dev, void* workspace, void* out,
                            int32_t* info, void* stream_)
{
    if (N < 0 || N > GSI_MAX_N) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "voxelize: N=%d (need 0 <= N <= 2^30)", N);
    if (fp64 != 0 && fp64 != 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "voxelize: fp64=%d (need 0 or 1)", fp64);
    if (!info || (N > 0 && (!points || !workspace || !out)))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "voxelize: points, workspace, out or info is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    if (N == 0) GSR_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int32_t), stream), "voxelize");
    else if (fp64) GSR_HIP(gsi_voxelize_typed<double>(N, (const double*)points, voxel_size, voxel_size_dev, workspace, (double*)out, info, stream), "voxelize");
    else GSR_HIP(gsi_voxelize_typed<float>(N, (const float*)points, voxel_size, voxel_size_dev, workspace, (float*)out, info, stream), "voxelize");
    return GSR_OK;
}

extern "C" size_t gsr_kth_smallest_workspace_bytes(int N) { return N < 1 || N > GSI_MAX_N ? 0 : gsi_kth_carve(nullptr).bytes; }

extern "C" int gsr_kth_smallest_f32(int N, int k, const float* values, void* workspace, float* out, void* stream_)
{
    if (N < 1 || N > GSI_MAX_N) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "kth smallest: N=%d (need 1 <= N <= 2^30)", N);
    if (k < 1 || k > N) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "kth smallest: k=%d out of range for %d values (need 1 <= k <= N)", k, N);
    if (!values || !workspace || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "kth smallest: values, workspace or out is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    uint32_t* ws = gsi_kth_carve(workspace).ws;
    GSR_HIP(hipMemsetAsync(ws, 0, (size_t)GSI_KTH_WORDS * 4, stream), "kth smallest");
    const int nb = gsi_blocks(N, GSI_KTH_TILE);
    for (int level = 0; level < 4; level++) {
        hipLaunchKernelGGL(gsi_kth_hist_kernel, dim3(nb), dim3(GSI_THREADS), 0, stream, N, level, values, ws);
        hipLaunchKernelGGL(gsi_kth_pick_kernel, dim3(1), dim3(256), 0, stream, level, k, ws, out);
    }
    GSR_HIP(hipGetLastError(), "kth smallest");
    return GSR_OK;
}

extern "C" int gsr_scene_init_fill(int M, int K, int F, const float* anchors, const float* dist2, float opacity, float* scaling, float* offset,
                                   float* anchor_feat, float* rotation, float* opacity_out, float* uncertainty_out, float* max_radii2D,
                                   float* xyz_max, void* stream_)
{
    if (M < 0 || K < 0 || F < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scene init fill: M=%d K=%d F=%d (need all >= 0)", M, K, F);
    const int64_t widest = (int64_t)M * (3 * (int64_t)K > (int64_t)F ? (3 * (int64_t)K > 6 ? 3 * (int64_t)K : 6) : ((int64_t)F > 6 ? (int64_t)F : 6));
    if (widest >= 0x7fffffffLL) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scene init fill: M=%d K=%d F=%d (need M * max(3 K, F, 6) < 2^31)", M, K, F);
    if (!xyz_max) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scene init fill: xyz_max is NULL");
    if (M > 0 && (!anchors || !dist2 || !scaling || !rotation || !opacity_out || !uncertainty_out || !max_radii2D || (K > 0 && !offset)
                  || (F > 0 && !anchor_feat)))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scene init fill: a required pointer is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    GSR_HIP(hipMemsetD32Async((hipDeviceptr_t)xyz_max, (int)0xff800000u, 3, stream), "scene init fill");  // -inf
    if (M == 0) return GSR_OK;
    hipLaunchKernelGGL(gsi_fill_kernel, dim3((unsigned)((widest + GSI_THREADS - 1) / GSI_THREADS)), dim3(GSI_THREADS), 0, stream, M, K, F, anchors,
                       dist2, opacity, scaling, offset, anchor_feat, rotation, opacity_out, uncertainty_out, max_radii2D, xyz_max);
    GSR_HIP(hipGetLastError(), "scene init fill");
    return GSR_OK;
}
