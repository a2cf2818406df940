// anchor_grow.hip -- one growth level of GScream's anchor densification, and a segmented max (torch_scatter.scatter_max).
//
// Replaces the tensor math of scene/gaussian_model.py:834-874 (GaussianModel.anchor_growing, one pass of its level loop):
//   all_xyz      = anchor[:,None] + offset * scaling[:,None,:3]                    two eager kernels: two roundings (:829)
//   grid_coords  = round(anchor / cur_size).int()                                  existing anchors' cells (:838)
//   cells        = round(all_xyz[candidate_mask] / cur_size).int()                  candidates' cells (:840-841)
//   unique, inv  = torch.unique(cells, dim=0, return_inverse=True)                 ascending (x, y, z), signed (:843)
//   dup          = (unique[:,None] == grid_coords[chunk]).all(-1).any(-1), OR over chunks of 4096 anchors   U x N (:846-857)
//   candidate_anchor = unique[~dup] * cur_size                                     (:863)
//   new_feat     = scatter_max(anchor_feat[row / K], inv, dim=0)[0][~dup]           (:872-874)
// The U x N test becomes an open-addressing hash of the N anchor cells; torch.unique becomes a sort of 63-bit cell keys (done
// by the caller between the two entry points: torch.sort is plumbing) plus segment heads.
//
// Bit-exactness.  x / cur_size with a Python scalar is, in PyTorch's GPU true-division kernel, x * (1.0f / (float)cur_size):
// the caller passes that reciprocal, the kernels multiply.  Every product / sum is written with __fmul_rn / __fadd_rn so that
// hipcc does not contract them into an FMA (the reference rounds after each eager kernel).  torch.round is rintf (ties to
// even); the cells are integral, so .int() is exact wherever they are in range.
//
// Key range.  A candidate cell packs into 21 bits per axis biased by 2^20 (x in bits 42..62, y 21..41, z 0..20): signed
// lexicographic order of (x, y, z) = unsigned order of the key, and the key is a non-negative int64.  A candidate cell outside
// [-2^20, 2^20) or a non-finite coordinate sets info[1] bit 0; a non-finite anchor coordinate sets bit 1.  Either makes the
// caller run the level through the reference expressions instead (gscream_amd/anchor_growing.py).  A finite anchor cell
// outside that range cannot equal an in-range candidate cell, so it is simply not put into the table.
//
// Atomics are vector atomics on global memory only: atomicCAS to claim a table slot (the slot holds an anchor index; key
// comparisons read the cell array the previous kernel wrote, so the kernel boundary is the only ordering needed), atomicOr for
// the range flags, atomicMax / atomicMin on order-preserving 32-bit encodings for the per-channel maxima and argmax.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"
#include "gsr_carve.h"
#include "gsr_scan.h"

#define GAG_THREADS 256
#define GAG_BIAS (1 << 20)
#define GAG_EMPTY (-1)
#define GAG_OUT_OF_RANGE 0x7fffffff  // cell.x of an anchor whose cell cannot equal any in-range candidate cell

static __host__ __device__ inline int gag_blocks(long long n) { return (int)((n + GAG_THREADS - 1) / GAG_THREADS); }

// ---- order-preserving float <-> uint32 (0 = "nothing written": below every float's code; every NaN -> the largest code) ----
__device__ __forceinline__ uint32_t gag_enc(float f)
{
    const uint32_t u = __float_as_uint(f);
    if (f != f) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gag_dec(uint32_t k)
{
    if (k == 0u) return 0.0f;
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ uint32_t gag_hash(int x, int y, int z)
{
    uint32_t h = (uint32_t)x * 0x9e3779b1u ^ (uint32_t)y * 0x85ebca77u ^ (uint32_t)z * 0xc2b2ae3du;
    h ^= h >> 15;
    h *= 0x2c1b3c6du;
    h ^= h >> 12;
    return h;
}

// cell of one coordinate: rint(x * inv), as float (integral or non-finite)
__device__ __forceinline__ float gag_cell(float x, float inv) { return rintf(__fmul_rn(x, inv)); }
__device__ __forceinline__ bool gag_in_range(float q) { return q >= -(float)GAG_BIAS && q < (float)GAG_BIAS; }

// exclusive scan of the block totals in place; the grand total's low and high 32-bit halves go to *lo / *hi when given
__global__ void __launch_bounds__(1024) gag_top_scan_kernel(int nb, unsigned long long* __restrict__ block_sum, int32_t* __restrict__ lo,
                                                            int32_t* __restrict__ hi)
{
    const unsigned long long tot = gsr_top_scan(nb, block_sum);
    if (threadIdx.x == 0) {
        if (lo) lo[0] = (int32_t)(uint32_t)tot;
        if (hi) hi[0] = (int32_t)(uint32_t)(tot >> 32);
    }
}

// ---- phase 1: anchor cells, hash table, candidate keys ----------------------------------------------------------------
__global__ void __launch_bounds__(GAG_THREADS) gag_anchor_cells_kernel(int N, const float* __restrict__ anchor, float inv,
                                                                       int32_t* __restrict__ cells, int32_t* __restrict__ info)
{
    const int n = blockIdx.x * GAG_THREADS + threadIdx.x;
    if (n >= N) return;
    const float qx = gag_cell(anchor[3 * (size_t)n], inv), qy = gag_cell(anchor[3 * (size_t)n + 1], inv),
                qz = gag_cell(anchor[3 * (size_t)n + 2], inv);
    const bool finite = fabsf(qx) <= 3.0e38f && fabsf(qy) <= 3.0e38f && fabsf(qz) <= 3.0e38f;
    if (!finite) atomicOr(&info[1], 2);
    const bool in = finite && gag_in_range(qx) && gag_in_range(qy) && gag_in_range(qz);
    cells[3 * (size_t)n] = in ? (int)qx : GAG_OUT_OF_RANGE;
    cells[3 * (size_t)n + 1] = in ? (int)qy : 0;
    cells[3 * (size_t)n + 2] = in ? (int)qz : 0;
}

// Linear probing; a slot is claimed with atomicCAS(EMPTY -> n).  Coarse levels put many anchors into one cell: an anchor whose
// cell is already in the table stops there (one representative per cell is all the test needs).  The table has at least 2N
// slots, so the probe always finds a free one.
__global__ void __launch_bounds__(GAG_THREADS) gag_insert_kernel(int N, const int32_t* __restrict__ cells, int32_t* __restrict__ table,
                                                                 uint32_t cap_mask)
{
    const int n = blockIdx.x * GAG_THREADS + threadIdx.x;
    if (n >= N) return;
    const int x = cells[3 * (size_t)n], y = cells[3 * (size_t)n + 1], z = cells[3 * (size_t)n + 2];
    if (x == GAG_OUT_OF_RANGE) return;
    uint32_t h = gag_hash(x, y, z) & cap_mask;
    for (;;) {
        const int prev = atomicCAS(&table[h], GAG_EMPTY, n);
        if (prev == GAG_EMPTY) return;
        if (cells[3 * (size_t)prev] == x && cells[3 * (size_t)prev + 1] == y && cells[3 * (size_t)prev + 2] == z) return;
        h = (h + 1u) & cap_mask;
    }
}

__device__ __forceinline__ bool gag_table_has(int x, int y, int z, const int32_t* __restrict__ cells, const int32_t* __restrict__ table,
                                              uint32_t cap_mask)
{
    uint32_t h = gag_hash(x, y, z) & cap_mask;
    for (;;) {
        const int e = table[h];
        if (e == GAG_EMPTY) return false;
        if (cells[3 * (size_t)e] == x && cells[3 * (size_t)e + 1] == y && cells[3 * (size_t)e + 2] == z) return true;
        h = (h + 1u) & cap_mask;
    }
}

__global__ void __launch_bounds__(GAG_THREADS) gag_mask_count_kernel(int L, const uint8_t* __restrict__ mask,
                                                                     unsigned long long* __restrict__ block_sum)
{
    const int i = blockIdx.x * GAG_THREADS + threadIdx.x;
    uint32_t c;
    (void)gsr_block_rank<GAG_THREADS>(i < L && mask[i] != 0, &c);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = (unsigned long long)c;
}

// candidate c = the c-th set mask bit (flat row i = n K + k, ascending: the order of all_xyz.view(-1, 3)[candidate_mask])
__global__ void __launch_bounds__(GAG_THREADS) gag_place_kernel(int L, int K, const uint8_t* __restrict__ mask,
                                                                const unsigned long long* __restrict__ block_base,
                                                                const float* __restrict__ anchor, const float* __restrict__ offset,
                                                                const float* __restrict__ scaling, float inv, int64_t* __restrict__ keys,
                                                                int32_t* __restrict__ rows, int32_t* __restrict__ info)
{
    const int i = blockIdx.x * GAG_THREADS + threadIdx.x;
    const bool set = i < L && mask[i] != 0;
    const unsigned long long pos = block_base[blockIdx.x] + gsr_block_rank<GAG_THREADS>(set);
    if (!set) return;
    const int n = (int)((uint32_t)i / (uint32_t)K);
    float q[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const float t = __fmul_rn(offset[3 * (size_t)i + d], scaling[6 * (size_t)n + d]);  // offset * scaling[:, :3]
        q[d] = gag_cell(__fadd_rn(anchor[3 * (size_t)n + d], t), inv);                     // anchor + (...), / cur_size, round
    }
    const bool in = gag_in_range(q[0]) && gag_in_range(q[1]) && gag_in_range(q[2]);  // (false for NaN / inf)
    if (!in) atomicOr(&info[1], 1);
    const uint64_t key = in ? ((uint64_t)((int)q[0] + GAG_BIAS) << 42) | ((uint64_t)((int)q[1] + GAG_BIAS) << 21) | (uint64_t)((int)q[2] + GAG_BIAS)
                            : 0ull;
    keys[pos] = (int64_t)key;
    rows[pos] = i;
}

// ---- phase 2 (after the caller's stable sort of keys[0:M]): segment heads, dedupe against the table, per-channel max ------
__device__ __forceinline__ void gag_key_cell(int64_t key, int& x, int& y, int& z)
{
    x = (int)(((uint64_t)key >> 42) & 0x1fffffu) - GAG_BIAS;
    y = (int)(((uint64_t)key >> 21) & 0x1fffffu) - GAG_BIAS;
    z = (int)((uint64_t)key & 0x1fffffu) - GAG_BIAS;
}

// value of sorted position s: bit 0 = segment head (first of its cell), bit 32 = head of a cell no anchor occupies (kept)
__device__ __forceinline__ unsigned long long gag_head_value(int s, int M, const int64_t* __restrict__ keys, const int32_t* __restrict__ cells,
                                                             const int32_t* __restrict__ table, uint32_t cap_mask)
{
    if (s >= M) return 0ull;
    const int64_t k = keys[s];
    if (s > 0 && keys[s - 1] == k) return 0ull;
    int x, y, z;
    gag_key_cell(k, x, y, z);
    return gag_table_has(x, y, z, cells, table, cap_mask) ? 1ull : 1ull | (1ull << 32);
}

__global__ void __launch_bounds__(GAG_THREADS) gag_head_count_kernel(int M, const int64_t* __restrict__ keys, const int32_t* __restrict__ cells,
                                                                     const int32_t* __restrict__ table, uint32_t cap_mask,
                                                                     uint8_t* __restrict__ head_kind, unsigned long long* __restrict__ block_sum)
{
    const int s = blockIdx.x * GAG_THREADS + threadIdx.x;
    const unsigned long long v = gag_head_value(s, M, keys, cells, table, cap_mask);
    if (s < M) head_kind[s] = (uint8_t)((v & 1ull) | ((v >> 31) & 2ull));
    unsigned long long tot;
    (void)gsr_block_scan_excl<GAG_THREADS>(v, &tot);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = tot;
}

// position s -> segment id (pos_seg); segment -> output slot or -1 (seg_slot); kept heads write candidate_anchor = cell * cur_size
__global__ void __launch_bounds__(GAG_THREADS) gag_head_place_kernel(int M, const int64_t* __restrict__ keys, const uint8_t* __restrict__ head_kind,
                                                                     const unsigned long long* __restrict__ block_base, float cur_size,
                                                                     uint32_t* __restrict__ pos_seg, int32_t* __restrict__ seg_slot,
                                                                     float* __restrict__ candidate_anchor)
{
    const int s = blockIdx.x * GAG_THREADS + threadIdx.x;
    const uint8_t hk = s < M ? head_kind[s] : (uint8_t)0;
    const unsigned long long v = (unsigned long long)(hk & 1u) | ((unsigned long long)(hk >> 1) << 32);
    const unsigned long long excl = block_base[blockIdx.x] + gsr_block_scan_excl<GAG_THREADS>(v);
    if (s >= M) return;
    const unsigned long long incl = excl + v;
    const uint32_t seg = (uint32_t)incl - 1u;
    pos_seg[s] = seg;
    if (!(hk & 1u)) return;
    const int slot = (hk & 2u) ? (int)(uint32_t)(excl >> 32) : -1;
    seg_slot[seg] = slot;
    if (slot < 0) return;
    int x, y, z;
    gag_key_cell(keys[s], x, y, z);
    candidate_anchor[3 * (size_t)slot] = __fmul_rn((float)x, cur_size);
    candidate_anchor[3 * (size_t)slot + 1] = __fmul_rn((float)y, cur_size);
    candidate_anchor[3 * (size_t)slot + 2] = __fmul_rn((float)z, cur_size);
}

// One wave per 64 consecutive sorted positions, lanes over channels.  The positions' output slots and anchor rows are loaded
// once per lane and broadcast with shuffles; a run of one segment is reduced in registers and flushed with one atomicMax per
// channel (max is order-free, so the result is exact whichever wave flushes first).  Dropped cells are skipped.
__global__ void __launch_bounds__(GAG_THREADS) gag_feat_max_kernel(int M, int K, int F, const int64_t* __restrict__ perm,
                                                                   const int32_t* __restrict__ rows, const uint32_t* __restrict__ pos_seg,
                                                                   const int32_t* __restrict__ seg_slot, const float* __restrict__ feat,
                                                                   uint32_t* __restrict__ acc /* [M, F] codes */)
{
    const int lane = threadIdx.x & 63;
    const long long s0 = ((long long)blockIdx.x * GAG_THREADS + threadIdx.x - lane);
    if (s0 >= M) return;
    const int cnt = (int)min((long long)64, (long long)M - s0);
    const long long s = s0 + lane;
    int my_slot = -1, my_row = 0;
    if (lane < cnt) {
        my_slot = seg_slot[pos_seg[s]];
        if (my_slot >= 0) my_row = (int)((uint32_t)rows[perm[s]] / (uint32_t)K);
    }
    for (int f0 = 0; f0 < F; f0 += 64) {
        const int f = f0 + lane;
        int cur = -1;
        uint32_t m = 0u;
        for (int j = 0; j < cnt; j++) {
            const int slot = __shfl(my_slot, j, 64);
            const int n = __shfl(my_row, j, 64);
            if (slot != cur) {
                if (cur >= 0 && f < F) atomicMax(&acc[(size_t)cur * F + f], m);
                cur = slot;
                m = 0u;
            }
            if (slot >= 0 && f < F) m = max(m, gag_enc(feat[(size_t)n * F + f]));
        }
        if (cur >= 0 && f < F) atomicMax(&acc[(size_t)cur * F + f], m);
    }
}

__global__ void __launch_bounds__(GAG_THREADS) gag_decode_kernel(size_t n, uint32_t* __restrict__ buf)
{
    const size_t i = (size_t)blockIdx.x * GAG_THREADS + threadIdx.x;
    if (i < n) buf[i] = __float_as_uint(gag_dec(buf[i]));
}

// ---- workspace ---------------------------------------------------------------------------------------------------------
struct GagWork {
    int32_t* cells;                 // [3N]
    int32_t* table;                 // [cap]
    unsigned long long* block_sum;  // [blocks(L)]
    uint8_t* head_kind;             // [L]
    uint32_t* pos_seg;              // [L]
    int32_t* seg_slot;              // [L]
    uint32_t cap;
    size_t bytes;
};

static uint32_t gag_capacity(int N)
{
    uint32_t cap = 64;
    while (cap < 2u * (uint32_t)N) cap <<= 1;
    return cap;
}

static GagWork gag_carve(void* base, int N, int L)
{
    GagWork w{};
    GsrCarver c(base);
    w.cap = gag_capacity(N);
    w.cells = c.take<int32_t>((size_t)3 * N);
    w.table = c.take<int32_t>(w.cap);
    w.block_sum = c.take<unsigned long long>((size_t)gag_blocks(L) + 1);
    w.head_kind = c.take<uint8_t>((size_t)L);
    w.pos_seg = c.take<uint32_t>((size_t)L);
    w.seg_slot = c.take<int32_t>((size_t)L);
    w.bytes = c.total();
    return w;
}

// ---- scatter_max along dim 0 with a row index: out[index[r], f] = max_r src[r, f]; argmax = smallest such r ---------------
__global__ void __launch_bounds__(GAG_THREADS) gag_smax_max_kernel(int R, int F, int S, const float* __restrict__ src, const int64_t* __restrict__ index,
                                                                   uint32_t* __restrict__ code)
{
    const size_t i = (size_t)blockIdx.x * GAG_THREADS + threadIdx.x;
    if (i >= (size_t)R * F) return;
    const size_t r = i / (size_t)F, f = i - r * (size_t)F;
    const int64_t o = index[r];
    if (o < 0 || o >= S) return;
    atomicMax(&code[(size_t)o * F + f], gag_enc(src[i]));
}

__global__ void __launch_bounds__(GAG_THREADS) gag_smax_arg_kernel(int R, int F, int S, const float* __restrict__ src, const int64_t* __restrict__ index,
                                                                   const uint32_t* __restrict__ code, int64_t* __restrict__ argmax)
{
    const size_t i = (size_t)blockIdx.x * GAG_THREADS + threadIdx.x;
    if (i >= (size_t)R * F) return;
    const size_t r = i / (size_t)F, f = i - r * (size_t)F;
    const int64_t o = index[r];
    if (o < 0 || o >= S) return;
    // compared as floats: -0 and +0 both match a zero maximum, NaN matches a NaN one (the torch path's rule)
    const float v = src[i], m = gag_dec(code[(size_t)o * F + f]);
    if (v == m || (v != v && m != m)) atomicMin((unsigned long long*)&argmax[(size_t)o * F + f], (unsigned long long)r);
}

__global__ void __launch_bounds__(GAG_THREADS) gag_smax_fill_kernel(size_t n, int64_t fill, int64_t* __restrict__ argmax)
{
    const size_t i = (size_t)blockIdx.x * GAG_THREADS + threadIdx.x;
    if (i < n) argmax[i] = fill;
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
extern "C" size_t gsr_anchor_grow_workspace_bytes(int N, int L)
{
    if (N < 0 || L < 0) return 0;
    return gag_carve(nullptr, N, L).bytes;
}

static int gag_check_sizes(const char* what, int N, int K, int L)
{
    if (N < 0 || K < 1 || L < 0 || (long long)L > (long long)N * K || L > 0x7fffff00)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes N=%d K=%d L=%d (need 0 <= L <= N*K < 2^31)", what, N, K, L);
    // (no accepted size wraps the carve: 3 N cells and L slots of 4 bytes, below 2^35)
    return GSR_OK;
}

extern "C" int gsr_anchor_grow_keys(int N, int K, int L, const float* anchor, const float* offset, const float* scaling,
                                    const uint8_t* candidate_mask, float inv_size, void* workspace, int64_t* keys, int32_t* rows,
                                    int32_t* info, void* stream_)
{
    if (int rc = gag_check_sizes("anchor grow keys", N, K, L)) return rc;
    if (!workspace || !info || (N > 0 && !anchor) || (L > 0 && (!offset || !scaling || !candidate_mask || !keys || !rows)))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor grow keys: a required pointer is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    const GagWork w = gag_carve(workspace, N, L);
    GSR_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int32_t), stream), "anchor grow keys");
    GSR_HIP(hipMemsetAsync(w.table, 0xff, (size_t)w.cap * 4, stream), "anchor grow keys");
    if (N > 0) {
        hipLaunchKernelGGL(gag_anchor_cells_kernel, dim3(gag_blocks(N)), dim3(GAG_THREADS), 0, stream, N, anchor, inv_size, w.cells, info);
        hipLaunchKernelGGL(gag_insert_kernel, dim3(gag_blocks(N)), dim3(GAG_THREADS), 0, stream, N, w.cells, w.table, w.cap - 1u);
    }
    if (L > 0) {
        const int nb = gag_blocks(L);
        hipLaunchKernelGGL(gag_mask_count_kernel, dim3(nb), dim3(GAG_THREADS), 0, stream, L, candidate_mask, w.block_sum);
        hipLaunchKernelGGL(gag_top_scan_kernel, dim3(1), dim3(1024), 0, stream, nb, w.block_sum, info, (int32_t*)nullptr);
        hipLaunchKernelGGL(gag_place_kernel, dim3(nb), dim3(GAG_THREADS), 0, stream, L, K, candidate_mask, w.block_sum, anchor, offset, scaling, inv_size,
                           keys, rows, info);
    }
    GSR_HIP(hipGetLastError(), "anchor grow keys");
    return GSR_OK;
}

extern "C" int gsr_anchor_grow_emit(int N, int K, int F, int L, int M, const float* anchor_feat, const int64_t* sorted_keys,
                                    const int64_t* order, const int32_t* rows, float cur_size, void* workspace, float* candidate_anchor,
                                    float* new_feat, int32_t* info, void* stream_)
{
    if (int rc = gag_check_sizes("anchor grow emit", N, K, L)) return rc;
    if (F < 0 || M < 0 || M > L) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor grow emit: bad sizes F=%d M=%d L=%d", F, M, L);
    if (!workspace || !info || (M > 0 && (!sorted_keys || !order || !rows || !candidate_anchor || (F > 0 && (!anchor_feat || !new_feat)))))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor grow emit: a required pointer is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    const GagWork w = gag_carve(workspace, N, L);
    GSR_HIP(hipMemsetAsync(info + 2, 0, sizeof(int32_t), stream), "anchor grow emit");
    if (M <= 0) return GSR_OK;
    GSR_HIP(hipMemsetAsync(new_feat, 0, (size_t)M * F * 4, stream), "anchor grow emit");
    const int nb = gag_blocks(M);
    hipLaunchKernelGGL(gag_head_count_kernel, dim3(nb), dim3(GAG_THREADS), 0, stream, M, sorted_keys, w.cells, w.table, w.cap - 1u,
                       w.head_kind, w.block_sum);
    hipLaunchKernelGGL(gag_top_scan_kernel, dim3(1), dim3(1024), 0, stream, nb, w.block_sum, (int32_t*)nullptr, info + 2);
    hipLaunchKernelGGL(gag_head_place_kernel, dim3(nb), dim3(GAG_THREADS), 0, stream, M, sorted_keys, w.head_kind, w.block_sum, cur_size,
                       w.pos_seg, w.seg_slot, candidate_anchor);
    if (F > 0) {
        hipLaunchKernelGGL(gag_feat_max_kernel, dim3(nb), dim3(GAG_THREADS), 0, stream, M, K, F, order, rows, w.pos_seg, w.seg_slot, anchor_feat,
                           (uint32_t*)new_feat);
        const size_t n = (size_t)M * F;
        hipLaunchKernelGGL(gag_decode_kernel, dim3((unsigned)((n + GAG_THREADS - 1) / GAG_THREADS)), dim3(GAG_THREADS), 0, stream, n,
                           (uint32_t*)new_feat);
    }
    GSR_HIP(hipGetLastError(), "anchor grow emit");
    return GSR_OK;
}

extern "C" int gsr_scatter_max(int R, int F, int S, const float* src, const int64_t* index, float* out, int64_t* argmax, void* stream_)
{
    if (R < 0 || F < 0 || S < 0 || (long long)R * F > (1ll << 40) || (long long)S * F > (1ll << 40))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scatter_max: bad sizes R=%d F=%d S=%d", R, F, S);
    if ((long long)S * F > 0 && (!out || !argmax)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scatter_max: out / argmax is NULL");
    if ((long long)R * F > 0 && (long long)S * F > 0 && (!src || !index)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scatter_max: src / index is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n_out = (size_t)S * F, n_in = (size_t)R * F;
    if (n_out == 0) return GSR_OK;
    GSR_HIP(hipMemsetAsync(out, 0, n_out * 4, stream), "scatter_max");
    const unsigned gout = (unsigned)((n_out + GAG_THREADS - 1) / GAG_THREADS), gin = (unsigned)((n_in + GAG_THREADS - 1) / GAG_THREADS);
    hipLaunchKernelGGL(gag_smax_fill_kernel, dim3(gout), dim3(GAG_THREADS), 0, stream, n_out, (int64_t)R, argmax);
    if (n_in > 0) {
        hipLaunchKernelGGL(gag_smax_max_kernel, dim3(gin), dim3(GAG_THREADS), 0, stream, R, F, S, src, index, (uint32_t*)out);
        hipLaunchKernelGGL(gag_smax_arg_kernel, dim3(gin), dim3(GAG_THREADS), 0, stream, R, F, S, src, index, (const uint32_t*)out, argmax);
    }
    hipLaunchKernelGGL(gag_decode_kernel, dim3(gout), dim3(GAG_THREADS), 0, stream, n_out, (uint32_t*)out);
    GSR_HIP(hipGetLastError(), "scatter_max");
    return GSR_OK;
}
