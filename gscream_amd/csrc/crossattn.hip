// crossattn.hip -- the attention core of BidirectionalCrossAttention (bidirectional-cross-attention 0.4, the module GScream's
// GaussianModel.run_crossattn calls, scene/gaussian_model.py:553-583), fp32 on the exact f32 matrix cores.
//
//   sim[i][j] = scale * qk[i] . cqk[j]          (one head of 64; masked pairs take -FLT_MAX)
//   out[i]    = sum_j softmax_j(sim)[i][j] cv[j]      ("x" direction:       rows of sim)
//   cout[j]   = sum_i softmax_i(sim)[i][j]  v[i]      ("context" direction: columns of sim)
//
// The context direction is the x direction with the two sides swapped (sim^T = cqk . qk^T), so there is ONE forward and ONE
// backward kernel, launched with blockIdx.z = direction: z picks which side owns the query rows and which side is walked
// as keys.  No [h, i, j] tensor is written anywhere; the backward recomputes tiles from the per-row (max, 1 / sum)
// pairs the forward leaves in the workspace.  DESIGN.md "Bidirectional cross-attention" has the reasoning and the numbers.
//
// Tile layout (v_mfma_f32_32x32x2_f32: lane l supplies A[row l & 31][k l >> 5] and B[k l >> 5][col l & 31] and holds
// D[row (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col l & 31] in register r of 16):
//   * a wave owns 32 query rows; the query row is the COLUMN of every product, so lane (i = l & 31, h = l >> 5) only ever holds
//     values of its own row i: the softmax over keys is a reduction over the lane's 16 registers + one exchange with lane l ^ 32,
//     and every per-row scalar (running max, sum, alpha, row dot) is a per-lane scalar;
//   * T^T[key][i] = sum_d X[key][d] Y[i][d] (gca_tile): A = a key tile in LDS (row key = l & 31, 16-byte reads of a 68-float
//     padded row), B = the query-side row Y[i][32 h .. 32 h + 31] held in 32 registers for the whole kernel; the sum over d is
//     order-free, so step s pairs lane half h with d = 32 h + s on both operands;
//   * acc^T[d][i] += sum_key X[key][d] T^T[key][i] (gca_accum): register r of the tile IS the B operand of step r (keys
//     (r & 3) + 8 (r >> 2) + 4 h, the same map read on the A side from LDS), so the tile goes from one product into the next
//     with no lane movement and no LDS round trip.
// Sums run in a fixed order and nothing is accumulated with atomics: two calls on the same inputs give the same bits.
#include <float.h>
#include <math.h>
#include "gsr_api.h"
#include "gsr_carve.h"

typedef float gca_v16 __attribute__((ext_vector_type(16)));
typedef float gca_v4 __attribute__((ext_vector_type(4)));
#define GCA_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_32x32x2f32((A), (B), (C), 0, 0, 0)
#define GCA_D 64                      // dim_head (the only one on this path)
#define GCA_LD 68                     // floats per LDS row: 64 + one 16-byte slot, so the 16-byte A reads of 32 rows spread over the banks
#define GCA_TK 64                     // keys staged per step (two 32-key MFMA tiles)
#define GCA_WAVES 4
#define GCA_ROWS (32 * GCA_WAVES)     // query rows per workgroup
#define GCA_THREADS (64 * GCA_WAVES)
#define GCA_ARR (GCA_TK * GCA_LD)     // floats of one staged [key][d] array

// one side of the attention (x or context); the kernels see a (query side, key side) pair
struct GcaSide {
    const float* qk;      // [b, n, h, 64]
    const float* v;       // [b, n, h, 64]
    const uint8_t* mask;  // [b, n] or NULL (all true)
    int n;
    float2* stats;        // [b, h, n] (max, 1 / sum) of this side's softmax rows
    float* dot;           // [b, h, n] sum_j P (d_out . v_other): the softmax backward's row term (gca_rowdot_kernel)
    float* out;           // forward: [b, n, h, 64]
    const float* d_out;   // backward
    float* d_qk;
    float* d_v;
};
struct GcaArgs {
    GcaSide s[2];
    int B, H;
    float scale;
};

__device__ __forceinline__ void gca_stage(float* dst, const float* src, size_t row_stride, int j0, int n, int tid)
{
#pragma unroll
    for (int idx = tid; idx < GCA_TK * 16; idx += GCA_THREADS) {
        const int row = idx >> 4, c4 = idx & 15, j = j0 + row;
        gca_v4 val = { 0.f, 0.f, 0.f, 0.f };
        if (j < n) val = *reinterpret_cast<const gca_v4*>(src + (size_t)j * row_stride + 4 * c4);
        *reinterpret_cast<gca_v4*>(dst + row * GCA_LD + 4 * c4) = val;
    }
}

__device__ __forceinline__ void gca_load_row(float (&x)[32], const float* row, bool ok)
{
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        gca_v4 val = { 0.f, 0.f, 0.f, 0.f };
        if (ok) val = *reinterpret_cast<const gca_v4*>(row + 4 * q);
        x[4 * q] = val.x; x[4 * q + 1] = val.y; x[4 * q + 2] = val.z; x[4 * q + 3] = val.w;
    }
}

// T^T[key][i] = sum_d tile[key][d] * x_i[d]   (tile: 32 keys in LDS)
__device__ __forceinline__ gca_v16 gca_tile(const float* tile, const float (&x)[32], int lane)
{
    gca_v16 acc = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    const float* p = tile + (lane & 31) * GCA_LD + (lane >> 5) * 32;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const gca_v4 a = *reinterpret_cast<const gca_v4*>(p + 4 * q);
        acc = GCA_MFMA(a.x, x[4 * q], acc);
        acc = GCA_MFMA(a.y, x[4 * q + 1], acc);
        acc = GCA_MFMA(a.z, x[4 * q + 2], acc);
        acc = GCA_MFMA(a.w, x[4 * q + 3], acc);
    }
    return acc;
}

// acc^T[d][i] += sum_key tile[key][d] * t[key][i]
__device__ __forceinline__ void gca_accum(const float* tile, const gca_v16& t, gca_v16 (&acc)[2], int lane)
{
    const float* p = tile + 4 * (lane >> 5) * GCA_LD + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float* pr = p + ((r & 3) + 8 * (r >> 2)) * GCA_LD;
        acc[0] = GCA_MFMA(pr[0], t[r], acc[0]);
        acc[1] = GCA_MFMA(pr[32], t[r], acc[1]);
    }
}

// register r of lane (i, h) of acc[dt] is element d = 32 dt + (r & 3) + 8 (r >> 2) + 4 h of row i
__device__ __forceinline__ void gca_store_row(float* row, const gca_v16 (&acc)[2], int half, float mul)
{
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const gca_v4 val = { acc[dt][4 * g] * mul, acc[dt][4 * g + 1] * mul, acc[dt][4 * g + 2] * mul, acc[dt][4 * g + 3] * mul };
            *reinterpret_cast<gca_v4*>(row + 32 * dt + 8 * g + 4 * half) = val;
        }
}

// key codes staged beside a tile: 0 = beyond the end (contributes nothing), 1 = masked out (-FLT_MAX), 2 = valid
#define GCA_KEY_OOR 0.f
#define GCA_KEY_MASKED 1.f
#define GCA_KEY_OK 2.f

__global__ __launch_bounds__(GCA_THREADS) void gca_forward_kernel(GcaArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[2 * GCA_ARR + GCA_TK];
    float* const ldsK = lds;
    float* const ldsV = lds + GCA_ARR;
    float* const kcode = lds + 2 * GCA_ARR;
    const int dir = blockIdx.z;
    const GcaSide& Q = a.s[dir];
    const GcaSide& K = a.s[1 - dir];
    const int i_block = blockIdx.x * GCA_ROWS;
    if (i_block >= Q.n) return;  // the grid is sized for the longer side
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
    const size_t rs = (size_t)a.H * GCA_D;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int i = i_block + (tid >> 6) * 32 + (lane & 31);
    const bool in_range = i < Q.n;
    const bool q_ok = in_range && (!Q.mask || Q.mask[(size_t)b * Q.n + i]);
    const float* kbase = K.qk + ((size_t)b * K.n * a.H + h) * GCA_D;
    const float* vbase = K.v + ((size_t)b * K.n * a.H + h) * GCA_D;
    const size_t qoff = ((size_t)b * Q.n + (in_range ? i : 0)) * rs + (size_t)h * GCA_D;

    float x[32];
    gca_load_row(x, Q.qk + qoff + 32 * half, in_range);
    float m = -INFINITY, l = 0.f;
    gca_v16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;

    for (int j0 = 0; j0 < K.n; j0 += GCA_TK) {
        __syncthreads();
        gca_stage(ldsK, kbase, rs, j0, K.n, tid);
        gca_stage(ldsV, vbase, rs, j0, K.n, tid);
        if (tid < GCA_TK) {
            const int j = j0 + tid;
            kcode[tid] = j >= K.n ? GCA_KEY_OOR : ((!K.mask || K.mask[(size_t)b * K.n + j]) ? GCA_KEY_OK : GCA_KEY_MASKED);
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < GCA_TK / 32; ++sub) {
            if (j0 + 32 * sub >= K.n) break;
            gca_v16 t = gca_tile(ldsK + sub * 32 * GCA_LD, x, lane);
            float mx = m;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const gca_v4 code = *reinterpret_cast<const gca_v4*>(kcode + 32 * sub + 8 * g + 4 * half);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float s = t[4 * g + e] * a.scale;
                    if (code[e] == GCA_KEY_MASKED || !q_ok) s = -FLT_MAX;
                    if (code[e] == GCA_KEY_OOR) s = -INFINITY;
                    t[4 * g + e] = s;
                    mx = fmaxf(mx, s);
                }
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));  // finite: key 32 * sub of this tile exists, and a real score is >= -FLT_MAX
            const float alpha = expf(m - mx);    // 0 on the first tile (m = -inf)
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = expf(t[r] - mx);
                t[r] = p;
                psum += p;
            }
            psum += __shfl_xor(psum, 32);
            l = l * alpha + psum;
            m = mx;
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[0][r] *= alpha; acc[1][r] *= alpha; }
            gca_accum(ldsV + sub * 32 * GCA_LD, t, acc, lane);
        }
    }
    if (!in_range) return;
    const float inv = 1.0f / l;
    gca_store_row(Q.out + qoff, acc, half, inv);
    if (half == 0) Q.stats[((size_t)b * a.H + h) * Q.n + i] = make_float2(m, inv);
}

// dot[b, h, i] = sum_j P[i][j] * (d_out_Q[i] . v_K[j]): the row term of the softmax backward, for the query side Q.
// In exact arithmetic this is d_out[i] . out[i]; it is summed here over the SAME P and the same d_out . v tiles the backward kernel
// recomputes (same operands, same order, so the same bits), as the softmax backward of the torch expressions does.  The term
// enters as P (d_out . v - dot): where a softmax is peaked the two cancel, and a dot taken another way (from the rounded `out`)
// leaves the rounding of two 64-term sums of size |d_out . v| where the eager path leaves an exact zero.
__global__ __launch_bounds__(GCA_THREADS) void gca_rowdot_kernel(GcaArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[2 * GCA_ARR + GCA_TK];
    float* const ldsK = lds;
    float* const ldsV = lds + GCA_ARR;
    float* const kcode = lds + 2 * GCA_ARR;
    const int dir = blockIdx.z;
    const GcaSide& Q = a.s[dir];
    const GcaSide& K = a.s[1 - dir];
    const int i_block = blockIdx.x * GCA_ROWS;
    if (i_block >= Q.n) return;
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
    const size_t rs = (size_t)a.H * GCA_D;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int i = i_block + (tid >> 6) * 32 + (lane & 31);
    const bool in_range = i < Q.n;
    const bool q_ok = in_range && (!Q.mask || Q.mask[(size_t)b * Q.n + i]);
    const size_t koff = ((size_t)b * K.n * a.H + h) * GCA_D;
    const size_t qoff = ((size_t)b * Q.n + (in_range ? i : 0)) * rs + (size_t)h * GCA_D;
    const size_t si = ((size_t)b * a.H + h) * Q.n + (in_range ? i : 0);

    float xq[32], xg[32];
    gca_load_row(xq, Q.qk + qoff + 32 * half, in_range);
    gca_load_row(xg, Q.d_out + qoff + 32 * half, in_range);
    float qmax = 0.f, qinv = 0.f;
    if (in_range) {
        const float2 st = Q.stats[si];
        qmax = st.x;
        qinv = st.y;
    }
    float dot = 0.f;
    for (int j0 = 0; j0 < K.n; j0 += GCA_TK) {
        __syncthreads();
        gca_stage(ldsK, K.qk + koff, rs, j0, K.n, tid);
        gca_stage(ldsV, K.v + koff, rs, j0, K.n, tid);
        if (tid < GCA_TK) {
            const int j = j0 + tid;
            kcode[tid] = j >= K.n ? GCA_KEY_OOR : ((!K.mask || K.mask[(size_t)b * K.n + j]) ? GCA_KEY_OK : GCA_KEY_MASKED);
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < GCA_TK / 32; ++sub) {
            if (j0 + 32 * sub >= K.n) break;
            const int o = sub * 32 * GCA_LD;
            const gca_v16 ts = gca_tile(ldsK + o, xq, lane);
            const gca_v16 tp = gca_tile(ldsV + o, xg, lane);
            float part = 0.f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const gca_v4 code = *reinterpret_cast<const gca_v4*>(kcode + 32 * sub + 8 * g + 4 * half);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e;
                    float s = ts[r] * a.scale;
                    if (code[e] != GCA_KEY_OK || !q_ok) s = -FLT_MAX;
                    if (code[e] == GCA_KEY_OOR || !in_range) s = -INFINITY;
                    part += (expf(s - qmax) * qinv) * tp[r];
                }
            }
            dot += part + __shfl_xor(part, 32);
        }
    }
    if (in_range && half == 0) Q.dot[si] = dot;
}

// For the query side Q (rows i) against the key side K (rows j), with S = the score matrix seen from Q:
//   P[i][j] = exp(S - maxQ[i]) / sumQ[i]   (Q's softmax, feeds Q.out = P K.v)
//   R[i][j] = exp(S - maxK[j]) / sumK[j]   (K's softmax seen transposed, feeds K.out = R^T Q.v)
//   dS = P (d_out_Q[i] . K.v[j] - dotQ[i]) + R (Q.v[i] . d_out_K[j] - dotK[j]),   0 where the pair is masked
//   Q.d_qk[i] = scale sum_j dS K.qk[j]          Q.d_v[i] = sum_j R d_out_K[j]
__global__ __launch_bounds__(GCA_THREADS) void gca_backward_kernel(GcaArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[3 * GCA_ARR + 4 * GCA_TK];
    float* const ldsK = lds;
    float* const ldsV = lds + GCA_ARR;
    float* const ldsG = lds + 2 * GCA_ARR;
    float* const kcode = lds + 3 * GCA_ARR;
    float* const kmax = kcode + GCA_TK;
    float* const kinv = kmax + GCA_TK;
    float* const kdot = kinv + GCA_TK;
    const int dir = blockIdx.z;
    const GcaSide& Q = a.s[dir];
    const GcaSide& K = a.s[1 - dir];
    const int i_block = blockIdx.x * GCA_ROWS;
    if (i_block >= Q.n) return;
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H;
    const size_t rs = (size_t)a.H * GCA_D;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5;
    const int i = i_block + (tid >> 6) * 32 + (lane & 31);
    const bool in_range = i < Q.n;
    const bool q_ok = in_range && (!Q.mask || Q.mask[(size_t)b * Q.n + i]);
    const size_t koff = ((size_t)b * K.n * a.H + h) * GCA_D;
    const size_t qoff = ((size_t)b * Q.n + (in_range ? i : 0)) * rs + (size_t)h * GCA_D;
    const size_t kstat = ((size_t)b * a.H + h) * K.n;

    float xq[32], xv[32], xg[32];
    gca_load_row(xq, Q.qk + qoff + 32 * half, in_range);
    gca_load_row(xv, Q.v + qoff + 32 * half, in_range);
    gca_load_row(xg, Q.d_out + qoff + 32 * half, in_range);
    float qmax = 0.f, qinv = 0.f, qdot = 0.f;
    if (in_range) {
        const size_t si = ((size_t)b * a.H + h) * Q.n + i;
        const float2 st = Q.stats[si];
        qmax = st.x;
        qinv = st.y;
        qdot = Q.dot[si];
    }
    gca_v16 dq[2], dv[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[0][r] = dq[1][r] = dv[0][r] = dv[1][r] = 0.f;

    for (int j0 = 0; j0 < K.n; j0 += GCA_TK) {
        __syncthreads();
        gca_stage(ldsK, K.qk + koff, rs, j0, K.n, tid);
        gca_stage(ldsV, K.v + koff, rs, j0, K.n, tid);
        gca_stage(ldsG, K.d_out + koff, rs, j0, K.n, tid);
        if (tid < GCA_TK) {
            const int j = j0 + tid;
            const bool ok = j < K.n;
            const float2 st = ok ? K.stats[kstat + j] : make_float2(0.f, 0.f);
            kcode[tid] = !ok ? GCA_KEY_OOR : ((!K.mask || K.mask[(size_t)b * K.n + j]) ? GCA_KEY_OK : GCA_KEY_MASKED);
            kmax[tid] = st.x;
            kinv[tid] = st.y;
            kdot[tid] = ok ? K.dot[kstat + j] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < GCA_TK / 32; ++sub) {
            if (j0 + 32 * sub >= K.n) break;
            const int o = sub * 32 * GCA_LD;
            gca_v16 ts = gca_tile(ldsK + o, xq, lane);        // qk_K[j] . qk_Q[i]
            const gca_v16 tp = gca_tile(ldsV + o, xg, lane);  // v_K[j] . d_out_Q[i]
            gca_v16 tr = gca_tile(ldsG + o, xv, lane);        // d_out_K[j] . v_Q[i]
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ko = 32 * sub + 8 * g + 4 * half;
                const gca_v4 code = *reinterpret_cast<const gca_v4*>(kcode + ko);
                const gca_v4 km = *reinterpret_cast<const gca_v4*>(kmax + ko);
                const gca_v4 ki = *reinterpret_cast<const gca_v4*>(kinv + ko);
                const gca_v4 kd = *reinterpret_cast<const gca_v4*>(kdot + ko);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e;
                    const bool pair_ok = code[e] == GCA_KEY_OK && q_ok;
                    float s = ts[r] * a.scale;
                    if (!pair_ok) s = -FLT_MAX;
                    if (code[e] == GCA_KEY_OOR || !in_range) s = -INFINITY;
                    const float p = expf(s - qmax) * qinv;
                    const float rr = expf(s - km[e]) * ki[e];
                    const float ds = p * (tp[r] - qdot) + rr * (tr[r] - kd[e]);
                    ts[r] = pair_ok ? ds * a.scale : 0.f;  // masked_fill replaces the value: no gradient reaches a masked score
                    tr[r] = rr;
                }
            }
            gca_accum(ldsK + o, ts, dq, lane);
            gca_accum(ldsG + o, tr, dv, lane);
        }
    }
    if (!in_range) return;
    gca_store_row(Q.d_qk + qoff, dq, half, 1.0f);
    gca_store_row(Q.d_v + qoff, dv, half, 1.0f);
}

// ---- host side ----------------------------------------------------------------------------------------------------
// workspace: stats of x rows, stats of context rows (float2 each), then the two backward row-dot arrays (float)
struct GcaWork { float2* stats[2]; float* dot[2]; size_t bytes; };
static GcaWork gca_carve(void* base, int B, int H, int I, int J)
{
    GcaWork w{};
    GsrCarver c(base);
    const size_t bh = (size_t)B * H;
    w.stats[0] = c.take<float2>(bh * I);
    w.stats[1] = c.take<float2>(bh * J);
    w.dot[0] = c.take<float>(bh * I);
    w.dot[1] = c.take<float>(bh * J);
    w.bytes = c.total();
    return w;
}

static GcaArgs gca_args(int B, int H, int I, int J, const float* qk, const float* v, const float* cqk, const float* cv, const uint8_t* mask,
                        const uint8_t* cmask, float scale, void* workspace)
{
    GcaArgs a = {};
    const GcaWork w = gca_carve(workspace, B, H, I, J);
    a.s[0].qk = qk; a.s[0].v = v; a.s[0].mask = mask; a.s[0].n = I;
    a.s[1].qk = cqk; a.s[1].v = cv; a.s[1].mask = cmask; a.s[1].n = J;
    for (int k = 0; k < 2; k++) { a.s[k].stats = w.stats[k]; a.s[k].dot = w.dot[k]; }
    a.B = B; a.H = H; a.scale = scale;
    return a;
}

static dim3 gca_grid(int B, int H, int I, int J)
{
    const int n = I > J ? I : J;
    return dim3((n + GCA_ROWS - 1) / GCA_ROWS, B * H, 2);
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
static int gca_check_sizes(const char* what, int B, int H, int I, int J, int dim_head)
{
    if (dim_head != 64) return gsr_fail(GSR_ERR_UNSUPPORTED, "%s: dim_head = %d (this path is built for 64)", what, dim_head);
    if (B < 1 || H < 1 || I < 1 || J < 1 || (long long)B * H > 65535 || (long long)B * H * ((long long)I + J) * 64 > 0x7fffffffLL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes b=%d heads=%d i=%d j=%d", what, B, H, I, J);
    // (no accepted size wraps the carve: B*H*(I + J) < 2^25 rows of 12 bytes)
    return GSR_OK;
}

extern "C" size_t gsr_crossattn_workspace_bytes(int B, int H, int I, int J)
{
    if (B < 1 || H < 1 || I < 1 || J < 1) return 0;
    return gca_carve(nullptr, B, H, I, J).bytes;
}

extern "C" int gsr_crossattn_forward(int B, int H, int I, int J, int dim_head, const float* qk, const float* v, const float* context_qk,
                                     const float* context_v, const uint8_t* mask, const uint8_t* context_mask, float scale, float* out,
                                     float* context_out, void* workspace, void* stream)
{
    if (int rc = gca_check_sizes("crossattn forward", B, H, I, J, dim_head)) return rc;
    if (!qk || !v || !context_qk || !context_v || !out || !context_out || !workspace)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "crossattn forward: a required pointer is NULL");
    GcaArgs a = gca_args(B, H, I, J, qk, v, context_qk, context_v, mask, context_mask, scale, workspace);
    a.s[0].out = out;
    a.s[1].out = context_out;
    hipLaunchKernelGGL(gca_forward_kernel, gca_grid(B, H, I, J), dim3(GCA_THREADS), 0, (hipStream_t)stream, a);
    GSR_HIP(hipGetLastError(), "crossattn forward");
    return GSR_OK;
}

extern "C" int gsr_crossattn_backward(int B, int H, int I, int J, int dim_head, const float* qk, const float* v, const float* context_qk,
                                      const float* context_v, const uint8_t* mask, const uint8_t* context_mask, float scale,
                                      const float* out, const float* context_out, const float* d_out, const float* d_context_out,
                                      void* workspace, float* d_qk, float* d_v, float* d_context_qk, float* d_context_v, void* stream_)
{
    if (int rc = gca_check_sizes("crossattn backward", B, H, I, J, dim_head)) return rc;
    if (!qk || !v || !context_qk || !context_v || !out || !context_out || !d_out || !d_context_out || !workspace || !d_qk || !d_v
        || !d_context_qk || !d_context_v)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "crossattn backward: a required pointer is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    GcaArgs a = gca_args(B, H, I, J, qk, v, context_qk, context_v, mask, context_mask, scale, workspace);
    a.s[0].out = const_cast<float*>(out);
    a.s[1].out = const_cast<float*>(context_out);
    a.s[0].d_out = d_out;
    a.s[1].d_out = d_context_out;
    a.s[0].d_qk = d_qk; a.s[0].d_v = d_v;
    a.s[1].d_qk = d_context_qk; a.s[1].d_v = d_context_v;
    hipLaunchKernelGGL(gca_rowdot_kernel, gca_grid(B, H, I, J), dim3(GCA_THREADS), 0, stream, a);
    GSR_HIP(hipGetLastError(), "crossattn backward");
    hipLaunchKernelGGL(gca_backward_kernel, gca_grid(B, H, I, J), dim3(GCA_THREADS), 0, stream, a);
    GSR_HIP(hipGetLastError(), "crossattn backward");
    return GSR_OK;
}
