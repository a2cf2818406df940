// adam.hip -- the optimiser step of the training iteration: gaussians.optimizer.step() (train.py:611, :615) for every tensor of
// every parameter group in ONE launch.
//
// The reference's Adam (scene/gaussian_model.py:376-409: eleven groups, ~23 tensors, seven learning rates) costs torch one launch
// per group at best.  The rule is a pure stream, 28 bytes per element (p, g, m, v in; p, m, v out), so here a table of tensors
// travels in the kernel arguments, as anchor_adjust.hip's gather table does, and the host sends nothing else.
//   tensor c owns the blocks [first[c], first[c + 1]); a block updates ADAM_CHUNK consecutive units of its tensor, thread t the
//   units t, t + 256, ...: every load and store instruction is contiguous over the wave.  A unit is four floats (16-byte
//   accesses) when p, g, m and v are all 16-byte aligned -- the n % 4 floats behind the last whole unit are then single floats of
//   the block that owns that position -- and one float otherwise.  The host decides per tensor (adam_unit).
// No atomics, no LDS, every element written by exactly one thread: repeated calls give identical bits.
//
// Exactness.  Per element, fp32, one rounding per operation, in the order of torch 1.12's
// mul_().add_(alpha=), mul_().addcmul_(value=), sqrt() / bias_correction2_sqrt .add_(eps), addcdiv_(value=):
//     m' = m*b1 + g*c1
//     v' = v*b2 + (c2*g)*g
//     d  = sqrt(v') / s2 + e
//     p' = p + (a*m') / d
// with the seven scalars computed by the caller in double and rounded once to fp32 (include/gsraster.h).  Every operation is a
// function of this file compiled under `#pragma clang fp contract(off)`: adam_mul / adam_add / adam_div / adam_sqrt are
// __fmul_rn / __fadd_rn / __fdiv_rn / __fsqrt_rn in meaning, and no compiler flag can fuse a product into a sum.  The toolchain's
// own __fmul_rn / __fadd_rn are plain `x * y` / `x + y` in a header that is compiled under the command line's contraction mode
// (hipcc's default contracts across inlined functions: m*b1 + g*c1 written with them came out as v_mul + v_fmac), and its
// __fsqrt_rn is the 1-ulp native instruction unless OCML_BASIC_ROUNDED_OPERATIONS is defined.  Here the two divisions are IEEE
// divisions and the square root is sqrtf, which hipcc expands to the correctly rounded one.  fp32 denormals are kept (the default
// kernel mode).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"

#pragma clang fp contract(off)

#define ADAM_THREADS 256
#define ADAM_PER_THREAD 4                    // units per thread: 16 loads of 16 bytes in flight before the arithmetic
#define ADAM_CHUNK (ADAM_THREADS * ADAM_PER_THREAD)

struct AdamTable {
    gsr_adam_tensor t[GSR_ADAM_MAX_TENSORS];  // 64 bytes each
    uint32_t first[GSR_ADAM_MAX_TENSORS + 1];
    uint8_t vec[GSR_ADAM_MAX_TENSORS];        // 4 or 1 floats per unit
    int32_t n;
};
static_assert(sizeof(gsr_adam_tensor) == 64, "gsr_adam_tensor is 4 pointers, a count and 7 floats");
static_assert(sizeof(AdamTable) <= 4096 - 64, "the table travels in the kernel arguments (4 KB)");

struct AdamScalars {
    float b1, c1, b2, c2, s2, e, a;
};

__device__ __forceinline__ float adam_mul(float x, float y) { return x * y; }  // (contraction is off from the pragma above on)
__device__ __forceinline__ float adam_add(float x, float y) { return x + y; }
__device__ __forceinline__ float adam_div(float x, float y) { return x / y; }
__device__ __forceinline__ float adam_sqrt(float x) { return sqrtf(x); }

__device__ __forceinline__ void adam_element(const AdamScalars& k, float& p, float g, float& m, float& v)
{
    m = adam_add(adam_mul(m, k.b1), adam_mul(g, k.c1));
    v = adam_add(adam_mul(v, k.b2), adam_mul(adam_mul(k.c2, g), g));
    const float d = adam_add(adam_div(adam_sqrt(v), k.s2), k.e);
    p = adam_add(p, adam_div(adam_mul(k.a, m), d));
}

// Units of V floats.  A unit beyond the stream reads unit 0 instead (the caller makes sure there is one), so that no load sits
// behind a branch and all of a thread's loads are in flight together.
template <int V>
struct AdamUnit {
    typedef float type __attribute__((ext_vector_type(V)));
    static __device__ __forceinline__ float get(const type& u, int i) { return u[i]; }
    static __device__ __forceinline__ void set(type& u, int i, float x) { u[i] = x; }
};
template <>
struct AdamUnit<1> {
    typedef float type;
    static __device__ __forceinline__ float get(const type& u, int) { return u; }
    static __device__ __forceinline__ void set(type& u, int, float x) { u = x; }
};

template <int V>
__device__ __forceinline__ void adam_units(const AdamScalars& k, float* __restrict__ p_f, const float* __restrict__ g_f,
                                           float* __restrict__ m_f, float* __restrict__ v_f, uint32_t total, uint32_t block)
{
    typedef AdamUnit<V> U;
    typedef typename U::type unit_t;
    unit_t* __restrict__ p = (unit_t*)p_f;
    const unit_t* __restrict__ g = (const unit_t*)g_f;
    unit_t* __restrict__ m = (unit_t*)m_f;
    unit_t* __restrict__ v = (unit_t*)v_f;
    const uint32_t e0 = block * (uint32_t)ADAM_CHUNK + threadIdx.x;  // < 2^31 / V + ADAM_CHUNK
    unit_t vp[ADAM_PER_THREAD], vg[ADAM_PER_THREAD], vm[ADAM_PER_THREAD], vv[ADAM_PER_THREAD];
#pragma unroll
    for (int j = 0; j < ADAM_PER_THREAD; j++) {
        const uint32_t e = e0 + (uint32_t)j * ADAM_THREADS, ec = e < total ? e : 0u;
        vg[j] = g[ec];
        vp[j] = p[ec];
        vm[j] = m[ec];
        vv[j] = v[ec];
    }
#pragma unroll
    for (int j = 0; j < ADAM_PER_THREAD; j++) {
#pragma unroll
        for (int i = 0; i < V; i++) {
            float pe = U::get(vp[j], i), me = U::get(vm[j], i), ve = U::get(vv[j], i);
            adam_element(k, pe, U::get(vg[j], i), me, ve);
            U::set(vp[j], i, pe);
            U::set(vm[j], i, me);
            U::set(vv[j], i, ve);
        }
    }
#pragma unroll
    for (int j = 0; j < ADAM_PER_THREAD; j++) {
        const uint32_t e = e0 + (uint32_t)j * ADAM_THREADS;
        if (e < total) {
            m[e] = vm[j];
            v[e] = vv[j];
            p[e] = vp[j];
        }
    }
}

__global__ void __launch_bounds__(ADAM_THREADS) adam_step_kernel(const AdamTable tab)
{
    int c = 0;
    while (c + 1 < tab.n && blockIdx.x >= tab.first[c + 1]) c++;  // (uniform: at most 31 scalar steps)
    const uint32_t block = blockIdx.x - tab.first[c];
    const gsr_adam_tensor& t = tab.t[c];
    const AdamScalars k{t.b1, t.c1, t.b2, t.c2, t.s2, t.e, t.a};
    const uint32_t n = (uint32_t)t.n;
    if (tab.vec[c] == 4) {
        const uint32_t n4 = n / 4u, tail = n % 4u;
        if (block * (uint32_t)ADAM_CHUNK < n4) adam_units<4>(k, t.p, t.g, t.m, t.v, n4, block);
        if (block == n4 / (uint32_t)ADAM_CHUNK && threadIdx.x < tail) {  // the floats behind the last whole unit
            const uint32_t i = n4 * 4u + threadIdx.x;
            float pe = t.p[i], me = t.m[i], ve = t.v[i];
            adam_element(k, pe, t.g[i], me, ve);
            t.m[i] = me;
            t.v[i] = ve;
            t.p[i] = pe;
        }
    } else {
        adam_units<1>(k, t.p, t.g, t.m, t.v, n, block);  // n > 0: an empty tensor has no blocks
    }
}

static int adam_unit(const gsr_adam_tensor& t)
{
    const uintptr_t bits = (uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v;
    return bits % 16 == 0 ? 4 : 1;
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
extern "C" int gsr_adam_step(int n_tensors, const gsr_adam_tensor* tensors, void* stream)
{
    if (n_tensors < 0 || n_tensors > GSR_ADAM_MAX_TENSORS)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "adam step: n_tensors=%d (need 0 .. %d)", n_tensors, GSR_ADAM_MAX_TENSORS);
    if (n_tensors == 0) return GSR_OK;
    if (!tensors) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "adam step: tensors is NULL");
    for (int c = 0; c < n_tensors; c++) {
        const gsr_adam_tensor& t = tensors[c];
        if (t.n < 0 || t.n > 0x7fffff00)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "adam step: tensor %d has a bad size n=%d (need 0 <= n <= 2^31 - 256)", c, t.n);
        if (t.n > 0 && (!t.p || !t.g || !t.m || !t.v)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "adam step: tensor %d has a NULL pointer", c);
        if (t.n > 0 && (((uintptr_t)t.p | (uintptr_t)t.g | (uintptr_t)t.m | (uintptr_t)t.v) & 3))
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "adam step: tensor %d has a pointer that is not 4-byte aligned", c);
    }
    AdamTable tab{};
    uint32_t blocks = 0;
    int used = 0;
    for (int c = 0; c < n_tensors; c++) {
        if (tensors[c].n == 0) continue;
        const int vec = adam_unit(tensors[c]);
        tab.t[used] = tensors[c];
        tab.vec[used] = (uint8_t)vec;
        tab.first[used] = blocks;
        const uint32_t units = ((uint32_t)tensors[c].n + (uint32_t)vec - 1u) / (uint32_t)vec;  // the partial unit counts: its block runs the tail
        blocks += (units + ADAM_CHUNK - 1u) / ADAM_CHUNK;                                      // <= 32 * 2^21 in all
        used++;
    }
    if (used == 0) return GSR_OK;
    tab.first[used] = blocks;
    tab.n = used;
    hipLaunchKernelGGL(adam_step_kernel, dim3(blocks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, tab);
    GSR_HIP(hipGetLastError(), "adam step");
    return GSR_OK;
}
