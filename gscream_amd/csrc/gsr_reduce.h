// gsr_reduce.h -- the reductions of the kernels around the rasterizer (losses, metrics, frames, LPIPS, kNN, scene initialisation, PNG decode) and
// of the binning's key range; the other half of gsr_scan.h.  ONE association order: lanes by the xor butterfly d = 32, 16, ... 1,
// v = join(v, shuffled) at every step, then the waves in order 0, 1, ... NT / 64 - 1, left to right from wave 0's value.  The fp64 sums of
// the callers are reproducible bit for bit because of it; a new kernel takes its reductions from here.
//
// A join is called as join(a, b) by the scalar forms and as join(slot, a, b) by the array forms, so that it may depend on the slot
// (frames.hip: five sums, a minimum and a maximum in one call); gsr_add / gsr_min / gsr_max / gsr_or / gsr_xor answer both.
//
// The block-wide forms keep their per-wave values in a static LDS array (one per NT, type and value count) and hold exactly ONE
// barrier: a kernel that calls the same form a second time needs a __syncthreads() between the two calls.  All threads of the block
// must make the call.  A site that shares its barrier with other work, or joins the waves with something else (scene_init.hip's LDS
// atomics), takes the wave form alone and keeps its own cross-wave step.  (png.hip, the encoder, still carries its own butterflies.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GSR_JOIN(NAME, EXPR)                                                                           \
    struct NAME {                                                                                      \
        template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return EXPR; } \
        template <typename T> __device__ __forceinline__ T operator()(int, T a, T b) const { return EXPR; } \
    };
GSR_JOIN(gsr_add, a + b)
GSR_JOIN(gsr_min, min(a, b))  // (float / double: fminf / fmin, a NaN loses)
GSR_JOIN(gsr_max, max(a, b))
GSR_JOIN(gsr_or, a | b)
GSR_JOIN(gsr_xor, a ^ b)
#undef GSR_JOIN

// over the wave; the result is in every lane
template <typename T, typename Join>
__device__ __forceinline__ T gsr_wave_reduce(T v, Join join)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = join(v, (T)__shfl_xor(v, d, 64));
    return v;
}
template <typename T, int NV, typename Join>
__device__ __forceinline__ void gsr_wave_reduce(T (&v)[NV], Join join)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int q = 0; q < NV; q++) v[q] = join(q, v[q], (T)__shfl_xor(v[q], d, 64));
}
template <typename T>
__device__ __forceinline__ T gsr_wave_max(T v) { return gsr_wave_reduce(v, gsr_max()); }

// the per-wave values of the block forms (not one array per join type: a kernel's calls with different joins share it)
template <int NT, typename T, int NV>
__device__ __forceinline__ T (&gsr_block_reduce_lds())[NV][NT / 64]
{
    __shared__ T wred[NV][NT / 64];
    return wred;
}
// the wave step of the block forms: lane 0 of each wave leaves its values, then the barrier
template <int NT, typename T, int NV, typename Join>
__device__ __forceinline__ T (&gsr_block_reduce_waves(T (&v)[NV], Join join))[NV][NT / 64]
{
    T (&wred)[NV][NT / 64] = gsr_block_reduce_lds<NT, T, NV>();
    gsr_wave_reduce(v, join);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int q = 0; q < NV; q++) wred[q][threadIdx.x >> 6] = v[q];
    __syncthreads();
    return wred;
}
template <int NT, typename T, int NV, typename Join>
__device__ __forceinline__ void gsr_block_reduce_join(T (&v)[NV], const T (&wred)[NV][NT / 64], Join join)
{
#pragma unroll
    for (int q = 0; q < NV; q++) {
        v[q] = wred[q][0];
#pragma unroll
        for (int w = 1; w < NT / 64; w++) v[q] = join(q, v[q], wred[q][w]);
    }
}

// Over a block of NT threads, NV values per thread, in place: valid in thread 0 afterwards (the other threads keep their wave's values)
template <int NT, typename T, int NV, typename Join>
__device__ __forceinline__ void gsr_block_reduce(T (&v)[NV], Join join)
{
    const T (&wred)[NV][NT / 64] = gsr_block_reduce_waves<NT>(v, join);
    if (threadIdx.x == 0) gsr_block_reduce_join<NT>(v, wred, join);
}
template <int NT, typename T, typename Join>
__device__ __forceinline__ T gsr_block_reduce(T v, Join join)
{
    T a[1] = { v };
    gsr_block_reduce<NT>(a, join);
    return a[0];
}
// ... valid in every thread: each thread joins the wave values itself, as gsr_block_scan_excl does
template <int NT, typename T, int NV, typename Join>
__device__ __forceinline__ void gsr_block_reduce_all(T (&v)[NV], Join join)
{
    gsr_block_reduce_join<NT>(v, gsr_block_reduce_waves<NT>(v, join), join);
}
template <int NT, typename T, typename Join>
__device__ __forceinline__ T gsr_block_reduce_all(T v, Join join)
{
    T a[1] = { v };
    gsr_block_reduce_all<NT>(a, join);
    return a[0];
}
