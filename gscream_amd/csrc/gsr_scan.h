// gsr_scan.h -- the scans and the ordered compaction ("count, scan, place") of the kernels around the rasterizer: decode,
// kNN, anchor growth, anchor sampling -- and of the rasterizer's binning (binning.hip: gsr_block_scan_runs and the C = 4 form) and per-Gaussian
// backward (gauss_bwd.hip: the written-slot counts of a flag pass across the cooperative kernel's four waves).
// Integer sums only, with one fixed association order per output element.  (gsr_fwd_order_block keeps its own scan; the reductions
// are in gsr_reduce.h.)
//
// The block-wide forms keep their per-wave totals in a static LDS array and hold exactly ONE barrier: a kernel that calls
// the same form a second time needs a __syncthreads() between the two calls (binning.hip does, and has one).  All threads
// of the block must make the call.
#pragma once
#include "gsr_math.h"  // gsr_wave_scan_add(uint32_t): the DPP form

// inclusive wave scan of 64-bit values (DPP moves 32 bits; this is the one shuffle loop)
__device__ __forceinline__ unsigned long long gsr_wave_scan_add(unsigned long long v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// Exclusive scan over a block of NT threads, in place, of C independent values per thread behind one barrier; the block's
// totals go to totals[0..C) when given.  LOOP = true: the C * NT / 64 wave totals are read in a loop over the waves, not all at
// once -- the caller's choice, for a kernel at its register budget (the binning's scatter, C = 4 and 1024 threads: 82 -> 110 VGPRs
// and an occupancy step with the 64 totals in flight; measured on that kernel alone).
template <int NT, typename T, int C, bool LOOP = false>
__device__ __forceinline__ void gsr_block_scan_excl(T (&v)[C], T* totals = nullptr)
{
    __shared__ T wsum[C][NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T incl[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        incl[c] = gsr_wave_scan_add(v[c]);
        if (lane == 63) wsum[c][wave] = incl[c];
    }
    __syncthreads();
    constexpr int UNROLL = LOOP ? 1 : NT / 64;
#pragma unroll
    for (int c = 0; c < C; c++) {
        T base = 0, tot = 0;
#pragma unroll UNROLL
        for (int w = 0; w < NT / 64; w++) { const T sw = wsum[c][w]; base += w < wave ? sw : (T)0; tot += sw; }
        v[c] = base + incl[c] - v[c];
        if (totals) totals[c] = tot;
    }
}
template <int NT, typename T>
__device__ __forceinline__ T gsr_block_scan_excl(T v, T* total = nullptr)
{
    T a[1] = { v };
    gsr_block_scan_excl<NT>(a, total);
    return a[0];
}

// Exclusive scan, by a block of NT threads, of n entries of which thread i owns the run [i * per, (i + 1) * per), per =
// ceil(n / NT): get(j) reads entry j, put(j, start, v) receives the entry's exclusive start and its value -- in place when
// put stores start where get read.  *total, when given, is the block's sum, set before the first put.  PER > 0: a compile-time
// bound on per; the entries are then read ONCE, all loads in flight together, and kept in registers (PER = 0: any n, get
// runs a second time).  (gsr_top_scan below is the same ownership over C arrays at once with one barrier for all of them, which
// get / put of one value cannot express; it keeps its own loops.)  bmax, when given: an LDS word the caller zeroed behind a barrier; holds the largest entry afterwards.
template <int NT, int PER, typename Get, typename Put>
__device__ __forceinline__ void gsr_block_scan_runs(const int n, Get get, Put put, uint32_t* total = nullptr, uint32_t* bmax = nullptr)
{
    const int per = (n + NT - 1) / NT, i0 = (int)threadIdx.x * per;  // per <= PER
    uint32_t v[PER > 0 ? PER : 1];
    uint32_t sum = 0, mx = 0;
    if (PER > 0) {
#pragma unroll
        for (int i = 0; i < PER; i++) v[i] = (i < per && i0 + i < n) ? get(i0 + i) : 0u;
#pragma unroll
        for (int i = 0; i < PER; i++) { sum += v[i]; mx = max(mx, v[i]); }
    } else {
        for (int i = 0; i < per; i++) {
            const uint32_t c = i0 + i < n ? get(i0 + i) : 0u;
            sum += c;
            mx = max(mx, c);
        }
    }
    if (bmax) {
        mx = gsr_wave_scan_max(mx);
        if ((threadIdx.x & 63) == 63) atomicMax(bmax, mx);
    }
    uint32_t run = gsr_block_scan_excl<NT>(sum, total);
    if (PER > 0) {
#pragma unroll
        for (int i = 0; i < PER; i++)
            if (i < per && i0 + i < n) { put(i0 + i, run, v[i]); run += v[i]; }
    } else {
        for (int i = 0; i < per && i0 + i < n; i++) { const uint32_t c = get(i0 + i); put(i0 + i, run, c); run += c; }
    }
}

// Exclusive scan in place of the nb block totals in each of C arrays, by ONE block of 1024 (thread i owns a contiguous run
// of ceil(nb / 1024) of them); every thread gets the grand totals.
template <typename T, int C>
__device__ __forceinline__ void gsr_top_scan(int nb, T* const (&arr)[C], T (&total)[C])
{
    const int per = (nb + 1023) / 1024, i0 = threadIdx.x * per;
    T run[C];
#pragma unroll
    for (int c = 0; c < C; c++) {
        run[c] = 0;
        for (int i = 0; i < per; i++) run[c] += i0 + i < nb ? arr[c][i0 + i] : (T)0;
    }
    gsr_block_scan_excl<1024>(run, total);
#pragma unroll
    for (int c = 0; c < C; c++)
        for (int i = 0; i < per && i0 + i < nb; i++) { const T v = arr[c][i0 + i]; arr[c][i0 + i] = run[c]; run[c] += v; }
}
template <typename T>
__device__ __forceinline__ T gsr_top_scan(int nb, T* arr)
{
    T* const a[1] = { arr };
    T total[1];
    gsr_top_scan(nb, a, total);
    return total[0];
}

// Ordered compaction of a flag per thread: the number of set flags of the block's lower threads (a set flag's position
// among the block's set flags); the block's count goes to *block_count when given.
template <int NT>
__device__ __forceinline__ uint32_t gsr_block_rank(bool set, uint32_t* block_count = nullptr)
{
    __shared__ uint32_t wsum[NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(set);
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; w++) { const uint32_t sw = wsum[w]; base += w < wave ? sw : 0u; tot += sw; }
    if (block_count) *block_count = tot;
    return base + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}
