// png_crc.h -- the slice-combining arithmetic of CRC-32 that png.hip (writing) and png_decode.hip (checking) share: a thread runs the
// table-driven CRC over its slice from a zero state, multiplies by x^(8 * bytes behind the slice) mod P, and the slices are XORed;
// the initial state 0xffffffff contributes 0xffffffff * x^(8 N).
#pragma once
#include <stdint.h>

#define PNG_POLY 0xEDB88320u

// a * b mod P, both in the reflected representation of CRC-32 (bit 31 = x^0)
__device__ __forceinline__ uint32_t png_gf2_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll 4
    for (int i = 0; i < 32; i++) {
        p ^= (a & (0x80000000u >> i)) ? b : 0u;
        b = (b & 1u) ? (b >> 1) ^ PNG_POLY : b >> 1;
    }
    return p;
}
// x^(8 n) mod P
__device__ __forceinline__ uint32_t png_x8n(uint32_t n)
{
    uint32_t r = 0x80000000u, b = 0x00800000u;
    for (int i = 0; i < 32 && n; i++, n >>= 1) {
        if (n & 1u) r = png_gf2_mul(r, b);
        b = png_gf2_mul(b, b);
    }
    return r;
}
// entry i of the byte table
__device__ __forceinline__ uint32_t png_crc_table_entry(uint32_t i)
{
    uint32_t c = i;
#pragma unroll
    for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ PNG_POLY : c >> 1;
    return c;
}
