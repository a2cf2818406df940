// normals.hip -- the normal picture of render_set's RGBD frames (train.py:820-821): depth -> world-space point map
// (depth2pcd_fromplane, :252-267) -> per-pixel normal from a masked plane fit over the size x size neighbourhood
// (least_square_normal_regress_fast01, :270-298: normal equations A = sum q q^T, n ~ A^-1 sum q).
//
// The reference unfolds the point map to [1, 3, h, w, size^2] and runs batched det / inverse over h*w 3x3 systems.  The algorithm
// needs three fp32 planes read once, a size^2 window and one 3x3 solve per pixel:
//   points  : one thread per pixel, K and c2w read from the device (the caller holds them as tensors), three coalesced stores.
//   normals : one thread per pixel, a 16 x 16 tile per workgroup.  The workgroup stages its tile plus a halo of size/2 pixels as
//             three planes in LDS (structure of arrays: the 16 lanes of a tile row read 16 consecutive dwords; the pitch of 48
//             dwords puts the next tile row, the other half of a 32-lane group, on the other 16 banks).  Replicate padding is
//             index clamping at staging time, so an image smaller than the window needs nothing special.
//
// Arithmetic.  The mask decision is the reference's fp32 expression bit for bit: |(q.z - c.z) / c.z| > gamma with one rounding per
// operation (a NaN quotient keeps the point, an infinite one drops it).  Everything after it is fp64: the normal equations are
// not centred, cond(A) ~ (|p| / patch extent)^2 is 1e5 .. 1e7 at a real focal length, and an fp32 evaluation of det(A) is noise
// there (INTEGRATION Q).  Products of two fp32 values are exact in fp64, so the nine sums carry one rounding per addition, in the
// reference's window order (rows, then columns); determinant and solve are one Gaussian elimination with partial pivoting.  The kernel is 81 x (3 LDS reads + 9 fp64 FMAs) per pixel and
// measures 0.06 ms at 567 x 1008 (profiles/normals_timing.json), so no compensated-fp32 variant exists.
// No atomics, every output written by exactly one thread: repeated calls give identical bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"

// The exact fp32 operations are functions of this file below `#pragma clang fp contract(off)`, as in adam.hip: nrm_sub / nrm_mul /
// nrm_add / nrm_div are __fsub_rn / __fmul_rn / __fadd_rn / __fdiv_rn in meaning.  The toolchain's own are plain operators in a header
// that is compiled under the command line's contraction mode, and the point map's c0*xc + c1*yc written with them came out as
// v_mul + v_fmac.  The division is the IEEE one (hipcc's default), fp32 denormals are kept (the default kernel mode).
#pragma clang fp contract(off)

__device__ __forceinline__ float nrm_sub(float x, float y) { return x - y; }
__device__ __forceinline__ float nrm_mul(float x, float y) { return x * y; }
__device__ __forceinline__ float nrm_add(float x, float y) { return x + y; }
__device__ __forceinline__ float nrm_div(float x, float y) { return x / y; }

#define NRM_THREADS 256
#define NRM_TILE 16
#define NRM_MAX_SIZE 15
#define NRM_ROWS (NRM_TILE + NRM_MAX_SIZE - 1)  // 30 staged rows at most
#define NRM_PITCH 48                            // >= NRM_ROWS, and 16 mod 32 (see above)
static_assert(NRM_PITCH >= NRM_ROWS && NRM_PITCH % 32 == 16, "pitch: holds a staged row, alternates bank halves");
static_assert(NRM_TILE * NRM_TILE == NRM_THREADS, "one thread per pixel of the tile");

// P = c2w * (xn d, yn d, d, 1), xn = (j - K[0][2]) / K[0][0], yn = (i - K[1][2]) / K[1][1]; each row summed left to right.
__global__ void __launch_bounds__(NRM_THREADS) depth_points_kernel(int H, int W, const float* __restrict__ depth,
                                                                   const float* __restrict__ K, const float* __restrict__ c2w,
                                                                   float* __restrict__ points)
{
    const uint32_t n = (uint32_t)H * (uint32_t)W;  // < 2^31 - 256
    const uint32_t pix = blockIdx.x * (uint32_t)NRM_THREADS + threadIdx.x;
    if (pix >= n) return;
    const uint32_t i = pix / (uint32_t)W, j = pix - i * (uint32_t)W;
    const float d = depth[pix];
    const float xn = nrm_div(nrm_sub((float)j, K[2]), K[0]);
    const float yn = nrm_div(nrm_sub((float)i, K[5]), K[4]);
    const float xc = nrm_mul(xn, d), yc = nrm_mul(yn, d);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float* c = c2w + 4 * r;
        const float t = nrm_add(nrm_add(nrm_mul(c[0], xc), nrm_mul(c[1], yc)), nrm_mul(c[2], d));
        points[(size_t)r * n + pix] = nrm_add(t, c[3]);
    }
}

__global__ void __launch_bounds__(NRM_THREADS) point_normals_kernel(int H, int W, int tiles_x, const float* __restrict__ points, int size,
                                                                    float gamma, double eps, float* __restrict__ normals)
{
    __shared__ float plane[3][NRM_ROWS * NRM_PITCH];  // 17 280 bytes
    const int r = size >> 1, span = NRM_TILE + 2 * r;  // span <= NRM_ROWS
    const int tile_y = (int)(blockIdx.x / (uint32_t)tiles_x), tile_x = (int)(blockIdx.x - (uint32_t)tile_y * (uint32_t)tiles_x);
    const int x0 = tile_x * NRM_TILE - r, y0 = tile_y * NRM_TILE - r;
    const size_t n = (size_t)H * (size_t)W;
    for (int e = threadIdx.x; e < span * span; e += NRM_THREADS) {
        const int ty = e / span, tx = e - ty * span;
        const int gy = min(max(y0 + ty, 0), H - 1), gx = min(max(x0 + tx, 0), W - 1);  // replicate padding
        const size_t g = (size_t)gy * (size_t)W + (size_t)gx;                          // < n
        const int l = ty * NRM_PITCH + tx;
        plane[0][l] = points[g];
        plane[1][l] = points[n + g];
        plane[2][l] = points[2 * n + g];
    }
    __syncthreads();
    const int lx = threadIdx.x & (NRM_TILE - 1), ly = threadIdx.x / NRM_TILE;
    const int px = tile_x * NRM_TILE + lx, py = tile_y * NRM_TILE + ly;
    if (px >= W || py >= H) return;  // (behind the only barrier)

    const float cz = plane[2][(ly + r) * NRM_PITCH + lx + r];
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
    for (int dy = 0; dy < size; dy++) {
        const int row = (ly + dy) * NRM_PITCH + lx;
        for (int dx = 0; dx < size; dx++) {
            const float qx = plane[0][row + dx], qy = plane[1][row + dx], qz = plane[2][row + dx];
            const bool drop = fabsf(nrm_div(nrm_sub(qz, cz), cz)) > gamma;  // false for a NaN quotient
            const double x = drop ? 0.0 : (double)qx, y = drop ? 0.0 : (double)qy, z = drop ? 0.0 : (double)qz;
            a00 = fma(x, x, a00);  // (the products are exact: one rounding per step either way)
            a01 = fma(x, y, a01);
            a02 = fma(x, z, a02);
            a11 = fma(y, y, a11);
            a12 = fma(y, z, a12);
            a22 = fma(z, z, a22);
            sx += x;
            sy += y;
            sz += z;
        }
    }
    // [A | s] by Gaussian elimination with partial pivoting: the determinant is the signed product of the pivots.  (The adjugate's
    // cofactors cancel to |A|^2 2^-53 absolutely: its error grew with cond(A)^2 and missed the cond(A) bound fivefold at focal 800.)
    double m00 = a00, m01 = a01, m02 = a02, b0 = sx;
    double m10 = a01, m11 = a11, m12 = a12, b1 = sy;
    double m20 = a02, m21 = a12, m22 = a22, b2 = sz;
    double sign = 1.0, t;
#define NRM_SWAP(x, y) (t = (x), (x) = (y), (y) = t)
    if (fabs(m10) > fabs(m00)) { NRM_SWAP(m00, m10); NRM_SWAP(m01, m11); NRM_SWAP(m02, m12); NRM_SWAP(b0, b1); sign = -sign; }
    if (fabs(m20) > fabs(m00)) { NRM_SWAP(m00, m20); NRM_SWAP(m01, m21); NRM_SWAP(m02, m22); NRM_SWAP(b0, b2); sign = -sign; }
    bool singular = m00 == 0.0;  // an empty column: det = 0 without dividing by it
    const double p0 = singular ? 1.0 : m00, l1 = m10 / p0, l2 = m20 / p0;
    m11 -= l1 * m01, m12 -= l1 * m02, b1 -= l1 * b0;
    m21 -= l2 * m01, m22 -= l2 * m02, b2 -= l2 * b0;
    if (fabs(m21) > fabs(m11)) { NRM_SWAP(m11, m21); NRM_SWAP(m12, m22); NRM_SWAP(b1, b2); sign = -sign; }
#undef NRM_SWAP
    singular = singular || m11 == 0.0;
    const double l3 = m21 / (m11 == 0.0 ? 1.0 : m11);
    m22 -= l3 * m12, b2 -= l3 * b1;
    const double det = singular ? 0.0 : sign * ((m00 * m11) * m22);
    double vx = sx, vy = sy, vz = sz;  // det < eps: the reference puts the identity in A's place
    if (!(det < eps)) {                // (a NaN determinant takes the solve, and comes out as NaN -> 0)
        vz = b2 / m22;
        vy = (b1 - m12 * vz) / m11;
        vx = ((b0 - m01 * vy) - m02 * vz) / m00;
    }
    const double len = sqrt((vx * vx + vy * vy) + vz * vz);
    const double div = len < 1e-12 ? 1e-12 : len;  // max(len, 1e-12) that keeps a NaN length
    vx /= div;
    vy /= div;
    vz /= div;
    float* out = normals + ((size_t)py * (size_t)W + (size_t)px) * 3;
    out[0] = (float)-(vx != vx ? 0.0 : vx);
    out[1] = (float)-(vy != vy ? 0.0 : vy);
    out[2] = (float)-(vz != vz ? 0.0 : vz);
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
static int normals_check_frame(const char* what, int H, int W)
{
    if (H <= 0 || W <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: H=%d W=%d (need both > 0)", what, H, W);
    if ((int64_t)H * (int64_t)W >= 0x7fffff00LL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: H=%d W=%d has too many pixels (need H*W < 2^31 - 256)", what, H, W);
    return GSR_OK;
}

extern "C" int gsr_depth_points(int H, int W, const float* depth, const float* K, const float* c2w, float* points, void* stream)
{
    if (int rc = normals_check_frame("depth points", H, W)) return rc;
    if (!depth || !K || !c2w || !points) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "depth points: depth, K, c2w or points is NULL");
    const uint32_t n = (uint32_t)H * (uint32_t)W;
    hipLaunchKernelGGL(depth_points_kernel, dim3((n + NRM_THREADS - 1u) / NRM_THREADS), dim3(NRM_THREADS), 0, (hipStream_t)stream, H, W, depth, K, c2w,
                       points);
    GSR_HIP(hipGetLastError(), "depth points");
    return GSR_OK;
}

extern "C" int gsr_point_normals(int H, int W, const float* points, int size, float gamma, double eps, float* normals, void* stream)
{
    if (int rc = normals_check_frame("point normals", H, W)) return rc;
    if (size < 1 || size > 15 || size % 2 == 0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "point normals: size=%d (need an odd size, 1 .. 15)", size);
    if (!points || !normals) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "point normals: points or normals is NULL");
    const int tiles_x = (W + NRM_TILE - 1) / NRM_TILE, tiles_y = (H + NRM_TILE - 1) / NRM_TILE;  // tiles_x * tiles_y <= 2^27 + 2^24
    hipLaunchKernelGGL(point_normals_kernel, dim3((uint32_t)tiles_x * (uint32_t)tiles_y), dim3(NRM_THREADS), 0, (hipStream_t)stream, H, W, tiles_x, points,
                       size, gamma, eps, normals);
    GSR_HIP(hipGetLastError(), "point normals");
    return GSR_OK;
}
