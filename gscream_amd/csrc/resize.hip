// resize.hip -- PIL's Image.resize on the device: the step between a decoded picture and the tensor a Camera or a metric holds.
// readImages (train.py:887-902) resizes every mask with LANCZOS; loadCam (utils/camera_utils.py:19-102) sends every image, mask and
// depth map through pil_image.resize(resolution) with PIL's default BICUBIC (utils/general_utils.py:35-75).  The rule is in
// include/gsraster.h ("Resize") in full; the coefficient tables are built on the host in double (gscream_amd/resize.py) and arrive
// as ordinary device tensors.
//
// One launch per axis, the intermediate in HBM, rounded to the picture's own type as PIL rounds it:
//   horizontal : a workgroup takes RZ_TILE = 64 consecutive outputs of RZ_ROWS = 4 rows at a time, RZ_GROUPS row groups in turn.  The
//                bounds are monotone in the output index, so the sources the tile needs are ONE segment [xmin(first), xmin(last) +
//                n(last)) of the row, 64 scale + 2 support elements at most; it is staged in LDS (consecutive bytes / dwords, the loads
//                coalesced) together with the tile's 64 coefficient rows.  A thread owns one output pixel, all its channels.
//                ksize = 2 ceil(support) + 1 is odd, so the 64 coefficient rows start an odd number of dwords (or of doubles) apart:
//                a half-wave reading tap k of its 32 rows touches 32 different banks.
//                A segment or a table beyond the LDS tile (200 -> 7 with LANCZOS has 173 taps) is read from global memory by the same
//                loop with the same arithmetic; the choice is per workgroup and uniform.
//   vertical   : a thread owns one element of an output row (W C bytes or W floats, consecutive over the lanes: the loads and stores
//                are coalesced) and walks its taps down the column; the bound and the coefficients are the same for the whole
//                workgroup and come through scalar loads.
//   nearest    : a gather through two index tables (NULL = the identity, which is how the loader's epilogue runs alone at equal sizes).
// Every load is inside [xmin, xmin + n) of its row: the kernels clip the table's bound to the row again (max(xmin, 0), n <= in - xmin,
// n <= ksize), so a bad table cannot take a load outside the picture.
//
// Arithmetic.  8-bit: int32 multiply-add from 2^21, an arithmetic shift by 22, a clamp.  float32: ss = ss + double(src) * k in index
// order with one rounding per operation (__dmul_rn, __dadd_rn; contraction is off below), over every tap of the bound -- a tap whose
// coefficient is exactly 0 meets an infinity as 0 * inf = NaN, as in PIL -- and one rounding to float32 at the end.
// Contraction is switched off below AND on the command line (Makefile, SRCFLAGS_resize): the pragma alone does not reach the bodies of
// __dmul_rn / __dadd_rn, and the chain would come out as v_fmac_f64.
// Resource usage (gfx950, -Rpass-analysis=kernel-resource-usage): DESIGN 14.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsr_api.h"

#pragma clang fp contract(off)

#define RZ_THREADS 256
#define RZ_TILE 64                       // outputs of a row per workgroup = one wave per row
#define RZ_ROWS (RZ_THREADS / RZ_TILE)   // rows computed at a time
#define RZ_GROUPS 4                      // row groups a workgroup takes in turn (it stages its coefficient rows once)
#define RZ_SEG_BYTES 2048                // LDS per staged row: 2048 bytes of an 8-bit row, 512 floats
#define RZ_K_BYTES 16384                 // LDS for the tile's coefficient rows: ksize <= 64 (int32) / 32 (double)
static_assert(RZ_TILE == 64, "a wave is one row of the tile");

struct RzBound { int xmin, n; };

__device__ __forceinline__ RzBound rz_bound(const int32_t* __restrict__ bounds, int xx, int in_len, int ksize)
{
    RzBound b;
    b.xmin = bounds[2 * xx];
    b.n = bounds[2 * xx + 1];
    if (b.xmin < 0) b.xmin = 0;
    if (b.xmin > in_len) b.xmin = in_len;
    if (b.n > in_len - b.xmin) b.n = in_len - b.xmin;
    if (b.n > ksize) b.n = ksize;
    return b;  // (n <= 0: no tap)
}

__device__ __forceinline__ int rz_clip8(int acc)
{
    const int v = acc >> GSR_RESIZE_PRECISION_BITS;  // arithmetic
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// the three forms an 8-bit result leaves in: a byte of an HWC picture, or a float of a CHW tensor with the loader's last step
__device__ __forceinline__ void rz_store8(void* __restrict__ out, int epilogue, int v, long long img_off, long long row_stride, int y, int x, int c,
                                          int C, int H_out)
{
    if (epilogue == GSR_RESIZE_U8) {
        ((uint8_t*)out)[img_off + (long long)y * row_stride + (long long)x * C + c] = (uint8_t)v;
    } else {
        const float f = epilogue == GSR_RESIZE_DIV255 ? __fdiv_rn((float)v, 255.0f) : (v > 0 ? 1.0f : 0.0f);
        ((float*)out)[img_off + ((long long)c * H_out + y) * row_stride + x] = f;
    }
}

// ---- horizontal pass, 8-bit --------------------------------------------------------------------------------------------------------
template <int C>
__global__ void __launch_bounds__(RZ_THREADS) resize_h_u8_kernel(const uint8_t* __restrict__ src, long long src_image_stride, long long src_row_stride,
                                                                 int H, int W, int out_len, const int32_t* __restrict__ bounds,
                                                                 const int32_t* __restrict__ coeffs, int ksize, void* __restrict__ out,
                                                                 long long out_image_stride, long long out_row_stride, int epilogue)
{
    __shared__ uint8_t seg[RZ_ROWS][RZ_SEG_BYTES];
    __shared__ int32_t ktab[RZ_K_BYTES / 4];
    const int lane = (int)threadIdx.x % RZ_TILE, wrow = (int)threadIdx.x / RZ_TILE;
    const int x0 = (int)blockIdx.x * RZ_TILE;
    const int x1 = x0 + RZ_TILE < out_len ? x0 + RZ_TILE : out_len;
    const int xx = x0 + lane;
    const bool live = xx < out_len;
    const RzBound first = rz_bound(bounds, x0, W, ksize), last = rz_bound(bounds, x1 - 1, W, ksize);
    RzBound mine = first;
    if (live) mine = rz_bound(bounds, xx, W, ksize);
    // the tile's segment; a table that is not monotone (never PIL's) leaves the LDS path
    const int seg0 = first.xmin, seg_len = last.xmin + last.n - first.xmin;
    bool in_lds = seg_len >= 0 && (long long)seg_len * C <= RZ_SEG_BYTES;
    {
        const int ok = !live || (mine.xmin >= seg0 && mine.xmin + mine.n <= seg0 + seg_len);
        in_lds = in_lds && __syncthreads_and(ok);
    }
    const bool k_lds = (long long)RZ_TILE * ksize * 4 <= RZ_K_BYTES;
    if (k_lds)
        for (int i = (int)threadIdx.x; i < (x1 - x0) * ksize; i += RZ_THREADS) ktab[i] = coeffs[(long long)x0 * ksize + i];
    const int32_t* __restrict__ kglobal = coeffs + (long long)xx * ksize;
    const int32_t* kshared = ktab + lane * ksize;
    const uint8_t* __restrict__ image = src + (long long)blockIdx.z * src_image_stride;
    const long long out_img = (long long)blockIdx.z * out_image_stride;
    const int H_out = H;
    const int ybase = (int)blockIdx.y * (RZ_ROWS * RZ_GROUPS);
    for (int g = 0; g < RZ_GROUPS; g++) {
        const int y = ybase + g * RZ_ROWS + wrow;
        __syncthreads();  // the table is staged; the previous group's segment has been read
        if (in_lds) {
            for (int r = 0; r < RZ_ROWS; r++) {
                const int yr = ybase + g * RZ_ROWS + r;
                if (yr >= H) break;
                const uint8_t* __restrict__ row = image + (long long)yr * src_row_stride + (long long)seg0 * C;
                for (int i = (int)threadIdx.x; i < seg_len * C; i += RZ_THREADS) seg[r][i] = row[i];
            }
        }
        __syncthreads();
        if (!live || y >= H) continue;
        int acc[C];
#pragma unroll
        for (int c = 0; c < C; c++) acc[c] = 1 << (GSR_RESIZE_PRECISION_BITS - 1);
        if (in_lds) {
            const uint8_t* p = &seg[wrow][(mine.xmin - seg0) * C];
            for (int k = 0; k < mine.n; k++) {
                const int kv = k_lds ? kshared[k] : kglobal[k];
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] += (int)p[k * C + c] * kv;
            }
        } else {
            const uint8_t* __restrict__ p = image + (long long)y * src_row_stride + (long long)mine.xmin * C;
            for (int k = 0; k < mine.n; k++) {
                const int kv = k_lds ? kshared[k] : kglobal[k];
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] += (int)p[(long long)k * C + c] * kv;
            }
        }
#pragma unroll
        for (int c = 0; c < C; c++) rz_store8(out, epilogue, rz_clip8(acc[c]), out_img, out_row_stride, y, xx, c, C, H_out);
    }
}

// ---- horizontal pass, float32 ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RZ_THREADS) resize_h_f32_kernel(const float* __restrict__ src, long long src_image_stride, long long src_row_stride,
                                                                  int H, int W, int out_len, const int32_t* __restrict__ bounds,
                                                                  const double* __restrict__ coeffs, int ksize, float* __restrict__ out,
                                                                  long long out_image_stride, long long out_row_stride)
{
    __shared__ float seg[RZ_ROWS][RZ_SEG_BYTES / 4];
    __shared__ double ktab[RZ_K_BYTES / 8];
    const int lane = (int)threadIdx.x % RZ_TILE, wrow = (int)threadIdx.x / RZ_TILE;
    const int x0 = (int)blockIdx.x * RZ_TILE;
    const int x1 = x0 + RZ_TILE < out_len ? x0 + RZ_TILE : out_len;
    const int xx = x0 + lane;
    const bool live = xx < out_len;
    const RzBound first = rz_bound(bounds, x0, W, ksize), last = rz_bound(bounds, x1 - 1, W, ksize);
    RzBound mine = first;
    if (live) mine = rz_bound(bounds, xx, W, ksize);
    const int seg0 = first.xmin, seg_len = last.xmin + last.n - first.xmin;
    bool in_lds = seg_len >= 0 && seg_len <= RZ_SEG_BYTES / 4;
    {
        const int ok = !live || (mine.xmin >= seg0 && mine.xmin + mine.n <= seg0 + seg_len);
        in_lds = in_lds && __syncthreads_and(ok);
    }
    const bool k_lds = (long long)RZ_TILE * ksize * 8 <= RZ_K_BYTES;
    if (k_lds)
        for (int i = (int)threadIdx.x; i < (x1 - x0) * ksize; i += RZ_THREADS) ktab[i] = coeffs[(long long)x0 * ksize + i];
    const double* __restrict__ kglobal = coeffs + (long long)xx * ksize;
    const double* kshared = ktab + lane * ksize;
    const float* __restrict__ image = src + (long long)blockIdx.z * src_image_stride;
    float* __restrict__ out_image = out + (long long)blockIdx.z * out_image_stride;
    const int ybase = (int)blockIdx.y * (RZ_ROWS * RZ_GROUPS);
    for (int g = 0; g < RZ_GROUPS; g++) {
        const int y = ybase + g * RZ_ROWS + wrow;
        __syncthreads();
        if (in_lds) {
            for (int r = 0; r < RZ_ROWS; r++) {
                const int yr = ybase + g * RZ_ROWS + r;
                if (yr >= H) break;
                const float* __restrict__ row = image + (long long)yr * src_row_stride + seg0;
                for (int i = (int)threadIdx.x; i < seg_len; i += RZ_THREADS) seg[r][i] = row[i];
            }
        }
        __syncthreads();
        if (!live || y >= H) continue;
        double ss = 0.0;
        if (in_lds) {
            const float* p = &seg[wrow][mine.xmin - seg0];
            for (int k = 0; k < mine.n; k++) ss = __dadd_rn(ss, __dmul_rn((double)p[k], k_lds ? kshared[k] : kglobal[k]));
        } else {
            const float* __restrict__ p = image + (long long)y * src_row_stride + mine.xmin;
            for (int k = 0; k < mine.n; k++) ss = __dadd_rn(ss, __dmul_rn((double)p[k], k_lds ? kshared[k] : kglobal[k]));
        }
        out_image[(long long)y * out_row_stride + xx] = __double2float_rn(ss);
    }
}

// ---- vertical pass -----------------------------------------------------------------------------------------------------------------
// grid: (ceil(W C / 256), out_len, n); a thread owns byte j = x C + c of output row blockIdx.y
__global__ void __launch_bounds__(RZ_THREADS) resize_v_u8_kernel(const uint8_t* __restrict__ src, long long src_image_stride, long long src_row_stride,
                                                                 int H, int W, int C, int out_len, const int32_t* __restrict__ bounds,
                                                                 const int32_t* __restrict__ coeffs, int ksize, void* __restrict__ out,
                                                                 long long out_image_stride, long long out_row_stride, int epilogue)
{
    const int j = (int)(blockIdx.x * RZ_THREADS + threadIdx.x), yy = (int)blockIdx.y;
    if (j >= W * C) return;
    const RzBound b = rz_bound(bounds, yy, H, ksize);
    const int32_t* __restrict__ kk = coeffs + (long long)yy * ksize;
    const uint8_t* __restrict__ p = src + (long long)blockIdx.z * src_image_stride + (long long)b.xmin * src_row_stride + j;
    int acc = 1 << (GSR_RESIZE_PRECISION_BITS - 1);
    for (int k = 0; k < b.n; k++) acc += (int)p[(long long)k * src_row_stride] * kk[k];
    const int x = j / C;
    rz_store8(out, epilogue, rz_clip8(acc), (long long)blockIdx.z * out_image_stride, out_row_stride, yy, x, j - x * C, C, out_len);
}

__global__ void __launch_bounds__(RZ_THREADS) resize_v_f32_kernel(const float* __restrict__ src, long long src_image_stride, long long src_row_stride,
                                                                  int H, int W, int out_len, const int32_t* __restrict__ bounds,
                                                                  const double* __restrict__ coeffs, int ksize, float* __restrict__ out,
                                                                  long long out_image_stride, long long out_row_stride)
{
    const int x = (int)(blockIdx.x * RZ_THREADS + threadIdx.x), yy = (int)blockIdx.y;
    if (x >= W) return;
    const RzBound b = rz_bound(bounds, yy, H, ksize);
    const double* __restrict__ kk = coeffs + (long long)yy * ksize;
    const float* __restrict__ p = src + (long long)blockIdx.z * src_image_stride + (long long)b.xmin * src_row_stride + x;
    double ss = 0.0;
    for (int k = 0; k < b.n; k++) ss = __dadd_rn(ss, __dmul_rn((double)p[(long long)k * src_row_stride], kk[k]));
    out[(long long)blockIdx.z * out_image_stride + (long long)yy * out_row_stride + x] = __double2float_rn(ss);
}

// ---- NEAREST: a gather through two index tables ------------------------------------------------------------------------------------
// grid: (ceil(W_out / 256), H_out, n); a thread owns one output pixel
__device__ __forceinline__ int rz_index(const int32_t* __restrict__ table, int i, int in_len)
{
    int v = table ? table[i] : i;
    if (v < 0) v = 0;
    if (v > in_len - 1) v = in_len - 1;
    return v;
}

__global__ void __launch_bounds__(RZ_THREADS) resize_nearest_u8_kernel(const uint8_t* __restrict__ src, long long src_image_stride,
                                                                       long long src_row_stride, int H, int W, int C, int H_out, int W_out,
                                                                       const int32_t* __restrict__ yidx, const int32_t* __restrict__ xidx,
                                                                       void* __restrict__ out, long long out_image_stride, long long out_row_stride,
                                                                       int epilogue)
{
    const int x = (int)(blockIdx.x * RZ_THREADS + threadIdx.x), y = (int)blockIdx.y;
    if (x >= W_out) return;
    const int sx = rz_index(xidx, x, W), sy = rz_index(yidx, y, H);
    const uint8_t* __restrict__ p = src + (long long)blockIdx.z * src_image_stride + (long long)sy * src_row_stride + (long long)sx * C;
    for (int c = 0; c < C; c++) rz_store8(out, epilogue, (int)p[c], (long long)blockIdx.z * out_image_stride, out_row_stride, y, x, c, C, H_out);
}

__global__ void __launch_bounds__(RZ_THREADS) resize_nearest_f32_kernel(const float* __restrict__ src, long long src_image_stride,
                                                                        long long src_row_stride, int H, int W, int H_out, int W_out,
                                                                        const int32_t* __restrict__ yidx, const int32_t* __restrict__ xidx,
                                                                        float* __restrict__ out, long long out_image_stride, long long out_row_stride)
{
    const int x = (int)(blockIdx.x * RZ_THREADS + threadIdx.x), y = (int)blockIdx.y;
    if (x >= W_out) return;
    const int sx = rz_index(xidx, x, W), sy = rz_index(yidx, y, H);
    // (the bits are moved as they are: a NaN keeps its payload)
    const uint32_t* __restrict__ p = (const uint32_t*)src;
    ((uint32_t*)out)[(long long)blockIdx.z * out_image_stride + (long long)y * out_row_stride + x] =
        p[(long long)blockIdx.z * src_image_stride + (long long)sy * src_row_stride + sx];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static inline uint32_t rz_div_up(long long a, long long b) { return (uint32_t)((a + b - 1) / b); }

static hipError_t resize_launch_nearest(const void* src, long long src_image_stride, long long src_row_stride, int n, int H, int W, int C, int is_f32,
                                        int H_out, int W_out, const int32_t* yidx, const int32_t* xidx, void* out, long long out_image_stride,
                                        long long out_row_stride, int epilogue, hipStream_t stream)
{
    const dim3 grid(rz_div_up(W_out, RZ_THREADS), (uint32_t)H_out, (uint32_t)n);
    if (is_f32)
        hipLaunchKernelGGL(resize_nearest_f32_kernel, grid, dim3(RZ_THREADS), 0, stream, (const float*)src, src_image_stride, src_row_stride, H, W,
                           H_out, W_out, yidx, xidx, (float*)out, out_image_stride, out_row_stride);
    else
        hipLaunchKernelGGL(resize_nearest_u8_kernel, grid, dim3(RZ_THREADS), 0, stream, (const uint8_t*)src, src_image_stride, src_row_stride, H, W, C,
                           H_out, W_out, yidx, xidx, out, out_image_stride, out_row_stride, epilogue);
    return hipGetLastError();
}

// ---- C entry points (include/gsraster.h): check the arguments, launch ----
static int resize_check(const char* what, const void* src, const void* out, long long src_image_stride, long long src_row_stride, int n, int H, int W,
                        int C, int H_out, int W_out, long long out_image_stride, long long out_row_stride, int epilogue)
{
    if (!src || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: src or out is NULL", what);
    if (n < 1 || H < 1 || W < 1 || H_out < 1 || W_out < 1)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: n, H, W and the output sizes must be >= 1 (got %d, %d x %d -> %d x %d)", what, n, H, W, H_out, W_out);
    if (C < 1 || C > 4) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: C=%d (need 1 .. 4)", what, C);
    if (n > 65535 || H > 65535 || W > 65535 || H_out > 65535 || W_out > 65535)
        return gsr_fail(GSR_ERR_UNSUPPORTED, "%s: n, H, W and the output sizes are at most 65535", what);
    if (epilogue != GSR_RESIZE_U8 && epilogue != GSR_RESIZE_DIV255 && epilogue != GSR_RESIZE_GT0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: epilogue=%d", what, epilogue);
    if (src_row_stride < (long long)W * C || (n > 1 && src_image_stride < (long long)(H - 1) * src_row_stride + (long long)W * C))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: source strides %lld / %lld are below the row or the picture", what, src_image_stride, src_row_stride);
    if (epilogue == GSR_RESIZE_U8) {
        if (out_row_stride < (long long)W_out * C || (n > 1 && out_image_stride < (long long)(H_out - 1) * out_row_stride + (long long)W_out * C))
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: output strides %lld / %lld are below the row or the picture", what, out_image_stride, out_row_stride);
    } else if (out_row_stride != W_out || out_image_stride != (long long)C * H_out * W_out) {
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: the float forms are contiguous [n][C][H'][W'] (strides %lld / %lld)", what, out_image_stride, out_row_stride);
    }
    return GSR_OK;
}

static int resize_check_pass(const char* what, int axis, int out_len, const void* bounds, const void* coeffs, int ksize)
{
    if (axis != GSR_RESIZE_HORIZONTAL && axis != GSR_RESIZE_VERTICAL) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: axis=%d", what, axis);
    if (!bounds || !coeffs) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: bounds or coeffs is NULL", what);
    if (ksize < 1 || out_len < 1 || (long long)out_len * ksize > 0x7fffffffLL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: ksize=%d, out_len=%d", what, ksize, out_len);
    return GSR_OK;
}

extern "C" int gsr_resize_u8(const uint8_t* src, long long src_image_stride, long long src_row_stride, int n, int H, int W, int C, int axis, int out_len,
                             const int32_t* bounds, const int32_t* coeffs, int ksize, void* out, long long out_image_stride, long long out_row_stride,
                             int epilogue, void* stream_)
{
    if (int rc = resize_check_pass("resize_u8", axis, out_len, bounds, coeffs, ksize)) return rc;
    const int H_out = axis == GSR_RESIZE_VERTICAL ? out_len : H, W_out = axis == GSR_RESIZE_VERTICAL ? W : out_len;
    if (int rc = resize_check("resize_u8", src, out, src_image_stride, src_row_stride, n, H, W, C, H_out, W_out, out_image_stride, out_row_stride, epilogue))
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (axis == GSR_RESIZE_VERTICAL) {
        hipLaunchKernelGGL(resize_v_u8_kernel, dim3(rz_div_up((long long)W * C, RZ_THREADS), (uint32_t)out_len, (uint32_t)n), dim3(RZ_THREADS), 0, stream,
                           src, src_image_stride, src_row_stride, H, W, C, out_len, bounds, coeffs, ksize, out, out_image_stride, out_row_stride,
                           epilogue);
        GSR_HIP(hipGetLastError(), "resize_u8");
        return GSR_OK;
    }
    const dim3 grid(rz_div_up(out_len, RZ_TILE), rz_div_up(H, RZ_ROWS * RZ_GROUPS), (uint32_t)n);
#define RZ_LAUNCH_H(CH)                                                                                                                        \
    hipLaunchKernelGGL(resize_h_u8_kernel<CH>, grid, dim3(RZ_THREADS), 0, stream, src, src_image_stride, src_row_stride, H, W, out_len, bounds, \
                       coeffs, ksize, out, out_image_stride, out_row_stride, epilogue)
    switch (C) {
    case 1: RZ_LAUNCH_H(1); break;
    case 2: RZ_LAUNCH_H(2); break;
    case 3: RZ_LAUNCH_H(3); break;
    default: RZ_LAUNCH_H(4); break;
    }
#undef RZ_LAUNCH_H
    GSR_HIP(hipGetLastError(), "resize_u8");
    return GSR_OK;
}

extern "C" int gsr_resize_f32(const float* src, long long src_image_stride, long long src_row_stride, int n, int H, int W, int axis, int out_len,
                              const int32_t* bounds, const double* coeffs, int ksize, float* out, long long out_image_stride, long long out_row_stride,
                              void* stream_)
{
    if (int rc = resize_check_pass("resize_f32", axis, out_len, bounds, coeffs, ksize)) return rc;
    const int H_out = axis == GSR_RESIZE_VERTICAL ? out_len : H, W_out = axis == GSR_RESIZE_VERTICAL ? W : out_len;
    if (int rc = resize_check("resize_f32", src, out, src_image_stride, src_row_stride, n, H, W, 1, H_out, W_out, out_image_stride, out_row_stride,
                              GSR_RESIZE_U8))
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (axis == GSR_RESIZE_VERTICAL)
        hipLaunchKernelGGL(resize_v_f32_kernel, dim3(rz_div_up(W, RZ_THREADS), (uint32_t)out_len, (uint32_t)n), dim3(RZ_THREADS), 0, stream, src,
                           src_image_stride, src_row_stride, H, W, out_len, bounds, coeffs, ksize, out, out_image_stride, out_row_stride);
    else
        hipLaunchKernelGGL(resize_h_f32_kernel, dim3(rz_div_up(out_len, RZ_TILE), rz_div_up(H, RZ_ROWS * RZ_GROUPS), (uint32_t)n), dim3(RZ_THREADS), 0,
                           stream, src, src_image_stride, src_row_stride, H, W, out_len, bounds, coeffs, ksize, out, out_image_stride,
                           out_row_stride);
    GSR_HIP(hipGetLastError(), "resize_f32");
    return GSR_OK;
}

extern "C" int gsr_resize_nearest_u8(const uint8_t* src, long long src_image_stride, long long src_row_stride, int n, int H, int W, int C, int H_out,
                                     int W_out, const int32_t* yidx, const int32_t* xidx, void* out, long long out_image_stride,
                                     long long out_row_stride, int epilogue, void* stream)
{
    if (int rc = resize_check("resize_nearest_u8", src, out, src_image_stride, src_row_stride, n, H, W, C, H_out, W_out, out_image_stride,
                              out_row_stride, epilogue))
        return rc;
    if ((!yidx && H_out != H) || (!xidx && W_out != W))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "resize_nearest_u8: a NULL index table is the identity and needs equal sizes");
    GSR_HIP(resize_launch_nearest(src, src_image_stride, src_row_stride, n, H, W, C, 0, H_out, W_out, yidx, xidx, out, out_image_stride, out_row_stride,
                                  epilogue, (hipStream_t)stream), "resize_nearest_u8");
    return GSR_OK;
}

extern "C" int gsr_resize_nearest_f32(const float* src, long long src_image_stride, long long src_row_stride, int n, int H, int W, int H_out, int W_out,
                                      const int32_t* yidx, const int32_t* xidx, float* out, long long out_image_stride, long long out_row_stride,
                                      void* stream)
{
    if (int rc = resize_check("resize_nearest_f32", src, out, src_image_stride, src_row_stride, n, H, W, 1, H_out, W_out, out_image_stride,
                              out_row_stride, GSR_RESIZE_U8))
        return rc;
    if ((!yidx && H_out != H) || (!xidx && W_out != W))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "resize_nearest_f32: a NULL index table is the identity and needs equal sizes");
    GSR_HIP(resize_launch_nearest(src, src_image_stride, src_row_stride, n, H, W, 1, 1, H_out, W_out, yidx, xidx, out, out_image_stride, out_row_stride,
                                  GSR_RESIZE_U8, (hipStream_t)stream), "resize_nearest_f32");
    return GSR_OK;
}
