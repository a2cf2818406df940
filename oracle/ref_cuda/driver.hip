// C ABI over the reference's CudaRasterizer::Rasterizer (cuda_rasterizer/rasterizer.h), built by `make -C oracle ref`
// into oracle/_ref/libgsref.so and loaded by oracle/ref_cuda.py.  TEST INFRASTRUCTURE: host arrays in, host arrays
// out; this file owns every device allocation (hipMalloc / hipMemcpy, default stream, synchronous).  What it does
// around the reference's calls follows what the reference's torch binding does around them (rasterize_points.cu):
// zero-filled outputs, P == 0 skips the call, absent optional inputs are null pointers.  `prefiltered` is always
// false (the reference traps the kernel when a prefiltered point fails the frustum test).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include <hip/hip_runtime.h>

#include "rasterizer.h"
#include "rasterizer_impl.h"

namespace {

thread_local char g_err[256] = "";

struct Fail {};

void check(hipError_t e, const char* what)
{
    if (e != hipSuccess) {
        snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
        throw Fail{};
    }
}

// Every device allocation of one call; freed when the call returns (the three opaque buffers of a forward live on in
// its Frame until gsref_release).
struct Arena {
    std::vector<void*> ptrs;
    ~Arena() { for (void* p : ptrs) (void)hipFree(p); }
    // zero-filled allocation, size rounded up to 256 bytes and never zero: never returns null
    char* zeros(size_t bytes)
    {
        size_t n = ((bytes ? bytes : 1) + 255) & ~size_t(255);
        void* p = nullptr;
        check(hipMalloc(&p, n), "hipMalloc");
        ptrs.push_back(p);
        check(hipMemset(p, 0, n), "hipMemset");
        return static_cast<char*>(p);
    }
    // device copy of n elements of a host array; null stays null (an absent optional input)
    template <typename T> T* up(const T* host, size_t n)
    {
        if (!host) return nullptr;
        char* d = zeros(n * sizeof(T));
        if (n) check(hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy H2D");
        return reinterpret_cast<T*>(d);
    }
    template <typename T> T* out(size_t n) { return reinterpret_cast<T*>(zeros(n * sizeof(T))); }
};

template <typename T> void down(T* host, const void* dev, size_t n)
{
    if (host && n) check(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy D2H");
}

void sync(const char* what)
{
    check(hipGetLastError(), what);
    check(hipDeviceSynchronize(), what);
}

// One forward's opaque buffers, kept for gsref_state / gsref_backward.
struct Frame {
    Arena mem;
    char *geom = nullptr, *binning = nullptr, *img = nullptr;
    int P = 0, W = 0, H = 0, R = 0;
};

std::function<char*(size_t)> grower(Arena& a, char*& slot)
{
    return [&a, &slot](size_t n) { slot = a.zeros(n); return slot; };
}

}  // namespace

extern "C" {

const char* gsref_last_error() { return g_err; }

void gsref_release(void* frame) { delete static_cast<Frame*>(frame); }

// Rasterizer::forward.  Returns num_rendered (>= 0) or -1 (gsref_last_error()).  *frame_out receives the handle that
// gsref_state / gsref_backward read; release it with gsref_release.  shs / colors_precomp / scales / rotations /
// cov3D_precomp may be null.  out_color [3,H,W], out_depth [H,W], out_unc [H,W], radii [P]: host, zero-filled here.
int gsref_forward(int P, int D, int M, const float* bg, int W, int H, const float* means3D, const float* shs,
                  const float* colors_precomp, const float* opacities, const float* uncertainties, const float* scales,
                  float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                  const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, float* out_color,
                  float* out_depth, float* out_unc, int* radii, void** frame_out)
{
    Frame* f = new Frame;
    f->P = P; f->W = W; f->H = H;
    *frame_out = nullptr;
    try {
        const size_t N = size_t(W) * H;
        memset(out_color, 0, 3 * N * sizeof(float));
        memset(out_depth, 0, N * sizeof(float));
        memset(out_unc, 0, N * sizeof(float));
        memset(radii, 0, size_t(P) * sizeof(int));
        if (P != 0) {
            Arena in;
            float* d_color = in.out<float>(3 * N);
            float* d_depth = in.out<float>(N);
            float* d_unc = in.out<float>(N);
            int* d_radii = in.out<int>(P);
            f->R = CudaRasterizer::Rasterizer::forward(
                grower(f->mem, f->geom), grower(f->mem, f->binning), grower(f->mem, f->img), P, D, M, in.up(bg, 3), W, H,
                in.up(means3D, size_t(P) * 3), in.up(shs, size_t(P) * M * 3), in.up(colors_precomp, size_t(P) * 3),
                in.up(opacities, P), in.up(uncertainties, P), in.up(scales, size_t(P) * 3), scale_modifier,
                in.up(rotations, size_t(P) * 4), in.up(cov3D_precomp, size_t(P) * 6), in.up(viewmatrix, 16),
                in.up(projmatrix, 16), in.up(campos, 3), tan_fovx, tan_fovy, /*prefiltered=*/false, d_color, d_depth, d_unc,
                d_radii, /*debug=*/false);
            sync("Rasterizer::forward");
            down(out_color, d_color, 3 * N);
            down(out_depth, d_depth, N);
            down(out_unc, d_unc, N);
            down(radii, d_radii, P);
        }
    } catch (const Fail&) {
        delete f;
        return -1;
    } catch (const std::exception& e) {
        snprintf(g_err, sizeof g_err, "Rasterizer::forward: %s", e.what());
        delete f;
        return -1;
    }
    *frame_out = f;
    return f->R;
}

// The state a forward left in its three opaque buffers, carved with the reference's own fromChunk.  Every pointer may be
// null.  Per Gaussian [P]: tiles_touched, clamped [P,3] (bytes), means2D [P,2], depths, cov3D [P,6], conic_opacity [P,4],
// rgb [P,3], unc, point_offsets.  Per tile: ranges [tiles,2].  Per instance [R]: point_list, point_keys.  Per pixel: n_contrib,
// final_T.
int gsref_state(void* frame, uint32_t* tiles_touched, unsigned char* clamped, float* means2D, float* depths, float* cov3D,
                float* conic_opacity, float* rgb, float* unc, uint32_t* point_offsets, uint32_t* ranges, uint32_t* point_list,
                uint64_t* point_keys, uint32_t* n_contrib, float* final_T)
{
    Frame* f = static_cast<Frame*>(frame);
    if (!f || f->P == 0) return 0;
    try {
        static_assert(sizeof(bool) == 1, "clamped is copied out as bytes");
        const size_t P = f->P, N = size_t(f->W) * f->H, R = f->R;
        const size_t tiles = size_t((f->W + 15) / 16) * ((f->H + 15) / 16);
        char* c = f->geom;
        auto g = CudaRasterizer::GeometryState::fromChunk(c, P);
        c = f->img;
        auto im = CudaRasterizer::ImageState::fromChunk(c, N);
        c = f->binning;
        auto b = CudaRasterizer::BinningState::fromChunk(c, R);
        down(tiles_touched, g.tiles_touched, P);
        down(clamped, g.clamped, 3 * P);
        down(means2D, g.means2D, 2 * P);
        down(depths, g.depths, P);
        down(cov3D, g.cov3D, 6 * P);
        down(conic_opacity, g.conic_opacity, 4 * P);
        down(rgb, g.rgb, 3 * P);
        down(unc, g.uncertainty, P);
        down(point_offsets, g.point_offsets, P);
        down(ranges, im.ranges, 2 * tiles);
        down(n_contrib, im.n_contrib, N);
        down(final_T, im.accum_alpha, N);
        down(point_list, b.point_list, R);
        down(point_keys, b.point_list_keys, R);
    } catch (const Fail&) {
        return -1;
    }
    return 0;
}

// Rasterizer::backward on the buffers of `frame`.  Outputs (host, zero-filled here): dL_dmean2D [P,3], dL_dconic [P,4],
// dL_dopacity [P], dL_dcolor [P,3], dL_ddepth [P], dL_dunc [P], dL_dmean3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3],
// dL_dscale [P,3], dL_drot [P,4].  Returns 0 or -1.
int gsref_backward(void* frame, int D, int M, const float* bg, const float* means3D, const float* shs,
                   const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                   const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
                   float tan_fovx, float tan_fovy, const int* radii, const float* dL_dpix, const float* dL_dpix_depth,
                   const float* dL_dpix_unc, float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor,
                   float* dL_ddepth, float* dL_dunc, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                   float* dL_drot)
{
    Frame* f = static_cast<Frame*>(frame);
    if (!f) { snprintf(g_err, sizeof g_err, "gsref_backward: no frame"); return -1; }
    try {
        const size_t P = f->P, N = size_t(f->W) * f->H;
        struct { float* host; size_t n; float* dev; } o[] = {
            {dL_dmean2D, 3 * P, nullptr}, {dL_dconic, 4 * P, nullptr}, {dL_dopacity, P, nullptr}, {dL_dcolor, 3 * P, nullptr},
            {dL_ddepth, P, nullptr}, {dL_dunc, P, nullptr}, {dL_dmean3D, 3 * P, nullptr}, {dL_dcov3D, 6 * P, nullptr},
            {dL_dsh, P * M * 3, nullptr}, {dL_dscale, 3 * P, nullptr}, {dL_drot, 4 * P, nullptr}};
        for (auto& e : o) memset(e.host, 0, e.n * sizeof(float));
        if (P != 0) {
            Arena in;
            for (auto& e : o) e.dev = in.out<float>(e.n);
            CudaRasterizer::Rasterizer::backward(
                f->P, D, M, f->R, in.up(bg, 3), f->W, f->H, in.up(means3D, 3 * P), in.up(shs, P * M * 3),
                in.up(colors_precomp, 3 * P), in.up(scales, 3 * P), scale_modifier, in.up(rotations, 4 * P),
                in.up(cov3D_precomp, 6 * P), in.up(viewmatrix, 16), in.up(projmatrix, 16), in.up(campos, 3), tan_fovx, tan_fovy,
                in.up(radii, P), f->geom, f->binning, f->img, in.up(dL_dpix, 3 * N), in.up(dL_dpix_depth, N),
                in.up(dL_dpix_unc, N), o[0].dev, o[1].dev, o[2].dev, o[3].dev, o[4].dev, o[5].dev, o[6].dev, o[7].dev, o[8].dev,
                o[9].dev, o[10].dev, /*debug=*/false);
            sync("Rasterizer::backward");
            for (auto& e : o) down(e.host, e.dev, e.n);
        }
    } catch (const Fail&) {
        return -1;
    } catch (const std::exception& e) {
        snprintf(g_err, sizeof g_err, "Rasterizer::backward: %s", e.what());
        return -1;
    }
    return 0;
}

// Rasterizer::markVisible -> present [P] (bytes).
int gsref_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, unsigned char* present)
{
    try {
        memset(present, 0, size_t(P));
        if (P != 0) {
            Arena in;
            bool* d = in.out<bool>(P);
            CudaRasterizer::Rasterizer::markVisible(P, in.up(means3D, size_t(P) * 3), in.up(viewmatrix, 16), in.up(projmatrix, 16), d);
            sync("Rasterizer::markVisible");
            down(reinterpret_cast<bool*>(present), d, P);
        }
    } catch (const Fail&) {
        return -1;
    }
    return 0;
}

// Rasterizer::visible_filter (x == y == null) or Rasterizer::position2D_filter -> radii [P] (+ x [P], y [P]).
int gsref_filter(int P, int M, int W, int H, const float* means3D, const float* scales, float scale_modifier,
                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                 float tan_fovx, float tan_fovy, int* radii, float* x, float* y)
{
    try {
        memset(radii, 0, size_t(P) * sizeof(int));
        if (x) memset(x, 0, size_t(P) * sizeof(float));
        if (y) memset(y, 0, size_t(P) * sizeof(float));
        if (P != 0) {
            Arena in;
            char *geom = nullptr, *binning = nullptr, *img = nullptr;
            int* d_radii = in.out<int>(P);
            float* d_m = in.up(means3D, size_t(P) * 3);
            float* d_s = in.up(scales, size_t(P) * 3);
            float* d_r = in.up(rotations, size_t(P) * 4);
            float* d_c = in.up(cov3D_precomp, size_t(P) * 6);
            float* d_v = in.up(viewmatrix, 16);
            float* d_p = in.up(projmatrix, 16);
            if (x && y) {
                float* d_x = in.out<float>(P);
                float* d_y = in.out<float>(P);
                CudaRasterizer::Rasterizer::position2D_filter(grower(in, geom), grower(in, binning), grower(in, img), P, M, W, H, d_m,
                                                              d_s, scale_modifier, d_r, d_c, d_v, d_p, tan_fovx, tan_fovy,
                                                              /*prefiltered=*/false, d_radii, d_x, d_y, /*debug=*/false);
                sync("Rasterizer::position2D_filter");
                down(x, d_x, P);
                down(y, d_y, P);
            } else {
                CudaRasterizer::Rasterizer::visible_filter(grower(in, geom), grower(in, binning), grower(in, img), P, M, W, H, d_m, d_s,
                                                           scale_modifier, d_r, d_c, d_v, d_p, tan_fovx, tan_fovy,
                                                           /*prefiltered=*/false, d_radii, /*debug=*/false);
                sync("Rasterizer::visible_filter");
            }
            down(radii, d_radii, P);
        }
    } catch (const Fail&) {
        return -1;
    } catch (const std::exception& e) {
        snprintf(g_err, sizeof g_err, "Rasterizer filter: %s", e.what());
        return -1;
    }
    return 0;
}

}  // extern "C"
