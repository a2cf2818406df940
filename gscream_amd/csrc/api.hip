// api.hip -- the rasterizer's part of the extern "C" surface declared in include/gsraster.h (host code only): the error buffer
// behind gsr_last_error(), stage profiling, the per-thread device state and the rasterizer's entry points, up to gsr_mark_visible.
// Every other module (loss.hip, decode.hip, png.hip, ...) defines its entry points at the end of its own file (gsr_api.h).
//
// Each entry validates its arguments, carves the caller-allocated workspaces, enqueues the stage
// kernels on the caller's stream and reports failures as an int code + thread-local message.
// Orchestration replaces CudaRasterizer::Rasterizer::{forward,backward,visible_filter,
// position2D_filter,markVisible} (DGR rasterizer_impl.cu:141-153,199-347,350-530,536-643).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "gsr_api.h"
#include "gsr_common.h"

static thread_local char g_err[512] = "";

int gsr_fail(int code, const char* fmt, ...)  // (the one definition; every module reports through it, gsr_api.h)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ---- optional per-stage timing with HIP events on the caller's stream (bench / profiling only) ----
#include <mutex>
#include <vector>
static const char* const g_stage_names[GSR_NUM_STAGES] = { "preprocess", "count_scan", "scatter", "tile_sort",
                                                           "blend_forward", "blend_backward", "gauss_backward" };
struct GsrProfRec { int stage; hipEvent_t t0, t1; };
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static unsigned g_prof_mask = 0xffffffffu;
static unsigned g_prof_every = 1;                  // time every n-th invocation of a stage (gsr_profile_begin_sampled)
static unsigned g_prof_seen[GSR_NUM_STAGES] = {};  // invocations of each stage since gsr_profile_begin
static std::vector<GsrProfRec> g_prof;

struct GsrStageTimer {
    bool on = false;
    GsrProfRec rec{};
    hipStream_t stream;
    GsrStageTimer(int stage, hipStream_t s) : stream(s)
    {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        if (!g_prof_on || !((g_prof_mask >> stage) & 1u)) return;
        if (g_prof_seen[stage]++ % g_prof_every != 0u) return;  // sampled: the markers perturb the stream (a bubble on either side)
        if (hipEventCreate(&rec.t0) != hipSuccess || hipEventCreate(&rec.t1) != hipSuccess) return;
        rec.stage = stage;
        on = hipEventRecord(rec.t0, stream) == hipSuccess;
    }
    ~GsrStageTimer()
    {
        if (!on) return;
        (void)hipEventRecord(rec.t1, stream);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof.push_back(rec);
    }
};

// debug semantics of the reference's CHECK_CUDA (auxiliary.h:166-173): sync + check after a stage
#define GSR_STAGE(stage_id, stream, debug, expr, what)               \
    do {                                                             \
        {                                                            \
            GsrStageTimer timer_(stage_id, stream);                  \
            GSR_HIP(expr, what);                                     \
        }                                                            \
        if (debug) GSR_HIP(hipStreamSynchronize(stream), what);      \
    } while (0)

extern "C" const char* gsr_stage_name(int stage)
{
    return (stage >= 0 && stage < GSR_NUM_STAGES) ? g_stage_names[stage] : "";
}

extern "C" int gsr_profile_begin_sampled(unsigned stage_mask, unsigned every)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_mask = stage_mask ? stage_mask : 0xffffffffu;
    g_prof_every = every ? every : 1u;
    for (unsigned& n : g_prof_seen) n = 0u;
    for (auto& r : g_prof) { (void)hipEventDestroy(r.t0); (void)hipEventDestroy(r.t1); }
    g_prof.clear();
    g_prof_on = true;
    return GSR_OK;
}

extern "C" int gsr_profile_begin(unsigned stage_mask) { return gsr_profile_begin_sampled(stage_mask, 1u); }

extern "C" int gsr_profile_end(gsr_profile* out_host)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = false;
    if (!out_host) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "out_host is NULL");
    memset(out_host, 0, sizeof(*out_host));
    int rc = GSR_OK;
    for (auto& r : g_prof) {
        float ms = 0.f;
        hipError_t e = hipEventSynchronize(r.t1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, r.t0, r.t1);
        if (e != hipSuccess) rc = gsr_fail(GSR_ERR_HIP, "profile: %s", hipGetErrorString(e));
        else { out_host->total_ms[r.stage] += ms; out_host->launches[r.stage] += 1; }
        (void)hipEventDestroy(r.t0); (void)hipEventDestroy(r.t1);
    }
    g_prof.clear();
    return rc;
}

extern "C" const char* gsr_version(void) { return "gsraster 0.4 (gfx950)"; }
extern "C" int gsr_abi_version(void) { return GSR_ABI_VERSION; }
extern "C" const char* gsr_last_error(void) { return g_err; }

extern "C" int gsr_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return gsr_fail(GSR_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

extern "C" size_t gsr_geom_bytes(int P) { return gsr_carve_geom(nullptr, P).bytes; }
extern "C" size_t gsr_image_bytes(int P, int W, int H) { return gsr_carve_image(nullptr, P, W, H).bytes; }
extern "C" size_t gsr_binning_bytes(int R) { return gsr_carve_binning(nullptr, R).bytes; }
extern "C" size_t gsr_backward_scratch_bytes(int P, int num_slots) { return gsr_carve_backward_scratch(nullptr, P, num_slots).bytes; }

extern "C" int gsr_workspace_layout(int which, int P, int W, int H, int R, gsr_layout_piece* out_host, int capacity)
{
    if (capacity < 0 || (capacity > 0 && !out_host)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "out_host is NULL or the capacity negative (%d)", capacity);
    GsrCarveRecord record = { out_host, capacity, 0 };
    switch (which) {
    case GSR_LAYOUT_GEOM: gsr_carve_geom(nullptr, P, &record); break;
    case GSR_LAYOUT_IMAGE: gsr_carve_image(nullptr, P, W, H, &record); break;
    case GSR_LAYOUT_BINNING: gsr_carve_binning(nullptr, R, &record); break;
    case GSR_LAYOUT_BACKWARD_SCRATCH: gsr_carve_backward_scratch(nullptr, P, R, &record); break;
    default: return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "unknown workspace %d (GSR_LAYOUT_*)", which);
    }
    return record.count;
}
extern "C" int gsr_layout_constant(int which)
{
    switch (which) {
    case GSR_CONSTANT_SEG1: return GSR_SEG1;
    case GSR_CONSTANT_SEG2: return GSR_SEG2;
    case GSR_CONSTANT_SEG_MAX: return GSR_SEG_MAX;
    case GSR_CONSTANT_XCD_CHUNK: return GSR_XCD_CHUNK;
    }
    return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "unknown constant %d (GSR_CONSTANT_*)", which);
}
extern "C" int gsr_layout_ckpt_pos(int k, int L) { return gsr_ckpt_pos(k, L); }
extern "C" int gsr_layout_num_chunks(int P) { return gsr_num_chunks(P); }
extern "C" int gsr_layout_xcd_tiles(int T) { return gsr_xcd_tiles(T); }
extern "C" int gsr_layout_xcd_tile(int xcd, int i, int T) { return gsr_xcd_tile(xcd, i, T); }

static bool gsr_partial_sort(const gsr_tuning* tuning) { return !(tuning && tuning->disable_partial_sort); }
static bool gsr_inference(const gsr_tuning* tuning) { return tuning && tuning->inference; }
static int gsr_forced_bands(const gsr_tuning* tuning) { return tuning ? tuning->scatter_bands : 0; }
// per-view walk depths of the forward blend (gsraster.h): the caller's array + whether it already holds a previous visit's
struct GsrWalkHint { uint32_t* depths; bool valid; };
static GsrWalkHint gsr_walk_hint(const gsr_tuning* tuning)
{
    GsrWalkHint h = { nullptr, false };
    if (tuning && tuning->walk_depths) { h.depths = reinterpret_cast<uint32_t*>((uintptr_t)tuning->walk_depths); h.valid = tuning->walk_depths_valid != 0; }
    return h;
}
// the occlusion cut-off works on the tile-cull masks and keeps its table in LDS beside the histogram
static bool gsr_occlusion(const gsr_tuning* tuning, int T)
{
    return tuning && tuning->occlusion_cut && !tuning->disable_tile_cull && T <= GSR_OCC_MAX_TILES;
}

static GsrCam gsr_make_cam(int W, int H, const float* view_d, const float* proj_d, const float* campos_d, float tan_fovx,
                           float tan_fovy, float scale_modifier)
{
    GsrCam cam;
    cam.view = view_d; cam.proj = proj_d; cam.campos = campos_d;
    cam.tan_fovx = tan_fovx; cam.tan_fovy = tan_fovy;
    cam.focal_y = H / (2.0f * tan_fovy);  // DGR rasterizer_impl.cu:226-227
    cam.focal_x = W / (2.0f * tan_fovx);
    cam.scale_modifier = scale_modifier;
    cam.W = W; cam.H = H;
    const GsrGrid grid = gsr_tile_grid(W, H);
    cam.gx = grid.gx; cam.gy = grid.gy;
    return cam;
}

static int gsr_check_dims(int P, int W, int H)
{
    if (P < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "P must be >= 0 (got %d)", P);
    if (W <= 0 || H <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image size must be positive (got %dx%d)", W, H);
    const GsrGrid grid = gsr_tile_grid(W, H);
    const long gx = grid.gx, gy = grid.gy;
    if (gx > 65535 || gy > 65535) return gsr_fail(GSR_ERR_UNSUPPORTED, "image too large: %ldx%ld tiles", gx, gy);
    // more than GSR_MAX_TILES_LDS tiles: supported through the global-counter binning fallback (binning.hip)
    if (gx * gy > (1L << 24)) return gsr_fail(GSR_ERR_UNSUPPORTED, "image too large: %ld tiles", gx * gy);
    // (no accepted size wraps a carve, GsrCarver::ok(): at most 2^24 tiles = 2^32 pixels of 648 checkpoint bytes, P and R below 2^31 of 64 B)
    return GSR_OK;
}

// The frame of one entry point: the only place (besides the *_bytes queries) that carves the caller's workspaces.  Pointers are not
// checked here -- carving a NULL workspace yields pointers nobody follows, the entry points report it -- and an entry point without
// a binning workspace (stage 1) leaves `bin` / `capacity` unset.
static GsrFrame gsr_make_frame(int P, int W, int H, const void* geom_ws, const void* image_ws, const void* binning_ws, int capacity,
                               int debug, hipStream_t stream)
{
    GsrFrame f{};
    const GsrGrid grid = gsr_tile_grid(W, H);
    f.P = P; f.W = W; f.H = H;
    f.gx = grid.gx; f.gy = grid.gy; f.T = grid.gx * grid.gy;
    f.geom = gsr_carve_geom(const_cast<void*>(geom_ws), P);
    f.image = gsr_carve_image(const_cast<void*>(image_ws), P, W, H);
    if (binning_ws) { f.bin = gsr_carve_binning(const_cast<void*>(binning_ws), capacity); f.capacity = capacity; }
    f.stream = stream; f.debug = debug;
    return f;
}

// Per host thread and device: the pinned, device-mapped words the tile-scan kernel writes {R, longest list} into (valid
// to read after the stream / event the caller waits on) and the event that marks "R is on the host".  A thread that
// alternates between devices finds each device's pair again (nothing is re-allocated on a switch); the pairs live as
// long as the thread and are released when it exits.
#define GSR_MAX_DEVICES 64
struct GsrDeviceState {
    volatile uint32_t* host = nullptr;  // the pinned block (16 words, indices below) ...
    uint32_t* dev = nullptr;            // ... and its address on the device
    hipEvent_t ev = nullptr;            // created by the first gsr_forward
    uint8_t heavy_mode = 0;   // per-Gaussian backward: 1 = launch the heavy-group kernel (gsr_heavy_groups_expected)
    uint8_t heavy_probe = 0;  // backwards to wait before the heavy kernel is launched again just to count the groups
    // partial sort of long tile lists, the bet and its feedback (gsr_partial_bet)
    uint32_t fwd_serial = 0;   // forwards of this thread on the device (what a resumed quadrant reports back)
    uint32_t ranoff_seen = 0;  // the last report acted upon
    uint8_t bet_hold = 0;      // forwards left during which lists up to GSR_SORT_CAP_SMALL are sorted completely at once
};
struct GsrThreadDevices {
    GsrDeviceState of[GSR_MAX_DEVICES];
    ~GsrThreadDevices()
    {
        for (int d = 0; d < GSR_MAX_DEVICES; d++) {
            // kernels of this thread's last calls may still store into the block (the heavy-group hint is written without a
            // host wait): drain the owning device before the block goes away
            if (of[d].host && hipSetDevice(d) == hipSuccess) (void)hipDeviceSynchronize();
            if (of[d].host) (void)hipHostFree(const_cast<uint32_t*>(of[d].host));
            if (of[d].ev) (void)hipEventDestroy(of[d].ev);
        }
    }
};
static thread_local GsrThreadDevices g_tds;

// words of the pinned, device-mapped block (one per host thread and device): 0, 1 = {R, longest list} of stage 1, 4 = prefiltered
// trap, 8 = the per-Gaussian backward's report on heavy groups (0 = nothing new, 1 = the one-wave kernel met one, 2 + n = the
// heavy kernel was given n)
#define GSR_PINNED_HEAVY_SEEN 8
// 9 = the forward's fix-up pass: serial number of the last forward in which a quadrant ran off its tile's partially sorted prefix
#define GSR_PINNED_RANOFF 9
#define GSR_BET_HOLD 64  // forwards without the partial sort after a lost bet, then one forward probes again
#define GSR_HEAVY_MIN_GROUPS 192  // fewer heavy groups than this: the one-wave kernel does them itself (gauss_bwd.hip, launcher)

// This thread's state on the current device; its pinned block is allocated at the first call.
static int gsr_device_state(GsrDeviceState** state)
{
    int d = 0;
    GSR_HIP(hipGetDevice(&d), "hipGetDevice");
    if (d < 0 || d >= GSR_MAX_DEVICES) return gsr_fail(GSR_ERR_UNSUPPORTED, "device index %d out of range", d);
    GsrDeviceState& s = g_tds.of[d];
    if (!s.host) {
        void* p = nullptr;
        GSR_HIP(hipHostMalloc(&p, 64, hipHostMallocMapped), "hipHostMalloc(info)");
        void* pd = nullptr;
        GSR_HIP(hipHostGetDevicePointer(&pd, p, 0), "hipHostGetDevicePointer(info)");
        memset(p, 0, 64);
        s.host = (uint32_t*)p; s.dev = (uint32_t*)pd;
    }
    *state = &s;
    return GSR_OK;
}

// The state machine behind `heavy_expected` (see gsr_backward): report = the pinned word, mode / probe = the thread's state.
static bool gsr_heavy_groups_expected(uint32_t report, uint8_t* mode, uint8_t* probe)
{
    if (report >= 2u) {  // counted by the heavy kernel
        *mode = (report - 2u) >= GSR_HEAVY_MIN_GROUPS;
        *probe = (report - 2u) > 0u ? 64 : 0;  // none at all: the next sighting is counted at once
    } else if (report == 1u && !*mode) {  // met by the one-wave kernel while it was doing them itself
        if (*probe > 0) --*probe;
        else *mode = 1;
    }  // 0, or 1 in heavy mode (the heavy kernel of that call has not reported yet): nothing new
    return *mode != 0;
}

// Partial sort of long lists -- the bet and its feedback (round 6).  Lists beyond GSR_NEAR_CAP are depth-sorted only as far as the blend is
// expected to walk (binning.hip); a tile whose pixels are still blending at the end of that prefix is sorted completely and its
// quadrants resume in a SECOND forward-blend launch.  On frames that saturate the bet wins (large splats: tile sort 133 instead of
// 239 us).  On the frames of an initialised, untrained scene it loses on every long list -- nothing saturates -- and the second launch is
// ~140 us of a mostly idle GPU (init-state frame: 18 tiles of 2 049 - 3 238 entries, forward 2 x 169 us).  Which kind of frame a
// scene produces is a property of its training state, not of the view: a resumed quadrant stores the forward's serial number in a
// host-mapped word, and after such a report the next GSR_BET_HOLD forwards of this thread on this device sort lists that fit the
// small LDS class (<= GSR_SORT_CAP_SMALL entries) completely at once -- one launch, no fix-up -- then one forward bets again.  Longer
// lists always bet: a complete sort of 10 000-entry lists costs more than the fix-up.  Results never depend on any of this (the
// partial sort is bit-identical to a complete one, tests + tools/fuzz_parity.py).  -> the partial sort is worth betting on
static bool gsr_partial_bet(GsrDeviceState& s, int longest, bool longest_is_a_provision)
{
    const uint32_t rep = s.host[GSR_PINNED_RANOFF];
    if (rep != s.ranoff_seen) { s.ranoff_seen = rep; s.bet_hold = GSR_BET_HOLD; }
    const bool hold = s.bet_hold > 0;
    if (hold) --s.bet_hold;
    // (a speculative caller provisions the longest list with slack over what its last frames had -- gsraster.h: 1.25 x: the call then
    // sorts completely up to GSR_SORT_CAP_SMALL and treats anything longer like any list beyond its provision: GSR_NEED_CAPACITY)
    const int limit = longest_is_a_provision ? GSR_SORT_CAP_SMALL + GSR_SORT_CAP_SMALL / 4 + 64 : GSR_SORT_CAP_SMALL;
    return !(hold && longest > GSR_NEAR_CAP && longest <= limit);
}

// One more forward of this thread on the current device that may sort partially: does it bet (gsr_partial_bet)?
static int gsr_count_forward_and_bet(int longest, bool longest_is_a_provision, bool* bet)
{
    GsrDeviceState* s = nullptr;
    const int rc = gsr_device_state(&s);
    if (rc) return rc;
    ++s->fwd_serial;
    *bet = gsr_partial_bet(*s, longest, longest_is_a_provision);
    return GSR_OK;
}

extern "C" void gsr_adaptive_reset(void)
{
    // forget what this thread's previous calls taught the launch heuristics (tests, gscream_amd.set_tuning): reports that are
    // still on their way count as seen
    for (GsrDeviceState& s : g_tds.of) {
        s.bet_hold = 0;
        if (s.host) s.ranoff_seen = s.host[GSR_PINNED_RANOFF];
    }
}

// `prefiltered` (GaussianRasterizationSettings field 11).  The reference uses it for one thing: a point that fails the near
// plane although the caller declared the cloud pre-filtered prints "Point is filtered although prefiltered is set" and
// traps the kernel (DGR auxiliary.h:154-162) -- the process then dies at its next synchronisation.  Here the same
// condition is an ordinary error of the call, checked in debug mode (`debug=True` synchronises after every stage anyway);
// without debug the flag costs nothing and culled points are simply culled.  (Missing pointers are left to the argument
// checks that follow in the forward entry points.)
static int gsr_prefiltered_trap(int P, int prefiltered, int debug, const float* means3D, const float* viewmatrix, hipStream_t stream)
{
    if (!prefiltered || !debug || P <= 0 || !means3D || !viewmatrix) return GSR_OK;
    GsrDeviceState* s = nullptr;
    int rc = gsr_device_state(&s);
    if (rc) return rc;
    GSR_HIP(hipStreamSynchronize(stream), "prefiltered check");  // nothing in flight may still write the info words
    s->host[4] = 0u;
    GSR_HIP(gsr_launch_prefiltered_check(P, means3D, viewmatrix, s->dev + 4, stream), "prefiltered check");
    GSR_HIP(hipStreamSynchronize(stream), "prefiltered check");
    const uint32_t n = s->host[4];
    if (n) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "Point is filtered although prefiltered is set. This shouldn't happen! "
                                                    "(%u of %d points have view-space z <= 0.2)", n, P);
    return GSR_OK;
}

// The opening gsr_forward and gsr_forward_stage1 share.  *empty: there is nothing to render, the call is over (result zeroed).
static int gsr_open_forward(int P, int W, int H, int prefiltered, int debug, const float* means3D, const float* viewmatrix,
                            gsr_stage1_result* result_host, hipStream_t stream, bool* empty)
{
    *empty = true;
    const int rc = gsr_check_dims(P, W, H);
    if (rc) return rc;
    if (!result_host) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "result_host is NULL");
    memset(result_host, 0, sizeof(*result_host));
    if (P == 0) return GSR_OK;  // DGR rasterize_points.cu:85
    *empty = false;
    return gsr_prefiltered_trap(P, prefiltered, debug, means3D, viewmatrix, stream);
}

// Validates the stage-1 arguments and enqueues preprocess + counting; *state: where the scan kernel's {R, longest list} arrive.
static int gsr_enqueue_stage1(const GsrFrame& f, int D, int M, const float* means3D, const float* scales,
                              float scale_modifier, const float* rotations, const float* opacities,
                              const float* features, const float* shs, const float* cov3D_precomp,
                              const float* colors_precomp, const float* viewmatrix, const float* projmatrix,
                              const float* campos, float tan_fovx, float tan_fovy, int32_t* radii, GsrDeviceState** state,
                              bool defer_tile_scan, const gsr_tuning* tuning,
                              bool* ordered /* out (or NULL): the forward blend's dispatch order was computed beside the column scan
                              (gsr_tuning.walk_depths) */)
{
    // (geom.rec and image.ranges are the first things carved: the workspace pointers themselves)
    if (!means3D || !opacities || !features || !viewmatrix || !projmatrix || !f.geom.rec || !f.image.ranges || !radii)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "a required pointer is NULL");
    if ((!scales || !rotations) == (cov3D_precomp == nullptr))  // DGR __init__.py:227-228
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "provide exactly one of scales+rotations or cov3D_precomp");
    if ((shs == nullptr) == (colors_precomp == nullptr))  // DGR __init__.py:224-225
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "provide exactly one of shs or colors_precomp");
    if (shs && (!campos || M <= 0)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "SH colours need campos and M > 0");
    const GsrCam cam = gsr_make_cam(f.W, f.H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, scale_modifier);
    const bool occlusion = gsr_occlusion(tuning, f.T);
    if (occlusion) GSR_HIP(hipMemsetAsync(f.image.occ_mass, 0, (size_t)GSR_OCC_COPIES * f.T * GSR_OCC_BUCKETS * sizeof(uint32_t), f.stream), "clear occlusion masses");
    GSR_STAGE(GSR_STAGE_PREPROCESS, f.stream, f.debug,
              gsr_launch_preprocess(0, f.P, D, M, cam, means3D, scales, rotations, opacities, features, shs, cov3D_precomp, colors_precomp,
                                    &f.geom, radii, nullptr, nullptr, !(tuning && tuning->disable_tile_cull),
                                    occlusion ? f.image.occ_mass : nullptr, f.stream),
              "preprocess");
    // {R, longest list} reach the host through a pinned, device-mapped word pair the scan kernel stores into (one per
    // host thread and device, 8 bytes, kept for the life of the thread): no copy kernel between the scan and the scatter.
    const int rc = gsr_device_state(state);
    if (rc) return rc;
    const GsrWalkHint walk = gsr_walk_hint(tuning);
    GSR_STAGE(GSR_STAGE_COUNT_SCAN, f.stream, f.debug,
              gsr_launch_count(f, (*state)->dev, defer_tile_scan, occlusion, (ordered && walk.valid) ? walk.depths : nullptr, ordered),
              "tile count / scans");
    return GSR_OK;
}

static int gsr_publish_stage1(const volatile uint32_t* info, gsr_stage1_result* out)
{
    const uint32_t got[3] = { info[0], info[1], info[2] };
    if (got[0] > 0x7fffffffu) return gsr_fail(GSR_ERR_UNSUPPORTED, "instance count %u overflows int32", got[0]);
    out->num_rendered = (int32_t)got[0];
    out->max_tile_count = (int32_t)got[1];
    out->num_slots = (int32_t)got[0];  // one gradient slot per binned instance
    out->num_occluded = (int32_t)got[2];
    return GSR_OK;
}

extern "C" int gsr_forward_stage1(int P, int D, int M, int W, int H, const float* means3D, const float* scales,
                                  float scale_modifier, const float* rotations, const float* opacities,
                                  const float* features, const float* shs, const float* cov3D_precomp,
                                  const float* colors_precomp, const float* viewmatrix, const float* projmatrix,
                                  const float* campos, float tan_fovx, float tan_fovy, int prefiltered, void* geom_ws,
                                  void* image_ws, int32_t* radii, gsr_stage1_result* result_host,
                                  const gsr_tuning* tuning, int debug, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    bool empty = false;
    int rc = gsr_open_forward(P, W, H, prefiltered, debug, means3D, viewmatrix, result_host, stream, &empty);
    if (rc || empty) return rc;
    const GsrFrame f = gsr_make_frame(P, W, H, geom_ws, image_ws, nullptr, 0, debug, stream);
    GsrDeviceState* state = nullptr;
    rc = gsr_enqueue_stage1(f, D, M, means3D, scales, scale_modifier, rotations, opacities, features, shs, cov3D_precomp,
                            colors_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, &state, false, tuning, nullptr);
    if (rc) return rc;
    GSR_HIP(hipStreamSynchronize(stream), "read num_rendered");
    return gsr_publish_stage1(state->host, result_host);
}

// After a forward over partially sorted lists (binning.hip): tiles whose pixels were still blending at the end of their
// sorted prefix get a full sort and are blended again.  Nothing happens on the GPU beyond a few empty launches when no
// tile asked for it; not enqueued at all when no list was long enough to be partially sorted.
static int gsr_enqueue_fixup(const GsrFrame& f, int max_tile_count, const GsrTargets& to, bool inference, GsrWalkHint walk)
{
    if (max_tile_count <= GSR_NEAR_CAP) return GSR_OK;
    GsrDeviceState* s = nullptr;
    const int rc = gsr_device_state(&s);
    if (rc) return rc;
    GSR_STAGE(GSR_STAGE_TILE_SORT, f.stream, f.debug, gsr_launch_sort_fixup(f, max_tile_count, inference), "tile sort (fix-up)");
    GsrBlendPass pass{};
    pass.only_flagged = true;
    pass.inference = inference;
    pass.walk_depths = walk.depths;
    pass.walk_depths_valid = walk.valid;
    pass.ranoff_report = s->dev + GSR_PINNED_RANOFF;  // where a resumed quadrant reports the lost bet (gsr_partial_bet)
    pass.serial = s->fwd_serial;
    GSR_STAGE(GSR_STAGE_BLEND_FWD, f.stream, f.debug,
              gsr_launch_blend_forward(f, to, max_tile_count, pass), "forward blend (fix-up)");
    return GSR_OK;
}

// Stage 2 -- scatter, tile sort, forward blend -- in its two forms, told apart by `scattered`:
//   exact (gsr_forward_stage2, `scattered` NULL): R and the longest list are known; `longest` is the longest list.
//   speculative (gsr_forward, `scattered` = the thread's event): enqueued BEFORE the host waits for R, so the GPU never idles on
//     the host round trip the reference pays at rasterizer_impl.cu:287; `longest` is the caller's hint (-1: none), which chooses
//     the sort variants -- with partial sorting it only sizes the LDS of the lists up to GSR_NEAR_CAP.  The event is recorded
//     behind the scatter, whose kernel stores {R, longest list} (scatter.fused_tile_scan; beyond the LDS tile limit stage 1 ran
//     the stand-alone tile scan: the same words, written earlier).
static int gsr_enqueue_stage2(const GsrFrame& f, hipEvent_t scattered, int longest, int sort_mode /* gsr_launch_tile_sort */,
                              const GsrScatterPass& scatter, bool ordered, GsrWalkHint walk, const GsrTargets& to)
{
    const bool speculative = scattered != nullptr;
    // info[3] (quadrant walks that entered the second depth tier) is zeroed by the tile scan of stage 1 and counted up by the forward
    // blend: a stage 2 that REPEATS a speculative forward (GSR_NEED_CAPACITY) would count those walks twice and could flip the
    // backward's launch order on exactly the frames that outgrew their hint (results never depended on it)
    if (!speculative) GSR_HIP(hipMemsetAsync(f.image.info + 3, 0, sizeof(uint32_t), f.stream), "reset the deep-walk counter");
    GSR_STAGE(GSR_STAGE_SCATTER, f.stream, f.debug, gsr_launch_scatter(f, scatter), "scatter");
    if (speculative) GSR_HIP(hipEventRecord(scattered, f.stream), "record");
    // sort mode 1: lists beyond GSR_NEAR_CAP take the fixed-LDS prefix sort whatever `longest` says
    GSR_STAGE(GSR_STAGE_TILE_SORT, f.stream, f.debug, gsr_launch_tile_sort(f, longest, sort_mode, speculative, scatter.inference), "tile sort");
    GsrBlendPass pass{};
    pass.inference = scatter.inference;
    pass.walk_depths = walk.depths;
    pass.walk_depths_valid = walk.valid;
    pass.already_ordered = ordered;
    GSR_STAGE(GSR_STAGE_BLEND_FWD, f.stream, f.debug,
              gsr_launch_blend_forward(f, to, longest, pass), "forward blend");
    // longest list known (exact form): the fix-up can follow at once; the speculative form enqueues it after the read-back
    if (!speculative && sort_mode == 1 && longest >= 0) return gsr_enqueue_fixup(f, longest, to, scatter.inference, walk);
    return GSR_OK;
}

extern "C" int gsr_forward(int P, int D, int M, int W, int H, const float* means3D, const float* scales,
                           float scale_modifier, const float* rotations, const float* opacities, const float* features,
                           const float* shs, const float* cov3D_precomp, const float* colors_precomp,
                           const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                           float tan_fovy, int prefiltered, const float* background, void* geom_ws, void* image_ws,
                           void* binning_ws, int binning_capacity, int max_tile_count_hint, int32_t* radii,
                           float* out_color, float* out_depth, float* out_feature, gsr_stage1_result* result_host,
                           const gsr_tuning* tuning, int debug, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    bool empty = false;
    int rc = gsr_open_forward(P, W, H, prefiltered, debug, means3D, viewmatrix, result_host, stream, &empty);
    if (rc || empty) return rc;
    if (!background || !binning_ws || !out_color || !out_depth || !out_feature || binning_capacity <= 0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "a required pointer is NULL or the binning capacity is not positive");
    const GsrFrame f = gsr_make_frame(P, W, H, geom_ws, image_ws, binning_ws, binning_capacity, debug, stream);
    const GsrTargets to = { background, out_color, out_depth, out_feature };
    // The tile scan (ranges, R, longest list) is folded into the scatter kernel here: nobody needs R before stage 2 is
    // enqueued, and the one-block launch cost as much as the whole column scan.  The event therefore follows the scatter.
    GsrDeviceState* state = nullptr;
    bool ordered = false;
    rc = gsr_enqueue_stage1(f, D, M, means3D, scales, scale_modifier, rotations, opacities, features, shs, cov3D_precomp,
                            colors_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, radii, &state, true, tuning, &ordered);
    if (rc) return rc;
    // One event per thread and device marks "R is on the host" (created at the thread's first forward on the device)
    if (!state->ev) GSR_HIP(hipEventCreateWithFlags(&state->ev, hipEventDisableTiming), "hipEventCreate");
    bool partial = gsr_partial_sort(tuning);
    int sort_mode = partial ? 1 : 0;
    if (partial) {  // ... unless this thread's recent forwards lost the bet on lists like these (gsr_partial_bet)
        rc = gsr_count_forward_and_bet(max_tile_count_hint, true, &partial);
        if (rc) return rc;
        if (!partial) {  // complete sorts, the few long lists in a launch of their own, nothing beyond the small LDS class
            sort_mode = 2;
            if (max_tile_count_hint > GSR_SORT_CAP_SMALL) max_tile_count_hint = GSR_SORT_CAP_SMALL;
        }
    }
    const bool inference = gsr_inference(tuning);
    const GsrWalkHint walk = gsr_walk_hint(tuning);
    GsrScatterPass scatter{};
    // the caller provisions the workspace with slack over what it expects (gsraster.h: "e.g. 1.25 x the previous frame's
    // num_rendered"): the scatter's staging (and its bands, binning.hip) is sized for the expectation, not for the provision
    scatter.expected_instances = (int)(0.8 * (double)binning_capacity);
    scatter.forced_bands = gsr_forced_bands(tuning);
    scatter.fused_tile_scan = true;
    scatter.fused_info_host = state->dev;
    scatter.inference = inference;
    scatter.occlusion_cut = gsr_occlusion(tuning, f.T);
    rc = gsr_enqueue_stage2(f, state->ev, max_tile_count_hint > 0 ? max_tile_count_hint : -1, sort_mode, scatter, ordered, walk, to);
    if (rc) return rc;
    GSR_HIP(hipEventSynchronize(state->ev), "read num_rendered");
    rc = gsr_publish_stage1(state->host, result_host);
    if (rc) return rc;
    // the guesses hold iff every list fitted the workspace AND the sort variants that were launched cover the longest list
    const bool ok = result_host->num_rendered <= binning_capacity &&
                    (max_tile_count_hint <= 0 || result_host->max_tile_count <= max_tile_count_hint ||
                     (partial && max_tile_count_hint > GSR_NEAR_CAP));  // lists beyond the cap do not depend on the hint
    // (strictly greater: gsr_launch_tile_sort starts the prefix-sort kernel only for a provision > GSR_NEAR_CAP)
    if (!ok) return GSR_NEED_CAPACITY;
    if (partial) return gsr_enqueue_fixup(f, result_host->max_tile_count, to, inference, walk);
    return GSR_OK;
}

extern "C" int gsr_forward_stage2(int P, int W, int H, int R, int max_tile_count, const float* background,
                                  void* geom_ws, void* image_ws, void* binning_ws, float* out_color, float* out_depth,
                                  float* out_feature, const gsr_tuning* tuning, int debug, void* stream_)
{
    int rc = gsr_check_dims(P, W, H);
    if (rc) return rc;
    if (P == 0) return GSR_OK;  // outputs keep the caller's zero fill, like DGR rasterize_points.cu:69-85
    if (!background || !geom_ws || !image_ws || !binning_ws || !out_color || !out_depth || !out_feature)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "a required pointer is NULL");
    if (R < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "R must be >= 0");
    int sort_mode = 0;
    if (gsr_partial_sort(tuning)) {  // (gsr_partial_bet: not when this thread's recent forwards lost the bet on lists like these)
        bool bet = false;
        rc = gsr_count_forward_and_bet(max_tile_count, false, &bet);
        if (rc) return rc;
        sort_mode = bet ? 1 : 2;
    }
    const GsrFrame f = gsr_make_frame(P, W, H, geom_ws, image_ws, binning_ws, R, debug, (hipStream_t)stream_);
    GsrScatterPass scatter{};
    scatter.expected_instances = R;
    scatter.forced_bands = gsr_forced_bands(tuning);
    scatter.inference = gsr_inference(tuning);
    return gsr_enqueue_stage2(f, nullptr, max_tile_count, sort_mode, scatter, false, gsr_walk_hint(tuning),
                              GsrTargets{ background, out_color, out_depth, out_feature });
}

extern "C" int gsr_backward(int P, int D, int M, int W, int H, int R, int binning_capacity, int max_tile_count, const float* background,
                            const float* means3D,
                            const int32_t* radii, const float* colors_precomp, const float* shs, const float* scales,
                            float scale_modifier, const float* rotations, const float* cov3D_precomp,
                            const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                            float tan_fovy, const float* dL_dout_color, const float* dL_dout_depth,
                            const float* dL_dout_feature, const void* geom_ws, void* image_ws,
                            void* binning_ws, void* scratch, float* dL_dmeans2D, float* dL_dcolors,
                            float* dL_dopacity, float* dL_dfeatures, float* dL_dmeans3D, float* dL_dcov3D,
                            float* dL_dsh, float* dL_dscales, float* dL_drotations, const gsr_tuning* tuning, int debug,
                            void* stream_)
{
    (void)colors_precomp;  // colours live in the geometry records written by the forward
    hipStream_t stream = (hipStream_t)stream_;
    int rc = gsr_check_dims(P, W, H);
    if (rc) return rc;
    if (P == 0) return GSR_OK;  // DGR rasterize_points.cu:172
    if (!background || !means3D || !radii || !viewmatrix || !projmatrix || !dL_dout_color || !geom_ws || !image_ws || !binning_ws || !scratch || !dL_dmeans2D || !dL_dcolors ||
        !dL_dopacity || !dL_dfeatures || !dL_dmeans3D)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "a required pointer is NULL");
    if ((!scales || !rotations) == (cov3D_precomp == nullptr))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "provide exactly one of scales+rotations or cov3D_precomp");
    if (!cov3D_precomp && (!dL_dscales || !dL_drotations))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "dL_dscales / dL_drotations are required with scales+rotations");
    if (shs && (!dL_dsh || !campos || M <= 0))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "SH colours need dL_dsh, campos and M > 0");
    if (R < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "R must be >= 0");
    if (binning_capacity < R) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "binning_capacity < R");

    const GsrCam cam = gsr_make_cam(W, H, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy, scale_modifier);
    const GsrFrame f = gsr_make_frame(P, W, H, geom_ws, image_ws, binning_ws, binning_capacity, debug, stream);
    const GsrBackwardScratch sc = gsr_carve_backward_scratch(scratch, P, R);
    float* slots = sc.slots;
    uint32_t* heavy = sc.heavy;
    // written-slot flags: cleared by the forward's tile sort, set by the backward blend; the set of written slots is a function
    // of the forward state alone, so a second backward over the same forward state finds exactly the flags it would set
    uint8_t* slot_written = f.bin.slot_written;
    if (R > 0)
        GSR_STAGE(GSR_STAGE_BLEND_BWD, stream, debug,
                  gsr_launch_blend_backward(f, background, dL_dout_color, dL_dout_depth, dL_dout_feature, slots, slot_written, heavy,
                                            max_tile_count > 0 ? max_tile_count : -1),
                  "backward blend");
    else
        GSR_HIP(hipMemsetAsync(heavy, 0, 2 * sizeof(uint32_t), stream), "heavy-group counters");
    // Is the heavy-group kernel worth its launch?  Decided from what this thread's previous backwards (on this device) reported
    // through one word of the pinned block, read and cleared here without waiting for anything -- a hint only: both ways give the
    // same bits.  The heavy kernel reports how many groups it was given; below GSR_HEAVY_MIN_GROUPS the next calls go without it
    // (then only "met one" is known, so every 64th call launches it again to count).
    GsrDeviceState* state = nullptr;
    rc = gsr_device_state(&state);
    if (rc) return rc;
    bool heavy_expected = gsr_heavy_groups_expected(state->host[GSR_PINNED_HEAVY_SEEN], &state->heavy_mode, &state->heavy_probe);
    if (tuning && tuning->heavy_groups) heavy_expected = tuning->heavy_groups == 1;
    state->host[GSR_PINNED_HEAVY_SEEN] = 0u;
    GSR_STAGE(GSR_STAGE_GAUSS_BWD, stream, debug,
              gsr_launch_gauss_backward(P, D, M, cam, means3D, radii, shs, scales, rotations, cov3D_precomp, f.geom, slots, slot_written, heavy,
                                        state->dev + GSR_PINNED_HEAVY_SEEN, heavy_expected, R,
                                        dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dfeatures, dL_dmeans3D, dL_dcov3D,
                                        dL_dsh, dL_dscales, dL_drotations, stream),
              "per-Gaussian backward");
    return GSR_OK;
}

extern "C" int gsr_filter(int P, int W, int H, const float* means3D, const float* scales, float scale_modifier,
                          const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                          const float* projmatrix, float tan_fovx, float tan_fovy, int prefiltered, int32_t* radii,
                          float* px, float* py, int debug, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0 || W <= 0 || H <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "bad sizes P=%d W=%d H=%d", P, W, H);
    if (P == 0) return GSR_OK;
    if (!means3D || !viewmatrix || !projmatrix || !radii) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "a required pointer is NULL");
    const int rc = gsr_prefiltered_trap(P, prefiltered, debug, means3D, viewmatrix, stream);
    if (rc) return rc;
    if ((!scales || !rotations) == (cov3D_precomp == nullptr))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "provide exactly one of scales+rotations or cov3D_precomp");
    if ((px == nullptr) != (py == nullptr)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "px and py go together");
    const GsrCam cam = gsr_make_cam(W, H, viewmatrix, projmatrix, nullptr, tan_fovx, tan_fovy, scale_modifier);
    GSR_STAGE(GSR_STAGE_PREPROCESS, stream, debug,
              gsr_launch_preprocess(px ? 2 : 1, P, 0, 0, cam, means3D, scales, rotations, nullptr, nullptr, nullptr,
                                    cov3D_precomp, nullptr, nullptr, radii, px, py, 0, nullptr, stream),
              "filter preprocess");
    return GSR_OK;
}

extern "C" int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                                uint8_t* present, void* stream_)
{
    (void)projmatrix;  // unused by the reference's test as well (auxiliary.h:154 checks view-space z only)
    hipStream_t stream = (hipStream_t)stream_;
    if (P < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "P must be >= 0");
    if (P == 0) return GSR_OK;
    if (!means3D || !viewmatrix || !present) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "a required pointer is NULL");
    GSR_HIP(gsr_launch_mark_visible(P, means3D, viewmatrix, present, stream), "mark_visible");
    return GSR_OK;
}
