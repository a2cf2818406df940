// api.hip -- the extern "C" surface declared in include/gsraster.h (host code only).
//
// Each entry validates its arguments, carves the caller-allocated workspaces, enqueues the stage
// kernels on the caller's stream and reports failures as an int code + thread-local message.
// Orchestration replaces CudaRasterizer::Rasterizer::{forward,backward,visible_filter,
// position2D_filter,markVisible} (DGR rasterizer_impl.cu:141-153,199-347,350-530,536-643).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include "gsr_common.h"

static thread_local char g_err[512] = "";

static int gsr_fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define GSR_HIP(expr, what)                                                                                     \
    do {                                                                                                        \
        hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) return gsr_fail(GSR_ERR_HIP, "%s: %s (%s)", what, hipGetErrorString(e_), #expr); \
    } while (0)

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

// ---- image-space RGB loss (loss.hip) ----
extern "C" size_t gsr_loss_workspace_bytes(int C, int H, int W) { return gsl_workspace_bytes(C, H, W); }

static int gsr_check_loss_args(int C, int H, int W, const float* img, const float* gt, const void* workspace)
{
    if (C < 1 || H < 1 || W < 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "loss: C, H, W must be >= 1 (got %d, %d, %d)", C, H, W);
    if ((long long)C * H * W > 0x7fffffffLL) return gsr_fail(GSR_ERR_UNSUPPORTED, "loss: image too large");
    // (no accepted size wraps the carve: three planes of C*H*W floats, below 2^35 bytes)
    if (!img || !gt || !workspace) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "loss: a required pointer is NULL");
    return GSR_OK;
}

static int gsr_check_window(int window_size)
{
    if (window_size < 1 || window_size > 11 || (window_size & 1) == 0)
        return gsr_fail(GSR_ERR_UNSUPPORTED, "loss: window_size must be odd and in 1..11 (got %d)", window_size);
    return GSR_OK;
}

extern "C" int gsr_rgb_loss_forward_window(int C, int H, int W, const float* img, const float* gt, const float* weight,
                                           float a_l1, float a_ssim, int window_size, void* workspace, float* out3, int keep_state,
                                           void* stream)
{
    int rc = gsr_check_loss_args(C, H, W, img, gt, workspace);
    if (rc) return rc;
    rc = gsr_check_window(window_size);
    if (rc) return rc;
    if (!out3) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "loss: out3 is NULL");
    GSR_HIP(gsl_launch_forward(C, H, W, img, gt, weight, a_l1, a_ssim, workspace, out3, keep_state, window_size, (hipStream_t)stream),
            "rgb loss forward");
    return GSR_OK;
}

extern "C" int gsr_rgb_loss_backward_window(int C, int H, int W, const float* img, const float* gt, const float* weight,
                                            float a_l1, float a_ssim, int window_size, const void* workspace,
                                            const float* upstream, float* dL_dimg, void* stream)
{
    int rc = gsr_check_loss_args(C, H, W, img, gt, workspace);
    if (rc) return rc;
    rc = gsr_check_window(window_size);
    if (rc) return rc;
    if (!dL_dimg) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "loss: dL_dimg is NULL");
    GSR_HIP(gsl_launch_backward(C, H, W, img, gt, weight, a_l1, a_ssim, workspace, upstream, dL_dimg, window_size, (hipStream_t)stream),
            "rgb loss backward");
    return GSR_OK;
}

extern "C" int gsr_rgb_loss_forward(int C, int H, int W, const float* img, const float* gt, const float* weight,
                                    float a_l1, float a_ssim, void* workspace, float* out3, int keep_state, void* stream)
{
    return gsr_rgb_loss_forward_window(C, H, W, img, gt, weight, a_l1, a_ssim, 11, workspace, out3, keep_state, stream);
}

extern "C" int gsr_rgb_loss_backward(int C, int H, int W, const float* img, const float* gt, const float* weight,
                                     float a_l1, float a_ssim, const void* workspace, const float* upstream,
                                     float* dL_dimg, void* stream)
{
    return gsr_rgb_loss_backward_window(C, H, W, img, gt, weight, a_l1, a_ssim, 11, workspace, upstream, dL_dimg, stream);
}

// ---- simple_knn (knn.hip) ----
extern "C" size_t gsr_knn_workspace_bytes(int P) { return gsk_workspace_bytes(P); }

extern "C" int gsr_knn_mean_dist2(int P, const float* points, float* mean_dist2, void* workspace, void* stream)
{
    if (P < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "knn: P must be >= 0 (got %d)", P);
    if (P == 0) return GSR_OK;
    if (!points || !mean_dist2 || !workspace) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "knn: a required pointer is NULL");
    const char* why = "";
    hipError_t e = gsk_launch(P, points, mean_dist2, workspace, (hipStream_t)stream, &why);
    if (e != hipSuccess) return gsr_fail(GSR_ERR_HIP, "knn: %s %s", hipGetErrorString(e), why);
    return GSR_OK;
}

// ---- scene initialisation (scene_init.hip) ----
#define GSI_MAX_N (1 << 30)  // (no accepted N wraps a carve: the largest piece is N keys of 8 bytes = 2^33)
extern "C" int gsr_sort_block_keys(void) { return GSR_SORT_BLOCK_KEYS; }

extern "C" size_t gsr_sort_keys_workspace_bytes(int N) { return N < 0 || N > GSI_MAX_N ? 0 : gsi_sort_workspace_bytes(N); }

extern "C" int gsr_sort_keys_u64(int N, const uint64_t* keys_in, uint64_t* keys_out, void* workspace, void* stream)
{
    if (N < 0 || N > GSI_MAX_N) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "sort keys: N=%d (need 0 <= N <= 2^30)", N);
    if (N == 0) return GSR_OK;
    if (!keys_in || !keys_out || !workspace) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "sort keys: keys_in, keys_out or workspace is NULL");
    GSR_HIP(gsi_sort_launch(N, keys_in, keys_out, workspace, (hipStream_t)stream), "sort keys");
    return GSR_OK;
}

extern "C" size_t gsr_voxelize_workspace_bytes(int N) { return N < 0 || N > GSI_MAX_N ? 0 : gsi_voxelize_workspace_bytes(N); }

extern "C" int gsr_voxelize(int N, int fp64, const void* points, double voxel_size, const float* voxel_size_dev, void* workspace, void* out,
                            int32_t* info, void* stream)
{
    if (N < 0 || N > GSI_MAX_N) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "voxelize: N=%d (need 0 <= N <= 2^30)", N);
    if (fp64 != 0 && fp64 != 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "voxelize: fp64=%d (need 0 or 1)", fp64);
    if (!info || (N > 0 && (!points || !workspace || !out)))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "voxelize: points, workspace, out or info is NULL");
    GSR_HIP(gsi_voxelize_launch(N, fp64, points, voxel_size, voxel_size_dev, workspace, out, info, (hipStream_t)stream), "voxelize");
    return GSR_OK;
}

extern "C" size_t gsr_kth_smallest_workspace_bytes(int N) { return N < 1 || N > GSI_MAX_N ? 0 : gsi_kth_workspace_bytes(N); }

extern "C" int gsr_kth_smallest_f32(int N, int k, const float* values, void* workspace, float* out, void* stream)
{
    if (N < 1 || N > GSI_MAX_N) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "kth smallest: N=%d (need 1 <= N <= 2^30)", N);
    if (k < 1 || k > N) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "kth smallest: k=%d out of range for %d values (need 1 <= k <= N)", k, N);
    if (!values || !workspace || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "kth smallest: values, workspace or out is NULL");
    GSR_HIP(gsi_kth_launch(N, k, values, workspace, out, (hipStream_t)stream), "kth smallest");
    return GSR_OK;
}

extern "C" int gsr_scene_init_fill(int M, int K, int F, const float* anchors, const float* dist2, float opacity, float* scaling, float* offset,
                                   float* anchor_feat, float* rotation, float* opacity_out, float* uncertainty_out, float* max_radii2D,
                                   float* xyz_max, void* stream)
{
    if (M < 0 || K < 0 || F < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scene init fill: M=%d K=%d F=%d (need all >= 0)", M, K, F);
    const int64_t widest = (int64_t)M * (3 * (int64_t)K > (int64_t)F ? (3 * (int64_t)K > 6 ? 3 * (int64_t)K : 6) : ((int64_t)F > 6 ? (int64_t)F : 6));
    if (widest >= 0x7fffffffLL) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scene init fill: M=%d K=%d F=%d (need M * max(3 K, F, 6) < 2^31)", M, K, F);
    if (!xyz_max) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scene init fill: xyz_max is NULL");
    if (M > 0 && (!anchors || !dist2 || !scaling || !rotation || !opacity_out || !uncertainty_out || !max_radii2D || (K > 0 && !offset)
                  || (F > 0 && !anchor_feat)))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scene init fill: a required pointer is NULL");
    GSR_HIP(gsi_fill_launch(M, K, F, anchors, dist2, opacity, scaling, offset, anchor_feat, rotation, opacity_out, uncertainty_out, max_radii2D,
                            xyz_max, (hipStream_t)stream),
            "scene init fill");
    return GSR_OK;
}

// ---- neural-Gaussian decode (decode.hip) ----
static int gsr_check_decode(int N, int K, const float* const* weights)
{
    if (N < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: N must be >= 0 (got %d)", N);
    if (K < 1 || K > 10) return gsr_fail(GSR_ERR_UNSUPPORTED, "decode: n_offsets must be in 1..10 (got %d)", K);
    if (!weights) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: weights is NULL");
    for (int i = 0; i < 16; i++)
        if (!weights[i]) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: weights[%d] is NULL", i);
    return GSR_OK;
}

extern "C" int gsr_decode_visible_rows(int N, const uint8_t* visible_mask, int32_t* rows, uint32_t* count, uint32_t* block_scratch, void* stream)
{
    if (N < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: N must be >= 0 (got %d)", N);
    if (!count || (N > 0 && (!visible_mask || !rows || !block_scratch))) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: a required pointer is NULL");
    GSR_HIP(gsd_launch_visible_rows(N, visible_mask, rows, count, block_scratch, (hipStream_t)stream), "decode visible rows");
    return GSR_OK;
}

extern "C" int gsr_decode_count(int N, int K, const float* const* weights, const int32_t* visible, const uint32_t* visible_count, const float* feat, const float* anchor,
                                const float* campos, float* neural_opacity, uint8_t* mask, uint8_t* count, uint32_t* first,
                                uint32_t* total, uint32_t* block_scratch, void* stream)
{
    int rc = gsr_check_decode(N, K, weights);
    if (rc) return rc;
    if (!total) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: total is NULL");
    if (N == 0) { GSR_HIP(hipMemsetAsync(total, 0, 4, (hipStream_t)stream), "decode total"); return GSR_OK; }
    if (!feat || !anchor || !campos || !neural_opacity || !mask || !count || !first || !block_scratch)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: a required pointer is NULL");
    if (visible_count && !visible) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: visible_count without a row list");
    GSR_HIP(gsd_launch_count(N, K, weights, visible, visible_count, feat, anchor, campos, neural_opacity, mask, count, first, total, block_scratch,
                             (hipStream_t)stream),
            "decode count");
    return GSR_OK;
}

extern "C" int gsr_decode_emit(int N, int K, const float* const* weights, const int32_t* visible, const uint32_t* visible_count, const float* feat, const float* anchor,
                               const float* offsets, const float* grid_scaling, const float* campos,
                               const float* neural_opacity, const uint8_t* mask, const uint32_t* first, float* xyz, float* color, float* opacity, float* uncertainty,
                               float* scaling, float* rot, void* stream)
{
    int rc = gsr_check_decode(N, K, weights);
    if (rc) return rc;
    if (N == 0) return GSR_OK;
    if (!feat || !anchor || !offsets || !grid_scaling || !campos || !neural_opacity || !mask || !first)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: a required pointer is NULL");
    GSR_HIP(gsd_launch_emit(N, K, weights, visible, visible_count, feat, anchor, offsets, grid_scaling, campos, neural_opacity, mask, first, xyz, color, opacity,
                            uncertainty, scaling, rot, (hipStream_t)stream), "decode emit");
    return GSR_OK;
}

extern "C" int gsr_decode_backward(int N, int K, const float* const* weights, const int32_t* visible, const float* feat,
                                   const float* anchor, const float* offsets, const float* grid_scaling, const float* campos,
                                         const uint8_t* mask, const uint32_t* first, const float* g_xyz, const float* g_color,
                                         const float* g_opacity, const float* g_uncertainty, const float* g_scaling,
                                         const float* g_rot, float* d_feat, float* d_anchor, float* d_offsets,
                                         float* d_grid_scaling, void* workspace, float* const* grads16, void* stream)
{
    int rc = gsr_check_decode(N, K, weights);
    if (rc) return rc;
    if (!workspace || !grads16) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: workspace / grads16 is NULL");
    for (int i = 0; i < 16; i++)
        if (!grads16[i]) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: grads16[%d] is NULL", i);
    if (N > 0 && (!feat || !anchor || !offsets || !grid_scaling || !campos || !mask || !first || !d_feat || !d_anchor || !d_offsets ||
                  !d_grid_scaling))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: a required pointer is NULL");
    if (!campos) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: campos is NULL");
    GSR_HIP(gsd_launch_backward(N, K, weights, visible, feat, anchor, offsets, grid_scaling, campos, mask, first, g_xyz, g_color,
                                      g_opacity, g_uncertainty, g_scaling, g_rot, d_feat, d_anchor, d_offsets, d_grid_scaling,
                                      workspace, grads16, (hipStream_t)stream), "decode backward");
    return GSR_OK;
}

extern "C" size_t gsr_decode_weight_grad_workspace_bytes(void) { return gsd_weight_grad_workspace_bytes(); }

extern "C" int gsr_decode_zero_hidden_rows(int N, int K, const uint8_t* visible_mask, float* d_feat, float* d_anchor, float* d_offsets,
                                           float* d_grid_scaling, void* stream)
{
    if (N < 0 || K < 1 || K > 10) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: bad sizes N=%d K=%d", N, K);
    if (N == 0) return GSR_OK;
    if (!visible_mask || !d_feat || !d_anchor || !d_offsets || !d_grid_scaling)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "decode: a required pointer is NULL");
    GSR_HIP(gsd_launch_zero_hidden(N, K, visible_mask, d_feat, d_anchor, d_offsets, d_grid_scaling, (hipStream_t)stream), "decode zero hidden rows");
    return GSR_OK;
}

// ---- depth loss (depth_loss.hip) ----
extern "C" size_t gsr_depth_loss_workspace_bytes(int H, int W) { return gdl_workspace_bytes(H, W); }

extern "C" int gsr_depth_loss_forward(int H, int W, const float* depth, const float* target, const float* lsq_mask,
                                      const float* l1_weight, const float* grad_mask, float lambda_l1, float lambda_smooth,
                                      void* workspace, float* out5, void* stream)
{
    if (H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "depth loss: bad size %dx%d", W, H);
    if (!depth || !target || !workspace || !out5) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "depth loss: a required pointer is NULL");
    GSR_HIP(gdl_launch_forward(H, W, depth, target, lsq_mask, l1_weight, grad_mask, lambda_l1, lambda_smooth, workspace, out5,
                               (hipStream_t)stream), "depth loss forward");
    return GSR_OK;
}

extern "C" int gsr_depth_loss_backward(int H, int W, const float* depth, const float* target, const float* lsq_mask,
                                       const void* workspace, const float* upstream, float* dL_ddepth, void* stream)
{
    if (H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "depth loss: bad size %dx%d", W, H);
    if (!depth || !target || !workspace || !dL_ddepth) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "depth loss: a required pointer is NULL");
    GSR_HIP(gdl_launch_backward(H, W, depth, target, lsq_mask, workspace, upstream, dL_ddepth, (hipStream_t)stream), "depth loss backward");
    return GSR_OK;
}

// ---- densification statistics (stats.hip) ----
extern "C" int gsr_training_stats(int Nv, int K, int M, const int32_t* visible, const float* neural_opacity, const uint8_t* selection,
                                  const uint32_t* first, const uint8_t* update_filter, const float* viewspace_grad,
                                  float* opacity_accum, float* anchor_demon, float* offset_gradient_accum,
                                  float* offset_denom, void* stream)
{
    if (Nv < 0 || K < 1 || M < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "training stats: bad sizes Nv=%d K=%d M=%d", Nv, K, M);
    if (Nv == 0) return GSR_OK;
    if (!neural_opacity || !selection || !first || !opacity_accum || !anchor_demon || !offset_gradient_accum || !offset_denom)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "training stats: a required pointer is NULL");
    // update_filter / viewspace_grad may be NULL only if no offset was selected (M = 0); the kernel then never reads them
    if (M > 0 && (!update_filter || !viewspace_grad)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "training stats: update_filter / viewspace_grad is NULL with M = %d", M);
    GSR_HIP(gst_launch_training_stats(Nv, K, M, visible, neural_opacity, selection, first, update_filter, viewspace_grad,
                                      opacity_accum, anchor_demon, offset_gradient_accum, offset_denom, (hipStream_t)stream),
            "training stats");
    return GSR_OK;
}


// ---- anchor growing (anchor_grow.hip) ----
extern "C" size_t gsr_anchor_grow_workspace_bytes(int N, int L)
{
    if (N < 0 || L < 0) return 0;
    return gag_workspace_bytes(N, L);
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
                                    int32_t* info, void* stream)
{
    if (int rc = gag_check_sizes("anchor grow keys", N, K, L)) return rc;
    if (!workspace || !info || (N > 0 && !anchor) || (L > 0 && (!offset || !scaling || !candidate_mask || !keys || !rows)))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor grow keys: a required pointer is NULL");
    GSR_HIP(gag_launch_keys(N, K, L, anchor, offset, scaling, candidate_mask, inv_size, workspace, keys, rows, info, (hipStream_t)stream),
            "anchor grow keys");
    return GSR_OK;
}

extern "C" int gsr_anchor_grow_emit(int N, int K, int F, int L, int M, const float* anchor_feat, const int64_t* sorted_keys,
                                    const int64_t* order, const int32_t* rows, float cur_size, void* workspace, float* candidate_anchor,
                                    float* new_feat, int32_t* info, void* stream)
{
    if (int rc = gag_check_sizes("anchor grow emit", N, K, L)) return rc;
    if (F < 0 || M < 0 || M > L) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor grow emit: bad sizes F=%d M=%d L=%d", F, M, L);
    if (!workspace || !info || (M > 0 && (!sorted_keys || !order || !rows || !candidate_anchor || (F > 0 && (!anchor_feat || !new_feat)))))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor grow emit: a required pointer is NULL");
    GSR_HIP(gag_launch_emit(N, K, F, L, M, anchor_feat, sorted_keys, order, rows, cur_size, workspace, candidate_anchor, new_feat, info,
                            (hipStream_t)stream),
            "anchor grow emit");
    return GSR_OK;
}

extern "C" int gsr_scatter_max(int R, int F, int S, const float* src, const int64_t* index, float* out, int64_t* argmax, void* stream)
{
    if (R < 0 || F < 0 || S < 0 || (long long)R * F > (1ll << 40) || (long long)S * F > (1ll << 40))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scatter_max: bad sizes R=%d F=%d S=%d", R, F, S);
    if ((long long)S * F > 0 && (!out || !argmax)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scatter_max: out / argmax is NULL");
    if ((long long)R * F > 0 && (long long)S * F > 0 && (!src || !index)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "scatter_max: src / index is NULL");
    GSR_HIP(gag_launch_scatter_max(R, F, S, src, index, out, argmax, (hipStream_t)stream), "scatter_max");
    return GSR_OK;
}

// ---- bidirectional cross-attention core (crossattn.hip) ----
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
    return gca_workspace_bytes(B, H, I, J);
}

extern "C" int gsr_crossattn_forward(int B, int H, int I, int J, int dim_head, const float* qk, const float* v, const float* context_qk,
                                     const float* context_v, const uint8_t* mask, const uint8_t* context_mask, float scale, float* out,
                                     float* context_out, void* workspace, void* stream)
{
    if (int rc = gca_check_sizes("crossattn forward", B, H, I, J, dim_head)) return rc;
    if (!qk || !v || !context_qk || !context_v || !out || !context_out || !workspace)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "crossattn forward: a required pointer is NULL");
    GSR_HIP(gca_launch_forward(B, H, I, J, qk, v, context_qk, context_v, mask, context_mask, scale, out, context_out, workspace,
                               (hipStream_t)stream),
            "crossattn forward");
    return GSR_OK;
}

extern "C" int gsr_crossattn_backward(int B, int H, int I, int J, int dim_head, const float* qk, const float* v, const float* context_qk,
                                      const float* context_v, const uint8_t* mask, const uint8_t* context_mask, float scale,
                                      const float* out, const float* context_out, const float* d_out, const float* d_context_out,
                                      void* workspace, float* d_qk, float* d_v, float* d_context_qk, float* d_context_v, void* stream)
{
    if (int rc = gca_check_sizes("crossattn backward", B, H, I, J, dim_head)) return rc;
    if (!qk || !v || !context_qk || !context_v || !out || !context_out || !d_out || !d_context_out || !workspace || !d_qk || !d_v
        || !d_context_qk || !d_context_v)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "crossattn backward: a required pointer is NULL");
    GSR_HIP(gca_launch_backward(B, H, I, J, qk, v, context_qk, context_v, mask, context_mask, scale, out, context_out, d_out,
                                d_context_out, workspace, d_qk, d_v, d_context_qk, d_context_v, (hipStream_t)stream),
            "crossattn backward");
    return GSR_OK;
}

// ---- cross-attention anchor sampler (anchor_sample.hip) ----
static int gas_check_sizes(int N, int H, int W, int max_pairs)
{
    if (N < 0 || N > 0x7fffff00 || max_pairs < 0 || H < 1 || W < 1 || H > (1 << 24) || W > (1 << 24) || (long long)H * W > 0x7fffffffLL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor sample: bad sizes N=%d H=%d W=%d max_pairs=%d", N, H, W, max_pairs);
    // (no accepted size wraps the carve: N < 2^31 bytes per array)
    return GSR_OK;
}

extern "C" size_t gsr_anchor_sample_workspace_bytes(int N, int max_pairs)
{
    if (N < 0 || N > 0x7fffff00 || max_pairs < 0) return 0;
    return gas_workspace_bytes(N, max_pairs);
}

extern "C" int gsr_anchor_sample(int N, int H, int W, const uint8_t* visible, const float* px, const float* py, const float* gt_mask,
                                 int min_y, int max_y, int min_x, int max_x, int max_pairs, uint64_t seed, void* workspace,
                                 uint8_t* src_mask, uint8_t* dst_mask, int64_t* src_rows, int64_t* dst_rows, int32_t* info, void* stream)
{
    if (int rc = gas_check_sizes(N, H, W, max_pairs)) return rc;
    if (!info || (N > 0 && (!workspace || !visible || !px || !py || !gt_mask || !src_mask || !dst_mask))
        || (N > 0 && max_pairs > 0 && (!src_rows || !dst_rows)))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor sample: a required pointer is NULL");
    GSR_HIP(gas_launch(N, H, W, visible, px, py, gt_mask, min_y, max_y, min_x, max_x, max_pairs, seed, workspace, src_mask, dst_mask,
                       src_rows, dst_rows, info, (hipStream_t)stream),
            "anchor sample");
    return GSR_OK;
}

// ---- anchor pruning (anchor_adjust.hip) ----
extern "C" size_t gsr_anchor_adjust_workspace_bytes(int N)
{
    if (N < 0 || N > 0x7fffff00) return 0;  // (no accepted N wraps the carve: N bytes + N / 256 sums)
    return gaa_workspace_bytes(N);
}

extern "C" int gsr_anchor_adjust_offsets(int L0, const float* offset_gradient_accum, const float* offset_denom, float denom_threshold,
                                         float* grads_norm, uint8_t* offset_mask, void* stream)
{
    if (L0 < 0 || L0 > 0x7fffff00) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust offsets: bad size L0=%d", L0);
    if (L0 > 0 && (!offset_gradient_accum || !offset_denom || !grads_norm || !offset_mask))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust offsets: a required pointer is NULL");
    GSR_HIP(gaa_launch_offsets(L0, offset_gradient_accum, offset_denom, denom_threshold, grads_norm, offset_mask, (hipStream_t)stream),
            "anchor adjust offsets");
    return GSR_OK;
}

extern "C" int gsr_anchor_adjust_plan(int N, const float* opacity_accum, const float* anchor_demon, const uint8_t* prune_mask,
                                      float min_opacity, float demon_threshold, void* workspace, int32_t* keep_rows, uint8_t* reset,
                                      int32_t* info, void* stream)
{
    if (N < 0 || N > 0x7fffff00) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust plan: bad size N=%d", N);
    if (!info || (N > 0 && (!workspace || !keep_rows || !reset || (!prune_mask && (!opacity_accum || !anchor_demon)))))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust plan: a required pointer is NULL");
    GSR_HIP(gaa_launch_plan(N, opacity_accum, anchor_demon, prune_mask, min_opacity, demon_threshold, workspace, keep_rows, reset, info,
                            (hipStream_t)stream),
            "anchor adjust plan");
    return GSR_OK;
}

extern "C" int gsr_anchor_adjust_gather(int N, int n_keep, int n_copies, const gsr_adjust_copy* copies, const int32_t* keep_rows,
                                        const uint8_t* offset_mask, int L0, const uint8_t* reset, void* stream)
{
    if (N < 0 || n_keep < 0 || n_keep > N || n_copies < 0 || n_copies > GSR_ADJUST_MAX_COPIES || L0 < 0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: bad sizes N=%d n_keep=%d n_copies=%d L0=%d", N, n_keep, n_copies, L0);
    if (n_keep == 0 || n_copies == 0) return GSR_OK;
    if (!copies || !keep_rows) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: copies / keep_rows is NULL");
    for (int c = 0; c < n_copies; c++) {
        const gsr_adjust_copy& d = copies[c];
        if (d.width < 1 || (long long)N * d.width > 0x7fffffffLL || d.mode < GSR_ADJUST_COPY || d.mode > GSR_ADJUST_ANCHOR_STAT)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: copy %d has width %d, mode %d (need 1 <= width, N*width < 2^31)", c,
                            d.width, d.mode);
        if (!d.dst || (!d.src && !(d.mode == GSR_ADJUST_OFFSET_STAT && L0 == 0)))
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: copy %d has a NULL pointer", c);
        if (d.mode == GSR_ADJUST_OFFSET_STAT && L0 > 0 && !offset_mask)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: copy %d is OFFSET_STAT but offset_mask is NULL", c);
        if (d.mode == GSR_ADJUST_OFFSET_STAT && (long long)L0 > (long long)N * d.width)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: L0=%d exceeds N*K=%lld", L0, (long long)N * d.width);
        if (d.mode == GSR_ADJUST_ANCHOR_STAT && (d.width != 1 || !reset))
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "anchor adjust gather: copy %d is ANCHOR_STAT: width must be 1 and reset given", c);
    }
    GSR_HIP(gaa_launch_gather(n_keep, n_copies, copies, keep_rows, offset_mask, L0, reset, (hipStream_t)stream), "anchor adjust gather");
    return GSR_OK;
}

// ---- optimiser step (adam.hip) ----
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
    GSR_HIP(adam_launch(n_tensors, tensors, (hipStream_t)stream), "adam step");
    return GSR_OK;
}

// ---- normals from rendered depth (normals.hip) ----
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
    GSR_HIP(normals_launch_points(H, W, depth, K, c2w, points, (hipStream_t)stream), "depth points");
    return GSR_OK;
}

extern "C" int gsr_point_normals(int H, int W, const float* points, int size, float gamma, double eps, float* normals, void* stream)
{
    if (int rc = normals_check_frame("point normals", H, W)) return rc;
    if (size < 1 || size > 15 || size % 2 == 0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "point normals: size=%d (need an odd size, 1 .. 15)", size);
    if (!points || !normals) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "point normals: points or normals is NULL");
    GSR_HIP(normals_launch_fit(H, W, points, size, gamma, eps, normals, (hipStream_t)stream), "point normals");
    return GSR_OK;
}

// ---- test-view metrics (metrics.hip) ----
static int metrics_check_sizes(int B, int C, int H, int W)
{
    if (B <= 0 || C <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: B=%d C=%d (need both > 0)", B, C);
    if ((int64_t)B * (int64_t)C > 65535)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: B=%d C=%d has too many planes (need B*C <= 65535)", B, C);
    if (H < 3 || W < 3) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: H=%d W=%d (need both >= 3: reflect padding of 2)", H, W);
    if ((double)C * (double)H * (double)W >= 2147483392.0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: C=%d H=%d W=%d has too many elements (need C*H*W < 2^31 - 256)", C, H, W);
    // (no accepted size wraps the carve: 65535 planes of fewer than 2^22 tiles, 64 bytes each)
    return GSR_OK;
}

extern "C" size_t gsr_image_metrics_workspace_bytes(int B, int C, int H, int W)
{
    if (metrics_check_sizes(B, C, H, W)) return 0;
    return metrics_workspace_bytes(B, C, H, W);
}

extern "C" int gsr_image_metrics(int B, int C, int H, int W, const float* pred, const float* gt, const uint8_t* mask, long long mask_stride_b,
                                 long long mask_stride_c, int flags, void* workspace, double* sums, float* metrics, void* stream)
{
    if (int rc = metrics_check_sizes(B, C, H, W)) return rc;
    if (!pred || !gt || !workspace || !sums || !metrics)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: pred, gt, workspace, sums or metrics is NULL");
    if (flags & ~(GSR_METRICS_CLAMP | GSR_METRICS_QUANTIZE)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: unknown flag bits in %d", flags);
    if (mask_stride_b < 0 || mask_stride_c < 0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "image metrics: negative mask stride (%lld, %lld)", mask_stride_b, mask_stride_c);
    double taps[3], total = 0.0;  // g_k = exp(-(k-2)^2 / 4.5) / sum, k = 0 .. 4 (sigma 1.5), in fp64
    for (int k = 0; k < 3; k++) taps[k] = exp(-(double)((k - 2) * (k - 2)) / 4.5);
    total = ((taps[0] + taps[1]) + taps[2]) + (taps[1] + taps[0]);
    for (int k = 0; k < 3; k++) taps[k] /= total;
    GSR_HIP(metrics_launch(B, C, H, W, pred, gt, mask, mask_stride_b, mask_stride_c, flags, taps, workspace, sums, metrics, (hipStream_t)stream),
            "image metrics");
    return GSR_OK;
}

// ---- LPIPS (lpips.hip) ----
static int lpips_check_sizes(int B, int H, int W)
{
    if (B <= 0 || B > 32767) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: B=%d (need 1 .. 32767 views: 2B images are one batch)", B);
    if (H < 16 || W < 16) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: H=%d W=%d (need both >= 16: four 2x2 pools)", H, W);
    if ((int64_t)H * (int64_t)W >= 0x7fffff00LL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: H=%d W=%d has too many pixels (need H*W < 2^31 - 256)", H, W);
    // (no accepted size wraps the carve: an activation buffer is 2 B * 64 * H*W floats < 2^15 * 2^9 * 2^31 = 2^55 bytes)
    return GSR_OK;
}

extern "C" size_t gsr_lpips_workspace_bytes(int B, int H, int W)
{
    if (lpips_check_sizes(B, H, W)) return 0;
    return lpips_workspace_bytes(B, H, W);
}

extern "C" int gsr_lpips(int B, int H, int W, const float* in0, const float* in1, int flags, const float* conv_weights, const float* conv_bias,
                         const float* lin_weights, const uint8_t* mask, long long mask_stride_b, void* workspace, float* out_plain,
                         float* out_layers, float* out_masked, float* out_spatial, void* stream)
{
    if (int rc = lpips_check_sizes(B, H, W)) return rc;
    if (!in0 || !in1 || !conv_weights || !conv_bias || !lin_weights || !workspace || !out_plain)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: in0, in1, conv_weights, conv_bias, lin_weights, workspace or out_plain is NULL");
    if (flags & ~GSR_LPIPS_NORMALIZE) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: unknown flag bits in %d", flags);
    if (mask_stride_b < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "lpips: negative mask stride %lld", mask_stride_b);
    GSR_HIP(lpips_launch(B, H, W, in0, in1, flags, conv_weights, conv_bias, lin_weights, mask, mask_stride_b, workspace, out_plain, out_layers,
                         out_masked, out_spatial, (hipStream_t)stream),
            "lpips");
    return GSR_OK;
}

extern "C" int gsr_conv3x3_relu(int B, int Cin, int Cout, int H, int W, const float* in, const float* weights_packed, const float* bias,
                                float* out, int flags, void* stream)
{
    if (B <= 0 || B > 65535) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: B=%d (need 1 .. 65535 images)", B);
    if (Cin <= 0 || Cout <= 0 || Cout % LPIPS_CONV_NB != 0)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: Cin=%d Cout=%d (need Cin > 0 and Cout a positive multiple of %d)", Cin, Cout, LPIPS_CONV_NB);
    if (Cin > 65536 || Cout > 65536) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: Cin=%d Cout=%d is too wide", Cin, Cout);
    if (H <= 0 || W <= 0 || (int64_t)H * (int64_t)W >= 0x7fffff00LL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: H=%d W=%d (need both > 0 and H*W < 2^31 - 256)", H, W);
    if (!in || !weights_packed || !bias || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: in, weights_packed, bias or out is NULL");
    if (flags & ~(GSR_LPIPS_NORMALIZE | GSR_LPIPS_SCALING)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: unknown flag bits in %d", flags);
    if (flags && Cin != 3) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "conv3x3: the input transforms are for Cin = 3 (got %d)", Cin);
    GSR_HIP(lpips_launch_conv(B, Cin, Cout, H, W, in, weights_packed, bias, out, flags, (hipStream_t)stream), "conv3x3");
    return GSR_OK;
}

// ---- render_set's output frames (frames.hip) ----
static int frames_check_sizes(const char* what, int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: B=%d H=%d W=%d (need all > 0)", what, B, H, W);
    if (B > 65535) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: B=%d has too many frames (need B <= 65535)", what, B);
    if ((int64_t)H * (int64_t)W >= 0x7fffff00LL / 4)  // (H*W*4 itself can pass 2^63)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "%s: H=%d W=%d has too many pixels (need H*W*4 < 2^31 - 256)", what, H, W);
    // (no accepted size wraps the carve: 65535 frames of fewer than 2^17 chunks, 64 bytes each)
    return GSR_OK;
}

extern "C" size_t gsr_frame_stats_workspace_bytes(int B, int H, int W)
{
    if (frames_check_sizes("frame stats", B, H, W)) return 0;
    return frames_stats_workspace_bytes(B, H, W);
}

extern "C" int gsr_frame_stats(int B, int H, int W, const float* depth, const float* target, const float* lsq_mask, void* workspace,
                               double* stats, float* params, void* stream)
{
    if (int rc = frames_check_sizes("frame stats", B, H, W)) return rc;
    if (!depth || !workspace || !stats || !params)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame stats: depth, workspace, stats or params is NULL");
    if (lsq_mask && !target) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame stats: an lsq_mask needs a target, which is NULL");
    GSR_HIP(frames_launch_stats(B, H, W, depth, target, lsq_mask, workspace, stats, params, (hipStream_t)stream), "frame stats");
    return GSR_OK;
}

extern "C" int gsr_frame_compose(int B, int H, int W_out, int channels_out, int n, const gsr_frame_panel* panels, const float* params,
                                 uint8_t* out, void* stream)
{
    if (int rc = frames_check_sizes("frame compose", B, H, W_out)) return rc;
    if (channels_out != 3 && channels_out != 4)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: channels_out=%d (need 3 or 4)", channels_out);
    if (n < 1 || n > GSR_FRAME_MAX_PANELS)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: n=%d panels (need 1 .. %d)", n, GSR_FRAME_MAX_PANELS);
    if (!panels || !out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panels or out is NULL");
    int order[GSR_FRAME_MAX_PANELS];
    for (int j = 0; j < n; j++) {
        const gsr_frame_panel& p = panels[j];
        if (p.mode < GSR_FRAME_QUANT || p.mode > GSR_FRAME_CMAP_MPL)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d has the unknown mode %d", j, p.mode);
        if (!p.src) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d has a NULL src", j);
        if (p.mode == GSR_FRAME_ABSDIFF && !p.src2) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d is ABSDIFF with a NULL src2", j);
        if (p.mode >= GSR_FRAME_CMAP_CV && (!p.lut || !params))
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d has a CMAP mode with a NULL lut or params", j);
        if (p.width <= 0 || p.x0 < 0 || (int64_t)p.x0 + (int64_t)p.width > (int64_t)W_out)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d covers columns [%d, %lld), outside [0, %d) or empty", j, p.x0,
                            (long long)p.x0 + (long long)p.width, W_out);
        int k = j;  // insertion by x0
        for (; k > 0 && panels[order[k - 1]].x0 > p.x0; k--) order[k] = order[k - 1];
        order[k] = j;
    }
    int next = 0;
    for (int k = 0; k < n; k++) {
        const gsr_frame_panel& p = panels[order[k]];
        if (p.x0 != next)
            return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: panel %d starts at column %d where %d is next (the panels %s)", order[k], p.x0,
                            next, p.x0 < next ? "overlap" : "leave a gap");
        next = p.x0 + p.width;
    }
    if (next != W_out) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "frame compose: the panels end at column %d of %d (they leave a gap)", next, W_out);
    const bool dwords = ((uintptr_t)out & 3) == 0 && (channels_out == 4 || W_out % 4 == 0);
    GSR_HIP(frames_launch_compose(B, H, W_out, channels_out, n, panels, params, out, dwords, (hipStream_t)stream), "frame compose");
    return GSR_OK;
}

// ---- PNG encoding (png.hip) ----
static int png_check_sizes(int B, int H, int W, int C)
{
    if (B <= 0 || H <= 0 || W <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: B=%d H=%d W=%d (need all > 0)", B, H, W);
    if (C != 1 && C != 3 && C != 4) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: C=%d (need 1, 3 or 4)", C);
    if (B > 65535) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: B=%d has too many pictures (need B <= 65535)", B);
    if ((int64_t)W * C >= (1 << 24)) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: W=%d C=%d has too long a row (need W*C < 2^24)", W, C);
    if ((int64_t)H * ((int64_t)W * C + 1) >= 0x70000000LL)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: H=%d W=%d C=%d has too many bytes (need H*(1 + W*C) < 0x70000000)", H, W, C);
    // (no accepted size wraps the layout: a picture's part is below 2^32 bytes, B below 2^16)
    return GSR_OK;
}

extern "C" size_t gsr_png_capacity(int H, int W, int C) { return png_check_sizes(1, H, W, C) ? 0 : png_layout(H, W, C).capacity; }

extern "C" size_t gsr_png_workspace_bytes(int B, int H, int W, int C)
{
    return png_check_sizes(B, H, W, C) ? 0 : (size_t)B * png_layout(H, W, C).per_picture;
}

extern "C" int gsr_png_encode(const uint8_t* images, long long row_stride, long long image_stride, int B, int H, int W, int C, int filter,
                              uint8_t* out, size_t out_stride, void* workspace, void* stream)
{
    if (int rc = png_check_sizes(B, H, W, C)) return rc;
    if (!images || !out || !workspace) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: images, out or workspace is NULL");
    if (filter < 0 || filter > GSR_PNG_FILTER_ADAPTIVE)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: filter=%d (need 0 .. 4 or GSR_PNG_FILTER_ADAPTIVE)", filter);
    if (row_stride < (long long)W * C) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: row_stride=%lld is below W*C=%lld", row_stride, (long long)W * C);
    if (B > 1 && image_stride < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: image_stride=%lld is negative", image_stride);
    const size_t need = GSR_PNG_HEADER_BYTES + png_layout(H, W, C).capacity;
    if (out_stride < need || out_stride % 4 || ((uintptr_t)out & 3))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: out_stride=%zu (need >= %zu = header + capacity, a multiple of 4) or out is not 4-byte aligned",
                        out_stride, need);
    if ((uintptr_t)workspace & 15) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png: workspace is not 16-byte aligned");
    GSR_HIP(png_launch_encode(images, row_stride, image_stride, B, H, W, C, filter, out, out_stride, workspace, (hipStream_t)stream), "png encode");
    return GSR_OK;
}

// ---- JPEG encoding (jpeg.hip) ----
static int jpeg_check_sizes(int B, int H, int W, int C, int subsampling)
{
    if (B <= 0 || H <= 0 || W <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: B=%d H=%d W=%d (need all > 0)", B, H, W);
    if (C != 1 && C != 3) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: C=%d (need 1 or 3)", C);
    if (B > 65535 || H > 65535 || W > 65535) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: B=%d H=%d W=%d (need all <= 65535)", B, H, W);
    if (subsampling != 444 && subsampling != 420) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: subsampling=%d (need 444 or 420)", subsampling);
    if (subsampling == 420 && C == 1) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: subsampling 420 with C=1 (a grey picture has no chroma)");
    if (jpeg_layout(H, W, C, subsampling, 0).capacity >= ((size_t)1 << 31))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: H=%d W=%d C=%d has a capacity of 2^31 bytes or more", H, W, C);
    // (no accepted size wraps the layout: a picture's part is below 2^32 bytes, B below 2^16)
    return GSR_OK;
}

static int jpeg_check_interval(int C, int subsampling, int restart_interval)
{
    const int most = GSR_JPEG_INTERVAL_BLOCKS / (C == 1 ? 1 : (subsampling == 420 ? 6 : 3));
    if (restart_interval < 0 || restart_interval > most)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: restart_interval=%d (need 0 = the default, or 1 .. %d MCUs)", restart_interval, most);
    return GSR_OK;
}

// a pointer the kernels may use: device memory of this process
static bool jpeg_on_device(const void* p)
{
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();  // (an unregistered host pointer: the error is ours to clear)
        return false;
    }
    return attr.type == hipMemoryTypeDevice;
}

extern "C" size_t gsr_jpeg_capacity(int H, int W, int C, int subsampling)
{
    return jpeg_check_sizes(1, H, W, C, subsampling) ? 0 : jpeg_layout(H, W, C, subsampling, 0).capacity;
}

extern "C" size_t gsr_jpeg_workspace_bytes(int B, int H, int W, int C, int subsampling, int restart_interval)
{
    if (jpeg_check_sizes(B, H, W, C, subsampling) || jpeg_check_interval(C, subsampling, restart_interval)) return 0;
    return (size_t)B * jpeg_layout(H, W, C, subsampling, restart_interval).per_picture;
}

extern "C" int gsr_jpeg_encode(const uint8_t* images, long long row_stride, long long image_stride, int B, int H, int W, int C, int quality,
                               int subsampling, int restart_interval, uint8_t* out, size_t out_stride, void* workspace, void* stream)
{
    if (int rc = jpeg_check_sizes(B, H, W, C, subsampling)) return rc;
    if (int rc = jpeg_check_interval(C, subsampling, restart_interval)) return rc;
    if (!images || !out || !workspace) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: images, out or workspace is NULL");
    if (quality < 1 || quality > 100) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: quality=%d (need 1 .. 100)", quality);
    if (row_stride < (long long)W * C) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: row_stride=%lld is below W*C=%lld", row_stride, (long long)W * C);
    if (B > 1 && image_stride < 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: image_stride=%lld is negative", image_stride);
    const JpegLayout lay = jpeg_layout(H, W, C, subsampling, restart_interval);
    const size_t need = GSR_JPEG_HEADER_BYTES + lay.file_header;
    if (out_stride < need || out_stride % 4 || ((uintptr_t)out & 3))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: out_stride=%zu (need >= %zu = the four words + the file header, a multiple of 4) or out is not 4-byte aligned",
                        out_stride, need);
    if ((uintptr_t)workspace & 15) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: workspace is not 16-byte aligned");
    if (!jpeg_on_device(images) || !jpeg_on_device(out) || !jpeg_on_device(workspace))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg: images, out or workspace is not device memory");
    JpegTables tables;
    jpeg_fill_tables(&tables, H, W, C, quality, subsampling, lay);
    GSR_HIP(jpeg_launch_encode(images, row_stride, image_stride, B, H, W, C, tables, lay, out, out_stride, workspace, (hipStream_t)stream), "jpeg encode");
    return GSR_OK;
}

// ---- PNG decoding (png_decode.hip) ----
extern "C" size_t gsr_png_decode_workspace_bytes(size_t stream_bytes, int nfiles, int npieces)
{
    if (nfiles <= 0 || npieces <= 0 || stream_bytes >= ((size_t)1 << 40)) return 0;  // (no accepted size wraps the carve: 2^40 + 2^31 * 12 + 2^31 * 4)
    return png_decode_workspace_bytes(stream_bytes, nfiles, npieces);
}

extern "C" int gsr_png_decode(const uint8_t* bytes, size_t nbytes, const gsr_png_file* files, int nfiles, const gsr_png_piece* pieces, int npieces,
                              int verify_crc, uint8_t* out, size_t out_bytes, int32_t* status, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!bytes || !files || !pieces || !out || !status || !workspace)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png decode: bytes, files, pieces, out, status or workspace is NULL");
    if (nfiles <= 0 || npieces <= 0) return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png decode: nfiles=%d npieces=%d (need both > 0)", nfiles, npieces);
    if (nbytes >= ((size_t)1 << 32) || out_bytes >= ((size_t)1 << 32))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png decode: nbytes=%zu out_bytes=%zu (need both < 2^32)", nbytes, out_bytes);
    if (((uintptr_t)bytes & 15) || ((uintptr_t)out & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)files & 7) || ((uintptr_t)pieces & 7) ||
        ((uintptr_t)status & 3))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png decode: bytes, out and workspace are 16-byte aligned, the tables 8, status 4");
    if (workspace_bytes < pd_tables_bytes(nfiles, npieces))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "png decode: workspace_bytes=%zu is below the tables' part alone", workspace_bytes);
    GSR_HIP(png_launch_decode(bytes, nbytes, files, nfiles, pieces, npieces, verify_crc, out, out_bytes, status, workspace, workspace_bytes,
                              (hipStream_t)stream),
            "png decode");
    return GSR_OK;
}

// ---- JPEG decoding (jpeg_decode.hip; declared in include/gsraster_jpeg_decode.h) ----
extern "C" size_t gsr_jpeg_decode_workspace_bytes(size_t area_bytes, int nfiles, int nintervals)
{
    if (nfiles <= 0 || nintervals <= 0 || area_bytes >= ((size_t)1 << 40)) return 0;  // (no accepted size wraps the carve: 2^40 + 2^31 * 16)
    return jpeg_decode_workspace_bytes(area_bytes, nintervals);
}

extern "C" int gsr_jpeg_decode(const uint8_t* bytes, size_t nbytes, const gsr_jpeg_file* files, int nfiles, int nintervals, const uint16_t* quant,
                               int nquant, const gsr_jpeg_huffman* huffman, int nhuffman, uint8_t* out, size_t out_bytes, int32_t* status,
                               void* workspace, size_t workspace_bytes, void* stream)
{
    if (!bytes || !files || !quant || !huffman || !out || !status || !workspace)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode: bytes, files, quant, huffman, out, status or workspace is NULL");
    if (nfiles <= 0 || nintervals <= 0 || nquant <= 0 || nhuffman <= 0 || nfiles > 65535)
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode: nfiles=%d nintervals=%d nquant=%d nhuffman=%d (need all > 0, nfiles <= 65535)", nfiles,
                        nintervals, nquant, nhuffman);
    if (nbytes >= ((size_t)1 << 32) || out_bytes >= ((size_t)1 << 32))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode: nbytes=%zu out_bytes=%zu (need both < 2^32)", nbytes, out_bytes);
    if (((uintptr_t)bytes & 15) || ((uintptr_t)out & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)quant & 15) || ((uintptr_t)files & 7) ||
        ((uintptr_t)status & 3))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode: bytes, out, workspace and quant are 16-byte aligned, files 8, status 4");
    if (workspace_bytes < jd_tables_bytes(nintervals))
        return gsr_fail(GSR_ERR_INVALID_ARGUMENT, "jpeg decode: workspace_bytes=%zu is below the tables' part alone", workspace_bytes);
    GSR_HIP(jpeg_launch_decode(bytes, nbytes, files, nfiles, nintervals, quant, nquant, huffman, nhuffman, out, out_bytes, status, workspace,
                               workspace_bytes, (hipStream_t)stream),
            "jpeg decode");
    return GSR_OK;
}

extern "C" const char* gsr_jpeg_decode_status_name(int code)
{
    static const char* const names[] = {"ok", "truncated", "bit pattern with no symbol", "invalid symbol", "run past coefficient 63",
                                        "restart markers miscounted, misnumbered or misplaced", "table entry out of bounds"};
    return code >= GSR_JPEG_DECODE_OK && code <= GSR_JPEG_DECODE_TABLE ? names[code] : "?";
}

// ---- resize (resize.hip) ----
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
                             int epilogue, void* stream)
{
    if (int rc = resize_check_pass("resize_u8", axis, out_len, bounds, coeffs, ksize)) return rc;
    const int H_out = axis == GSR_RESIZE_VERTICAL ? out_len : H, W_out = axis == GSR_RESIZE_VERTICAL ? W : out_len;
    if (int rc = resize_check("resize_u8", src, out, src_image_stride, src_row_stride, n, H, W, C, H_out, W_out, out_image_stride, out_row_stride, epilogue))
        return rc;
    GSR_HIP(resize_launch_u8(src, src_image_stride, src_row_stride, n, H, W, C, axis, out_len, bounds, coeffs, ksize, out, out_image_stride,
                             out_row_stride, epilogue, (hipStream_t)stream), "resize_u8");
    return GSR_OK;
}

extern "C" int gsr_resize_f32(const float* src, long long src_image_stride, long long src_row_stride, int n, int H, int W, int axis, int out_len,
                              const int32_t* bounds, const double* coeffs, int ksize, float* out, long long out_image_stride, long long out_row_stride,
                              void* stream)
{
    if (int rc = resize_check_pass("resize_f32", axis, out_len, bounds, coeffs, ksize)) return rc;
    const int H_out = axis == GSR_RESIZE_VERTICAL ? out_len : H, W_out = axis == GSR_RESIZE_VERTICAL ? W : out_len;
    if (int rc = resize_check("resize_f32", src, out, src_image_stride, src_row_stride, n, H, W, 1, H_out, W_out, out_image_stride, out_row_stride,
                              GSR_RESIZE_U8))
        return rc;
    GSR_HIP(resize_launch_f32(src, src_image_stride, src_row_stride, n, H, W, axis, out_len, bounds, coeffs, ksize, out, out_image_stride,
                              out_row_stride, (hipStream_t)stream), "resize_f32");
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
