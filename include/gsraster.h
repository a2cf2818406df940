/*
 * gsraster.h -- C ABI of libgsraster.so, the MI355X (gfx950) differentiable Gaussian rasterizer.
 *
 * This is the drop-in boundary for the ONE hot path of W-Ted/GScream: the native module
 * `diff_gaussian_rasterization._C` (reference: submodules/diff-gaussian-rasterization, "DGR").
 * The reference binds five pybind11 functions (DGR/ext.cpp:15-21) that take torch::Tensor; this
 * library exposes the same operations as plain `extern "C"` entry points taking raw DEVICE
 * pointers, sizes and a hipStream_t -- no torch types, no C++ types, no exceptions.
 * gscream_amd/_native.py (ctypes) is the only caller; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every pointer is a device pointer unless its name ends in _host;
 *   - all float arrays are contiguous row-major fp32, images are CHW (DGR forward.cu:563);
 *   - matrices are the transposed / row-vector form GScream passes (scene/cameras.py:64-67):
 *     p_view = [x y z 1] * viewmatrix, indexed m[0]x + m[4]y + m[8]z + m[12] (auxiliary.h:58-77);
 *   - a NULL optional pointer means "not provided", like the reference's empty tensors
 *     (DGR forward.cu:209,245; backward.cu:400,404);
 *   - every function returns 0 on success and a negative gsr_status on failure;
 *     gsr_last_error() returns a thread-local message for the last failure on this thread;
 *   - the library owns no device memory: workspaces are sized by the gsr_*_bytes queries, allocated by the
 *     caller (PyTorch's caching allocator) and passed in.  All workspace pointers must be 256-byte aligned.
 *     State it does keep, none of it observable through results: per host thread and device one 64-byte pinned,
 *     device-mapped word block (the read-back of num_rendered; a flag "the last backward met a group of very large
 *     splats", which only selects between two launch plans that produce the same bits) and one event, created on
 *     first use and released when the thread exits; the last-error string (thread-local); the optional profiler's event list
 *     (process-wide, mutex-guarded, only between gsr_profile_begin / _end).  Entry points are re-entrant.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream, which is what the reference
 *     launches on).  debug != 0 synchronises and checks for errors after every stage, the
 *     semantics of the reference's CHECK_CUDA (auxiliary.h:166-173).
 */
#ifndef GSRASTER_H_INCLUDED
#define GSRASTER_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gsr_status {
    GSR_OK = 0,
    GSR_ERR_INVALID_ARGUMENT = -1,
    GSR_ERR_HIP = -2,          /* a HIP runtime call or kernel launch failed */
    GSR_ERR_UNSUPPORTED = -3,  /* e.g. more tiles than the binning kernels support */
    GSR_ERR_NO_DEVICE = -4,
    GSR_NEED_CAPACITY = 1      /* gsr_forward only: the binning workspace was too small, see there */
} gsr_status;

/* Result of forward stage 1, written to host memory (pinned memory avoids a staging copy). */
typedef struct gsr_stage1_result {
    int32_t num_rendered;  /* R: number of binned (Gaussian, tile) instances.  With tile culling disabled this
                              is the reference's return value of Rasterizer::forward (rasterizer_impl.cu:346) */
    int32_t max_tile_count; /* longest per-tile list; selects the per-tile sort variant */
    int32_t num_slots;      /* number of gradient slots the backward scratch must hold: one per BINNED instance, i.e.
                               equal to num_rendered (tiles the cull or the occlusion cut-off dropped own no slot) */
    int32_t num_occluded;   /* instances the conservative occlusion cut-off removed before binning (gsr_tuning.occlusion_cut;
                               0 when it is off): lets the caller judge whether the pass pays on this kind of frame */
} gsr_stage1_result;

/* Tunables; zero-initialise for defaults.  Pure performance knobs: images, radii and gradients do not
 * depend on them. */
typedef struct gsr_tuning {
    int32_t disable_tile_cull; /* 1 = bin every tile of the rectangle like the reference (the internal per-tile
                                  lists and num_rendered become bit-identical to the reference's; slower).
                                  Default 0: skip tiles the Gaussian cannot change (gsr_math.h) */
    int32_t disable_speculation; /* host-side hint (the library ignores it): 1 = the binding should always use the
                                  two-stage forward instead of gsr_forward */
    int32_t disable_partial_sort; /* 1 = sort every per-tile list completely, like the reference.  Default 0: lists longer
                                  than 2048 entries are put in depth order only for their nearest <= 2048 instances first
                                  (the blend stops where the tile's pixels saturate); a tile whose pixels are still
                                  blending at the end of that prefix is sorted completely and blended again */
    int32_t inference; /* 1 = no backward will follow this forward (render under no_grad, the reference's eval loops
                                  train.py:756-763,861-878): the forward writes no depth checkpoints, contributor counts,
                                  per-tile traversal depths or gradient-slot offsets and clears no slot flags.  Images and
                                  radii are bit-identical to the training forward; gsr_backward on that state is undefined */
    int32_t scatter_bands; /* 0 = automatic.  n > 0 forces the scatter launch to n bands of tile rows per chunk (binning.hip: large images /
                                  instance counts stage their keys per band so that they leave in runs; a test / tuning knob) */
    int32_t occlusion_cut; /* 1 = conservative per-tile occlusion cut-off in front of the binning (frames of large splats: lists of
                                  thousands of instances of which the blend walks a tenth).  Every (Gaussian, tile) instance that covers
                                  its whole tile with alpha >= 1/255 adds -log2(1 - its smallest alpha in the tile) to a fixed-point sum per
                                  (tile, depth bucket; 16 buckets per octave of view depth); behind the bucket at which a tile's sum says
                                  "every pixel's transmittance is below 1e-4" nothing can blend (DGR forward.cu:537), and those instances
                                  are never binned.  Images, radii, gradients unchanged bit for bit; num_rendered and the lists shrink */
    int32_t heavy_groups; /* per-Gaussian backward, groups of 64 Gaussians with more than 1024 gradient slots (large splats).  0 = automatic:
                                  a second, cooperative kernel takes them when the caller's previous backwards met enough of them to pay for
                                  its launch; 1 = always launch it, 2 = never (the one-wave kernel does them).  Same bits in every mode */
    int32_t walk_depths_valid; /* see walk_depths: 1 = the array holds a previous visit's depths (order by them), 0 = only record */
    uint64_t walk_depths; /* device address of 4 * ceil(W/16) * ceil(H/16) uint32 the caller keeps PER VIEW (camera), or 0.  The forward's
                                  launch lasts as long as its deepest walks, and the ones that start late are what it waits for; how deep a
                                  quadrant walks hardly changes between two visits of one view, and training revisits its views every
                                  epoch.  With this array the forward records the list depth every 8x8 quadrant walked, and -- when
                                  walk_depths_valid says the array holds a previous visit's -- first dispatches its tasks deepest first
                                  (forward blend -7 % config 2, -11 % config 3, -16 % on GScream's iteration-0 frame).  Any content is safe:
                                  images and gradients do not depend on it.  The array must not be written by other work while the
                                  forward runs. */
} gsr_tuning;

/* Pipeline stages, for the optional per-stage timing below. */
enum { GSR_STAGE_PREPROCESS = 0, GSR_STAGE_COUNT_SCAN, GSR_STAGE_SCATTER, GSR_STAGE_TILE_SORT, GSR_STAGE_BLEND_FWD,
       GSR_STAGE_BLEND_BWD, GSR_STAGE_GAUSS_BWD, GSR_NUM_STAGES };

typedef struct gsr_profile {
    double total_ms[GSR_NUM_STAGES];   /* sum of HIP-event elapsed times per stage */
    int64_t launches[GSR_NUM_STAGES];  /* number of timed stage invocations */
} gsr_profile;

const char* gsr_version(void);
/* Integer version of this header's binary interface: bumped whenever an entry point's argument list, a struct layout or a
 * workspace size formula changes incompatibly.  Bindings compare it with GSR_ABI_VERSION at load time. */
#define GSR_ABI_VERSION 9
int gsr_abi_version(void);
const char* gsr_last_error(void);
/* Forget what the calling thread's previous calls taught the launch heuristics that learn from feedback (ABI 7): today the partial
 * sort's bet -- after a forward in which a quadrant ran off its tile's partially sorted prefix, the next 64 forwards sort lists of up to
 * 4096 entries completely at once instead of paying a second forward-blend launch (api.hip gsr_partial_bet; no counterpart in the
 * reference, which always sorts everything: rasterizer_impl.cu:300-320).  Results never depend on these heuristics; tests and
 * benchmarks that compare launch patterns call this between cases (gscream_amd.set_tuning does). */
void gsr_adaptive_reset(void);
/* Number of visible HIP devices, or a negative gsr_status. */
int gsr_device_count(void);

/* ---- workspace sizes (replace the obtain()/required<T>() carving of rasterizer_impl.h:21-74) ---- */
size_t gsr_geom_bytes(int P);                 /* per-Gaussian state kept from forward to backward   */
size_t gsr_image_bytes(int P, int W, int H);  /* per-pixel / per-tile state kept forward -> backward (16 B + 192 B of
                                                 depth checkpoints per pixel, of which only the reached ones are touched;
                                                 + 5 KiB per tile, up to 8192 tiles, for the occlusion cut-off's mass tables,
                                                 touched only when gsr_tuning.occlusion_cut is set) */
size_t gsr_binning_bytes(int R);              /* per-instance state: sorted point list (+ sort keys)  */
size_t gsr_backward_scratch_bytes(int P, int num_slots); /* per-instance gradient slots + the heavy-group list of the per-Gaussian backward */

/* ---- what is where in those four workspaces (ABI 9): for tests and debugging tools that decode a forward's state (gscream_amd/_layout.py).
 * The library answers from the very walk that carves the caller's pointer, run without one, and from its own compiled constants:
 * a build with other internal values is decoded by what it says.  Host-only: no stream, no device needed.
 * gsr_workspace_layout writes the first `capacity` pieces of workspace `which` (sized like its gsr_*_bytes query: geometry P; image P, W, H;
 * binning R; backward scratch P and R = num_slots; the other arguments are ignored) to out_host, in carving order, and returns how many
 * pieces there are, whatever the capacity (out_host may be NULL with capacity 0), or a negative gsr_status.  Pieces do not overlap,
 * except that the image's `ckpt` and `occ_mass` share one area (the masses are dead before the checkpoints are written). */
enum { GSR_LAYOUT_GEOM = 0, GSR_LAYOUT_IMAGE, GSR_LAYOUT_BINNING, GSR_LAYOUT_BACKWARD_SCRATCH };
typedef struct gsr_layout_piece {
    const char* name; /* the array's name inside the library (a string the library owns) */
    size_t offset;    /* bytes from the workspace's start */
    size_t count;     /* elements */
    size_t elem_size; /* bytes per element */
} gsr_layout_piece;
int gsr_workspace_layout(int which, int P, int W, int H, int R, gsr_layout_piece* out_host, int capacity);
/* Depth segments per tile in the first tier / behind it / in all (= checkpoint slots of `ckpt`), and consecutive tiles an XCD is dealt at
 * a time; gsr_layout_constant returns the value, or a negative gsr_status for an unknown `which`. */
enum { GSR_CONSTANT_SEG1 = 0, GSR_CONSTANT_SEG2, GSR_CONSTANT_SEG_MAX, GSR_CONSTANT_XCD_CHUNK };
int gsr_layout_constant(int which);
int gsr_layout_ckpt_pos(int k, int L);            /* list position of checkpoint k = 0 .. SEG_MAX - 2 at segment length L (64 up to 4096 tiles, 128 beyond) */
int gsr_layout_num_chunks(int P);                 /* rows of the image's (chunk, tile) count table for P Gaussians (one row when the tiles outgrow the LDS histogram) */
int gsr_layout_xcd_tiles(int T);                  /* tile slots per XCD */
int gsr_layout_xcd_tile(int xcd, int i, int T);   /* the i-th tile of XCD `xcd`, -1 = none */

/*
 * Forward, stage 1 of 2: per-Gaussian preprocess + tile histogram + scans.
 * Replaces FORWARD::preprocess, cub::DeviceScan::InclusiveSum and the 4-byte D2H read of
 * num_rendered in CudaRasterizer::Rasterizer::forward (DGR rasterizer_impl.cu:252-287).
 *   means3D[P,3] opacities[P] features[P] (GScream's per-Gaussian `uncertainty`)
 *   scales[P,3]+rotations[P,4]  XOR  cov3D_precomp[P,6]
 *   colors_precomp[P,3]         XOR  shs[P,M,3] with degree D (campos[3] needed for SH)
 * Outputs: radii[P] (int32; 0 = culled), *result_host.  The call synchronises `stream` once,
 * like the reference's blocking cudaMemcpy (rasterizer_impl.cu:287).
 * prefiltered: the caller's promise that no point fails the near-plane test.  The reference traps the kernel on a
 * violation (auxiliary.h:154-162); here, with prefiltered != 0 AND debug != 0, the entry points that take the flag
 * (stage 1, gsr_forward, gsr_filter) check the promise first and fail with GSR_ERR_INVALID_ARGUMENT and the
 * reference's message; without debug the flag is ignored (culled points are culled).
 */
int gsr_forward_stage1(int P, int D, int M, int W, int H,
                       const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                       const float* opacities, const float* features, const float* shs,
                       const float* cov3D_precomp, const float* colors_precomp,
                       const float* viewmatrix, const float* projmatrix, const float* campos,
                       float tan_fovx, float tan_fovy, int prefiltered,
                       void* geom, void* image, int32_t* radii, gsr_stage1_result* result_host,
                       const gsr_tuning* tuning, int debug, void* stream);

/*
 * Forward, stage 2 of 2: instance scatter into per-tile segments, per-tile depth sort, blend.
 * Replaces duplicateWithKeys, cub::DeviceRadixSort::SortPairs, identifyTileRanges and
 * FORWARD::render (DGR rasterizer_impl.cu:295-344).  `binning` must hold gsr_binning_bytes(R).
 * Outputs (every pixel is written): out_color[3,H,W], out_depth[1,H,W], out_feature[1,H,W].
 */
int gsr_forward_stage2(int P, int W, int H, int R, int max_tile_count, const float* background,
                       void* geom, void* image, void* binning,
                       float* out_color, float* out_depth, float* out_feature,
                       const gsr_tuning* tuning, int debug, void* stream);

/*
 * Forward in ONE call, without the GPU-idle window of the two-stage form.  The caller passes a binning workspace
 * sized for `binning_capacity` instances (gsr_binning_bytes(binning_capacity); e.g. 1.25 x the previous frame's
 * num_rendered).  Stage 2 is enqueued before the host waits for num_rendered, so the device never waits for the
 * host.  `max_tile_count_hint` (> 0) bounds the longest per-tile list the caller expects: only the sort variants
 * needed for it are launched; <= 0 launches all of them.  Returns GSR_OK when num_rendered <= binning_capacity and
 * max_tile_count <= hint (outputs valid; keep `binning_capacity` for gsr_backward).  Returns GSR_NEED_CAPACITY (> 0)
 * otherwise: nothing was written out of bounds, but the images are invalid -- allocate
 * gsr_binning_bytes(result_host->num_rendered) and call gsr_forward_stage2 to redo stage 2.
 * (Performance only: the instance scatter sizes its staging -- and decides whether to split its launch into bands of tile
 * rows -- for 0.8 x binning_capacity instances, i.e. it assumes the provision carries the 25 % of slack suggested above.)
 */
int gsr_forward(int P, int D, int M, int W, int H,
                const float* means3D, const float* scales, float scale_modifier, const float* rotations,
                const float* opacities, const float* features, const float* shs,
                const float* cov3D_precomp, const float* colors_precomp,
                const float* viewmatrix, const float* projmatrix, const float* campos,
                float tan_fovx, float tan_fovy, int prefiltered, const float* background,
                void* geom, void* image, void* binning, int binning_capacity, int max_tile_count_hint, int32_t* radii,
                float* out_color, float* out_depth, float* out_feature, gsr_stage1_result* result_host,
                const gsr_tuning* tuning, int debug, void* stream);

/*
 * Backward.  Replaces CudaRasterizer::Rasterizer::backward (DGR rasterizer_impl.cu:536-643):
 * BACKWARD::render + computeCov2DCUDA + preprocessCUDA(bwd).  geom/image/binning are the buffers
 * the forward filled.  Every output row is written (culled Gaussians get exact zeros), so the
 * caller need not zero-fill.  Optional outputs may be NULL: dL_dcov3D[P,6], dL_dsh[P,M,3].
 *   dL_dmeans2D[P,3] (z = 0)  dL_dcolors[P,3]  dL_dopacity[P]  dL_dfeatures[P]
 *   dL_dmeans3D[P,3]  dL_dscales[P,3]  dL_drotations[P,4]
 * dL_dout_depth and dL_dout_feature may each be NULL (= no gradient flows into that map; with both NULL a
 * cheaper kernel variant runs).  No floating-point atomics on global memory are used.
 * The image workspace (backward task list) and the binning workspace (one "slot written" byte per instance: cleared
 * by the forward, set by the blend -- to the same set on every backward of one forward state) are used as scratch
 * during the call, so the backward may run again on the same forward state; two backward calls on ONE forward state
 * must not overlap on different streams.
 */
int gsr_backward(int P, int D, int M, int W, int H, int R, int binning_capacity /* what the forward's binning
                 workspace was sized for; = R after the two-stage forward */,
                 int max_tile_count /* gsr_stage1_result.max_tile_count of THAT forward (its longest per-tile list), or <= 0 if the
                 caller did not keep it: the grid of depth-segment tasks covers the segments of lists up to that length (workgroups
                 of segments no list reaches would only be dispatched to leave at once); unknown = the full grid, same results.  A
                 SMALLER figure than the true one is safe: the grid's last segment takes the rest of every list, so longer lists are
                 still traversed completely, by one longer task -- the figure is a performance hint, not a bound */,
                 const float* background,
                 const float* means3D, const int32_t* radii, const float* colors_precomp, const float* shs,
                 const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                 const float* viewmatrix, const float* projmatrix, const float* campos,
                 float tan_fovx, float tan_fovy,
                 const float* dL_dout_color, const float* dL_dout_depth, const float* dL_dout_feature,
                 const void* geom, void* image /* scratch: the task list */, void* binning /* scratch: the slot flags */, void* scratch,
                 float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dfeatures,
                 float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                 const gsr_tuning* tuning, int debug, void* stream);

/*
 * Visibility filters on a point cloud (GScream calls them on the anchors every iteration,
 * train.py:433).  Replaces Rasterizer::visible_filter (px = py = NULL) and
 * Rasterizer::position2D_filter (DGR rasterizer_impl.cu:350-406, :470-530).  No workspace.
 * radii[P]; px[P], py[P] = pixel-space centre, 0 when culled (forward.cu:378-379).
 */
int gsr_filter(int P, int W, int H, const float* means3D, const float* scales, float scale_modifier,
               const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
               const float* projmatrix, float tan_fovx, float tan_fovy, int prefiltered,
               int32_t* radii, float* px, float* py, int debug, void* stream);

/* Replaces Rasterizer::markVisible (DGR rasterizer_impl.cu:141-153): present[i] = view-space z > 0.2. */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream);

/*
 * ---- fused neural-Gaussian decode + compaction, the step right before the rasterizer ----------
 * Replaces the body of gaussian_renderer/__init__.py:18-102 generate_neural_gaussians after the visible-anchor
 * gather: view vector/distance, the four MLPs 36->32->{K, K, 3K, 7K} (scene/gaussian_model.py:118-144: opacity+Tanh,
 * uncertainty+Sigmoid, color+Sigmoid, cov linear), the opacity>0 mask, the boolean-mask compaction and the
 * post-processing.  N anchors, K = n_offsets <= 10, feat_dim = 32.  All pointers are device pointers, fp32
 * contiguous: feat[N,32], anchor[N,3], offsets[N,K,3], grid_scaling[N,6] (= exp(_scaling)), campos[3].
 * weights[16] = { w1[4], b1[4], w2[4], b2[4] } for the MLPs {opacity, uncertainty, color, cov} (torch Linear layout).
 * visible (optional): int32[N] rows of the model-sized tensors to decode -- the visible-anchor gather (:25-28) folded
 * in; NULL = rows 0..N-1.  With `visible`, feat/anchor/offsets/grid_scaling and the four d_* outputs are MODEL-sized
 * (the backward writes the visible rows only: pre-zero them, or let
 * gsr_decode_zero_hidden_rows fill the others).
 * visible_count (optional, with `visible`): device word holding how many entries of `visible` are valid, read by the kernels
 * instead of being passed by the host (N is then the upper bound everything was sized for); with gsr_decode_visible_rows, which
 * compacts a boolean mask into that row list + count on the device, a training iteration needs no host round trip for the
 * visible-anchor gather (the reference's x[visible_mask] synchronises; so does torch.nonzero).
 *   gsr_decode_visible_rows : rows[<= N] = ascending indices of the set bytes of visible_mask[N], count[1]; block_scratch: ceil(N/256) u32
 *   gsr_decode_count : neural_opacity[N*K], mask[N*K] (u8), count[N] (u8), first[N] (u32, exclusive scan), total[1] (u32);
 *                      block_scratch: ceil(N/256) u32 of scratch
 *   gsr_decode_emit  : the total[0] surviving rows, in boolean-mask order: xyz[M,3], color[M,3], opacity[M], uncertainty[M],
 *                      scaling[M,3], rot[M,4]
 *   gsr_decode_backward : upstream gradients of those rows (each of the six may be NULL = no gradient flows into that
 *                      output: read as zeros) -> d_feat[N,32], d_anchor[N,3], d_offsets[N,K,3],
 *                      d_grid_scaling[N,6] AND the 16 weight / bias gradients grads16 = { gw1[4] [32,36], gb1[4] [32],
 *                      gw2[4] [out,32], gb2[4] [out] } in the order of `weights` (every element written; bit-reproducible),
 *                      in one pass on the f32 matrix cores; workspace of gsr_decode_weight_grad_workspace_bytes() bytes
 *                      (workgroup partials, nothing to initialise).  Replaces the autograd backward of
 *                      generate_neural_gaussians including the reference's nn.Linear layers (scene/gaussian_model.py:118-144).
 */
int gsr_decode_visible_rows(int N, const uint8_t* visible_mask, int32_t* rows, uint32_t* count, uint32_t* block_scratch, void* stream);
int gsr_decode_count(int N, int K, const float* const* weights, const int32_t* visible, const uint32_t* visible_count, const float* feat, const float* anchor, const float* campos,
                     float* neural_opacity, uint8_t* mask, uint8_t* count, uint32_t* first, uint32_t* total,
                     uint32_t* block_scratch, void* stream);
int gsr_decode_emit(int N, int K, const float* const* weights, const int32_t* visible, const uint32_t* visible_count, const float* feat, const float* anchor, const float* offsets,
                    const float* grid_scaling, const float* campos, const float* neural_opacity /* from gsr_decode_count */,
                    const uint8_t* mask, const uint32_t* first, float* xyz,
                    float* color, float* opacity, float* uncertainty, float* scaling, float* rot, void* stream);
int gsr_decode_backward(int N, int K, const float* const* weights, const int32_t* visible, const float* feat, const float* anchor,
                        const float* offsets, const float* grid_scaling, const float* campos, const uint8_t* mask,
                        const uint32_t* first, const float* g_xyz, const float* g_color, const float* g_opacity,
                        const float* g_uncertainty, const float* g_scaling, const float* g_rot, float* d_feat, float* d_anchor,
                        float* d_offsets, float* d_grid_scaling, void* workspace, float* const* grads16, void* stream);
size_t gsr_decode_weight_grad_workspace_bytes(void);
/* With `visible`, gsr_decode_backward writes the visible rows of the model-sized d_* tensors only.  This fills the OTHER rows
 * (visible_mask[r] == 0, one byte per model row: the boolean mask the row list was made from) with zeros, so that the caller
 * can hand in uninitialised tensors instead of zero-filling all N rows.  N = model rows here. */
int gsr_decode_zero_hidden_rows(int N, int K, const uint8_t* visible_mask, float* d_feat, float* d_anchor, float* d_offsets,
                                float* d_grid_scaling, void* stream);

/*
 * Densification statistics of one training iteration: replaces the body of
 * GaussianModel.training_statis (scene/gaussian_model.py:730-757).  Nv visible anchors, K offsets each.
 * visible[Nv] (int32 rows of the model, NULL = identity), neural_opacity[Nv*K], selection[Nv*K] (u8, the decode's
 * mask), first[Nv] (u32, first output row of each anchor: gsr_decode_count), update_filter[M] (u8: radii > 0 of the
 * decoded Gaussians), viewspace_grad[M,3] (gradient of the screen-space means).  Accumulates IN PLACE into the
 * model-sized opacity_accum[N], anchor_demon[N], offset_gradient_accum[N*K], offset_denom[N*K] (fp32).
 */
int gsr_training_stats(int Nv, int K, int M, const int32_t* visible, const float* neural_opacity, const uint8_t* selection,
                       const uint32_t* first, const uint8_t* update_filter, const float* viewspace_grad,
                       float* opacity_accum, float* anchor_demon, float* offset_gradient_accum, float* offset_denom,
                       void* stream);

/*
 * Anchor growing, one level (the tensor math of GaussianModel.anchor_growing, scene/gaussian_model.py:834-874): quantise the
 * candidates all_xyz = anchor + offset * scaling[:, :3] (:829) to cells round(xyz / cur_size) (:840-841), keep one per cell
 * in ascending (x, y, z) order (torch.unique(dim=0), :843), drop cells an existing anchor occupies (the chunked U x N test
 * of :846-857, here a hash table of the N anchor cells), write candidate_anchor = cell * cur_size (:863) and new_feat = the
 * per-channel max of anchor_feat[row / K] over the cell's candidates (scatter_max, :872-874).  Bit-identical, same row order.
 * Two calls around a STABLE sort of the keys done by the caller:
 *   gsr_anchor_grow_keys: anchor[N,3], offset[N,K,3], scaling[N,>=3 of 6] (the ACTIVATED scaling, row stride 6),
 *     candidate_mask[L] (u8, L <= N*K: rows beyond L are not candidates), inv_size = 1.0f / (float)cur_size (PyTorch's GPU
 *     division by a Python scalar multiplies by this reciprocal).  Writes the 63-bit cell keys[M] (int64, 21 bits per axis
 *     biased by 2^20) and flat mask rows rows[M] (int32) of the M candidates in mask order, and info[0] = M,
 *     info[1] = flags: bit 0 a candidate cell outside [-2^20, 2^20) or non-finite, bit 1 a non-finite anchor; with a flag
 *     set the level must be computed another way (the keys do not represent it).  info: int32[4] on the device.
 *   gsr_anchor_grow_emit: sorted_keys[M] and order[M] (int64: the stably sorted keys and their positions in keys[]),
 *     rows[] and the workspace of the keys call, anchor_feat[N,F], cur_size as fp32.  Writes candidate_anchor[C,3],
 *     new_feat[C,F] (buffers sized M) and info[2] = C.
 * workspace: gsr_anchor_grow_workspace_bytes(N, L), the same for both calls.
 */
size_t gsr_anchor_grow_workspace_bytes(int N, int L);
int gsr_anchor_grow_keys(int N, int K, int L, const float* anchor, const float* offset, const float* scaling,
                         const uint8_t* candidate_mask, float inv_size, void* workspace, int64_t* keys, int32_t* rows,
                         int32_t* info, void* stream);
int gsr_anchor_grow_emit(int N, int K, int F, int L, int M, const float* anchor_feat, const int64_t* sorted_keys,
                         const int64_t* order, const int32_t* rows, float cur_size, void* workspace, float* candidate_anchor,
                         float* new_feat, int32_t* info, void* stream);
/*
 * torch_scatter.scatter_max(src, index, dim=0) for fp32 src[R,F] and a row index index[R] (int64; the broadcast form
 * gaussian_model.py:874 uses): out[S,F] = per-channel max over the rows r with index[r] = s, argmax[S,F] = the smallest such
 * r; slots no row reaches hold 0 and argmax R.  Rows whose index is outside [0, S) are ignored.
 */
int gsr_scatter_max(int R, int F, int S, const float* src, const int64_t* index, float* out, int64_t* argmax, void* stream);

/*
 * The attention core of BidirectionalCrossAttention (bidirectional-cross-attention 0.0.4, GaussianModel.run_crossattn,
 * scene/gaussian_model.py:553-583): everything between the input projections and the output projections, for both directions.
 *     sim[b,h,i,j]   = scale * qk[b,i,h,:] . context_qk[b,j,h,:];  a pair with mask[b,i] & context_mask[b,j] false takes -FLT_MAX
 *     out[b,i,h,:]         = sum_j softmax_j(sim) context_v[b,j,h,:]
 *     context_out[b,j,h,:] = sum_i softmax_i(sim) v[b,i,h,:]
 * qk, v, out: [B,I,H,64]; context_qk, context_v, context_out: [B,J,H,64] -- the layout nn.Linear leaves ([b, n, h*d] contiguous),
 * fp32.  mask [B,I], context_mask [B,J]: one byte per entry (torch.bool), NULL = all true.  dim_head must be 64
 * (GSR_ERR_UNSUPPORTED otherwise).  fp32 on the exact f32 matrix cores; no [h,i,j] tensor is written.  The forward leaves each
 * softmax row's (max, 1 / sum) in the workspace (gsr_crossattn_workspace_bytes(B, H, I, J)); the backward takes the same inputs,
 * both outputs (not read at present: the kernels recompute what they need from the inputs and the workspace), the two output
 * gradients and that workspace (it also uses it as scratch) and writes the four input gradients.
 * No atomics: repeated calls give identical bits.
 */
size_t gsr_crossattn_workspace_bytes(int B, int H, int I, int J);
int gsr_crossattn_forward(int B, int H, int I, int J, int dim_head, const float* qk, const float* v, const float* context_qk,
                          const float* context_v, const uint8_t* mask, const uint8_t* context_mask, float scale, float* out,
                          float* context_out, void* workspace, void* stream);
int gsr_crossattn_backward(int B, int H, int I, int J, int dim_head, const float* qk, const float* v, const float* context_qk,
                           const float* context_v, const uint8_t* mask, const uint8_t* context_mask, float scale, const float* out,
                           const float* context_out, const float* d_out, const float* d_context_out, void* workspace, float* d_qk,
                           float* d_v, float* d_context_qk, float* d_context_v, void* stream);

/*
 * The anchor sampler of the cross-attention step (train.py:436-511), without a host stop: from what prefilter_position2D
 * returns (visible[N] one byte per anchor, px[N], py[N] fp32), the view's mask gt_mask[H,W] (fp32) and the patch rectangle, the
 * two anchor sets GaussianModel.run_crossattn pairs up.  Per anchor a, x = px[a], y = py[a]:
 *     valid    visible[a] and 0 < x < W and 0 < y < H  (strict, floating point; NaN is invalid);  pixel (iy, ix) = ((int)y, (int)x)
 *     sampled  valid and min_y <= iy < max_y and min_x <= ix < max_x  (an empty or inverted rectangle samples nothing)
 *     label    (long)gt_mask[iy, ix];  fg: sampled and label > 0;  bg: sampled and label == 0;  a negative label is in neither
 *     ok       n_fg > 11 and n_bg > 11;   min_num = min(n_fg, n_bg, max_pairs)
 *     src / dst  the min_num members of fg / bg with the smallest (key, index): a uniformly random min_num-subset of the class
 * key, modulo 2^32, with s_lo / s_hi the halves of `seed` and i the anchor index:
 *     mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *     key(i) = mix(((mix((i ^ s_lo) + s_hi)) + s_lo) ^ s_hi)        (a bijection of uint32: keys never tie)
 * Writes src_mask[N], dst_mask[N] (one byte per anchor, 0 / 1, every entry), the selected anchor indices in ASCENDING order in
 * src_rows[0:min_num], dst_rows[0:min_num] (the order of feat[mask]; entries from min_num on are left untouched) and
 * info[8] = {n_sampled, n_fg, n_bg, min_num, ok, 0, 0, 0} (int32, on the device).  When ok == 0 the masks are all zero and min_num
 * is still reported.  N == 0 is valid.  Integer atomics only: repeated calls give identical bits.  A fixed number of launches on
 * `stream`, no read-back.  workspace: gsr_anchor_sample_workspace_bytes(N, max_pairs).
 */
size_t gsr_anchor_sample_workspace_bytes(int N, int max_pairs);
int gsr_anchor_sample(int N, int H, int W, const uint8_t* visible, const float* px, const float* py, const float* gt_mask /* [H,W] */,
                      int min_y, int max_y, int min_x, int max_x, int max_pairs, uint64_t seed, void* workspace,
                      uint8_t* src_mask /* [N] */, uint8_t* dst_mask /* [N] */,
                      int64_t* src_rows /* [max_pairs] */, int64_t* dst_rows /* [max_pairs] */,
                      int32_t* info /* [8]: n_sampled, n_fg, n_bg, min_num, ok, 0, 0, 0 */, void* stream);

/*
 * Anchor pruning: GaussianModel.adjust_anchor around its anchor_growing call, with prune_anchor / _prune_anchor_optimizer
 * (scene/gaussian_model.py:914-973, :762-805).  fp32 / integer, no atomics: repeated calls give identical bits.  Python scalars
 * arrive rounded to fp32, which is how torch compares / multiplies a float tensor with them.
 *   gsr_anchor_adjust_offsets (:916-919), over the L0 = N0*K offset rows that exist BEFORE growing:
 *     g = offset_gradient_accum / offset_denom (IEEE fp32 division), NaN -> 0, grads_norm[L0] = |g|,
 *     offset_mask[L0] (one byte, 0 / 1) = offset_denom > denom_threshold  ((float)(check_interval*success_threshold*0.5)).
 *   gsr_anchor_adjust_plan (:937-939), over the N anchors that exist AFTER growing (opacity_accum[N], anchor_demon[N]):
 *     reset = anchor_demon > demon_threshold  ((float)(check_interval*success_threshold));
 *     prune = reset and opacity_accum < anchor_demon * min_opacity  (one fp32 product).
 *     With prune_mask[N] (one byte per anchor) given, prune is that mask and reset is all zero (the standalone prune_anchor;
 *     opacity_accum / anchor_demon may then be NULL).
 *     Writes keep_rows[0:n_keep] (int32, the kept anchors in ASCENDING order; buffer of N entries, the rest untouched), reset[N]
 *     (one byte, 0 / 1) and info[4] = {n_keep, n_prune, n_reset, 0} (int32, on the device).  A fixed number of launches, no
 *     read-back.  N == 0 is valid.  workspace: gsr_anchor_adjust_workspace_bytes(N).
 *   gsr_anchor_adjust_gather: ONE launch moves the kept rows of up to GSR_ADJUST_MAX_COPIES tensors.  `copies` is a HOST array; it
 *     travels in the kernel arguments (no host-to-device copy).  Copy c treats dst as a flat stream of n_keep * width floats:
 *     element e -> row = e / width, col = e % width, a = keep_rows[row], s = a * width + col, and by mode
 *       GSR_ADJUST_COPY         dst[e] = src[s]                                   bit for bit (NaN, -0.0)
 *       GSR_ADJUST_CLAMP_TAIL   col >= 3: v > 0.05f ? 0.05f : v (NaN stays), else COPY     the `scaling` parameter (:776-780), not its moments
 *       GSR_ADJUST_OFFSET_STAT  width K: (s < L0 && !offset_mask[s]) ? src[s] : +0.0f      the resets :924/:930, the zero padding
 *                               :925-934 and the gather :942-950 of offset_denom / offset_gradient_accum; src has L0 entries
 *                               and is never read beyond them
 *       GSR_ADJUST_ANCHOR_STAT  width 1: reset[a] ? +0.0f : src[s]                         :953-956 with :958-968
 *     COPY / CLAMP_TAIL rows move in units of 16 or 8 bytes where the width is a multiple of 4 or 2 floats and both pointers are
 *     aligned to the unit (checked per copy on the host), else float by float; any alignment of 4 is accepted.
 *     N is the row count of the sources (keep_rows[] < N; N * width < 2^31 for every copy), n_keep the host's copy of info[0].
 */
#define GSR_ADJUST_MAX_COPIES 32
enum { GSR_ADJUST_COPY = 0, GSR_ADJUST_CLAMP_TAIL = 1, GSR_ADJUST_OFFSET_STAT = 2, GSR_ADJUST_ANCHOR_STAT = 3 };
typedef struct gsr_adjust_copy {
    const float* src;
    float* dst;
    int32_t width; /* floats per anchor row */
    int32_t mode;  /* GSR_ADJUST_* */
} gsr_adjust_copy;
size_t gsr_anchor_adjust_workspace_bytes(int N);
int gsr_anchor_adjust_offsets(int L0, const float* offset_gradient_accum, const float* offset_denom, float denom_threshold,
                              float* grads_norm, uint8_t* offset_mask, void* stream);
int gsr_anchor_adjust_plan(int N, const float* opacity_accum, const float* anchor_demon, const uint8_t* prune_mask /* or NULL */,
                           float min_opacity, float demon_threshold, void* workspace, int32_t* keep_rows /* [N] */,
                           uint8_t* reset /* [N] */, int32_t* info /* [4]: n_keep, n_prune, n_reset, 0 */, void* stream);
int gsr_anchor_adjust_gather(int N, int n_keep, int n_copies, const gsr_adjust_copy* copies /* host */, const int32_t* keep_rows,
                             const uint8_t* offset_mask /* [L0] */, int L0, const uint8_t* reset /* [N] */, void* stream);

/*
 * The optimiser step: gaussians.optimizer.step() (train.py:611, :615), Adam without amsgrad / weight decay, for up to
 * GSR_ADAM_MAX_TENSORS tensors of any parameter groups in ONE launch.  `tensors` is a HOST array; it travels in the kernel
 * arguments (no host-to-device copy).  Per element, fp32, one rounding per operation (nothing contracts into an FMA), in the order of
 * torch 1.12's mul_().add_(alpha=), mul_().addcmul_(value=), sqrt()/bias_correction2_sqrt .add_(eps), addcdiv_(value=):
 *     m' = m*b1 + g*c1                 b1 = (float)beta1, c1 = (float)(1 - beta1)
 *     v' = v*b2 + (c2*g)*g             b2 = (float)beta2, c2 = (float)(1 - beta2)
 *     d  = sqrt(v') / s2 + e           s2 = (float)sqrt(1 - beta2^t), e = (float)eps
 *     p' = p + (a*m') / d              a  = (float)(-(lr / (1 - beta1^t)))
 * sqrt and both divisions are the correctly rounded ones; fp32 denormals are kept.  The caller computes each scalar in double from
 * the group's lr, betas, eps and the parameter's own step count t (after its increment) and rounds it once to fp32, which is how
 * torch passes Python scalars to its kernels.  p, m and v are updated in place; g is read only.  Tensors whose four pointers are all
 * 16-byte aligned move in 16-byte units (the n % 4 floats behind them singly), others float by float; any alignment of 4 is accepted.
 * No atomics: repeated calls give identical bits.  n_tensors == 0 and tensors with n == 0 (whose pointers may be NULL) do nothing.
 */
#define GSR_ADAM_MAX_TENSORS 32
typedef struct gsr_adam_tensor {
    float* p;       /* [n] parameter, in place */
    const float* g; /* [n] gradient */
    float* m;       /* [n] exp_avg, in place */
    float* v;       /* [n] exp_avg_sq, in place */
    int32_t n;      /* elements, 0 <= n < 2^31 */
    float b1, c1, b2, c2, s2, e, a;
} gsr_adam_tensor;
int gsr_adam_step(int n_tensors, const gsr_adam_tensor* tensors /* host */, void* stream /* hipStream_t */);

/*
 * Normals from rendered depth: the two functions render_set applies to every frame of the RGBD video (train.py:820-821).
 *
 * gsr_depth_points: depth2pcd_fromplane (train.py:252-267).  depth [H,W], K [3,3] and c2w [3,4] are fp32 DEVICE pointers (the caller
 * holds K and c2w as tensors; nothing is read back); points is [3,H,W] fp32.  Per pixel (i, j), fp32, one rounding per operation,
 * nothing contracts into an FMA:
 *     xn = (j - K[0][2]) / K[0][0]     yn = (i - K[1][2]) / K[1][1]          (IEEE division)
 *     xc = xn*d   yc = yn*d   zc = d
 *     P[r] = ((c2w[r][0]*xc + c2w[r][1]*yc) + c2w[r][2]*zc) + c2w[r][3]      (summed left to right)
 *
 * gsr_point_normals: least_square_normal_regress_fast01 (train.py:270-298).  points [3,H,W] fp32 -> normals [H*W,3] fp32, row-major by
 * pixel.  size is odd, 1 .. 15 (the reference uses 9); no workspace.  Per pixel with centre c and the size*size window points q taken
 * with replicate padding (indices clamped to the image, which may be smaller than the window), rows then columns:
 *     mask    q := (0,0,0)  iff  fabsf((q.z - c.z) / c.z) > gamma  in fp32, one rounding per operation: the reference's decision bit
 *             for bit (only z decides; a NaN quotient keeps the point, an infinite one drops it; a zeroed point still counts as a row)
 *     sums    A = sum q q^T (six entries) and s = sum q, accumulated in fp64 in window order
 *     solve   det(A) in fp64 (Gaussian elimination with partial pivoting: the signed product of the pivots);  det < eps -> v = s (the
 *             reference substitutes the identity), otherwise v = A^-1 s from the same elimination, fp64
 *     output  v / max(|v|_2, 1e-12), a NaN component becomes 0, negated, rounded to fp32 once
 * Both launch on `stream`, never synchronise and read nothing back; repeated calls give identical bits.  Rejected before launching
 * (GSR_ERR_INVALID_ARGUMENT, text in gsr_last_error): NULL pointers, H or W <= 0, H*W >= 2^31 - 256, an even size or one outside 1 .. 15.
 */
int gsr_depth_points(int H, int W, const float* depth, const float* K /* [3,3] device */, const float* c2w /* [3,4] device */,
                     float* points /* [3,H,W] */, void* stream /* hipStream_t */);
int gsr_point_normals(int H, int W, const float* points /* [3,H,W] */, int size, float gamma, double eps, float* normals /* [H*W,3] */,
                      void* stream /* hipStream_t */);

/*
 * Test-view metrics: what evaluate() (train.py:905-990) and training_report (train.py:655-708) log per view -- L1, MSE, PSNR
 * (utils/image_utils.py:22-32) and my_ssim (utils/loss_utils.py:123-128) -- over the whole image and over a boolean mask, for a
 * batch of images in one call.  pred and gt are fp32 [B,C,H,W]; mask is NULL or bytes (0 = false) read through
 * mask + b*mask_stride_b + c*mask_stride_c + i*W + j, so mask_stride_c = 0 is a channel-broadcast mask (evaluate()'s expand) and
 * mask_stride_b = 0 one mask for the whole batch.  H, W >= 3 is what reflect padding of 2 needs.
 *
 *   input transform, per element, fp32, one rounding per operation, no contraction:
 *       flag CLAMP     x := min(max(x, 0), 1)                                  (training_report's torch.clamp; NaN stays NaN)
 *       flag QUANTIZE  x := trunc(min(max(x*255 + 0.5, 0), 255)) / 255         (torchvision save_image, then to_tensor: evaluate()'s PNG round trip)
 *                      applied to pred and gt alike; implies nothing else (with both flags: CLAMP, then QUANTIZE)
 *   d      = x - y                                            fp32 (exact once widened)
 *   window g_k = exp(-(k-2)^2 / 4.5) / sum_k(...)  k = 0..4, evaluated in fp64; w_ij = g_i g_j
 *   pad    reflect without repeating the edge: index -1 -> 1, -2 -> 2, H -> H-2, H+1 -> H-3 (torch 'reflect', scipy 'mirror')
 *   mu1 = w*x   mu2 = w*y   e11 = w*(x x)   e22 = w*(y y)   e12 = w*(x y)          fp64 (products of fp32 values are exact in fp64)
 *   s1 = e11 - mu1^2   s2 = e22 - mu2^2   s12 = e12 - mu1 mu2
 *   ssim  = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2) + 1e-12)      C1 = 1e-4, C2 = 9e-4
 *   dssim = min(max((1 - ssim)/2, 0), 1)
 *   per image b, over all C*H*W elements, and over the elements where the mask is true:
 *       sums[b] = { n, sum|d|, sum d^2, sum dssim,  n_m, sum_m|d|, sum_m d^2, sum_m dssim }     fp64; n and n_m are exact integers
 *       metrics[b] = { l1, mse, psnr, ssim, l1_m, mse_m, psnr_m, ssim_m }                        each formed in fp64, rounded to fp32 once
 *       l1 = sum|d| / n     mse = sum d^2 / n     psnr = -10 log10(mse)     ssim = 1 - 2 (sum dssim / n)
 *
 * An empty mask gives NaN in the four masked entries (0/0, as torch.mean of an empty selection) and leaves the unmasked ones alone;
 * mse == 0 gives psnr = +inf; a NaN pixel makes that image's affected entries NaN (the mask selects, it does not multiply: a NaN
 * outside the mask reaches the masked entries only through the 5x5 windows that hold it) and touches no other image of the batch;
 * without a mask the four masked entries equal the unmasked ones.  The window sums are separable (rows, then columns), every sum is
 * taken in a fixed order without atomics: the same inputs give the same bits.
 *
 * The PSNR half is pinned by a run of the reference's utils/image_utils.py (tests/golden/ref_metrics.npz).  The SSIM half is NOT pinned
 * by a reference run: the expression is kornia 0.6.12's metrics.ssim(img1, img2, 5, 1.0, 1e-12, 'same') with filter2d's default reflect
 * border, as utils/my_ssim.py calls it, written down from its source; the reference evaluates it (and E[x^2] - mu^2 in it) in fp32,
 * this call in fp64, and returns the value the expression defines (INTEGRATION R has the measured gap).
 *
 * workspace: gsr_image_metrics_workspace_bytes(B, C, H, W) bytes (0 for sizes the call rejects), written before it is read.  The call
 * launches on `stream`, never synchronises and reads nothing back.  Rejected before launching (GSR_ERR_INVALID_ARGUMENT, text in
 * gsr_last_error): NULL pred, gt, workspace, sums or metrics; B or C <= 0 or B*C > 65535; H or W < 3; C*H*W >= 2^31 - 256; unknown
 * flag bits; negative mask strides.
 */
#define GSR_METRICS_CLAMP    1
#define GSR_METRICS_QUANTIZE 2
size_t gsr_image_metrics_workspace_bytes(int B, int C, int H, int W);
int gsr_image_metrics(int B, int C, int H, int W, const float* pred, const float* gt,
                      const uint8_t* mask /* or NULL */, long long mask_stride_b, long long mask_stride_c,
                      int flags, void* workspace, double* sums /* [B,8] */, float* metrics /* [B,8] */, void* stream /* hipStream_t */);

/*
 * LPIPS: the third metric evaluate() (train.py:905-987) reports per view, plain (lpips_fn, :948) and masked (the mean of
 * loss_fn_vgg_spatial's map under the mask, :952-953), from ONE VGG-16 pass over the pair.  This is LPIPS v0.1, net = 'vgg',
 * lpips = True, eval mode.  in0, in1 are fp32 [B,3,H,W] with H, W >= 16, nominally in [-1, 1].
 *
 *   flag NORMALIZE (the package's normalize=True; evaluate() writes 2*x-1 itself):  x := 2x - 1              one fp32 rounding
 *   scaling layer   x := (x - shift[c]) / scale[c]    shift = (-.030, -.088, -.188)  scale = (.458, .448, .450)
 *                   one fp32 subtraction and one IEEE fp32 division.  The zero padding of the first convolution is applied AFTER
 *                   this step: a border tap contributes 0, not (0 - shift) / scale.
 *   features        13 convolutions, 3x3, stride 1, zero pad 1, bias, ReLU, of widths
 *                       3->64, 64->64 | 64->128, 128->128 | 128->256, 256->256, 256->256 | 256->512, 512->512, 512->512 |
 *                       512->512, 512->512, 512->512
 *                   `|` = 2x2 stride-2 max-pool with floor (an odd last row or column is dropped: 567 -> 283 -> 141 -> 70 -> 35).
 *                   The taps f_l, l = 0..4, are the ReLU outputs that end the five groups, C_l = 64, 128, 256, 512, 512.
 *                   Each output element is ONE fp32 fma chain (v_mfma_f32_32x32x2_f32, bit for bit an fmaf chain):
 *                       acc = bias[co];  for chunk = 0 .. ceil(Cin/8)-1:  for ky = 0..2: for kx = 0..2:  for ci = 8 chunk .. 8 chunk + 7:
 *                           acc = fma(w[co][ci][ky][kx], x[ci][y+ky-1][x+kx-1], acc)
 *                   (the bias is the start value of the chain; channels ci >= Cin of the last chunk are fma(0, 0, acc) = acc);
 *                   out = acc < 0 ? 0 : acc.  The order is the same for every element: the same inputs give the same bits.
 *   head, per tap   n = sqrt(sum_c f^2) for both images;  fh = f / (n + 1e-10);  d_c = (fh0_c - fh1_c)^2;
 *                   m_l[y,x] = sum_c lin_l[c] d_c   (the bias-free 1x1 `lin` convolution; dropout is the identity)
 *                   every step in fp64 on the fp32 features, the channel sums in ascending c, no contraction; m_l is stored
 *                   rounded to fp32 once (the spatial map reads that), its fp64 value enters the plain sums
 *   out_layers[b,l] = mean_{y,x} m_l        out_plain[b] = sum_l mean_l       spatial sums and the sum over l in fp64, in a fixed order
 *                   without atomics; each rounded to fp32 once
 *   out_spatial[b,y,x] = sum_l bilinear_l(m_l)[y,x]  at H x W, fp32, one rounding per operation, the taps added in ascending l.
 *                   torch's Upsample(size=(H,W), mode='bilinear', align_corners=False):  scale = in / out;
 *                   src = max(scale (dst + 0.5) - 0.5, 0);  i0 = trunc(src);  i1 = min(i0 + 1, in - 1);  t = src - i0;
 *                   value = (1-ty) ((1-tx) v00 + tx v01) + ty ((1-tx) v10 + tx v11)
 *   out_masked[b]   = the mean of out_spatial[b] over the pixels where mask (bytes, 0 = false, read through
 *                   mask + b*mask_stride_b + y*W + x; stride 0 = one mask for all views; NULL = every pixel) is true; the sum and
 *                   the count in fp64, the quotient rounded to fp32.  An empty mask gives NaN (0/0), as torch's mean does.
 *
 * The rule is pinned AS WRITTEN ABOVE ONLY: neither the lpips package nor torchvision nor any VGG / LPIPS weights are on this
 * stack, so no run of the package stands behind it.  The caller brings the weights:
 *   conv_weights  the 13 layers in order, each packed [Cout/64][ceil(Cin/8)][9 = ky*3+kx][8 = ci % 8][64 = co % 64] with zeros where
 *                 ci >= Cin (14 713 344 floats: the sum over the layers of (Cout/64) * ceil(Cin/8) * 4608)
 *   conv_bias     the 13 biases in order (4224 floats)         lin_weights   the five lin vectors in order (1472 floats)
 * workspace: gsr_lpips_workspace_bytes(B, H, W) bytes (0 for sizes the call rejects; two activation buffers of 2B*64*H*W floats,
 * the five maps and the partial sums), written before it is read.  out_layers [B,5], out_masked [B] and out_spatial [B,H,W] may be
 * NULL.  The call launches on `stream`, never synchronises and reads nothing back.  Rejected before launching
 * (GSR_ERR_INVALID_ARGUMENT, text in gsr_last_error): B outside 1 .. 32767; H or W < 16; H*W >= 2^31 - 256; NULL in0, in1,
 * conv_weights, conv_bias, lin_weights, workspace or out_plain; flag bits other than NORMALIZE; a negative mask stride.
 *
 * gsr_conv3x3_relu is one layer of the chain on its own: in [B,Cin,H,W] -> out [B,Cout,H,W], Cout a multiple of 64, weights packed
 * as above.  flags NORMALIZE and SCALING (Cin = 3 only) apply the two input steps to the pixels inside the image.  Rejected before
 * launching: B outside 1 .. 65535; Cin <= 0; Cout no positive multiple of 64; Cin or Cout > 65536; H or W <= 0; H*W >= 2^31 - 256;
 * a NULL pointer; unknown flag bits; flags with Cin != 3.
 */
#define GSR_LPIPS_NORMALIZE 1
#define GSR_LPIPS_SCALING   2
size_t gsr_lpips_workspace_bytes(int B, int H, int W);
int gsr_lpips(int B, int H, int W, const float* in0 /* [B,3,H,W] */, const float* in1, int flags, const float* conv_weights,
              const float* conv_bias, const float* lin_weights, const uint8_t* mask /* or NULL */, long long mask_stride_b,
              void* workspace, float* out_plain /* [B] */, float* out_layers /* [B,5] or NULL */, float* out_masked /* [B] or NULL */,
              float* out_spatial /* [B,H,W] or NULL */, void* stream /* hipStream_t */);
int gsr_conv3x3_relu(int B, int Cin, int Cout, int H, int W, const float* in, const float* weights_packed, const float* bias,
                     float* out, int flags, void* stream /* hipStream_t */);

/*
 * Output frames: what render_set (train.py:710-848) does between the render and the PNG encoder -- save_image's quantisation, the
 * error map, the normal picture's second normalisation, the least-squares depth alignment of compute_scale_and_shift (:198-218), the
 * two colour maps (cv2.applyColorMap for the spiral video, plt.imsave for the train / test sets), the flips, the one-channel expand
 * and the concat -- as finished uint8 pictures on the device, in HWC order.  Everything per pixel is fp32 with one rounding per
 * operation, nothing contracts into an FMA, division and sqrt are the correctly rounded ones; every rule ends in an integer:
 *
 *   quantise   q(x) = (uint8) trunc(min(max(x*255 + 0.5, 0), 255))          torchvision save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8):
 *              the expression of GSR_METRICS_QUANTIZE.  NaN -> 0: the reference's float -> uint8 conversion of a NaN is unspecified
 *              (it depends on the host), this is a choice.  -0.0 -> 0, +inf -> 255, -inf -> 0.
 *              clamp, where a mode says so, comes first: x := min(max(x, 0), 1), a NaN stays  (render_set's torch.clamp, :766, :771)
 *   abs-diff   e = |clamp(a) - b|, then q(e)                                 the error map, :794
 *   normal     s = (x*x + y*y) + z*z;  r = max(sqrt(s), 1e-12f) (a NaN stays);  c = (v/r + 1) / 2 per component, then q(c)      :823-824
 *   stats      per frame b over its H*W depths d:  lo = min d, hi = max d (a NaN anywhere makes both NaN).  With a target y and an lsq
 *              mask m (fp32, NULL = ones), in fp64, the products m d and m y exact, m d d and m d y rounded once, each sum in a fixed order:
 *                  a00 = sum m d d   a01 = sum m d   a11 = sum m   b0 = sum m d y   b1 = sum m y
 *                  det = a00 a11 - a01 a01;   det == 0 -> x0 = x1 = 0,  else  x0 = (a11 b0 - a01 b1) / det,  x1 = (-a01 b0 + a00 b1) / det
 *              (each product, difference and quotient one fp64 rounding), scale = |(float) x0|, shift = (float) x1.  The mask multiplies
 *              (as the reference's does): a NaN depth under m = 0 still makes the sums NaN.  Then, in a second pass over the frame,
 *              lo2 / hi2 = min / max over the 2 H W values of the panel [aligned | y], aligned = d*scale + shift (two fp32 roundings);
 *              a NaN anywhere in it makes both NaN.  Without a target the five sums, scale, shift, lo2 and hi2 are 0.
 *   CV map     t = (d - lo) / (hi - lo);  i = trunc(min(max(255 t, 0), 255)), NaN -> 0;  RGB = lut[i]          :807-810
 *              hi == lo, or lo or hi not finite -> i = 0 for every pixel (the reference divides 0 by 0 there and converts the NaN
 *              to uint8, which is unspecified: a choice).  With lo / hi the frame's own extrema 255 t lies in [0, 255] without the clamp.
 *   MPL map    v = the value (the target half) or d*scale + shift (the aligned half);  den = (float)((double) hi2 - (double) lo2);
 *              t = (v - lo2) / den;  i = min(max((int) trunc(t * 256), 0), 255);  RGBA = (lut[i], 255)           plt.imsave, :789
 *              hi2 == lo2 -> i = 0;  lo2 or hi2 NaN -> every pixel (0, 0, 0, 0);  a pixel whose t is NaN -> (0, 0, 0, 0).  Pinned by
 *              matplotlib's imsave on finite panels, a constant one and one with a NaN (tests/golden/ref_frames.npz); panels with
 *              infinities are not pinned.
 *
 * gsr_frame_stats: depth, target (or NULL), lsq_mask (or NULL; needs a target) are fp32 [B,H,W].  Block partials (one workgroup per
 * 4096 elements of a frame, eight doubles each), then one workgroup per frame sums them in a fixed order; with a target the same
 * again for lo2 / hi2 once scale and shift exist (they are not derived from lo, hi and the sign of scale: the rounded products
 * decide).  stats[b] = {a00, a01, a11, b0, b1, det, x0, x1} (fp64), params[b] = {lo, hi, scale, shift, lo2, hi2, 0, 0} (fp32).
 * workspace: gsr_frame_stats_workspace_bytes(B, H, W) bytes (0 for sizes the call rejects), written before it is read.
 *
 * gsr_frame_compose: writes out[B, H, W_out, channels_out] uint8 from `n` panels, a HOST array that travels in the kernel arguments.
 * Panel k covers the output columns [x0, x0 + width) of every row and reads, for output pixel (b, i, x0 + j) and channel c,
 *     src[b*stride_b + c*stride_c + i*stride_y + j*stride_x]      (fp32 elements, signed strides; src2 through the same strides)
 * so a horizontal flip is stride_x = -1 with src at the row's last element, a one-channel expand is stride_c = 0, and the [H*W, 3]
 * normals of gsr_point_normals are stride_c = 1, stride_x = 3, stride_y = 3 W: nothing is materialised.  The modes:
 *     QUANT              q(src), three channels                      QUANT_CLAMP   q(clamp(src))
 *     ABSDIFF            q(|clamp(src) - src2|)                      NORMAL        the normal rule on src's three channels
 *     CMAP_CV            the CV map of src (one channel: stride_c is not used) with params[b].lo / hi and lut
 *     CMAP_MPL_ALIGNED   the MPL map of src*scale + shift            CMAP_MPL      the MPL map of src; both with params[b].lo2 / hi2 and lut
 * lut is a device uint8 [256,3] (RGB).  channels_out = 4 adds alpha: 255, or the MPL map's; channels_out = 3 drops it.  params is
 * [B,8] fp32 as gsr_frame_stats writes it and may be NULL when no panel has a CMAP mode.  The panels must tile [0, W_out) exactly,
 * in any order.  One thread makes four consecutive output pixels of one row; they are stored as whole dwords when out is 4-byte
 * aligned and channels_out = 4 or W_out % 4 == 0, else byte by byte (decided per call on the host).
 *
 * Both calls launch on `stream`, never synchronise, read nothing back, use no atomics and give the same bits for the same inputs.
 * Rejected before launching (GSR_ERR_INVALID_ARGUMENT, text in gsr_last_error): NULL pointers (depth, workspace, stats, params; a mask
 * without a target; panels, out, a panel's src, src2 for ABSDIFF, lut and params for the CMAP modes); B, H, W, W_out or a panel's width
 * <= 0; B > 65535; H*W*4 (H*W_out*4) >= 2^31 - 256; channels_out other than 3 or 4; n outside 1 .. GSR_FRAME_MAX_PANELS; unknown
 * modes; panels that overlap, leave a gap or leave [0, W_out).
 */
#define GSR_FRAME_MAX_PANELS 8
#define GSR_FRAME_QUANT            0
#define GSR_FRAME_QUANT_CLAMP      1
#define GSR_FRAME_ABSDIFF          2
#define GSR_FRAME_NORMAL           3
#define GSR_FRAME_CMAP_CV          4
#define GSR_FRAME_CMAP_MPL_ALIGNED 5
#define GSR_FRAME_CMAP_MPL         6
typedef struct {
    const float* src;   /* device */
    const float* src2;  /* device; ABSDIFF only, read through src's strides */
    const uint8_t* lut; /* device [256,3]; the CMAP modes only */
    long long stride_b, stride_c, stride_y, stride_x; /* elements, signed */
    int32_t x0, width;  /* output columns [x0, x0 + width) */
    int32_t mode;       /* GSR_FRAME_* */
} gsr_frame_panel;
size_t gsr_frame_stats_workspace_bytes(int B, int H, int W);
int gsr_frame_stats(int B, int H, int W, const float* depth, const float* target /* or NULL */, const float* lsq_mask /* or NULL */,
                    void* workspace, double* stats /* [B,8] */, float* params /* [B,8] */, void* stream /* hipStream_t */);
int gsr_frame_compose(int B, int H, int W_out, int channels_out, int n, const gsr_frame_panel* panels /* host */,
                      const float* params /* [B,8] or NULL */, uint8_t* out /* [B,H,W_out,channels_out] */, void* stream /* hipStream_t */);

/*
 * ---- PNG encoding (png.hip): the finished uint8 pictures -> the bytes of their .png files, on the device ----------------------
 * Replaces the encoder behind torchvision.utils.save_image, cv2.imwrite and plt.imsave in render_set (train.py:776-834).  A file
 * made here is a plain PNG that any decoder reads to the exact pixels; which of the many valid files it is, is fixed by these rules:
 *
 *   container  the 8 signature bytes, IHDR, one IDAT per deflate chunk, IEND; no ancillary chunks.  IHDR: width, height, bit depth 8,
 *              colour type 0 / 2 / 6 for C = 1 / 3 / 4, compression 0, filter method 0, no interlace.  Every chunk carries the CRC-32
 *              of its type and data.  The Adler-32 closes the last IDAT.
 *   zlib       the bytes 78 01, the deflate data, the Adler-32 of the filtered stream S, big-endian.
 *   S          H (1 + W C) bytes: per row the filter type, then the W C residuals with bpp = C; the row above the first is zeros.
 *              residual = (x - predictor) mod 256; the predictor of type 0 is 0, of 1 the byte a to the left (bpp back; 0 in the first
 *              pixel), of 2 the byte b above, of 3 floor((a + b) / 2), of 4 Paeth's: with c the byte above a and p = a + b - c, a
 *              when |p - a| <= |p - b| and |p - a| <= |p - c|, else b when |p - b| <= |p - c|, else c.
 *   filter     0 .. 4: that type in every row.  GSR_PNG_FILTER_ADAPTIVE: per row the type with the smallest sum over the row of
 *              |signed residual| (r < 128 ? r : 256 - r), ties to the lowest type (libpng's heuristic, stated as a rule).
 *   chunks     S is cut every GSR_PNG_CHUNK bytes, wherever that falls in a row.  A chunk is a deflate sequence of its own: nothing
 *              refers across a cut, and every chunk starts on a byte boundary.
 *   tokens     the first byte of a chunk is a literal.  A maximal run of L equal bytes is its first byte as a literal, then its
 *              L - 1 repeats cut into pieces of 258 from the front: a piece of 3 .. 258 is one match of that length at distance 1,
 *              a piece of 1 or 2 is literals.  (The greedy rule of zlib's Z_RLE strategy.)  Then the end-of-block symbol.
 *   block      one dynamic-Huffman block (BTYPE 10) or one stored block (BTYPE 00) per chunk, whichever has fewer bits, counted
 *              exactly; a tie is stored.  No fixed blocks.  A chunk that is not the last is followed by an empty stored block
 *              (BFINAL 0, BTYPE 00, padding to the byte, 00 00 FF FF); the last chunk's block has BFINAL set and is padded with zeros.
 *   codes      literal / length: Huffman's code lengths by a two-queue merge of the used symbols in ascending (count, symbol) order,
 *              a leaf before an internal node of the same weight; lengths beyond 15 are folded to 15, then, while the Kraft sum
 *              exceeds 1, one code of length 15 is taken away and one code of the greatest length below 15 that occurs becomes two
 *              codes one bit longer; the lengths go to the symbols longest first in ascending (count, symbol) order.  Kraft sum = 1
 *              exactly.  Canonical codes as RFC 1951 3.2.2.  Distance: HDIST = 1 code; its length is 1 when the chunk has a match
 *              (RFC 1951 3.2.7's single code of one bit, sent as 0), else 0.  Code-length code: the same construction with the limit
 *              7; if only one of its symbols occurs, symbol 0 (or 1, if that one is 0) also gets length 1 so that the code is
 *              complete.  HLIT = 257 or the last used length symbol + 1; HCLEN drops the trailing zeros of the permuted order.
 *   header     the HLIT + 1 code lengths as one sequence (runs cross into the distance code): a run of r zeros is, while r >= 3,
 *              symbol 17 (3 .. 10) or 18 (11 .. 138) for min(r, 138), then single zeros; a run of r equal nonzero lengths is the
 *              length once, then symbol 16 for min(r', 6) while the rest r' >= 3, then the length itself.
 *
 * gsr_png_capacity(H, W, C): what a file can take when every chunk is stored,
 *     8 + 25 + chunks (12 + 5 + 5) + H (1 + W C) + 2 + 4 + 12,   chunks = ceil(H (1 + W C) / GSR_PNG_CHUNK);
 * no file is larger.  0 for sizes the call rejects, as gsr_png_workspace_bytes.
 *
 * gsr_png_encode: images are B pictures of uint8 [H, W, C], pixel (b, y, x, c) at images[b*image_stride + y*row_stride + x*C + c]
 * (strides in bytes): the inner two dimensions are dense, the row stride is free (>= W C), so a panel of a wider sheet is read in
 * place.  Picture b's result is out + b*out_stride: GSR_PNG_HEADER_BYTES of header -- four uint32 words {the file's byte count, its
 * number of IDAT chunks, 0, 0} -- then the file.  Nothing behind the file's last byte is written.  out_stride >= header +
 * capacity and a multiple of 4, out 4-byte aligned, workspace 16-byte aligned and of gsr_png_workspace_bytes(B, H, W, C) bytes,
 * written before it is read.  Three launches on `stream` (filter: a workgroup per row; deflate: a workgroup per chunk with the
 * chunk and its output in LDS; assemble: a workgroup per IDAT, CRC-32 by slices combined through x^(8n) mod P); no synchronisation,
 * nothing read back, no dependency between workgroups, the same bytes for the same input.
 * Rejected before launching (GSR_ERR_INVALID_ARGUMENT): NULL pointers; B, H or W <= 0; C other than 1, 3, 4; B > 65535; W C >= 2^24;
 * H (1 + W C) >= 0x70000000; a filter outside 0 .. 5; row_stride < W C; a negative image_stride; out_stride or an alignment as above.
 */
#define GSR_PNG_CHUNK 32768
#define GSR_PNG_HEADER_BYTES 16
#define GSR_PNG_FILTER_ADAPTIVE 5
size_t gsr_png_capacity(int H, int W, int C);
size_t gsr_png_workspace_bytes(int B, int H, int W, int C);
int gsr_png_encode(const uint8_t* images, long long row_stride, long long image_stride, int B, int H, int W, int C, int filter,
                   uint8_t* out, size_t out_stride, void* workspace, void* stream /* hipStream_t */);

/*
 * ---- JPEG encoding (jpeg.hip): uint8 pictures -> baseline JPEG files, on the device -------------------------------------------
 * The lossy frames of the spiral video (gscream_amd/video.py: Motion-JPEG in an AVI), which stands where render_set calls ffmpeg
 * (train.py:844-846).  A file made here is a baseline sequential JFIF file that any decoder reads; which one it is, byte for byte,
 * is fixed by these rules (tests/jpeg_helpers.py states them in numpy, gscream_amd/jpeg.py's host path a second time):
 *
 *   input      uint8 [H, W, C], C = 1 (grey) or 3 (RGB)
 *   container  SOI; APP0 "JFIF\0" version 1.01, units 0, density 1:1, no thumbnail; one DQT per table (8-bit, id 0 luminance, id 1
 *              chrominance, zigzag order); SOF0 (precision 8, H, W, component ids 1, 2, 3, sampling 1x1 1x1 1x1 for 4:4:4 and
 *              2x2 1x1 1x1 for 4:2:0, quantisation tables 0, 1, 1); DHT DC 0, AC 0, DC 1, AC 1 (grey: DC 0, AC 0; one table per
 *              segment); DRI; SOS (components with tables 0/0, 1/1, 1/1; Ss 0, Se 63, Ah/Al 0); the scan; EOI; nothing behind EOI.
 *              A file without restart markers (the host path only) has no DRI segment.
 *   tables     Huffman: the typical tables of Annex K.3.  Quantisation: Annex K.1 / K.2 scaled as libjpeg does, for quality q = 1 .. 100:
 *              s = 5000 / q (q < 50, integer division) or 200 - 2 q;  t = clamp((base s + 50) / 100, 1, 255).
 *   colour     Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *              Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *              Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16          (arithmetic shifts; grey: Y = the input)
 *   padding    every plane is extended to whole MCUs (8x8; 16x16 for 4:2:0) by repeating its last column, then its last row
 *   4:2:0      a chroma sample is (a + b + c + d + bias) >> 2 over its 2x2 full-resolution samples, bias 1 in even output columns, 2 in odd
 *   DCT        C[k][n] = rint(8192 s_k cos((2n + 1) k pi / 16)), s_0 = 1 / sqrt(8), s_k = 1 / 2;  x = sample - 128
 *              rows:    r[m][k]  = (sum_n C[k][n] x[m][n] + 512) >> 10
 *              columns: c8[k][j] = (sum_m C[k][m] r[m][j] + 4096) >> 13            (8 x the orthonormal DCT; everything fits int32)
 *   quantise   v = sign(c8) ((|c8| + 4 Q) / (8 Q)), integer division, Q the table entry of (k, j); coded in zigzag order
 *   scan       MCUs in raster order; in an MCU the luminance blocks (4:2:0: top left, top right, bottom left, bottom right), Cb, Cr
 *   entropy    baseline Huffman: the DC difference against the previous block of the same component (0 at the start of an interval)
 *              as category + value bits; AC as (run, size) symbols + value bits, ZRL for every 16 zeros in front of a non-zero value,
 *              EOB unless coefficient 63 is non-zero; MSB first; a 0x00 behind every 0xFF byte; an interval's last byte is padded
 *              with 1 bits
 *   restart    DRI = Ri MCUs; RSTm (m = 0 .. 7 cycling) between intervals, none behind the last
 *
 * An interval holds at most GSR_JPEG_INTERVAL_BLOCKS blocks: Ri <= GSR_JPEG_INTERVAL_BLOCKS / (blocks per MCU: 1 grey, 3 4:4:4, 6 4:2:0).
 * restart_interval = 0 stands for min(the MCUs of one MCU row, that bound).
 *
 * gsr_jpeg_capacity(H, W, C, subsampling): file header + 416 blocks + 3 MCUs + 2, the file header being 629 bytes (C = 3) or 334
 * (C = 1).  No file of any restart interval is larger: a block is at most 22 + 63 * 26 bits (a DC code of 11 bits and 11 value bits,
 * 63 AC codes of 16 bits and 10 value bits) = 208 bytes, doubled by stuffing; an interval adds at most a padded byte and a marker,
 * and a picture has at most as many intervals as MCUs; EOI.  0 for sizes the call rejects.
 *
 * gsr_jpeg_encode: images as gsr_png_encode's (byte strides; the inner two dimensions dense, row_stride >= W C, so a panel of a sheet
 * is read in place).  Picture b's result is out + b*out_stride: GSR_JPEG_HEADER_BYTES of header -- four uint32 words {the file's byte
 * count, status, restart intervals, 0} -- then the file.  The room for a file is cap = out_stride - GSR_JPEG_HEADER_BYTES, ANY value
 * from the file header's size up: a file that does not fit has status GSR_JPEG_NEED_CAPACITY, its byte count (what it needs) in
 * word 0 and nothing written behind the four words; gsr_jpeg_capacity always fits.  Nothing behind a file's last byte is written.
 * out 4-byte aligned, out_stride a multiple of 4; workspace 16-byte aligned, of gsr_jpeg_workspace_bytes bytes (the coefficients, 128
 * bytes a block, and 4 bytes per interval), written before it is read.
 * Four launches on `stream`, no synchronisation, nothing read back, no global atomics, no workgroup waits for another, the same
 * bytes for the same input:
 *   transform  a thread per row of an 8x8 block: reads the picture through its strides, converts, pads, downsamples; row pass, LDS,
 *              column pass, quantise; int16 coefficients in zigzag order, blocks in scan order
 *   measure    a workgroup per restart interval, a thread per block: token bits, block scan, bits ORed into LDS words in pieces of
 *              32 KiB, 0xFF bytes counted -> the interval's byte count
 *   offsets    a workgroup per picture: scan of the interval sizes; the file header (built on the host from the tables compiled
 *              into the library, carried in the kernel arguments), EOI and the four words
 *   write      `measure` again, with each piece's bytes stuffed and written straight to their place in the file, and the RST marker
 * (Measuring and writing in two passes, where gsr_png_encode keeps a slot per chunk, saves a workspace of 416 bytes a block -- three
 * times the picture -- and a copy; it codes every block twice.)
 * Rejected before launching (GSR_ERR_INVALID_ARGUMENT): NULL pointers or pointers that are not device memory; B, H or W <= 0; H or
 * W > 65535; B > 65535; C other than 1, 3; quality outside 1 .. 100; subsampling other than 444, 420 (420 with C = 1); a capacity of
 * 2^31 or more; row_stride < W C; a negative image_stride; out_stride below header + file header, not a multiple of 4, out or
 * workspace misaligned; restart_interval < 0 or beyond the bound above.
 */
#define GSR_JPEG_HEADER_BYTES 16
#define GSR_JPEG_INTERVAL_BLOCKS 1024
#define GSR_JPEG_OK 0
#define GSR_JPEG_NEED_CAPACITY 1
size_t gsr_jpeg_capacity(int H, int W, int C, int subsampling);
size_t gsr_jpeg_workspace_bytes(int B, int H, int W, int C, int subsampling, int restart_interval);
int gsr_jpeg_encode(const uint8_t* images, long long row_stride, long long image_stride, int B, int H, int W, int C, int quality,
                    int subsampling, int restart_interval, uint8_t* out, size_t out_stride, void* workspace, void* stream /* hipStream_t */);

/*
 * ---- PNG decoding (png_decode.hip, png_inflate.h): the bytes of .png files -> uint8 [H, W, C] pictures, on the device ------------
 * Replaces Image.open + to_tensor + upload in readImages (train.py:887-902) and Scene's picture loading.  The host reads only the
 * chunk headers; inflate, Adler-32, unfilter and CRC-32 run on the device, a batch of files of any sizes in one call.
 *
 *   accepted   bit depth 8, no interlace, colour type 0 / 2 / 4 / 6 (C = 1 / 3 / 2 / 4); any number of IDAT chunks cut anywhere;
 *              ancillary chunks (skipped); any conforming zlib stream -- stored, fixed and dynamic blocks, distances to 32768,
 *              lengths to 258, overlapping copies; the five row filters in any mixture.  Everything else (16-bit and sub-byte depths,
 *              palette, Adam7, a bad signature or IHDR, no IDAT or IEND, a zlib header that is not deflate with a window of at most
 *              32 KiB and no dictionary) is the host parser's to reject: the device is never given such a file.
 *   bytes      the files' bytes, unmodified, back to back in one device buffer of `nbytes`.
 *   pieces     one gsr_png_piece per chunk of every file, in file order: the offset of the chunk's data in `bytes` (its type is
 *              the 4 bytes in front, its CRC the 4 bytes behind), the data's length, the file's index, and flags:
 *              GSR_PNG_PIECE_IDAT; GSR_PNG_PIECE_START on the first IDAT of a file and on every restart candidate.
 *   segments   an IDAT is a restart candidate when the IDAT before it ends in 00 00 FF FF (an empty stored block: the deflate
 *              stream is on a byte boundary there).  The candidates cut a file's IDATs into segments.  A file of one segment is
 *              decoded by one wavefront straight to its stream.  A file of several is measured first: every segment is decoded alone
 *              for its size only, and flagged when it fails in any way, when a distance reaches before its own first byte, when it
 *              does not end exactly at its last byte on a block boundary, or when BFINAL comes anywhere but in the last segment.
 *              No flag: the sizes are scanned and every segment is decoded by a wavefront of its own to its offset (path word 1,
 *              "parallel").  Any flag: one wavefront decodes the file with all IDATs joined (path word 0, "serial"), in the same
 *              launch sequence.  The files of gsr_png_encode take the parallel path; a Z_SYNC_FLUSH stream the serial one.
 *   files      one gsr_png_file per file: H, W, C; its first piece and piece count; its number of segments (START flags); the byte
 *              offset of its picture in `out` (H W C bytes, dense) and of its inflated stream in the workspace (H (1 + W C) bytes;
 *              offsets are multiples of 16 and the areas do not overlap).
 *   status     two int32 per file: {code, path}.  Codes:
 *                0 GSR_PNG_OK
 *                1 GSR_PNG_TRUNCATED      the deflate data or the Adler-32 ends early
 *                2 GSR_PNG_BLOCK_TYPE     block type 3
 *                3 GSR_PNG_STORED_LEN     a stored block's LEN and NLEN disagree
 *                4 GSR_PNG_BAD_CODE       an over-subscribed or incomplete code, no end-of-block code, a repeat with nothing before it
 *                5 GSR_PNG_BAD_SYMBOL     a bit pattern with no symbol, length symbol 286 / 287, distance symbol 30 / 31
 *                6 GSR_PNG_DISTANCE       a distance before the start of the stream
 *                7 GSR_PNG_TOO_LONG       the stream is longer than H (1 + W C)
 *                8 GSR_PNG_TOO_SHORT      ... or shorter
 *                9 GSR_PNG_FILTER         a filter byte above 4
 *               10 GSR_PNG_ADLER          the Adler-32 of the inflated stream differs from the trailer
 *               11 GSR_PNG_CRC            a chunk's CRC-32 differs (verify_crc only; every chunk is checked, also the skipped ones)
 *               12 GSR_PNG_TABLE          a table entry points outside `bytes`, `out` or the workspace: the file is not touched
 *              The first failing stage in the order inflate, size, Adler-32, filter, CRC decides.  A failed file's picture is
 *              unspecified; the other files of the batch are not affected.
 *   safety     every read is bounded by its piece and by nbytes, every write by the stream's or picture's size, every distance is
 *              checked against the bytes produced, every loop consumes a bit or produces a byte.  A corrupt file ends in a code.
 *
 * gsr_png_decode_workspace_bytes(stream_bytes, nfiles, npieces): stream_bytes = the end of the last stream area.
 * gsr_png_decode: all pointers are device pointers (bytes, out, workspace 16-byte aligned); launches on `stream` (validate, measure,
 * plan, inflate, Adler-32, unfilter, CRC-32), allocates nothing, never synchronises, reads nothing back.  Rejected before launching:
 * NULL pointers, nfiles or npieces <= 0, nbytes or out_bytes of 2^32 or more, a misaligned pointer.
 */
#define GSR_PNG_PIECE_IDAT 1u
#define GSR_PNG_PIECE_START 2u
typedef struct gsr_png_piece {
    uint64_t offset;  /* of the chunk's data in `bytes` */
    uint32_t length, flags, file, reserved;
} gsr_png_piece;
typedef struct gsr_png_file {
    int32_t H, W, C, first_piece, piece_count, segments;
    uint64_t out_offset, stream_offset;
} gsr_png_file;
enum {
    GSR_PNG_OK = 0, GSR_PNG_TRUNCATED, GSR_PNG_BLOCK_TYPE, GSR_PNG_STORED_LEN, GSR_PNG_BAD_CODE, GSR_PNG_BAD_SYMBOL, GSR_PNG_DISTANCE,
    GSR_PNG_TOO_LONG, GSR_PNG_TOO_SHORT, GSR_PNG_FILTER, GSR_PNG_ADLER, GSR_PNG_CRC, GSR_PNG_TABLE
};
size_t gsr_png_decode_workspace_bytes(size_t stream_bytes, int nfiles, int npieces);
int gsr_png_decode(const uint8_t* bytes, size_t nbytes, const gsr_png_file* files, int nfiles, const gsr_png_piece* pieces, int npieces,
                   int verify_crc, uint8_t* out, size_t out_bytes, int32_t* status, void* workspace, size_t workspace_bytes,
                   void* stream /* hipStream_t */);

/*
 * ---- Resize (resize.hip): PIL's Image.resize, byte for byte for 8-bit pictures and bit for bit for mode F ---------------------
 * Replaces mask.resize((1008, 567), Image.LANCZOS) of readImages (train.py:887-902) and pil_image.resize(resolution) of the
 * PILtoTorch* functions (utils/general_utils.py:35-75; PIL's default filter, BICUBIC) with their last step: / 255.0, > 0, or nothing.
 *
 * The rule, along one axis, inS -> outS, for a filter f of support s (BOX 0.5, BILINEAR 1, BICUBIC 2 with a = -0.5, LANCZOS 3):
 *   tables   (host, double; gscream_amd/resize.py)  scale = inS / outS, fs = max(scale, 1), support = s fs, ksize = ceil(support) 2 + 1;
 *            per output xx: c = (xx + 0.5) scale, xmin = max(int(c - support + 0.5), 0), n = min(int(c + support + 0.5), inS) - xmin,
 *            w[x] = f((x + xmin - c + 0.5) (1 / fs)), ww = their sum in index order, k[x] = w[x] / ww where ww != 0.
 *            bounds: int32 [outS][2] = {xmin, n};  coeffs: [outS][ksize], zero behind n.
 *   8-bit    coeffs int32 K = trunc(k 2^22 +- 0.5) (the sign of k);  acc = 2^21 + sum src[xmin + x] K[x] in int32 per channel;
 *            out = clamp(acc >> 22, 0, 255), the shift arithmetic.  Channels are independent.
 *   float32  coeffs double;  ss = 0, ss += double(src[xmin + x]) k[x] for x < n in index order, one rounding per operation, every
 *            tap of the bound included (0 * inf = NaN);  out = float(ss).
 *   passes   PIL runs the horizontal pass where the widths differ, then the vertical pass on its result where the heights differ;
 *            the intermediate is rounded to the picture's own type.  One call here is one pass: axis GSR_RESIZE_HORIZONTAL resamples
 *            W -> out_len in every row, GSR_RESIZE_VERTICAL resamples H -> out_len in every column.
 *   NEAREST  out[y][x] = src[yidx[y]][xidx[x]];  the tables are PIL's accumulated xo = 0.5 a, xo += a, index int(xo) (host).
 *            A NULL table is the identity, so equal sizes run an epilogue alone.
 * The kernels clip a bound to its row again (xmin >= 0, n <= inS - xmin, n <= ksize) and an index to [0, inS - 1]: no table takes a
 * load outside the picture.
 *
 * src: n pictures of H x W pixels of C interleaved channels (8-bit: C = 1 .. 4; float32: one channel), the channels of a pixel and
 * the pixels of a row adjacent, rows src_row_stride and pictures src_image_stride ELEMENTS apart (>= W C; a view of a wider tensor).
 * out, by `epilogue` (8-bit only):
 *   GSR_RESIZE_U8      uint8 [n][H'][W'][C], rows out_row_stride and pictures out_image_stride bytes apart
 *   GSR_RESIZE_DIV255  float32 [n][C][H'][W'] contiguous = __fdiv_rn(float(v), 255.0f): PILtoTorch's `/ 255.0` and permute
 *   GSR_RESIZE_GT0     float32 [n][C][H'][W'] contiguous = v > 0 ? 1 : 0: PILtoTorch_01mask's
 *   (for the float forms out_row_stride = W' and out_image_stride = C H' W' are required).
 * gsr_resize_f32 writes float32 [n][H'][W'] with the two strides in elements.
 * All pointers are device pointers; the calls launch one kernel on `stream`, allocate nothing, never synchronise, read nothing
 * back.  Rejected before launching: NULL pointers, sizes < 1, C outside 1 .. 4, H, W, out sizes or n above 65535, ksize < 1,
 * strides below the row or picture they step over, an unknown axis or epilogue.
 */
#define GSR_RESIZE_PRECISION_BITS 22
enum { GSR_RESIZE_HORIZONTAL = 0, GSR_RESIZE_VERTICAL = 1 };
enum { GSR_RESIZE_U8 = 0, GSR_RESIZE_DIV255 = 1, GSR_RESIZE_GT0 = 2 };
int gsr_resize_u8(const uint8_t* src, long long src_image_stride, long long src_row_stride, int n, int H, int W, int C, int axis, int out_len,
                  const int32_t* bounds, const int32_t* coeffs, int ksize, void* out, long long out_image_stride, long long out_row_stride,
                  int epilogue, void* stream /* hipStream_t */);
int gsr_resize_f32(const float* src, long long src_image_stride, long long src_row_stride, int n, int H, int W, int axis, int out_len,
                   const int32_t* bounds, const double* coeffs, int ksize, float* out, long long out_image_stride, long long out_row_stride,
                   void* stream /* hipStream_t */);
int gsr_resize_nearest_u8(const uint8_t* src, long long src_image_stride, long long src_row_stride, int n, int H, int W, int C, int H_out, int W_out,
                          const int32_t* yidx, const int32_t* xidx, void* out, long long out_image_stride, long long out_row_stride, int epilogue,
                          void* stream /* hipStream_t */);
int gsr_resize_nearest_f32(const float* src, long long src_image_stride, long long src_row_stride, int n, int H, int W, int H_out, int W_out,
                           const int32_t* yidx, const int32_t* xidx, float* out, long long out_image_stride, long long out_row_stride,
                           void* stream /* hipStream_t */);

/*
 * ---- the image-space RGB loss that follows the rasterizer ----------------------------------
 * Fused weighted L1 + weighted SSIM (11x11 Gaussian window, sigma 1.5, zero padding), value and gradient:
 *     L = a_l1 * mean(|img - gt| * m) + a_ssim * mean(ssim_map(img, gt) * m),   m = weight[H,W] (1 when NULL),
 * means over C*H*W.  Replaces GScream's utils/loss_utils.py:26-30 (l1_loss, l1_loss_masked) and :131-190 (ssim,
 * ssim_masked: five depthwise conv2d + ~10 elementwise passes each) as composed in train.py:538-545
 * (a_l1 = w (1 - lambda), a_ssim = -w lambda, the constant w lambda is added by the caller).
 * img, gt: [C,H,W] fp32 contiguous.  out3 (device): {L, mean(|d| m), mean(ssim m)}.  keep_state = 1 also stores what
 * the backward needs in the workspace (gsr_loss_workspace_bytes).  upstream: device pointer to dL/dL (NULL = 1).
 */
size_t gsr_loss_workspace_bytes(int C, int H, int W);
int gsr_rgb_loss_forward(int C, int H, int W, const float* img, const float* gt, const float* weight, float a_l1,
                         float a_ssim, void* workspace, float* out3, int keep_state, void* stream);
int gsr_rgb_loss_backward(int C, int H, int W, const float* img, const float* gt, const float* weight, float a_l1,
                          float a_ssim, const void* workspace, const float* upstream, float* dL_dimg, void* stream);
/* The same with ssim's `window_size` argument (utils/loss_utils.py:131,165; create_window :117-121): odd, 1..11 (11 = the two
 * entry points above = what GScream's trainer uses everywhere); other values -> GSR_ERR_UNSUPPORTED. */
int gsr_rgb_loss_forward_window(int C, int H, int W, const float* img, const float* gt, const float* weight, float a_l1,
                                float a_ssim, int window_size, void* workspace, float* out3, int keep_state, void* stream);
int gsr_rgb_loss_backward_window(int C, int H, int W, const float* img, const float* gt, const float* weight, float a_l1,
                                 float a_ssim, int window_size, const void* workspace, const float* upstream, float* dL_dimg,
                                 void* stream);

/*
 * The depth terms of the same loss (train.py:548-573): least-squares scale/shift alignment of the rendered depth to the
 * target over lsq_mask (utils/loss_utils.py:77-104), scale = |scale|, then
 *     L = lambda_l1 * mean(|a - y| * l1_weight) + sum_{k=0..3} 0.5 * lambda_smooth * gradient_loss(a[::2^k], y[::2^k], grad_mask[::2^k])
 * (utils/loss_utils.py:26-30, 40-49, 58-74), a = scale * depth + shift.  The gradient includes the path through the
 * fit.  depth, target, masks: [H,W] fp32 (masks may be NULL = ones).  out5 (device): {L, mean(|a-y| w), smooth part,
 * scale, shift}.  The forward keeps what the backward needs in the workspace.
 */
size_t gsr_depth_loss_workspace_bytes(int H, int W);
int gsr_depth_loss_forward(int H, int W, const float* depth, const float* target, const float* lsq_mask,
                           const float* l1_weight, const float* grad_mask, float lambda_l1, float lambda_smooth,
                           void* workspace, float* out5, void* stream);
int gsr_depth_loss_backward(int H, int W, const float* depth, const float* target, const float* lsq_mask,
                            const void* workspace, const float* upstream, float* dL_ddepth, void* stream);

/*
 * ---- SURVEY 8(f) rank 4 (init-only): simple_knn ------------------------------------------------------------------
 * mean_dist2[i] = mean of the three smallest squared fp32 distances from point i to the OTHER points.  Replaces
 * simple_knn._C.distCUDA2 (submodules/simple-knn/simple_knn.cu:185-220, spatial.cu), called once by
 * scene/gaussian_model.py at initialisation.  points: [P,3] fp32 contiguous; workspace: gsr_knn_workspace_bytes(P).
 */
size_t gsr_knn_workspace_bytes(int P);
int gsr_knn_mean_dist2(int P, const float* points, float* mean_dist2, void* workspace, void* stream);

/*
 * ---- scene initialisation (scene_init.hip): point cloud -> anchors -> the state create_from_pcd leaves ------------------------
 * Replaces GaussianModel.voxelize_sample and create_from_pcd (scene/gaussian_model.py:295-345).  All four calls launch on `stream`,
 * never allocate or synchronise and read nothing back; every counter and scan is an integer one, so the same inputs give the same
 * bits.  Workspaces: the *_workspace_bytes query of the call (0 for sizes the call rejects), written before they are read.
 *
 * gsr_sort_keys_u64: keys_out = the N unsigned 64-bit keys of keys_in in ascending order (all 64 bits significant; stable, which
 * a key-only sort cannot show but its users may rely on once it carries a payload).  keys_in == keys_out sorts in place.  LSD radix,
 * eight 8-bit digits; a workgroup ranks GSR_SORT_BLOCK_KEYS keys.  A pass whose digit is the same in every key is skipped; that is
 * decided on the device.  0 <= N <= 2^30.
 *
 * gsr_voxelize: points [N,3], fp32 (fp64 = 0) or fp64 (fp64 = 1); out [N,3] of the same type, of which the first M rows are written.
 * The voxel size v is the host double `voxel_size`, or, when voxel_size_dev is not NULL, the fp32 word it points to on the device.
 *     cell   r = round_half_even(p / v) per component, in the input's precision: fp32 input divides by (float) v (one IEEE fp32
 *            division, rintf), fp64 input by v in fp64 (rint).  -0.0 and +0.0 are the cell 0.
 *     key    (x - xmin, y - ymin, z - zmin) packed x-major into 64 bits; a field is as wide as its axis' range of cells needs
 *            (0 bits for a constant axis); minima and maxima are found on the device.
 *     rows   one per distinct key, in ascending key order = lexicographic (x, y, z) = the row order of numpy.unique(axis=0);
 *            value (T) cell * (T) v, one rounded product.
 * info (device int32 [4]) = {M, flags, the bits of (float) v, 0}.  A flag means the rows are not valid:
 *     GSR_VOXELIZE_NONFINITE   a quotient was NaN or infinite (a non-finite point, or v = 0 or NaN)
 *     GSR_VOXELIZE_CELL_RANGE  a cell index of magnitude >= 2^31
 *     GSR_VOXELIZE_KEY_WIDTH   the three field widths sum to more than 64 bits
 * 0 <= N <= 2^30.
 *
 * gsr_kth_smallest_f32: *out (device) = the k-th smallest (1-based, 1 <= k <= N) of N fp32 values = torch.kthvalue(v, k).values
 * (every NaN ordered last).  A radix select over four 8-bit digits of an order-preserving image of the bit patterns.
 *
 * gsr_scene_init_fill: one launch.  anchors [M,3], dist2 [M] (gsr_knn_mean_dist2 of the anchors) ->
 *     scaling [M,6] = logf(sqrtf(max(dist2, 1e-7f))) in all six columns;  offset [M,K,3] = 0;  anchor_feat [M,F] = 0;
 *     rotation [M,4] = (1, 0, 0, 0);  opacity, uncertainty [M,1] = `opacity` (the caller's inverse_sigmoid(0.1));
 *     max_radii2D [M] = 0;  xyz_max [3] = the column maxima of anchors (-inf for M = 0; -0.0 counts as +0.0).
 * M * max(3 K, F, 6) < 2^31.
 */
#define GSR_SORT_BLOCK_KEYS 2048
#define GSR_VOXELIZE_NONFINITE  1
#define GSR_VOXELIZE_CELL_RANGE 2
#define GSR_VOXELIZE_KEY_WIDTH  4
int gsr_sort_block_keys(void); /* GSR_SORT_BLOCK_KEYS of the library */
size_t gsr_sort_keys_workspace_bytes(int N);
int gsr_sort_keys_u64(int N, const uint64_t* keys_in, uint64_t* keys_out, void* workspace, void* stream /* hipStream_t */);
size_t gsr_voxelize_workspace_bytes(int N);
int gsr_voxelize(int N, int fp64, const void* points, double voxel_size, const float* voxel_size_dev /* or NULL */, void* workspace,
                 void* out /* [N,3] */, int32_t* info /* [4] */, void* stream);
size_t gsr_kth_smallest_workspace_bytes(int N);
int gsr_kth_smallest_f32(int N, int k, const float* values, void* workspace, float* out, void* stream);
int gsr_scene_init_fill(int M, int K, int F, const float* anchors, const float* dist2, float opacity, float* scaling, float* offset,
                        float* anchor_feat, float* rotation, float* opacity_out, float* uncertainty_out, float* max_radii2D,
                        float* xyz_max, void* stream);

/*
 * Optional per-stage timing (bench.py's roofline numbers; the reference has no counterpart -- its only
 * timing is two CUDA events around a whole training iteration, train.py:343-344,406,578).
 * Between gsr_profile_begin() and gsr_profile_end() every stage of every call is bracketed by a pair
 * of HIP events recorded on the stream the stage is launched on.  gsr_profile_end() waits for them and
 * returns the per-stage totals.  This is the only process-wide state in the library; off by default.
 */
int gsr_profile_begin(unsigned stage_mask /* bit i = time stage i; 0 = all */);
/* The same, timing only every `every`-th invocation of each selected stage (the first one included): an event pair costs the
 * stream a bubble on either side of the stage, so a benchmark that wants a stage's duration from inside its timed region samples. */
int gsr_profile_begin_sampled(unsigned stage_mask, unsigned every);
int gsr_profile_end(gsr_profile* out_host);
const char* gsr_stage_name(int stage);

#ifdef __cplusplus
}
#endif
#endif /* GSRASTER_H_INCLUDED */
