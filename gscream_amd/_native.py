"""ctypes binding of libgsraster.so (the C ABI declared in include/gsraster.h).

This is the only place that touches the native library.  There is NO fallback: if the HIP
library is missing or a call fails, a RuntimeError is raised -- the product path never routes
through the CPU oracle or through eager PyTorch.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB") or os.path.join(_HERE, "libgsraster.so")  # GSR_LIB: diagnostic builds

#: every symbol include/gsraster.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = (
    "gsr_version", "gsr_abi_version", "gsr_last_error", "gsr_device_count", "gsr_geom_bytes", "gsr_image_bytes",
    "gsr_binning_bytes", "gsr_backward_scratch_bytes", "gsr_forward_stage1", "gsr_forward_stage2", "gsr_forward",
    "gsr_backward", "gsr_filter", "gsr_mark_visible", "gsr_profile_begin", "gsr_profile_begin_sampled", "gsr_profile_end", "gsr_stage_name",
    "gsr_loss_workspace_bytes", "gsr_rgb_loss_forward", "gsr_rgb_loss_backward", "gsr_rgb_loss_forward_window",
    "gsr_rgb_loss_backward_window",
    "gsr_knn_workspace_bytes", "gsr_knn_mean_dist2", "gsr_decode_count", "gsr_decode_emit", "gsr_decode_backward",
    "gsr_depth_loss_workspace_bytes", "gsr_depth_loss_forward", "gsr_depth_loss_backward", "gsr_training_stats",
    "gsr_decode_weight_grad_workspace_bytes", "gsr_decode_zero_hidden_rows", "gsr_decode_visible_rows", "gsr_adaptive_reset",
    "gsr_anchor_grow_workspace_bytes", "gsr_anchor_grow_keys", "gsr_anchor_grow_emit", "gsr_scatter_max",
    "gsr_crossattn_workspace_bytes", "gsr_crossattn_forward", "gsr_crossattn_backward",
    "gsr_anchor_sample_workspace_bytes", "gsr_anchor_sample",
    "gsr_anchor_adjust_workspace_bytes", "gsr_anchor_adjust_offsets", "gsr_anchor_adjust_plan", "gsr_anchor_adjust_gather",
    "gsr_adam_step",
    "gsr_depth_points", "gsr_point_normals",
    "gsr_image_metrics_workspace_bytes", "gsr_image_metrics",
    "gsr_lpips_workspace_bytes", "gsr_lpips", "gsr_conv3x3_relu",
    "gsr_frame_stats_workspace_bytes", "gsr_frame_stats", "gsr_frame_compose",
    "gsr_png_capacity", "gsr_png_workspace_bytes", "gsr_png_encode",
    "gsr_jpeg_capacity", "gsr_jpeg_workspace_bytes", "gsr_jpeg_encode",
    "gsr_png_decode_workspace_bytes", "gsr_png_decode",
    "gsr_sort_block_keys", "gsr_sort_keys_workspace_bytes", "gsr_sort_keys_u64", "gsr_voxelize_workspace_bytes", "gsr_voxelize",
    "gsr_kth_smallest_workspace_bytes", "gsr_kth_smallest_f32", "gsr_scene_init_fill",
    "gsr_resize_u8", "gsr_resize_f32", "gsr_resize_nearest_u8", "gsr_resize_nearest_f32",
)
NUM_STAGES = 7
ABI_VERSION = 8  # include/gsraster.h GSR_ABI_VERSION this binding was written against


class Stage1Result(ctypes.Structure):
    _fields_ = [("num_rendered", ctypes.c_int32), ("max_tile_count", ctypes.c_int32),
                ("num_slots", ctypes.c_int32), ("num_occluded", ctypes.c_int32)]


class Tuning(ctypes.Structure):
    _fields_ = [("disable_tile_cull", ctypes.c_int32), ("disable_speculation", ctypes.c_int32),
                ("disable_partial_sort", ctypes.c_int32), ("inference", ctypes.c_int32), ("scatter_bands", ctypes.c_int32),
                ("occlusion_cut", ctypes.c_int32), ("heavy_groups", ctypes.c_int32), ("walk_depths_valid", ctypes.c_int32),
                ("walk_depths", ctypes.c_uint64)]


class AdjustCopy(ctypes.Structure):
    """gsr_adjust_copy: one tensor of gsr_anchor_adjust_gather's table (device pointers, floats per anchor row, ADJUST_* mode)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("width", ctypes.c_int32), ("mode", ctypes.c_int32)]


ADJUST_MAX_COPIES = 32
ADJUST_COPY, ADJUST_CLAMP_TAIL, ADJUST_OFFSET_STAT, ADJUST_ANCHOR_STAT = range(4)


class AdamTensor(ctypes.Structure):
    """gsr_adam_tensor: one tensor of gsr_adam_step's table (device pointers, element count, the seven fp32 scalars of its update)."""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("n", ctypes.c_int32),
                ("b1", ctypes.c_float), ("c1", ctypes.c_float), ("b2", ctypes.c_float), ("c2", ctypes.c_float), ("s2", ctypes.c_float),
                ("e", ctypes.c_float), ("a", ctypes.c_float)]


ADAM_MAX_TENSORS = 32


class FramePanel(ctypes.Structure):
    """gsr_frame_panel: one panel of gsr_frame_compose's table (device pointers, signed strides in elements, output columns, FRAME_* mode)."""
    _fields_ = [("src", ctypes.c_void_p), ("src2", ctypes.c_void_p), ("lut", ctypes.c_void_p), ("stride_b", ctypes.c_longlong),
                ("stride_c", ctypes.c_longlong), ("stride_y", ctypes.c_longlong), ("stride_x", ctypes.c_longlong), ("x0", ctypes.c_int32),
                ("width", ctypes.c_int32), ("mode", ctypes.c_int32)]


FRAME_MAX_PANELS = 8
PNG_CHUNK, PNG_HEADER_BYTES, PNG_FILTER_ADAPTIVE = 32768, 16, 5  # GSR_PNG_* of include/gsraster.h
PNG_PIECE_IDAT, PNG_PIECE_START = 1, 2
JPEG_HEADER_BYTES, JPEG_INTERVAL_BLOCKS, JPEG_NEED_CAPACITY = 16, 1024, 1  # GSR_JPEG_* of include/gsraster.h
PNG_STATUS = ("ok", "truncated", "reserved block type", "stored LEN/NLEN mismatch", "over-subscribed or incomplete code", "invalid symbol",
              "distance before the start of the stream", "stream longer than the picture's", "stream shorter than the picture's",
              "filter byte above 4", "Adler-32 mismatch", "CRC-32 mismatch", "table entry out of bounds")  # GSR_PNG_OK .. GSR_PNG_TABLE
RESIZE_HORIZONTAL, RESIZE_VERTICAL = 0, 1  # GSR_RESIZE_* of include/gsraster.h
RESIZE_U8, RESIZE_DIV255, RESIZE_GT0 = range(3)
FRAME_QUANT, FRAME_QUANT_CLAMP, FRAME_ABSDIFF, FRAME_NORMAL, FRAME_CMAP_CV, FRAME_CMAP_MPL_ALIGNED, FRAME_CMAP_MPL = range(7)


class Profile(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double * NUM_STAGES), ("launches", ctypes.c_int64 * NUM_STAGES)]


_lib = None
_c_int, _c_float, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p


def load():
    """Load libgsraster.so once.  Raises RuntimeError (never falls back) if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"gscream_amd: native library {LIB_PATH} is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C gscream_amd/csrc`. "
            "There is no CPU fallback for the rasterizer.")
    lib = ctypes.CDLL(LIB_PATH)
    try:
        lib.gsr_abi_version.restype = _c_int
        abi = int(lib.gsr_abi_version())
    except AttributeError:
        abi = None
    if abi != ABI_VERSION and not os.environ.get("GSR_SKIP_ABI_CHECK"):  # (the knob: tools/cut_probe.py, tools/gpu_ab.sh)
        raise RuntimeError(f"gscream_amd: {LIB_PATH} has C-ABI version {abi}, this binding needs {ABI_VERSION} "
                           "(rebuild with `make -C gscream_amd/csrc`)")
    lib.gsr_version.restype = ctypes.c_char_p
    lib.gsr_last_error.restype = ctypes.c_char_p
    lib.gsr_device_count.restype = _c_int
    for name in ("gsr_geom_bytes", "gsr_binning_bytes"):
        getattr(lib, name).restype = ctypes.c_size_t
        getattr(lib, name).argtypes = [_c_int]
    lib.gsr_image_bytes.restype = ctypes.c_size_t
    lib.gsr_image_bytes.argtypes = [_c_int, _c_int, _c_int]
    lib.gsr_backward_scratch_bytes.restype = ctypes.c_size_t
    lib.gsr_backward_scratch_bytes.argtypes = [_c_int, _c_int]
    lib.gsr_forward_stage1.restype = _c_int
    lib.gsr_forward_stage1.argtypes = (
        [_c_int] * 5 + [_vp, _vp, _c_float, _vp] + [_vp] * 5 + [_vp, _vp, _vp, _c_float, _c_float, _c_int]
        + [_vp, _vp, _vp, ctypes.POINTER(Stage1Result), ctypes.POINTER(Tuning), _c_int, _vp])
    lib.gsr_forward_stage2.restype = _c_int
    lib.gsr_forward_stage2.argtypes = [_c_int] * 5 + [_vp] * 7 + [ctypes.POINTER(Tuning), _c_int, _vp]
    lib.gsr_forward.restype = _c_int
    lib.gsr_forward.argtypes = (
        [_c_int] * 5 + [_vp, _vp, _c_float, _vp] + [_vp] * 5 + [_vp, _vp, _vp, _c_float, _c_float, _c_int]
        + [_vp, _vp, _vp, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp, ctypes.POINTER(Stage1Result), ctypes.POINTER(Tuning), _c_int, _vp])
    lib.gsr_backward.restype = _c_int
    lib.gsr_backward.argtypes = (
        [_c_int] * 8 + [_vp] * 6 + [_c_float] + [_vp] * 5 + [_c_float, _c_float] + [_vp] * 3 + [_vp] * 4
        + [_vp] * 9 + [ctypes.POINTER(Tuning), _c_int, _vp])
    lib.gsr_filter.restype = _c_int
    lib.gsr_filter.argtypes = [_c_int] * 3 + [_vp, _vp, _c_float] + [_vp] * 4 + [_c_float, _c_float, _c_int] + [_vp] * 3 + [_c_int, _vp]
    lib.gsr_mark_visible.restype = _c_int
    lib.gsr_mark_visible.argtypes = [_c_int] + [_vp] * 5
    lib.gsr_profile_begin.restype = _c_int
    lib.gsr_profile_begin.argtypes = [ctypes.c_uint]
    lib.gsr_profile_begin_sampled.restype = _c_int
    lib.gsr_profile_begin_sampled.argtypes = [ctypes.c_uint, ctypes.c_uint]
    lib.gsr_profile_end.restype = _c_int
    lib.gsr_profile_end.argtypes = [ctypes.POINTER(Profile)]
    lib.gsr_adaptive_reset.restype = None
    lib.gsr_adaptive_reset.argtypes = []
    lib.gsr_stage_name.restype = ctypes.c_char_p
    lib.gsr_stage_name.argtypes = [_c_int]
    lib.gsr_loss_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_loss_workspace_bytes.argtypes = [_c_int] * 3
    lib.gsr_rgb_loss_forward.restype = _c_int
    lib.gsr_rgb_loss_forward.argtypes = [_c_int] * 3 + [_vp] * 3 + [_c_float, _c_float, _vp, _vp, _c_int, _vp]
    lib.gsr_rgb_loss_backward.restype = _c_int
    lib.gsr_rgb_loss_backward.argtypes = [_c_int] * 3 + [_vp] * 3 + [_c_float, _c_float, _vp, _vp, _vp, _vp]
    lib.gsr_rgb_loss_forward_window.restype = _c_int
    lib.gsr_rgb_loss_forward_window.argtypes = [_c_int] * 3 + [_vp] * 3 + [_c_float, _c_float, _c_int, _vp, _vp, _c_int, _vp]
    lib.gsr_rgb_loss_backward_window.restype = _c_int
    lib.gsr_rgb_loss_backward_window.argtypes = [_c_int] * 3 + [_vp] * 3 + [_c_float, _c_float, _c_int, _vp, _vp, _vp, _vp]
    lib.gsr_knn_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_knn_workspace_bytes.argtypes = [_c_int]
    lib.gsr_knn_mean_dist2.restype = _c_int
    lib.gsr_knn_mean_dist2.argtypes = [_c_int, _vp, _vp, _vp, _vp]
    lib.gsr_decode_count.restype = _c_int
    lib.gsr_decode_count.argtypes = [_c_int, _c_int] + [_vp] * 13
    lib.gsr_decode_emit.restype = _c_int
    lib.gsr_decode_emit.argtypes = [_c_int, _c_int] + [_vp] * 18
    lib.gsr_decode_visible_rows.restype = _c_int
    lib.gsr_decode_visible_rows.argtypes = [_c_int] + [_vp] * 5
    lib.gsr_decode_backward.restype = _c_int
    lib.gsr_decode_backward.argtypes = [_c_int, _c_int] + [_vp] * 22
    lib.gsr_decode_weight_grad_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_decode_weight_grad_workspace_bytes.argtypes = []
    lib.gsr_decode_zero_hidden_rows.restype = _c_int
    lib.gsr_decode_zero_hidden_rows.argtypes = [_c_int, _c_int] + [_vp] * 6
    lib.gsr_depth_loss_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_depth_loss_workspace_bytes.argtypes = [_c_int, _c_int]
    lib.gsr_depth_loss_forward.restype = _c_int
    lib.gsr_depth_loss_forward.argtypes = [_c_int, _c_int] + [_vp] * 5 + [_c_float, _c_float, _vp, _vp, _vp]
    lib.gsr_depth_loss_backward.restype = _c_int
    lib.gsr_depth_loss_backward.argtypes = [_c_int, _c_int] + [_vp] * 7
    lib.gsr_training_stats.restype = _c_int
    lib.gsr_training_stats.argtypes = [_c_int, _c_int, _c_int] + [_vp] * 11
    lib.gsr_anchor_grow_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_anchor_grow_workspace_bytes.argtypes = [_c_int, _c_int]
    lib.gsr_anchor_grow_keys.restype = _c_int
    lib.gsr_anchor_grow_keys.argtypes = [_c_int] * 3 + [_vp] * 4 + [_c_float] + [_vp] * 5
    lib.gsr_anchor_grow_emit.restype = _c_int
    lib.gsr_anchor_grow_emit.argtypes = [_c_int] * 5 + [_vp] * 4 + [_c_float] + [_vp] * 5
    lib.gsr_scatter_max.restype = _c_int
    lib.gsr_scatter_max.argtypes = [_c_int] * 3 + [_vp] * 5
    lib.gsr_crossattn_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_crossattn_workspace_bytes.argtypes = [_c_int] * 4
    lib.gsr_crossattn_forward.restype = _c_int
    lib.gsr_crossattn_forward.argtypes = [_c_int] * 5 + [_vp] * 6 + [_c_float] + [_vp] * 4
    lib.gsr_crossattn_backward.restype = _c_int
    lib.gsr_crossattn_backward.argtypes = [_c_int] * 5 + [_vp] * 6 + [_c_float] + [_vp] * 10
    lib.gsr_anchor_sample_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_anchor_sample_workspace_bytes.argtypes = [_c_int, _c_int]
    lib.gsr_anchor_sample.restype = _c_int
    lib.gsr_anchor_sample.argtypes = [_c_int] * 3 + [_vp] * 4 + [_c_int] * 5 + [ctypes.c_uint64] + [_vp] * 7
    lib.gsr_anchor_adjust_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_anchor_adjust_workspace_bytes.argtypes = [_c_int]
    lib.gsr_anchor_adjust_offsets.restype = _c_int
    lib.gsr_anchor_adjust_offsets.argtypes = [_c_int, _vp, _vp, _c_float, _vp, _vp, _vp]
    lib.gsr_anchor_adjust_plan.restype = _c_int
    lib.gsr_anchor_adjust_plan.argtypes = [_c_int, _vp, _vp, _vp, _c_float, _c_float] + [_vp] * 5
    lib.gsr_anchor_adjust_gather.restype = _c_int
    lib.gsr_anchor_adjust_gather.argtypes = [_c_int] * 3 + [ctypes.POINTER(AdjustCopy), _vp, _vp, _c_int, _vp, _vp]
    lib.gsr_adam_step.restype = _c_int
    lib.gsr_adam_step.argtypes = [_c_int, ctypes.POINTER(AdamTensor), _vp]
    lib.gsr_depth_points.restype = _c_int
    lib.gsr_depth_points.argtypes = [_c_int, _c_int] + [_vp] * 5
    lib.gsr_point_normals.restype = _c_int
    lib.gsr_point_normals.argtypes = [_c_int, _c_int, _vp, _c_int, _c_float, ctypes.c_double, _vp, _vp]
    lib.gsr_image_metrics_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_image_metrics_workspace_bytes.argtypes = [_c_int] * 4
    lib.gsr_image_metrics.restype = _c_int
    lib.gsr_image_metrics.argtypes = [_c_int] * 4 + [_vp] * 3 + [ctypes.c_longlong] * 2 + [_c_int] + [_vp] * 4
    lib.gsr_lpips_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_lpips_workspace_bytes.argtypes = [_c_int] * 3
    lib.gsr_lpips.restype = _c_int
    lib.gsr_lpips.argtypes = [_c_int] * 3 + [_vp, _vp, _c_int] + [_vp] * 4 + [ctypes.c_longlong] + [_vp] * 6
    lib.gsr_conv3x3_relu.restype = _c_int
    lib.gsr_conv3x3_relu.argtypes = [_c_int] * 5 + [_vp] * 4 + [_c_int, _vp]
    lib.gsr_frame_stats_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_frame_stats_workspace_bytes.argtypes = [_c_int] * 3
    lib.gsr_frame_stats.restype = _c_int
    lib.gsr_frame_stats.argtypes = [_c_int] * 3 + [_vp] * 7
    lib.gsr_frame_compose.restype = _c_int
    lib.gsr_frame_compose.argtypes = [_c_int] * 5 + [ctypes.POINTER(FramePanel)] + [_vp] * 3
    lib.gsr_png_capacity.restype = ctypes.c_size_t
    lib.gsr_png_capacity.argtypes = [_c_int] * 3
    lib.gsr_png_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_png_workspace_bytes.argtypes = [_c_int] * 4
    lib.gsr_png_encode.restype = _c_int
    lib.gsr_png_encode.argtypes = [_vp, ctypes.c_longlong, ctypes.c_longlong] + [_c_int] * 5 + [_vp, ctypes.c_size_t, _vp, _vp]
    lib.gsr_jpeg_capacity.restype = ctypes.c_size_t
    lib.gsr_jpeg_capacity.argtypes = [_c_int] * 4
    lib.gsr_jpeg_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_jpeg_workspace_bytes.argtypes = [_c_int] * 6
    lib.gsr_jpeg_encode.restype = _c_int
    lib.gsr_jpeg_encode.argtypes = [_vp, ctypes.c_longlong, ctypes.c_longlong] + [_c_int] * 7 + [_vp, ctypes.c_size_t, _vp, _vp]
    lib.gsr_png_decode_workspace_bytes.restype = ctypes.c_size_t
    lib.gsr_png_decode_workspace_bytes.argtypes = [ctypes.c_size_t, _c_int, _c_int]
    lib.gsr_png_decode.restype = _c_int
    lib.gsr_png_decode.argtypes = [_vp, ctypes.c_size_t, _vp, _c_int, _vp, _c_int, _c_int, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_size_t, _vp]
    lib.gsr_sort_block_keys.restype = _c_int
    lib.gsr_sort_block_keys.argtypes = []
    for name in ("gsr_sort_keys_workspace_bytes", "gsr_voxelize_workspace_bytes", "gsr_kth_smallest_workspace_bytes"):
        getattr(lib, name).restype = ctypes.c_size_t
        getattr(lib, name).argtypes = [_c_int]
    lib.gsr_sort_keys_u64.restype = _c_int
    lib.gsr_sort_keys_u64.argtypes = [_c_int] + [_vp] * 4
    lib.gsr_voxelize.restype = _c_int
    lib.gsr_voxelize.argtypes = [_c_int, _c_int, _vp, ctypes.c_double] + [_vp] * 5
    lib.gsr_kth_smallest_f32.restype = _c_int
    lib.gsr_kth_smallest_f32.argtypes = [_c_int, _c_int] + [_vp] * 4
    lib.gsr_scene_init_fill.restype = _c_int
    lib.gsr_scene_init_fill.argtypes = [_c_int] * 3 + [_vp, _vp, _c_float] + [_vp] * 9
    _ll = ctypes.c_longlong
    lib.gsr_resize_u8.restype = _c_int
    lib.gsr_resize_u8.argtypes = [_vp, _ll, _ll] + [_c_int] * 6 + [_vp, _vp, _c_int, _vp, _ll, _ll, _c_int, _vp]
    lib.gsr_resize_f32.restype = _c_int
    lib.gsr_resize_f32.argtypes = [_vp, _ll, _ll] + [_c_int] * 5 + [_vp, _vp, _c_int, _vp, _ll, _ll, _vp]
    lib.gsr_resize_nearest_u8.restype = _c_int
    lib.gsr_resize_nearest_u8.argtypes = [_vp, _ll, _ll] + [_c_int] * 6 + [_vp, _vp, _vp, _ll, _ll, _c_int, _vp]
    lib.gsr_resize_nearest_f32.restype = _c_int
    lib.gsr_resize_nearest_f32.argtypes = [_vp, _ll, _ll] + [_c_int] * 5 + [_vp, _vp, _vp, _ll, _ll, _vp]
    _lib = lib
    return lib


STAGE_NAMES = ("preprocess", "count_scan", "scatter", "tile_sort", "blend_forward", "blend_backward", "gauss_backward")
NEED_CAPACITY = 1


def profile_begin(stages=None, every=1):
    """Start timing stages with HIP events (all stages, or only the named ones to keep the stream undisturbed; every = n
    times only every n-th invocation of a stage)."""
    mask = 0 if not stages else sum(1 << STAGE_NAMES.index(s) for s in stages)
    check(load().gsr_profile_begin_sampled(mask, int(every)), "gsr_profile_begin_sampled")


def profile_end():
    """-> {stage name: (total ms, launches)} measured with HIP events on the launch stream."""
    lib = load()
    p = Profile()
    check(lib.gsr_profile_end(ctypes.byref(p)), "gsr_profile_end")
    return {lib.gsr_stage_name(i).decode(): (float(p.total_ms[i]), int(p.launches[i])) for i in range(NUM_STAGES)}


def check(rc, what):
    if rc != 0:
        msg = load().gsr_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"gscream_amd native call {what} failed (code {rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor, or NULL for None / empty tensors (the reference's 'not provided').  A tensor in host memory
    raises: the native entry points do not look at their pointers, so a kernel handed one faults instead of failing."""
    if t is None or t.numel() == 0:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"gscream_amd: a {t.device} tensor ({tuple(t.shape)}, {t.dtype}) was about to be passed to a HIP kernel; "
                           "move it to the device first (the kernels do not check their pointers)")
    return ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # the handle without building a torch.cuda.Stream


def stream_handle(index):
    """HIP stream handle of torch's current stream on device `index` (what the kernels are enqueued on)."""
    if _raw_stream is not None:
        return _raw_stream(index)
    return torch.cuda.current_stream(index).cuda_stream


class on_device:
    """`with torch.cuda.device(dev)` that costs nothing when `dev` already is the current device (the training case)."""
    __slots__ = ("index", "prev")

    def __init__(self, index):
        self.index, self.prev = index, -1

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.index:
            self.prev = cur
            torch.cuda.set_device(self.index)
        return self.index

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
        return False


def run(name, device, *args):
    """lib.<name>(*args, stream) with `device` (a tensor's) current and on its current stream; raises unless it returns 0.
    The caller keeps every tensor behind `args` referenced until this returns (the launches are then enqueued).  A tensor among
    `args` is passed as ptr(tensor): its device is checked here, at the launch."""
    if any(isinstance(a, torch.Tensor) for a in args):
        args = [ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    with on_device(device.index) as index:
        check(getattr(load(), name)(*args, ctypes.c_void_p(stream_handle(index))), name)
