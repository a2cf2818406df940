"""ctypes binding of libgsraster.so (the C ABI declared in include/gsraster.h).

This is the only place that touches the native library.  There is NO fallback: if the HIP
library is missing or a call fails, a RuntimeError is raised -- the product path never routes
through the CPU oracle or through eager PyTorch.

The header is the source of this binding (_abi.py reads it): a new entry point or constant is an edit of
include/gsraster.h and the module's own .hip file (its C entry points are at the file's end), and of nothing here unless a wrapper wants the constant under a name of its own (_CONSTANTS).
"""
import ctypes
import os

import torch

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB") or os.path.join(_HERE, "libgsraster.so")  # GSR_LIB: diagnostic builds

_ABI = _abi.header()  # include/gsraster.h, parsed once: the symbol list, every signature and every constant below come from it
#: every symbol include/gsraster.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = tuple(_ABI.functions)
ABI_VERSION = _ABI.constants["GSR_ABI_VERSION"]  # a library that reports another value is refused by load()
NUM_STAGES = _ABI.constants["GSR_NUM_STAGES"]
#: GSR_<NAME> of the header, each under the name <NAME>
_CONSTANTS = ("NEED_CAPACITY", "ADJUST_MAX_COPIES", "ADJUST_COPY", "ADJUST_CLAMP_TAIL", "ADJUST_OFFSET_STAT",
              "ADJUST_ANCHOR_STAT", "ADAM_MAX_TENSORS", "FRAME_MAX_PANELS", "FRAME_QUANT", "FRAME_QUANT_CLAMP", "FRAME_ABSDIFF", "FRAME_NORMAL",
              "FRAME_CMAP_CV", "FRAME_CMAP_MPL_ALIGNED", "FRAME_CMAP_MPL", "PNG_CHUNK", "PNG_HEADER_BYTES", "PNG_FILTER_ADAPTIVE",
              "PNG_PIECE_IDAT", "PNG_PIECE_START", "JPEG_HEADER_BYTES", "JPEG_INTERVAL_BLOCKS", "JPEG_NEED_CAPACITY", "RESIZE_HORIZONTAL",
              "RESIZE_VERTICAL", "RESIZE_U8", "RESIZE_DIV255", "RESIZE_GT0", "METRICS_CLAMP", "METRICS_QUANTIZE", "LPIPS_NORMALIZE",
              "LPIPS_SCALING", "SORT_BLOCK_KEYS", "VOXELIZE_NONFINITE", "VOXELIZE_CELL_RANGE", "VOXELIZE_KEY_WIDTH")
globals().update({name: _ABI.constants["GSR_" + name] for name in _CONSTANTS})
# what the header holds as comments only; the lengths are held to its constants
STAGE_NAMES = ("preprocess", "count_scan", "scatter", "tile_sort", "blend_forward", "blend_backward", "gauss_backward")
PNG_STATUS = ("ok", "truncated", "reserved block type", "stored LEN/NLEN mismatch", "over-subscribed or incomplete code", "invalid symbol",
              "distance before the start of the stream", "stream longer than the picture's", "stream shorter than the picture's",
              "filter byte above 4", "Adler-32 mismatch", "CRC-32 mismatch", "table entry out of bounds")  # GSR_PNG_OK .. GSR_PNG_TABLE
assert len(STAGE_NAMES) == NUM_STAGES and len(PNG_STATUS) == _ABI.constants["GSR_PNG_TABLE"] + 1


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


class AdamTensor(ctypes.Structure):
    """gsr_adam_tensor: one tensor of gsr_adam_step's table (device pointers, element count, the seven fp32 scalars of its update)."""
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("n", ctypes.c_int32),
                ("b1", ctypes.c_float), ("c1", ctypes.c_float), ("b2", ctypes.c_float), ("c2", ctypes.c_float), ("s2", ctypes.c_float),
                ("e", ctypes.c_float), ("a", ctypes.c_float)]


class FramePanel(ctypes.Structure):
    """gsr_frame_panel: one panel of gsr_frame_compose's table (device pointers, signed strides in elements, output columns, FRAME_* mode)."""
    _fields_ = [("src", ctypes.c_void_p), ("src2", ctypes.c_void_p), ("lut", ctypes.c_void_p), ("stride_b", ctypes.c_longlong),
                ("stride_c", ctypes.c_longlong), ("stride_y", ctypes.c_longlong), ("stride_x", ctypes.c_longlong), ("x0", ctypes.c_int32),
                ("width", ctypes.c_int32), ("mode", ctypes.c_int32)]


class LayoutPiece(ctypes.Structure):
    """gsr_layout_piece: one array of a rasterizer workspace as gsr_workspace_layout reports it (name: a C string the library owns)."""
    _fields_ = [("name", ctypes.c_void_p), ("offset", ctypes.c_size_t), ("count", ctypes.c_size_t), ("elem_size", ctypes.c_size_t)]


class Profile(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double * NUM_STAGES), ("launches", ctypes.c_int64 * NUM_STAGES)]


#: the header's structs that have a class here (tests hold every field to the header); a pointer to one is typed, any other is void*
STRUCTS = {"gsr_stage1_result": Stage1Result, "gsr_tuning": Tuning, "gsr_adjust_copy": AdjustCopy, "gsr_adam_tensor": AdamTensor,
           "gsr_frame_panel": FramePanel, "gsr_profile": Profile, "gsr_layout_piece": LayoutPiece}
_lib = None


def load():
    """Load libgsraster.so once and type every function the header declares from its declaration (_abi.ctype: an unknown type raises).
    Raises RuntimeError (never falls back) if the library is not built, AttributeError if it lacks a declared function."""
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
        abi = int(lib.gsr_abi_version())
    except AttributeError:
        abi = None
    if abi != ABI_VERSION and not os.environ.get("GSR_SKIP_ABI_CHECK"):  # (the knob: tools/cut_probe.py, tools/gpu_ab.sh)
        raise RuntimeError(f"gscream_amd: {LIB_PATH} has C-ABI version {abi}, this binding needs {ABI_VERSION} "
                           "(rebuild with `make -C gscream_amd/csrc`)")
    for name, (returns, params) in _ABI.functions.items():
        fn = getattr(lib, name)
        fn.restype = _abi.ctype(returns, returns=True)
        fn.argtypes = [_abi.ctype(ctype, STRUCTS) for ctype, _, _, _ in params]
    _lib = lib
    return lib


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
