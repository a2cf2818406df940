"""The first stage of a run on the HIP path: point cloud -> anchors -> the state `GaussianModel.create_from_pcd` leaves
(scene/gaussian_model.py:295-345), and the device sort of 64-bit keys it is built on (gscream_amd/csrc/scene_init.hip).

The voxel rule, per component p of a point and voxel size v, in the INPUT's precision (what numpy does with a Python-float divisor):

    cell   r = round_half_even(p / v)      fp32 input: one IEEE fp32 division by float32(v), rintf; fp64 input: p / v and rint in fp64
    row    r * v                            one rounded product in the same precision; -0.0 and +0.0 are one cell
    rows   one per distinct (rx, ry, rz), in lexicographic (x, y, z) order: exactly numpy.unique(axis=0)

On the device a cell is an int32 (|r| < 2^31), the three cells minus their per-axis minima are packed x-major into one 64-bit key
whose field widths come from the cloud's own ranges (21 bits on every axis at once fit; the widths may sum to at most 64), the keys
are sorted (`sort_keys`' kernels), heads are marked where a key differs from its predecessor and placed by ordered compaction.

Device tensors take the kernels; a missing library raises.  CPU inputs, or force_torch=True, take the numpy / torch statement of the
same rules below (it is what the CPU tests run).  `last_path` says which one the last call took ("hip" / "torch")."""
import struct
import types

import numpy as np
import torch

from . import _native
from .simple_knn import distCUDA2

__all__ = ["SORT_BLOCK_KEYS", "sort_keys", "voxelize_sample", "kth_smallest", "create_from_pcd", "model_from_points", "opacity_init"]

SORT_BLOCK_KEYS = _native.SORT_BLOCK_KEYS  # keys one workgroup of the sort ranks (tests size their cases by it)
NONFINITE, CELL_RANGE, KEY_WIDTH = _native.VOXELIZE_NONFINITE, _native.VOXELIZE_CELL_RANGE, _native.VOXELIZE_KEY_WIDTH  # flag bits of info[1]
last_path = None  # "hip" / "torch": the path the last voxelize_sample() / kth_smallest() took

_FLAG_TEXT = (
    (NONFINITE, "a point or the voxel size is not finite, or the voxel size is 0 (limit: every round(p / voxel_size) must be finite)"),
    (CELL_RANGE, "a cell index is too large (limit: |round(p / voxel_size)| < 2^31)"),
    (KEY_WIDTH, "the cloud spans too many cells for a 64-bit key (limit: bits(x range) + bits(y range) + bits(z range) <= 64, "
                "where range = max cell - min cell on the axis)"),
)


def _raise_flags(flags):
    for bit, text in _FLAG_TEXT:
        if flags & bit:
            raise ValueError(f"voxelize_sample: {text}")


def opacity_init():
    """inverse_sigmoid(0.1) as CPU torch evaluates it in fp32 (utils/general_utils.py: log(x / (1 - x)) on 0.1 * ones):
    the value of create_from_pcd's `_opacity` and `_uncertainty`."""
    x = 0.1 * torch.ones((1, 1), dtype=torch.float)
    return float(torch.log(x / (1 - x)))


def _ws(nbytes, device):
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)


# ---- sort ---------------------------------------------------------------------------------------------------------------------
def sort_keys(keys):
    """The int64 or uint64 device tensor `keys` (one-dimensional) in ascending order of its 64-bit patterns read as UNSIGNED, for
    either dtype (so negative int64 values come last); the input is left as it is.  gsr_sort_keys_u64: a stable LSD radix sort, no
    host stop, the same bits for the same input."""
    if not isinstance(keys, torch.Tensor) or keys.dtype not in (torch.int64, torch.uint64) or keys.dim() != 1:
        raise ValueError("sort_keys: expected a one-dimensional int64 or uint64 tensor")
    if not keys.is_cuda:
        raise RuntimeError("sort_keys: keys must be on a HIP device (no CPU fallback)")
    lib = _native.load()
    src = keys.detach().contiguous()
    out = torch.empty_like(src)
    n = int(src.shape[0])
    if n == 0:
        return out
    ws = _ws(lib.gsr_sort_keys_workspace_bytes(n), src.device)
    _native.run("gsr_sort_keys_u64", src.device, n, _native.ptr(src), _native.ptr(out), _native.ptr(ws))
    return out


# ---- voxelize -----------------------------------------------------------------------------------------------------------------
def _voxelize_numpy(points, voxel_size):
    """The rule in numpy; `points` is a float32 / float64 array [N,3], `voxel_size` a Python float."""
    with np.errstate(all="ignore"):
        r = np.round(points / voxel_size)
    if not np.isfinite(r).all():
        _raise_flags(NONFINITE)
    if r.size and not (np.abs(r) < 2.0 ** 31).all():
        _raise_flags(CELL_RANGE)
    if r.size:
        cells = r.astype(np.int64)
        if sum(int(w).bit_length() for w in cells.max(axis=0) - cells.min(axis=0)) > 64:
            _raise_flags(KEY_WIDTH)
    return np.unique(r, axis=0) * voxel_size


def _voxelize_hip(points, voxel_size, voxel_size_dev=None):
    """gsr_voxelize on a contiguous fp32 / fp64 device tensor [N,3] -> (out [N,3], info int32 [4] on the device); the voxel size is
    the Python float, or the fp32 device word when given.  Nothing is read back."""
    lib = _native.load()
    n, dev = int(points.shape[0]), points.device
    out = torch.empty_like(points)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    ws = _ws(lib.gsr_voxelize_workspace_bytes(n), dev)
    _native.run("gsr_voxelize", dev, n, int(points.dtype == torch.float64), _native.ptr(points), float(voxel_size),
                _native.ptr(voxel_size_dev), _native.ptr(ws), _native.ptr(out), _native.ptr(info))
    return out, info


def _check_points(points, what):
    if points.ndim != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: expected [N,3] points, got {tuple(points.shape)}")


def voxelize_sample(points, voxel_size=0.01, force_torch=False):
    """GaussianModel.voxelize_sample (scene/gaussian_model.py:295-299): snap the points to a voxel_size grid and keep one per voxel,
    -> [M,3] in the input's dtype and kind (numpy array or tensor, on the input's device), rows in lexicographic (x, y, z) order.

    The reference shuffles the caller's array in place before numpy.unique, which sorts: the shuffle has no effect on the result,
    so it is not done here and the caller's array is NOT shuffled (or changed in any way).

    fp32 or fp64 input; other dtypes are taken as fp32.  Device tensors take gsr_voxelize, with one host stop, the read-back of
    `info` (M and the flags).  CPU inputs, or force_torch=True, take the numpy statement of the rule.  ValueError when a cell has no
    index (a non-finite point, voxel_size 0 or NaN), when an index reaches 2^31, or when the cloud's ranges need more than 64 key bits."""
    global last_path
    voxel_size = float(voxel_size)
    if isinstance(points, torch.Tensor):
        _check_points(points, "voxelize_sample")
        pts = points.detach()
        if pts.dtype not in (torch.float32, torch.float64):
            pts = pts.float()
        if pts.is_cuda and not force_torch:
            last_path = "hip"
            if pts.shape[0] == 0:
                return pts.clone()
            out, info = _voxelize_hip(pts.contiguous(), voxel_size)
            info_host = info.tolist()  # the one host stop: M for the shape, and the flags
            _raise_flags(info_host[1])
            return out[:info_host[0]]
        last_path = "torch"
        return torch.from_numpy(_voxelize_numpy(pts.cpu().numpy(), voxel_size)).to(pts.device)
    pts = np.asarray(points)
    _check_points(pts, "voxelize_sample")
    if pts.dtype not in (np.float32, np.float64):
        pts = pts.astype(np.float32)
    last_path = "torch"
    return _voxelize_numpy(pts, voxel_size)


# ---- k-th smallest ------------------------------------------------------------------------------------------------------------
def kth_smallest(values, k):
    """torch.kthvalue(values, k).values for a one-dimensional fp32 tensor: the k-th smallest, 1-based, as a 0-dim tensor on the
    values' device.  Device tensors take gsr_kth_smallest_f32 (a radix select on the bit patterns, no host stop); CPU tensors take
    torch.kthvalue.  k outside 1 .. N raises the error torch raises."""
    global last_path
    if not isinstance(values, torch.Tensor) or values.dim() != 1:
        raise ValueError("kth_smallest: expected a one-dimensional tensor")
    n, k = int(values.shape[0]), int(k)
    if n == 0:
        raise IndexError("kthvalue(): Expected reduction dim 0 to have non-zero size.")
    if k < 1 or k > n:
        raise RuntimeError("kthvalue(): selected number k out of range for dimension 0")
    if not values.is_cuda:
        last_path = "torch"
        return torch.kthvalue(values.detach(), k).values
    last_path = "hip"
    lib = _native.load()
    v = values.detach().contiguous().float()
    out = torch.empty((), dtype=torch.float32, device=v.device)
    ws = _ws(lib.gsr_kth_smallest_workspace_bytes(n), v.device)
    _native.run("gsr_kth_smallest_f32", v.device, n, k, _native.ptr(v), _native.ptr(ws), _native.ptr(out))
    return out


# ---- create_from_pcd ----------------------------------------------------------------------------------------------------------
def create_from_pcd(points, voxel_size=0.001, n_offsets=10, feat_dim=32, device="cuda"):
    """GaussianModel.create_from_pcd (scene/gaussian_model.py:301-345) -> a namespace with the reference's attribute names:
    _anchor [M,3], _offset [M,n_offsets,3], _anchor_feat [M,feat_dim], _scaling [M,6], _rotation [M,4], _opacity, _uncertainty [M,1],
    max_radii2D [M], all fp32 on the device, plus xyz_max [1,3], voxel_size (the Python float that was used) and dist2 [M] (distCUDA2
    of the anchors, unclamped).

    points: an fp32 / fp64 device tensor [N,3] (a numpy array is copied to `device` first; a CPU tensor raises: there is no CPU
    path).  voxel_size <= 0 means the reference's "median 3-NN distance": kthvalue(distCUDA2(points.float()), int(N * 0.5)), which
    stays on the device -- gsr_voxelize reads it from there.  There is exactly ONE host stop, the read-back of `info` (M, the flags
    and the voxel size): M has to reach the host for the shapes and for the kNN call.  The kNN and the fill are enqueued behind it."""
    if isinstance(points, np.ndarray):
        points = torch.from_numpy(np.ascontiguousarray(points)).to(device)
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError("gscream_amd.scene_init.create_from_pcd: points must be on a HIP device (no CPU fallback)")
    _check_points(points, "create_from_pcd")
    pts = points.detach()
    if pts.dtype not in (torch.float32, torch.float64):
        pts = pts.float()
    pts = pts.contiguous()
    n, dev, voxel_size = int(pts.shape[0]), pts.device, float(voxel_size)
    if n == 0:
        raise ValueError("create_from_pcd: the point cloud is empty")
    v_dev = None
    if voxel_size <= 0:
        k = int(n * 0.5)
        if k < 1:
            raise RuntimeError("kthvalue(): selected number k out of range for dimension 0")  # what torch.kthvalue(dist, 0) raises
        v_dev = kth_smallest(distCUDA2(pts.float()), k).reshape(1)
    out, info = _voxelize_hip(pts, voxel_size, v_dev)
    info_host = info.tolist()  # the one host stop: M, the flags, the bits of the voxel size
    _raise_flags(info_host[1])
    m = info_host[0]
    if v_dev is not None:
        voxel_size = struct.unpack("<f", struct.pack("<i", info_host[2]))[0]
    anchors = out[:m].float() if out.dtype != torch.float32 else (out[:m].clone() if m < n else out)
    dist2 = distCUDA2(anchors)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    s = types.SimpleNamespace(_anchor=anchors, _offset=new(m, n_offsets, 3), _anchor_feat=new(m, feat_dim), _scaling=new(m, 6),
                              _rotation=new(m, 4), _opacity=new(m, 1), _uncertainty=new(m, 1), max_radii2D=new(m), xyz_max=new(1, 3),
                              voxel_size=voxel_size, dist2=dist2)
    _native.load()
    _native.run("gsr_scene_init_fill", dev, m, int(n_offsets), int(feat_dim), _native.ptr(anchors), _native.ptr(dist2), opacity_init(),
                _native.ptr(s._scaling), _native.ptr(s._offset), _native.ptr(s._anchor_feat), _native.ptr(s._rotation), _native.ptr(s._opacity),
                _native.ptr(s._uncertainty), _native.ptr(s.max_radii2D), _native.ptr(s.xyz_max))
    return s


def model_from_points(points, voxel_size=0.001, n_offsets=10, feat_dim=32, seed=0, device="cuda"):
    """create_from_pcd's tensors in a standin_model.Model (Model.from_pcd: the MLPs keep nn.Linear's default initialisation), on the
    points' device -> (model, the namespace create_from_pcd returned)."""
    from . import standin_model as SM
    s = create_from_pcd(points, voxel_size=voxel_size, n_offsets=n_offsets, feat_dim=feat_dim, device=device)
    model = SM.Model.from_pcd(s._anchor, torch.clamp_min(s.dist2, 0.0000001), K=n_offsets, feat_dim=feat_dim, seed=seed).to(s._anchor.device)
    with torch.no_grad():
        model._scaling.copy_(s._scaling)
    return model, s
