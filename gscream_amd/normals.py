"""Normals from rendered depth on the HIP path: the two functions render_set applies to every frame of the RGBD video.

Drop-ins for train.py's `depth2pcd_fromplane` (:252-267) and `least_square_normal_regress_fast01` (:270-298), same arguments in the
same order, same return shapes; integration is two rebindings in front of render_set (INTEGRATION Q):

    depth2pcd_fromplane = gscream_amd.normals.depth2pcd_fromplane
    least_square_normal_regress_fast01 = gscream_amd.normals.least_square_normal_regress_fast01

or `normal_map(depth, c2w, K)` for lines :820-824 in one call.  The rules (include/gsraster.h has them in full):

  points   xn = (j - K[0][2]) / K[0][0], yn = (i - K[1][2]) / K[1][1], P[r] = ((c2w[r][0] xn d + c2w[r][1] yn d) + c2w[r][2] d) + c2w[r][3],
           fp32 with one rounding per operation.
  normals  per pixel, over the size x size window with replicate padding: a window point is zeroed iff |(q.z - c.z) / c.z| > gamma in
           fp32 (the reference's decision bit for bit: only z decides, NaN keeps, inf drops); A = sum q q^T and s = sum q in fp64;
           det(A) < eps -> v = s, otherwise v = A^-1 s; -v / max(|v|, 1e-12) with NaN -> 0, rounded to fp32 once.

The reference evaluates the sums, det and inverse in fp32, where cond(A) ~ (|p| / patch extent)^2 of the uncentred normal equations
(1e5 .. 1e7 at a real focal length) leaves no correct digit; both paths here carry them in fp64 and return the value the expression
defines.  The return keeps the reference's layout: it views its [h*w, 3] result as [1, w, h, 3] and permutes, so the result is a
[1, 3, w, h] tensor r with r[0, c, a, b] = n[a*h + b, c], and the caller's r.reshape(3, h, w)[c, i, j] is pixel (i, j).

The HIP path (gscream_amd/csrc/normals.hip; `last_path = "hip"`) takes fp32, contiguous tensors on a HIP device with batch 1 and an
odd size <= 15; it launches on torch's current stream, allocates its output and nothing else, never synchronises, and does not read
global_eye / global_b (None is accepted: the caller can drop its [h*w, 81, 1] ones).  Everything else -- CPU tensors, other dtypes,
`force_torch = True` -- takes `_normals_torch`, a torch statement of the same rules that uses global_eye / global_b when they are
given (`last_path = "torch"`).  A missing library raises; nothing falls back quietly."""
import numpy as np
import torch

from . import _native

__all__ = ["depth2pcd_fromplane", "least_square_normal_regress_fast01", "normal_map"]

force_torch = False
last_path = None  # "hip" / "torch": the path the last call took

MAX_SIZE = 15            # gsr_point_normals: odd, 1 .. 15
MAX_PIXELS = 0x7FFFFF00  # both kernels' limit on h*w


def _hip_tensor(t):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


# ---- depth -> point map ----
def _points_torch(depth2d, c2w, K, h, w):
    """The point-map rule in torch, in the kernel's operation order (eager elementwise operations round once each)."""
    dt, dev = depth2d.dtype, depth2d.device
    K = torch.as_tensor(K, dtype=dt, device=dev)
    c = torch.as_tensor(c2w, dtype=dt, device=dev)
    d = depth2d.reshape(h, w)
    j = torch.arange(w, dtype=dt, device=dev)[None, :]
    i = torch.arange(h, dtype=dt, device=dev)[:, None]
    xc = (j - K[0][2]) / K[0][0] * d
    yc = (i - K[1][2]) / K[1][1] * d
    rows = [((c[r][0] * xc + c[r][1] * yc) + c[r][2] * d) + c[r][3] for r in range(3)]
    return torch.stack(rows).reshape(1, 3, h, w)


def depth2pcd_fromplane(depth2d, c2w, K, h, w):
    """depth2d [1, h, w] (or [h, w]), c2w [3, 4], K [3, 3] -> world-space point map [1, 3, h, w]."""
    global last_path
    h, w = int(h), int(w)
    if not isinstance(depth2d, torch.Tensor):
        depth2d = torch.as_tensor(depth2d)
    if depth2d.numel() != h * w:
        raise ValueError(f"depth2pcd_fromplane: depth has {depth2d.numel()} elements, h*w = {h * w}")
    if force_torch or not _hip_tensor(depth2d) or h * w == 0 or h * w >= MAX_PIXELS:
        last_path = "torch"
        return _points_torch(depth2d, c2w, K, h, w)
    dev = depth2d.device
    K = torch.as_tensor(K, dtype=torch.float32, device=dev).contiguous()    # (no copy for what render_set passes: device tensors)
    c2w = torch.as_tensor(c2w, dtype=torch.float32, device=dev).contiguous()
    if tuple(K.shape) != (3, 3) or tuple(c2w.shape) != (3, 4):
        raise ValueError(f"depth2pcd_fromplane: K is {tuple(K.shape)}, c2w is {tuple(c2w.shape)} (need [3, 3] and [3, 4])")
    last_path = "hip"
    points = torch.empty((1, 3, h, w), dtype=torch.float32, device=dev)
    _native.run("gsr_depth_points", dev, h, w, _native.ptr(depth2d), _native.ptr(K), _native.ptr(c2w), _native.ptr(points))
    return points


# ---- point map -> normals ----
def _window_sums_torch(points, size, gamma, dtype, global_b=None):
    """points [3, h, w] -> (X [h*w, size^2, 3] the masked window points in `dtype`, A = X^T X [h*w, 3, 3], b [h*w, size^2, 1]: ones, or global_b).
    The mask decision is taken in fp32 whatever `dtype` is."""
    _, h, w = points.shape
    r = size // 2
    dev = points.device
    p32 = points.to(torch.float32)
    off = torch.arange(-r, r + 1, device=dev)
    iy = (torch.arange(h, device=dev)[:, None] + off[None, :]).clamp_(0, h - 1)  # replicate padding = clamped indices
    ix = (torch.arange(w, device=dev)[:, None] + off[None, :]).clamp_(0, w - 1)
    win = p32[:, iy[:, None, :, None], ix[None, :, None, :]].reshape(3, h, w, size * size)  # rows, then columns
    cz = p32[2][:, :, None]
    drop = ((win[2] - cz) / cz).abs() > float(np.float32(gamma))  # fp32 against the fp32 value of gamma; False for NaN
    X = torch.where(drop[None], win.new_zeros(()), win).permute(1, 2, 3, 0).reshape(h * w, size * size, 3).to(dtype)
    Xt = X.transpose(1, 2)
    A = torch.bmm(Xt, X)
    b = X.new_ones((h * w, size * size, 1)) if global_b is None else global_b.to(dtype)
    return X, A, b


def _normals_torch(points, size=9, gamma=0.15, eps=1e-5, dtype=torch.float64, global_eye=None, global_b=None):
    """The rules in torch: points [3, h, w] (or [1, 3, h, w]) -> normals [h*w, 3] in `dtype`, by pixel.  dtype=float64 is the product's
    fallback (the caller rounds to fp32); dtype=float32 is the reference's arithmetic -- batched matmul, det and inverse in fp32 --
    and exists for tools/normals_bench.py only."""
    if points.dim() == 4:
        points = points[0]
    X, A, b = _window_sums_torch(points, size, gamma, dtype, global_b)
    det = torch.linalg.det(A)
    eye = torch.eye(3, dtype=dtype, device=A.device) if global_eye is None else global_eye.to(dtype)
    A = torch.where((det < eps)[:, None, None], eye, A)
    inv = torch.linalg.inv_ex(A).inverse  # (no error check: a singular system gives inf / NaN, which end as 0 below)
    v = torch.matmul(torch.matmul(inv, X.transpose(1, 2)), b).reshape(-1, 3)
    length = torch.sqrt((v * v).sum(1, keepdim=True))
    v = v / torch.where(length < 1e-12, torch.full_like(length, 1e-12), length)  # max(length, 1e-12) that keeps a NaN length
    return -torch.where(torch.isnan(v), torch.zeros_like(v), v)


def _as_reference_returns(n, h, w):
    """[h*w, 3] by pixel -> the reference's return: the rows viewed as [1, w, h, 3], permuted to [1, 3, w, h]."""
    return n.view(1, w, h, 3).permute(0, 3, 1, 2)


def least_square_normal_regress_fast01(x_depth3d, global_eye=None, global_b=None, size=9, gamma=0.15, depth_scaling_factor=1, eps=1e-5):
    """x_depth3d [1, 3, h, w] -> [1, 3, w, h] in the reference's layout (see the module text).  depth_scaling_factor is unused, as in the
    reference."""
    global last_path
    if x_depth3d.dim() != 4 or x_depth3d.shape[1] != 3:
        raise ValueError(f"least_square_normal_regress_fast01: x_depth3d is {tuple(x_depth3d.shape)} (need [batch, 3, h, w])")
    size = int(size)
    batch, _, h, w = x_depth3d.shape
    if (force_torch or not _hip_tensor(x_depth3d) or batch != 1 or size < 1 or size > MAX_SIZE or size % 2 == 0 or h * w == 0
            or h * w >= MAX_PIXELS):
        last_path = "torch"
        if size < 1 or size % 2 == 0:
            raise ValueError(f"least_square_normal_regress_fast01: size={size} (need an odd size: the window has a centre)")
        parts = [_normals_torch(x_depth3d[k], size, gamma, eps, torch.float64, global_eye, global_b).to(x_depth3d.dtype) for k in range(batch)]
        n = parts[0] if batch == 1 else torch.cat(parts)
        return n.view(batch, w, h, 3).permute(0, 3, 1, 2)
    last_path = "hip"
    n = torch.empty((h * w, 3), dtype=torch.float32, device=x_depth3d.device)
    _native.run("gsr_point_normals", x_depth3d.device, h, w, _native.ptr(x_depth3d), size, float(np.float32(gamma)), float(eps), _native.ptr(n))
    return _as_reference_returns(n, h, w)


def _picture_tail(normal, h, w):
    """train.py:822-824: the caller's reshape, second normalisation and map to [0, 1]."""
    normal = normal.reshape(3, h, w).permute(1, 2, 0)
    normal = torch.nn.functional.normalize(normal, p=2, dim=-1).permute(2, 0, 1)
    return (normal + 1) / 2


def normal_map(depth, c2w, K):
    """depth [1, h, w] (or [h, w]), c2w [3, 4], K [3, 3] -> the normal picture [3, h, w] in [0, 1]: train.py:820-824 in one call
    (the caller keeps its horizontal flip)."""
    h, w = int(depth.shape[-2]), int(depth.shape[-1])
    points = depth2pcd_fromplane(depth, c2w, K, h, w)
    return _picture_tail(least_square_normal_regress_fast01(points), h, w)
