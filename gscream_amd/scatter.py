"""Segmented maximum (`torch_scatter.scatter_max`), on the HIP path for the form GScream uses.

`scatter_max(src, index, dim=-1, out=None, dim_size=None) -> (out, argmax)` follows torch_scatter 2.x's documented contract
(the package itself is a compiled CUDA extension and is not a dependency here; the contract is pinned by its documentation):
`index` is broadcast against `src` (a 1-D index runs along `dim`), the output has `dim_size` (default `index.max() + 1`)
slots along `dim`, a slot no element reaches holds 0 and argmax `src.size(dim)`.  When `out` is given it supplies the
starting values and is written in place (a slot keeps its value unless a larger element arrives).  Ties: argmax is the
SMALLEST source position holding the maximum -- a documented choice (torch_scatter promises no order among ties; GScream
reads only the values, scene/gaussian_model.py:874).

fp32 `src` of one or two dimensions reduced along dim 0 with a row index (1-D, or 2-D broadcast from one column such as
`index.unsqueeze(1).expand(-1, F)`) and no `out` runs one HIP kernel sequence (gsr_scatter_max).  Every other form runs exact
torch (scatter_reduce "amax" + an argmax pass): a different dtype or layout, not a missing kernel."""

import torch

from . import _native

__all__ = ["scatter_max"]


def _row_index(src, index, dim):
    """The [R] row index when (src, index, dim) is the HIP form, else None."""
    if src.dtype != torch.float32 or not src.is_cuda or src.dim() not in (1, 2) or dim % src.dim() != 0:
        return None
    if index.dim() == 1 and index.shape[0] == src.shape[0]:
        return index
    if (index.dim() == 2 and src.dim() == 2 and tuple(index.shape) == tuple(src.shape)
            and (index.shape[1] <= 1 or index.stride(1) == 0)):
        return index[:, 0] if index.shape[1] > 0 else None
    return None


def _broadcast(index, src, dim):
    """torch_scatter.utils.broadcast: a lower-dimensional index runs along `dim` and is expanded to src's shape."""
    if index.dim() == 1:
        view = [1] * src.dim()
        view[dim] = -1
        index = index.view(view)
    while index.dim() < src.dim():
        index = index.unsqueeze(-1)
    return index.expand_as(src)


def _torch_scatter_max(src, index, dim, out, dim_size):
    index = _broadcast(index, src, dim).long()
    if out is None:
        size = list(src.shape)
        size[dim] = dim_size
        out = src.new_zeros(size)
        res = out.scatter_reduce(dim, index, src, "amax", include_self=False)
    else:
        res = out.scatter_reduce(dim, index, src, "amax", include_self=True)
    n = src.size(dim)
    pos = torch.arange(n, device=src.device).view([-1 if d == dim else 1 for d in range(src.dim())]).expand_as(src)
    got = res.gather(dim, index)
    hit = (src == got) | (torch.isnan(src) & torch.isnan(got))
    arg = torch.full(res.shape, n, dtype=torch.long, device=src.device)
    arg = arg.scatter_reduce(dim, index, torch.where(hit, pos, torch.full_like(pos, n)), "amin", include_self=True)
    if out is not None:
        out.copy_(res)
        res = out
    return res, arg


def scatter_max(src, index, dim=-1, out=None, dim_size=None):
    dim = dim % src.dim() if src.dim() else 0
    if dim_size is None:
        if out is not None:
            dim_size = out.size(dim)
        else:
            dim_size = int(index.max()) + 1 if index.numel() > 0 else 0
    rows = _row_index(src, index, dim) if out is None else None
    if rows is None:
        return _torch_scatter_max(src, index, dim, out, int(dim_size))
    src = src.detach().contiguous()
    rows = rows.detach().long().contiguous()
    R = int(src.shape[0])
    F = int(src.shape[1]) if src.dim() == 2 else 1
    S = int(dim_size)
    shape = (S, F) if src.dim() == 2 else (S,)
    res = torch.empty(shape, dtype=torch.float32, device=src.device)
    arg = torch.empty(shape, dtype=torch.long, device=src.device)
    _native.run("gsr_scatter_max", src.device, R, F, S, _native.ptr(src), _native.ptr(rows), _native.ptr(res), _native.ptr(arg))
    return res, arg
