"""Anchor growing on the HIP path (the step that consumes the densification statistics).

`anchor_growing(model, grads, threshold, offset_mask)` mirrors GaussianModel.anchor_growing (scene/gaussian_model.py:808-900;
`model` takes the place of `self`) line for line: the same thresholds, the same torch.rand_like draw per level -- drawn before
the `length_inc == 0 and i > 0` skip --, the same padded mask, the same new-anchor tensors, accumulator padding and
`model.cat_tensors_to_optimizer` call (`torch.cuda.empty_cache()` is left out).  Integration is one line:

    GaussianModel.anchor_growing = gscream_amd.anchor_growing.anchor_growing

The tensor math of one level (:829-874: candidate cells, torch.unique, the chunked U x N duplicate test against the existing
anchors' cells, scatter_max of the features) is `grow_level`: HIP kernels around a torch.sort of 63-bit cell keys
(gscream_amd/csrc/anchor_grow.hip), bit-identical to the reference expressions in the same row order.  A level whose
candidate cells do not fit the keys (a cell outside [-2^20, 2^20) per axis, or a non-finite coordinate) runs the reference
expressions in torch on the device instead (`reference_level`)."""
from functools import reduce

import numpy as np
import torch

from . import _native
from .scatter import scatter_max

__all__ = ["grow_level", "reference_level", "anchor_growing"]


def _u8(mask):
    m = mask.detach().reshape(-1)
    return (m.view(torch.uint8) if m.dtype == torch.bool else (m != 0).view(torch.uint8)).contiguous()


def reference_level(anchor, offset, scaling, anchor_feat, candidate_mask, cur_size):
    """scene/gaussian_model.py:829-874 as the reference writes them (the fallback of grow_level)."""
    K, F = offset.shape[1], anchor_feat.shape[1]
    mask = candidate_mask.reshape(-1).bool()
    if mask.numel() < anchor.shape[0] * K:
        mask = torch.cat([mask, torch.zeros(anchor.shape[0] * K - mask.numel(), dtype=torch.bool, device=mask.device)], dim=0)
    all_xyz = anchor.unsqueeze(dim=1) + offset * scaling[:, :3].unsqueeze(dim=1)
    grid_coords = torch.round(anchor / cur_size).int()
    selected_xyz = all_xyz.view([-1, 3])[mask]
    selected_grid_coords = torch.round(selected_xyz / cur_size).int()
    selected_grid_coords_unique, inverse_indices = torch.unique(selected_grid_coords, return_inverse=True, dim=0)
    chunk_size = 4096
    max_iters = grid_coords.shape[0] // chunk_size + (1 if grid_coords.shape[0] % chunk_size != 0 else 0)
    remove_duplicates_list = []
    for j in range(max_iters):
        cur = (selected_grid_coords_unique.unsqueeze(1) == grid_coords[j * chunk_size:(j + 1) * chunk_size, :]).all(-1).any(-1).view(-1)
        remove_duplicates_list.append(cur)
    remove_duplicates = ~reduce(torch.logical_or, remove_duplicates_list)
    candidate_anchor = selected_grid_coords_unique[remove_duplicates] * cur_size
    new_feat = anchor_feat.unsqueeze(dim=1).repeat([1, K, 1]).view([-1, F])[mask]
    new_feat = scatter_max(new_feat, inverse_indices.unsqueeze(1).expand(-1, new_feat.size(1)), dim=0)[0][remove_duplicates]
    return candidate_anchor, new_feat


def grow_level(anchor, offset, scaling, anchor_feat, candidate_mask, cur_size):
    """One level: -> (candidate_anchor [C,3], new_feat [C,F]), fp32, bit-identical to reference_level.

    anchor [N,3], offset [N,K,3], scaling [N,6] (the ACTIVATED model.get_scaling), anchor_feat [N,F]: fp32 on a HIP device;
    candidate_mask [L] bool with L <= N*K (rows beyond L are not candidates: the reference pads with zeros); cur_size: the
    Python float the reference divides and multiplies by."""
    lib = _native.load()
    if not anchor.is_cuda:
        raise RuntimeError("gscream_amd.anchor_growing: tensors must be on a HIP device (no CPU fallback)")
    for t in (anchor, offset, scaling, anchor_feat):
        if t.dtype != torch.float32:
            raise ValueError("grow_level: anchor, offset, scaling and anchor_feat must be float32")
    dev = anchor.device
    N, K, F = int(anchor.shape[0]), int(offset.shape[1]), int(anchor_feat.shape[1])
    if tuple(offset.shape) != (N, K, 3) or tuple(scaling.shape) != (N, 6) or int(anchor_feat.shape[0]) != N:
        raise ValueError(f"grow_level: shapes anchor {tuple(anchor.shape)}, offset {tuple(offset.shape)}, scaling {tuple(scaling.shape)}, "
                         f"anchor_feat {tuple(anchor_feat.shape)} do not describe one set of N anchors with K offsets")
    mask = _u8(candidate_mask)
    L = int(mask.numel())
    if L > N * K:
        raise ValueError(f"grow_level: candidate_mask has {L} entries, more than N*K = {N * K}")
    anchor, offset, scaling, feat = (t.detach().contiguous() for t in (anchor, offset, scaling, anchor_feat))
    inv = float(np.float32(1.0) / np.float32(cur_size))  # x / cur_size on the GPU = x * (1.0f / (float)cur_size)
    size_f = float(np.float32(cur_size))
    ws = torch.empty(int(lib.gsr_anchor_grow_workspace_bytes(N, L)), dtype=torch.uint8, device=dev)
    keys = torch.empty(L, dtype=torch.int64, device=dev)
    rows = torch.empty(L, dtype=torch.int32, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    P = _native.ptr
    with _native.on_device(dev.index):
        _native.run("gsr_anchor_grow_keys", dev, N, K, L, P(anchor), P(offset), P(scaling), P(mask), inv, P(ws), P(keys), P(rows), P(info))
        M, flags = info[:2].tolist()
        if flags:
            return reference_level(anchor, offset, scaling, feat, candidate_mask, cur_size)
        cand = torch.empty((M, 3), dtype=torch.float32, device=dev)
        new_feat = torch.empty((M, F), dtype=torch.float32, device=dev)
        if M == 0:
            return cand, new_feat
        skeys, order = torch.sort(keys[:M], stable=True)  # torch.unique(dim=0)'s order; O(M log M) plumbing
        _native.run("gsr_anchor_grow_emit", dev, N, K, F, L, M, P(feat), P(skeys), P(order), P(rows), size_f, P(ws), P(cand), P(new_feat), P(info))
        C = int(info[2])
    return cand[:C], new_feat[:C]


def _inverse_sigmoid(x):  # utils/general_utils.py inverse_sigmoid
    return torch.log(x / (1 - x))


def anchor_growing(model, grads, threshold, offset_mask):
    init_length = model.get_anchor.shape[0] * model.n_offsets
    for i in range(model.update_depth):
        # update threshold
        cur_threshold = threshold * ((model.update_hierachy_factor // 2) ** i)
        # mask from grad threshold
        candidate_mask = (grads >= cur_threshold)
        candidate_mask = torch.logical_and(candidate_mask, offset_mask)

        # random pick
        rand_mask = torch.rand_like(candidate_mask.float()) > (0.5 ** (i + 1))
        rand_mask = rand_mask.to(candidate_mask.device)
        candidate_mask = torch.logical_and(candidate_mask, rand_mask)

        length_inc = model.get_anchor.shape[0] * model.n_offsets - init_length
        if length_inc == 0:
            if i > 0:
                continue
        # (length_inc > 0: the reference pads candidate_mask with zeros; grow_level treats the missing rows as zeros)

        size_factor = model.update_init_factor // (model.update_hierachy_factor ** i)
        cur_size = model.voxel_size * size_factor

        candidate_anchor, new_feat = grow_level(model.get_anchor.detach(), model._offset.detach(), model.get_scaling.detach(),
                                                model._anchor_feat.detach(), candidate_mask, cur_size)

        if candidate_anchor.shape[0] > 0:
            dev = candidate_anchor.device
            new_scaling = torch.ones_like(candidate_anchor).repeat([1, 2]).float() * cur_size
            new_scaling = torch.log(new_scaling)
            new_rotation = torch.zeros([candidate_anchor.shape[0], 4], device=dev).float()
            new_rotation[:, 0] = 1.0

            new_opacities = _inverse_sigmoid(0.1 * torch.ones((candidate_anchor.shape[0], 1), dtype=torch.float, device=dev))
            new_uncertainties = _inverse_sigmoid(0.1 * torch.ones((candidate_anchor.shape[0], 1), dtype=torch.float, device=dev))

            new_offsets = torch.zeros_like(candidate_anchor).unsqueeze(dim=1).repeat([1, model.n_offsets, 1]).float()

            d = {
                "anchor": candidate_anchor,
                "scaling": new_scaling,
                "rotation": new_rotation,
                "anchor_feat": new_feat,
                "offset": new_offsets,
                "opacity": new_opacities,
                "uncertainty": new_uncertainties,
            }

            model.anchor_demon = torch.cat([model.anchor_demon, torch.zeros([new_opacities.shape[0], 1], device=dev).float()], dim=0)
            model.opacity_accum = torch.cat([model.opacity_accum, torch.zeros([new_opacities.shape[0], 1], device=dev).float()], dim=0)
            model.uncertainty_accum = torch.cat([model.uncertainty_accum, torch.zeros([new_uncertainties.shape[0], 1], device=dev).float()],
                                                dim=0)

            optimizable_tensors = model.cat_tensors_to_optimizer(d)
            model._anchor = optimizable_tensors["anchor"]
            model._scaling = optimizable_tensors["scaling"]
            model._rotation = optimizable_tensors["rotation"]
            model._anchor_feat = optimizable_tensors["anchor_feat"]
            model._offset = optimizable_tensors["offset"]
            model._opacity = optimizable_tensors["opacity"]
            model._uncertainty = optimizable_tensors["uncertainty"]
