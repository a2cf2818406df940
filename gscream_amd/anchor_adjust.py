"""Anchor pruning on the HIP path: the method that drives densification.

`adjust_anchor(model, check_interval, success_threshold, grad_threshold, min_opacity)` mirrors GaussianModel.adjust_anchor
(scene/gaussian_model.py:914-973) and `prune_anchor(model, mask)` mirrors GaussianModel.prune_anchor with
_prune_anchor_optimizer (:762-805); `model` takes the place of `self`, both run under the caller's torch.no_grad()
(train.py:580).  Integration is two lines:

    GaussianModel.adjust_anchor = gscream_amd.anchor_adjust.adjust_anchor
    GaussianModel.prune_anchor = gscream_amd.anchor_adjust.prune_anchor

fp32 CUDA tensors take gscream_amd/csrc/anchor_adjust.hip:

    gsr_anchor_adjust_offsets   grads_norm = |offset_gradient_accum / offset_denom| (NaN -> 0), offset_mask          :916-919
    anchor_growing.anchor_growing(model, grads_norm, grad_threshold, offset_mask)      unchanged, looked up at call time :921
    gsr_anchor_adjust_plan      prune / reset per anchor, the kept rows in ascending order, info = n_keep, n_prune, n_reset
    info.tolist()               the ONE read-back the pruning half adds: the new tensors need n_keep to be allocated
    gsr_anchor_adjust_gather    one launch: every parameter, Adam moment and accumulator moves its kept rows; the offset
                                resets and zero padding (:924-934), the anchor resets (:953-956) and the clamp of
                                scaling[:, 3:] at 0.05 (:776-780) ride on it
    the optimiser is re-keyed as _prune_anchor_optimizer does: groups whose name contains mlp / conv / feat_base are skipped,
    a new nn.Parameter replaces each remaining group's one parameter, the old state dict object moves to the new key (`step`
    kept), a group without state gets the parameter only.  New parameters have .grad None, as in the reference.

The thresholds are the reference's Python products (check_interval*success_threshold*0.5, check_interval*success_threshold)
rounded to fp32: torch compares a float tensor with a Python scalar in fp32.  min_opacity*anchor_demon is one fp32 product.

CPU tensors, non-fp32 tensors or `force_torch = True` (module attribute) take `_adjust_torch` / `_prune_torch`: the reference's
expression sequence in its order (it synchronises at every boolean mask).  `last_path` is "hip" or "torch".  A missing library
raises; nothing falls back quietly."""
import numpy as np
import torch
from torch import nn

from . import _native
from . import anchor_growing as _grow

__all__ = ["adjust_anchor", "prune_anchor"]

PARAMS = ("anchor", "offset", "anchor_feat", "opacity", "uncertainty", "scaling", "rotation")  # what prune_anchor assigns (:799-805)
ANCHOR_STATS = ("opacity_accum", "uncertainty_accum", "anchor_demon")
BLOCK_ANCHORS = 256  # anchors per block of the compaction kernels (anchor_adjust.hip GAA_THREADS)
force_torch = False
last_path = None  # "hip" / "torch": the path the last adjust_anchor() / prune_anchor() took


def _skipped(group):
    return "mlp" in group["name"] or "conv" in group["name"] or "feat_base" in group["name"]


def _check_shapes(model, N, L0=None):
    """The shapes the reference's indexing would trip over, as ValueError (before anything is changed)."""
    for group in model.optimizer.param_groups:
        if not _skipped(group) and int(group["params"][0].shape[0]) != N:
            raise ValueError(f"parameter group {group['name']!r} has {int(group['params'][0].shape[0])} rows, the model has {N} anchors")
    for a in ANCHOR_STATS:
        if int(getattr(model, a).numel()) != N:
            raise ValueError(f"{a} has {int(getattr(model, a).numel())} entries, the model has {N} anchors")
    if L0 is not None:
        for a in ("offset_denom", "offset_gradient_accum"):
            if int(getattr(model, a).numel()) != L0:
                raise ValueError(f"{a} has {int(getattr(model, a).numel())} entries, expected anchors * n_offsets = {L0}")


def _hip_ok(model, with_stats):
    ts = []
    for group in model.optimizer.param_groups:
        if _skipped(group):
            continue
        p = group["params"][0]
        st = model.optimizer.state.get(p, None)
        ts += [p] + ([st["exp_avg"], st["exp_avg_sq"]] if st is not None else [])
    if with_stats:
        ts += [getattr(model, a) for a in ANCHOR_STATS + ("offset_denom", "offset_gradient_accum")]
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)


# ---- the torch path: the reference's expressions, in its order --------------------------------------------------------------
def _prune_optimizer_torch(model, mask):  # :762-792
    optimizable_tensors = {}
    for group in model.optimizer.param_groups:
        if _skipped(group):
            continue
        stored_state = model.optimizer.state.get(group["params"][0], None)
        if stored_state is not None:
            stored_state["exp_avg"] = stored_state["exp_avg"][mask]
            stored_state["exp_avg_sq"] = stored_state["exp_avg_sq"][mask]
            del model.optimizer.state[group["params"][0]]
            group["params"][0] = nn.Parameter(group["params"][0][mask].requires_grad_(True))
            model.optimizer.state[group["params"][0]] = stored_state
        else:
            group["params"][0] = nn.Parameter(group["params"][0][mask].requires_grad_(True))
        if group["name"] == "scaling":
            temp = group["params"][0][:, 3:]
            temp[temp > 0.05] = 0.05
            group["params"][0][:, 3:] = temp
        optimizable_tensors[group["name"]] = group["params"][0]
    return optimizable_tensors


def _prune_torch(model, mask):  # :794-805
    optimizable_tensors = _prune_optimizer_torch(model, ~mask)
    for p in PARAMS:
        setattr(model, "_" + p, optimizable_tensors[p])


def _adjust_torch(model, check_interval, success_threshold, grad_threshold, min_opacity):  # :914-973
    grads = model.offset_gradient_accum / model.offset_denom
    grads[grads.isnan()] = 0.0
    grads_norm = torch.norm(grads, dim=-1)
    offset_mask = (model.offset_denom > check_interval * success_threshold * 0.5).squeeze(dim=1)

    _grow.anchor_growing(model, grads_norm, grad_threshold, offset_mask)

    K = model.n_offsets
    for name in ("offset_denom", "offset_gradient_accum"):
        t = getattr(model, name)
        t[offset_mask] = 0
        pad = torch.zeros([model.get_anchor.shape[0] * K - t.shape[0], 1], dtype=torch.int32, device=t.device)
        setattr(model, name, torch.cat([t, pad], dim=0))

    prune_mask = (model.opacity_accum < min_opacity * model.anchor_demon).squeeze(dim=1)
    anchors_mask = (model.anchor_demon > check_interval * success_threshold).squeeze(dim=1)
    prune_mask = torch.logical_and(prune_mask, anchors_mask)

    for name in ("offset_denom", "offset_gradient_accum"):
        setattr(model, name, getattr(model, name).view([-1, K])[~prune_mask].view([-1, 1]))

    if anchors_mask.sum() > 0:
        for name in ANCHOR_STATS:
            t = getattr(model, name)
            t[anchors_mask] = torch.zeros([anchors_mask.sum(), 1], device=t.device).float()
    for name in ANCHOR_STATS:
        setattr(model, name, getattr(model, name)[~prune_mask])

    if prune_mask.shape[0] > 0:
        _prune_torch(model, prune_mask)
    model.max_radii2D = torch.zeros((model.get_anchor.shape[0]), device=model.get_anchor.device)


# ---- the HIP path ----------------------------------------------------------------------------------------------------------
def _offsets_hip(accum, denom, threshold):
    """-> (grads_norm [L0] fp32, offset_mask [L0] bool) of :916-919; `threshold` is the Python product, rounded to fp32 here."""
    dev, L0 = denom.device, int(denom.numel())
    accum, denom = accum.detach().reshape(-1).contiguous(), denom.detach().reshape(-1).contiguous()
    grads_norm = torch.empty(L0, dtype=torch.float32, device=dev)
    offset_mask = torch.empty(L0, dtype=torch.bool, device=dev)
    _native.run("gsr_anchor_adjust_offsets", dev, L0, _native.ptr(accum), _native.ptr(denom), float(np.float32(threshold)),
                _native.ptr(grads_norm), _native.ptr(offset_mask))
    return grads_norm, offset_mask


def _plan_hip(N, dev, opacity_accum=None, anchor_demon=None, prune_mask=None, min_opacity=0.0, threshold=0.0):
    """-> (keep_rows [N] int32: the first info[0] entries are the kept anchors, ascending; reset [N] bool; info [4] int32 =
    n_keep, n_prune, n_reset, 0), all on the device; nothing is read back."""
    lib = _native.load()
    keep_rows = torch.zeros(N, dtype=torch.int32, device=dev)  # (zeros: entries from n_keep on stay valid row numbers)
    reset = torch.empty(N, dtype=torch.bool, device=dev)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.gsr_anchor_adjust_workspace_bytes(N)), dtype=torch.uint8, device=dev)
    if prune_mask is not None:
        pm = prune_mask.detach().reshape(-1)
        pm = (pm.view(torch.uint8) if pm.dtype == torch.bool else (pm != 0).view(torch.uint8)).contiguous()
        acc = dem = None
    else:
        pm = None
        acc, dem = opacity_accum.detach().reshape(-1).contiguous(), anchor_demon.detach().reshape(-1).contiguous()
    _native.run("gsr_anchor_adjust_plan", dev, N, _native.ptr(acc), _native.ptr(dem), _native.ptr(pm), float(np.float32(min_opacity)),
                float(np.float32(threshold)), _native.ptr(ws), _native.ptr(keep_rows), _native.ptr(reset), _native.ptr(info))
    return keep_rows, reset, info


def _gather_hip(N, n_keep, copies, keep_rows, offset_mask, L0, reset):
    """copies: [(src, dst, width, mode)] with contiguous fp32 tensors; one launch per GSR_ADJUST_MAX_COPIES of them."""
    dev = keep_rows.device
    for i in range(0, len(copies), _native.ADJUST_MAX_COPIES):
        part = copies[i:i + _native.ADJUST_MAX_COPIES]
        table = (_native.AdjustCopy * len(part))()
        for d, (src, dst, width, mode) in zip(table, part):
            d.src, d.dst, d.width, d.mode = (src.data_ptr() if src.numel() else None), (dst.data_ptr() if dst.numel() else None), width, mode
        _native.run("gsr_anchor_adjust_gather", dev, N, n_keep, len(part), table, _native.ptr(keep_rows), _native.ptr(offset_mask), L0,
                    _native.ptr(reset))


def _apply_hip(model, n_keep, keep_rows, reset=None, offset_mask=None, L0=0):
    """Gather every tensor's kept rows into new tensors and re-key the optimiser (no host stop: n_keep is the host's).
    reset given = adjust_anchor (the five accumulators move too, max_radii2D is renewed); None = the standalone prune_anchor."""
    N, dev = int(keep_rows.shape[0]), keep_rows.device
    new = lambda old: torch.empty((n_keep,) + tuple(old.shape[1:]), dtype=torch.float32, device=dev)
    copies, keyed = [], []
    for group in model.optimizer.param_groups:
        if _skipped(group):
            continue
        old = group["params"][0]
        state = model.optimizer.state.get(old, None)
        width = int(old.numel() // N)
        mode = _native.ADJUST_CLAMP_TAIL if group["name"] == "scaling" else _native.ADJUST_COPY
        dst = [new(old)]
        copies.append((old.detach().contiguous(), dst[0], width, mode))
        if state is not None:
            for s in ("exp_avg", "exp_avg_sq"):
                if state[s].shape != old.shape:
                    raise ValueError(f"optimizer state {s!r} of group {group['name']!r} has shape {tuple(state[s].shape)}, "
                                     f"its parameter {tuple(old.shape)}")
                dst.append(new(old))
                copies.append((state[s].detach().contiguous(), dst[-1], width, _native.ADJUST_COPY))
        keyed.append((group, old, state, dst))
    stats = {}
    if reset is not None:
        K = int(model.n_offsets)
        for name in ("offset_denom", "offset_gradient_accum"):
            stats[name] = torch.empty((n_keep * K, 1), dtype=torch.float32, device=dev)
            copies.append((getattr(model, name).detach().reshape(-1).contiguous(), stats[name], K, _native.ADJUST_OFFSET_STAT))
        for name in ANCHOR_STATS:
            stats[name] = torch.empty((n_keep, 1), dtype=torch.float32, device=dev)
            copies.append((getattr(model, name).detach().reshape(-1).contiguous(), stats[name], 1, _native.ADJUST_ANCHOR_STAT))
    _gather_hip(N, n_keep, copies, keep_rows, offset_mask, L0, reset)
    optimizable_tensors = {}
    for group, old, state, dst in keyed:
        param = nn.Parameter(dst[0].requires_grad_(True))
        if state is not None:
            state["exp_avg"], state["exp_avg_sq"] = dst[1], dst[2]
            del model.optimizer.state[old]
            group["params"][0] = param
            model.optimizer.state[param] = state
        else:
            group["params"][0] = param
        optimizable_tensors[group["name"]] = param
    for p in PARAMS:
        setattr(model, "_" + p, optimizable_tensors[p])
    for name, t in stats.items():
        setattr(model, name, t)
    if reset is not None:
        model.max_radii2D = torch.zeros(n_keep, device=dev)


def _adjust_hip(model, check_interval, success_threshold, grad_threshold, min_opacity, info=None):
    """`info`: the host's (n_keep, n_prune, n_reset, 0) when the caller already knows it (tests); None = read it back."""
    K = int(model.n_offsets)
    dev = model.offset_denom.device
    offset_denom, offset_gradient_accum = model.offset_denom, model.offset_gradient_accum
    L0 = int(offset_denom.numel())
    with _native.on_device(dev.index):
        grads_norm, offset_mask = _offsets_hip(offset_gradient_accum, offset_denom, check_interval * success_threshold * 0.5)
        _grow.anchor_growing(model, grads_norm, grad_threshold, offset_mask)
        N = int(model.get_anchor.shape[0])
        _check_shapes(model, N)
        if L0 > N * K or int(model.offset_denom.numel()) != L0 or int(model.offset_gradient_accum.numel()) != L0:
            raise ValueError(f"the offset statistics must keep their {L0} entries while the anchors grow (now {N} anchors, "
                             f"offset_denom {int(model.offset_denom.numel())}, offset_gradient_accum {int(model.offset_gradient_accum.numel())})")
        keep_rows, reset, info_dev = _plan_hip(N, dev, model.opacity_accum, model.anchor_demon, None, min_opacity,
                                               check_interval * success_threshold)
        n_keep = int((info_dev.tolist() if info is None else info)[0])  # the one host stop of the pruning half
        if N > 0:
            _apply_hip(model, n_keep, keep_rows, reset, offset_mask, L0)
        else:  # :970 `if prune_mask.shape[0] > 0`: the parameters stay the objects they are
            for name in ("offset_denom", "offset_gradient_accum") + ANCHOR_STATS:
                setattr(model, name, torch.empty((0, 1), dtype=torch.float32, device=dev))
            model.max_radii2D = torch.zeros(0, device=dev)
    return info_dev


def adjust_anchor(model, check_interval=100, success_threshold=0.8, grad_threshold=0.0002, min_opacity=0.005):
    global last_path
    N0 = int(model.get_anchor.shape[0])
    _check_shapes(model, N0, N0 * int(model.n_offsets))
    if force_torch or not _hip_ok(model, True):
        last_path = "torch"
        _adjust_torch(model, check_interval, success_threshold, grad_threshold, min_opacity)
        return
    last_path = "hip"
    _adjust_hip(model, check_interval, success_threshold, grad_threshold, min_opacity)


def prune_anchor(model, mask):
    global last_path
    N = int(model.get_anchor.shape[0])
    if mask.dim() != 1 or int(mask.shape[0]) != N:
        raise ValueError(f"mask must be [N] with N = {N} anchors, got {tuple(mask.shape)}")
    for group in model.optimizer.param_groups:
        if not _skipped(group) and int(group["params"][0].shape[0]) != N:
            raise ValueError(f"parameter group {group['name']!r} has {int(group['params'][0].shape[0])} rows, the model has {N} anchors")
    if force_torch or not (mask.is_cuda and _hip_ok(model, False)) or N == 0:
        last_path = "torch"
        _prune_torch(model, mask.bool())
        return
    last_path = "hip"
    dev = mask.device
    with _native.on_device(dev.index):
        keep_rows, _reset, info = _plan_hip(N, dev, prune_mask=mask)
        _apply_hip(model, int(info.tolist()[0]), keep_rows)
