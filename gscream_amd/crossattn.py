"""Bidirectional cross-attention (the cross-view feature propagation of GScream) with its attention core on the HIP path.

`BidirectionalCrossAttention` has the constructor, the parameter names and the forward of bidirectional-cross-attention 0.0.4 (the
version gscream.yaml pins; scene/gaussian_model.py:29 imports it, :161-167 builds it with dim = context_dim = 32, 8 heads of 64).
One similarity matrix between the two sequences is softmaxed along both axes; each side then attends to the other's values.

    qk, v = to_qk(x), to_v(x)                    context_qk, context_v likewise          (split heads b n (h d) -> b h n d)
    sim = einsum('bhid,bhjd->bhij', qk, context_qk) * scale  [+ rel_pos_bias]
    sim.masked_fill(~(mask[:, None, :, None] & context_mask[:, None, None, :]), -finfo.max)     (if either mask is given)
    attn, context_attn = sim.softmax(-1), sim.softmax(-2)        -> dropout -> talking heads
    out = einsum('bhij,bhjd->bhid', attn, context_v)             context_out = einsum('bhji,bhjd->bhid', context_attn, v)
    merge heads, to_out / context_to_out

Everything between the input and the output projections is the attention core.  For dim_head == 64, fp32 CUDA tensors, no active
dropout, no talking heads, no rel_pos_bias and return_attn=False -- the form GScream runs -- it is one HIP kernel per pass
(gsr_crossattn_forward / gsr_crossattn_backward: no [h, i, j] tensor is ever written, both directions in one launch, bit-reproducible).
Every other form runs the torch expressions above: a different form, not a missing kernel; a missing library on the HIP form raises.
`module.last_path` says which one the last call took ("hip" / "torch").

`run_crossattn`, `crossattn_param_group` and `crossattn_lr` are GaussianModel.run_crossattn (:553-583), the optimizer_c group (:396-409)
and its learning-rate schedule (:450-453).  `run_crossattn_rows` is run_crossattn on ascending row lists instead of boolean masks
(what gscream_amd/anchor_sampler.py produces): the same bits, no nonzero and so no host stop."""
import math

import torch
from torch import nn

from . import _native

__all__ = ["BidirectionalCrossAttention", "run_crossattn", "run_crossattn_rows", "crossattn_param_group", "crossattn_optimizer", "crossattn_lr"]

HIP_DIM_HEAD = 64


class _AttentionCore(torch.autograd.Function):
    """(qk, v, context_qk, context_v) [b, n, h * 64] -> (out [b, i, h * 64], context_out [b, j, h * 64]) through the C ABI."""

    @staticmethod
    def forward(ctx, qk, v, cqk, cv, mask, cmask, scale, heads):
        lib = _native.load()
        qk, v, cqk, cv = (t.detach().contiguous() for t in (qk, v, cqk, cv))
        B, I, J = int(qk.shape[0]), int(qk.shape[1]), int(cqk.shape[1])
        if mask is not None:
            mask = mask.detach().to(torch.bool).contiguous()
        if cmask is not None:
            cmask = cmask.detach().to(torch.bool).contiguous()
        out, cout = torch.empty_like(qk), torch.empty_like(cqk)
        ws = torch.empty(int(lib.gsr_crossattn_workspace_bytes(B, heads, I, J)), dtype=torch.uint8, device=qk.device)
        _native.run(
            "gsr_crossattn_forward", qk.device,
            B, heads, I, J, HIP_DIM_HEAD, _native.ptr(qk), _native.ptr(v), _native.ptr(cqk), _native.ptr(cv), _native.ptr(mask),
            _native.ptr(cmask), scale, _native.ptr(out), _native.ptr(cout), _native.ptr(ws))
        ctx.save_for_backward(qk, v, cqk, cv, out, cout, ws)
        ctx.masks, ctx.scale, ctx.heads = (mask, cmask), scale, heads
        return out, cout

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_cout):
        qk, v, cqk, cv, out, cout, ws = ctx.saved_tensors
        mask, cmask = ctx.masks
        B, I, J = int(qk.shape[0]), int(qk.shape[1]), int(cqk.shape[1])
        d_out, d_cout = d_out.contiguous(), d_cout.contiguous()
        grads = [torch.empty_like(t) for t in (qk, v, cqk, cv)]
        _native.run(
            "gsr_crossattn_backward", qk.device,
            B, ctx.heads, I, J, HIP_DIM_HEAD, _native.ptr(qk), _native.ptr(v), _native.ptr(cqk), _native.ptr(cv), _native.ptr(mask),
            _native.ptr(cmask), ctx.scale, _native.ptr(out), _native.ptr(cout), _native.ptr(d_out), _native.ptr(d_cout),
            _native.ptr(ws), _native.ptr(grads[0]), _native.ptr(grads[1]), _native.ptr(grads[2]), _native.ptr(grads[3]))
        return grads[0], grads[1], grads[2], grads[3], None, None, None, None


class BidirectionalCrossAttention(nn.Module):
    def __init__(self, *, dim, heads=8, dim_head=64, context_dim=None, dropout=0., talking_heads=False, prenorm=False):
        super().__init__()
        context_dim = dim if context_dim is None else context_dim
        self.norm = nn.LayerNorm(dim) if prenorm else nn.Identity()
        self.context_norm = nn.LayerNorm(context_dim) if prenorm else nn.Identity()
        self.heads = heads
        self.dim_head = dim_head
        self.scale = dim_head ** -0.5
        inner = dim_head * heads
        self.dropout = nn.Dropout(dropout)
        self.context_dropout = nn.Dropout(dropout)
        self.to_qk = nn.Linear(dim, inner, bias=False)
        self.context_to_qk = nn.Linear(context_dim, inner, bias=False)
        self.to_v = nn.Linear(dim, inner, bias=False)
        self.context_to_v = nn.Linear(context_dim, inner, bias=False)
        self.to_out = nn.Linear(inner, dim)
        self.context_to_out = nn.Linear(inner, context_dim)
        self.talking_heads = nn.Conv2d(heads, heads, 1, bias=False) if talking_heads else nn.Identity()
        self.context_talking_heads = nn.Conv2d(heads, heads, 1, bias=False) if talking_heads else nn.Identity()
        self.last_path = None        # "hip" / "torch": the path the last forward() took
        self.force_torch = False     # True: run the torch expressions even for the HIP form (tests, timing against eager)

    def _hip_form(self, x, context, return_attn, rel_pos_bias):
        if self.force_torch or return_attn or rel_pos_bias is not None or self.dim_head != HIP_DIM_HEAD:
            return False
        if (self.training and self.dropout.p > 0.) or not isinstance(self.talking_heads, nn.Identity):
            return False
        tensors = (x, context, self.to_qk.weight, self.to_v.weight, self.context_to_qk.weight, self.context_to_v.weight)
        return all(t.is_cuda and t.dtype == torch.float32 for t in tensors) and x.dim() == 3 and context.dim() == 3

    def forward(self, x, context, mask=None, context_mask=None, return_attn=False, rel_pos_bias=None):
        b, i, j, h = x.shape[0], x.shape[-2], context.shape[-2], self.heads
        x = self.norm(x)
        context = self.context_norm(context)
        qk, v = self.to_qk(x), self.to_v(x)
        context_qk, context_v = self.context_to_qk(context), self.context_to_v(context)

        if self._hip_form(x, context, return_attn, rel_pos_bias) and i > 0 and j > 0 and b > 0:
            self.last_path = "hip"
            out, context_out = _AttentionCore.apply(qk, v, context_qk, context_v, mask, context_mask, float(self.scale), h)
            return self.to_out(out), self.context_to_out(context_out)

        self.last_path = "torch"
        split = lambda t: t.reshape(b, t.shape[1], h, -1).permute(0, 2, 1, 3)    # b n (h d) -> b h n d
        qk, context_qk, v, context_v = map(split, (qk, context_qk, v, context_v))
        sim = torch.einsum('bhid,bhjd->bhij', qk, context_qk) * self.scale
        if rel_pos_bias is not None:
            sim = sim + rel_pos_bias
        if mask is not None or context_mask is not None:
            mask = torch.ones((b, i), device=x.device, dtype=torch.bool) if mask is None else mask
            context_mask = torch.ones((b, j), device=x.device, dtype=torch.bool) if context_mask is None else context_mask
            attn_mask = mask[:, None, :, None] & context_mask[:, None, None, :]
            sim = sim.masked_fill(~attn_mask, -torch.finfo(sim.dtype).max)
        attn = sim.softmax(dim=-1)
        context_attn = sim.softmax(dim=-2)
        attn = self.talking_heads(self.dropout(attn))
        context_attn = self.context_talking_heads(self.context_dropout(context_attn))
        out = torch.einsum('bhij,bhjd->bhid', attn, context_v)
        context_out = torch.einsum('bhji,bhjd->bhid', context_attn, v)
        merge = lambda t: t.permute(0, 2, 1, 3).reshape(b, t.shape[2], -1)       # b h n d -> b n (h d)
        out, context_out = self.to_out(merge(out)), self.context_to_out(merge(context_out))
        if return_attn:
            return out, context_out, attn, context_attn
        return out, context_out


def _rebind_anchor_feat(model, value):
    """`self._anchor_feat = tensor` of the reference (a plain attribute there).  An nn.Module refuses to replace a registered
    Parameter by a plain tensor, so on one (the stand-in model) the registration goes first; the optimizer keeps the old leaf, as it
    does in the reference."""
    params = getattr(model, "_parameters", None)
    if isinstance(params, dict) and "_anchor_feat" in params:
        del params["_anchor_feat"]
    model._anchor_feat = value


def run_crossattn(model, fg_anchor_mask, bg_anchor_mask, pe=False, ema=1.0, is_ref=True):
    """GaussianModel.run_crossattn (scene/gaussian_model.py:553-583), statement for statement.  Binds as
    `GaussianModel.run_crossattn = gscream_amd.crossattn.run_crossattn`; `model.crossattn` is the attention module."""
    assert fg_anchor_mask.shape == bg_anchor_mask.shape
    if pe:
        raise NotImplementedError("run_crossattn(pe=True): the positional-embedding branch is commented out in the reference (:561-563)")

    _rebind_anchor_feat(model, model._anchor_feat.detach())

    fg_feat = model._anchor_feat[fg_anchor_mask][None, :, :].clone()  # 1, N, 32
    bg_feat = model._anchor_feat[bg_anchor_mask][None, :, :].clone()  # 1, N, 32

    fg_feat_mask = torch.ones_like(fg_feat[:, :, 0]).bool()
    bg_feat_mask = torch.ones_like(bg_feat[:, :, 0]).bool()

    fg_feat_out, bg_feat_out = model.crossattn(fg_feat, bg_feat, mask=fg_feat_mask, context_mask=bg_feat_mask)

    if is_ref:  # only update the fg feature under reference view
        model._anchor_feat[fg_anchor_mask] = ema * fg_feat_out[0, :, :] + (1 - ema) * model._anchor_feat[fg_anchor_mask]
    # always update the bg feature
    model._anchor_feat[bg_anchor_mask] = ema * bg_feat_out[0, :, :] + (1 - ema) * model._anchor_feat[bg_anchor_mask]

    model._anchor_feat.retain_grad()
    return


def run_crossattn_rows(model, fg_rows, bg_rows, pe=False, ema=1.0, is_ref=True):
    """run_crossattn with the two anchor sets given as ASCENDING int64 row tensors (the nonzeros of its masks, in `feat[mask]` order):
    index_select / index_copy_ in the place of the boolean-mask gathers and assignments, each of which is a nonzero plus a size
    read-back.  Bit-identical to the mask form for the same sets, values and gradients."""
    assert fg_rows.dim() == 1 and bg_rows.dim() == 1 and fg_rows.dtype == bg_rows.dtype == torch.int64
    if pe:
        raise NotImplementedError("run_crossattn_rows(pe=True): the positional-embedding branch is commented out in the reference (:561-563)")

    _rebind_anchor_feat(model, model._anchor_feat.detach())

    fg_feat = model._anchor_feat.index_select(0, fg_rows)[None, :, :].clone()  # 1, N, 32
    bg_feat = model._anchor_feat.index_select(0, bg_rows)[None, :, :].clone()  # 1, N, 32

    fg_feat_mask = torch.ones_like(fg_feat[:, :, 0]).bool()
    bg_feat_mask = torch.ones_like(bg_feat[:, :, 0]).bool()

    fg_feat_out, bg_feat_out = model.crossattn(fg_feat, bg_feat, mask=fg_feat_mask, context_mask=bg_feat_mask)

    if is_ref:  # only update the fg feature under reference view
        model._anchor_feat.index_copy_(0, fg_rows, ema * fg_feat_out[0, :, :] + (1 - ema) * model._anchor_feat.index_select(0, fg_rows))
    # always update the bg feature
    model._anchor_feat.index_copy_(0, bg_rows, ema * bg_feat_out[0, :, :] + (1 - ema) * model._anchor_feat.index_select(0, bg_rows))

    model._anchor_feat.retain_grad()
    return


def crossattn_param_group(model, training_args):
    """The one group of optimizer_c (scene/gaussian_model.py:396-398)."""
    return [{"params": model.crossattn.parameters(), "lr": training_args.crossattn_lr_init, "name": "crossattn"}]


def crossattn_optimizer(model, training_args):
    """optimizer_c (:409)."""
    return torch.optim.Adam(crossattn_param_group(model, training_args), lr=0.0, eps=1e-15)


def crossattn_lr(iteration, lr_init=0.01, lr_final=0.00001, lr_delay_mult=0.01, max_steps=30_000, lr_delay_steps=0):
    """crossattn_scheduler_args(iteration) (scene/gaussian_model.py:450-453): utils/general_utils.py:104-137 get_expon_lr_func with its
    delay term (fit.expon_lr is the same function without it).  The defaults are arguments/__init__.py:147-150; the reference never
    passes lr_delay_steps, so lr_delay_mult is inert there, as it is here unless lr_delay_steps > 0."""
    if iteration < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    if lr_delay_steps > 0:
        delay_rate = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(iteration / lr_delay_steps, 0.0), 1.0))
    else:
        delay_rate = 1.0
    t = min(max(iteration / max_steps, 0.0), 1.0)
    return delay_rate * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
