"""An independent fp64 restatement of BidirectionalCrossAttention's forward (bidirectional-cross-attention 0.0.4), for the
crossattn tests.  Written from the published semantics, with explicit matmuls per head instead of the module's einsums: the
module under test (either path) is never its own yardstick."""
import torch
import torch.nn.functional as F


class FixedDropout(torch.nn.Dropout):
    """nn.Dropout with a keep-mask chosen by the test instead of drawn: the restatement can then apply the same one."""

    def __init__(self, p, keep):
        super().__init__(p)
        self.keep = keep

    def forward(self, t):
        return t * self.keep.to(t.dtype) / (1.0 - self.p) if self.training and self.p > 0 else t


def params64(module):
    """The module's state in float64, detached leaves that require grad (keyed like state_dict())."""
    return {k: v.detach().double().clone().requires_grad_(True) for k, v in module.state_dict().items()}


def ref_forward(p, x, context, heads, mask=None, context_mask=None, rel_pos_bias=None, dim_head=None, drop=None):
    """-> (out, context_out, attn, context_attn) in the dtype of `p` / `x` (call it with float64).  drop = (keep, context_keep, p):
    the two dropout keep-masks [b, h, i, j] of a training-mode call and its rate (see FixedDropout)."""
    b, i, _ = x.shape
    j = context.shape[1]
    if "norm.weight" in p:
        x = F.layer_norm(x, x.shape[-1:], p["norm.weight"], p["norm.bias"])
        context = F.layer_norm(context, context.shape[-1:], p["context_norm.weight"], p["context_norm.bias"])
    inner = p["to_qk.weight"].shape[0]
    d = inner // heads if dim_head is None else dim_head
    proj = lambda t, n, w: (t @ p[w].t()).view(b, n, heads, d).transpose(1, 2)  # noqa: E731  [b, h, n, d]
    qk, v = proj(x, i, "to_qk.weight"), proj(x, i, "to_v.weight")
    cqk, cv = proj(context, j, "context_to_qk.weight"), proj(context, j, "context_to_v.weight")
    sim = torch.matmul(qk, cqk.transpose(-1, -2)) * (d ** -0.5)  # [b, h, i, j]
    if rel_pos_bias is not None:
        sim = sim + rel_pos_bias
    if mask is not None or context_mask is not None:
        m = torch.ones(b, i, dtype=torch.bool, device=x.device) if mask is None else mask.bool()
        cm = torch.ones(b, j, dtype=torch.bool, device=x.device) if context_mask is None else context_mask.bool()
        pair = m[:, None, :, None] & cm[:, None, None, :]
        sim = torch.where(pair, sim, torch.full_like(sim, -torch.finfo(torch.float32).max))
    attn = torch.softmax(sim, dim=3)
    context_attn = torch.softmax(sim, dim=2)
    if drop is not None:
        attn = attn * drop[0].to(attn.dtype) / (1.0 - drop[2])
        context_attn = context_attn * drop[1].to(attn.dtype) / (1.0 - drop[2])
    if "talking_heads.weight" in p:
        attn = torch.einsum("gh,bhij->bgij", p["talking_heads.weight"][:, :, 0, 0], attn)
        context_attn = torch.einsum("gh,bhij->bgij", p["context_talking_heads.weight"][:, :, 0, 0], context_attn)
    out = torch.matmul(attn, cv)                               # [b, h, i, d]
    cout = torch.matmul(context_attn.transpose(-1, -2), v)     # [b, h, j, d]
    out = out.transpose(1, 2).reshape(b, i, inner) @ p["to_out.weight"].t() + p["to_out.bias"]
    cout = cout.transpose(1, 2).reshape(b, j, inner) @ p["context_to_out.weight"].t() + p["context_to_out.bias"]
    return out, cout, attn, context_attn


def run_ref(module, x, context, g_out, g_cout, mask=None, context_mask=None, rel_pos_bias=None, drop=None):
    """fp64 values and gradients of sum(out * g_out) + sum(context_out * g_cout): -> dict name -> float64 tensor."""
    p = params64(module)
    x64 = x.detach().double().clone().requires_grad_(True)
    c64 = context.detach().double().clone().requires_grad_(True)
    rb = None if rel_pos_bias is None else rel_pos_bias.double()
    out, cout, attn, cattn = ref_forward(p, x64, c64, module.heads, mask, context_mask, rb, dim_head=module.dim_head, drop=drop)
    ((out * g_out.double()).sum() + (cout * g_cout.double()).sum()).backward()
    res = {"out": out.detach(), "context_out": cout.detach(), "attn": attn.detach(), "context_attn": cattn.detach(),
           "d_x": x64.grad, "d_context": c64.grad}
    res.update({"d_" + k: t.grad for k, t in p.items()})
    return res


def run_module(module, x, context, g_out, g_cout, **kw):
    """The same quantities from the module itself, in its own dtype (its .grad fields are reset first)."""
    module.zero_grad(set_to_none=True)
    xx = x.detach().clone().requires_grad_(True)
    cc = context.detach().clone().requires_grad_(True)
    out, cout = module(xx, cc, **kw)[:2]
    ((out * g_out).sum() + (cout * g_cout).sum()).backward()
    res = {"out": out.detach(), "context_out": cout.detach(), "d_x": xx.grad, "d_context": cc.grad}
    res.update({"d_" + k: t.grad.clone() for k, t in module.named_parameters()})
    return res
