"""Bidirectional cross-attention, the CPU side: the drop-in package, the module's contract (parameter names, forward semantics on the
torch path, which CPU tensors take), run_crossattn on a stand-in model, the optimizer group and schedule, and the C symbols.
The GPU side (the HIP attention core) is tests/test_gpu_crossattn.py.

Tolerance of the fp32-module-vs-fp64-restatement comparisons: 3e-5 * max|reference| per tensor = 512 * 2^-24, the worst-case
linear rounding bound of the longest reduction in the chain (the 512-wide output projection); the sizes here are far below 512
everywhere else."""
import os
import sys
import types

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crossattn_helpers as CH  # noqa: E402

NEW_SYMBOLS = ("gsr_crossattn_workspace_bytes", "gsr_crossattn_forward", "gsr_crossattn_backward")
RTOL = 512 * 2.0 ** -24


def make(seed=0, **kw):
    from bidirectional_cross_attention import BidirectionalCrossAttention
    torch.manual_seed(seed)
    args = dict(dim=32, heads=8, dim_head=64, context_dim=32)
    args.update(kw)
    return BidirectionalCrossAttention(**args)


def inputs(i, j, b=1, seed=1, dim=32, cdim=32):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(b, i, dim), r(b, j, cdim), r(b, i, dim), r(b, j, cdim)


def assert_close(got, ref, what):
    for k, v in got.items():
        err = float((v.double() - ref[k]).abs().max())
        bound = RTOL * float(ref[k].abs().max())
        assert err <= bound, (what, k, err, bound)


def test_state_dict_is_the_eight_tensors_of_the_package():
    m = make()
    want = {"to_qk.weight": (512, 32), "context_to_qk.weight": (512, 32), "to_v.weight": (512, 32), "context_to_v.weight": (512, 32),
            "to_out.weight": (32, 512), "to_out.bias": (32,), "context_to_out.weight": (32, 512), "context_to_out.bias": (32,)}
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert len(list(m.parameters())) == 8
    assert m.scale == 64 ** -0.5
    assert isinstance(m.norm, nn.Identity) and isinstance(m.talking_heads, nn.Identity) and isinstance(m.dropout, nn.Dropout)
    full = make(dim=16, context_dim=24, heads=2, dim_head=8, dropout=0.1, talking_heads=True, prenorm=True)
    keys = set(full.state_dict())
    assert {"norm.weight", "norm.bias", "context_norm.weight", "context_norm.bias", "talking_heads.weight",
            "context_talking_heads.weight"} <= keys
    assert tuple(full.talking_heads.weight.shape) == (2, 2, 1, 1) and full.context_to_out.out_features == 24
    assert full.dropout.p == 0.1 and full.context_dropout.p == 0.1


@pytest.mark.parametrize("case", ["no_masks", "all_true_masks", "partial_masks", "i_ne_j", "prenorm_talking", "context_mask_only"])
def test_module_on_cpu_equals_the_fp64_restatement(case):
    i, j, b = (9, 9, 2)
    kw, mkw = {}, {}
    if case == "i_ne_j":
        i, j = 5, 13
    if case == "prenorm_talking":
        mkw = dict(prenorm=True, talking_heads=True)
    m = make(**mkw)
    x, c, g1, g2 = inputs(i, j, b)
    if case == "all_true_masks":
        kw = dict(mask=torch.ones(b, i, dtype=torch.bool), context_mask=torch.ones(b, j, dtype=torch.bool))
    if case == "partial_masks":
        mask, cmask = torch.ones(b, i, dtype=torch.bool), torch.ones(b, j, dtype=torch.bool)
        mask[0, 2] = False          # one fully masked row of sim (uniform attn row)
        cmask[0, 4:6] = False
        cmask[1, 0] = False
        mask[1, 7] = False
        kw = dict(mask=mask, context_mask=cmask)
    if case == "context_mask_only":
        cmask = torch.ones(b, j, dtype=torch.bool)
        cmask[:, 1] = False
        kw = dict(context_mask=cmask)
    got = CH.run_module(m, x, c, g1, g2, **kw)
    assert m.last_path == "torch"  # CPU tensors never reach the HIP core
    ref = CH.run_ref(m, x, c, g1, g2, **kw)
    assert_close(got, ref, case)
    if case == "partial_masks":   # the fully masked row averages the context values uniformly
        assert float((ref["attn"][0, :, 2] - 1.0 / j).abs().max()) < 1e-12


def test_return_attn_gives_both_softmaxes():
    m = make()
    x, c, g1, g2 = inputs(6, 11)
    out, cout, attn, cattn = m(x, c, return_attn=True)
    assert attn.shape == (1, 8, 6, 11) and cattn.shape == (1, 8, 6, 11)
    assert float((attn.detach().sum(-1) - 1).abs().max()) < 1e-5      # rows of attn
    assert float((cattn.detach().sum(-2) - 1).abs().max()) < 1e-5     # columns of context_attn
    ref = CH.run_ref(m, x, c, g1, g2)
    assert_close({"out": out.detach(), "context_out": cout.detach(), "attn": attn.detach(), "context_attn": cattn.detach()}, ref, "attn")


def test_rel_pos_bias_and_fixed_dropout_match_the_restatement():
    m = make(heads=4, dim_head=16)
    x, c, g1, g2 = inputs(7, 5)
    bias = torch.randn(1, 4, 7, 5, generator=torch.Generator().manual_seed(3))
    assert_close(CH.run_module(m, x, c, g1, g2, rel_pos_bias=bias), CH.run_ref(m, x, c, g1, g2, rel_pos_bias=bias), "rel_pos_bias")
    g = torch.Generator().manual_seed(4)
    keep, ckeep = torch.rand(1, 4, 7, 5, generator=g) > 0.25, torch.rand(1, 4, 7, 5, generator=g) > 0.25
    m.dropout, m.context_dropout = CH.FixedDropout(0.25, keep), CH.FixedDropout(0.25, ckeep)
    m.train()
    assert_close(CH.run_module(m, x, c, g1, g2), CH.run_ref(m, x, c, g1, g2, drop=(keep, ckeep, 0.25)), "dropout")
    m.eval()
    assert_close(CH.run_module(m, x, c, g1, g2), CH.run_ref(m, x, c, g1, g2), "dropout in eval mode")


# ---- run_crossattn on a stand-in model ---------------------------------------------------------------------------------
def standin(N=40, seed=0, plain=False):
    """What run_crossattn reads from GaussianModel: `_anchor_feat` and `crossattn`.  plain: a bare namespace with a tensor attribute
    (the reference's GaussianModel is no nn.Module); otherwise the project's stand-in model, whose `_anchor_feat` is a Parameter."""
    feat = torch.randn(N, 32, generator=torch.Generator().manual_seed(seed))
    if plain:
        m = types.SimpleNamespace(_anchor_feat=feat.clone().requires_grad_(True))
    else:
        from gscream_amd import standin_model as SM
        m = SM.Model(N, K=2, dtype=torch.float32)
        with torch.no_grad():
            m._anchor_feat.copy_(feat)
    m.crossattn = make(seed=5)
    fg, bg = torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
    fg[[1, 4, 5, 9, 20, 33]] = True
    bg[[0, 2, 7, 8, 21, 22, 23, 39]] = True
    return m, feat, fg, bg


@pytest.mark.parametrize("plain", [False, True])
@pytest.mark.parametrize("is_ref,ema", [(True, 1.0), (True, 0.03), (False, 0.03)])
def test_run_crossattn_writes_back_like_the_reference(plain, is_ref, ema):
    from gscream_amd import crossattn as CA
    m, old, fg, bg = standin(plain=plain)
    old_leaf = m._anchor_feat
    with torch.no_grad():
        fo, bo = m.crossattn(old[fg][None], old[bg][None], mask=torch.ones(1, int(fg.sum()), dtype=torch.bool),
                             context_mask=torch.ones(1, int(bg.sum()), dtype=torch.bool))
    assert CA.run_crossattn(m, fg, bg, ema=ema, is_ref=is_ref) is None
    new = m._anchor_feat
    rest = ~(fg | bg)
    assert torch.equal(new[rest], old[rest])                                  # untouched rows: bitwise
    assert torch.equal(new[bg].detach(), (ema * bo[0] + (1 - ema) * old[bg]))  # the background rows are always written
    if is_ref:
        assert torch.equal(new[fg].detach(), (ema * fo[0] + (1 - ema) * old[fg]))
    else:
        assert torch.equal(new[fg], old[fg])
    # the new feature tensor carries a graph to the eight attention parameters and none to the old feature tensor
    assert new.requires_grad and new.grad_fn is not None and new.retains_grad
    w = torch.randn(new.shape, generator=torch.Generator().manual_seed(9))
    (new * w).sum().backward()
    live = {k for k, p in m.crossattn.named_parameters() if p.grad is not None and float(p.grad.abs().max()) > 0}
    assert all(torch.isfinite(p.grad).all() for p in m.crossattn.parameters() if p.grad is not None)
    # the background rows are context_out = context_to_out(softmax_i(sim)^T to_v(x)); the foreground rows add context_to_v and to_out
    through_bg = {"to_qk.weight", "context_to_qk.weight", "to_v.weight", "context_to_out.weight", "context_to_out.bias"}
    assert live == (set(dict(m.crossattn.named_parameters())) if is_ref else through_bg), live
    assert len(live) == (8 if is_ref else 5)
    assert old_leaf.grad is None
    assert torch.equal(new.grad, w)


def test_run_crossattn_refuses_pe():
    from gscream_amd import crossattn as CA
    m, _old, fg, bg = standin()
    with pytest.raises(NotImplementedError):
        CA.run_crossattn(m, fg, bg, pe=True)
    with pytest.raises(AssertionError):
        CA.run_crossattn(m, fg, bg[:-1])


def test_param_group_optimizer_and_schedule():
    from gscream_amd import crossattn as CA
    from gscream_amd import fit
    m, _old, _fg, _bg = standin()
    args = types.SimpleNamespace(crossattn_lr_init=0.01, crossattn_lr_final=0.00001, crossattn_lr_delay_mult=0.01, crossattn_lr_max_steps=30_000)
    groups = CA.crossattn_param_group(m, args)
    assert len(groups) == 1 and groups[0]["name"] == "crossattn" and groups[0]["lr"] == 0.01
    opt = CA.crossattn_optimizer(m, args)
    assert isinstance(opt, torch.optim.Adam) and len(opt.param_groups) == 1
    g = opt.param_groups[0]
    assert g["name"] == "crossattn" and g["lr"] == 0.01 and g["eps"] == 1e-15 and len(g["params"]) == 8
    assert {id(p) for p in g["params"]} == {id(p) for p in m.crossattn.parameters()}
    lr = lambda it, **kw: CA.crossattn_lr(it, args.crossattn_lr_init, args.crossattn_lr_final, args.crossattn_lr_delay_mult,
                                          args.crossattn_lr_max_steps, **kw)
    assert lr(0) == pytest.approx(0.01, rel=1e-12) and lr(30_000) == pytest.approx(0.00001, rel=1e-12)
    assert lr(45_000) == pytest.approx(0.00001, rel=1e-12) and lr(-1) == 0.0
    assert lr(15_000) == pytest.approx((0.01 * 0.00001) ** 0.5, rel=1e-12)     # log-linear in between
    for it in (0, 1, 777, 15_000, 29_999, 30_000):                             # = the project's schedule where there is no delay
        assert lr(it) == pytest.approx(fit.expon_lr(it, 0.01, 0.00001, 30_000), rel=1e-12)
    # get_expon_lr_func's delay term: lr_delay_mult at step 0, eased out by lr_delay_steps (the reference leaves lr_delay_steps at 0)
    assert lr(0, lr_delay_steps=100) == pytest.approx(0.01 * 0.01, rel=1e-12)
    assert lr(100, lr_delay_steps=100) == pytest.approx(fit.expon_lr(100, 0.01, 0.00001, 30_000), rel=1e-12)
    mid = 0.01 + 0.99 * 2 ** -0.5
    assert lr(50, lr_delay_steps=100) == pytest.approx(mid * fit.expon_lr(50, 0.01, 0.00001, 30_000), rel=1e-12)
    assert CA.crossattn_lr(5, 0.0, 0.0) == 0.0


def test_new_symbols_in_header_binding_and_library(native_lib):
    from gscream_amd import _abi, _native
    for s in NEW_SYMBOLS:
        assert s in _abi.header().functions, s
        assert s in _native.EXPORTED_SYMBOLS, s
        assert hasattr(native_lib, s), s
    assert native_lib.gsr_abi_version() == 9
    assert native_lib.gsr_crossattn_workspace_bytes(1, 8, 2000, 2000) >= 8 * 4000 * 12
    assert native_lib.gsr_crossattn_workspace_bytes(1, 8, 0, 5) == 0
    # argument checks run before anything touches a device
    assert native_lib.gsr_crossattn_forward(1, 8, 4, 4, 32, *([None] * 6), 0.125, None, None, None, None) == -3   # dim_head != 64
    assert b"dim_head" in native_lib.gsr_last_error()
    assert native_lib.gsr_crossattn_forward(1, 8, 4, 4, 64, *([None] * 6), 0.125, None, None, None, None) == -1   # NULL pointers
    assert native_lib.gsr_crossattn_backward(1, 8, 0, 4, 64, *([None] * 6), 0.125, *([None] * 10)) == -1          # i = 0
