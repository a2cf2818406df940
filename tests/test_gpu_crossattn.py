"""The HIP attention core of BidirectionalCrossAttention on the device (gsr_crossattn_forward / gsr_crossattn_backward).

Accuracy is judged against the fp64 restatement (tests/crossattn_helpers.py) with the eager fp32 torch path of the same module as
the yardstick, per output tensor and per gradient tensor (x, context and all eight parameters):

    e_ref = max|eager_fp32 - fp64|      e_hip = max|hip - fp64|      require  e_hip <= 4 * e_ref + 1e-7 * max|fp64|

The factor 4 allows a different but equally valid summation order across up to 2000 terms, the floor covers tensors where eager
happens to be exact.  Every figure is printed before it is asserted (run with -s to see them)."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import crossattn_helpers as CH  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make(seed=0, weight_mul=1.0, **kw):
    from bidirectional_cross_attention import BidirectionalCrossAttention
    torch.manual_seed(seed)
    args = dict(dim=32, heads=8, dim_head=64, context_dim=32)
    args.update(kw)
    m = BidirectionalCrossAttention(**args)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(weight_mul)
    return m.to(DEV)


def inputs(i, j, b=1, seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return r(b, i, 32), r(b, j, 32), r(b, i, 32), r(b, j, 32)


def check_4x(hip, eager, ref, what):
    """The rule of the module docstring, for every tensor of `hip`.  -> the worst e_hip / max(e_ref, floor) ratio."""
    worst, failures = 0.0, []
    for k, v in hip.items():
        r = ref[k]
        e_hip = float((v.double() - r).abs().max())
        e_ref = float((eager[k].double() - r).abs().max())
        floor = 1e-7 * float(r.abs().max())
        bound = 4.0 * e_ref + floor
        ratio = e_hip / max(e_ref, floor, 1e-300)
        worst = max(worst, ratio)
        print(f"{what:28s} {k:28s} e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  max|fp64| {float(r.abs().max()):.3e}  e_hip/e_ref {ratio:.2f}")
        assert np.isfinite(e_hip), (what, k)
        if not e_hip <= bound:
            failures.append((k, e_hip, e_ref, bound))
    assert not failures, (what, failures)
    return worst


def three_ways(m, x, c, g1, g2, **kw):
    m.force_torch = False
    hip = CH.run_module(m, x, c, g1, g2, **kw)
    assert m.last_path == "hip"
    m.force_torch = True
    eager = CH.run_module(m, x, c, g1, g2, **kw)
    assert m.last_path == "torch"
    m.force_torch = False
    ref = CH.run_ref(m, x, c, g1, g2, **kw)
    return hip, eager, ref


@pytest.mark.parametrize("weight_mul", [1.0, 8.0])
@pytest.mark.parametrize("b,i,j", [(1, 2000, 2000), (1, 12, 12), (1, 777, 1301), (1, 1, 5), (1, 2000, 37), (2, 300, 450)])
def test_hip_core_against_fp64_with_eager_as_yardstick(b, i, j, weight_mul):
    m = make(weight_mul=weight_mul)
    x, c, g1, g2 = inputs(i, j, b)
    hip, eager, ref = three_ways(m, x, c, g1, g2)
    assert len(hip) == 12  # out, context_out, d_x, d_context, eight parameter gradients
    check_4x(hip, eager, ref, f"b{b} {i}x{j} w*{weight_mul:g}")


@pytest.mark.parametrize("weight_mul", [1.0, 8.0])
def test_masked_pairs_and_fully_masked_rows_and_columns(weight_mul):
    b, i, j = 2, 197, 131
    m = make(weight_mul=weight_mul)
    x, c, g1, g2 = inputs(i, j, b, seed=2)
    g = torch.Generator().manual_seed(7)
    mask = (torch.rand(b, i, generator=g) > 0.2).to(DEV)     # every False entry is a fully masked row of sim
    cmask = (torch.rand(b, j, generator=g) > 0.2).to(DEV)    # ... a fully masked column
    mask[0, 0], mask[1, i - 1], cmask[0, j - 1], cmask[1, 64] = False, False, False, False
    hip, eager, ref = three_ways(m, x, c, g1, g2, mask=mask, context_mask=cmask)
    check_4x(hip, eager, ref, f"masked w*{weight_mul:g}")
    hip, eager, ref = three_ways(m, x, c, g1, g2, mask=mask)  # the missing mask is filled with ones
    check_4x(hip, eager, ref, f"x mask only w*{weight_mul:g}")
    none_true = torch.zeros(b, j, dtype=torch.bool, device=DEV)  # everything masked: both directions are uniform averages
    hip, eager, ref = three_ways(m, x, c, g1, g2, context_mask=none_true)
    check_4x(hip, eager, ref, f"all masked w*{weight_mul:g}")


def test_prenorm_stays_on_the_hip_path():
    m = make(prenorm=True)
    x, c, g1, g2 = inputs(150, 90)
    hip, eager, ref = three_ways(m, x, c, g1, g2)
    assert len(hip) == 16  # the four LayerNorm tensors as well
    check_4x(hip, eager, ref, "prenorm")


def test_two_runs_are_bit_identical():
    m = make(weight_mul=8.0)
    x, c, g1, g2 = inputs(2000, 1777)
    mask = (torch.rand(1, 2000, generator=torch.Generator().manual_seed(3)) > 0.1).to(DEV)
    a = CH.run_module(m, x, c, g1, g2, mask=mask)
    b = CH.run_module(m, x, c, g1, g2, mask=mask)
    assert m.last_path == "hip"
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_forms_outside_the_hip_path_run_torch_and_match_the_restatement():
    x, c, g1, g2 = inputs(60, 45)
    tol = lambda got, ref, what: [  # noqa: E731  (fp32 torch against fp64: 512 * 2^-24 of the tensor's scale, as in the CPU tests)
        pytest.fail(f"{what} {k}") for k, v in got.items() if float((v.double() - ref[k]).abs().max()) > 512 * 2.0 ** -24 * float(ref[k].abs().max())]
    m = make(dim_head=32)
    got = CH.run_module(m, x, c, g1, g2)
    assert m.last_path == "torch"
    tol(got, CH.run_ref(m, x, c, g1, g2), "dim_head=32")
    m = make(talking_heads=True)
    got = CH.run_module(m, x, c, g1, g2)
    assert m.last_path == "torch"
    tol(got, CH.run_ref(m, x, c, g1, g2), "talking_heads")
    m = make()
    bias = torch.randn(1, 8, 60, 45, generator=torch.Generator().manual_seed(3)).to(DEV)
    got = CH.run_module(m, x, c, g1, g2, rel_pos_bias=bias)
    assert m.last_path == "torch"
    tol(got, CH.run_ref(m, x, c, g1, g2, rel_pos_bias=bias), "rel_pos_bias")
    m(x, c, return_attn=True)
    assert m.last_path == "torch"
    g = torch.Generator().manual_seed(4)
    keep, ckeep = (torch.rand(1, 8, 60, 45, generator=g) > 0.25).to(DEV), (torch.rand(1, 8, 60, 45, generator=g) > 0.25).to(DEV)
    m = make(dropout=0.25)
    m.dropout, m.context_dropout = CH.FixedDropout(0.25, keep), CH.FixedDropout(0.25, ckeep)
    m.train()
    got = CH.run_module(m, x, c, g1, g2)
    assert m.last_path == "torch"
    tol(got, CH.run_ref(m, x, c, g1, g2, drop=(keep, ckeep, 0.25)), "dropout in training mode")
    m.eval()                                      # dropout > 0 in eval mode is the HIP form again
    CH.run_module(m, x, c, g1, g2)
    assert m.last_path == "hip"
    m = make().double()                           # not fp32
    m(x.double(), c.double())
    assert m.last_path == "torch"


class _Fp64Attention(torch.nn.Module):
    """The attention step in fp64 (the restatement) on the fp32 parameters of `module`, result cast back to fp32: the reference
    chain of the end-to-end test.  Gradients reach module's own parameters through the casts."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, x, context, mask=None, context_mask=None):
        p = {k: v.double() for k, v in self.module.named_parameters()}
        out, cout, _a, _c = CH.ref_forward(p, x.double(), context.double(), self.module.heads, mask, context_mask)
        return out.float(), cout.float()


def test_end_to_end_run_crossattn_render_loss_backward_step():
    """run_crossattn on 2000 + 2000 anchors of the stand-in model -> render -> RGB loss -> backward -> optimizer_c.step()."""
    from gscream_amd import crossattn as CA
    from gscream_amd import fit as F
    from gscream_amd import gaussian_renderer as GR
    from gscream_amd import loss_utils as L
    from gscream_amd import set_tuning
    from gscream_amd import simple_knn as KN
    from gscream_amd import standin_model as SM
    from gscream_amd import synthetic as S
    set_tuning()
    W, H, tanfovx, seed = 208, 117, 0.6, 3
    ts = F.teacher_scene(seed + 100, 80_000, W, H, tanfovx, DEV)
    cams = F.orbit_cameras(2, W, H, tanfovx, ts["means3D"].astype(np.float64).mean(0), device=DEV)
    gts, _depths = F.render_teacher(ts, cams, DEV)
    pts = SM.voxelize(S.surface_point_cloud(seed, 20_000, tanfovx, H / W), 0.001)
    anchors = torch.from_numpy(pts).float().to(DEV)
    base = SM.Model.from_pcd(anchors, torch.clamp_min(KN.distCUDA2(anchors), 0.0000001), K=10, seed=seed).to(DEV)
    N = int(anchors.shape[0])
    assert N >= 4000
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        base._anchor_feat.copy_((torch.randn(N, 32, generator=g) * 0.5).to(DEV))
    perm = torch.randperm(N, generator=g)
    fg, bg = torch.zeros(N, dtype=torch.bool), torch.zeros(N, dtype=torch.bool)
    fg[perm[:2000]] = True
    bg[perm[2000:4000]] = True
    fg, bg = fg.to(DEV), bg.to(DEV)
    attn = make(seed=5)
    bgcol = torch.zeros(3, device=DEV)
    args = types.SimpleNamespace(crossattn_lr_init=0.01)

    def chain(kind):
        model = copy.deepcopy(base)
        model.train()
        mod = copy.deepcopy(attn)
        mod.force_torch = kind == "torch"
        model.crossattn = _Fp64Attention(mod) if kind == "fp64" else mod
        CA.run_crossattn(model, fg, bg, ema=1.0, is_ref=True)
        if kind != "fp64":
            assert mod.last_path == ("torch" if kind == "torch" else "hip")
        vis, _x, _y = GR.prefilter_position2D(cams[1], model, F._Pipe, bgcol)
        pkg = GR.render(cams[1], model, F._Pipe, bgcol, visible_mask=vis, retain_grad=True)
        loss = L.rgb_loss(pkg["render"], gts[1], None, 0.2, 1.0)
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in mod.named_parameters()}
        return model, mod, grads, float(loss.detach())

    model, mod, hip, loss_hip = chain("hip")
    _m2, _mod2, eager, loss_eager = chain("torch")
    _m3, _mod3, ref, loss_ref = chain("fp64")
    print("losses (hip, eager, fp64 attention):", loss_hip, loss_eager, loss_ref)
    assert len(hip) == 8
    for k, v in hip.items():
        assert torch.isfinite(v).all() and float(v.abs().max()) > 0, k
    assert model._anchor_feat.grad is not None and float(model._anchor_feat.grad.abs().max()) > 0  # retain_grad() of run_crossattn
    check_4x(hip, eager, {k: v.double() for k, v in ref.items()}, "end to end")
    model.crossattn = mod
    opt = CA.crossattn_optimizer(model, args)
    before = {k: p.detach().clone() for k, p in mod.named_parameters()}
    opt.step()
    for k, p in mod.named_parameters():
        assert not torch.equal(p.detach(), before[k]), k
