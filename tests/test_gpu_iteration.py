"""One training iteration of the HIP chain, audited seam by seam against the chained oracles (tests/iteration_helpers.py; the
harness and its tolerances are proven on the CPU by tests/test_iteration.py), the sequences a trainer produces around it, and the
tensors that arrive on the wrong device.  Each docstring records the worst figure measured on an MI355X next to its bound."""
import copy
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers as H  # noqa: E402
import iteration_helpers as IH  # noqa: E402
from oracle import decode_oracle as DO  # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}
WARM_STEPS = 25


@pytest.fixture(scope="module", autouse=True)
def pointer_guard():
    """Nothing here runs unless _native.ptr() refuses host memory: an incomplete fix then raises instead of faulting the device."""
    from gscream_amd import _native
    with pytest.raises(RuntimeError):
        _native.ptr(torch.zeros(1))


@pytest.fixture(autouse=True)
def default_tuning():
    from gscream_amd.rasterizer import set_tuning
    set_tuning()
    yield
    set_tuning()


def scene(K):
    if K not in _cache:
        _cache[K] = IH.build_scene(K)
    return _cache[K]


def model_of(K, state):
    """The CPU copy of the model an audit starts from: the scene's fresh student, or that student after WARM_STEPS steps of fit.fit
    on the device (accumulators back at zero), where opacities and scales have left the untrained regime."""
    sc = scene(K)
    if state == "fresh":
        return sc.model
    if ("warm", K) not in _cache:
        from gscream_amd import fit as F
        from gscream_amd.adam import Adam
        be = IH.backend("hip")
        model = be.model(sc.model)
        gts = torch.stack([t.image for t in sc.targets]).cuda()
        gdepths = torch.stack([t.depth for t in sc.targets]).cuda()
        F.fit(model, [be.camera(c) for c in sc.cams], gts, gdepths, WARM_STEPS, seed=1, optimizer=lambda groups: Adam(groups, lr=0.0, eps=1e-15))
        model = copy.deepcopy(model).cpu()
        for n in IH.ACC_NAMES:
            getattr(model, n).zero_()
        assert float((model._anchor_feat.detach() != 0).float().mean()) > 0.3 and float(model._offset.detach().abs().max()) > 0
        _cache["warm", K] = model
    return _cache["warm", K]


def hip_record(view, K, state="fresh", **kw):
    key = ("rec", view, K, state)
    if kw:
        return IH.run(IH.backend("hip"), scene(K), model_of(K, state), view, **kw)
    if key not in _cache:
        _cache[key] = IH.run(IH.backend("hip"), scene(K), model_of(K, state), view)
    return _cache[key]


def _equal(a, b, path=""):
    """Bit-for-bit equality of two recorded values (tensors, arrays, floats, lists, dicts)."""
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _equal(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, f"{path}/{i}")
    elif isinstance(a, torch.Tensor):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), path
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    else:
        assert a == b or (a is None and b is None), (path, a, b)


def records_equal(a, b):
    _equal(a.iters, b.iters, "iters")
    _equal(a.acc, b.acc, "acc")


# ---- the audit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [10, 4])
@pytest.mark.parametrize("view", ["ref", "other"])
@pytest.mark.parametrize("state", ["fresh", "warm"])
def test_iteration_seam_by_seam(state, view, K):
    """Two iterations (camera 0, camera 1) of the HIP chain with set_tuning() defaults, on the fresh student and after 25 steps of
    fit.fit: every seam check of iteration_helpers.SEAMS at the tolerance of the module downstream of the seam, then the
    end-to-end rule per parameter tensor, e_hip <= max(4 e_ref, 1e-3 max|ref|), against the fully chained oracle with the
    float32 oracle chain's own error e_ref as the yardstick.  The fresh scenes hold no depth pixel on the L1 kink (asserted), so
    there the depth-gradient bound and the rule are the plain ones; a warmed-up model may hold one, which is then enumerated on
    the oracle's side (iteration_helpers._depth_gradient_choices, end_to_end).  The figures are printed before anything is asserted.
    Worst measured over the eight cases, next to the bound: decode forward 2.1e-7 (2e-5); rendered maps 2.9e-6 (1e-4), radii and
    every walk's last Gaussian equal; loss terms rgb 1.3e-8, rgb_fg 1.1e-7 (2e-6), depth 9.8e-7 (5e-6); gradient at render 1.9e-5 of
    its largest entry (1e-4); depth-gradient pixels beyond 1e-4 of the largest entry: at most 2 of a picture's 17 472, and they are
    the two endpoints of ONE edge term of the four-scale gradient loss that the float64 oracle puts within 4e-6 of zero (of up to 15
    such terms in a picture; loss_helpers.assert_depth_grad: deviation at most that term's sign, 1.8e-3 .. 9.7e-3 of the largest
    entry measured), every other pixel within 4.2e-7 of the largest entry; no L1-kink pixel in the fresh cases, 1 in three of the
    warm ones; rasterizer backward 1.3e-4 rel (1e-3), nothing to classify; decode
    backward 1.1e-6 (2e-4), .grad bit-equal to the replay; hidden rows exactly zero; accumulators 9.5e-7 abs on
    offset_gradient_accum, the others exact; Adam at most 0.57 / 0.67 / 0.49 of the m / v / p bounds.
    End to end, the worst tensor of each case as e_hip / max|ref| (e_ref / max|ref| beside it, both relative to that tensor's largest
    reference entry): fresh ref K=10 1.5e-6 (5.5e-5), fresh other K=10 6.9e-7 (4.2e-4), fresh ref K=4 9.4e-6 (9.5e-7), fresh other
    K=4 5.6e-7 (1.2e-6), warm ref K=10 2.6e-6 (3.7e-5), warm other K=10 2.1e-5 (3.1e-4), warm ref K=4 3.7e-6 (2.0e-6), warm other
    K=4 5.5e-6 (2.7e-6): every tensor at most 2.1 % of the rule's bound, all inside the 1e-3 floor."""
    sc, model = scene(K), model_of(K, state)
    rec = hip_record(view, K, state)
    worst = IH.check_all(rec, sc)
    table, kinks = IH.end_to_end(rec, sc, model, view)
    assert state == "warm" or (worst["loss L1 kink pixels"] == 0 and kinks == 0)


@pytest.mark.parametrize("knob", ["speculative", "view_cache"])
def test_tuning_knobs_do_not_change_the_record(knob):
    """ref / K = 10 with speculative=False (the two-stage forward) and with view_cache=False: every recorded tensor -- images, radii,
    all gradients, accumulators, parameters and Adam state after the step -- equals the default record's bit for bit."""
    from gscream_amd.rasterizer import set_tuning
    base = hip_record("ref", 10)
    set_tuning(**{knob: False})
    records_equal(hip_record("ref", 10, iterations=2), base)


# ---- sequences the trainer produces -----------------------------------------------------------------------------------------------
def test_second_backward_accumulates():
    """A second loss.backward(retain_graph=True) through the retained graph doubles every parameter gradient: grad2 - grad1 equals
    grad1 bit for bit (the decode's and the rasterizer's backward are reproducible and read nothing the first one consumed)."""
    seen = []

    def again(c):
        g1 = [p.grad.clone() for p in c.params]
        v1 = c.pkg["viewspace_points"].grad.clone()
        c.loss.backward(retain_graph=True)
        for n, p, a in zip(c.names, c.params, g1):
            assert torch.equal(p.grad - a, a), n
            p.grad = a   # what the plain iteration steps on
        assert torch.equal(c.pkg["viewspace_points"].grad - v1, v1)
        c.pkg["viewspace_points"].grad = v1
        seen.append(c.it)
    rec = hip_record("ref", 10, hooks={"after_backward": again})
    assert seen == [0, 1]
    records_equal(rec, hip_record("ref", 10))


def test_eval_render_between_backward_and_statistics():
    """training_report (train.py:591) renders other cameras in eval mode under no_grad between the backward and training_statis.
    The decode's bookkeeping on the training render's selection mask still matches its visibility mask afterwards, and the whole
    record -- the accumulators included -- equals the plain iteration's bit for bit."""
    from gscream_amd import gaussian_renderer as GR
    seen = []

    def report(c):
        other = c.be.camera(c.scene.cams[1 - c.scene.cams.index(c.cam)])
        bg = torch.tensor(IH.BG, device="cuda")
        c.model.eval()
        with torch.no_grad():
            vis2, _x, _y = GR.prefilter_position2D(other, c.model, IH._Pipe, bg)
            out = GR.render(other, c.model, IH._Pipe, bg, visible_mask=vis2)
        c.model.train()
        assert "selection_mask" not in out and not torch.equal(vis2, c.vis)
        book = c.pkg["selection_mask"]._gsr_decode
        assert book.matches(c.vis, c.scene.K) and book.M == c.pkg["radii"].shape[0] and book.N == int(c.vis.sum())
        seen.append(c.it)
    rec = hip_record("ref", 10, hooks={"after_backward": report})
    assert seen == [0, 1]
    records_equal(rec, hip_record("ref", 10))


def test_two_training_forwards_alive_at_once():
    """Cameras A (168 x 104) and B (96 x 64) are rendered in training mode one after the other, then loss_B.backward() runs before
    loss_A.backward(): each view's parameter gradients and viewspace gradient equal those of that view rendered alone, bit for bit.
    (rasterizer.py's backward takes num_rendered, the binning capacity, max_tile_count and its three workspaces from its own ctx,
    the decode's its row list and dims likewise; neither reads _capacity_hint, _pinned_tls or the view cache.)"""
    from gscream_amd import fit as F
    from gscream_amd import gaussian_renderer as GR
    from gscream_amd import loss_utils as L
    sc = scene(10)
    be = IH.backend("hip")
    model = be.model(sc.model)
    bg = torch.tensor(IH.BG, device="cuda")
    centre = sc.model._anchor.detach().double().mean(0).numpy()
    cam_a = be.camera(sc.cams[0])
    cam_b = F.orbit_cameras(2, 96, 64, IH.TANFOVX, centre, angle=0.2, device="cuda")[1]
    g = torch.Generator().manual_seed(5)
    targets = {}
    for name, (h, w) in (("a", (IH.H_IMG, IH.W)), ("b", (64, 96))):
        targets[name] = (torch.rand(3, h, w, generator=g).cuda(), (torch.rand(1, h, w, generator=g) * 4 + 2).cuda())

    def forward(cam, name):
        vis, _x, _y = GR.prefilter_position2D(cam, model, IH._Pipe, bg)
        pkg = GR.render(cam, model, IH._Pipe, bg, visible_mask=vis, retain_grad=True)
        img, dep = targets[name]
        return pkg, L.rgb_loss(pkg["render"], img, None, 0.2, 1.0) + L.depth_loss(pkg["render_depth"], dep, None, None, None, 1.0, 1.0)

    def grads(pkg):
        out = [p.grad.clone() for p in model.parameters()] + [pkg["viewspace_points"].grad.clone()]
        for p in model.parameters():
            p.grad = None
        return out
    alone = {}
    for name, cam in (("a", cam_a), ("b", cam_b)):
        pkg, loss = forward(cam, name)
        loss.backward()
        alone[name] = grads(pkg)
    pkg_a, loss_a = forward(cam_a, "a")
    pkg_b, loss_b = forward(cam_b, "b")
    assert pkg_a["render"].shape[1:] == (IH.H_IMG, IH.W) and pkg_b["render"].shape[1:] == (64, 96)
    loss_b.backward()
    got_b = grads(pkg_b)
    loss_a.backward()
    got_a = grads(pkg_a)
    for name, got in (("a", got_a), ("b", got_b)):
        assert len(got) == len(alone[name])
        for i, (x, y) in enumerate(zip(got, alone[name])):
            assert x.shape == y.shape and torch.equal(x, y), (name, i)
        assert float(got[-1].abs().sum()) > 0 and float(got[1].abs().sum()) > 0


# ---- the device of a pointer ------------------------------------------------------------------------------------------------------
WIDTHS = (3, 3, 1, 1, 3, 4)


def _decode_with(model, cam, vis_arg, fields):
    from gscream_amd.neural_gaussians import generate_neural_gaussians
    for p in model.parameters():
        p.grad = None
    out = generate_neural_gaussians(cam, model, vis_arg, True)
    keys = torch.nonzero(out[7]).view(-1)
    sum((o * f[keys]).sum() for o, f in zip(out[:6], fields)).backward()
    return out, {n: p.grad.clone() for n, p in model.named_parameters()}


def test_visibility_mask_on_any_device_and_as_index_list():
    """generate_neural_gaussians at the ref / K = 10 scene with the visibility as a device mask, a CPU mask, a CPU index list and a
    device index list (what x[visible_mask] accepts): all eight outputs and every parameter gradient are bit-equal.  The index
    lists reach decode() without a mask, so the backward takes its zero-fill branch: its outputs against the float64 oracle at 2e-5,
    its gradients at 2e-4 (upstream zero on ambiguous keys and kinked anchors, as tests/test_gpu_training_sizes.py), the gradient
    rows outside the list exactly zero.
    Worst measured: outputs rot 1.8e-7, the others <= 7.9e-8; gradients <= 5.9e-7 (mlp_uncertainty.0.bias); no ambiguous key,
    2 kinked anchors."""
    sc = scene(10)
    be = IH.backend("hip")
    model, cam = be.model(sc.model), be.camera(sc.cams[0])
    vis, _x, _y = be.prefilter(sc.cams[0], model, sc)
    Nv, K = int(vis.sum()), sc.K
    # the oracle first: which keys are ambiguous, which anchors sit on a ReLU kink
    ref = copy.deepcopy(sc.model).double().train()
    seen, unhook = H.record_first_layers(ref)
    out_r = DO.generate_neural_gaussians(DO.Camera(sc.cams[0].camera_center.double()), ref, vis.cpu(), True)
    unhook()
    kinked = (torch.cat(seen, 1).abs() <= 1e-5).any(1)
    g = torch.Generator().manual_seed(9)
    variants = {"device mask": vis, "cpu mask": vis.cpu(), "cpu index list": torch.nonzero(vis.cpu()).view(-1),
                "device index list": torch.nonzero(vis).view(-1)}
    results = {}
    fields = None
    for name, arg in variants.items():
        if fields is None:
            from gscream_amd.neural_gaussians import generate_neural_gaussians
            with torch.no_grad():
                mask0 = generate_neural_gaussians(cam, model, arg, True)[7]
            al = H.align_decode_rows(mask0, out_r[7], out_r[6])
            fields64 = H.upstream_fields(Nv * K, WIDTHS, al.ambiguous | kinked.repeat_interleave(K), g)
            fields = [f.float().cuda() for f in fields64]
        results[name] = _decode_with(model, cam, arg, fields)
    base_out, base_grads = results["device mask"]
    for name, (out, grads) in results.items():
        for i, (a, b) in enumerate(zip(out, base_out)):
            assert a.shape == b.shape and torch.equal(a, b), (name, "output", i)
        for n in base_grads:
            assert torch.equal(grads[n], base_grads[n]), (name, "grad", n)
    # the zero-fill branch against the oracle
    out_d, grads_d = results["device index list"]
    worst = {"ambiguous keys": int(al.ambiguous.sum()), "kinked anchors": int(kinked.sum())}
    for nm, a, b in zip(IH.DEC_NAMES, out_d[:6], out_r[:6]):
        worst[nm] = e = H.max_scaled_err(a.detach().cpu()[al.rows_got], b.detach()[al.rows_ref])
        assert e <= 2e-5, (nm, e)
    sum((o * f[al.keys_ref]).sum() for o, f in zip(out_r[:6], fields64)).backward()
    hidden = ~vis.cpu()
    for n, p in ref.named_parameters():
        worst["grad " + n] = e = H.max_scaled_err(grads_d[n], p.grad)
        assert e <= 2e-4, ("grad " + n, e)
    for n in IH.HIDDEN_ROW_PARAMS:
        assert bool(hidden.any()) and bool((grads_d[n].cpu()[hidden] == 0).all()), n
    print("\n[worst] decode through an index list: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_index_list_must_be_ascending_rows():
    from gscream_amd.neural_gaussians import generate_neural_gaussians
    sc = scene(4)
    be = IH.backend("hip")
    model, cam = be.model(sc.model), be.camera(sc.cams[0])
    with pytest.raises(NotImplementedError):
        generate_neural_gaussians(cam, model, torch.tensor([5, 3, 9]), True)
    with pytest.raises(IndexError):
        generate_neural_gaussians(cam, model, torch.tensor([0, sc.N]), True)


def test_rasterizer_moves_host_opacities_to_the_device():
    """The rasterizer's forward hands its own pointers to the library (not through _native.ptr()): opacities and uncertainties in host
    memory are moved like scales, rotations and colours are, and the maps and radii equal the all-device call's bit for bit."""
    from gscream_amd import GaussianRasterizer
    from gscream_amd import synthetic as S
    s = S.scene_config1(seed=7, P=700, W=88, H=56)
    t = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rast = GaussianRasterizer(raster_settings=H.hip_settings(s))
    outs = []
    for dev in ("cuda", "cpu"):
        m = t(s["means3D"], "cuda")
        with torch.no_grad():
            outs.append(rast(means3D=m, means2D=torch.zeros_like(m), opacities=t(s["opacities"], dev), uncertainties=t(s["uncertainties"], dev),
                             colors_precomp=t(s["colors"], dev), scales=t(s["scales"], dev), rotations=t(s["rotations"], dev)))
    for a, b in zip(*outs):
        assert a.is_cuda and torch.equal(a, b)
    assert float(outs[0][0].std()) > 0


def test_training_statistics_with_host_masks():
    """training_statis with the visibility mask, update_filter, the selection mask, the neural opacity and viewspace_points.grad in host
    memory gives the accumulators of the all-device call bit for bit (and the restated reference's at rtol 1e-6, atol 1e-7)."""
    from gscream_amd.densify_stats import training_statis
    sc = scene(10)
    rec = hip_record("ref", 10)
    r = rec.iters[0]
    N, K = sc.N, sc.K
    mk = lambda dev: types.SimpleNamespace(n_offsets=K, opacity_accum=torch.zeros(N, 1, device=dev), anchor_demon=torch.zeros(N, 1, device=dev),
                                           offset_gradient_accum=torch.zeros(N * K, 1, device=dev), offset_denom=torch.zeros(N * K, 1, device=dev))
    args = (r["nop"], r["radii"] > 0, r["sel_mask"], r["vis"])
    acc_host, acc_dev, acc_ref = mk("cuda"), mk("cuda"), mk("cpu")
    training_statis(acc_host, types.SimpleNamespace(grad=r["vsp_grad"]), *args)
    training_statis(acc_dev, types.SimpleNamespace(grad=r["vsp_grad"].cuda()), *[a.cuda() for a in args])
    DO.training_statis(acc_ref, types.SimpleNamespace(grad=r["vsp_grad"]), *args)
    for n in IH.ACC_NAMES:
        assert torch.equal(getattr(acc_host, n), getattr(acc_dev, n)), n
        assert torch.allclose(getattr(acc_host, n).cpu(), getattr(acc_ref, n), rtol=1e-6, atol=1e-7), n
    assert float(acc_host.offset_denom.sum()) > 0
