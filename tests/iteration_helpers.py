"""One training iteration, seam by seam (tests/test_iteration.py on the CPU, tests/test_gpu_iteration.py on the device).

`run(backend, scene, model, view)` runs the body of fit.fit's loop twice (camera 0, then camera 1) -- prefilter, decode, rasterize,
RGB and depth losses of train.py:535-573, `loss.backward(retain_graph=True)`, training_statis, one Adam step -- and records every
tensor that crosses from one module into the next.  Backends:

    "hip"    the package's own modules on the device (gscream_amd.gaussian_renderer, loss_utils, densify_stats, adam.Adam)
    "cpu32"  the oracles chained in float32 on the CPU: oracle.decode_oracle, the C rasterizer oracle, oracle.loss_oracle, the
             restated training_statis and a float32 numpy Adam in the kernel's expression sequence.  It stands in for the device,
             so that the harness and its tolerances can be shown to hold without one
    "cpu64"  the same chain with the decode and the losses in float64 (the C rasterizer reads float32 casts of the decode's outputs):
             the fully chained oracle of the end-to-end figure

`SEAMS` maps a seam's name to its check.  Every check compares what the module DOWNSTREAM of a seam produced with that module's
own oracle fed with the RECORDED tensors upstream of it, so a discrete decision that falls the other way in one module (a mask
bit, a radius, an alpha test) never leaks into the next module's comparison.  Tolerances are the ones the module's own tests use.
A check raises AssertionError; the planted-fault tests of tests/test_iteration.py show that each of them can."""
import copy
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers as H  # noqa: E402
import loss_helpers as LH  # noqa: E402
from gscream_amd import standin_model as SM  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402
from gscream_amd.adam import adam_scalars  # noqa: E402
from oracle import decode_oracle as DO  # noqa: E402
from oracle import knn_oracle as KO  # noqa: E402
from oracle import loss_oracle as LO  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_adam import adam_oracle  # noqa: E402  (tests/ is on sys.path, as for `helpers`)

W, H_IMG, TANFOVX = 168, 104, 0.45   # 10.5 x 6.5 tiles: ragged on both edges
CLOUD_TANFOVX = 0.6                  # the cloud fills a wider frustum than the cameras see: about an eighth of the anchors are hidden
BG = (0.0, 0.0, 0.0)
DEC_NAMES = ("xyz", "color", "opacity", "uncertainty", "scaling", "rot")
ACC_NAMES = ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")
HIDDEN_ROW_PARAMS = ("_anchor_feat", "_offset", "_scaling", "_anchor")
# the shipped run configuration (scripts/run.py): lambda_dssim, refer_rgb_lr / _fg, other_rgb_lr / _fg, refer_depth_lr / _fg /
# _smooth, other_depth_lr / _smooth
CFG = dict(lambda_dssim=0.2, refer_rgb_lr=1.0, refer_rgb_lr_fg=20.0, other_rgb_lr=1.0, other_rgb_lr_fg=0.0, refer_depth_lr=1.0,
           refer_depth_lr_fg=100.0, refer_depth_lr_smooth=1.0, other_depth_lr=0.1, other_depth_lr_smooth=0.1)
#: points sampled, cloud seed, orbit angle and the seed of the MLPs per K.  The MLP seeds were found by a search for the scene
#: conditions of check_scene_conditions (tests/test_iteration.py asserts them from the "cpu32" backend): with zero anchor features
#: the opacity MLP sees only the view direction and distance, so few initialisations mask every offset of some anchor; the seeds of
#: the targets' jitter keep every depth pixel off the L1 kink
SCENES = {10: dict(n_points=2100, seed=3, angle=0.12, model_seed=870, target_seed=2004), 4: dict(n_points=1900, seed=5, angle=0.12, model_seed=51, target_seed=2002)}
U32, TAU = 2.0 ** -24, 2.0 ** -149
NTHREADS = 8


def _np(t):
    return np.ascontiguousarray(t.detach().cpu().float().numpy())


# ---- scene -----------------------------------------------------------------------------------------------------------------------
def build_scene(K, n_points=None, seed=None, angle=None, model_seed=None, target_seed=None):
    """Everything both sides read, built on the CPU: the student model (float32, Model.from_pcd of a voxelised surface cloud with the
    exact 3-NN distances), two orbit cameras, and per camera a target image, a target depth, gt_mask and the foreground mask."""
    from gscream_amd import fit as F
    p = dict(SCENES[K])
    p.update({k: v for k, v in dict(n_points=n_points, seed=seed, angle=angle, model_seed=model_seed, target_seed=target_seed).items() if v is not None})
    pts = SM.voxelize(S.surface_point_cloud(p["seed"], p["n_points"], CLOUD_TANFOVX, H_IMG / W), 0.001)
    anchors = torch.from_numpy(pts).float()
    dist2 = torch.clamp_min(torch.from_numpy(KO.mean_dist2(anchors.numpy())).float(), 1e-7)
    model = SM.Model.from_pcd(anchors, dist2, K=K, seed=p["model_seed"])
    model.train()
    centre = pts.astype(np.float64).mean(0)
    cams = F.orbit_cameras(2, W, H_IMG, TANFOVX, centre, angle=p["angle"], device="cpu")
    scene = types.SimpleNamespace(K=K, model=model, cams=cams, N=int(anchors.shape[0]), tanfovy=TANFOVX * H_IMG / W, params=p, targets=[])
    rng = np.random.default_rng(p["target_seed"])
    for c, cam in enumerate(cams):
        # targets: the C oracle's render of a jittered copy of the student's own Gaussians (inputs only, but with structure)
        with torch.no_grad():
            xyz, color, opacity, unc, scaling, rot = DO.generate_neural_gaussians(cam, model, None, False)
        s = raster_scene([xyz, color, opacity, unc, scaling, rot], cam, scene)
        s["means3D"] = (s["means3D"] + rng.normal(0, 0.02, s["means3D"].shape)).astype(np.float32)
        s["colors"] = np.clip(s["colors"] + rng.normal(0, 0.15, s["colors"].shape), 0, 1).astype(np.float32)
        s["opacities"] = np.clip(s["opacities"] * 1.5, 0, 1).astype(np.float32)
        st = H.oracle_forward(s, nthreads=NTHREADS)
        gt_mask = torch.zeros(1, H_IMG, W)
        gt_mask[:, 30:75, 50 + 10 * c:120 + 10 * c] = 1.0
        fg = torch.zeros(1, H_IMG, W)
        fg[:, 22:84, 38 + 10 * c:134 + 10 * c] = 1.0   # get_random_mask: an enlarged box around gt_mask
        scene.targets.append(types.SimpleNamespace(image=torch.from_numpy(st["out_color"].copy()).clamp(0, 1), depth=torch.from_numpy(st["out_depth"].copy()),
                                                   gt_mask=gt_mask, fg_mask=fg))
    return scene


def raster_scene(dec, cam, scene):
    """The rasterizer-level scene dict of six decode outputs (any dtype / device; cast to float32) seen from `cam`."""
    xyz, color, opacity, unc, scaling, rot = (_np(t) for t in dec)
    return dict(means3D=xyz, colors=color, opacities=opacity.reshape(-1, 1), uncertainties=unc.reshape(-1, 1), scales=scaling, rotations=rot,
                W=W, H=H_IMG, tanfovx=TANFOVX, tanfovy=scene.tanfovy, viewmatrix=_np(cam.world_view_transform),
                projmatrix=_np(cam.full_proj_transform), campos=_np(cam.camera_center), bg=np.asarray(BG, np.float32), scale_modifier=1.0)


def cam_kwargs(cam, scene):
    return dict(W=W, H=H_IMG, tanfovx=TANFOVX, tanfovy=scene.tanfovy, viewmatrix=_np(cam.world_view_transform), projmatrix=_np(cam.full_proj_transform))


# ---- the two loss configurations of train.py:535-573 --------------------------------------------------------------------------------
class _OracleLosses:
    """oracle.loss_oracle behind gscream_amd.loss_utils' two entry points (in the dtype of its inputs)."""

    @staticmethod
    def rgb_loss(image, gt, weight=None, lambda_dssim=0.2, scale=1.0):
        return LO.rgb_loss(image, gt.to(image.dtype), None if weight is None else weight.to(image.dtype), lambda_dssim, scale)

    @staticmethod
    def depth_loss(depth, target, lsq_mask=None, l1_weight=None, grad_mask=None, lambda_l1=1.0, lambda_smooth=1.0, fg_mask=None, lambda_fg=0.0):
        c = lambda t: None if t is None else t.to(depth.dtype)
        if depth.dtype == torch.float64:
            return LO.depth_loss(depth, c(target), c(lsq_mask), c(l1_weight), c(grad_mask), lambda_l1, lambda_smooth, c(fg_mask), lambda_fg)[0]
        # float32: the five products of the scale-and-shift fit formed, summed and solved in float64 from the float32 inputs, as
        # depth_loss.hip does (widened BEFORE multiplying, so a fit the reference calls singular has det = 0 here too; the normal
        # equations cancel: solved in float32 they miss the depth loss' own 5e-6 bound), everything per pixel in float32
        d64 = lambda t: None if t is None else t.double()
        m = torch.ones_like(depth) if lsq_mask is None else c(lsq_mask)
        scale, shift = LO.compute_scale_and_shift(depth.double(), d64(target), m.double())
        aligned = torch.abs(scale).to(depth.dtype).view(-1, 1, 1) * depth + shift.to(depth.dtype).view(-1, 1, 1)
        target = c(target)
        loss = lambda_l1 * (LO.l1_loss(aligned, target) if l1_weight is None else LO.l1_loss_masked(aligned, target, c(l1_weight)))
        if fg_mask is not None:
            loss = loss + lambda_fg * LO.l1_loss_masked(aligned, target, c(fg_mask))
        g = torch.ones_like(depth) if grad_mask is None else c(grad_mask)
        for k in range(4):
            step = pow(2, k)
            loss = loss + 0.5 * lambda_smooth * LO.gradient_loss(aligned[:, ::step, ::step], target[:, ::step, ::step], g[:, ::step, ::step])
        return loss


def depth_config(view, tg):
    """The depth loss' arguments in the two configurations, as loss_helpers.depth_terms takes them."""
    valid = 1.0 - tg.gt_mask
    if view == "ref":
        return dict(lsq=valid, w=None, g=None, lambda_l1=CFG["refer_depth_lr"], lambda_smooth=CFG["refer_depth_lr_smooth"], fg=tg.fg_mask,
                    lambda_fg=CFG["refer_depth_lr_fg"] - CFG["refer_depth_lr"])
    assert view == "other", view
    return dict(lsq=valid, w=valid, g=valid, lambda_l1=CFG["other_depth_lr"], lambda_smooth=CFG["other_depth_lr_smooth"], fg=None, lambda_fg=0.0)


def loss_parts(L, view, image, depth, tg):
    """-> [(name, tensor, scale)]: the terms of train.py:535-573 for the reference view ("ref") or any other ("other"), through
    `L.rgb_loss` / `L.depth_loss` (gscream_amd.loss_utils or the oracle).  Their sum is the loss."""
    lam = CFG["lambda_dssim"]
    if view == "ref":
        lr, lr_fg = CFG["refer_rgb_lr"], CFG["refer_rgb_lr_fg"]
        return [("rgb", L.rgb_loss(image, tg.image, None, lam, lr), lr),
                ("rgb_fg", L.rgb_loss(image, tg.image, tg.gt_mask, lam, lr_fg - lr), lr_fg - lr),  # :539-540
                ("depth", L.depth_loss(depth, tg.depth, lsq_mask=1.0 - tg.gt_mask, l1_weight=None, grad_mask=None, lambda_l1=CFG["refer_depth_lr"],
                                       lambda_smooth=CFG["refer_depth_lr_smooth"], fg_mask=tg.fg_mask,
                                       lambda_fg=CFG["refer_depth_lr_fg"] - CFG["refer_depth_lr"]), 1.0)]
    assert view == "other", view
    weight = (1.0 - tg.gt_mask) + CFG["other_rgb_lr_fg"] * tg.gt_mask   # :542
    valid = 1.0 - tg.gt_mask
    return [("rgb", L.rgb_loss(image, tg.image, weight, lam, CFG["other_rgb_lr"]), CFG["other_rgb_lr"]),
            ("depth", L.depth_loss(depth, tg.depth, lsq_mask=valid, l1_weight=valid, grad_mask=valid, lambda_l1=CFG["other_depth_lr"],
                                   lambda_smooth=CFG["other_depth_lr_smooth"]), 1.0)]


# ---- the CPU chain's rasterizer and optimiser -------------------------------------------------------------------------------------
class _OracleRaster(torch.autograd.Function):
    """The C rasterizer oracle as an autograd node with GaussianRasterizer's inputs and outputs (float32 inside)."""

    @staticmethod
    def forward(ctx, xyz, means2D, color, opacity, unc, scaling, rot, cam, scene, keep):
        s = raster_scene([xyz, color, opacity, unc, scaling, rot], cam, scene)
        st = H.oracle_forward(s, nthreads=NTHREADS)
        ctx.s, ctx.st, ctx.dtype = s, st, xyz.dtype
        ctx.set_materialize_grads(False)
        keep.update(st=st, s=s)
        t = lambda a: torch.from_numpy(a.copy()).to(xyz.dtype)
        radii = torch.from_numpy(st["radii"].copy())
        ctx.mark_non_differentiable(radii)
        return t(st["out_color"]), t(st["out_depth"]), t(st["out_unc"]), radii

    @staticmethod
    def backward(ctx, gc, gd, gu, _gr):
        z = lambda g, c: np.zeros((c, H_IMG, W), np.float32) if g is None else _np(g)
        g = H.oracle_backward(ctx.s, ctx.st, (z(gc, 3), z(gd, 1), z(gu, 1)), nthreads=NTHREADS)
        t = lambda k: torch.from_numpy(g[k]).to(ctx.dtype)
        return (t("dL_dmeans3D"), t("dL_dmeans2D"), t("dL_dcolors"), t("dL_dopacity"), t("dL_duncertainty"), t("dL_dscales"),
                t("dL_drotations"), None, None, None)


def adam_step_f32(p, g, m, v, lr, betas, eps, t):
    """One Adam step in float32 numpy with one rounding per operation, in the expression sequence of gscream_amd/adam.py."""
    f = np.float32
    b1, c1, b2, c2, s2, e, a = (f(x) for x in adam_scalars(lr, betas, eps, t))
    p, g, m, v = (np.asarray(x, f) for x in (p, g, m, v))
    m1 = m * b1 + g * c1
    v1 = v * b2 + (c2 * g) * g
    d = np.sqrt(v1) / s2 + e
    return p + (a * m1) / d, m1, v1


class _NumpyAdam:
    """torch.optim.Adam's interface as far as the harness reads it (param_groups, state, step), stepping with adam_step_f32."""

    def __init__(self, groups, lr=0.0, eps=1e-15, betas=(0.9, 0.999)):
        self.param_groups = [{"lr": lr, "eps": eps, "betas": betas, **g, "params": list(g["params"])} for g in groups]
        self.state = {}

    @torch.no_grad()
    def step(self):
        for grp in self.param_groups:
            for p in grp["params"]:
                if p.grad is None:
                    continue
                st = self.state.setdefault(p, {})
                if not st:
                    st.update(step=torch.tensor(0.0), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
                st["step"] += 1
                p1, m1, v1 = adam_step_f32(p.numpy(), p.grad.numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), grp["lr"], grp["betas"],
                                           grp["eps"], float(st["step"]))
                for dst, src in ((p, p1), (st["exp_avg"], m1), (st["exp_avg_sq"], v1)):
                    dst.copy_(torch.from_numpy(src).to(dst.dtype))


# ---- backends ---------------------------------------------------------------------------------------------------------------------
class _Pipe:
    debug, compute_cov3D_python = False, False


class _Cpu:
    """The chained oracles in `dtype` (float32: "cpu32", the device's stand-in; float64: "cpu64", the fully chained oracle)."""

    def __init__(self, dtype):
        self.dtype, self.device, self.L = dtype, "cpu", _OracleLosses
        self.name = "cpu32" if dtype == torch.float32 else "cpu64"

    def model(self, model_cpu):
        m = copy.deepcopy(model_cpu).to(self.dtype)
        for n in ACC_NAMES:   # the accumulators stay float32 whatever the model's dtype
            setattr(m, n, getattr(m, n).float())
        return m.train()

    def optimizer(self, groups):
        return _NumpyAdam(groups, lr=0.0, eps=1e-15)

    def camera(self, cam):
        c = copy.copy(cam)
        c.camera_center = cam.camera_center.to(self.dtype)
        return c

    def prefilter(self, cam, model, scene):
        r, x, y = O.position2D_filter(_np(model.get_anchor), _np(model.get_scaling[:, :3]), _np(model.get_rotation), **cam_kwargs(cam, scene))
        return torch.from_numpy(r > 0), torch.from_numpy(x), torch.from_numpy(y)

    def render(self, cam, model, vis, scene, on_decode):
        out = DO.generate_neural_gaussians(self.camera(cam), model, vis, True)
        on_decode(out)
        xyz, color, opacity, unc, scaling, rot, nop, mask = out
        vsp = torch.zeros_like(xyz, requires_grad=True)
        keep = {}
        image, depth, umap, radii = _OracleRaster.apply(xyz, vsp, color, opacity, unc, scaling, rot, cam, scene, keep)
        st = keep["st"]
        ends = (st["final_T"].copy(), H.last_gaussian(st["ranges"], st["point_list"], st["n_contrib"], W, H_IMG))
        return dict(render=image, render_depth=depth, uncertainty=umap, viewspace_points=vsp, visibility_filter=radii > 0, radii=radii,
                    selection_mask=mask, neural_opacity=nop), ends

    def training_statis(self, model, pkg, vis):
        DO.training_statis(model, pkg["viewspace_points"], pkg["neural_opacity"].float(), pkg["visibility_filter"], pkg["selection_mask"], vis)


class _Hip:
    name, dtype, device = "hip", torch.float32, "cuda"

    def __init__(self, between=None):
        from gscream_amd import loss_utils
        self.L, self.between = loss_utils, between

    def model(self, model_cpu):
        return copy.deepcopy(model_cpu).float().to(self.device).train()

    def optimizer(self, groups):
        from gscream_amd.adam import Adam
        return Adam(groups, lr=0.0, eps=1e-15)

    def camera(self, cam):
        if getattr(cam, "_dev", None) is None:   # one device copy per camera: the view cache keys on the view matrix' address
            t = lambda a: a.to(self.device)
            cam._dev = SM.Camera(t(cam.camera_center), image_height=cam.image_height, image_width=cam.image_width, FoVx=cam.FoVx, FoVy=cam.FoVy,
                                 world_view_transform=t(cam.world_view_transform), full_proj_transform=t(cam.full_proj_transform))
        return cam._dev

    def prefilter(self, cam, model, scene):
        from gscream_amd import gaussian_renderer as GR
        return GR.prefilter_position2D(self.camera(cam), model, _Pipe, torch.tensor(BG, device=self.device))

    def render(self, cam, model, vis, scene, on_decode):
        import pytest
        from gscream_amd import gaussian_renderer as GR
        real = GR.generate_neural_gaussians

        def recording(*a, **k):
            out = real(*a, **k)
            on_decode(out)
            return out
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(GR, "generate_neural_gaussians", recording)
            pkg = GR.render(self.camera(cam), model, _Pipe, torch.tensor(BG, device=self.device), visible_mask=vis, retain_grad=True)
        return pkg, H.walk_ends(pkg["render"], int(pkg["radii"].shape[0]), W, H_IMG)

    def training_statis(self, model, pkg, vis):
        from gscream_amd import densify_stats as DS
        DS.training_statis(model, pkg["viewspace_points"], pkg["neural_opacity"], pkg["visibility_filter"], pkg["selection_mask"], vis)


def backend(name, **kw):
    return _Hip(**kw) if name == "hip" else _Cpu(torch.float32 if name == "cpu32" else torch.float64)


# ---- one run: two iterations, everything recorded ---------------------------------------------------------------------------------
def _c(t):
    return None if t is None else t.detach().cpu().clone()


def _targets(tg, be):
    return types.SimpleNamespace(**{k: v.to(device=be.device, dtype=be.dtype) for k, v in vars(tg).items()})


def _oracle_decode(model_cpu_state, scene, cam, vis_cpu):
    """The float64 decode oracle on the model as it stands, with the recorded visibility mask: outputs (attached), the model, the
    ReLU inputs of the four first layers."""
    ref = copy.deepcopy(scene.model).double()
    ref.load_state_dict(model_cpu_state)
    ref.train()
    seen, unhook = H.record_first_layers(ref)
    c64 = copy.copy(cam)
    c64.camera_center = cam.camera_center.double()
    out = DO.generate_neural_gaussians(c64, ref, vis_cpu, True)
    unhook()
    return out, ref, torch.cat(seen, 1)


def run(be, scene, model_cpu=None, view="ref", iterations=2, hooks=None, cams=(0, 1), vis_from=None, depth_nudge=None):
    """`iterations` iterations of the trainer's loop body on backend `be`, iteration i on camera cams[i] with the loss configuration
    `view`.  -> record (a namespace: .iters, a list of dicts of CPU tensors, one per iteration; .names, the parameter names).
    `hooks`: {"after_backward": f(namespace of be, model, pkg, scene, it, loss, params, names, vis, cam)} runs between the backward
    and training_statis.  `vis_from`: a record
    whose visibility masks are used in place of this backend's own prefilter result (which is still computed and recorded).
    `depth_nudge`: a constant [1, H, W] added to the rendered depth in front of the losses (end_to_end moves a pixel off a kink)."""
    from gscream_amd import fit as F
    hooks = hooks or {}
    model = be.model(scene.model if model_cpu is None else model_cpu)
    names = [n for n, _ in model.named_parameters()]
    params = [p for _, p in model.named_parameters()]
    opt = be.optimizer(F.adam_groups(model))
    rec = types.SimpleNamespace(backend=be.name, view=view, K=scene.K, names=names, iters=[], model=model, opt=opt)
    for it in range(iterations):
        r = {}
        rec.iters.append(r)
        cam, tg = scene.cams[cams[it]], _targets(scene.targets[cams[it]], be)
        r["cam"] = cams[it]
        F.update_learning_rate(opt, it + 1)
        state64 = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
        r["params_before"] = {n: _c(p) for n, p in zip(names, params)}
        vis, px, py = be.prefilter(cam, model, scene)
        if vis_from is not None:
            vis = vis_from.iters[it]["vis"].to(vis.device)
        r.update(vis=_c(vis), pf_x=_c(px), pf_y=_c(py), anchor=_c(model.get_anchor), anchor_scale=_c(model.get_scaling[:, :3]),
                 anchor_rot=_c(model.get_rotation))
        live = {}

        def on_decode(out, live=live):
            for o in out[:6]:
                o.retain_grad()
            live["dec"] = out
        pkg, ends = be.render(cam, model, vis, scene, on_decode)
        pkg["render"].retain_grad()
        pkg["render_depth"].retain_grad()
        dec = live["dec"]
        r.update(dec=[_c(o) for o in dec[:6]], nop=_c(dec[6]), sel_mask=_c(dec[7]), render=_c(pkg["render"]), depth=_c(pkg["render_depth"]),
                 unc_map=_c(pkg["uncertainty"]), radii=_c(pkg["radii"]), final_T=ends[0], last_gid=ends[1])
        assert pkg["selection_mask"] is dec[7] and pkg["neural_opacity"] is dec[6]
        depth_in = pkg["render_depth"] if depth_nudge is None else pkg["render_depth"] + depth_nudge.to(pkg["render_depth"])
        parts = loss_parts(be.L, view, pkg["render"], depth_in, tg)
        loss = sum(p for _, p, _ in parts)
        r["loss"], r["parts"] = float(loss.detach()), {n: float(p.detach()) for n, p, _ in parts}
        loss.backward(retain_graph=True)   # train.py:575
        r.update(g_render=_c(pkg["render"].grad), g_depth=_c(pkg["render_depth"].grad), vsp_grad=_c(pkg["viewspace_points"].grad),
                 dec_grad=[_c(o.grad) for o in dec[:6]], param_grads={n: _c(p.grad) for n, p in zip(names, params)})
        # decode backward, tied to the float64 oracle through the retained graph (see check_decode_backward)
        out_r, ref, relu_in = _oracle_decode(state64, scene, cam, r["vis"])
        al = H.align_decode_rows(dec[7], out_r[7], out_r[6])
        kinked = (relu_in.abs() <= 1e-5).any(1)
        r.update(oracle_dec=[_c(o) for o in out_r[:6]], oracle_nop=_c(out_r[6]), oracle_mask=_c(out_r[7]), kinked=kinked,
                 ambiguous=al.ambiguous.clone())
        drop = al.ambiguous | kinked.repeat_interleave(scene.K)
        have = [i for i in range(6) if dec[i].grad is not None]
        ups = [dec[i].grad.detach().clone() for i in have]
        replay = torch.autograd.grad([dec[i] for i in have], params, ups, retain_graph=True, allow_unused=True)
        r["replay_grads"] = {n: _c(g) for n, g in zip(names, replay)}
        drop_got = drop[al.keys_got].to(ups[0].device)
        for u in ups:
            u[drop_got] = 0
        second = torch.autograd.grad([dec[i] for i in have], params, ups, retain_graph=True, allow_unused=True)
        r["second_grads"] = {n: _c(g) for n, g in zip(names, second)}
        ups_ref = []
        for i, u in zip(have, ups):
            field = torch.zeros((drop.numel(), u.shape[1]), dtype=torch.float64)
            field[al.keys_got] = u.detach().cpu().double()
            ups_ref.append(field[al.keys_ref])
        pr = dict(ref.named_parameters())
        want = torch.autograd.grad([out_r[i] for i in have], [pr[n] for n in names], ups_ref, allow_unused=True)
        r["oracle_second_grads"] = {n: _c(g) for n, g in zip(names, want)}
        if "after_backward" in hooks:
            hooks["after_backward"](types.SimpleNamespace(be=be, model=model, pkg=pkg, scene=scene, it=it, loss=loss, params=params, names=names,
                                                          vis=vis, cam=cam))
        with torch.no_grad():
            be.training_statis(model, pkg, vis)
        r["acc_after"] = {n: _c(getattr(model, n)) for n in ACC_NAMES}
        adam = r["adam"] = {}
        for grp in opt.param_groups:
            for p in grp["params"]:
                n = names[[q is p for q in params].index(True)]
                st = opt.state.get(p) or {}
                adam[n] = dict(lr=grp["lr"], betas=tuple(grp["betas"]), eps=grp["eps"], t=float(st["step"]) + 1 if st else 1.0, g=_c(p.grad),
                               p_before=_c(p), m_before=_c(st["exp_avg"]) if st else torch.zeros_like(p).cpu(),
                               v_before=_c(st["exp_avg_sq"]) if st else torch.zeros_like(p).cpu())
        opt.step()
        for grp in opt.param_groups:
            for p in grp["params"]:
                n = names[[q is p for q in params].index(True)]
                st = opt.state[p]
                assert float(st["step"]) == adam[n]["t"], n
                adam[n].update(p_after=_c(p), m_after=_c(st["exp_avg"]), v_after=_c(st["exp_avg_sq"]))
        for p in params:   # zero_grad(set_to_none=True)
            p.grad = None
    rec.acc = rec.iters[-1]["acc_after"]
    return rec


def copy_record(rec):
    """A deep copy of the recorded tensors (the planted faults change a copy, never the record)."""
    new = types.SimpleNamespace(**{k: v for k, v in vars(rec).items() if k not in ("model", "opt")})
    new.iters = copy.deepcopy(rec.iters)
    new.acc = copy.deepcopy(rec.acc)
    return new


# ---- seam checks ------------------------------------------------------------------------------------------------------------------
def _raster_inputs(r, scene):
    return raster_scene(r["dec"], scene.cams[r["cam"]], scene)


def _oracle_raster(r, scene, cache):
    """The C oracle's forward state on the recorded decode outputs (shared by the forward and the backward check)."""
    key = ("st", id(r))
    if key not in cache:
        s = _raster_inputs(r, scene)
        cache[key] = (s, H.oracle_forward(s, nthreads=NTHREADS))
    return cache[key]


def check_prefilter(rec, scene, cache, worst):
    """Recorded anchors, scales and rotations through the oracle's position2D_filter: the visibility mask and the pixel centres are
    equal (tests/test_gpu_parity.py test_filters_match_oracle_and_known_answers: radii equal, centres bit-exact)."""
    for r in rec.iters:
        radii, x, y = O.position2D_filter(_np(r["anchor"]), _np(r["anchor_scale"]), _np(r["anchor_rot"]), **cam_kwargs(scene.cams[r["cam"]], scene))
        assert r["vis"].dtype == torch.bool and np.array_equal(r["vis"].numpy(), radii > 0), "prefilter: visibility mask"
        assert np.array_equal(r["pf_x"].numpy(), x) and np.array_equal(r["pf_y"].numpy(), y), "prefilter: pixel centres"
        frac = float(r["vis"].float().mean())
        assert 0.3 < frac < 0.95, f"visible fraction {frac}: the scene must hide some anchors"
        worst["visible fraction"] = frac


def check_decode_forward(rec, scene, cache, worst):
    """The float64 decode of the model under the recorded visibility mask: six outputs on the rows both kept and neural_opacity
    within 2e-5 (max_scaled_err), the mask equal wherever |neural_opacity| > 1e-5 (tests/test_gpu_decode.py)."""
    for r in rec.iters:
        al = H.align_decode_rows(r["sel_mask"], r["oracle_mask"], r["oracle_nop"])
        for nm, a, b in zip(DEC_NAMES, r["dec"], r["oracle_dec"]):
            e = H.max_scaled_err(a[al.rows_got], b[al.rows_ref])
            worst["decode " + nm] = max(worst.get("decode " + nm, 0.0), e)
            assert e <= 2e-5, ("decode forward", nm, e)
        e = H.max_scaled_err(r["nop"], r["oracle_nop"])
        worst["decode neural_opacity"] = max(worst.get("decode neural_opacity", 0.0), e)
        assert r["nop"].shape == r["oracle_nop"].shape and e <= 2e-5, ("decode forward neural_opacity", e)
        assert r["sel_mask"].dtype == torch.bool and r["dec"][0].shape[0] == int(r["sel_mask"].sum())
        assert r["sel_mask"].numel() == int(r["vis"].sum()) * scene.K


def _got_images(r):
    return dict(out_color=r["render"].numpy(), out_depth=r["depth"].numpy().reshape(1, H_IMG, W), out_unc=r["unc_map"].numpy().reshape(1, H_IMG, W),
                final_T=r["final_T"], last_gid=r["last_gid"], radii=r["radii"].numpy())


def check_raster_forward(rec, scene, cache, worst):
    """The C oracle on the recorded float32 decode outputs: helpers.assert_parity_strict on the three maps and where every pixel's
    walk ended, radii equal."""
    for r in rec.iters:
        s, st = _oracle_raster(r, scene, cache)
        assert np.array_equal(r["radii"].numpy(), st["radii"]), "raster forward: radii"
        rep = H.assert_parity_strict(_got_images(r), st, context=f"{rec.backend} raster forward", nthreads=NTHREADS)
        worst["raster forward max abs"] = max(worst.get("raster forward max abs", 0.0), rep["max_abs"])


def _oracle_losses(r, scene, view, depth=None):
    x = r["render"].double().requires_grad_(True)
    d = (r["depth"].double() if depth is None else depth.clone()).requires_grad_(True)
    tg = types.SimpleNamespace(**{k: v.double() for k, v in vars(scene.targets[r["cam"]]).items()})
    parts = loss_parts(_OracleLosses, view, x, d, tg)
    sum(p for _, p, _ in parts).backward()
    return parts, x.grad, d.grad


KINK = LH.KINK                # |aligned - target| below this is inside float32's rounding of values the size of a depth: the sign there is anybody's
KINK_MARGIN = LH.KINK_MARGIN  # the scenes as built keep every L1 residual of the cpu32 chain this far from zero (check_scene_conditions)
MAX_KINKS = 3


def l1_kinks(depth, tg):
    """The depth pixels on the L1 kink: |aligned - target| < KINK in float64, for `depth` [1, H, W] and the targets of its camera.
    -> (|scale|, shift, residual [H, W], [(y, x)])"""
    d, y, m = depth.double(), tg.depth.double(), 1.0 - tg.gt_mask.double()   # (both views fit over 1 - gt_mask)
    s, t = LO.compute_scale_and_shift(d, y, m)
    s, t = max(float(s.abs()), 1e-12), float(t)
    res = (s * d + t - y).reshape(H_IMG, W)
    return s, t, res, torch.nonzero(res.abs() < KINK).tolist()


def f32_residual_rounds_to_zero(depth, tg, s, t, yy, xx):
    """Whether float32 arithmetic gives (s d + t) - y == 0 exactly at a pixel, with or without a fused multiply-add: only then may a
    float32 implementation's |.| have the derivative 0 there."""
    f = np.float32
    s32, t32, d, y = f(s), f(t), f(depth.reshape(H_IMG, W)[yy, xx]), f(tg.depth.reshape(H_IMG, W)[yy, xx])
    plain = f(f(s32 * d) + t32) - y
    fused = f(np.float64(s32) * np.float64(d) + np.float64(t32)) - y
    return bool(plain == 0 or fused == 0)


def _mix(a, b):
    return {k: 0.5 * (a[k] + b[k]) for k in a} if isinstance(a, dict) else 0.5 * (a + b)


def sign_variants(corner, zero_ok):
    """What a quantity affine in the signs at n kink pixels may be.  corner(signs) evaluates it with every kink pixel moved to the
    side signs[i] = +1 / -1 of its kink; the sign 0 at a pixel (allowed where zero_ok[i]: float32 really rounds that residual to
    zero) is the mean of the two sides.  -> list of values, one per admissible combination."""
    import itertools
    n, cache = len(zero_ok), {}

    def value(signs):
        if signs not in cache:
            if 0 in signs:
                i = signs.index(0)
                cache[signs] = _mix(value(signs[:i] + (1,) + signs[i + 1:]), value(signs[:i] + (-1,) + signs[i + 1:]))
            else:
                cache[signs] = corner(signs)
        return cache[signs]
    return [value(c) for c in itertools.product(*[((1, -1, 0) if z else (1, -1)) for z in zero_ok])]


def _off_the_kinks(res, s, kinks, signs):
    """[1, H, W] to add to a depth map so that every kink pixel's residual becomes signs[i] * 2 KINK."""
    nudge = torch.zeros(1, H_IMG, W, dtype=torch.float64)
    for (yy, xx), sign in zip(kinks, signs):
        nudge[0, yy, xx] = (sign * 2.0 * KINK - float(res[yy, xx])) / s
    return nudge


def _depth_gradient_choices(r, scene, view, gd):
    """The oracle's depth gradient under each sign the L1 residual may take at the pixels where |aligned - target| < KINK in float64
    (a float32 evaluation lands on either side of zero there; on zero itself only where f32_residual_rounds_to_zero).  Unlike a kink
    of a neighbour difference, which moves two pixels, this one reaches every pixel of the fit mask through the scale-and-shift fit,
    with the foreground weight of the shipped configuration by as much as 1e-4 of the largest entry -- so the choice is the
    device's to make, as a mask bit within rounding of zero is in the decode seam; the bound itself is unchanged.  The gradient is
    affine in those signs: the one-sided gradients come from the oracle with the pixels' depths moved off their kinks.  The fresh
    scenes hold no such pixel (check_scene_conditions), so there the plain bound applies.  -> (list of gradients, kink pixels)"""
    tg = scene.targets[r["cam"]]
    s, t, res, kinks = l1_kinks(r["depth"], tg)
    assert len(kinks) <= MAX_KINKS, ("losses: more pixels on the L1 kink than the check enumerates", len(kinks))
    if not kinks:
        return [gd], 0
    d = r["depth"].double()
    corner = lambda signs: _oracle_losses(r, scene, view, depth=d + _off_the_kinks(res, s, kinks, signs).reshape(d.shape))[2]
    return sign_variants(corner, [f32_residual_rounds_to_zero(r["depth"], tg, s, t, yy, xx) for yy, xx in kinks]), len(kinks)


def check_losses(rec, scene, cache, worst):
    """The float64 loss oracle on the recorded render and depth.  Values: every RGB term within 2e-6, the depth term within 5e-6
    (relative beyond 1), the loss within the sum of those; the gradient arriving at `render` within 1e-4 of its largest entry; at
    `render_depth` loss_helpers.assert_depth_grad: every pixel within 1e-4 of the largest entry, except an endpoint of an EDGE term of
    the four-scale gradient loss that the oracle itself puts within KINK of zero (at most 1e-4 of the pixel count; the rendered depth
    is given, not built, so it may hold one), by no more than that term's sign can move it.  The sign at a pixel on the L1 kink, if
    there is one (at most MAX_KINKS; counted in worst["loss L1 kink pixels"]), reaches every pixel of the fit mask and stays
    enumerated on the oracle's side (_depth_gradient_choices): the gradient must pass under one of the choices."""
    for r in rec.iters:
        parts, gx, gd = _oracle_losses(r, scene, rec.view)
        total, bound = 0.0, 0.0
        for nm, p, scale in parts:
            want = float(p.detach())
            b = 5e-6 * max(1.0, abs(want)) if nm == "depth" else 2e-6
            e = abs(r["parts"][nm] - want)
            worst["loss " + nm] = max(worst.get("loss " + nm, 0.0), e)
            assert e < b, ("losses", nm, r["parts"][nm], want)
            assert want != 0.0, ("losses: a term is zero", nm)
            total, bound = total + want, bound + b
        assert abs(r["loss"] - total) < bound, ("losses: total", r["loss"], total)
        assert r["g_render"] is not None and r["g_depth"] is not None, "losses: a rendered map received no gradient"
        e = float((r["g_render"].double() - gx).abs().max() / gx.abs().max())
        worst["loss grad render"] = max(worst.get("loss grad render", 0.0), e)
        assert e <= 1e-4, ("losses: gradient at render", e)
        choices, nk = _depth_gradient_choices(r, scene, rec.view, gd)
        tg = scene.targets[r["cam"]]
        terms = LH.depth_terms(r["depth"], tg.depth, **depth_config(rec.view, tg))
        got = r["g_depth"].double().reshape(H_IMG, W).numpy()
        explained, failures = None, []
        for c in choices:
            try:
                explained = LH.assert_depth_grad(got, c.reshape(H_IMG, W).numpy(), terms, terms.scale, l1_enumerated=nk > 0, max_kinks=LH.kinks_of_continuous_data(terms),
                                                 context=f"{rec.backend} {rec.view} K={rec.K} camera {r['cam']}")
                break
            except AssertionError as err:
                failures.append(err)
        assert explained is not None, ("losses: gradient at render_depth", failures[0].args)
        worst["loss L1 kink pixels"] = max(worst.get("loss L1 kink pixels", 0), nk)
        worst["loss edge kink terms"] = max(worst.get("loss edge kink terms", 0), int((terms.k[LH.kink_terms(terms, LH.kink_margin(terms))] >= 0).sum()))
        worst["loss grad depth pixels beyond, explained"] = max(worst.get("loss grad depth pixels beyond, explained", 0), explained)


RASTER_GRADS = (("dL_dmeans3D", 0), ("dL_dcolors", 1), ("dL_dopacity", 2), ("dL_duncertainty", 3), ("dL_dscales", 4), ("dL_drotations", 5))


def check_raster_backward(rec, scene, cache, worst):
    """The C oracle's backward on the recorded decode outputs and the recorded image gradients (the uncertainty map's as zeros):
    the gradients arriving at the six decode outputs and viewspace_points.grad, helpers.assert_parity_strict."""
    for r in rec.iters:
        s, st = _oracle_raster(r, scene, cache)
        grads = (_np(r["g_render"]), _np(r["g_depth"]).reshape(1, H_IMG, W), np.zeros((1, H_IMG, W), np.float32))
        ref = H.oracle_backward(s, st, grads, nthreads=NTHREADS)
        got = _got_images(r)
        P = st["radii"].shape[0]
        for k, i in RASTER_GRADS:
            g = r["dec_grad"][i]
            assert g is not None, ("raster backward: no gradient arrived at", DEC_NAMES[i])
            got[k] = g.numpy().reshape(P, -1)
        assert r["vsp_grad"] is not None and tuple(r["vsp_grad"].shape) == (P, 3), "raster backward: viewspace_points.grad"
        got["dL_dmeans2D"] = r["vsp_grad"].numpy()
        rep = H.assert_parity_strict(got, st, ref, s=s, grads=grads, context=f"{rec.backend} raster backward", nthreads=NTHREADS)
        worst["raster backward worst rel"] = max(worst.get("raster backward worst rel", 0.0), rep["worst_rel"])


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and torch.equal(a, b))


def check_decode_backward(rec, scene, cache, worst):
    """Two steps that together tie every parameter's .grad to the float64 decode:
      * the .grad the real loss.backward left equals, bit for bit, torch.autograd.grad through the retained graph with the
        recorded arriving gradients as upstream (an output that received none is left out);
      (the uncertainty MLP's gradients are identically zero on both sides -- no loss of train.py reads the uncertainty map -- so for
      that MLP both steps show no more than that zero stays zero)
      * a second such backward, upstream zeroed on the ambiguous keys and on anchors with a hidden ReLU input within 1e-5 of zero
        (as tests/test_gpu_training_sizes.py does), is within 2e-4 (max_scaled_err) of the float64 decode's gradients under the
        same upstream gathered by key."""
    for r in rec.iters:
        for n in rec.names:
            assert _same(r["param_grads"][n], r["replay_grads"][n]), ("decode backward: .grad is not the decode's backward of the arriving gradients", n)
            a, b = r["second_grads"][n], r["oracle_second_grads"][n]
            assert (a is None) == (b is None), ("decode backward", n)
            if a is not None:
                e = H.max_scaled_err(a, b)
                worst["grad " + n] = max(worst.get("grad " + n, 0.0), e)
                assert e <= 2e-4, ("decode backward", n, e)


def check_hidden_rows(rec, scene, cache, worst):
    """Gradient rows of the per-anchor parameters outside the visibility mask are exactly zero (the sign of a zero is ignored)."""
    for r in rec.iters:
        hidden = ~r["vis"]
        assert bool(hidden.any()) and not bool(hidden.all())
        for n in HIDDEN_ROW_PARAMS:
            g = r["param_grads"][n]
            assert g is not None, n
            assert bool((g[hidden] == 0).all()), ("hidden rows", n, int((g[hidden] != 0).sum()))
            assert bool((g[~hidden] != 0).any()), ("hidden rows: no gradient reached the visible rows", n)


def check_stats(rec, scene, cache, worst):
    """The restated training_statis on the recorded tensors of every iteration, from zero: the four accumulators after the last
    iteration at rtol 1e-6, atol 1e-7 (tests/test_gpu_decode.py)."""
    N, K = scene.N, scene.K
    acc = types.SimpleNamespace(n_offsets=K, opacity_accum=torch.zeros(N, 1), anchor_demon=torch.zeros(N, 1),
                                offset_gradient_accum=torch.zeros(N * K, 1), offset_denom=torch.zeros(N * K, 1))
    for r in rec.iters:
        DO.training_statis(acc, types.SimpleNamespace(grad=r["vsp_grad"].float()), r["nop"].float(), r["radii"] > 0, r["sel_mask"], r["vis"])
    for n in ACC_NAMES:
        a, b = rec.acc[n], getattr(acc, n)
        worst["stats " + n] = float((a - b).abs().max())
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-6, atol=1e-7), ("stats", n, worst["stats " + n])
    assert float(acc.anchor_demon.max()) == len(rec.iters) and float(acc.offset_denom.sum()) > 0


def check_optimiser(rec, scene, cache, worst):
    """tests/test_adam.adam_oracle on the recorded gradients and the recorded state before each step: parameters, m and v after it
    within the three bounds of tests/test_gpu_adam.py's docstring.  Every parameter of the groups must have stepped, on the very
    gradient the backward left."""
    for r in rec.iters:
        for n, a in r["adam"].items():
            assert _same(a["g"], r["param_grads"][n]), ("optimiser: stepped on another gradient", n)
            f = lambda t: t.numpy().astype(np.float64)
            p0, g, m0, v0 = f(a["p_before"]), f(a["g"]), f(a["m_before"]), f(a["v_before"])
            ps, ms, vs, D, ss = adam_oracle(p0, g, m0, v0, a["lr"], a["betas"], a["eps"], a["t"])
            A = np.abs(a["betas"][0] * m0) + np.abs((1.0 - a["betas"][0]) * g)
            rm = np.abs(f(a["m_after"]) - ms) / (4 * U32 * A + 4 * TAU)
            rv = np.abs(f(a["v_after"]) - vs) / (5 * U32 * vs + 4 * TAU)
            rp = np.abs(f(a["p_after"]) - ps) / (2 * U32 * np.abs(ps) + 16 * U32 * ss * A / D + 4 * TAU)
            for what, ratio in (("m", rm), ("v", rv), ("p", rp)):
                worst["adam " + what] = max(worst.get("adam " + what, 0.0), float(ratio.max()))
                assert float(ratio.max()) <= 1.0, ("optimiser", n, what, float(ratio.max()))
        assert set(r["adam"]) == {n for n in rec.names if n != "_anchor"}, "optimiser: parameters that did not step"


SEAMS = {"prefilter": check_prefilter, "decode_forward": check_decode_forward, "raster_forward": check_raster_forward,
         "losses": check_losses, "raster_backward": check_raster_backward, "decode_backward": check_decode_backward,
         "hidden_rows": check_hidden_rows, "stats": check_stats, "optimiser": check_optimiser}


def check_all(rec, scene, only=None):
    """Every seam check (or those named) -> {figure: worst value measured}, printed."""
    cache, worst = {}, {}
    for name, fn in SEAMS.items():
        if only is None or name in only:
            fn(rec, scene, cache, worst)
    print(f"\n[worst] {rec.backend} {rec.view} K={rec.K}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return worst


def check_scene_conditions(rec, scene):
    """What the scene must offer for the checks to mean something (asserted from the "cpu32" backend, so the reference alone is shown
    to stay within them): few ambiguous keys and kinked anchors, hidden anchors, no loss term zero, Gaussians on both sides of
    radii > 0, no depth pixel whose L1 residual comes within KINK_MARGIN of zero (so that neither this chain nor one whose rendered
    depth differs by the image tolerance's few 1e-6 meets a kink) -- in every iteration -- and a visible anchor with every offset masked out in the scene as built (the first
    iteration: one optimiser step on the opacity MLP may well unmask it)."""
    K = scene.K
    for i, r in enumerate(rec.iters):
        Nv = int(r["vis"].sum())
        assert int(r["ambiguous"].sum()) <= 2, int(r["ambiguous"].sum())
        assert int(r["kinked"].sum()) <= Nv // 200, (int(r["kinked"].sum()), Nv)
        assert bool((~r["vis"]).any())
        assert i > 0 or bool((r["sel_mask"].view(Nv, K).sum(1) == 0).any()), "no visible anchor with every offset masked out"
        assert all(v != 0.0 for v in r["parts"].values()), r["parts"]
        on = float((r["radii"] > 0).float().mean())
        assert 0.1 <= on <= 0.9, on
        res = l1_kinks(r["depth"], scene.targets[r["cam"]])[2]
        assert float(res.abs().min()) >= KINK_MARGIN, ("a depth pixel near the L1 kink", float(res.abs().min()))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def end_to_end(rec, scene, model_cpu=None, view="ref"):
    """Every parameter gradient of `rec`'s first iteration against the fully chained oracle ("cpu64": float64 decode, cast to
    float32, C rasterizer, float64 losses, and back).  Yardstick: e_ref, the same error of the "cpu32" chain -- what float32 rounding
    alone does to the final gradients through the reference algorithm.  Rule per tensor: e <= max(4 e_ref, 1e-3 max|ref|) -- 4: the
    allowance the cross-attention tests make for an equally valid summation order; 1e-3: helpers.GRAD_REL_TOL.

    Where the oracle's own rendered depth holds a pixel on the L1 kink (l1_kinks; at most MAX_KINKS, none in the scenes as built),
    the oracle is taken under each sign that pixel's residual may have -- either side, and zero where float32 rounds the recorded
    residual to zero -- and the chain under test is held, in all its tensors, against the one of those it is nearest to: the same
    enumeration on the reference side as in the losses seam.  e_ref stays the cpu32 chain's error against the oracle as it stands.
    All e, e_ref in the gradient's own units (absolute).  The mlp_uncertainty gradients are identically zero on both sides (no loss
    of train.py reads the uncertainty map), so for that MLP this shows no more than that zero stays zero.
    -> ({name: (e, e_ref, max|ref|)}, kink pixels), printed before anything is asserted."""
    it0 = rec.iters[0]
    kw = dict(iterations=1, cams=(it0["cam"],), vis_from=rec)
    r64 = run(backend("cpu64"), scene, model_cpu, view, **kw).iters[0]
    r32 = it0 if rec.backend == "cpu32" else run(backend("cpu32"), scene, model_cpu, view, **kw).iters[0]
    assert torch.equal(r64["vis"], it0["vis"]), "the chained oracle saw another visibility mask"
    tg = scene.targets[it0["cam"]]
    s, t, res, kinks = l1_kinks(r64["depth"], tg)
    assert len(kinks) <= MAX_KINKS, ("end to end: more pixels on the L1 kink than the check enumerates", len(kinks))
    names = [n for n in rec.names if r64["param_grads"][n] is not None]
    assert names == [n for n in rec.names if it0["param_grads"][n] is not None]
    variants = [{n: r64["param_grads"][n] for n in names}]
    if kinks:
        def corner(signs):
            g = run(backend("cpu64"), scene, model_cpu, view, depth_nudge=_off_the_kinks(res, s, kinks, signs), **kw).iters[0]["param_grads"]
            return {n: g[n] for n in names}
        variants = sign_variants(corner, [f32_residual_rounds_to_zero(it0["depth"], tg, s, t, yy, xx) for yy, xx in kinks])
    mx = {n: float(r64["param_grads"][n].abs().max()) for n in names}
    errs = [{n: float((it0["param_grads"][n].double() - v[n]).abs().max()) for n in names} for v in variants]
    e = min(errs, key=lambda d: max(d[n] / mx[n] for n in names if mx[n] > 0))
    table = {n: (e[n], float((r32["param_grads"][n].double() - r64["param_grads"][n]).abs().max()), mx[n]) for n in names}
    print(f"\n[end to end] {rec.backend} {view} K={scene.K}, {len(kinks)} L1-kink pixel(s), {len(variants)} oracle variant(s): tensor, e, e_ref, max|ref|")
    for n, (e_, e_ref, m_) in table.items():
        print(f"  {n:28s} {e_:.3e} {e_ref:.3e} {m_:.3e}")
    for n, (e_, e_ref, m_) in table.items():
        assert e_ <= max(4 * e_ref, 1e-3 * m_), ("end to end", n, e_, e_ref, m_)
    return table, len(kinks)
