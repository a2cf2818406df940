"""Shared test plumbing: run a synthetic scene through the oracle or through the HIP path and compare.

Tolerances (BASELINE.json north_star): rendered RGB / depth / feature maps within 1e-4 abs, gradients
within 1e-3 rel, where rel uses the denominator |ref| + 1e-3 * max|ref| (hard part 2).
Discontinuous decisions (alpha < 1/255, T < 1e-4, ...) can flip on a 1-ulp difference of exp(); one
flip moves a pixel by up to ~4e-3 (SURVEY hard part 1), so image checks also report / bound the
fraction of outlier pixels instead of demanding zero.
"""
import numpy as np

IMG_ABS_TOL = 1e-4
GRAD_REL_TOL = 1e-3
GRAD_KEYS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_duncertainty", "dL_dscales", "dL_drotations")


def cam_kwargs(s):
    return dict(W=s["W"], H=s["H"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], viewmatrix=s["viewmatrix"],
                projmatrix=s["projmatrix"])


def oracle_forward(s, nthreads=1, **extra):
    from oracle import oracle as O
    kw = dict(colors_precomp=s.get("colors"), campos=s["campos"], bg=s["bg"], scale_modifier=s["scale_modifier"],
              nthreads=nthreads)
    if "shs" in s:
        kw.update(colors_precomp=None, shs=s["shs"], sh_degree=s["sh_degree"])
    if "cov3D_precomp" in s:
        kw.update(cov3D_precomp=s["cov3D_precomp"])
    kw.update(extra)
    scales = None if "cov3D_precomp" in s else s["scales"]
    rots = None if "cov3D_precomp" in s else s["rotations"]
    return O.forward(s["means3D"], scales, rots, s["opacities"], s["uncertainties"], **cam_kwargs(s), **kw)


def oracle_backward(s, st, grads, nthreads=1):
    from oracle import oracle as O
    gc, gd, gu = grads
    scales = None if "cov3D_precomp" in s else s["scales"]
    rots = None if "cov3D_precomp" in s else s["rotations"]
    return O.backward(st, s["means3D"], scales, rots, gc, gd, gu, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"],
                      viewmatrix=s["viewmatrix"], projmatrix=s["projmatrix"], campos=s["campos"],
                      scale_modifier=s["scale_modifier"], shs=s.get("shs"), sh_degree=s.get("sh_degree", 0),
                      nthreads=nthreads)


def oracle_envelope(s, st, grads, gids, K=64, seed=1):
    """Order-noise envelope of the reference algorithm for the Gaussians `gids` (oracle.backward_envelope)."""
    from oracle import oracle as O
    gc, gd, gu = grads
    scales = None if "cov3D_precomp" in s else s["scales"]
    rots = None if "cov3D_precomp" in s else s["rotations"]
    return O.backward_envelope(st, gids, s["means3D"], scales, rots, gc, gd, gu, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"],
                               viewmatrix=s["viewmatrix"], projmatrix=s["projmatrix"], campos=s["campos"],
                               scale_modifier=s["scale_modifier"], shs=s.get("shs"), sh_degree=s.get("sh_degree", 0), K=K, seed=seed)


VARIANTS = ("scale_modifier", "sh_deg0", "sh_deg1", "sh_deg2", "huge_gaussians", "opacity_edges", "thin_image", "tall_image",
            "tiny_gaussians")


def variant_scene(variant):
    """The scenes of tests/test_gpu_parity.py::test_more_cases_against_live_oracle (shared with tests/test_gpu_reference_kernels.py,
    which holds the oracle against the reference's own kernels on the same inputs) -> (scene, upstream gradients)."""
    import zlib
    from gscream_amd import synthetic as S
    assert variant in VARIANTS, variant
    rng = np.random.default_rng(zlib.crc32(variant.encode()) % 1000)  # (str hash() is salted per process: not a seed)
    if variant == "scale_modifier":
        s = S.scene_config1(seed=80, P=1500, W=120, H=90)
        s["scale_modifier"] = 0.6
    elif variant.startswith("sh_deg"):
        deg = int(variant[-1])
        s = S.scene_config1(seed=81 + deg, P=1200, W=112, H=80, w2c=S.random_w2c(rng))
        s["shs"] = rng.normal(0, 0.35, size=(1200, (deg + 1) ** 2, 3)).astype(np.float32)
        s["sh_degree"] = deg
        del s["colors"]
    elif variant == "huge_gaussians":
        # rectangles far beyond 64 tiles (the tile-cull mask covers the first 64; the rest is always binned)
        s = S.scene_config1(seed=85, P=300, W=320, H=256)
        s["scales"][:40] = rng.uniform(0.8, 2.5, size=(40, 3)).astype(np.float32)
        s["opacities"][:40] = rng.uniform(0.02, 0.6, size=(40, 1)).astype(np.float32)
    elif variant == "opacity_edges":
        s = S.scene_config1(seed=86, P=1500, W=120, H=90)
        s["opacities"][:300:6] = 0.0
        s["opacities"][1:300:6] = 1.0 / 255.0
        s["opacities"][2:300:6] = 0.0039
        s["opacities"][3:300:6] = 1.0
        s["opacities"][4:300:6] = 3.0     # alpha clamps at 0.99
        s["opacities"][5:300:6] = -0.5    # never blended
    elif variant == "thin_image":
        s = S.scene_config1(seed=87, P=800, W=200, H=3)
    elif variant == "tall_image":
        s = S.scene_config1(seed=88, P=800, W=5, H=130)
    else:
        s = S.scene_config1(seed=89, P=3000, W=150, H=100)
        s["scales"] *= 0.01   # sub-pixel: the 0.3 low-pass dominates
    return s, S.upstream_grads(90, s["W"], s["H"])


def hip_settings(s, device="cuda", debug=False):
    import torch
    from gscream_amd import GaussianRasterizationSettings
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]),
        scale_modifier=s["scale_modifier"], viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]),
        sh_degree=s.get("sh_degree", 1), campos=t(s["campos"]), prefiltered=False, debug=debug)


def hip_run(s, grads=None, device="cuda", debug=False, keep_state=False, rs=None):
    """Forward (+ backward if `grads`) through the public API, exactly like gaussian_renderer.render():
    means2D is a zero tensor that only carries the screen-space gradient."""
    import torch
    from gscream_amd import GaussianRasterizer
    from gscream_amd import rasterizer as RZ
    t = lambda a, rg=False: torch.from_numpy(np.ascontiguousarray(a)).to(device).requires_grad_(rg)
    rg = grads is not None
    rs = hip_settings(s, device, debug) if rs is None else rs   # (rs given: the SAME view again -- the view cache keys on its matrix)
    inp = dict(means3D=t(s["means3D"], rg), opacities=t(s["opacities"], rg), uncertainties=t(s["uncertainties"], rg))
    kw = {}
    if "cov3D_precomp" in s:
        kw["cov3D_precomp"] = t(s["cov3D_precomp"], rg)
    else:
        kw["scales"] = t(s["scales"], rg)
        kw["rotations"] = t(s["rotations"], rg)
    if "shs" in s:
        kw["shs"] = t(s["shs"], rg)
    else:
        kw["colors_precomp"] = t(s["colors"], rg)
    means2D = torch.zeros_like(inp["means3D"], requires_grad=True) + 0
    if rg:
        means2D.retain_grad()
    rast = GaussianRasterizer(raster_settings=rs)
    out = {}
    if keep_state:
        # same call, but through the internal entry so the opaque workspaces can be decoded
        e = torch.Tensor([])
        g = lambda k: kw[k].detach() if k in kw else e
        R, color, depth, unc, radii, geom, binning, img, _ns = RZ._forward_native(
            inp["means3D"].detach(), g("shs"), g("colors_precomp"), inp["opacities"].detach(),
            inp["uncertainties"].detach(), g("scales"), g("rotations"), g("cov3D_precomp"), rs)
        out.update(num_rendered=R, geom=geom, binning=binning, img=img, binning_capacity=_ns)
    else:
        color, depth, unc, radii = rast(means3D=inp["means3D"], means2D=means2D, opacities=inp["opacities"],
                                        uncertainties=inp["uncertainties"], **kw)
    out.update(out_color=color.detach().cpu().numpy(), out_depth=depth.detach().cpu().numpy(),
               out_unc=unc.detach().cpu().numpy(), radii=radii.cpu().numpy())
    if rg and not keep_state and color.grad_fn is not None and s["means3D"].shape[0] > 0:
        # where every pixel's walk ended (decoded from the workspaces autograd holds, before the backward consumes anything): the
        # Gaussian blended last and the final transmittance -- a T = 1e-4 stop that differs from the oracle's shows here directly
        out["final_T"], out["last_gid"] = walk_ends(color, s["means3D"].shape[0], s["W"], s["H"])
    if rg and not keep_state:
        gc, gd, gu = (torch.from_numpy(g).to(device) for g in grads)
        loss = (color * gc).sum() + (depth * gd).sum() + (unc * gu).sum()
        loss.backward()
        out["dL_dmeans3D"] = inp["means3D"].grad.cpu().numpy()
        out["dL_dmeans2D"] = means2D.grad.cpu().numpy()
        out["dL_dopacity"] = inp["opacities"].grad.cpu().numpy()
        out["dL_duncertainty"] = inp["uncertainties"].grad.cpu().numpy()
        if "colors_precomp" in kw:
            out["dL_dcolors"] = kw["colors_precomp"].grad.cpu().numpy()
        if "shs" in kw:
            out["dL_dsh"] = kw["shs"].grad.cpu().numpy()
        if "scales" in kw:
            out["dL_dscales"] = kw["scales"].grad.cpu().numpy()
            out["dL_drotations"] = kw["rotations"].grad.cpu().numpy()
        if "cov3D_precomp" in kw:
            out["dL_dcov3D"] = kw["cov3D_precomp"].grad.cpu().numpy()
    return out


def walk_ends(color, P, W, H):
    """(final_T [H, W], last_gid [H, W]) of the forward that produced the rendered image `color` (a tensor still attached to its
    rasterizer node, from GaussianRasterizer or from gaussian_renderer.render), decoded from the workspaces autograd holds for the
    backward.  P: the number of Gaussians that forward was given."""
    from gscream_amd import _layout
    geom, binning, img = color.grad_fn.saved_tensors[-3:]
    R = int(color.grad_fn.num_rendered)
    iv = _layout.image_views(img, P, W, H)
    bv = _layout.binning_views(binning, R, capacity=int(color.grad_fn.binning_capacity))
    last = last_gaussian(iv["ranges"].cpu().numpy().astype(np.int64), bv["point_list"].cpu().numpy().astype(np.int64),
                         (iv["n_contrib"].cpu().numpy().astype(np.int64) & 0x3fffffff), W, H)
    return iv["final_T"].cpu().numpy().copy(), last


def last_gaussian(ranges, point_list, n_contrib, W, H):
    """[H, W] id of the Gaussian each pixel blended last (-1: none): point_list[ranges[tile, 0] + n_contrib - 1].  Comparable between
    implementations whose lists differ (tile culling drops instances no pixel blends, so list POSITIONS differ, Gaussians do not)."""
    gx = (W + 15) // 16
    ys, xs = np.mgrid[0:H, 0:W]
    tile = (ys // 16) * gx + (xs // 16)
    nc = np.asarray(n_contrib, np.int64).reshape(H, W)
    pos = np.asarray(ranges, np.int64).reshape(-1, 2)[tile, 0] + nc - 1
    pl = np.asarray(point_list, np.int64)
    out = np.full((H, W), -1, np.int64)
    ok = nc > 0
    out[ok] = pl[pos[ok]]
    return out


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    den = np.abs(ref) + 1e-3 * max(np.abs(ref).max(), 1e-30)
    return float((np.abs(got - ref) / den).max())


def image_report(got, ref, tol=IMG_ABS_TOL):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    return dict(max_abs=float(d.max()) if d.size else 0.0, outliers=int((d > tol).sum()), n=int(d.size))


def assert_images_close(got, ref, name, max_outlier_frac=0.0, hard_cap=5e-3):
    """<= 1e-4 abs on EVERY pixel (round 6: the one-pixel allowance of rounds 1-5 is gone -- since the alpha = 1/255 guard band and the
    T = 1e-4 replay no GPU test shows a pixel beyond 1e-4; a pair within an ulp of expf of 1/255 is the only thing that still can, and
    assert_parity_strict names such a pixel from the oracle's own walk instead of tolerating an anonymous one).  `max_outlier_frac` is
    for comparisons between two CPU implementations with different arithmetic (tests/test_oracle.py)."""
    rep = image_report(got, ref)
    if rep["outliers"]:
        print(f"[threshold flips] {name}: {rep['outliers']} of {rep['n']} pixels beyond {IMG_ABS_TOL} (max {rep['max_abs']:.2e})")
    assert rep["outliers"] <= max_outlier_frac * rep["n"], f"{name}: {rep['outliers']}/{rep['n']} pixels differ by > {IMG_ABS_TOL} (max {rep['max_abs']:.3e})"
    # the cap is relative to the map's range: colour and feature maps live in [0, 1], a depth map holds view-space depths
    cap = hard_cap * max(1.0, float(np.abs(np.asarray(ref)).max()) if np.asarray(ref).size else 1.0)
    assert rep["max_abs"] <= cap, f"{name}: max abs error {rep['max_abs']:.3e} (cap {cap:.1e})"
    return rep


def grad_report(got, ref, tol=GRAD_REL_TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64).reshape(np.asarray(got).shape)
    if ref.size == 0:
        return dict(max=0.0, p999=0.0, n_bad=0, n=0)
    rel = np.abs(got - ref) / (np.abs(ref) + 1e-3 * max(np.abs(ref).max(), 1e-30))
    return dict(max=float(rel.max()), p999=float(np.quantile(rel, 0.999)), n_bad=int((rel > tol).sum()), n=int(rel.size))


def assert_grads_close(got, ref, keys=GRAD_KEYS, tol=GRAD_REL_TOL, context="", max_bad_frac=0.0, min_bad_allowed=0, max_rel=None):
    """Every element of every gradient family within `tol` rel (denominator |ref| + 1e-3 max|ref|).  Round 6: no allowance.  Rounds
    1-5 tolerated a handful per family (4 elements / 2e-5 of them, up to 1 % off) for alpha = 1/255 / T = 1e-4 decisions that fell the
    other way; the guard band (round 4) and the exact replay (round 5) settled those with the reference's own expressions, and what
    can still exceed `tol` -- an expf tie, or an ill-conditioned dL/dscale / dL/drot element inside the reference's own fp32
    summation-order noise -- is examined element by element by assert_parity_strict, which the oracle-backed GPU tests now use.  This
    plain form remains for comparisons against committed vectors and between implementations."""
    rep = {}
    for k in keys:
        if k not in ref or k not in got:
            continue
        rep[k] = grad_report(got[k], ref[k], tol)
    flips = {k: (v["n_bad"], round(v["max"], 5)) for k, v in rep.items() if v["n_bad"]}
    if flips:  # shows with `pytest -s` / in the failure report: (elements beyond tol, worst relative error) per family
        print(f"[beyond tol] {context}: {flips}")
    bad = {k: v for k, v in rep.items()
           if v["n_bad"] > max(min_bad_allowed, max_bad_frac * v["n"]) or (max_rel is not None and not v["max"] <= max_rel)}
    assert not bad, f"{context} gradient mismatch (rel tol {tol}): {bad}; all: {rep}"
    return {k: v["max"] for k, v in rep.items()}


def assert_grads_nearly_equal(a, b, keys=GRAD_KEYS, context=""):
    """Two HIP runs of the same math in a different summation order (other batch composition, unordered LDS adds):
    equal to rounding.  dL/dscale and dL/drot amplify rounding through the covariance chain, hence the loose max."""
    for k in keys:
        if k in a and k in b:
            rep = grad_report(a[k], b[k], tol=1e-4)
            assert rep["p999"] < 1e-4 and rep["max"] < 5e-3, f"{context} {k}: {rep}"


# Decision bands used to CLASSIFY an outlier: the oracle's walk of that pixel came within this relative distance of the
# alpha = 1/255 threshold (forward.cu:534) / the T = 1e-4 stop (forward.cu:537).  Far wider than any arithmetic difference
# between two fp32 evaluations of the same expression (~1e-6), far narrower than where a random pixel lands.
ALPHA_BAND, T_BAND = 1e-4, 1e-3


def parity_report(got, st, ref=None, nthreads=1, s=None, grads=None, envelope_orders=256, envelope_max_rows=64, keys=None):
    """Element-wise parity of HIP outputs `got` against the oracle state `st` (+ gradients `ref`), with every outlier
    classified by the decision its pixel / Gaussian sits next to in the ORACLE's walk (oracle.margins):
      alpha = only the alpha >= 1/255 test is within ALPHA_BAND, T = only the T < 1e-4 stop is within T_BAND, both, neither.
    A gradient element (row = Gaussian) is classified by whether its Gaussian is the near-threshold instance of some pixel."""
    from oracle import oracle as O
    keys = GRAD_KEYS if keys is None else tuple(keys)
    mg = O.margins(st, nthreads=nthreads)
    near_a, near_t = mg["m_alpha"] < ALPHA_BAND, mg["m_T"] < T_BAND
    H, W = near_a.shape
    bad = np.zeros((H, W), bool)
    out = {"px_gt_1e-4": 0, "max_abs": 0.0, "images": {}}
    for k in ("out_color", "out_depth", "out_unc"):
        d = np.abs(got[k].astype(np.float64) - st[k].astype(np.float64)).reshape(-1, H, W)
        out["images"][k] = {"gt_1e-4": int((d > IMG_ABS_TOL).sum()), "max": float(d.max())}
        out["max_abs"] = max(out["max_abs"], float(d.max()))
        bad |= (d > IMG_ABS_TOL).any(axis=0)
    out["px_gt_1e-4"] = int(bad.sum())
    out["px_by_cause"] = {"alpha": int((bad & near_a & ~near_t).sum()), "T": int((bad & near_t & ~near_a).sum()),
                          "both": int((bad & near_a & near_t).sum()), "neither": int((bad & ~near_a & ~near_t).sum())}
    # every outlier pixel with how close the ORACLE's own walk of it came to flipping a decision: a margin of a few 1e-7 means the pair
    # sits within an ulp of expf of the threshold -- which way it falls then depends on the libm (glibc here, ocml on the GPU, CUDA's in
    # the reference), not on the algorithm
    ys, xs = np.nonzero(bad)
    out["outlier_pixels"] = [{"x": int(x), "y": int(y), "oracle_margin_alpha_rel": float(mg["m_alpha"][y, x]), "oracle_margin_T_rel": float(mg["m_T"][y, x]),
                              "expf_tie": bool(mg["m_alpha"][y, x] < 1e-6 or mg["m_T"][y, x] < 1e-6),
                              "tie_kind": "alpha" if mg["m_alpha"][y, x] < 1e-6 else "T stop" if mg["m_T"][y, x] < 1e-6 else None}
                             for y, x in list(zip(ys, xs))[:16]]
    out["pixels_at_risk"] = {"alpha": int(near_a.sum()), "T": int(near_t.sum()), "power_sign(|power|<1e-6)": int((mg["m_pow"] < 1e-6).sum())}
    if "last_gid" in got:
        # pixels whose walk ended at another Gaussian than the oracle's: a flipped T = 1e-4 stop (or a flipped alpha test of the last instance)
        ref_last = last_gaussian(st["ranges"], st["point_list"], st["n_contrib"], W, H)
        diff = got["last_gid"] != ref_last
        # ... of which the ORACLE's own stop test came within an ulp-sized margin (1e-6 relative) of T = 1e-4: which side test_T falls on
        # then depends on the last bit of an expf upstream (glibc in the oracle, ocml on the GPU; the parity build flips the same pixels) --
        # the T-stop twin of the alpha expf tie
        # ... and `unexplained`: the differing walks whose oracle walk holds NEITHER tie (no pair within 1e-6 of alpha = 1/255, no stop
        # test within 1e-6 of T = 1e-4), counted per pixel on the walk itself, not by subtracting tie counts from a total
        out["last_contributor_differs"] = {"pixels": int(diff.sum()), "near_T_stop": int((diff & near_t).sum()), "near_alpha": int((diff & near_a & ~near_t).sum()),
                                           "expf_tie_at_the_T_stop": int((diff & (mg["m_T"] < 1e-6)).sum()),
                                           "unexplained": int((diff & ~((mg["m_alpha"] < 1e-6) | (mg["m_T"] < 1e-6))).sum())}
        ft, rt = got["final_T"].astype(np.float64), st["final_T"].astype(np.float64)
        same = ~diff & (rt > 0)
        # ... measured over the pixels whose oracle walk holds no expf tie at alpha = 1/255: where one does, glibc's and ocml's expf may put
        # that instance on opposite sides of the test somewhere IN THE MIDDLE of the walk -- T then differs by exactly that instance's
        # (1 - 1/255) = 0.39 % although both walks end at the same Gaussian and the colours agree to 1e-4 (fuzz case 56 of seed 1000)
        tie = (mg["m_alpha"] < 1e-6) | (mg["m_T"] < 1e-6)
        rel_T = np.where(same, np.abs(ft - rt) / np.where(rt > 0, rt, 1.0), 0.0)
        out["final_T_max_rel_where_same_stop"] = float(rel_T[same & ~tie].max()) if (same & ~tie).any() else 0.0
        out["final_T_in_expf_tie_walks"] = {"pixels": int((same & tie).sum()), "max_rel": float(rel_T[same & tie].max()) if (same & tie).any() else 0.0}
    if ref is not None:
        P = st["radii"].shape[0]
        ga = np.zeros(P, bool); gt = np.zeros(P, bool)
        ga[mg["g_alpha"][near_a]] = True
        gt[mg["g_T"][near_t]] = True
        out["grad_elems_gt_1e-3"], out["worst_rel"], out["grads"] = 0, 0.0, {}
        cause = {"alpha": 0, "T": 0, "both": 0, "neither": 0}
        # Gaussians in the walk of a pixel whose alpha decision is an expf tie (see outlier_pixels): if the pair fell the other way on
        # the GPU, every instance BEHIND it in that pixel sees another transmittance -- their rows move together with the tied one's
        tied = np.zeros(P, bool)
        gxt = (W + 15) // 16
        tie_px = (mg["m_alpha"] < 1e-6) | (mg["m_T"] < 1e-6)
        for y, x in zip(*np.nonzero(tie_px)):
            t = (y // 16) * gxt + x // 16
            r0, r1 = int(st["ranges"][t][0]), int(st["ranges"][t][1])
            # (a tie at the T stop: the walk that falls the other way blends one more instance -- the next one of the list that reaches
            # the pixel, a few positions behind the oracle's last contributor)
            extra = 64 if mg["m_T"][y, x] < 1e-6 else 0
            tied[np.asarray(st["point_list"][r0:min(r1, r0 + int(st["n_contrib"][y, x]) + extra)], np.int64)] = True
        tie_rows = 0
        for k in keys:
            if k in ref and k in got:
                g64 = np.asarray(got[k], np.float64)
                r64 = np.asarray(ref[k], np.float64).reshape(g64.shape)
                if r64.size == 0:
                    continue
                r = np.abs(g64 - r64) / (np.abs(r64) + 1e-3 * max(np.abs(r64).max(), 1e-30))
                badrows = (r > GRAD_REL_TOL).reshape(P, -1)
                nb = int(badrows.sum())
                out["grads"][k] = {"n_bad": nb, "max": float(r.max()) if r.size else 0.0}
                out["grad_elems_gt_1e-3"] += nb
                out["worst_rel"] = max(out["worst_rel"], out["grads"][k]["max"])
                per_row = badrows.sum(axis=1)
                cause["alpha"] += int(per_row[ga & ~gt].sum()); cause["T"] += int(per_row[gt & ~ga].sum())
                cause["both"] += int(per_row[ga & gt].sum()); cause["neither"] += int(per_row[~ga & ~gt].sum())
                tie_rows += int(per_row[tied].sum())
        out["grad_elems_by_cause"] = cause
        out["grad_elems_in_walks_of_expf_tie_pixels"] = {"elements": tie_rows, "tie_pixels": int(tie_px.sum()),
                                                         "note": "outlier elements of Gaussians some pixel blends together with a pair whose alpha lies within 1e-6 (relative) of 1/255 in "
                                                                 "the oracle, or in a walk whose stop test lies within 1e-6 (relative) of T = 1e-4 there"}
        if s is not None and grads is not None and out["grad_elems_gt_1e-3"]:
            # ORDER-NOISE ENVELOPE (round 5): the reference scatters its per-contribution terms with unordered fp32 atomicAdd
            # (backward.cu:554-601), so its own result for a Gaussian moves with the order its pixels were served in.  For every
            # outlier row: the same sums in `envelope_orders` random orders (oracle.backward_envelope) -> is our value inside the
            # range the reference algorithm itself produces?  Listed per element with the range.
            rows = np.zeros(P, bool)
            fam_bad = {}
            for k in keys:
                if k in ref and k in got and np.asarray(ref[k]).size:
                    g64 = np.asarray(got[k], np.float64)
                    r64 = np.asarray(ref[k], np.float64).reshape(g64.shape)
                    r = np.abs(g64 - r64) / (np.abs(r64) + 1e-3 * max(np.abs(r64).max(), 1e-30))
                    fam_bad[k] = (r > GRAD_REL_TOL).reshape(P, -1)
                    rows |= fam_bad[k].any(axis=1)
            gids = np.nonzero(rows)[0][:envelope_max_rows].astype(np.int32)
            env = oracle_envelope(s, st, grads, gids, K=envelope_orders)
            listing, inside, outside = [], 0, 0
            for qi, g in enumerate(gids):
                for k, fb in fam_bad.items():
                    if k not in env:
                        continue
                    for c in np.nonzero(fb[g])[0]:
                        ours = float(np.asarray(got[k]).reshape(P, -1)[g, c])
                        dbl = float(np.asarray(ref[k]).reshape(P, -1)[g, c])
                        e = env[k][qi].reshape(envelope_orders, -1)[:, c].astype(np.float64)
                        lo, hi = float(e.min()), float(e.max())
                        half = max(abs(lo - dbl), abs(hi - dbl))
                        ok = lo <= ours <= hi
                        inside += ok; outside += (not ok)
                        cls = "alpha" if (ga[g] and not gt[g]) else "T" if (gt[g] and not ga[g]) else "both" if (ga[g] and gt[g]) else "neither"
                        listing.append({"gaussian": int(g), "family": k, "component": int(c), "cause": cls, "in_expf_tie_walk": bool(tied[g]), "ours": ours, "oracle_double": dbl,
                                        "reference_fp32_orders_min": lo, "reference_fp32_orders_max": hi,
                                        "ours_minus_double_over_envelope_halfwidth": (abs(ours - dbl) / half) if half > 0 else float("inf"),
                                        "inside_envelope": bool(ok)})
            out["order_noise_envelope"] = {"orders": envelope_orders, "rows_examined": int(len(gids)), "rows_total": int(rows.sum()),
                                           "elements_inside": int(inside), "elements_outside": int(outside),
                                           "elements_outside_not_in_an_expf_tie_walk": int(sum(1 for e in listing if not e["inside_envelope"] and not e["in_expf_tie_walk"])),
                                           "elements": listing}
    out["bands"] = {"alpha_rel": ALPHA_BAND, "T_rel": T_BAND}
    return out


STRICT_KEYS = GRAD_KEYS + ("dL_dsh", "dL_dcov3D")


def assert_parity_strict(got, st, ref=None, s=None, grads=None, context="", keys=STRICT_KEYS, nthreads=1, max_ties=2, envelope_max_rows=64):
    """The BAR itself, as tests/test_gpu_fullsize.py asserts it at BASELINE's sizes (round 6: every small-scene case too; the blanket
    allowances of assert_images_close / assert_grads_close -- one pixel up to 5e-3, four elements per family up to 1 % -- predate the
    alpha guard band and the T = 1e-4 replay):
      * a pixel may differ from the oracle by more than 1e-4 only if the ORACLE's own walk of it holds a pair within 1e-6 (relative)
        of alpha = 1/255, or ends with a stop test within 1e-6 (relative) of T = 1e-4 -- an expf tie, settled by the libm (glibc in the
        oracle, ocml on the GPU, CUDA's in the reference): one more or one fewer instance blended (seed-2000 sweep, case 39: the depth
        of one pixel moves by 3.7e-4, its colour by 9.6e-5);
      * no pixel's walk may end at another Gaussian than the oracle's, ties apart (alpha ties, and pixels whose stop test in the oracle
        lies within 1e-6 (relative) of T = 1e-4: the same expf tie on the other decision);
      * a gradient element may differ by more than 1e-3 (rel; |ref| + 1e-3 max|ref|) only if our value lies inside the range the
        reference algorithm's own unordered fp32 atomicAdd sums span (oracle.backward_envelope, 256 random orders), or its Gaussian
        is blended by a tie pixel; every such element is examined, none is waved through.
    Returns the classified report (printed when anything was classified)."""
    rep = parity_report(got, st, ref, nthreads=nthreads, s=s, grads=grads, keys=keys, envelope_max_rows=envelope_max_rows)
    ties = sum(1 for p_ in rep["outlier_pixels"] if p_["expf_tie"])
    assert rep["px_gt_1e-4"] <= len(rep["outlier_pixels"]), f"{context}: {rep['px_gt_1e-4']} pixels beyond {IMG_ABS_TOL}: more than the report lists"
    assert rep["px_gt_1e-4"] == ties <= max_ties, \
        f"{context}: {rep['px_gt_1e-4']} pixels beyond {IMG_ABS_TOL}, {ties} of them expf ties: {rep['outlier_pixels']} ({rep['images']})"
    for k in ("out_color", "out_depth", "out_unc"):
        cap = 5e-3 * max(1.0, float(np.abs(st[k]).max()) if np.asarray(st[k]).size else 1.0)
        assert rep["images"][k]["max"] <= cap, f"{context}/{k}: max abs error {rep['images'][k]['max']:.3e} (cap {cap:.1e})"
    if "final_T_max_rel_where_same_stop" in rep:  # (over the pixels without an expf tie in their oracle walk: parity_report; asserted
        # whether or not the frame holds a tie elsewhere -- one tie pixel must not switch the bound off for every other pixel)
        # the forward's exact replay finds every pixel whose stop could differ from the reference's ONLY IF the fast walk's transmittance
        # stays within GSR_TBAND (1e-4, relative) of the reference chain's (blend.hip, GSR_T_STOP); v_exp / v_rcp errors accumulate with
        # the number of blends, so the bound is checked on every case here, the walks of thousands of instances included
        assert rep["final_T_max_rel_where_same_stop"] < 1e-4, f"{context}: fast-walk T drifts {rep['final_T_max_rel_where_same_stop']:.2e} from the oracle's chain (band 1e-4)"
    if "last_contributor_differs" in rep:
        lc = rep["last_contributor_differs"]
        if lc["pixels"]:
            print(f"[classified] {context}: walks ending at another Gaussian than the oracle's: {lc}")
        # every differing walk must itself be a tie walk: a pixel that is both an image outlier and a T-stop tie appears in `ties` AND in
        # expf_tie_at_the_T_stop, so the count bound below alone would let one unexplained walk through beside it
        assert lc["unexplained"] == 0, f"{context}: walks ending at another Gaussian than the oracle's with no expf tie in the oracle's walk: {lc}"
        assert lc["pixels"] <= ties + lc["expf_tie_at_the_T_stop"] and lc["expf_tie_at_the_T_stop"] <= max_ties, \
            f"{context}: walks ending at another Gaussian than the oracle's: {lc}"
    if ref is not None:
        nb = rep["grad_elems_gt_1e-3"]
        if nb:
            env = rep.get("order_noise_envelope")
            assert env is not None, f"{context}: {nb} gradient elements beyond {GRAD_REL_TOL} and no scene / upstream gradients to examine them with"
            bad_fams = {k: v for k, v in rep["grads"].items() if v["n_bad"]}
            print(f"[classified] {context}: {nb} gradient elements beyond {GRAD_REL_TOL} (worst {rep['worst_rel']:.2e}; {bad_fams}): "
                  f"{env['elements_inside']} inside the reference algorithm's own fp32 order range, {env['elements_outside']} outside, "
                  f"{rep['grad_elems_in_walks_of_expf_tie_pixels']['elements']} in walks of {ties} tie pixel(s)")
            assert env["rows_examined"] == env["rows_total"], f"{context}: {env['rows_total']} outlier rows, the envelope examines {env['rows_examined']}"
            assert env["elements_inside"] + env["elements_outside"] == nb, f"{context}: {nb} outlier elements, {env['elements_inside'] + env['elements_outside']} examined"
            stray = [e for e in env["elements"] if not e["inside_envelope"] and not e["in_expf_tie_walk"]]
            assert not stray, f"{context}: gradient elements beyond {GRAD_REL_TOL} outside the reference's own order range and in no tie walk: {stray}"
        for k in rep["grads"]:  # 99.9th percentile inside the tolerance wherever 0.1 % of a family is more than a handful
            g = grad_report(got[k], ref[k])
            assert g["n"] < 4000 or g["p999"] <= GRAD_REL_TOL, f"{context}/{k}: {g}"
    if ties:
        print(f"[classified] {context}: {ties} expf-tie pixel(s): {[p_ for p_ in rep['outlier_pixels'] if p_['expf_tie']]}")
    return rep



# ---- compacted decode rows at training sizes -------------------------------------------------------------------------
# The decode keeps offset k of anchor n (key n*K + k) when tanh(z) > 0.  With millions of keys, some z sits within fp32
# rounding of zero and the kernel and the fp64 oracle may keep different sets; a seed search for a clean mask does not
# scale.  Instead both sides' output rows are mapped back to their keys and compared on the keys both kept, and the
# upstream gradient is one field over the keys, zero where the masks differ, gathered by each side through its own mask.
def align_decode_rows(mask_got, mask_ref, nop_ref, sure=1e-5):
    """mask_got / mask_ref: the two selection masks [Nv*K]; nop_ref: the reference's neural_opacity (same keys).
    Asserts that the masks agree wherever |nop_ref| > `sure`.  Returns a namespace with
      keys_got / keys_ref : the key of every output row of each side (its mask's nonzero positions, in row order)
      rows_got / rows_ref : for every key both sides kept, its output row on either side (ascending key order)
      ambiguous           : bool [Nv*K], the keys where the masks differ
    """
    import types
    import torch
    mg = mask_got.detach().cpu().view(-1).bool()
    mr = mask_ref.detach().cpu().view(-1).bool()
    assert mg.shape == mr.shape, (mg.shape, mr.shape)
    diff = mg != mr
    near_zero = nop_ref.detach().cpu().view(-1).abs() <= sure
    assert not bool((diff & ~near_zero).any()), f"mask differs away from zero at keys {torch.nonzero(diff & ~near_zero).view(-1)[:8].tolist()}"
    row_g = torch.cumsum(mg.long(), 0) - 1  # output row of key i on either side (valid where the mask keeps i)
    row_r = torch.cumsum(mr.long(), 0) - 1
    both = torch.nonzero(mg & mr).view(-1)
    return types.SimpleNamespace(keys_got=torch.nonzero(mg).view(-1), keys_ref=torch.nonzero(mr).view(-1),
                                 rows_got=row_g[both], rows_ref=row_r[both], ambiguous=diff)


def upstream_fields(nkeys, widths, ambiguous, generator, mean=0.0, dtype=None):
    """One random upstream-gradient field [nkeys, w] per output width (N(mean, 1) entries), zero on the ambiguous keys."""
    import torch
    out = []
    for w in widths:
        f = torch.randn((nkeys, w), generator=generator, dtype=dtype or torch.float64) + mean
        f[ambiguous] = 0.0
        out.append(f)
    return out


def max_scaled_err(a, b):
    """max |a - b| / max(1, max |b|): the measure of the decode tests' `_close`."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    if not a.numel():
        return 0.0
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


def morton_bucket_counts(pts, bits=12):
    """Occupancy of the kNN kernel's Morton buckets (knn.hip gsk_morton_kernel): the cloud's bounding box (its reduction
    starts from the origin), 10-bit cells per axis in fp32, x | y << 1 | z << 2 interleaved, bucket = the top `bits` of the
    30-bit code."""
    p = np.asarray(pts, dtype=np.float32)
    lo = np.minimum(p.min(0), np.float32(0)).astype(np.float32)
    hi = np.maximum(p.max(0), np.float32(0)).astype(np.float32)
    q = (((p - lo) / (hi - lo)) * np.float32(1023)).astype(np.uint32)
    code = np.zeros(p.shape[0], np.uint32)
    for b in range(10):
        for k in range(3):
            code |= ((q[:, k] >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b + k)
    return np.bincount(code >> np.uint32(30 - bits), minlength=1 << bits)


def record_first_layers(model, names=("mlp_opacity", "mlp_uncertainty", "mlp_color", "mlp_cov")):
    """Forward hooks on the first Linear layer of the decode's four MLPs: -> (list that collects their outputs, the ReLU
    inputs [n, 32] of every decoded anchor, in call order; a function that removes the hooks).  A ReLU input within fp32
    rounding of zero flips the unit's derivative between an fp32 kernel and the fp64 oracle: the anchor's input gradient
    then differs by a whole weight column, as CPU fp32 torch on the same expressions shows.  (Cloned: the ReLU runs in place.)"""
    seen = []
    hooks = [getattr(model, n)[0].register_forward_hook(lambda _m, _i, o: seen.append(o.detach().clone())) for n in names]
    return seen, lambda: [h.remove() for h in hooks]
