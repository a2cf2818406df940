"""The iteration harness of tests/iteration_helpers.py, proven without a GPU: the "cpu32" backend (the oracles chained in float32)
passes every seam check and every scene condition, and each seam check raises on the fault it exists for, planted into a copy of
the record.  tests/test_gpu_iteration.py runs the same checks on the HIP chain.  Also the CPU half of the pointer guard:
_native.ptr() refuses host memory."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iteration_helpers as IH  # noqa: E402

_cache = {}


def scene(K):
    if K not in _cache:
        _cache[K] = IH.build_scene(K)
    return _cache[K]


def record(view, K):
    if (view, K) not in _cache:
        _cache[view, K] = IH.run(IH.backend("cpu32"), scene(K), view=view)
    return _cache[view, K]


@pytest.mark.parametrize("K", [10, 4])
def test_scene_is_what_the_issue_asks_for(K):
    sc = scene(K)
    assert 1500 <= sc.N <= 2500 and sc.N % 16 and sc.N % 256
    assert IH.W % 16 and IH.H_IMG % 16
    for tg in sc.targets:
        assert tg.image.shape == (3, IH.H_IMG, IH.W) and float(tg.image.std()) > 0.01 and float(tg.depth.std()) > 0.01
        assert 0 < float(tg.gt_mask.mean()) < float(tg.fg_mask.mean()) < 1


@pytest.mark.parametrize("K", [10, 4])
@pytest.mark.parametrize("view", ["ref", "other"])
def test_cpu32_chain_passes_every_seam(view, K):
    """Two iterations of the float32 oracle chain: the scene conditions, every seam check, and the end-to-end rule (whose yardstick
    is this very chain, so here it shows only that the fully chained oracle runs and sees the same masks)."""
    rec, sc = record(view, K), scene(K)
    IH.check_scene_conditions(rec, sc)
    worst = IH.check_all(rec, sc)
    assert worst["raster forward max abs"] == 0.0 and worst["raster backward worst rel"] == 0.0  # the same C code on the same inputs
    assert worst["loss L1 kink pixels"] == 0   # the scenes as built: the plain depth-gradient bound
    table, kinks = IH.end_to_end(rec, sc, view=view)
    assert kinks == 0 and set(table) == set(rec.names)
    assert all(e == e_ref for e, e_ref, _ in table.values())
    live = [n for n, (_, _, mx) in table.items() if mx > 0]
    assert {"_anchor", "_anchor_feat", "_offset", "_scaling", "mlp_opacity.2.bias", "mlp_cov.2.bias", "mlp_color.2.bias"} <= set(live)


def _swap_opacity_and_uncertainty(rec):
    g = rec.iters[0]["dec_grad"]
    g[2], g[3] = g[3], g[2]


def _zero_depth_gradient(rec):
    rec.iters[0]["g_depth"].zero_()


def _depth_gradient_shifted(rec):
    g = rec.iters[0]["g_depth"]
    g += 2e-4 * g.abs().max()


def _depth_gradient_scaled(rec):
    rec.iters[0]["g_depth"] *= 1.0 + 2e-4


def _one_depth_pixel_wrong(rec):
    """One pixel of 17 472 off by ten bounds: inside the old `2e-3 of the pixels may be anything`; no term of that pixel is near zero."""
    g = rec.iters[0]["g_depth"]
    g[0, 50, 80] += 1e-3 * g.abs().max()


def _second_backward_cov_bias_scaled(rec):
    rec.iters[0]["second_grads"]["mlp_cov.2.bias"] *= 1.0 + 1e-3


def _second_backward_opacity_and_uncertainty_swapped(rec):
    g = rec.iters[0]["second_grads"]
    g["mlp_opacity.2.bias"], g["mlp_uncertainty.2.bias"] = g["mlp_uncertainty.2.bias"], g["mlp_opacity.2.bias"]


def _viewspace_in_ndc_units(rec):
    rec.iters[0]["vsp_grad"][:, :2] *= 0.5 * IH.W


def _one_hidden_row(rec):
    r = rec.iters[0]
    row = int(torch.nonzero(~r["vis"]).view(-1)[0])
    r["param_grads"]["_anchor_feat"][row, 5] = 1e-12


def _offset_rolled(rec):
    g = rec.iters[0]["param_grads"]
    g["_offset"] = torch.roll(g["_offset"], 1, 0)


def _cov_bias_scaled(rec):
    rec.iters[0]["param_grads"]["mlp_cov.2.bias"] *= 1.0 + 1e-3


def _stats_of_first_iteration(rec):
    rec.acc = rec.iters[0]["acc_after"]


def _adam_v_one_step_late(rec):
    a = rec.iters[1]["adam"]["_offset"]
    a["v_after"] = a["v_before"].clone()


FAULTS = [("raster_backward", _swap_opacity_and_uncertainty), ("losses", _zero_depth_gradient), ("raster_backward", _viewspace_in_ndc_units),
          ("hidden_rows", _one_hidden_row), ("decode_backward", _offset_rolled), ("decode_backward", _cov_bias_scaled),
          ("stats", _stats_of_first_iteration), ("optimiser", _adam_v_one_step_late),
          # beyond the issue's list: the tolerance halves of two checks, which the faults above never reach
          ("losses", _depth_gradient_shifted), ("losses", _depth_gradient_scaled), ("losses", _one_depth_pixel_wrong),
          ("decode_backward", _second_backward_cov_bias_scaled),
          ("decode_backward", _second_backward_opacity_and_uncertainty_swapped)]


@pytest.mark.parametrize("seam,plant", FAULTS, ids=[f.__name__.lstrip("_") for _, f in FAULTS])
def test_planted_fault_is_caught(seam, plant):
    """A fault planted into a copy of the ref / K = 10 record (no package code is touched) makes the seam check named for it raise;
    the untouched copy passes that same check."""
    rec, sc = record("ref", 10), scene(10)
    good = IH.copy_record(rec)
    IH.check_all(good, sc, only=(seam,))
    bad = IH.copy_record(rec)
    plant(bad)
    with pytest.raises(AssertionError):
        IH.check_all(bad, sc, only=(seam,))


def test_every_seam_has_a_planted_fault_or_is_exact():
    """prefilter, decode_forward and raster_forward compare outputs the planted faults (all on gradients and state) do not touch:
    they are shown to bite by a perturbed output each."""
    rec, sc = record("ref", 10), scene(10)
    assert {s for s, _ in FAULTS} | {"prefilter", "decode_forward", "raster_forward"} == set(IH.SEAMS)
    for seam, plant in (("prefilter", lambda r: r.iters[0]["pf_x"].__setitem__(int(torch.nonzero(r.iters[0]["vis"])[0]), 1.0)),
                        ("decode_forward", lambda r: r.iters[0]["dec"][4].mul_(1.0 + 1e-4)),
                        ("raster_forward", lambda r: r.iters[0]["depth"].__setitem__((0, 50, 80), r.iters[0]["depth"][0, 50, 80] + 1e-3))):
        bad = IH.copy_record(rec)
        plant(bad)
        with pytest.raises(AssertionError):
            IH.check_all(bad, sc, only=(seam,))


def test_l1_kink_pixel_is_enumerated_and_the_bound_still_bites():
    """The scenes as built hold no depth pixel on the L1 kink; a model that has trained for a while may.  One is made here: the
    foreground pixel nearest to the kink has its depth moved until its residual is 1e-7, and the depth gradient "under test" is the
    oracle's with that pixel on the OTHER side of zero (what a float32 evaluation may give).  That gradient differs from the oracle's
    as it stands by a whole sign at the pixel and, through the scale-and-shift fit, a little at every pixel of the fit mask (in the
    first GPU audit of this harness: just over 1e-4 of the largest entry at 129 pixels).  The losses seam, which takes the oracle
    under either sign, passes; the same gradient shifted by 2e-4 of its largest entry still fails."""
    rec, sc = IH.copy_record(record("ref", 10)), scene(10)
    r = rec.iters[0]
    tg = sc.targets[r["cam"]]
    s, t, res, kinks = IH.l1_kinks(r["depth"], tg)
    assert not kinks
    near = torch.where(tg.fg_mask[0] > 0, res.abs(), torch.full_like(res, 1e9))   # inside the foreground box (weight 100), and the
    yy, xx = divmod(int(near.argmin()), IH.W)                                      # nearest to the kink already: the loss barely moves
    assert float(near[yy, xx]) < 1e-3
    r["depth"][0, yy, xx] += float((1e-7 - res[yy, xx]) / s)
    s, t, res, kinks = IH.l1_kinks(r["depth"], tg)
    assert kinks == [[yy, xx]] and 0 < float(res[yy, xx]) < IH.KINK
    plain = IH._oracle_losses(r, sc, "ref")[2]
    other = r["depth"].double().clone()
    other[0, yy, xx] -= 2.0 * IH.KINK / s
    flipped = IH._oracle_losses(r, sc, "ref", depth=other)[2]
    assert float((flipped - plain).abs().max()) > 0.1 * float(plain.abs().max())   # a whole sign at weight 100, at its own pixel
    assert float((flipped - plain).abs().median()) > 0                             # and something at every pixel of the fit mask
    r["g_depth"] = flipped.float().reshape(r["g_depth"].shape)
    worst = IH.check_all(rec, sc, only=("losses",))
    assert worst["loss L1 kink pixels"] == 1
    r["g_depth"] = (flipped + 2e-4 * flipped.abs().max()).float().reshape(r["g_depth"].shape)
    with pytest.raises(AssertionError):
        IH.check_all(rec, sc, only=("losses",))


# ---- the device of a pointer ------------------------------------------------------------------------------------------------------
def test_ptr_refuses_host_memory():
    from gscream_amd import _native
    with pytest.raises(RuntimeError, match="HIP kernel"):
        _native.ptr(torch.zeros(3))
    with pytest.raises(RuntimeError):
        _native.ptr(torch.zeros(4, dtype=torch.bool))


def test_ptr_is_null_for_none_and_empty_tensors():
    from gscream_amd import _native
    assert _native.ptr(None) is None
    assert _native.ptr(torch.zeros(0)) is None and _native.ptr(torch.zeros((0, 3), dtype=torch.int32)) is None
