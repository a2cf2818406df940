"""CPU tests of the gate itself: helpers.assert_parity_strict on synthetic reports and on an oracle state with one
planted difference.  The GPU parity tests (and tests/test_gpu_reference_kernels.py) lean on this gate, so what it lets
through is checked without a GPU."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers as Hh  # noqa: E402
from gscream_amd import synthetic as S  # noqa: E402

_ST = {k: np.zeros((1, 4, 4), np.float32) for k in ("out_color", "out_depth", "out_unc")}
_TIE_PIXEL = {"x": 1, "y": 2, "oracle_margin_alpha_rel": 0.3, "oracle_margin_T_rel": 4e-7, "expf_tie": True, "tie_kind": "T stop"}


def _report(**kw):
    """A clean report of parity_report's shape: no outlier, no differing walk, T drift far inside the band."""
    rep = {"px_gt_1e-4": 0, "max_abs": 1e-6, "images": {k: {"gt_1e-4": 0, "max": 1e-6} for k in _ST}, "outlier_pixels": [],
           "last_contributor_differs": {"pixels": 0, "near_T_stop": 0, "near_alpha": 0, "expf_tie_at_the_T_stop": 0, "unexplained": 0},
           "final_T_max_rel_where_same_stop": 2e-6, "final_T_in_expf_tie_walks": {"pixels": 0, "max_rel": 0.0}}
    rep.update(copy.deepcopy(kw))
    return rep


def _gate(monkeypatch, rep):
    monkeypatch.setattr(Hh, "parity_report", lambda *a, **k: rep)
    return Hh.assert_parity_strict({}, _ST, context="synthetic")


def test_clean_report_and_one_classified_tie_pass(monkeypatch):
    _gate(monkeypatch, _report())
    # one pixel that is an image outlier AND whose walk ends elsewhere, both explained by the same T-stop tie
    tie = _report(**{"px_gt_1e-4": 1, "outlier_pixels": [_TIE_PIXEL],
                     "last_contributor_differs": {"pixels": 1, "near_T_stop": 1, "near_alpha": 0, "expf_tie_at_the_T_stop": 1, "unexplained": 0}})
    tie["images"]["out_depth"] = {"gt_1e-4": 1, "max": 3.7e-4}
    _gate(monkeypatch, tie)


def test_unexplained_walk_beside_a_double_counted_tie_fails(monkeypatch):
    """The tie pixel counts once as an image outlier and once as a T-stop tie: 2 differing walks <= 1 + 1 held although the
    second walk has no tie at all."""
    rep = _report(**{"px_gt_1e-4": 1, "outlier_pixels": [_TIE_PIXEL],
                     "last_contributor_differs": {"pixels": 2, "near_T_stop": 1, "near_alpha": 0, "expf_tie_at_the_T_stop": 1, "unexplained": 1}})
    with pytest.raises(AssertionError, match="no expf tie"):
        _gate(monkeypatch, rep)


def test_a_single_unexplained_walk_fails(monkeypatch):
    rep = _report(last_contributor_differs={"pixels": 1, "near_T_stop": 0, "near_alpha": 0, "expf_tie_at_the_T_stop": 0, "unexplained": 1})
    with pytest.raises(AssertionError, match="no expf tie"):
        _gate(monkeypatch, rep)


def test_drift_bound_holds_on_non_tie_pixels_when_a_tie_exists(monkeypatch):
    rep = _report(**{"px_gt_1e-4": 1, "outlier_pixels": [_TIE_PIXEL], "final_T_max_rel_where_same_stop": 3e-4,
                     "last_contributor_differs": {"pixels": 1, "near_T_stop": 1, "near_alpha": 0, "expf_tie_at_the_T_stop": 1, "unexplained": 0}})
    with pytest.raises(AssertionError, match="drifts"):
        _gate(monkeypatch, rep)
    with pytest.raises(AssertionError, match="drifts"):
        _gate(monkeypatch, _report(final_T_max_rel_where_same_stop=3e-4))


def test_too_many_ties_and_anonymous_outliers_still_fail(monkeypatch):
    three = _report(**{"px_gt_1e-4": 3, "outlier_pixels": [_TIE_PIXEL] * 3})
    with pytest.raises(AssertionError):
        _gate(monkeypatch, three)
    anonymous = _report(**{"px_gt_1e-4": 1, "outlier_pixels": [dict(_TIE_PIXEL, expf_tie=False, tie_kind=None, oracle_margin_T_rel=0.2)]})
    with pytest.raises(AssertionError):
        _gate(monkeypatch, anonymous)


def test_planted_walk_difference_on_a_real_oracle_state_is_counted_and_refused():
    """The real parity_report on the oracle's own outputs: identical -> passes; the last contributor of one pixel with no tie
    in its walk replaced by another Gaussian -> `unexplained` counts it and the gate refuses it."""
    from oracle import oracle as O
    s = S.scene_config1(seed=3, P=300, W=48, H=32)
    st = Hh.oracle_forward(s)
    got = {k: st[k].copy() for k in ("out_color", "out_depth", "out_unc", "final_T")}
    got["last_gid"] = Hh.last_gaussian(st["ranges"], st["point_list"], st["n_contrib"], s["W"], s["H"])
    rep = Hh.assert_parity_strict(got, st, context="oracle vs itself")
    assert rep["last_contributor_differs"] == {"pixels": 0, "near_T_stop": 0, "near_alpha": 0, "expf_tie_at_the_T_stop": 0, "unexplained": 0}
    mg = O.margins(st)
    free = (got["last_gid"] >= 0) & (mg["m_alpha"] > Hh.ALPHA_BAND) & (mg["m_T"] > Hh.T_BAND)
    assert free.any()
    y, x = (int(v[0]) for v in np.nonzero(free))
    got["last_gid"][y, x] = (got["last_gid"][y, x] + 1) % 300
    rep = Hh.parity_report(got, st)
    assert rep["last_contributor_differs"]["pixels"] == 1 and rep["last_contributor_differs"]["unexplained"] == 1
    with pytest.raises(AssertionError, match="no expf tie"):
        Hh.assert_parity_strict(got, st, context="planted")
    # a drifted transmittance on one such pixel: refused as well
    got["last_gid"][y, x] = Hh.last_gaussian(st["ranges"], st["point_list"], st["n_contrib"], s["W"], s["H"])[y, x]
    got["final_T"][y, x] *= np.float32(1.0 + 5e-4)
    with pytest.raises(AssertionError, match="drifts"):
        Hh.assert_parity_strict(got, st, context="planted drift")
