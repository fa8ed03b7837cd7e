"""CPU side of the held-out validation rows (include/mk.h: log score, Brier score, error rate):
tests/score_ref.py, the restatement the GPU tests compare the device with, is pinned here against cases
worked by hand, validation_report's AUC and reliability table too, and the binding is checked against
the header."""
import ctypes
import os
import re
from math import log

import numpy as np
import pytest

from score_ref import NAMES, score_ref, score_ref_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mk.h")


def test_two_states_by_hand():
    """Two states with p = (1/4, 3/4) in every column.
    (y, wt) = (1, 1): pmean 1/2, exp(l) = (1/4, 3/4), lpd ln(1/2), squared error (1/2 - 1)^2 = 1/4;
    (2, 3): exp(l) = p^2 (1 - p) = (3/64, 9/64), their mean 3/32, squared error (1/2 - 2/3)^2 = 1/36,
            lconst ln C(3, 2) = ln 3;
    wt = 0: lpd 0 and not counted.
    pmean = 1/2 >= 0.5 predicts 1 everywhere: wrong trials 0 + 1 of 4."""
    p = np.tile(np.array([[0.25], [0.75]]), (1, 3))
    y, wt = np.array([1.0, 2.0, 0.0]), np.array([1.0, 3.0, 0.0])
    row, pw = score_ref_p(p, y, wt)
    np.testing.assert_allclose(pw[:, 0], 0.5, rtol=1e-15)
    np.testing.assert_allclose(pw[:, 1], [log(0.5), log(3 / 32), 0.0], rtol=1e-14, atol=1e-16)
    want = [2.0, log(0.5) + log(3 / 32), (1 / 4 + 1 / 36) / 2, 1 / 4, log(3.0)]
    np.testing.assert_allclose(row, want, rtol=1e-14)
    assert dict(zip(NAMES, row))["n"] == 2.0


def test_the_sample_route_is_the_same_numbers():
    """logit with x = 1, beta = (-ln 3, ln 3), w = 0 gives p = (1/4, 3/4): the rows above from samples,
    kriging draws and covariates; `first` picks the states."""
    l3 = log(3.0)
    samples = np.array([[9.0, 1.0, 6.0], [-l3, 1.0, 6.0], [l3, 1.0, 6.0]])
    y, wt = np.array([1.0, 2.0, 0.0]), np.array([1.0, 3.0, 0.0])
    row, pw = score_ref(samples, np.zeros((3, 2)), np.ones((3, 1)), y, wt, 1, "logit", first=2)
    ref, rpw = score_ref_p(np.tile(np.array([[0.25], [0.75]]), (1, 3)), y, wt)
    np.testing.assert_allclose(row, ref, rtol=1e-14)
    np.testing.assert_allclose(pw, rpw, rtol=1e-14, atol=1e-16)
    # probit at eta = 0: p = 1/2 in both states, lpd_c = ln(1/2) for a binary column
    row, pw = score_ref(np.zeros((2, 3)), np.zeros((1, 2)), np.ones((1, 1)), [1.0], [1.0], 1, "probit")
    np.testing.assert_allclose([pw[0, 0], pw[0, 1], row[2], row[3]], [0.5, log(0.5), 0.25, 0.0], rtol=1e-15)


def test_certain_and_wrong_is_minus_infinity_and_nan_is_nan():
    """p = 1 in every state with y < wt: the outcome had probability 0, lpd = -inf (legitimate).  A NaN
    draw makes its column's pair NaN and lpd, brier and err NaN; n and lconst depend on the data alone."""
    p = np.array([[1.0, 0.3], [1.0, 0.6]])
    y, wt = np.array([0.0, 1.0]), np.array([1.0, 1.0])
    row, pw = score_ref_p(p, y, wt)
    assert pw[0, 1] == -np.inf and row[1] == -np.inf and pw[0, 0] == 1.0
    np.testing.assert_allclose(pw[1], [0.45, log(0.45)], rtol=1e-14)
    np.testing.assert_allclose(row[[0, 2, 3]], [2.0, (1.0 + 0.55 ** 2) / 2, 1.0], rtol=1e-14)
    # one state at -inf, one finite: the finite one carries the mean
    row2, pw2 = score_ref_p(np.array([[1.0], [0.5]]), [0.0], [1.0])
    np.testing.assert_allclose(pw2[0, 1], log(0.25), rtol=1e-14)
    p[1, 1] = np.nan
    row, pw = score_ref_p(p, y, wt)
    assert np.isnan(pw[1]).all() and pw[0, 1] == -np.inf
    assert np.isnan(row[1:4]).all() and row[0] == 2.0 and row[4] == 0.0


def test_validation_report_by_hand(mk):
    """pmean (0.1, 0.4, 0.35, 0.8) with y (0, 0, 1, 1): of the four (positive, negative) pairs only
    (0.35, 0.4) is ordered wrongly: AUC 3/4.  Ties count half; columns with weights != 1 stay out of the
    AUC; the reliability table counts every observed column."""
    rep = mk.validation_report([0.1, 0.4, 0.35, 0.8], [0, 0, 1, 1])
    assert rep["auc"] == 0.75
    assert rep["count"].tolist() == [0, 1, 0, 1, 1, 0, 0, 0, 1, 0]
    np.testing.assert_allclose(rep["mean_pmean"][[1, 3, 4, 8]], [0.1, 0.35, 0.4, 0.8])
    np.testing.assert_allclose(rep["mean_observed"][[1, 3, 4, 8]], [0.0, 1.0, 0.0, 1.0])
    assert mk.validation_report([0.5, 0.5], [0, 1])["auc"] == 0.5
    rep = mk.validation_report([0.2, 0.9, 0.7, 0.6], [0, 1, 2, 0], weights=[1, 1, 3, 0], bins=2)
    assert rep["auc"] == 1.0 and rep["count"].tolist() == [1, 2]
    np.testing.assert_allclose(rep["mean_observed"], [0.0, (1.0 + 2 / 3) / 2])
    assert mk.validation_report([0.2, 0.9], [1, 1])["auc"] is None


def test_scores_structs_and_entry_points_match_header(mk):
    binding = __import__(mk.__name__ + "._lib", fromlist=["x"])
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for cname, py, want in (("mk_validation", binding.Validation, ["y_test", "wt_test"]),
                            ("mk_scores", binding.Scores, ["subsets", "pointwise", "combined", "combined_pointwise"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        fields = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*;", body)
        assert fields == [f[0] for f in py._fields_] == want
    assert int(re.search(r"#define MK_N_SCORE (\d+)", src).group(1)) == binding.N_SCORE == len(binding.SCORE_NAMES) == 5
    assert binding.SCORE_NAMES == NAMES
    lib = mk.load()
    nargs = {}
    for name, n in (("mk_session_set_validation", 2), ("mk_session_scores", 2), ("mk_score_grid", 8),
                    ("mk_meta_fit_val", 12), ("mk_meta_fit_ex", 10)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, flags=re.S)
        assert decl, name
        nargs[name] = decl.group(1).count(",") + 1
        assert nargs[name] == n == len(binding.EXPORTS[name][1]), name
        assert hasattr(lib, name)
    ex, val = binding.EXPORTS["mk_meta_fit_ex"][1], binding.EXPORTS["mk_meta_fit_val"][1]
    assert val[:len(ex)] == ex and len(val) == len(ex) + 2      # mk_meta_fit_ex's arguments plus two
    assert mk.session.KS_SCORE == 16


def test_scores_fail_loudly_without_gpu(mk):
    """Null handles are argument errors anywhere; so are bad held-out data in mk_score_grid, before any
    device is touched.  Without a device the session route raises MkError and leaves no session."""
    lib = mk.load()
    binding = __import__(mk.__name__ + "._lib", fromlist=["x"])
    sc, va = binding.Scores(), binding.Validation()
    assert lib.mk_session_scores(None, ctypes.byref(sc)) == binding.MK_E_ARG
    assert lib.mk_session_set_validation(None, ctypes.byref(va)) == binding.MK_E_ARG
    assert lib.mk_score_grid(None, 1, 1, None, None, None, None, 0) == binding.MK_E_ARG
    with pytest.raises(mk.MkError) as e:
        mk.score_grid(np.full((2, 3), 0.5), [0, 1, 2], weights=1)           # y > wt at index 2
    assert e.value.code == binding.MK_E_ARG and "entry 2" in str(e.value)
    with pytest.raises(ValueError):
        mk.score_grid(np.full((2, 3), 0.5), [0, 1])
    if lib.mk_device_count() == 0:
        d = mk.synthetic.generate(20, q=1, n_test=2, seed=1)
        cfg = mk.SamplerConfig(1, 2, [0, 0], [0.1, 0.1], n_batch=1, batch_length=2, burn_in=1)
        sub = dict(coords=d["coords"], y=d["y"], weights=np.ones(20), x=d["x"])
        with pytest.raises(mk.MkError):
            with mk.Session([sub], cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
                ses.set_validation(d["y_test"])
                ses.scores()
        assert lib.mk_session_count() == 0
        with pytest.raises(mk.MkError):
            mk.score_grid(np.full((2, 3), 0.5), [0, 1, 1])
        with pytest.raises(mk.MkError) as e:
            mk.meta_fit_node([sub], cfg, coords_test=d["coords_test"], x_test=d["x_test"], devices=[0],
                             validation=d["y_test"])
        assert e.value.code == binding.MK_E_NODEV
