"""CPU side of the model-assessment rows (include/mk.h: DIC and WAIC per subset): tests/crit_ref.py,
the restatement the GPU tests compare the device with, is pinned here against cases worked by hand,
and the binding is checked against the header."""
import ctypes
import os
import re
from math import log, sqrt

import numpy as np
import pytest

from crit_ref import NAMES, crit_ref, lconst, loglik

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mk.h")


def test_chain_that_never_moves():
    """Every state the same: the deviance has no spread (pD = 0), the pointwise variance is 0 (p.waic =
    0), log mean exp of equal terms is the term, so WAIC = DIC = bar.D = D at that state."""
    rng = np.random.default_rng(3)
    N, p, n = 7, 2, 5
    X, y, wt = rng.normal(size=(N, p)), rng.integers(0, 3, N).astype(float), np.full(N, 2.0)
    beta, w = rng.normal(size=p), rng.normal(size=N)
    samples = np.tile(np.concatenate([beta, [1.0, 6.0]]), (n, 1))
    w_samples = np.tile(w[:, None], (1, n))
    for link in ("logit", "probit"):
        rows, pw = crit_ref(samples, w_samples, y, wt, X, p, link, (1, n))
        D = -2.0 * loglik(y, wt, X @ beta + w, link).sum()
        r = dict(zip(NAMES, rows))
        assert abs(r["pD"]) <= 1e-12 * abs(D) and r["p.waic"] <= 1e-24
        for k in ("bar.D", "D.bar.Omega", "DIC", "WAIC"):
            np.testing.assert_allclose(r[k], D, rtol=1e-12)
        np.testing.assert_allclose(pw[:, 0], loglik(y, wt, X @ beta + w, link), rtol=1e-12)


def test_two_states_three_observations_by_hand():
    """logit, p = 1, x = (1, 1, 0), beta = (0, ln 3), w_3 = (0, -ln 3), (y, wt) = (1, 1), (0, 1), (2, 3).
    eta: obs 1, 2: (0, ln 3); obs 3: (0, -ln 3).  l = y eta - wt ln(1 + e^eta):
      obs 1: (-ln 2, ln 3 - ln 4)            obs 2: (-ln 2, -ln 4)
      obs 3: (-3 ln 2, -2 ln 3 - 3 ln(4/3)) = (ln(1/8), ln(3/64))
    D_1 = 10 ln 2, D_2 = -2 ln((3/4)(1/4)(3/64)) = 2 ln(1024/9); bar.D = ln(32768/9).
    Means: beta = ln sqrt 3, w_3 = -ln sqrt 3, so eta = (ln sqrt 3, ln sqrt 3, -ln sqrt 3).
    mean_k exp(l): (1/2 + 3/4)/2 = 5/8, (1/2 + 1/4)/2 = 3/8, (1/8 + 3/64)/2 = 11/128.
    Two states: M2/(n - 1) = (l_1 - l_2)^2 / 2 with differences ln(2/3), ln 2, ln(8/3).
    lconst = ln C(3, 2) = ln 3."""
    l3, r3 = log(3.0), sqrt(3.0)
    samples = np.array([[0.0, 1.0, 6.0], [l3, 1.0, 6.0]])
    w_samples = np.array([[0.0, 0.0], [0.0, 0.0], [0.0, -l3]])
    y, wt, X = np.array([1.0, 0.0, 2.0]), np.array([1.0, 1.0, 3.0]), np.array([[1.0], [1.0], [0.0]])
    rows, pw = crit_ref(samples, w_samples, y, wt, X, 1, "logit", (1, 2))
    bar_d = log(32768.0 / 9.0)
    d_hat = -2.0 * ((log(r3) - log(1 + r3)) + (-log(1 + r3)) + (-l3 - 3 * log(1 + 1 / r3)))
    lppd = log(5 / 8) + log(3 / 8) + log(11 / 128)
    p_waic = (log(2 / 3) ** 2 + log(2.0) ** 2 + log(8 / 3) ** 2) / 2
    want = [bar_d, d_hat, bar_d - d_hat, 2 * bar_d - d_hat, lppd, p_waic, -2 * (lppd - p_waic), l3]
    np.testing.assert_allclose(rows, want, rtol=1e-13)
    np.testing.assert_allclose(pw[:, 0], [log(5 / 8), log(3 / 8), log(11 / 128)], rtol=1e-13)
    np.testing.assert_allclose(pw[:, 1], [log(2 / 3) ** 2 / 2, log(2.0) ** 2 / 2, log(8 / 3) ** 2 / 2], rtol=1e-13)
    # a window and a thin pick states: rows 1 and 3 of three are the two states above
    s3 = np.vstack([samples[:1], [[7.0, 1.0, 6.0]], samples[1:]])
    w3 = np.insert(w_samples, 1, 5.0, axis=1)
    np.testing.assert_array_equal(crit_ref(s3, w3, y, wt, X, 1, "logit", (1, 3), thin=2)[0], rows)
    with pytest.raises(ValueError):
        crit_ref(s3, w3, y, wt, X, 1, "logit", (2, 2))


def test_probit_tails_stay_finite():
    """|eta| = 30: Phi(-30) ~ 5e-198 has a finite log (~ -454.3); a naive log(1 - Phi(30)) would be -inf."""
    y, wt = np.array([0.0, 1.0, 1.0, 0.0]), np.ones(4)
    ell = loglik(y, wt, np.array([30.0, 30.0, -30.0, -30.0]), "probit")
    assert np.isfinite(ell).all()
    np.testing.assert_allclose(ell[[0, 2]], -454.3212439955, rtol=1e-9)      # log Phi(-30)
    assert abs(ell[1]) < 1e-190 and abs(ell[3]) < 1e-190
    X = np.array([[30.0], [30.0], [-30.0], [-30.0]])
    samples = np.array([[1.0, 1.0, 6.0], [1.0, 1.0, 6.0], [0.99, 1.0, 6.0]])
    rows, _ = crit_ref(samples, np.zeros((4, 3)), y, wt, X, 1, "probit", (1, 3))
    assert np.isfinite(rows).all()


def test_lconst_three_trials():
    """wt = 3: log C(3, y) = 0, ln 3, ln 3, 0; binary data (wt = 1) have none."""
    for yv, want in zip((0.0, 1.0, 2.0, 3.0), (0.0, log(3.0), log(3.0), 0.0)):
        assert abs(lconst(np.array([yv]), np.array([3.0])) - want) < 1e-14
    assert abs(lconst(np.array([0.0, 1.0, 2.0, 3.0]), np.full(4, 3.0)) - 2 * log(3.0)) < 1e-14
    assert lconst(np.array([0.0, 1.0, 1.0]), np.ones(3)) == 0.0


def test_criteria_struct_and_entry_points_match_header(mk):
    binding = __import__(mk.__name__ + "._lib", fromlist=["x"])
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct mk_criteria \{(.*?)\} mk_criteria;", src, flags=re.S).group(1)
    fields = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*;", body)
    assert fields == [f[0] for f in binding.Criteria._fields_] == ["subsets", "total", "pointwise"]
    assert int(re.search(r"#define MK_N_CRIT (\d+)", src).group(1)) == binding.N_CRIT == len(binding.CRIT_NAMES) == 8
    assert binding.CRIT_NAMES == NAMES
    lib = mk.load()
    for name, nargs in (("mk_session_set_criteria", 2), ("mk_session_criteria", 3), ("mk_meta_fit_ex", 10)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, flags=re.S)
        assert decl, name
        assert decl.group(1).count(",") + 1 == nargs == len(binding.EXPORTS[name][1]), name
        assert hasattr(lib, name)


def test_criteria_fail_loudly_without_gpu(mk):
    """No CPU fallback: without a device the session (and with it Session.criteria) and the node call
    raise MkError; null handles are argument errors anywhere."""
    lib = mk.load()
    binding = __import__(mk.__name__ + "._lib", fromlist=["x"])
    cb = binding.Criteria()
    assert lib.mk_session_criteria(None, 1, ctypes.byref(cb)) == binding.MK_E_ARG
    assert lib.mk_session_set_criteria(None, 1) == binding.MK_E_ARG
    if lib.mk_device_count() == 0:
        d = mk.synthetic.generate(20, q=1, n_test=2, seed=1)
        cfg = mk.SamplerConfig(1, 2, [0, 0], [0.1, 0.1], n_batch=1, batch_length=2, burn_in=1)
        sub = dict(coords=d["coords"], y=d["y"], weights=np.ones(20), x=d["x"])
        with pytest.raises(mk.MkError):
            with mk.Session([sub], cfg, record_w=True, criteria=True) as ses:
                ses.criteria()
        assert lib.mk_session_count() == 0
        with pytest.raises(mk.MkError) as e:
            mk.meta_fit_node([sub], cfg, devices=[0], criteria=True)
        assert e.value.code == binding.MK_E_NODEV
