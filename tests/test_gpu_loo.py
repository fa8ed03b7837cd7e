"""PSIS-LOO on the device (include/mk.h "leave-one-out") against its NumPy restatement tests/loo_ref.py.

The bar is measured, per case.  g is the largest |float64 - longdouble| over the case's finite entries of the
restatement itself: the rounding the definitions carry at 64 bits on those inputs.  A device value v is held
to |v - restatement in long double| <= 16 g + 16 eps64 max(1, |value|): the factor 16 is the margin the
kriging parity test gives LAPACK, and covers device exp / log / log1p an ulp or two from libm and another,
but fixed, summation order.  k-hat = +inf and NaN match exactly, and so does n_k_bad.  Every case prints g
and its largest deviation (DESIGN.md section 7 records a run).

Matrix entry (psis_loo): n = 25 (M = 5, the minimum), 26, 48 (M = 9), 100 (M = 20 = floor(n/5)), 1,251 (M = 107
= ceil(3 sqrt n)), 2,048 and 2,049 (both sides of a power of two: the padded sort), 8,192 (the cap); 5
observations, at n = 100 1 and 257 (an upload chunk and a reduction stride crossed).  Row types: Bernoulli-logit
terms with eta ~ N(0.3, 1); eta ~ N(0.3, 3) (heavy: k-hat above 0.7 and above 1 occur); constant rows; a
constant tail under a varying body; two-valued rows whose ties straddle the cut; a row with one NaN.

Sessions: the criteria tests' two shapes (exponential, logit, q = 1, subsets of 100 and 257 sites with 3 trials;
Matern, probit, q = 2, subsets of 129 and 150 sites), 64 iterations, burn_in 1 so that every window is open."""
import numpy as np
import pytest

from crit_ref import lconst, loglik
from loo_ref import NAMES, loo_ref, loo_total, tail_length

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
KS_LOO = 20
TYPES = ["bern", "heavy", "const", "consttail", "twoval", "nan"]
SHAPES = [(25, 5), (26, 5), (48, 5), (100, 1), (100, 257), (1251, 5), (2048, 5), (2049, 5), (8192, 5)]
_CASES = {"exp": dict(sizes=[100, 257], q=1, cov="exponential", link="logit", trials=3.0),
          "mat": dict(sizes=[129, 150], q=2, cov="matern", link="probit", trials=1.0)}
_refs, _runs = {}, {}


def _matrix(kind, n, N):
    """The n x N matrix of terms of one row type (a function of kind, n and N alone)."""
    rng = np.random.default_rng(1000 * n + N)
    y = (np.arange(N) % 2).astype(float)
    eta = rng.normal(0.3, 3.0 if kind == "heavy" else 1.0, (n, N))
    ell = y[None, :] * eta - np.logaddexp(0.0, eta)
    M = tail_length(n)
    if kind == "const":
        ell = np.repeat((-0.3 - 0.1 * np.arange(N))[None, :], n, axis=0)
    elif kind == "consttail":
        for i in range(N):                               # the M + 2 smallest terms equal, below every other
            col = np.sort(ell[:, i])
            col[:M + 2] = col[0] - 0.5
            ell[:, i] = rng.permutation(col)
    elif kind == "twoval":
        # M - nb terms at a, the rest at b > a: nb of the ties at b are in the tail (exceedance 0), the others
        # below the cut.  Even columns: nb = 1..3, x* is an a and the fit is defined.  Odd columns: the ties reach
        # x*, so x* = 0 and k-hat is NaN in every precision.  At G = 40 (M = 100..120: n = 1,251) the grid point
        # g = 3 has sqrt(G / (g - 1/2)) = 4, and with every non-zero exceedance equal its theta is 1/x - 3/(3x):
        # zero, hence NaN, or not, by the last bit of exp.  No reference can pin that, so there every column
        # takes the odd columns' form.
        jstar = int(np.floor(M / 4 + 0.5)) - 1
        G = 30 + int(np.floor(np.sqrt(M)))
        for i in range(N):
            nb = 1 + i % 3 if (i % 2 == 0 and G != 40) else min(jstar + 1 + i % 3, M - 1)
            col = np.full(n, -0.4 - 0.01 * i)
            col[:M - nb] = -2.0 - 0.1 * i
            ell[:, i] = rng.permutation(col)
    elif kind == "nan":
        ell[n // 2, min(2, N - 1)] = np.nan
    return np.ascontiguousarray(ell)


def _ref(ell, key, lc=0.0):
    """The restatement in float64 and in long double, computed once per case and left unchanged."""
    if key not in _refs:
        _refs[key] = (loo_ref(ell, lc, np.float64), loo_ref(ell, lc, np.longdouble))
    return _refs[key]


def _judge(tag, dev, r64, r80):
    """dev against the long-double restatement r80 under the measured bar; non-finite entries match exactly."""
    dev, r64 = np.asarray(dev, float), np.asarray(r64, float)
    fin = np.isfinite(r80)
    assert np.array_equal(fin, np.isfinite(r64)), tag + ": the case is not well posed"
    assert np.array_equal(np.isnan(dev), np.isnan(r64)), tag
    assert np.array_equal(dev[~fin & ~np.isnan(dev)], r64[~fin & ~np.isnan(dev)]), tag      # the infinities
    if not fin.any():
        print(f"LOO {tag}: no finite entry")
        return
    g = float(np.abs(r64[fin] - r80[fin]).max())
    bar = 16.0 * g + 16.0 * EPS * np.maximum(1.0, np.abs(r80[fin].astype(float)))
    d = np.abs(dev[fin] - r80[fin]).astype(float)
    w = int(np.argmax(d / bar))
    print(f"LOO {tag}: g {g:.2e}  largest deviation {d.max():.2e}  worst deviation / bar {d[w] / bar[w]:.2f} "
          f"(device {dev[fin][w]:.17g}, restatement {float(r80[fin][w]):.17g})")
    assert (d <= bar).all(), tag


def _check(tag, rows, pw, ref):
    (rows64, pw64), (rows80, pw80) = ref
    assert pw.shape == pw64.shape and rows.shape == (8,)
    _judge(tag + " pointwise", pw, pw64, pw80)
    _judge(tag + " rows", rows, rows64, rows80)
    if not np.isnan(rows80[6]):
        assert rows[6] == float(rows80[6])
    assert rows[7] == float(rows80[7]) or abs(rows[7] - float(rows80[7])) <= 1e-9 * abs(float(rows80[7]))


# ---------------------------------------------------------------- the matrix entry
@pytest.mark.parametrize("kind", TYPES)
@pytest.mark.parametrize("n,N", SHAPES)
def test_matrix_against_restatement(mk, n, N, kind):
    ell = _matrix(kind, n, N)
    got = mk.psis_loo(ell)
    assert list(got)[:8] == NAMES
    rows = np.array([got[k] for k in NAMES])
    ref = _ref(ell, (kind, n, N))
    _check(f"matrix {kind} n={n} N={N}", rows, got["pointwise"], ref)
    kh = got["pointwise"][:, 1]
    if kind in ("const", "consttail"):
        assert (kh == np.inf).all() and rows[5] == np.inf and rows[6] == N
    if kind == "nan":
        assert np.isnan(got["pointwise"][min(2, N - 1)]).all() and np.isnan(rows[:7]).all() and rows[7] == 0.0
    if kind == "heavy" and N == 257:
        assert (kh > 1.0).any() and ((kh > 0.7) & (kh <= 1.0)).any() and (kh < 0.7).any()


@pytest.mark.parametrize("n", [24, 8193])
def test_matrix_state_limits(mk, n):
    with pytest.raises(mk.MkError) as e:
        mk.psis_loo(np.zeros((n, 3)))
    assert e.value.code == mk._lib.MK_E_ARG and str(n) in str(e.value)
    if n > 8192:
        assert "thin" in str(e.value)


@pytest.mark.parametrize("n,N", [(48, 5), (100, 257), (2049, 5)])
def test_matrix_same_bytes(mk, monkeypatch, n, N):
    """Two calls, and one column per upload against the default chunk: the same bytes."""
    ell = _matrix("heavy", n, N)
    a, b = mk.psis_loo(ell), mk.psis_loo(ell)
    monkeypatch.setenv("MK_LOO_CHUNK", "1")
    c = mk.psis_loo(ell)
    for other in (b, c):
        assert other["pointwise"].tobytes() == a["pointwise"].tobytes()
        assert [other[k] for k in NAMES] == [a[k] for k in NAMES]


# ---------------------------------------------------------------- sessions
def _problem(mk, sizes, q, trials, cov):
    off = np.concatenate([[0], np.cumsum(sizes)])
    d = mk.synthetic.generate(int(off[-1]), q=q, n_test=8, cov_model=1 if cov == "matern" else 0, seed=9 + q)
    subs = []
    for s, m in enumerate(sizes):
        rows = slice(off[s] * q, (off[s] + m) * q)
        subs.append(dict(coords=d["coords"][off[s]:off[s] + m], y=d["y"][rows], weights=np.full(m * q, trials),
                         x=d["x"][rows]))
    return subs


def _cfg(mk, c):
    p = 2 * c["q"]
    return mk.SamplerConfig(c["q"], p, beta_starting=np.zeros(p), beta_tuning=np.full(p, 0.05), cov_model=c["cov"],
                            link=c["link"], n_batch=4, batch_length=16, burn_in=1, seed=9)


def _run(mk, name, tmp_path_factory):
    """One fit per case with the chain recorded; every call the tests read made once, in a fixed order."""
    if name in _runs:
        return _runs[name]
    import os
    c = _CASES[name]
    subs, cfg = _problem(mk, c["sizes"], c["q"], c["trials"], c["cov"]), _cfg(mk, c)
    r = dict(subs=subs, cfg=cfg, q=c["q"], link=c["link"])
    path = str(tmp_path_factory.mktemp("loo") / f"{name}.npz")
    with mk.Session(subs, cfg, record_w=True) as ses:
        ses.run(64)
        r["before"] = ses.kernel_stats(KS_LOO)
        r["out"] = ses.outputs(quantiles=False, samples=True, w_samples=True)
        ses.set_kept_window(17, 64)
        r["w17"] = ses.loo(pointwise=True)
        r["after"] = ses.kernel_stats(KS_LOO)
        r["w17_again"] = ses.loo(pointwise=True)
        r["crit17"] = ses.criteria()
        os.environ["MK_LOO_CHUNK"] = "1"
        try:
            r["w17_chunk1"] = ses.loo(pointwise=True)
        finally:
            del os.environ["MK_LOO_CHUNK"]
        r["plain"] = ses.loo()
        ses.set_kept_window(1, 64)
        r["thin2"] = ses.loo(thin=2, pointwise=True)
        ses.set_kept_window(40, 60)
        with pytest.raises(mk.MkError) as e:
            ses.loo()
        r["short"] = e.value
        mk.fitfile.save_session(ses, path)
    with mk.fitfile.load_session(path, predict_tile=64) as back:
        assert back.imported
        back.set_kept_window(17, 64)
        r["loaded"] = back.loo(pointwise=True)
    a = mk.fitfile.read(path)
    samples, ws, acc = mk.fitfile.chain_of(a)
    with mk.Session(subs, mk.fitfile.config_from(a, predict_tile=64), record_w=True) as ses:
        ses.import_chain(samples, ws, acc)
        ses.set_kept_window(1, 64)
        r["imported"] = ses.loo(thin=2, pointwise=True)
    _runs[name] = r
    return r


def _session_check(tag, got, r, window, thin):
    n_sub = len(r["subs"])
    assert got["names"] == NAMES and got["subsets"].shape == (n_sub, 8) and got["total"].shape == (8,)
    p = 2 * r["q"]
    idx = np.arange(window[0] - 1, window[1], thin)
    for s in range(n_sub):
        sub = r["subs"][s]
        y, wt, X = np.asarray(sub["y"], float), np.asarray(sub["weights"], float), np.asarray(sub["x"], float)
        beta = r["out"]["samples"][s][idx, :p]
        w = r["out"]["w_samples"][s][:, idx]
        ell = loglik(y[:, None], wt[:, None], X @ beta.T + w, r["link"]).T         # n x N
        ref = _ref(ell, (tag, s), lconst(y, wt))
        _check(f"session {tag} subset {s}", got["subsets"][s], got["pointwise"][s], ref)
    tot = loo_total(got["subsets"])
    for k in (0, 1, 2, 4, 6, 7):
        t = got["subsets"][0, k]
        for s in range(1, n_sub):
            t = t + got["subsets"][s, k]
        assert got["total"][k] == t, NAMES[k]                                      # the subset-order sum
    assert got["total"][5] == tot[5]
    np.testing.assert_allclose(got["total"][3], tot[3], rtol=4 * EPS)


def _same(a, b):
    assert a["subsets"].tobytes() == b["subsets"].tobytes() and a["total"].tobytes() == b["total"].tobytes()
    if "pointwise" in a and "pointwise" in b:
        for x, y in zip(a["pointwise"], b["pointwise"]):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", list(_CASES))
def test_session_against_restatement(mk, name, tmp_path_factory):
    """Window 17..64 (n = 48, M = 9) and 1..64 with thin 2 (n = 32, M = 6), on the chain the session returns."""
    r = _run(mk, name, tmp_path_factory)
    _session_check(name + " 17..64", r["w17"], r, (17, 64), 1)
    _session_check(name + " 1..64 thin 2", r["thin2"], r, (1, 64), 2)
    if name == "exp":
        assert (r["w17"]["subsets"][:, 7] > 0).all()           # three trials: the dropped constant is there
    assert [a.shape for a in r["w17"]["pointwise"]] == [(m * r["q"], 3) for m in _CASES[name]["sizes"]]


@pytest.mark.parametrize("name", list(_CASES))
def test_session_lppd_is_the_criteria_s(mk, name, tmp_path_factory):
    r = _run(mk, name, tmp_path_factory)
    np.testing.assert_allclose(r["w17"]["subsets"][:, 4], r["crit17"]["subsets"][:, 4], rtol=1e-9, atol=0)
    np.testing.assert_allclose(r["w17"]["subsets"][:, 7], r["crit17"]["subsets"][:, 7], rtol=1e-9, atol=0)


@pytest.mark.parametrize("name", list(_CASES))
def test_session_same_bytes(mk, name, tmp_path_factory):
    """Two calls, one subset per chunk, without the pointwise output, a loaded fit file and an imported chain."""
    r = _run(mk, name, tmp_path_factory)
    _same(r["w17"], r["w17_again"])
    _same(r["w17"], r["w17_chunk1"])
    _same(r["w17"], r["plain"])
    _same(r["w17"], r["loaded"])
    _same(r["thin2"], r["imported"])


@pytest.mark.parametrize("name", list(_CASES))
def test_session_window_too_short_and_launch_count(mk, name, tmp_path_factory):
    r = _run(mk, name, tmp_path_factory)
    assert mk.session.KS_LOO == KS_LOO
    assert r["before"] == dict(launches=0, ms=0.0, flops=0.0)
    assert r["after"]["launches"] == 4 and r["after"]["ms"] > 0.0       # terms, psis, finish, total: one chunk
    e = r["short"]
    assert e.code == mk._lib.MK_E_ARG and "21" in str(e)                # 40..60: n = 21 < 25


def test_session_without_record_w(mk):
    c = _CASES["exp"]
    subs = _problem(mk, c["sizes"], c["q"], c["trials"], c["cov"])
    with mk.Session(subs[:1], _cfg(mk, c)) as ses:
        ses.run(16)
        with pytest.raises(mk.MkError) as e:
            ses.loo()                                        # the chain has not finished
        assert e.value.code == mk._lib.MK_E_ARG
        ses.run(48)
        with pytest.raises(mk.MkError) as e:
            ses.loo()
        assert e.value.code == mk._lib.MK_E_ARG and "record_w" in str(e.value)
        assert ses.kernel_stats(KS_LOO)["launches"] == 0


def test_run_metakriging_loo_line():
    """run_metakriging.py --loo prints one more JSON line, {"loo": the total row by name}."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "run_metakriging.py"), "--config", "1", "--n", "600", "--subsets", "3",
           "--n-test", "16", "--n-batch", "4", "--batch-length", "25", "--loo"]       # 26 kept states
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=100, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    loo = [l["loo"] for l in lines if "loo" in l]
    assert len(loo) == 1 and list(loo[0]) == NAMES
    row = np.array([loo[0][k] for k in NAMES])
    assert np.isfinite(row[:5]).all() and row[1] > 0 and row[2] == -2 * row[0] and row[7] == 0.0


def test_sploo_and_loo_compare(mk, tmp_path):
    """spLoo of a live fit, of the same fit loaded from its file, and Session.loo: the same bytes.  loo_compare of
    two windows of one fit is the three-line restatement on their pointwise values."""
    n = 80
    d = mk.synthetic.generate(n, q=1, n_test=8, seed=31)
    starting = {"beta": np.zeros(2), "phi": 3 / 0.5, "A": np.ones(1), "w": 0.0}
    tuning = {"beta": np.full(2, 0.05), "phi": 1.0, "A": 0.1, "w": 0.5}
    priors = {"phi.Unif": (3 / 0.75, 3 / 0.25), "K.IW": (1, 0.1 * np.eye(1))}
    amcmc = {"n.batch": 4, "batch.length": 16, "accept.rate": 0.43}
    path = str(tmp_path / "fit.npz")
    with mk.spMvGLM([(d["y"], d["x"])], d["coords"], np.ones((n, 1)), starting, tuning, priors, amcmc, seed=9) as fit:
        live = mk.spLoo(fit, start=17, end=64)
        early = mk.spLoo(fit, start=1, end=48)
        ses = fit["_session"].loo(pointwise=True)            # the window spLoo left: 1..48
        for bad in (dict(start=0), dict(start=10, end=9), dict(end=65), dict(thin=0)):
            with pytest.raises(ValueError):
                mk.spLoo(fit, **bad)
        with pytest.raises(mk.MkError):
            mk.spLoo(fit, start=50, end=64)                  # 15 states
        fit.save(path)
    with pytest.raises(ValueError):
        mk.spLoo(fit)                                        # closed
    assert list(live)[:8] == NAMES and live["pointwise"].shape == (n, 3)
    assert np.array([early[k] for k in NAMES]).tobytes() == ses["subsets"][0].tobytes()
    assert early["pointwise"].tobytes() == ses["pointwise"][0].tobytes()
    with mk.load_fit(path) as back:
        loaded = mk.spLoo(back, start=17, end=64)
        again = back["_session"].loo(pointwise=True)
    assert [loaded[k] for k in NAMES] == [live[k] for k in NAMES] == again["subsets"][0].tolist()
    assert loaded["pointwise"].tobytes() == live["pointwise"].tobytes() == again["pointwise"][0].tobytes()
    ell = loglik(d["y"][:, None], 1.0, d["x"] @ fit["p.beta.theta.samples"][16:64, :2].T + fit["p.w.samples"][:, 16:64],
                 "logit").T
    _check("spLoo 17..64", np.array([live[k] for k in NAMES]), live["pointwise"], _ref(ell, "sploo"))
    cmp_ = mk.loo_compare(live, early)
    dif = live["pointwise"][:, 0] - early["pointwise"][:, 0]
    np.testing.assert_allclose(cmp_["elpd_diff"], dif.sum(), rtol=1e-12)
    np.testing.assert_allclose(cmp_["se_diff"], np.sqrt(n * dif.var(ddof=1)), rtol=1e-12)
    assert cmp_["n_k_bad"] == int(np.sum((live["pointwise"][:, 1] > 0.7) | (early["pointwise"][:, 1] > 0.7)))
