"""Predictive probabilities at held-out sites: spPredict's p.y.predictive.samples for the binomial
family, p = linkinv(x(s)' beta + w(s)) evaluated jointly on every kept MCMC state, their 200-level
grids per subset (p.predict) and the combined grid (result3).

The oracle needs no change: p is a deterministic function of its `samples` and `w_pred`.  Bars:
1e-8 against the oracle (the project's replay bar, which the draws and beta already meet); bit
equality between the transform-on-load quantile kernel and the elementwise kernel, between the
fused and the tiled route, and between the node driver and one session; 1e-14 between the device's
p draws and the NumPy formula on the device's own beta and w draws (p <= 1 and |dp/deta| <= 1/4,
so the slack covers the roundings of eta and exp only).

Shapes: n_batch = 3, batch_length = 4, burn_in = 7 keeps 6 states, which the sort pads to 8;
24 test sites; subsets of 150 / 163 sites (two 128-tiles with the bordered row) and 64 / 71."""
import ctypes
import math

import numpy as np
import pytest

from oracle import spmvglm as om
from oracle.rstats import PROBS200, r_quantile7

pytestmark = pytest.mark.gpu
TOL = 1e-8
N_TEST = 24
KW = dict(n_batch=3, batch_length=4, burn_in=7, seed=9)
_erfc = np.vectorize(math.erfc)


def _linkinv(eta, link):
    if link == "probit":
        return 0.5 * _erfc(-eta * math.sqrt(0.5))
    return 1.0 / (1.0 + np.exp(-eta))


def _problem(mk, sizes, q, link="logit", seed=9):
    off = np.concatenate([[0], np.cumsum(sizes)])
    d = mk.synthetic.generate(int(off[-1]), q=q, n_test=N_TEST, seed=seed + q, link=link)
    subs = []
    for s, m in enumerate(sizes):
        rows = slice(off[s] * q, (off[s] + m) * q)
        subs.append(dict(coords=d["coords"][off[s]:off[s] + m], y=d["y"][rows], weights=np.ones(m * q), x=d["x"][rows]))
    return d, subs


def _cfg(mk, q, link="logit", predict_tile=0, **over):
    p = 2 * q
    kw = dict(KW, **over)
    return mk.SamplerConfig(q, p, beta_starting=np.zeros(p), beta_tuning=np.full(p, 0.05), link=link,
                            predict_tile=predict_tile, **kw)


def _device(mk, subs, cfg, ct, x_test, **outs):
    with mk.Session(subs, cfg, coords_test=ct, x_test=x_test) as ses:
        ses.run(cfg.n_samples)
        return ses.outputs(**outs)


_CASES = {"q1": ([150, 163], 1, "logit"), "q2": ([64, 71], 2, "logit"), "probit": ([150, 163], 1, "probit")}
_runs = {}


def _run(mk, name):
    """One device fit with x_test and one oracle fit per case, shared by the tests that read them."""
    if name not in _runs:
        sizes, q, link = _CASES[name]
        d, subs = _problem(mk, sizes, q, link)
        cfg = _cfg(mk, q, link)
        dev = _device(mk, subs, cfg, d["coords_test"], d["x_test"], samples=True, w_pred_samples=True,
                      p_pred_samples=True, p_predict_sum=True)
        p = 2 * q
        ocfg = om.Config(q, p, beta_starting=np.zeros(p), beta_tuning=np.full(p, 0.05), cov_model=0,
                         link=om.LINK_PROBIT if link == "probit" else om.LINK_LOGIT, **KW)
        refs = [om.fit_subset(sb["coords"], sb["y"], sb["weights"], sb["x"], ocfg, subset=s, coords_test=d["coords_test"])
                for s, sb in enumerate(subs)]
        _runs[name] = dict(d=d, subs=subs, cfg=cfg, dev=dev, refs=refs, q=q, link=link)
    return _runs[name]


def _check_against_oracle(dev, refs, x_test, p, link, burn_in=KW["burn_in"]):
    for s, ref in enumerate(refs):
        p_ref = _linkinv(ref["samples"][burn_in - 1:, :p] @ x_test.T + ref["w_pred"], link)   # kept x C
        print(f"subset {s}: p_ref in [{p_ref.min():.3f}, {p_ref.max():.3f}], "
              f"draws {np.abs(dev['p_pred_samples'][s].T - p_ref).max():.2e}, "
              f"grids {np.abs(dev['p_predict'][s] - r_quantile7(p_ref, PROBS200)).max():.2e}")
        np.testing.assert_allclose(dev["p_pred_samples"][s].T, p_ref, rtol=0, atol=TOL)
        np.testing.assert_allclose(dev["p_predict"][s], r_quantile7(p_ref, PROBS200), rtol=0, atol=TOL)


@pytest.mark.parametrize("name", list(_CASES))
def test_oracle_replay_fused(mk, name):
    """The device's p draws and p.predict grids against the oracle's own chain, and the session's
    other outputs untouched by the covariates."""
    r = _run(mk, name)
    dev, q = r["dev"], r["q"]
    assert dev["p_predict"][0].shape == (200, q * N_TEST) and dev["p_pred_samples"][0].shape == (q * N_TEST, 6)
    _check_against_oracle(dev, r["refs"], r["d"]["x_test"], 2 * q, r["link"])
    plain = _device(mk, r["subs"], r["cfg"], r["d"]["coords_test"], None)
    assert "p_predict" not in plain
    for s in range(len(r["subs"])):
        assert np.array_equal(dev["w_predict"][s], plain["w_predict"][s])
        assert np.array_equal(dev["parameters"][s], plain["parameters"][s])


@pytest.mark.parametrize("name", list(_CASES))
def test_grids_and_draws_are_self_consistent(mk, name):
    """The transform-on-load quantile kernel and the elementwise kernel compute the same p (bit for
    bit: the grids are the type-7 quantiles of the p draws), the draws are the formula on the
    session's own beta and w draws, and p_predict_sum is the sequential sum of the grids."""
    r = _run(mk, name)
    dev, p = r["dev"], 2 * r["q"]
    x_test = r["d"]["x_test"]
    acc = None
    for s in range(len(r["subs"])):
        pd = dev["p_pred_samples"][s].T                                        # kept x C
        assert np.array_equal(dev["p_predict"][s], r_quantile7(pd, PROBS200))
        beta = dev["samples"][s][KW["burn_in"] - 1:, :p]
        formula = _linkinv(beta @ x_test.T + dev["w_pred_samples"][s].T, r["link"])
        print(f"subset {s}: formula difference {np.abs(pd - formula).max():.2e}")
        np.testing.assert_allclose(pd, formula, rtol=0, atol=1e-14)
        assert pd.min() > 0.0 and pd.max() < 1.0
        acc = dev["p_predict"][s].copy() if acc is None else acc + dev["p_predict"][s]
    assert np.array_equal(dev["p_predict_sum"], acc)


def test_dense_covariates(mk):
    """q = 2 with a dense x_test (every outcome's row loads every coefficient), not the generator's
    block-diagonal one: the column stride of x_test and the order of the products."""
    r = _run(mk, "q2")
    x_test = np.random.default_rng(5).standard_normal((2 * N_TEST, 4))
    dev = _device(mk, r["subs"], r["cfg"], r["d"]["coords_test"], x_test, p_pred_samples=True)
    _check_against_oracle(dev, r["refs"], x_test, 4, "logit")
    for s in range(2):
        assert np.array_equal(dev["p_predict"][s], r_quantile7(dev["p_pred_samples"][s].T, PROBS200))
        assert np.array_equal(dev["w_predict"][s], r["dev"]["w_predict"][s])


def test_one_kept_state(mk):
    """burn_in = n.samples keeps one state: the sort holds one value and every level equals it."""
    d, subs = _problem(mk, [60, 50], 1)
    cfg = _cfg(mk, 1, burn_in=12)
    dev = _device(mk, subs, cfg, d["coords_test"], d["x_test"], p_pred_samples=True)
    for s in range(2):
        assert dev["p_pred_samples"][s].shape == (N_TEST, 1)
        assert np.array_equal(dev["p_predict"][s], np.repeat(dev["p_pred_samples"][s].T, 200, axis=0))


def test_tiled_equals_fused(mk, monkeypatch):
    """Tiles of 7, 7, 7 and 3 sites (q = 2: 14 / 6 columns; a tile's x_test rows start at t0 * q):
    grids, draws and their sum equal the fused session's bit for bit, and one tile's replay gives
    its columns of both grids."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    r = _run(mk, "q2")
    fused = r["dev"]
    ct, xt = r["d"]["coords_test"], r["d"]["x_test"]
    cfg = _cfg(mk, 2, predict_tile=7)
    with mk.Session(r["subs"], cfg, coords_test=ct, x_test=xt) as ses:
        ses.run(cfg.n_samples)
        assert ses.predict_tile == 7
        tiled = ses.outputs(w_pred_samples=True, p_pred_samples=True, p_predict_sum=True)
        gw, gp = ses.tile_grids(14, prob=True)
        only_w = ses.tile_grids(14)
    for s in range(2):
        for k in ("p_predict", "p_pred_samples", "w_predict", "w_pred_samples"):
            assert np.array_equal(tiled[k][s], fused[k][s]), (k, s)
        assert np.array_equal(gp[s], fused["p_predict"][s][:, 28:42])
        assert np.array_equal(gw[s], fused["w_predict"][s][:, 28:42])
    assert np.array_equal(only_w, gw)
    assert np.array_equal(tiled["p_predict_sum"], fused["p_predict_sum"])


def test_sppredict_window_and_thinning(mk):
    """spPredict(fit, coords, pred_covars, start = 5, end = 11, thin = 2): p.y.predictive.samples is
    the formula on the fit's own beta of iterations 5, 7, 9, 11 and the returned w draws; new sites
    without covariates return no p.y (the earlier covariates are dropped with the earlier sites)."""
    n = 80
    d = mk.synthetic.generate(n, q=1, n_test=N_TEST, seed=31)
    starting = {"beta": np.zeros(2), "phi": 3 / 0.5, "A": np.ones(1), "w": 0.0}
    tuning = {"beta": np.full(2, 0.05), "phi": 1.0, "A": 0.1, "w": 0.5}
    priors = {"phi.Unif": (3 / 0.75, 3 / 0.25), "K.IW": (1, 0.1 * np.eye(1))}
    amcmc = {"n.batch": 3, "batch.length": 4, "accept.rate": 0.43}
    ct, xt = d["coords_test"], d["x_test"]
    with mk.spMvGLM([(d["y"], d["x"])], d["coords"], np.ones((n, 1)), starting, tuning, priors, amcmc, seed=9) as fit:
        pred = mk.spPredict(fit, ct, pred_covars=xt, start=5, end=11, thin=2)
        beta = fit["p.beta.theta.samples"][4:11:2, :2]
        wd, pd = pred["p.w.predictive.samples"], pred["p.y.predictive.samples"]
        assert wd.shape == pd.shape == (N_TEST, 4)
        formula = _linkinv(beta @ xt.T + wd.T, "logit")
        print(f"formula difference {np.abs(pd.T - formula).max():.2e}")
        np.testing.assert_allclose(pd.T, formula, rtol=0, atol=1e-14)
        again = mk.spPredict(fit, ct[:9], start=5, end=11, thin=2)
        assert "p.y.predictive.samples" not in again
        assert np.array_equal(again["p.w.predictive.samples"], wd[:9])
        with pytest.raises(ValueError):
            mk.spPredict(fit, ct, pred_covars=xt[:-1], start=5, end=11)
        back = mk.spPredict(fit, ct, pred_covars=xt, start=5, end=11, thin=2)
        assert np.array_equal(back["p.y.predictive.samples"], pd)


_node = {}


def _node_problem(mk):
    if not _node:
        d, subs = _problem(mk, [70, 64, 80, 75, 66], 1, seed=3)
        _node.update(d=d, subs=subs)
    return _node["d"], _node["subs"]


@pytest.mark.parametrize("tile", [0, 7])
def test_node_combines_the_third_grid(mk, tile):
    """K = 5 subsets over three blocks of one device, fused and with 7-site tiles: per-subset p.predict
    as one session makes it, result3 the sequential mean of them, result / result2 as without x_test."""
    d, subs = _node_problem(mk)
    ct, xt = d["coords_test"], d["x_test"]
    cfg = _cfg(mk, 1, predict_tile=tile)
    one = _device(mk, subs, cfg, ct, xt, p_pred_samples=True, p_predict_sum=True)
    got = mk.meta_fit_node(subs, cfg, coords_test=ct, devices=[0, 0, 0], x_test=xt, p_pred_samples=True,
                           p_predict_sum=True)
    for s in range(5):
        assert np.array_equal(got["p_predict"][s], one["p_predict"][s]), s
        assert np.array_equal(got["p_pred_samples"][s], one["p_pred_samples"][s]), s
        assert np.array_equal(got["w_predict"][s], one["w_predict"][s]), s
    assert np.array_equal(got["p_predict_sum"], one["p_predict_sum"])
    assert np.array_equal(got["result3"], om.combine_mean(one["p_predict"]))
    plain = mk.meta_fit_node(subs, cfg, coords_test=ct, devices=[0, 0, 0])
    assert "result3" not in plain and "p_predict" not in plain
    assert np.array_equal(got["result"], plain["result"])
    assert np.array_equal(got["result2"], plain["result2"])


def test_node_median_of_the_third_grid(mk):
    """method = "median": result3 is the Weiszfeld W2 median of the subsets' p.predict grids, per
    column, as result2 is of the w.predict grids (the bar tests/test_gpu_node.py uses)."""
    d, subs = _node_problem(mk)
    ct, xt = d["coords_test"], d["x_test"]
    cfg = _cfg(mk, 1, predict_tile=7)
    one = _device(mk, subs, cfg, ct, xt)
    got = mk.meta_fit_node(subs, cfg, coords_test=ct, devices=[0, 0], x_test=xt, method="median")
    exp3, _ = mk.combine_median(one["p_predict"])
    exp2, _ = mk.combine_median(one["w_predict"])
    np.testing.assert_allclose(got["result3"], exp3, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["result2"], exp2, rtol=0, atol=1e-12)


def test_errors_leave_the_session_usable(mk):
    d, subs = _problem(mk, [60, 50], 1)
    cfg = _cfg(mk, 1)
    lib = mk.load()
    with mk.Session(subs, cfg, coords_test=d["coords_test"]) as ses:      # test sites, no covariates
        ses.run(cfg.n_samples)
        base = ses.outputs()
        assert "p_predict" not in base
        for kw in (dict(p_predict=True), dict(p_pred_samples=True), dict(p_predict_sum=True)):
            with pytest.raises(mk.MkError) as e:
                ses.outputs(**kw)
            assert e.value.code == mk._lib.MK_E_ARG and "x_test" in str(e.value)
        host = np.zeros(2 * N_TEST * 200)
        for which in (3, -1, 2):      # out of range twice, then p grids without covariates
            with pytest.raises(mk.MkError) as e:
                mk._lib.check(lib.mk_session_grids(ses._h, which, host.ctypes.data_as(ctypes.c_void_p), 0))
            assert e.value.code == mk._lib.MK_E_ARG
        after = ses.outputs()
        for s in range(2):
            assert np.array_equal(after["w_predict"][s], base["w_predict"][s])
            assert np.array_equal(after["parameters"][s], base["parameters"][s])
        # covariates set after the run: the grids a session created with them gives
        ses.set_test_covars(d["x_test"])
        late = ses.outputs()
        mk._lib.check(lib.mk_session_grids(ses._h, 2, host.ctypes.data_as(ctypes.c_void_p), 0))
    with_x = _device(mk, subs, cfg, d["coords_test"], d["x_test"])
    for s in range(2):
        assert np.array_equal(late["p_predict"][s], with_x["p_predict"][s])
    assert np.array_equal(host.reshape(2, N_TEST, 200), np.stack([g.T for g in with_x["p_predict"]]))
    with mk.Session(subs, cfg) as ses:                                     # no test sites
        with pytest.raises(mk.MkError) as e:
            mk._lib.check(lib.mk_session_set_test_covars(ses._h, mk._lib.dptr(np.zeros(4))))
        assert e.value.code == mk._lib.MK_E_ARG
        ses.run(cfg.n_samples)
        assert np.array_equal(ses.outputs()["parameters"][0], base["parameters"][0])
    with pytest.raises(mk.MkError) as e:                                   # covariates without test sites
        pr = mk.session.PackedProblem(subs, cfg, None)
        pr.c.x_test = mk._lib.dptr(np.zeros(4))
        c, keep = cfg.to_c()
        h = ctypes.c_void_p()
        mk._lib.check(lib.mk_session_create(ctypes.byref(pr.c), ctypes.byref(c), ctypes.byref(h)))
    assert e.value.code == mk._lib.MK_E_ARG


_ALL = dict(samples=True, w_samples=True, w_pred_samples=True, acceptance=True, w_predict_sum=True, p_predict=True,
            p_pred_samples=True, p_predict_sum=True)
# Session.outputs arguments that ask for one field (quantiles=True brings parameters with w_predict)
_ALONE = dict(parameters=dict(w_predict=False, p_predict=False), w_predict=dict(p_predict=False),
              p_predict=dict(quantiles=False, p_predict=True),
              **{k: {"quantiles": False, k: True} for k in _ALL if k != "p_predict"})


def _assert_same(a, b, what):
    if isinstance(a, list):
        assert len(a) == len(b), what
        for s, (x, y) in enumerate(zip(a, b)):
            assert x.shape == y.shape and np.array_equal(x, y), (what, s)
    else:
        assert a.shape == b.shape and np.array_equal(a, b), what


@pytest.mark.parametrize("tile", [0, 4])
def test_every_field_at_once_equals_each_alone(mk, tile):
    """Ragged subsets (37 / 64 / 50 sites), q = 2, 9 test sites, fused and in tiles of 4, 4 and 1
    sites: one outputs() call with every field on gives, field by field, the arrays of a call that
    asks for that field alone (both grid kinds share one call's scratch), and the node driver over
    two blocks of one device gives the session's arrays, its result2 / result3 the sequential mean
    of the per-subset grids."""
    d, subs = _problem(mk, [37, 64, 50], 2)
    ct, xt = d["coords_test"][:9], d["x_test"][:18]
    cfg = _cfg(mk, 2, predict_tile=tile, n_batch=4, batch_length=5)
    with mk.Session(subs, cfg, coords_test=ct, x_test=xt, record_w=True) as ses:
        ses.run(cfg.n_samples)
        assert ses.predict_tile == tile
        every = ses.outputs(**_ALL)
        assert set(every) == set(_ALONE)
        for field, kw in _ALONE.items():
            _assert_same(ses.outputs(**kw)[field], every[field], field)
    assert every["p_predict"][2].shape == (200, 18) and every["w_samples"][1].shape == (128, 20)
    node_kw = {k: v for k, v in _ALL.items() if k != "p_predict"}
    got = mk.meta_fit_node(subs, cfg, coords_test=ct, devices=[0, 0], x_test=xt, **node_kw)
    for field in ("parameters", "w_predict", "p_predict", "w_pred_samples", "p_pred_samples", "w_predict_sum",
                  "p_predict_sum"):
        _assert_same(got[field], every[field], "node " + field)
    assert np.array_equal(got["result2"], mk.combine(every["w_predict"]))
    assert np.array_equal(got["result3"], mk.combine(every["p_predict"]))
