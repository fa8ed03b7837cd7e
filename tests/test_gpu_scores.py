"""Held-out validation on the device (include/mk.h: log score, Brier score and error rate per subset
and of the combined p grid) against its NumPy restatement tests/score_ref.py, on the sessions' own
recorded chains and kriging draws.

Bar against the restatement: |device - ref| <= 1e-9 |ref| + 1e-12.  1e-9 is the standing bar for a
device reduction against a NumPy restatement (test_gpu_criteria.py); the absolute term covers lpd_c
near 0, whose absolute rounding is a few ulp of 1 over <= 48 terms (1e-12 leaves two orders of margin).
Tiled against fused, chunked against unchunked and the node driver against one session: bit equality --
a column's pair is one thread's serial work and the sums over columns run in an order fixed by q n_test.

Shapes (test_gpu_criteria.py's): 64 iterations (n_batch 4 x batch_length 16), burn_in 17: 48 kept; 24
test sites.  "exp": exponential, logit, q = 1, subsets of 100 and 257 sites, 3 trials at the test sites,
two test columns with wt = 0.  "mat": Matern, probit, q = 2, subsets of 129 and 150 sites, binary
held-out outcomes (48 columns).  Exact kriging (MK_KRIG_CHEB=0), so a tiled session kriges the fused
session's draws."""
import ctypes

import numpy as np
import pytest

from score_ref import NAMES, score_ref, score_ref_p

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
N_TEST = 24
KW = dict(n_batch=4, batch_length=16, burn_in=17, seed=9)
KS_SCORE = 16
_CASES = {"exp": dict(sizes=[100, 257], q=1, cov="exponential", link="logit", trials=3.0),
          "mat": dict(sizes=[129, 150], q=2, cov="matern", link="probit", trials=1.0)}
_runs = {}


def _close(dev, ref, what=""):
    dev, ref = np.asarray(dev, float), np.asarray(ref, float)
    assert dev.shape == ref.shape, what
    same = (dev == ref) | (np.isnan(dev) & np.isnan(ref))           # -inf, NaN and exact values
    with np.errstate(invalid="ignore"):
        ok = same | (np.abs(dev - ref) <= RTOL * np.abs(ref) + ATOL)
    assert ok.all(), (what, dev[~ok], ref[~ok])


def _problem(mk, sizes, q, seed=9, trials=1.0, cov="exponential"):
    off = np.concatenate([[0], np.cumsum(sizes)])
    d = mk.synthetic.generate(int(off[-1]), q=q, n_test=N_TEST, cov_model=1 if cov == "matern" else 0, seed=seed + q)
    subs = []
    for s, m in enumerate(sizes):
        rows = slice(off[s] * q, (off[s] + m) * q)
        subs.append(dict(coords=d["coords"][off[s]:off[s] + m], y=d["y"][rows], weights=np.full(m * q, trials),
                         x=d["x"][rows]))
    return d, subs


def _held_out(d, q, trials):
    """Binary outcomes as generated; with three trials, counts drawn here and two columns not observed."""
    C = q * N_TEST
    if trials == 1.0:
        return d["y_test"].copy(), np.ones(C)
    rng = np.random.default_rng(5)
    y, wt = rng.binomial(3, 0.5, C).astype(float), np.full(C, trials)
    y[[3, 17]] = 0.0
    wt[[3, 17]] = 0.0
    return y, wt


def _cfg(mk, q, cov="exponential", link="logit", **kw):
    p = 2 * q
    return mk.SamplerConfig(q, p, beta_starting=np.zeros(p), beta_tuning=np.full(p, 0.05), cov_model=cov, link=link,
                            **KW, **kw)


def _run(mk, name, monkeypatch):
    """One fused fit per case with validation data attached, shared and left unchanged."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    if name not in _runs:
        c = _CASES[name]
        d, subs = _problem(mk, c["sizes"], c["q"], trials=c["trials"], cov=c["cov"])
        y, wt = _held_out(d, c["q"], c["trials"])
        cfg = _cfg(mk, c["q"], c["cov"], c["link"])
        r = dict(d=d, subs=subs, q=c["q"], link=c["link"], y=y, wt=wt, c=c)
        with mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
            ses.run(64)
            ses.set_validation(y, wt)
            r["out"] = ses.outputs(samples=True, w_pred_samples=True, p_pred_samples=True)
            r["before"] = ses.kernel_stats(KS_SCORE)
            r["scores"] = ses.scores(pointwise=True)
            r["after"] = ses.kernel_stats(KS_SCORE)
            r["rows_only"] = ses.scores()
        _runs[name] = r
    return _runs[name]


def _check(got, r, out, first, what):
    """got (Session.scores' dict, with pointwise) against the restatement on the session's own samples
    and kriging draws (out), the draws' first column being iteration `first`."""
    n_sub, C = len(r["subs"]), r["q"] * N_TEST
    assert got["names"] == NAMES and got["subsets"].shape == (n_sub, 5)
    for s in range(n_sub):
        ref, pw = score_ref(out["samples"][s], out["w_pred_samples"][s], r["d"]["x_test"], r["y"], r["wt"], 2 * r["q"],
                            r["link"], first=first)
        dev, dpw = got["subsets"][s], got["pointwise"][s]
        print(f"{what} subset {s}:")
        for k, nm in enumerate(NAMES):
            print(f"  {nm:7s} device {dev[k]: .15e}  restatement {ref[k]: .15e}  difference {dev[k] - ref[k]: .2e}")
        print(f"  pointwise: pmean largest difference {np.abs(dpw[:, 0] - pw[:, 0]).max():.2e}, "
              f"lpd_c largest difference {np.abs(dpw[:, 1] - pw[:, 1]).max():.2e}")
        assert dpw.shape == (C, 2) and np.isfinite(dev).all()
        assert dev[0] == ref[0] == (r["wt"] > 0).sum()
        _close(dev, ref, what)
        _close(dpw, pw, what)
        _close(dpw[:, 0], out["p_pred_samples"][s].mean(axis=1), what + " pmean")      # the mean of the p draws
        assert (dpw[r["wt"] == 0, 1] == 0.0).all()                   # not observed: lpd_c = 0 by itself


def _same(a, b):
    assert np.array_equal(a["subsets"], b["subsets"], equal_nan=True)
    for x, y in zip(a["pointwise"], b["pointwise"]):
        assert np.array_equal(x, y, equal_nan=True)


# ---------------------------------------------------------------- 1. score_grid
def _grid_case(n_rows, C, seed=0):
    rng = np.random.default_rng(1000 * n_rows + C + seed)
    p = rng.uniform(0.0, 1.0, size=(n_rows, C))
    p = np.clip(p, 1e-12, 1.0 - 1e-12)
    wt = rng.choice([0.0, 1.0, 3.0], size=C)
    y = np.floor(rng.uniform(0.0, 1.0, C) * (wt + 1.0))
    if C > 1:
        wt[0], y[0] = 1.0, 1.0                                       # at least one observed column
    else:
        wt[:], y[:] = 3.0, 2.0
    return p, y, wt


@pytest.mark.parametrize("C", [1, 255, 256, 257, 1300])
@pytest.mark.parametrize("n_rows", [1, 2, 200, 1251])
def test_score_grid_against_restatement(mk, n_rows, C, monkeypatch):
    monkeypatch.delenv("MK_SCORE_CHUNK", raising=False)
    p, y, wt = _grid_case(n_rows, C)
    got = mk.score_grid(p, y, wt, pointwise=True)
    ref, pw = score_ref_p(p, y, wt)
    dev = np.array([got[k] for k in NAMES])
    print(f"n_rows {n_rows} C {C}: device {dev}\n  restatement {ref}\n  pointwise largest difference "
          f"{np.abs(got['pointwise'] - pw).max():.2e}")
    assert list(got)[:5] == NAMES and dev[0] == ref[0]
    _close(dev, ref, "row")
    _close(got["pointwise"], pw, "pointwise")
    assert (got["pointwise"][wt == 0, 1] == 0.0).all()
    if C == 1300:                       # chunks of 512: boundaries at 512 and 1024, the unchunked call bit for bit
        monkeypatch.setenv("MK_SCORE_CHUNK", "512")
        again = mk.score_grid(p, y, wt, pointwise=True)
        assert [again[k] for k in NAMES] == [got[k] for k in NAMES]
        assert np.array_equal(again["pointwise"], got["pointwise"])


def test_score_grid_minus_infinity_and_nan(mk, monkeypatch):
    """A column with p = 1 in every level and y < wt scores -inf; a NaN level makes its column's pair NaN
    and lpd, brier and err NaN; the other columns' pairs are untouched (chunked too)."""
    monkeypatch.delenv("MK_SCORE_CHUNK", raising=False)
    p, y, wt = _grid_case(200, 257, seed=3)
    clean = mk.score_grid(p, y, wt, pointwise=True)
    p[:, 5], y[5], wt[5] = 1.0, 1.0, 3.0
    p[7, 6], y[6], wt[6] = 0.0, 0.0, 1.0                              # a zero multiplier at p = 0: contributes 0
    inf = mk.score_grid(p, y, wt, pointwise=True)
    ref, pw = score_ref_p(p, y, wt)
    assert inf["lpd"] == -np.inf == ref[1] and inf["pointwise"][5, 1] == -np.inf and inf["pointwise"][5, 0] == 1.0
    assert np.isfinite(inf["pointwise"][6]).all()
    _close(np.array([inf[k] for k in NAMES]), ref, "row with -inf")
    _close(inf["pointwise"], pw, "pointwise with -inf")
    p[100, 200] = np.nan
    for chunk in (None, "64"):
        if chunk:
            monkeypatch.setenv("MK_SCORE_CHUNK", chunk)
        got = mk.score_grid(p, y, wt, pointwise=True)
        assert np.isnan(got["pointwise"][200]).all()
        assert np.isnan([got["lpd"], got["brier"], got["err"]]).all()
        assert got["n"] == inf["n"] and got["lconst"] == inf["lconst"]
        rest = np.ones(257, bool)
        rest[200] = False
        assert np.array_equal(got["pointwise"][rest], inf["pointwise"][rest])
    rest[[5, 6]] = False
    assert np.array_equal(inf["pointwise"][rest], clean["pointwise"][rest])


# ---------------------------------------------------------------- 2. fused sessions
@pytest.mark.parametrize("name", list(_CASES))
def test_fused_against_restatement(mk, name, monkeypatch):
    r = _run(mk, name, monkeypatch)
    _check(r["scores"], r, r["out"], KW["burn_in"], "fused " + name)
    if name == "exp":
        assert r["scores"]["subsets"][0, 0] == 22 and (r["scores"]["subsets"][:, 4] > 0).all()      # lconst of 3 trials
    else:
        assert (r["scores"]["subsets"][:, 4] == 0.0).all()
    assert "pointwise" not in r["rows_only"] and np.array_equal(r["rows_only"]["subsets"], r["scores"]["subsets"])
    # attached but not asked for: nothing launched; one scores() is k_score_cols + k_score_finish
    assert r["before"]["launches"] == 0 and r["after"]["launches"] == 2 and r["after"]["ms"] > 0.0


# ---------------------------------------------------------------- 3. tiled equals fused
@pytest.mark.parametrize("name", list(_CASES))
def test_tiled_equals_fused(mk, name, monkeypatch):
    """predict_tile = 16 over the 24 sites: tiles of 16 and 8.  Once through outputs, once tile by tile
    through tile_grids (scores() between the two tiles names the second); then the kept window (20, 60)
    against the restatement on those 41 states."""
    r = _run(mk, name, monkeypatch)
    c, d = r["c"], r["d"]
    cfg = _cfg(mk, c["q"], c["cov"], c["link"], predict_tile=16)
    with mk.Session(r["subs"], cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(64)
        assert ses.predict_tile == 16
        ses.set_validation(r["y"], r["wt"])
        with pytest.raises(mk.MkError) as none_yet:
            ses.scores()
        ses.outputs(quantiles=False, w_predict_sum=True)
        through_outputs = ses.scores(pointwise=True)
        launches = ses.kernel_stats(KS_SCORE)["launches"]
        ses.set_validation(r["y"], r["wt"])                      # attached anew: no tile replayed yet
        ses.tile_grids(0)
        with pytest.raises(mk.MkError) as second:
            ses.scores()
        ses.tile_grids(16, prob=True)
        by_tile = ses.scores(pointwise=True)
        ses.set_kept_window(20, 60)
        with pytest.raises(mk.MkError) as stale:
            ses.scores()                                         # the pairs in the buffer are another window's
        with pytest.raises(mk.MkError) as other_window:
            ses.tile_grids(0)
            ses.scores()                                         # tile 1 was scored over another window
        win_out = ses.outputs(quantiles=False, samples=True, w_pred_samples=True, p_pred_samples=True)
        window = ses.scores(pointwise=True)
    assert none_yet.value.code == mk._lib.MK_E_ARG and "tile 0 " in str(none_yet.value)
    assert second.value.code == mk._lib.MK_E_ARG and "tile 1 (test sites 16 .. 23)" in str(second.value)
    assert stale.value.code == mk._lib.MK_E_ARG and "tile 0 " in str(stale.value)
    assert other_window.value.code == mk._lib.MK_E_ARG and "tile 1 " in str(other_window.value)
    assert launches == 3                                         # one k_score_cols per tile, one k_score_finish
    _same(through_outputs, r["scores"])
    _same(by_tile, r["scores"])
    assert win_out["w_pred_samples"][0].shape == (c["q"] * N_TEST, 41)
    _check(window, r, win_out, 20, "window " + name)


# ---------------------------------------------------------------- 4. the node driver
_node = {}


@pytest.mark.parametrize("tile", [0, 16])
def test_node_equals_one_session(mk, tile, monkeypatch):
    """Four q = 1 subsets over two blocks of one device, fused and tiled: the rows and the pairs of one
    session bit for bit; 'combined' is score_grid of result3; without validation the call's other
    outputs are the same."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    if not _node:
        d, subs = _problem(mk, [150, 163, 140, 129], 1, seed=4)
        cfg = _cfg(mk, 1)
        with mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
            ses.run(64)
            ses.set_validation(d["y_test"])
            _node.update(d=d, subs=subs, one=ses.scores(pointwise=True))
    d, subs, one = _node["d"], _node["subs"], _node["one"]
    cfg = _cfg(mk, 1, predict_tile=tile)
    got = mk.meta_fit_node(subs, cfg, coords_test=d["coords_test"], devices=(0, 0), x_test=d["x_test"],
                           validation=dict(y_test=d["y_test"], pointwise=True))
    sc = got["scores"]
    _same(sc, one)
    assert sc["names"] == NAMES and sc["subsets"].shape == (4, 5) and np.isfinite(sc["subsets"]).all()
    grid = mk.score_grid(got["result3"], d["y_test"], pointwise=True)
    assert sc["combined"] == {k: grid[k] for k in NAMES}
    assert np.array_equal(sc["combined_pointwise"], grid["pointwise"])
    ref, pw = score_ref_p(got["result3"], d["y_test"], np.ones(N_TEST))
    _close(np.array([sc["combined"][k] for k in NAMES]), ref, "combined")
    _close(sc["combined_pointwise"], pw, "combined pointwise")
    if tile == 0:
        plain = mk.meta_fit_node(subs, cfg, coords_test=d["coords_test"], devices=(0, 0), x_test=d["x_test"])
        assert "scores" not in plain
        for f in ("result", "result2", "result3"):
            assert np.array_equal(plain[f], got[f]), f
        for f in ("parameters", "w_predict", "p_predict"):
            for s in range(4):
                assert np.array_equal(plain[f][s], got[f][s]), f


# ---------------------------------------------------------------- 5. off costs nothing; errors
def _free_bytes(mk):
    f, t = ctypes.c_int64(), ctypes.c_int64()
    mk._lib.check(mk.load().mk_device_memory(0, ctypes.byref(f), ctypes.byref(t)))
    return f.value


def test_off_costs_nothing_and_errors(mk, monkeypatch):
    """Nothing attached: no kind-16 launch, the same outputs bit for bit and free HBM back at its level
    after outputs (within one 2 MiB allocation granule).  set_test_sites detaches.  Argument errors name the entry."""
    r = _run(mk, "exp", monkeypatch)
    c, d = r["c"], r["d"]
    cfg = _cfg(mk, c["q"], c["cov"], c["link"], predict_tile=16)
    C = N_TEST
    with mk.Session(r["subs"], cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(64)
        ses.outputs()                                            # warm: the replay's own lazy buffers exist
        free0 = _free_bytes(mk)
        plain = ses.outputs(samples=True, w_pred_samples=True, p_pred_samples=True)
        assert abs(_free_bytes(mk) - free0) < 2 << 20
        assert ses.kernel_stats(KS_SCORE) == dict(launches=0, ms=0.0, flops=0.0)
        with pytest.raises(mk.MkError) as e:
            ses.scores()
        assert e.value.code == mk._lib.MK_E_ARG and "mk_session_set_validation" in str(e.value)
        for f in ("samples", "w_pred_samples", "p_pred_samples", "w_predict", "p_predict"):
            for s in range(2):
                assert np.array_equal(plain[f][s], r["out"][f][s]), f      # the fused, attached run's
        for (i, yv, wv) in ((4, 4.0, 3.0), (9, 0.0, -1.0), (11, np.nan, 3.0), (23, 1.0, np.inf)):
            y, wt = r["y"].copy(), r["wt"].copy()
            y[i], wt[i] = yv, wv
            with pytest.raises(mk.MkError) as e:
                ses.set_validation(y, wt)
            assert e.value.code == mk._lib.MK_E_ARG and f"entry {i} " in str(e.value)
        with pytest.raises(ValueError):
            ses.set_validation(r["y"][:-1], 1)
        ses.set_validation(r["y"], r["wt"])
        ses.set_test_sites(d["coords_test"], x_test=d["x_test"])     # new sites: the data are dropped
        ses.outputs(quantiles=False, w_predict_sum=True)
        assert ses.kernel_stats(KS_SCORE)["launches"] == 0
        with pytest.raises(mk.MkError) as e:
            ses.scores()
        assert "mk_session_set_validation" in str(e.value)
        ses.set_validation(r["y"], r["wt"])
        ses.set_validation(None)                                 # detached by hand
        with pytest.raises(mk.MkError):
            ses.scores()
    with mk.Session(r["subs"][:1], _cfg(mk, 1), coords_test=d["coords_test"]) as ses:      # no x_test
        with pytest.raises(mk.MkError) as e:
            ses.set_validation(r["y"], r["wt"])
        assert e.value.code == mk._lib.MK_E_ARG and "x_test" in str(e.value)
        ses.set_test_covars(d["x_test"])
        ses.set_validation(r["y"], r["wt"])
        with pytest.raises(mk.MkError) as e:
            ses.scores()                                         # the chain has not run
        assert e.value.code == mk._lib.MK_E_ARG and "iterations" in str(e.value)
    with pytest.raises(ValueError):
        mk.meta_fit_node(r["subs"], _cfg(mk, 1), coords_test=d["coords_test"], validation=r["y"])      # no x_test
    assert C == r["y"].size


def test_reference_flow_and_meta_fit_carry_the_rows(mk, monkeypatch):
    """reference_flow(validate=True) puts the combined grid's row, the subsets' rows, the median subset's
    row and the host report into the summary; meta_fit(y_test=) puts each subset's row on its dict: the
    same chains, the same rows bit for bit."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    d = mk.synthetic.generate(300, q=1, n_test=N_TEST, seed=12)
    # two blocks on one device: the device-copy exchange (an RCCL communicator takes seconds to create)
    ph, result, result2, summ, cfg = mk.metakriging.reference_flow(d, 2, 1, n_batch=4, batch_length=16, devices=(0, 0),
                                                                   samplesize=50, validate=True)
    v = summ["validation"]
    assert list(v["combined"]) == NAMES and v["names"] == NAMES and v["subsets"].shape == (2, 5)
    assert np.isfinite(v["subsets"]).all() and np.isfinite(list(v["combined"].values())).all()
    assert v["combined"] == {k: x for k, x in mk.score_grid(summ["result3"], d["y_test"]).items()}
    med = v["median_subset"]
    assert med["subset"] == int(np.argmax(v["subsets"][:, 1])) and med["lpd"] == v["subsets"][:, 1].max()   # the better of two
    assert 0.0 <= v["report"]["auc"] <= 1.0 and v["report"]["count"].sum() == N_TEST
    _, index_part = mk.partition(300, 2, seed=20250114, method="R")      # reference_flow's own partition
    obj = mk.meta_fit(d["y"], d["x"], 1.0, d["coords"], 1, index_part, coords_test=d["coords_test"], cfg=cfg,
                      x_test=d["x_test"], y_test=d["y_test"])
    assert "scores" not in mk.meta_fit(d["y"], d["x"], 1.0, d["coords"], 1, index_part[:1], coords_test=d["coords_test"],
                                       cfg=cfg, x_test=d["x_test"])[0]
    for i, o in enumerate(obj):
        assert list(o["scores"]) == NAMES
        assert np.array_equal(np.array([o["scores"][k] for k in NAMES]), v["subsets"][i])
        assert o["scores"]["n"] == N_TEST and o["scores"]["lconst"] == 0.0 and 0.0 <= o["scores"]["brier"] <= 1.0


# ---------------------------------------------------------------- 6. the spBayes surface
def test_spvalidate(mk, monkeypatch):
    """spValidate(fit, coords, covars, y, start, end) is the restatement on spPredict's
    p.y.predictive.samples of the same window (its pmean their mean) and on the fit's own samples and
    spPredict's w draws; spPredict still works afterwards, a closed fit raises."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    n = 80
    d = mk.synthetic.generate(n, q=1, n_test=N_TEST, seed=31)
    starting = {"beta": np.zeros(2), "phi": 3 / 0.5, "A": np.ones(1), "w": 0.0}
    tuning = {"beta": np.full(2, 0.05), "phi": 1.0, "A": 0.1, "w": 0.5}
    priors = {"phi.Unif": (3 / 0.75, 3 / 0.25), "K.IW": (1, 0.1 * np.eye(1))}
    amcmc = {"n.batch": 4, "batch.length": 16, "accept.rate": 0.43}
    wt = np.ones(N_TEST)
    wt[5] = 0.0
    y = d["y_test"] * wt
    with mk.spMvGLM([(d["y"], d["x"])], d["coords"], np.ones((n, 1)), starting, tuning, priors, amcmc, seed=9) as fit:
        got = mk.spValidate(fit, d["coords_test"], d["x_test"], y, weights=wt, start=17, end=64)
        pred = mk.spPredict(fit, d["coords_test"], d["x_test"], start=17, end=64)
        for bad in (dict(start=0), dict(start=10, end=9), dict(end=65)):
            with pytest.raises(ValueError):
                mk.spValidate(fit, d["coords_test"], d["x_test"], y, **bad)
    with pytest.raises(ValueError):
        mk.spValidate(fit, d["coords_test"], d["x_test"], y)     # closed
    assert list(got) == NAMES + ["pmean", "lpd.pointwise"] and got["n"] == N_TEST - 1
    ps = pred["p.y.predictive.samples"]                          # C x 48
    assert ps.shape == (N_TEST, 48)
    ref, pw = score_ref_p(ps.T, y, wt)                           # binary data: the same l from p
    ref2, pw2 = score_ref(fit["p.beta.theta.samples"], pred["p.w.predictive.samples"], d["x_test"], y, wt, 2, "logit",
                          first=17)
    dev = np.array([got[k] for k in NAMES])
    print(f"device {dev}\n from p draws {ref}\n from samples {ref2}")
    for r_, p_ in ((ref, pw), (ref2, pw2)):
        _close(dev, r_, "spValidate row")
        _close(got["pmean"], p_[:, 0], "pmean")
        _close(got["lpd.pointwise"], p_[:, 1], "lpd_c")
    assert got["lpd.pointwise"][5] == 0.0
