"""Cross-outcome prediction on the device (include/mk.h: per test site and pair of outcomes (a, b) the
200-level grids of p_a p_b and p_a - p_b and the planes both_mean, both_sd, diff_mean, diff_sd, corr, a_gt_b,
joint_1..J) against the NumPy restatement tests/pairs_ref.py, on the sessions' own p draws.

The restatement works from the session's p_pred_samples, which are pred_prob's values bit for bit, and a
product, a difference or a comparison of two doubles has one answer: the grids, a_gt_b and joint_j must be
EQUAL.  Means and sds: |device - ref| <= 1e-9 |ref| + 1e-12, the standing bar for a device result against
a NumPy restatement (test_gpu_maps.py).  corr: within 1e-9 absolute, under a guard asserted on the
restatement alone -- every column used has M2 / (n mean^2) > 1e-6, so Welford's relative error in M2 and in
the co-moment (a few n eps / that ratio's root, below 1e-11 at n = 48) stays far under the bar.  Tiled
against fused, stream groups and the node driver against one session: bit equality -- a pair column is one
workgroup's sort and one thread's serial walk.

Shapes (test_gpu_maps.py's): 64 iterations (n_batch 4 x batch_length 16), burn_in 17: 48 kept -- no power of
two, so the sort pads; 24 test sites.  "mat2": Matern, probit, q = 2, subsets of 129 and 150 sites.  "exp3":
exponential, logit, q = 3 (three pairs), subsets of 100 and 257 sites (n_pad 128 and 384).  Exact kriging
(MK_KRIG_CHEB=0), so a tiled session kriges the fused session's draws.

Largest deviations seen on an MI355X (each test prints its own; also in DESIGN.md 4.4): grids, a_gt_b and
joint planes equal; both_mean and diff_mean 0; both_sd 8.3e-17, diff_sd 1.4e-16, corr 1.4e-15; the smallest
M2 / (n mean^2) over the columns used was 1.2e-3."""
import numpy as np
import pytest

from pairs_ref import m2_ratio, names, pair_grids, pair_list, pair_planes

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
CORR_ATOL = 1e-9
M2_GUARD = 1e-6
N_TEST = 24
KW = dict(n_batch=4, batch_length=16, burn_in=17, seed=9)
KS_PAIRS = 18
THR = (0.2, 0.5, 0.8, 0.3141592653589793)
_CASES = {"mat2": dict(sizes=[129, 150], q=2, cov="matern", link="probit"),
          "exp3": dict(sizes=[100, 257], q=3, cov="exponential", link="logit")}
_runs = {}


def _close(dev, ref, what=""):
    dev, ref = np.asarray(dev, float), np.asarray(ref, float)
    assert dev.shape == ref.shape, what
    same = (dev == ref) | (np.isnan(dev) & np.isnan(ref))
    with np.errstate(invalid="ignore"):
        ok = same | (np.abs(dev - ref) <= RTOL * np.abs(ref) + ATOL)
    assert ok.all(), (what, dev[~ok], ref[~ok])


def _problem(mk, sizes, q, seed=9, cov="exponential"):
    off = np.concatenate([[0], np.cumsum(sizes)])
    d = mk.synthetic.generate(int(off[-1]), q=q, n_test=N_TEST, cov_model=1 if cov == "matern" else 0, seed=seed + q)
    subs = []
    for s, m in enumerate(sizes):
        rows = slice(off[s] * q, (off[s] + m) * q)
        subs.append(dict(coords=d["coords"][off[s]:off[s] + m], y=d["y"][rows], weights=np.ones(m * q), x=d["x"][rows]))
    return d, subs


def _cfg(mk, q, cov="exponential", link="logit", **kw):
    p = 2 * q
    return mk.SamplerConfig(q, p, beta_starting=np.zeros(p), beta_tuning=np.full(p, 0.05), cov_model=cov, link=link,
                            **KW, **kw)


def _run(mk, name, monkeypatch):
    """One fused fit per case with pairs attached, shared and left unchanged."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    if name not in _runs:
        c = _CASES[name]
        d, subs = _problem(mk, c["sizes"], c["q"], cov=c["cov"])
        cfg = _cfg(mk, c["q"], c["cov"], c["link"])
        r = dict(d=d, subs=subs, q=c["q"], c=c)
        with mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
            ses.run(64)
            r["out"] = ses.outputs(p_pred_samples=True)
            r["off"] = ses.kernel_stats(KS_PAIRS)                # nothing asked for yet
            with pytest.raises(mk.MkError) as e:
                ses.pairs()
            r["not_asked"] = str(e.value)
            ses.set_pairs(THR)
            ses.outputs()
            r["before"] = ses.kernel_stats(KS_PAIRS)
            r["pairs"] = ses.pairs()
            r["after"] = ses.kernel_stats(KS_PAIRS)
            r["planes_only"] = ses.pairs(grids=False)
            r["after2"] = ses.kernel_stats(KS_PAIRS)
            ses.set_pairs(())                                    # no thresholds: the six base planes
            r["base"] = ses.pairs()
            if name == "exp3":                                   # a NaN covariate: site 5, outcome 1
                x_bad = np.array(d["x_test"], float)
                x_bad[5 * 3 + 1, 0] = np.nan
                ses.set_test_covars(x_bad)
                ses.set_pairs(THR)
                r["poisoned"] = ses.pairs()
        _runs[name] = r
    return _runs[name]


def _check(got, r, p_draws, what, thr=THR):
    """got (Session.pairs' dict) against the restatement on the session's own p draws (per subset C x n)."""
    q, J = r["q"], len(thr)
    n_sub, C2 = len(r["subs"]), len(pair_list(q)) * N_TEST
    assert got["names"] == names(J) and got["pairs"] == pair_list(q) and got["thresholds"] == list(thr)
    assert len(got["subsets"]) == len(got["both_predict"]) == len(got["diff_predict"]) == n_sub
    for s in range(n_sub):
        p = p_draws[s]
        n = p.shape[1]
        both, diff = pair_grids(p, q)
        assert got["both_predict"][s].shape == got["diff_predict"][s].shape == (200, C2)
        assert np.array_equal(got["both_predict"][s], both), what
        assert np.array_equal(got["diff_predict"][s], diff), what
        ref, dev = pair_planes(p, q, thr), got["subsets"][s]
        assert dev.shape == ref.shape == (C2, 6 + J)
        dd = np.where(np.isnan(dev) & np.isnan(ref), 0.0, np.abs(dev - ref)).max(axis=0)
        print(f"{what} subset {s}: largest differences " + ", ".join(f"{nm} {x:.2e}" for nm, x in zip(got["names"], dd)))
        _close(dev[:, :4], ref[:, :4], what)
        assert np.array_equal(dev[:, 5:], ref[:, 5:]), what       # counts over n of the same doubles
        if n > 1:
            spread = m2_ratio(p).min()
            print(f"  smallest M2 / (n mean^2) over the columns: {spread:.3e}")
            assert spread > M2_GUARD, "a p column barely moves: the corr bar does not cover it"
            assert np.isfinite(dev).all() and (np.abs(dev[:, 4]) <= 1.0).all() and (dev[:, [1, 3]] > 0).all()
            assert (np.abs(dev[:, 4] - ref[:, 4]) <= CORR_ATOL).all(), what
        else:
            assert np.isnan(dev[:, [1, 3, 4]]).all() and np.isin(dev[:, 5:], (0.0, 1.0)).all()


def _same(a, b):
    assert a["names"] == b["names"] and a["pairs"] == b["pairs"]
    for f in ("subsets", "both_predict", "diff_predict"):
        assert len(a[f]) == len(b[f])
        for x, y in zip(a[f], b[f]):
            assert np.array_equal(x, y, equal_nan=True), f


# ---------------------------------------------------------------- 1. fused sessions
@pytest.mark.parametrize("name", list(_CASES))
def test_fused_against_restatement(mk, name, monkeypatch):
    r = _run(mk, name, monkeypatch)
    _check(r["pairs"], r, r["out"]["p_pred_samples"], "fused " + name)
    _check(r["base"], r, r["out"]["p_pred_samples"], "fused, no thresholds, " + name, thr=())
    for s in range(2):                                           # the same six planes whatever J, whatever else is asked
        assert np.array_equal(r["base"]["subsets"][s], r["pairs"]["subsets"][s][:, :6])
        assert np.array_equal(r["planes_only"]["subsets"][s], r["pairs"]["subsets"][s])
    assert "both_predict" not in r["planes_only"]
    # off: nothing launched; attached but not asked for: nothing launched; both kernels per pairs(), one for planes alone
    assert r["off"] == dict(launches=0, ms=0.0, flops=0.0) and "mk_session_set_pairs" in r["not_asked"]
    assert r["before"]["launches"] == 0 and r["after"]["launches"] == 2 and r["after2"]["launches"] == 3
    assert r["after"]["ms"] > 0.0


# ---------------------------------------------------------------- 2. tiled equals fused; windows
@pytest.mark.parametrize("name", list(_CASES))
def test_tiled_equals_fused_and_windows(mk, name, monkeypatch):
    """predict_tile = 16 over the 24 sites: tiles of 16 and 8 sites, so of 16 n_pairs and 8 n_pairs pair
    columns.  Once through outputs, once tile by tile through tile_grids (pairs() between the two tiles names
    the second).  Then the kept window (20, 60): stale until every tile is replayed over it, then the
    restatement on those 41 states; then the one-state window (30, 30)."""
    r = _run(mk, name, monkeypatch)
    c, d = r["c"], r["d"]
    cfg = _cfg(mk, c["q"], c["cov"], c["link"], predict_tile=16)
    with mk.Session(r["subs"], cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(64)
        assert ses.predict_tile == 16
        ses.set_pairs(THR)
        with pytest.raises(mk.MkError) as none_yet:
            ses.pairs()
        ses.outputs(quantiles=False, w_predict_sum=True)
        through_outputs = ses.pairs()
        launches = ses.kernel_stats(KS_PAIRS)["launches"]
        ses.set_pairs(THR)                                       # attached anew: no tile replayed yet
        ses.tile_grids(0)
        with pytest.raises(mk.MkError) as second:
            ses.pairs()
        ses.tile_grids(16, prob=True)
        by_tile = ses.pairs()
        launches2 = ses.kernel_stats(KS_PAIRS)["launches"]
        ses.set_kept_window(20, 60)
        with pytest.raises(mk.MkError) as stale:
            ses.pairs()                                          # the buffers hold another window
        ses.tile_grids(0)
        with pytest.raises(mk.MkError) as other_window:
            ses.pairs()                                          # tile 1 was filled over another window
        win_out = ses.outputs(quantiles=False, p_pred_samples=True)
        window = ses.pairs()
        ses.set_kept_window(30, 30)
        with pytest.raises(mk.MkError) as stale_one:
            ses.pairs()
        one_out = ses.outputs(quantiles=False, p_pred_samples=True)
        one = ses.pairs()
    for e, tile in ((none_yet, "tile 0 "), (second, "tile 1 (test sites 16 .. 23)"), (stale, "tile 0 "),
                    (other_window, "tile 1 "), (stale_one, "tile 0 ")):
        assert e.value.code == mk._lib.MK_E_ARG and tile in str(e.value)
    assert launches == 4 and launches2 == 8                      # two kernels per tile replay, none per pairs()
    _same(through_outputs, r["pairs"])
    _same(by_tile, r["pairs"])
    assert win_out["p_pred_samples"][0].shape == (c["q"] * N_TEST, 41)
    _check(window, r, win_out["p_pred_samples"], "window " + name)
    assert one_out["p_pred_samples"][0].shape == (c["q"] * N_TEST, 1)
    _check(one, r, one_out["p_pred_samples"], "one state " + name)


# ---------------------------------------------------------------- 3. stream groups
def test_stream_groups_equal_one(mk, monkeypatch):
    """n_streams = 2 (the two subsets on a stream each): the outputs of the one-stream session bit for bit
    (both on the sequential schedule, as stream groups run)."""
    r = _run(mk, "mat2", monkeypatch)
    c, d = r["c"], r["d"]
    got = {}
    for ns in (1, 2):
        cfg = _cfg(mk, c["q"], c["cov"], c["link"], n_streams=ns)
        with mk.Session(r["subs"], cfg, coords_test=d["coords_test"], x_test=d["x_test"],
                        lookahead=0 if ns == 1 else None) as ses:
            assert not ses.lookahead
            ses.run(64)
            ses.set_pairs(THR)
            got[ns] = ses.pairs()
    assert np.isfinite(got[1]["subsets"][1]).all()
    _same(got[2], got[1])


# ---------------------------------------------------------------- 4. the node driver
@pytest.mark.parametrize("method", ["mean", "median"])
@pytest.mark.parametrize("tile", [0, 16])
def test_node_equals_one_session(mk, tile, method, monkeypatch):
    """The two q = 3 subsets over two blocks of one device, fused and tiled: the per-subset outputs of one
    session bit for bit; result_both / result_diff are the combine of the per-subset grids (mean: also the
    in-order NumPy sum over K), pairs_combined is map_grid of them."""
    r = _run(mk, "exp3", monkeypatch)
    c, d, one = r["c"], r["d"], r["pairs"]
    cfg = _cfg(mk, c["q"], c["cov"], c["link"], predict_tile=tile)
    got = mk.meta_fit_node(r["subs"], cfg, coords_test=d["coords_test"], devices=(0, 0), x_test=d["x_test"], pairs=THR,
                           method=method)
    _same(got["pairs"], one)
    assert got["pairs"]["thresholds"] == list(THR) and got["pairs"]["names"] == names(4)
    C2 = 3 * N_TEST
    for f, key in (("both_predict", "result_both"), ("diff_predict", "result_diff")):
        grids = got["pairs"][f]
        assert got[key].shape == (200, C2) and np.isfinite(got[key]).all()
        if method == "mean":
            assert np.array_equal(got[key], mk.combine(grids))
            assert np.array_equal(got[key], (grids[0] + grids[1]) / 2.0)
        else:
            assert np.array_equal(got[key], mk.combine_median(grids)[0])
    pc = got["pairs_combined"]
    both, diff = mk.map_grid(got["result_both"], THR), mk.map_grid(got["result_diff"], (0.0,))
    assert pc["both"]["names"] == both["names"] and np.array_equal(pc["both"]["planes"], both["planes"])
    assert pc["diff"]["thresholds"] == [0.0] and np.array_equal(pc["diff"]["planes"], diff["planes"])
    assert pc["both"]["planes"].shape == (C2, 6) and pc["diff"]["planes"].shape == (C2, 3)
    # the rest of the node call is what it is without pairs
    for s in range(2):
        assert np.array_equal(got["p_predict"][s], r["out"]["p_predict"][s])


# ---------------------------------------------------------------- 5. a poisoned draw
def test_poisoned_draw(mk, monkeypatch):
    """A NaN covariate at (site 5, outcome 1) makes eta of that column NaN in every state: the planes of the
    pairs (0, 1) and (1, 2) at site 5 are NaN, every other pair column is what it was."""
    r = _run(mk, "exp3", monkeypatch)
    bad = np.zeros(3 * N_TEST, bool)
    bad[[5 * 3 + 0, 5 * 3 + 2]] = True
    for s in range(2):
        got, clean = r["poisoned"]["subsets"][s], r["pairs"]["subsets"][s]
        assert np.isnan(got[bad]).all()
        assert np.isfinite(got[~bad]).all() and np.array_equal(got[~bad], clean[~bad])
        for f in ("both_predict", "diff_predict"):
            assert np.array_equal(r["poisoned"][f][s][:, ~bad], r["pairs"][f][s][:, ~bad])


# ---------------------------------------------------------------- 6. off means free; errors
def test_off_means_free_and_errors(mk, monkeypatch):
    """Nothing asked for: no kind-18 launch through outputs() of a tiled session.  set_pairs(None) and
    set_test_sites detach.  Argument errors name the entry and leave the session usable."""
    r = _run(mk, "mat2", monkeypatch)
    c, d = r["c"], r["d"]
    cfg = _cfg(mk, c["q"], c["cov"], c["link"], predict_tile=16)
    with mk.Session(r["subs"], cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(64)
        ses.outputs()
        assert ses.kernel_stats(KS_PAIRS) == dict(launches=0, ms=0.0, flops=0.0)
        with pytest.raises(mk.MkError) as e:
            ses.pairs()
        assert e.value.code == mk._lib.MK_E_ARG and "mk_session_set_pairs" in str(e.value)
        for bad, what in (((0.2, np.nan), "threshold 1 "), (np.linspace(0.1, 0.9, 9), "n_thresholds = 9")):
            with pytest.raises(mk.MkError) as e:
                ses.set_pairs(bad)
            assert e.value.code == mk._lib.MK_E_ARG and what in str(e.value)
        ses.set_pairs(THR)
        ses.set_test_sites(d["coords_test"])                         # new sites: the pairs are dropped, no x_test yet
        with pytest.raises(mk.MkError) as e:
            ses.set_pairs(THR)
        assert e.value.code == mk._lib.MK_E_ARG and "x_test" in str(e.value)
        ses.set_test_covars(d["x_test"])
        ses.outputs(quantiles=False, w_predict_sum=True)
        assert ses.kernel_stats(KS_PAIRS)["launches"] == 0
        with pytest.raises(mk.MkError) as e:
            ses.pairs()
        assert "mk_session_set_pairs" in str(e.value)
        ses.set_pairs(THR)
        ses.set_pairs(None)                                      # detached by hand
        ses.outputs(quantiles=False, w_predict_sum=True)
        assert ses.kernel_stats(KS_PAIRS)["launches"] == 0
        with pytest.raises(mk.MkError):
            ses.pairs()
        ses.set_pairs(THR)
        ses.outputs(quantiles=False, w_predict_sum=True)
        assert ses.kernel_stats(KS_PAIRS)["launches"] == 4           # two kernels per tile replay
        _same(ses.pairs(), r["pairs"])
    d1, subs1 = _problem(mk, [60], 1)
    with mk.Session(subs1, _cfg(mk, 1), coords_test=d1["coords_test"], x_test=d1["x_test"]) as ses:      # q = 1
        with pytest.raises(mk.MkError) as e:
            ses.set_pairs(THR)
        assert e.value.code == mk._lib.MK_E_ARG and "q >= 2" in str(e.value)
        ses.run(64)
        assert ses.outputs()["p_predict"][0].shape == (200, N_TEST)      # still usable
        assert ses.kernel_stats(KS_PAIRS)["launches"] == 0
    with mk.Session(r["subs"][:1], _cfg(mk, c["q"], c["cov"], c["link"]), coords_test=d["coords_test"]) as ses:   # no x_test
        with pytest.raises(mk.MkError) as e:
            ses.set_pairs(THR)
        assert e.value.code == mk._lib.MK_E_ARG and "x_test" in str(e.value)
        ses.set_test_covars(d["x_test"])
        ses.set_pairs(THR)
        with pytest.raises(mk.MkError) as e:
            ses.pairs()                                          # the chain has not run
        assert e.value.code == mk._lib.MK_E_ARG and "iterations" in str(e.value)


# ---------------------------------------------------------------- 7. the Python surfaces
def test_sppairs_meta_fit_and_reference_flow(mk, monkeypatch):
    """spPairs(fit, coords, covars, thresholds, start, end) is the restatement on spPredict's p draws of the
    same window of a q = 2 fit; a closed fit raises.  reference_flow(pairs=) carries the node call's outputs,
    meta_fit(pairs=) each subset's: the same chains, the same numbers bit for bit."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    n, q = 80, 2
    d = mk.synthetic.generate(n, q=q, n_test=N_TEST, seed=31)
    p = d["x"].shape[1]
    starting = {"beta": np.zeros(p), "phi": np.full(q, 3 / 0.5), "A": np.array([1.0, 0.0, 1.0]), "w": 0.0}
    tuning = {"beta": np.full(p, 0.05), "phi": np.full(q, 1.0), "A": np.full(3, 0.1), "w": 0.5}
    priors = {"phi.Unif": (np.full(q, 3 / 0.75), np.full(q, 3 / 0.25)), "K.IW": (q, 0.1 * np.eye(q))}
    amcmc = {"n.batch": 4, "batch.length": 16, "accept.rate": 0.43}
    y = d["y"].reshape(n, q)
    formulas = [(y[:, h], d["x"][h::q][:, h * (p // q):(h + 1) * (p // q)]) for h in range(q)]
    with mk.spMvGLM(formulas, d["coords"], np.ones((n, q)), starting, tuning, priors, amcmc, seed=9) as fit:
        got = mk.spPairs(fit, d["coords_test"], d["x_test"], THR, start=17, end=64)
        pred = mk.spPredict(fit, d["coords_test"], d["x_test"], start=17, end=64)
        with pytest.raises(ValueError):
            mk.spPairs(fit, d["coords_test"], d["x_test"], THR, start=10, end=9)
    with pytest.raises(ValueError):
        mk.spPairs(fit, d["coords_test"], d["x_test"], THR)      # closed
    assert list(got) == ["both.predict", "diff.predict", "both.mean", "both.sd", "diff.mean", "diff.sd", "corr", "a.gt.b",
                         "joint", "pairs", "thresholds"]
    pk = pred["p.y.predictive.samples"]
    both, diff = pair_grids(pk, q)
    assert np.array_equal(got["both.predict"], both) and np.array_equal(got["diff.predict"], diff)
    ref = pair_planes(pk, q, THR)
    for k, nm in enumerate(("both.mean", "both.sd", "diff.mean", "diff.sd")):
        _close(got[nm], ref[:, k], nm)
    assert m2_ratio(pk).min() > M2_GUARD and (np.abs(got["corr"] - ref[:, 4]) <= CORR_ATOL).all()
    assert np.array_equal(got["a.gt.b"], ref[:, 5]) and np.array_equal(got["joint"], ref[:, 6:])
    assert got["pairs"] == [(0, 1)] and got["thresholds"] == list(THR)

    d = mk.synthetic.generate(300, q=q, n_test=N_TEST, seed=12)
    ph, result, result2, summ, cfg = mk.metakriging.reference_flow(d, 2, q, n_batch=4, batch_length=16, devices=(0, 0),
                                                                   samplesize=50, pairs=(0.5,))
    m = summ["pairs"]
    assert m["names"] == names(1) and m["pairs"] == [(0, 1)] and len(m["subsets"]) == 2
    assert m["result_both"].shape == m["result_diff"].shape == (200, N_TEST)
    assert np.array_equal(m["result_both"], mk.combine(m["both_predict"]))
    assert np.array_equal(m["combined"]["diff"]["planes"], mk.map_grid(m["result_diff"], (0.0,))["planes"])
    _, index_part = mk.partition(300, 2, seed=20250114, method="R")      # reference_flow's own partition
    obj = mk.meta_fit(d["y"], d["x"], 1.0, d["coords"], q, index_part, coords_test=d["coords_test"], cfg=cfg,
                      x_test=d["x_test"], pairs=(0.5,))
    for i, o in enumerate(obj):
        assert o["pairs.names"] == names(1) and o["pairs.list"] == [(0, 1)]
        assert np.array_equal(o["pairs"], m["subsets"][i])
        assert np.array_equal(o["both.predict"], m["both_predict"][i])
        assert np.array_equal(o["diff.predict"], m["diff_predict"][i])
