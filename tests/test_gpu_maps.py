"""Posterior maps on the device (include/mk.h: per test column the mean and sd of w and of p(y = 1) and
the exceedance probabilities of p) against their NumPy restatement tests/maps_ref.py, on the sessions'
own recorded chains and kriging draws.

Bar against the restatement, means and sds: |device - ref| <= 1e-9 |ref| + 1e-12, the standing bar for a
device result against a NumPy restatement (test_gpu_scores.py, test_gpu_criteria.py).  Exceedance planes
are counts over n: they must be equal.  In map_grid the values are read, not computed, so that holds
outright (entries equal to a threshold included); in a session p is computed on both sides, so it holds
under a guard asserted on the restatement alone -- no restated p_kc within 1e-9 of a threshold, seven
orders above the rounding of p.  Tiled against fused, stream groups, chunked against unchunked and the
node driver against one session: bit equality -- a column's planes are one thread's serial work.

Shapes (test_gpu_scores.py's): 64 iterations (n_batch 4 x batch_length 16), burn_in 17: 48 kept; 24 test
sites.  "exp": exponential, logit, q = 1, subsets of 100 and 257 sites.  "mat": Matern, probit, q = 2,
subsets of 129 and 150 sites.  Exact kriging (MK_KRIG_CHEB=0), so a tiled session kriges the fused
session's draws."""
import numpy as np
import pytest

from maps_ref import BASE_NAMES, map_ref, map_ref_grid, map_ref_p, names

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-9, 1e-12
GUARD = 1e-9
N_TEST = 24
KW = dict(n_batch=4, batch_length=16, burn_in=17, seed=9)
KS_MAPS = 17
THR = (0.2, 0.5, 0.8, 0.3141592653589793)
THR8 = THR + (0.1, 0.9, 0.65, 0.05)
_CASES = {"exp": dict(sizes=[100, 257], q=1, cov="exponential", link="logit", trials=3.0),
          "mat": dict(sizes=[129, 150], q=2, cov="matern", link="probit", trials=1.0)}
_runs = {}


def _close(dev, ref, what=""):
    dev, ref = np.asarray(dev, float), np.asarray(ref, float)
    assert dev.shape == ref.shape, what
    same = (dev == ref) | (np.isnan(dev) & np.isnan(ref))
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


def _cfg(mk, q, cov="exponential", link="logit", **kw):
    p = 2 * q
    return mk.SamplerConfig(q, p, beta_starting=np.zeros(p), beta_tuning=np.full(p, 0.05), cov_model=cov, link=link,
                            **KW, **kw)


def _run(mk, name, monkeypatch):
    """One fused fit per case with maps and validation data attached, shared and left unchanged."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    if name not in _runs:
        c = _CASES[name]
        d, subs = _problem(mk, c["sizes"], c["q"], trials=c["trials"], cov=c["cov"])
        cfg = _cfg(mk, c["q"], c["cov"], c["link"])
        r = dict(d=d, subs=subs, q=c["q"], link=c["link"], c=c)
        with mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
            ses.run(64)
            ses.outputs()
            r["off"] = ses.kernel_stats(KS_MAPS)                 # nothing asked for yet
            ses.set_maps(THR)
            ses.set_validation(d["y_test"])
            r["out"] = ses.outputs(samples=True, w_pred_samples=True, p_pred_samples=True)
            r["before"] = ses.kernel_stats(KS_MAPS)
            r["maps"] = ses.maps()
            r["after"] = ses.kernel_stats(KS_MAPS)
            r["again"] = ses.maps()
            r["after2"] = ses.kernel_stats(KS_MAPS)
            r["scores"] = ses.scores(pointwise=True)
            ses.set_maps(())                                     # no thresholds: the four base planes
            r["base"] = ses.maps()
        _runs[name] = r
    return _runs[name]


def _check(got, r, out, first, what, thr=THR):
    """got (Session.maps' dict) against the restatement on the session's own samples and kriging draws
    (out), the draws' first column being iteration `first`."""
    n_sub, C, p = len(r["subs"]), r["q"] * N_TEST, 2 * r["q"]
    J = len(thr)
    assert got["names"] == names(J) and got["thresholds"] == list(thr) and len(got["subsets"]) == n_sub
    n = out["w_pred_samples"][0].shape[1]
    for s in range(n_sub):
        ref = map_ref(out["samples"][s], out["w_pred_samples"][s], r["d"]["x_test"], p, r["link"], thr, first=first)
        pk = map_ref_p(out["samples"][s], out["w_pred_samples"][s], r["d"]["x_test"], p, r["link"], first=first)
        dev = got["subsets"][s]
        assert dev.shape == ref.shape == (C, 4 + J)
        diff = np.where(np.isnan(dev) & np.isnan(ref), 0.0, np.abs(dev - ref)).max(axis=0)
        print(f"{what} subset {s}: largest differences " + ", ".join(f"{nm} {x:.2e}" for nm, x in zip(got["names"], diff)))
        gap = min(np.abs(pk - u).min() for u in thr) if J else np.inf
        print(f"  nearest restated p to a threshold: {gap:.3e}")
        assert gap > GUARD, "a restated p lies within the guard of a threshold: change the thresholds"
        _close(dev[:, :4], ref[:, :4], what)
        assert np.array_equal(dev[:, 4:], ref[:, 4:]), what
        if n > 1:
            assert np.isfinite(dev).all() and (dev[:, [1, 3]] > 0).all()
        else:
            assert np.isnan(dev[:, [1, 3]]).all() and np.isin(dev[:, 4:], (0.0, 1.0)).all()
        if "p_pred_samples" in out:
            _close(dev[:, 2], out["p_pred_samples"][s].mean(axis=1), what + " p_mean")   # the mean of the p draws


def _same(a, b):
    assert a["names"] == b["names"]
    for x, y in zip(a["subsets"], b["subsets"]):
        assert np.array_equal(x, y, equal_nan=True)


# ---------------------------------------------------------------- 1. map_grid
def _grid_case(n_rows, C, thr):
    rng = np.random.default_rng(1000 * n_rows + C)
    g = rng.uniform(0.0, 1.0, size=(n_rows, C))
    for u in thr:                                                    # entries exactly at a threshold: not counted
        k = max(1, (n_rows * C) // 16)
        g[rng.integers(0, n_rows, k), rng.integers(0, C, k)] = u
    return g


@pytest.mark.parametrize("C", [1, 255, 256, 257, 1300])
@pytest.mark.parametrize("n_rows", [1, 2, 200, 1251])
def test_map_grid_against_restatement(mk, n_rows, C, monkeypatch):
    for J in (0, 3, 8):
        monkeypatch.delenv("MK_MAP_CHUNK", raising=False)
        thr = THR8[:J]
        g = _grid_case(n_rows, C, thr)
        got = mk.map_grid(g, thr)
        ref = map_ref_grid(g, thr)
        dev = got["planes"]
        assert got["names"] == names(J, ("mean", "sd")) and dev.shape == ref.shape == (C, 2 + J)
        with np.errstate(invalid="ignore"):
            print(f"n_rows {n_rows} C {C} J {J}: largest differences mean {np.abs(dev[:, 0] - ref[:, 0]).max():.2e}, "
                  f"sd {np.abs(dev[:, 1] - ref[:, 1]).max():.2e}; entries at a threshold "
                  f"{sum(int((g == u).sum()) for u in thr)}")
        _close(dev[:, :2], ref[:, :2], "mean, sd")
        assert np.isnan(dev[:, 1]).all() if n_rows == 1 else np.isfinite(dev).all()
        assert np.array_equal(dev[:, 2:], ref[:, 2:])                # read, not computed: equal
        if C > 100:                     # chunks of 100 columns: the unchunked call bit for bit
            monkeypatch.setenv("MK_MAP_CHUNK", "100")
            assert np.array_equal(mk.map_grid(g, thr)["planes"], dev, equal_nan=True)


def test_map_grid_poisoned_column(mk, monkeypatch):
    """One NaN in a column makes every plane of that column NaN and leaves its neighbours as they were
    (chunked too); so does an infinite entry."""
    monkeypatch.delenv("MK_MAP_CHUNK", raising=False)
    g = _grid_case(200, 257, THR)
    clean = mk.map_grid(g, THR)["planes"]
    g[100, 200] = np.nan
    g[0, 256] = np.inf
    rest = np.ones(257, bool)
    rest[[200, 256]] = False
    for chunk in (None, "64"):
        if chunk:
            monkeypatch.setenv("MK_MAP_CHUNK", chunk)
        got = mk.map_grid(g, THR)["planes"]
        assert np.isnan(got[[200, 256]]).all()
        assert np.isfinite(got[rest]).all() and np.array_equal(got[rest], clean[rest])
    assert np.array_equal(np.isnan(map_ref_grid(g, THR)), np.isnan(got))


# ---------------------------------------------------------------- 2. fused sessions
@pytest.mark.parametrize("name", list(_CASES))
def test_fused_against_restatement(mk, name, monkeypatch):
    r = _run(mk, name, monkeypatch)
    _check(r["maps"], r, r["out"], KW["burn_in"], "fused " + name)
    _check(r["base"], r, r["out"], KW["burn_in"], "fused, no thresholds, " + name, thr=())
    for s in range(2):                                           # the same four planes whatever J
        assert np.array_equal(r["base"]["subsets"][s], r["maps"]["subsets"][s][:, :4])
        # the scores' pmean is this plane, bit for bit
        assert np.array_equal(r["maps"]["subsets"][s][:, 2], r["scores"]["pointwise"][s][:, 0])
    _same(r["again"], r["maps"])
    # off: nothing launched; attached but not asked for: nothing launched; one k_map_cols per maps()
    assert r["off"] == dict(launches=0, ms=0.0, flops=0.0)
    assert r["before"]["launches"] == 0 and r["after"]["launches"] == 1 and r["after2"]["launches"] == 2
    assert r["after"]["ms"] > 0.0


# ---------------------------------------------------------------- 3, 4. tiled equals fused; windows
@pytest.mark.parametrize("name", list(_CASES))
def test_tiled_equals_fused_and_windows(mk, name, monkeypatch):
    """predict_tile = 16 over the 24 sites: tiles of 16 and 8.  Once through outputs, once tile by tile
    through tile_grids (maps() between the two tiles names the second).  Then the kept window (20, 60):
    stale until every tile is replayed over it, then the restatement on those 41 states; then the
    one-state window (30, 30): sd NaN, exceedance 0 or 1."""
    r = _run(mk, name, monkeypatch)
    c, d = r["c"], r["d"]
    cfg = _cfg(mk, c["q"], c["cov"], c["link"], predict_tile=16)
    with mk.Session(r["subs"], cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(64)
        assert ses.predict_tile == 16
        ses.set_maps(THR)
        with pytest.raises(mk.MkError) as none_yet:
            ses.maps()
        ses.outputs(quantiles=False, w_predict_sum=True)
        through_outputs = ses.maps()
        launches = ses.kernel_stats(KS_MAPS)["launches"]
        ses.set_maps(THR)                                        # attached anew: no tile replayed yet
        ses.tile_grids(0)
        with pytest.raises(mk.MkError) as second:
            ses.maps()
        ses.tile_grids(16, prob=True)
        by_tile = ses.maps()
        launches2 = ses.kernel_stats(KS_MAPS)["launches"]
        ses.set_kept_window(20, 60)
        with pytest.raises(mk.MkError) as stale:
            ses.maps()                                           # the planes in the buffer are another window's
        ses.tile_grids(0)
        with pytest.raises(mk.MkError) as other_window:
            ses.maps()                                           # tile 1 was filled over another window
        win_out = ses.outputs(quantiles=False, samples=True, w_pred_samples=True, p_pred_samples=True)
        window = ses.maps()
        ses.set_kept_window(30, 30)
        with pytest.raises(mk.MkError) as stale_one:
            ses.maps()
        one_out = ses.outputs(quantiles=False, samples=True, w_pred_samples=True, p_pred_samples=True)
        one = ses.maps()
    for e, tile in ((none_yet, "tile 0 "), (second, "tile 1 (test sites 16 .. 23)"), (stale, "tile 0 "),
                    (other_window, "tile 1 "), (stale_one, "tile 0 ")):
        assert e.value.code == mk._lib.MK_E_ARG and tile in str(e.value)
    assert launches == 2 and launches2 == 4                      # one k_map_cols per tile replay, none per maps()
    _same(through_outputs, r["maps"])
    _same(by_tile, r["maps"])
    assert win_out["w_pred_samples"][0].shape == (c["q"] * N_TEST, 41)
    _check(window, r, win_out, 20, "window " + name)
    assert one_out["w_pred_samples"][0].shape == (c["q"] * N_TEST, 1)
    _check(one, r, one_out, 30, "one state " + name)


def test_stream_groups_equal_one(mk, monkeypatch):
    """n_streams = 2 (the two subsets on a stream each): the planes of the one-stream session bit for bit
    (both on the sequential schedule, as stream groups run: test_gpu_post.py's invariant for the chains)."""
    r = _run(mk, "exp", monkeypatch)
    c, d = r["c"], r["d"]
    got = {}
    for ns in (1, 2):
        cfg = _cfg(mk, c["q"], c["cov"], c["link"], n_streams=ns)
        with mk.Session(r["subs"], cfg, coords_test=d["coords_test"], x_test=d["x_test"],
                        lookahead=0 if ns == 1 else None) as ses:
            assert not ses.lookahead
            ses.run(64)
            ses.set_maps(THR)
            got[ns] = ses.maps()
    assert np.isfinite(got[1]["subsets"][1]).all()
    _same(got[2], got[1])


# ---------------------------------------------------------------- 3. the node driver
_node = {}


@pytest.mark.parametrize("tile", [0, 16])
def test_node_equals_one_session(mk, tile, monkeypatch):
    """Four q = 1 subsets over two blocks of one device, fused and tiled: the planes of one session bit for
    bit; the combined planes are map_grid of the returned result2 (w_mean, w_sd) and result3 (the others),
    and those of the one-block call."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    if not _node:
        d, subs = _problem(mk, [150, 163, 140, 129], 1, seed=4)
        cfg = _cfg(mk, 1)
        with mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
            ses.run(64)
            ses.set_maps(THR)
            _node.update(d=d, subs=subs, one=ses.maps())
        monkeypatch.setenv("MK_EXCHANGE", "copy")               # one block: no RCCL communicator (seconds to create)
        _node["one_block"] = mk.meta_fit_node(subs, cfg, coords_test=d["coords_test"], devices=(0,), x_test=d["x_test"],
                                              maps=THR)
        monkeypatch.delenv("MK_EXCHANGE")
    d, subs, one = _node["d"], _node["subs"], _node["one"]
    cfg = _cfg(mk, 1, predict_tile=tile)
    got = mk.meta_fit_node(subs, cfg, coords_test=d["coords_test"], devices=(0, 0), x_test=d["x_test"], maps=THR)
    _same(got["maps"], one)
    assert got["maps"]["names"] == names(4) == BASE_NAMES + ["exc_1", "exc_2", "exc_3", "exc_4"]
    comb = got["maps_combined"]
    assert comb.shape == (N_TEST, 8) and np.isfinite(comb).all()
    w, p = mk.map_grid(got["result2"], ()), mk.map_grid(got["result3"], THR)
    assert np.array_equal(comb[:, :2], w["planes"]) and np.array_equal(comb[:, 2:], p["planes"])
    assert np.array_equal(comb, _node["one_block"]["maps_combined"])
    _same(_node["one_block"]["maps"], one)
    _close(comb[:, :2], map_ref_grid(got["result2"]), "combined w")
    ref = map_ref_grid(got["result3"], THR)
    _close(comb[:, 2:4], ref[:, :2], "combined p")
    assert np.array_equal(comb[:, 4:], ref[:, 2:])
    for f in ("result", "result2", "result3"):                   # the split changes nothing else either
        assert np.array_equal(_node["one_block"][f], got[f]), f


# ---------------------------------------------------------------- 5. off means free; errors
def test_off_means_free_and_errors(mk, monkeypatch):
    """Nothing asked for: no kind-17 launch through outputs() of a tiled session.  set_maps(None) and
    set_test_sites detach.  Argument errors name the entry."""
    r = _run(mk, "exp", monkeypatch)
    c, d = r["c"], r["d"]
    cfg = _cfg(mk, c["q"], c["cov"], c["link"], predict_tile=16)
    with mk.Session(r["subs"], cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(64)
        ses.outputs()
        assert ses.kernel_stats(KS_MAPS) == dict(launches=0, ms=0.0, flops=0.0)
        with pytest.raises(mk.MkError) as e:
            ses.maps()
        assert e.value.code == mk._lib.MK_E_ARG and "mk_session_set_maps" in str(e.value)
        for bad, what in (((0.2, np.nan), "threshold 1 "), (np.linspace(0.1, 0.9, 9), "n_thresholds = 9")):
            with pytest.raises(mk.MkError) as e:
                ses.set_maps(bad)
            assert e.value.code == mk._lib.MK_E_ARG and what in str(e.value)
        ses.set_maps(THR)
        ses.set_test_sites(d["coords_test"], x_test=d["x_test"])     # new sites: the maps are dropped
        ses.outputs(quantiles=False, w_predict_sum=True)
        assert ses.kernel_stats(KS_MAPS)["launches"] == 0
        with pytest.raises(mk.MkError) as e:
            ses.maps()
        assert "mk_session_set_maps" in str(e.value)
        ses.set_maps(THR)
        ses.set_maps(None)                                       # detached by hand
        ses.outputs(quantiles=False, w_predict_sum=True)
        assert ses.kernel_stats(KS_MAPS)["launches"] == 0
        with pytest.raises(mk.MkError):
            ses.maps()
        ses.set_maps(THR)
        ses.outputs(quantiles=False, w_predict_sum=True)
        assert ses.kernel_stats(KS_MAPS)["launches"] == 2            # one per tile replay
        _same(ses.maps(), r["maps"])
    with mk.Session(r["subs"][:1], _cfg(mk, 1), coords_test=d["coords_test"]) as ses:      # no x_test
        with pytest.raises(mk.MkError) as e:
            ses.set_maps(THR)
        assert e.value.code == mk._lib.MK_E_ARG and "x_test" in str(e.value)
        ses.set_test_covars(d["x_test"])
        ses.set_maps(THR)
        with pytest.raises(mk.MkError) as e:
            ses.maps()                                           # the chain has not run
        assert e.value.code == mk._lib.MK_E_ARG and "iterations" in str(e.value)


# ---------------------------------------------------------------- the Python surfaces
def test_spmaps_meta_fit_and_reference_flow(mk, monkeypatch):
    """spMaps(fit, coords, covars, thresholds, start, end) is the restatement on the fit's own samples and
    spPredict's w draws of the same window; spPredict still works afterwards, a closed fit raises.
    reference_flow(maps=) carries the node call's planes, meta_fit(maps=) each subset's: the same chains,
    the same planes bit for bit."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    n = 80
    d = mk.synthetic.generate(n, q=1, n_test=N_TEST, seed=31)
    starting = {"beta": np.zeros(2), "phi": 3 / 0.5, "A": np.ones(1), "w": 0.0}
    tuning = {"beta": np.full(2, 0.05), "phi": 1.0, "A": 0.1, "w": 0.5}
    priors = {"phi.Unif": (3 / 0.75, 3 / 0.25), "K.IW": (1, 0.1 * np.eye(1))}
    amcmc = {"n.batch": 4, "batch.length": 16, "accept.rate": 0.43}
    with mk.spMvGLM([(d["y"], d["x"])], d["coords"], np.ones((n, 1)), starting, tuning, priors, amcmc, seed=9) as fit:
        got = mk.spMaps(fit, d["coords_test"], d["x_test"], THR, start=17, end=64)
        pred = mk.spPredict(fit, d["coords_test"], d["x_test"], start=17, end=64)
        with pytest.raises(ValueError):
            mk.spMaps(fit, d["coords_test"], d["x_test"], THR, start=10, end=9)
    with pytest.raises(ValueError):
        mk.spMaps(fit, d["coords_test"], d["x_test"], THR)       # closed
    assert list(got) == ["w.mean", "w.sd", "p.mean", "p.sd", "exceedance", "thresholds"]
    ref = map_ref(fit["p.beta.theta.samples"], pred["p.w.predictive.samples"], d["x_test"], 2, "logit", THR, first=17)
    pk = map_ref_p(fit["p.beta.theta.samples"], pred["p.w.predictive.samples"], d["x_test"], 2, "logit", first=17)
    assert min(np.abs(pk - u).min() for u in THR) > GUARD
    for k, nm in enumerate(("w.mean", "w.sd", "p.mean", "p.sd")):
        _close(got[nm], ref[:, k], nm)
    assert np.array_equal(got["exceedance"], ref[:, 4:]) and got["thresholds"] == list(THR)
    _close(got["p.mean"], pred["p.y.predictive.samples"].mean(axis=1), "p.mean")

    d = mk.synthetic.generate(300, q=1, n_test=N_TEST, seed=12)
    ph, result, result2, summ, cfg = mk.metakriging.reference_flow(d, 2, 1, n_batch=4, batch_length=16, devices=(0, 0),
                                                                   samplesize=50, maps=(0.5,))
    m = summ["maps"]
    assert m["names"] == names(1) and m["combined"].shape == (N_TEST, 5) and len(m["subsets"]) == 2
    assert np.array_equal(m["combined"][:, 2:], mk.map_grid(summ["result3"], (0.5,))["planes"])
    _, index_part = mk.partition(300, 2, seed=20250114, method="R")      # reference_flow's own partition
    obj = mk.meta_fit(d["y"], d["x"], 1.0, d["coords"], 1, index_part, coords_test=d["coords_test"], cfg=cfg,
                      x_test=d["x_test"], maps=(0.5,))
    for i, o in enumerate(obj):
        assert o["maps.names"] == names(1) and np.array_equal(o["maps"], m["subsets"][i])
