"""Areal prediction on the device (include/mk.h "areal prediction": the prevalence of a region, r = sum_i
omega_i p_i over its test sites, from kriging draws that are joint across the region's sites) against the
NumPy / SciPy restatement tests/regions_ref.py, which works from the fit's recorded p.beta.theta.samples and
p.w.samples alone.

Fits: spMvGLM with n.batch = 4, batch.length = 10 (40 iterations, every one recorded), window 21..40.
"lmc": q = 2 exponential, one subset of 150 sites (n_pad = 256: two K tiles of the SYRK, a ragged tail, the
bordered row n_s = 150 inside the last 16-deep chunk), phi prior [4, 12]; 179 test sites on a jittered grid of
spacing 0.03 in regions of 1, 17, 128 and 33 sites (the 128-site region's window would pass column 256 of
X and is moved left; the last region ends the buffer's valid part), unequal weights.  "mat": q = 1 Matern, nu
prior [0.3, 0.9], 100 sites, 91 test sites at spacing 0.05 in regions of 1, 17, 40 and 33.

Bars.  Draws: 1e-8 absolute, the project's draw bar, under a guard asserted on the restatement alone: every
(state, outcome, region) has cond(S) <= 1e4, so the Cholesky's forward error stays near 128 x 2^-53 x 1e4 ~
1e-10.  One-site regions against p_pred_samples of the same replay: 1e-10 (only the summation order of the
kriging variance differs), where 1 - s >= 1e-3.  Grids: equal to the type-7 quantiles of the returned draws.
Planes: the maps' bars against tests/maps_ref.py's formulas on the returned draws (1e-9 relative + 1e-12;
exceedances equal).

Largest figures seen on an MI355X (each test prints its own): cond(S) 1.6e2 ("lmc") and 1.5e2 ("mat"); draws
against the restatement 1.6e-15 and 1.1e-14, with a flagged factor 1.6e-15; one-site regions against the p
draws 1.1e-15 (smallest 1 - s 9.5e-3); planes equal; region.sd of the 128-site region 0.0528 / 0.0468 against
0.0469 / 0.0466 for the averaged marginal draws."""
import ctypes

import numpy as np
import pytest

from regions_ref import RegionRef, grids, planes

pytestmark = pytest.mark.gpu
DRAW_ATOL = 1e-8
ONE_SITE_ATOL = 1e-10
COND_MAX = 1e4
RTOL, ATOL = 1e-9, 1e-12
FIRST, LAST = 21, 40
N_WIN = LAST - FIRST + 1
THR = (0.2, 0.5, 0.3141592653589793)
KS_REGIONS = 19
SEED = 9
_CASES = {"lmc": dict(q=2, n=150, cov="exponential", sizes=(1, 17, 128, 33), spacing=0.03, seed=5),
          "mat": dict(q=1, n=100, cov="matern", sizes=(1, 17, 40, 33), spacing=0.05, seed=6)}
_fits = {}


def _grid_sites(n_test, spacing, rng):
    """n_test sites on a square grid of the given spacing inside the unit square, row by row, each moved by up
    to a fifth of the spacing."""
    side = int(np.ceil(np.sqrt(n_test)))
    lo = 0.5 - 0.5 * spacing * (side - 1)
    ij = np.array([(i, j) for i in range(side) for j in range(side)][:n_test], float)
    return lo + spacing * ij + rng.uniform(-0.2 * spacing, 0.2 * spacing, size=(n_test, 2))


def _fit(mk, name):
    """One fit per case, shared: the fit object (its session stays open) and the problem."""
    if name not in _fits:
        c = _CASES[name]
        q, n = c["q"], c["n"]
        d = mk.synthetic.generate(n, q=q, n_test=1, cov_model=1 if c["cov"] == "matern" else 0, seed=c["seed"])
        p = 2 * q
        rng = np.random.default_rng(100 + c["seed"])
        n_test = sum(c["sizes"])
        ct = _grid_sites(n_test, c["spacing"], rng)
        xt = mk.synthetic.block_design(rng.standard_normal((n_test, q)), q)
        wts = rng.uniform(0.5, 3.0, size=n_test)
        formula = [(d["y"][a::q], d["x"][a::q, 2 * a:2 * a + 2]) for a in range(q)]
        starting = {"beta": np.zeros(p), "phi": 6.0, "A": np.eye(q)[np.tril_indices(q)], "w": 0.0}
        tuning = {"beta": np.full(p, 0.05), "phi": 1.0, "A": 0.1, "w": 0.5}
        priors = {"phi.Unif": (4.0, 12.0), "K.IW": (q, 0.1 * np.eye(q))}
        if c["cov"] == "matern":
            starting["nu"], tuning["nu"], priors["nu.Unif"] = 0.5, 0.1, (0.3, 0.9)
        amcmc = {"n.batch": 4, "batch.length": 10, "accept.rate": 0.43}
        fit = mk.spMvGLM(formula, d["coords"], np.ones((n, q)), starting, tuning, priors, amcmc, cov_model=c["cov"], seed=SEED)
        _fits[name] = dict(fit=fit, ses=fit["_session"], d=d, q=q, p=p, ct=ct, xt=xt, wts=wts, matern=c["cov"] == "matern",
                           offsets=np.concatenate([[0], np.cumsum(c["sizes"])]))
    return _fits[name]


def _replay(f, ct, xt, offsets, wts, thr=THR):
    """The one replay of the window with regions attached: (regions' dict, p_pred_samples)."""
    ses = f["ses"]
    ses.set_test_sites(ct, x_test=xt)
    ses.set_kept_window(FIRST, LAST)
    ses.set_regions(offsets, wts, thr)
    out = ses.outputs(quantiles=False, p_pred_samples=True)
    return ses.regions(samples=True), out["p_pred_samples"][0]


def _reference(f, ct, xt, offsets, wts):
    ref = RegionRef(f["d"]["coords"], ct, offsets, wts, matern=f["matern"])
    return ref, ref.window(f["fit"]["p.beta.theta.samples"], f["fit"]["p.w.samples"], f["q"], f["p"], SEED, 0, FIRST, LAST, xt)


def _base(mk, name):
    f = _fit(mk, name)
    if "dev" not in f:
        f["dev"], f["p_marg"] = _replay(f, f["ct"], f["xt"], f["offsets"], f["wts"])
        f["stats"] = f["ses"].kernel_stats(KS_REGIONS)
        f["ref_obj"], f["ref"] = _reference(f, f["ct"], f["xt"], f["offsets"], f["wts"])
    return f


def _close(dev, ref, what=""):
    dev, ref = np.asarray(dev, float), np.asarray(ref, float)
    assert dev.shape == ref.shape, what
    same = (dev == ref) | (np.isnan(dev) & np.isnan(ref))
    with np.errstate(invalid="ignore"):
        ok = same | (np.abs(dev - ref) <= RTOL * np.abs(ref) + ATOL)
    assert ok.all(), (what, dev[~ok], ref[~ok])


@pytest.mark.parametrize("name", ["lmc", "mat"])
def test_parity_with_the_restatement(mk, name):
    """Tests 1 and 5 of the issue: the regional draws against the restatement, under its cond(S) guard."""
    f = _base(mk, name)
    q, G = f["q"], len(f["offsets"]) - 1
    cond = f["ref"]["cond"]
    print(f"{name}: largest cond(S) over (state, region, outcome) {cond.max():.3e}")
    assert cond.shape == (N_WIN, G, q) and (cond <= COND_MAX).all(), "the draw bar does not cover these inputs"
    dev = f["dev"]["region_samples"][0]
    assert dev.shape == f["ref"]["draws"].shape == (G * q, N_WIN)
    err = np.abs(dev - f["ref"]["draws"])
    print(f"{name}: largest |device - restatement| per region column {err.max(axis=1)}")
    assert np.isfinite(dev).all() and (err <= DRAW_ATOL).all()
    assert (f["dev"]["singular"][0] == 0).all() and (f["ref"]["singular"] == 0).all()
    assert f["stats"]["launches"] == 2 * N_WIN + 2 and f["stats"]["ms"] > 0.0      # two kernels per state, two per replay
    t = f["dev"]["timing_ms"]
    assert (t > 0.0).all() and t.sum() == pytest.approx(f["stats"]["ms"], rel=1e-6)


def test_grids_and_planes_of_the_returned_draws(mk):
    f = _base(mk, "lmc")
    dev = f["dev"]
    draws = dev["region_samples"][0]
    assert dev["names"] == ["mean", "sd", "exc_1", "exc_2", "exc_3"] and dev["thresholds"] == list(THR)
    assert np.array_equal(dev["region_predict"][0], grids(draws))
    ref = planes(draws, THR)
    got = dev["subsets"][0]
    assert got.shape == ref.shape == (draws.shape[0], 2 + len(THR))
    print("largest plane differences", np.abs(got - ref).max(axis=0))
    _close(got[:, :2], ref[:, :2], "mean, sd")
    assert np.array_equal(got[:, 2:], ref[:, 2:])
    assert (got[:, 1] > 0).all()


def test_one_site_regions_are_the_marginal_draws(mk):
    f = _base(mk, "lmc")
    n_test = f["ct"].shape[0]
    one_minus_s = 1.0 - f["ref"]["s"]
    print(f"smallest 1 - s over states, sites and outcomes: {one_minus_s.min():.3e}")
    assert (one_minus_s >= 1e-3).all(), "the one-site bar does not cover these sites"
    got, p_marg = _replay(f, f["ct"], f["xt"], np.arange(n_test + 1), None, ())
    dev = got["region_samples"][0]
    assert dev.shape == p_marg.shape == (n_test * f["q"], N_WIN)
    err = np.abs(dev - p_marg)
    print(f"largest |one-site region - p_pred_samples| {err.max():.3e}")
    assert (err <= ONE_SITE_ATOL).all()
    assert got["subsets"][0].shape == (n_test * f["q"], 2) and (got["singular"][0] == 0).all()


def test_a_region_site_on_an_observed_site_is_flagged(mk):
    f = _base(mk, "lmc")
    q = f["q"]
    ct = f["ct"].copy()
    ct[18 + 40] = f["d"]["coords"][17]                           # site 40 of the 128-site region (region 2)
    got, _p = _replay(f, ct, f["xt"], f["offsets"], f["wts"])
    _ref_obj, ref = _reference(f, ct, f["xt"], f["offsets"], f["wts"])
    want = np.zeros(4 * q, dtype=np.int64)
    want[2 * q:3 * q] = N_WIN
    assert np.array_equal(ref["singular"], want)
    assert np.array_equal(got["singular"][0], want)
    dev = got["region_samples"][0]
    err = np.abs(dev - ref["draws"])
    print(f"flagged factors: largest |device - restatement| {err.max():.3e}")
    assert np.isfinite(dev).all() and np.isfinite(got["subsets"][0]).all() and np.isfinite(got["region_predict"][0]).all()
    assert (err <= DRAW_ATOL).all()


def test_joint_draws_are_wider_than_averaged_marginals(mk):
    """The point of the feature: the 128-site region's sd exceeds the sd of the same weighted average of the
    marginal p draws, which treats the sites' kriging errors as independent.  Both match their restatements."""
    f = _base(mk, "lmc")
    q = f["q"]
    a, b = int(f["offsets"][2]), int(f["offsets"][3])
    omega = f["ref_obj"].omega[a:b]
    assert np.abs(f["p_marg"] - f["ref"]["p_marginal"]).max() <= DRAW_ATOL
    for h in range(q):
        col = 2 * q + h
        avg_dev = omega @ f["p_marg"][a * q + h:b * q:q]
        avg_ref = omega @ f["ref"]["p_marginal"][a * q + h:b * q:q]
        sd_joint, sd_marg = f["dev"]["subsets"][0][col, 1], np.std(avg_dev, ddof=1)
        sd_joint_ref, sd_marg_ref = np.std(f["ref"]["draws"][col], ddof=1), np.std(avg_ref, ddof=1)
        print(f"outcome {h}: region.sd {sd_joint:.6f} (restatement {sd_joint_ref:.6f}), averaged marginals "
              f"{sd_marg:.6f} ({sd_marg_ref:.6f})")
        assert abs(sd_joint - sd_joint_ref) <= DRAW_ATOL and abs(sd_marg - sd_marg_ref) <= DRAW_ATOL
        assert sd_joint > sd_marg


def test_spregions_sorts_by_label(mk):
    """spRegions on the sites dealt round-robin over the regions (within a label the order is kept, so the stable
    sort restores the session's order): the session route's numbers, bit for bit, under the labels."""
    f = _base(mk, "lmc")
    q, off = f["q"], f["offsets"]
    n_test = f["ct"].shape[0]
    lab_sorted = np.repeat([7, 3, 11, 5], np.diff(off))          # region g's label; sorted by label: 3, 5, 7, 11
    rank = np.concatenate([np.arange(m) for m in np.diff(off)])
    perm = np.argsort(rank, kind="stable")
    rows = (perm[:, None] * q + np.arange(q)[None, :]).reshape(-1)
    res = mk.spRegions(f["fit"], f["ct"][perm], f["xt"][rows], lab_sorted[perm], weights=f["wts"][perm], thresholds=THR,
                       start=FIRST, end=LAST, samples=True)
    assert res["region.labels"] == [3, 5, 7, 11]
    order = [1, 3, 0, 2]                                         # the session's region of each sorted label
    # the sorted regions are other runs of the test sites, so other global site indices: compare through a
    # session replay of exactly that arrangement
    srt = np.argsort(lab_sorted, kind="stable")
    srows = (srt[:, None] * q + np.arange(q)[None, :]).reshape(-1)
    sizes = np.diff(off)[order]
    got, _p = _replay(f, f["ct"][srt], f["xt"][srows], np.concatenate([[0], np.cumsum(sizes)]), f["wts"][srt])
    assert np.array_equal(res["region.samples"], got["region_samples"][0])
    assert np.array_equal(res["region.predict"], got["region_predict"][0])
    assert np.array_equal(res["region.mean"], got["subsets"][0][:, 0]) and np.array_equal(res["region.sd"], got["subsets"][0][:, 1])
    assert np.array_equal(res["region.exceed"], got["subsets"][0][:, 2:]) and res["region.exceed"].shape == (4 * q, len(THR))
    assert (res["region.singular"] == 0).all() and res["thresholds"] == list(THR)
    with pytest.raises(ValueError):
        mk.spRegions(f["fit"], f["ct"], f["xt"], np.zeros(n_test - 1, dtype=int))
    with pytest.raises(mk.MkError) as e:                         # one label for all 179 sites: above 128
        mk.spRegions(f["fit"], f["ct"], f["xt"], np.zeros(n_test, dtype=int))
    assert "region 0 has 179 sites" in str(e.value)


def _two_subsets(mk):
    d = mk.synthetic.generate(290, q=2, n_test=1, seed=21)
    subs = []
    for a, b in ((0, 150), (150, 290)):
        subs.append(dict(coords=d["coords"][a:b], y=d["y"][2 * a:2 * b], weights=np.ones(2 * (b - a)), x=d["x"][2 * a:2 * b]))
    cfg = mk.SamplerConfig(2, 4, beta_starting=np.zeros(4), beta_tuning=np.full(4, 0.05), n_batch=4, batch_length=10,
                           burn_in=1, seed=SEED, predict_tile=256, phi_unif=(np.full(2, 4.0), np.full(2, 12.0)))
    rng = np.random.default_rng(77)
    ct = _grid_sites(40, 0.03, rng)
    xt = mk.synthetic.block_design(rng.standard_normal((40, 2)), 2)
    return subs, cfg, ct, xt, rng.uniform(0.5, 3.0, size=40)


def _session_regions(mk, subs, cfg, base, ct, xt, wts, offsets):
    with mk.Session(subs, cfg, subset_base=base) as ses:
        ses.run(cfg.n_samples)
        ses.set_test_sites(ct, x_test=xt)
        ses.set_kept_window(FIRST, LAST)
        ses.set_regions(offsets, wts, THR)
        ses.outputs(quantiles=False, w_predict_sum=True)
        got = ses.regions(samples=True)
        ses.set_kept_window(FIRST + 4, LAST)                     # another window, no replay: the buffers are stale
        with pytest.raises(mk.MkError) as e:
            ses.regions()
        assert e.value.code == mk._lib.MK_E_ARG
        assert "areal prediction: tile 0" in str(e.value) and "has not been replayed over this kept window" in str(e.value)
    return got


def test_subsets_do_not_depend_on_the_shard(mk):
    subs, cfg, ct, xt, wts = _two_subsets(mk)
    offsets = [0, 1, 13, 40]
    both = _session_regions(mk, subs, cfg, 0, ct, xt, wts, offsets)
    for i in range(2):
        alone = _session_regions(mk, [subs[i]], cfg, i, ct, xt, wts, offsets)
        for k in ("region_samples", "region_predict", "subsets", "singular"):
            assert np.array_equal(both[k][i], alone[k][0]), (i, k)
    assert not np.array_equal(both["region_samples"][0], both["region_samples"][1])


def _free_bytes(mk):
    f, t = ctypes.c_int64(), ctypes.c_int64()
    mk._lib.check(mk.load().mk_device_memory(0, ctypes.byref(f), ctypes.byref(t)))
    return f.value


def test_refusals_detach_and_off_costs_nothing(mk):
    subs, cfg, ct, xt, wts = _two_subsets(mk)
    subs = subs[:1]
    E = mk._lib.MK_E_ARG

    def refused(ses, what, *a, **kw):
        with pytest.raises(mk.MkError) as e:
            ses.set_regions(*a, **kw)
        assert e.value.code == E and what in str(e.value), str(e.value)

    with mk.Session(subs, cfg) as ses:
        ses.run(cfg.n_samples)
        refused(ses, "needs test sites", [0, 1])
        ses.set_test_sites(ct)
        refused(ses, "needs x_test", [0, 40])
        ses.set_test_sites(ct, x_test=xt)
        ses.set_kept_window(FIRST, LAST)
        plain = ses.outputs(quantiles=True, w_pred_samples=True, p_pred_samples=True)
        assert ses.kernel_stats(KS_REGIONS) == dict(launches=0, ms=0.0, flops=0.0)
        with pytest.raises(mk.MkError) as e:
            ses.regions()
        assert "no areal prediction asked for" in str(e.value)
        refused(ses, "offsets[0] = 2 must be 0", [2, 40])
        refused(ses, "offsets[2] = 10 is not above offsets[1] = 10", [0, 10, 10, 40])
        refused(ses, "offsets[2] = 39 must be n_test = 40", [0, 10, 39])
        refused(ses, "offsets[2] = 41 is past the 40 test sites", [0, 10, 41])
        bad = wts.copy()
        bad[7] = np.nan
        refused(ses, "weight 7 is", [0, 40], bad)
        bad[7] = -0.5
        refused(ses, "weight 7 is -0.5", [0, 40], bad)
        zero = wts.copy()
        zero[10:13] = 0.0
        refused(ses, "the weights of region 1 sum to 0", [0, 10, 13, 40], zero)
        refused(ses, "threshold 1 is", [0, 40], wts, (0.2, np.inf))
        refused(ses, "n_thresholds = 9", [0, 40], wts, np.linspace(0.1, 0.9, 9))
        free0 = _free_bytes(mk)
        # attach, replay, detach: the buffers come and go, and the replays without regions give the same bits
        ses.set_regions([0, 1, 13, 40], wts, THR)
        with pytest.raises(mk.MkError) as e:                     # attached, not replayed yet
            ses.regions()
        assert "has not been replayed" in str(e.value)
        assert ses.kernel_stats(KS_REGIONS)["launches"] == 0
        ses.outputs(quantiles=False, w_predict_sum=True)
        assert ses.kernel_stats(KS_REGIONS)["launches"] == 2 * N_WIN + 2
        assert ses.regions()["subsets"][0].shape == (6, 2 + len(THR))
        ses.set_regions(None)
        assert abs(_free_bytes(mk) - free0) <= (2 << 20)
        with pytest.raises(mk.MkError):
            ses.regions()
        again = ses.outputs(quantiles=True, w_pred_samples=True, p_pred_samples=True)
        assert ses.kernel_stats(KS_REGIONS)["launches"] == 2 * N_WIN + 2      # nothing more
        for k in ("w_predict", "p_predict", "w_pred_samples", "p_pred_samples", "parameters"):
            assert np.array_equal(plain[k][0], again[k][0]), k
        # two sites of one region at the same place; in different regions they are fine
        dup = ct.copy()
        dup[20] = dup[15]
        ses.set_test_sites(dup, x_test=xt)
        refused(ses, "test sites 15 and 20 of region 2 have identical coordinates", [0, 1, 13, 40], wts)
        ses.set_regions([0, 1, 13, 18, 40], wts)
        ses.set_test_sites(ct, x_test=xt)                        # new sites detach
        with pytest.raises(mk.MkError) as e:
            ses.regions()
        assert "no areal prediction asked for" in str(e.value)
        # a region above 128 sites, and more sites than the tile
        rng = np.random.default_rng(3)
        many = rng.uniform(size=(200, 2))
        xm = mk.synthetic.block_design(rng.standard_normal((200, 2)), 2)
        ses.set_test_sites(many, x_test=xm)
        refused(ses, "region 0 has 129 sites", [0, 129, 200])
        more = rng.uniform(size=(300, 2))
        ses.set_test_sites(more, x_test=mk.synthetic.block_design(rng.standard_normal((300, 2)), 2))
        assert ses.predict_tile == 256
        refused(ses, "exceed the session's tile of 256", [0, 100, 200, 300])
    # a session that keeps no chain states: the message names the remedy
    fused = mk.SamplerConfig(2, 4, beta_starting=np.zeros(4), beta_tuning=np.full(4, 0.05), n_batch=1, batch_length=4,
                             burn_in=2, seed=SEED)
    with mk.Session(subs, fused, coords_test=ct, x_test=xt) as ses:
        refused(ses, "predict_tile > 0", [0, 40])
        assert "predict_tile >= the number of test sites" in mk.load().mk_last_error().decode()


def test_meta_fit_regions_and_their_combine(mk):
    d = mk.synthetic.generate(120, q=1, n_test=12, seed=31)
    idx = [np.arange(0, 60), np.arange(60, 120)]
    kw = dict(beta_starting=np.zeros(2), beta_tuning=np.full(2, 0.05), n_batch=2, batch_length=8, seed=SEED)
    cfg = mk.SamplerConfig(1, 2, predict_tile=256, **kw)
    spec = dict(offsets=[0, 5, 12], weights=np.arange(1.0, 13.0), thresholds=(0.4,))
    obj = mk.meta_fit(d["y"], d["x"], 1, d["coords"], 1, idx, coords_test=d["coords_test"], cfg=cfg, x_test=d["x_test"],
                      regions=spec)
    assert len(obj) == 2
    for o in obj:
        assert o["region.predict"].shape == (200, 2) and o["regions"].shape == (2, 3)
        assert o["regions.names"] == ["mean", "sd", "exc_1"] and o["regions.singular"].tolist() == [0, 0]
        assert o["w.predict"].shape == (200, 12) and o["p.predict"].shape == (200, 12)
        assert (o["regions"][:, 0] > 0).all() and (o["regions"][:, 0] < 1).all()
    for method in ("mean", "median"):
        comb = mk.combine_regions(obj, method=method)
        want = mk.metakriging.combiner(method)([o["region.predict"] for o in obj])
        assert np.array_equal(comb["region.predict"], want)
        assert np.array_equal(comb["planes"], mk.map_grid(want, (0.4,))["planes"]) and comb["names"] == ["mean", "sd", "exc_1"]
    with pytest.raises(mk.MkError):                               # predict_tile = 0: the session's error surfaces
        mk.meta_fit(d["y"], d["x"], 1, d["coords"], 1, idx, coords_test=d["coords_test"], cfg=mk.SamplerConfig(1, 2, **kw),
                    x_test=d["x_test"], regions=spec)
