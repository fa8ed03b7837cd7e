"""Model assessment on the device (include/mk.h: DIC as spDiag names its rows, and WAIC, per subset)
against its NumPy restatement tests/crit_ref.py, on the sessions' own recorded chains.

Bars.  bar.D, D.bar.Omega, DIC, lppd, WAIC and lconst: rtol 1e-9, the standing bar for a device
reduction against a NumPy restatement (sums of <= 600 terms of one sign and 48 states carry ~1e-13).
pD and p.waic are differences of nearly equal sums, so their bars are absolute: 1e-9 |bar.D| and
1e-9 |lppd|; the pointwise pairs use the same bars per entry.  In-chain against replay, stream groups,
tiling and the node driver against one session: bit equality -- every sum's order depends on the
window's length and n_pad q alone.  Sessions compared bit for bit run the same launch schedule
(the lookahead and the sequential chains agree only to rounding, by design).

Shapes: 64 iterations (n_batch 4 x batch_length 16), burn_in 17: 48 kept.  "exp": exponential, logit,
q = 1, subsets of 100 and 257 sites with 3 trials each (n_pad 384: observation blocks of 256 + 128,
the second partly padding; lconst > 0).  "mat": Matern, probit, q = 2, subsets of 129 and 150 sites
(Np 512 with 258 / 300 valid rows: a block boundary inside the valid range, padding after)."""
import ctypes

import numpy as np
import pytest

from crit_ref import NAMES, crit_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-9
N_TEST = 8
KW = dict(n_batch=4, batch_length=16, burn_in=17, seed=9)
KS_CRIT = 15
_CASES = {"exp": dict(sizes=[100, 257], q=1, cov="exponential", link="logit", trials=3.0),
          "mat": dict(sizes=[129, 150], q=2, cov="matern", link="probit", trials=1.0)}
_runs = {}


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


def _ref(r, s, samples, w_samples, window, thin=1):
    sub = r["subs"][s]
    return crit_ref(samples, w_samples, sub["y"], sub["weights"], sub["x"], 2 * r["q"], r["link"], window, thin)


def _run(mk, name):
    """One fit per case with in-chain criteria and the chain recorded, every criteria() call the tests
    read made once, in a fixed order; shared and left unchanged."""
    if name not in _runs:
        c = _CASES[name]
        d, subs = _problem(mk, c["sizes"], c["q"], trials=c["trials"], cov=c["cov"])
        cfg = _cfg(mk, c["q"], c["cov"], c["link"])
        r = dict(d=d, subs=subs, q=c["q"], link=c["link"], cfg=cfg)
        with mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"], record_w=True, criteria=True) as ses:
            ses.run(64)
            r["launches"] = ses.kernel_stats(KS_CRIT)
            r["in_chain"] = ses.criteria(pointwise=True)
            r["after"] = ses.kernel_stats(KS_CRIT)
            r["out"] = ses.outputs(samples=True, w_samples=True, w_pred_samples=True)
            ses.set_kept_window(17, 64)
            r["replay"] = ses.criteria(pointwise=True)
            ses.set_kept_window(20, 60)
            r["thin3"] = ses.criteria(thin=3, pointwise=True)
            ses.set_kept_window(30, 31)
            r["two"] = ses.criteria(pointwise=True)
            ses.set_kept_window(40, 40)
            with pytest.raises(mk.MkError) as e:
                ses.criteria()
            r["one_state"] = e.value
            ses.set_kept_window(20, 60)
            with pytest.raises(mk.MkError) as e:
                ses.criteria(thin=41)               # one state of 41
            r["one_state_thin"] = e.value
        _runs[name] = r
    return _runs[name]


def _check(got, r, window, thin=1, samples=None, w_samples=None):
    """got (Session.criteria's dict, with pointwise) against the restatement on the recorded chain."""
    n_sub = len(r["subs"])
    assert got["names"] == NAMES and got["subsets"].shape == (n_sub, 8) and got["total"].shape == (8,)
    for s in range(n_sub):
        smp = r["out"]["samples"][s] if samples is None else samples[s]
        wsm = r["out"]["w_samples"][s] if w_samples is None else w_samples[s]
        ref, pw = _ref(r, s, smp, wsm, window, thin)
        dev, dpw = got["subsets"][s], got["pointwise"][s]
        print(f"subset {s} window {window} thin {thin}:")
        for k, nm in enumerate(NAMES):
            print(f"  {nm:12s} device {dev[k]: .15e}  restatement {ref[k]: .15e}  difference {dev[k] - ref[k]: .2e}")
        print(f"  pointwise: lppd_i largest relative difference {np.abs(dpw[:, 0] / pw[:, 0] - 1).max():.2e}, "
              f"variance largest difference {np.abs(dpw[:, 1] - pw[:, 1]).max():.2e}")
        assert np.isfinite(dev).all()
        for k in (0, 1, 3, 4, 6, 7):
            np.testing.assert_allclose(dev[k], ref[k], rtol=RTOL, atol=0, err_msg=NAMES[k])
        assert abs(dev[2] - ref[2]) <= RTOL * abs(ref[0]), "pD"
        assert abs(dev[5] - ref[5]) <= RTOL * abs(ref[4]), "p.waic"
        assert dpw.shape == pw.shape
        np.testing.assert_allclose(dpw[:, 0], pw[:, 0], rtol=RTOL, atol=0)
        assert (np.abs(dpw[:, 1] - pw[:, 1]) <= RTOL * np.abs(pw[:, 0])).all()
    tot = got["subsets"][0].copy()
    for s in range(1, n_sub):
        tot = tot + got["subsets"][s]
    assert np.array_equal(got["total"], tot)            # the subset-order sum


def _same(a, b):
    assert np.array_equal(a["subsets"], b["subsets"]) and np.array_equal(a["total"], b["total"])
    if "pointwise" in a and "pointwise" in b:
        for x, y in zip(a["pointwise"], b["pointwise"]):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("name", list(_CASES))
def test_against_restatement(mk, name):
    r = _run(mk, name)
    if name == "exp":
        assert (r["in_chain"]["subsets"][:, 7] > 0).all()      # three trials: the dropped constant is there
    _check(r["in_chain"], r, (17, 64))


@pytest.mark.parametrize("name", list(_CASES))
def test_in_chain_equals_replay(mk, name):
    r = _run(mk, name)
    _same(r["in_chain"], r["replay"])


@pytest.mark.parametrize("name", list(_CASES))
def test_window_and_thin(mk, name):
    """Rows 20, 23, ..., 59 of the window 20..60 (14 states); a window of two states; one state is an
    argument error, from the window or from thin."""
    r = _run(mk, name)
    _check(r["thin3"], r, (20, 60), thin=3)
    _check(r["two"], r, (30, 31))
    for e in (r["one_state"], r["one_state_thin"]):
        assert e.code == mk._lib.MK_E_ARG and "2 states" in str(e)


def test_does_not_touch_the_chain_and_off_costs_nothing(mk):
    """A plain session makes the same samples, kriging draws and grids bit for bit, and no criteria
    launch (kernel-stats kind 15); the other made one per kept iteration, then two to close them."""
    r = _run(mk, "exp")
    d = r["d"]
    with mk.Session(r["subs"], r["cfg"], coords_test=d["coords_test"], x_test=d["x_test"], record_w=True) as ses:
        ses.run(64)
        plain = ses.outputs(samples=True, w_samples=True, w_pred_samples=True)
        stats = ses.kernel_stats(KS_CRIT)
    assert stats["launches"] == 0 and stats["ms"] == 0.0
    assert r["launches"]["launches"] == 48 and r["launches"]["ms"] > 0.0
    assert r["after"]["launches"] == 50
    assert set(plain) == set(r["out"])
    for f, v in plain.items():
        for s in range(2):
            assert np.array_equal(r["out"][f][s], v[s]), f


@pytest.mark.parametrize("name", list(_CASES))
def test_stream_groups_and_tiling(mk, name):
    """Sequential schedule throughout (stream groups and the lookahead exclude each other): one stream
    fused, two stream groups, and kriging tiled after the fit give the same rows bit for bit, and the
    sequential chain's rows meet the restatement too."""
    r = _run(mk, name)
    c, d = _CASES[name], r["d"]
    got = {}
    for key, kw in (("one", {}), ("groups", dict(n_streams=2)), ("tiled", dict(predict_tile=4))):
        cfg = _cfg(mk, c["q"], c["cov"], c["link"], **kw)
        with mk.Session(r["subs"], cfg, coords_test=d["coords_test"], x_test=d["x_test"], record_w=True, criteria=True,
                        lookahead=False) as ses:
            ses.run(64)
            assert not ses.lookahead
            assert ses.predict_tile == (4 if key == "tiled" else 0)
            got[key] = ses.criteria(pointwise=True)
            if key == "one":
                chain = ses.outputs(quantiles=False, samples=True, w_samples=True)
            if key == "groups":
                assert ses.kernel_stats(KS_CRIT)["launches"] == 2 * 48 + 2      # one launch per group and kept state
    _check(got["one"], r, (17, 64), samples=chain["samples"], w_samples=chain["w_samples"])
    _same(got["one"], got["groups"])
    _same(got["one"], got["tiled"])


def test_node_equals_one_session(mk):
    """Four q = 1 subsets over two blocks of one device: the rows, the pointwise pairs and the totals of
    one session, bit for bit; the totals are the subset-order sum of the rows."""
    d, subs = _problem(mk, [150, 163, 140, 129], 1, seed=4)
    cfg = _cfg(mk, 1)
    with mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"], criteria=True) as ses:
        ses.run(64)
        one = ses.criteria(pointwise=True)
    got = mk.meta_fit_node(subs, cfg, coords_test=d["coords_test"], devices=(0, 0), x_test=d["x_test"],
                           criteria="pointwise")
    _same(got["criteria"], one)
    assert [a.shape for a in got["criteria"]["pointwise"]] == [(150, 2), (163, 2), (140, 2), (129, 2)]
    tot = one["subsets"][0].copy()
    for s in range(1, 4):
        tot = tot + one["subsets"][s]
    assert np.array_equal(got["criteria"]["total"], tot) and np.isfinite(tot).all()
    plain = mk.meta_fit_node(subs, cfg, coords_test=d["coords_test"], devices=(0, 0), x_test=d["x_test"])
    assert "criteria" not in plain and np.array_equal(plain["result"], got["result"])
    assert np.array_equal(plain["result2"], got["result2"])


def test_spbayes_surface(mk):
    """spDiag(fit, start, end, thin) is the restatement on the fit's own p.beta.theta.samples and
    p.w.samples; a closed fit and an invalid window raise spBayes-style errors."""
    n = 80
    d = mk.synthetic.generate(n, q=1, n_test=N_TEST, seed=31)
    starting = {"beta": np.zeros(2), "phi": 3 / 0.5, "A": np.ones(1), "w": 0.0}
    tuning = {"beta": np.full(2, 0.05), "phi": 1.0, "A": 0.1, "w": 0.5}
    priors = {"phi.Unif": (3 / 0.75, 3 / 0.25), "K.IW": (1, 0.1 * np.eye(1))}
    amcmc = {"n.batch": 4, "batch.length": 16, "accept.rate": 0.43}
    with mk.spMvGLM([(d["y"], d["x"])], d["coords"], np.ones((n, 1)), starting, tuning, priors, amcmc, seed=9) as fit:
        whole = mk.spDiag(fit, start=17, end=64)
        thinned = mk.spDiag(fit, start=17, end=64, thin=2)
        for bad in (dict(start=0), dict(start=10, end=9), dict(end=65), dict(thin=0)):
            with pytest.raises(ValueError):
                mk.spDiag(fit, **bad)
    with pytest.raises(ValueError):
        mk.spDiag(fit)                                   # closed
    for got, thin in ((whole, 1), (thinned, 2)):
        assert list(got) == ["DIC", "WAIC"] and list(got["DIC"]) == NAMES[:4] and list(got["WAIC"]) == NAMES[4:]
        dev = np.array([got["DIC"][k] for k in NAMES[:4]] + [got["WAIC"][k] for k in NAMES[4:]])
        ref, _ = crit_ref(fit["p.beta.theta.samples"], fit["p.w.samples"], d["y"], np.ones(n), d["x"], 2, "logit",
                          (17, 64), thin)
        print(f"thin {thin}: device {dev}\n        restatement {ref}")
        for k in (0, 1, 3, 4, 6, 7):
            np.testing.assert_allclose(dev[k], ref[k], rtol=RTOL, atol=0, err_msg=NAMES[k])
        assert abs(dev[2] - ref[2]) <= RTOL * abs(ref[0]) and abs(dev[5] - ref[5]) <= RTOL * abs(ref[4])


def test_reference_flow_and_meta_fit_carry_the_rows(mk):
    """reference_flow(criteria=True) puts the totals into the summary by name; meta_fit(criteria=True)
    puts each subset's rows on its dict.  Per subset DIC = bar.D + pD and WAIC = -2 (lppd - p.waic) hold
    exactly (the device forms them so); p.waic is positive once any latent value has moved."""
    d = mk.synthetic.generate(300, q=1, n_test=N_TEST, seed=12)
    # two blocks on one device: the device-copy exchange (an RCCL communicator takes seconds to create)
    ph, result, result2, summ, cfg = mk.metakriging.reference_flow(d, 2, 1, n_batch=4, batch_length=16, devices=(0, 0),
                                                                   samplesize=50, criteria=True)
    assert list(summ["criteria"]) == NAMES and np.isfinite(list(summ["criteria"].values())).all()
    _, index_part = mk.partition(300, 2, seed=20250114, method="R")      # reference_flow's own partition
    obj = mk.meta_fit(d["y"], d["x"], 1.0, d["coords"], 1, index_part, coords_test=d["coords_test"], cfg=cfg,
                      criteria=True)
    assert "criteria" not in mk.meta_fit(d["y"], d["x"], 1.0, d["coords"], 1, index_part[:1],
                                         coords_test=d["coords_test"], cfg=cfg)[0]
    tot = None
    for o in obj:
        c = o["criteria"]
        assert list(c) == NAMES
        assert c["DIC"] == c["bar.D"] + c["pD"] and c["WAIC"] == -2.0 * (c["lppd"] - c["p.waic"])
        assert c["p.waic"] > 0 and c["lconst"] == 0.0
        row = np.array([c[k] for k in NAMES])
        tot = row if tot is None else tot + row
    assert np.array_equal(tot, np.array([summ["criteria"][k] for k in NAMES]))      # the same chains, summed in order


def test_errors(mk):
    """Neither route available: the message names record_w.  In-chain criteria cannot be switched on
    once the chain has started."""
    r = _run(mk, "exp")
    d = r["d"]
    lib = mk.load()
    with mk.Session(r["subs"][:1], r["cfg"], coords_test=d["coords_test"]) as ses:
        ses.run(16)
        assert lib.mk_session_set_criteria(ses._h, 1) == mk._lib.MK_E_ARG
        with pytest.raises(mk.MkError) as e:
            ses.criteria()                               # the chain has not finished
        assert e.value.code == mk._lib.MK_E_ARG
        ses.run(48)
        with pytest.raises(mk.MkError) as e:
            ses.criteria()
        assert e.value.code == mk._lib.MK_E_ARG and "record_w" in str(e.value)
        cb = mk._lib.Criteria()
        assert lib.mk_session_criteria(ses._h, 0, ctypes.byref(cb)) == mk._lib.MK_E_ARG      # thin < 1
    # in-chain sums without a recorded chain close, but cannot serve a thin or a window
    with mk.Session(r["subs"][:1], r["cfg"], criteria=True) as ses:
        ses.run(64)
        got = ses.criteria()
        assert got["subsets"].shape == (1, 8) and np.isfinite(got["subsets"]).all()
        with pytest.raises(mk.MkError) as e:
            ses.criteria(thin=2)
        assert e.value.code == mk._lib.MK_E_ARG and "record_w" in str(e.value)
