"""Sessions from a recorded chain (include/mk.h "sessions from a recorded chain"; csrc/mk_import.hip): a session that
never ran imports samples and w_samples and then serves the kriging replay and every sink.

The bars are derived, none is measured: tests/krig_ref.py's hard and comparative bars of the kriging draws against
its 80-bit reference (tests/test_gpu_krig_parity.py's), |imported - live| <= 2 hard (both are within hard of the
same reference), the standing 1e-8 of a device chain against the CPU oracle (tests/test_gpu_sampler.py), the 1e-9
bars of the sinks against their NumPy restatements (tests/test_gpu_maps.py, tests/test_gpu_criteria.py), and byte
equality wherever the same arithmetic runs twice.

Chains: 4 batches x 10 iterations, burn_in = 21 (20 kept states) unless said; the exact replay (MK_KRIG_CHEB=0)
unless said; tile 256 under krig_ref's 261 test sites, so every session is tiled."""
import numpy as np
import pytest

from oracle import philox
from oracle import spmvglm as om

import krig_ref as kr
from crit_ref import crit_ref
from maps_ref import map_ref, map_ref_p

pytestmark = pytest.mark.gpu

WIN = dict(n_batch=4, batch_length=10, burn_in=21)
SEED, BASE, TILE = 12, 2, 256
_live_runs = {}


def _cfg(mk, case, tile=TILE, **kw):
    c = kr.CASES[case]
    q = c["q"]
    win = dict(WIN, **kw)
    return mk.SamplerConfig(q, 2 * q, np.zeros(2 * q), np.full(2 * q, 0.05), cov_model=c["model"], seed=SEED, predict_tile=tile,
                            **win)


def _state_ref(case, pb, cfg, samples, w_samples, s, k, subs=None, base=BASE):
    """krig_ref.predict_state of subset s, kept state k, from recorded samples (n x P) and w ((n_s q) x n_w, the
    last n_w iterations)."""
    q, p = cfg.q, cfg.p
    ntri = q * (q + 1) // 2
    matern = kr.CASES[case]["model"] == "matern"
    subs = _subrefs(case, pb) if subs is None else subs
    it = cfg.burn_in - 1 + k
    row = samples[s][it]
    nu = row[p + ntri + q:p + ntri + 2 * q] if matern else np.zeros(q)
    w = w_samples[s][:, it - (cfg.n_samples - w_samples[s].shape[1])]
    return kr.predict_state(subs[s], row[p:p + ntri], row[p + ntri:p + ntri + q], nu, w, philox.make_key(cfg.seed, base + s), it)


_subref_cache = {}


def _subrefs(case, pb):
    if case not in _subref_cache:
        matern = kr.CASES[case]["model"] == "matern"
        _subref_cache[case] = [kr.SubsetRef(sb["coords"], pb["coords_test"], matern) for sb in pb["subsets"]]
    return _subref_cache[case]


def _live(mk, monkeypatch, case):
    """Session A of a case: the chain run here, its outputs, and the reference of the first, a middle and the
    last kept state of every subset from its recorded states; shared and left unchanged."""
    if case not in _live_runs:
        monkeypatch.setenv("MK_KRIG_CHEB", "0")
        pb = kr.problem(case)
        cfg = _cfg(mk, case)
        with mk.Session(pb["subsets"], cfg, coords_test=pb["coords_test"], subset_base=BASE, record_w=True) as ses:
            ses.run(cfg.n_samples)
            out = ses.outputs(samples=True, w_samples=True, w_pred_samples=True, acceptance=True)
            crit2 = ses.criteria(thin=2, pointwise=True)
        refs = {(s, k): _state_ref(case, pb, cfg, out["samples"], out["w_samples"], s, k)
                for s in range(len(pb["subsets"])) for k in (0, cfg.kept // 2, cfg.kept - 1)}
        _live_runs[case] = dict(pb=pb, cfg=cfg, out=out, refs=refs, crit2=crit2)
    return _live_runs[case]


def _import(mk, r, monkeypatch, cheb="0"):
    """Session B: created anew over the case's data, A's chain imported; its outputs."""
    monkeypatch.setenv("MK_KRIG_CHEB", cheb)
    pb, cfg, a = r["pb"], r["cfg"], r["out"]
    with mk.Session(pb["subsets"], cfg, coords_test=pb["coords_test"], subset_base=BASE, record_w=True) as ses:
        assert not ses.imported and ses.iteration == 0
        ses.import_chain(a["samples"], a["w_samples"], a["acceptance"])
        assert ses.imported and ses.iteration == cfg.n_samples
        out = ses.outputs(samples=True, w_samples=True, w_pred_samples=True)
        out["stats"] = ses.import_stats()
        out["cheb"] = ses.kernel_stats(mk.session.KS_KRIG_CHEB)
        out["fallback"] = ses.kernel_stats(mk.session.KS_KRIG_FALLBACK)
    return out


def _judge(tag, r, out, interpolated=False, against=None):
    """Every reference state of r against out's draws: krig_ref.judge's violations, its figures printed; with
    `against` (another session's outputs) also |out - against| <= 2 hard per site."""
    pb, cfg = r["pb"], r["cfg"]
    T, q = pb["coords_test"].shape[0], cfg.q
    bad, figs = [], []
    for (s, k), ref in r["refs"].items():
        dev = out["w_pred_samples"][s][:, k].reshape(T, q)
        b, f = kr.judge(dev, ref, interpolated=interpolated)
        bad += [f"subset {s} state {k}: {x}" for x in b]
        figs.append(f)
        if against is not None:
            d = np.max(np.abs(dev - against["w_pred_samples"][s][:, k].reshape(T, q)), axis=1)
            lim = 2.0 * (ref["hard"] + (ref["interp"] if interpolated else 0.0))
            f["pair"] = float(np.max(d / lim))
            for t in np.flatnonzero(~(d <= lim))[:4]:
                bad.append(f"subset {s} state {k} site {t}: |imported - live| {d[t]:.3e} > 2 hard = {lim[t]:.3e}")
    top = {key: max(f[key] for f in figs) for key in figs[0]}
    ratio = max(f["dev_regular"] / f["scale"] for f in figs)
    print(f"\nIMPORT {tag:<14} kappa {top['kappa']:.2e}  regular {top['dev_regular']:.2e} | lapack {top['lapack_regular']:.2e}  "
          f"singular {top['dev_singular']:.2e} | {top['lapack_singular']:.2e}  ratio {ratio:5.2f}  |dev - ref| / hard "
          f"{top['hard_slack']:.1e}" + (f"  |imported - live| / 2 hard {top['pair']:.1e}" if against is not None else ""))
    assert not bad, "\n".join(bad[:12] + [f"... {len(bad)} in all"])


# ---------------------------------------------------------------- 1. round trip against the derived bars
@pytest.mark.parametrize("case", ["E1", "L1", "M1"])
def test_round_trip_against_the_derived_bars(mk, monkeypatch, case):
    """Session A runs the chain, session B imports A's samples and w_samples: parameters, samples and w_samples
    are A's bytes; B's draws at the first, a middle and the last kept state of every subset pass krig_ref's hard
    and comparative bars and lie within 2 hard of A's."""
    r = _live(mk, monkeypatch, case)
    b = _import(mk, r, monkeypatch=monkeypatch)
    a = r["out"]
    for s in range(len(r["pb"]["subsets"])):
        assert b["parameters"][s].tobytes() == a["parameters"][s].tobytes(), s
        assert b["samples"][s].tobytes() == a["samples"][s].tobytes(), s
        assert b["w_samples"][s].tobytes() == a["w_samples"][s].tobytes(), s
        assert np.isfinite(b["w_pred_samples"][s]).all()
    assert b["cheb"]["launches"] == 0 and b["fallback"]["launches"] == 0
    _judge(f"{case} exact", r, b, against=a)


# ---------------------------------------------------------------- 2. the interpolated route
@pytest.mark.parametrize("case", ["E1", "L1"])
def test_interpolated_route(mk, monkeypatch, case):
    """The phi-interpolated replay (MK_KRIG_CHEB=-1, tile 256) of an imported session: its g pass reads the
    imported z.  Judged with the interpolation's term in the bars."""
    r = _live(mk, monkeypatch, case)
    b = _import(mk, r, cheb="-1", monkeypatch=monkeypatch)
    assert b["cheb"]["launches"] > 0 and b["fallback"]["launches"] == 0, (b["cheb"], b["fallback"])
    _judge(f"{case} interpolated", r, b, interpolated=True)


# ---------------------------------------------------------------- 3. the same bytes however it is done
def test_same_bytes_however_it_is_done(mk, monkeypatch):
    r = _live(mk, monkeypatch, "E1")
    pb, cfg, a = r["pb"], r["cfg"], r["out"]
    first = _import(mk, r, monkeypatch=monkeypatch)
    again = _import(mk, r, monkeypatch=monkeypatch)
    monkeypatch.setenv("MK_IMPORT_BATCH", "1")
    one = _import(mk, r, monkeypatch=monkeypatch)
    monkeypatch.setenv("MK_IMPORT_BATCH", "2")
    two = _import(mk, r, monkeypatch=monkeypatch)
    monkeypatch.delenv("MK_IMPORT_BATCH")
    for s in range(len(pb["subsets"])):
        assert again["w_pred_samples"][s].tobytes() == first["w_pred_samples"][s].tobytes(), s
        assert one["w_pred_samples"][s].tobytes() == first["w_pred_samples"][s].tobytes(), s
        assert two["w_pred_samples"][s].tobytes() == first["w_pred_samples"][s].tobytes(), s
    assert first["stats"]["factorisations"] == again["stats"]["factorisations"] == one["stats"]["factorisations"]
    for i, sb in enumerate(pb["subsets"]):                    # subset i alone, as its own shard
        with mk.Session([sb], cfg, coords_test=pb["coords_test"], subset_base=BASE + i) as ses:
            ses.import_chain([a["samples"][i]], [a["w_samples"][i][:, -cfg.kept:]])   # the kept columns alone
            alone = ses.outputs(quantiles=False, w_pred_samples=True)
        assert alone["w_pred_samples"][0].tobytes() == first["w_pred_samples"][i].tobytes(), i


# ---------------------------------------------------------------- 4. runs and batches on a hand-made chain
def test_runs_and_batches_on_a_hand_made_chain(mk, monkeypatch):
    """E1's data, 24 kept states: phi constant over 11 states (longer than any batch), then another at every
    state, then two states back at the first run's phi; w from NumPy's generator, K fixed.  Every state of the
    127- and 129-site subsets against krig_ref, and the factorisations counted: 13 runs per pair."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    pb = kr.problem("E1")
    cfg = _cfg(mk, "E1", burn_in=17)
    assert cfg.kept == 24
    rng = np.random.default_rng(77)
    n, P, p = cfg.n_samples, cfg.P, cfg.p
    samples, ws = [], []
    for s, sb in enumerate(pb["subsets"]):
        phi = np.concatenate([np.full(11, 5.0 + 0.3 * s), 6.0 + 0.45 * np.arange(11) + 0.01 * s, np.full(2, 5.0 + 0.3 * s)])
        sm = np.zeros((n, P))
        sm[:, :p] = 0.1 * rng.standard_normal((n, p))
        sm[:, p] = 1.3                                              # K
        sm[:, p + 1] = np.concatenate([np.full(n - 24, phi[0]), phi])
        samples.append(sm)
        ws.append(0.5 * rng.standard_normal((sb["coords"].shape[0], 24)))
    with mk.Session(pb["subsets"], cfg, coords_test=pb["coords_test"], subset_base=BASE) as ses:
        ses.import_chain(samples, ws)
        out = ses.outputs(quantiles=False, samples=True, w_pred_samples=True)
        stats = ses.import_stats()
        with pytest.raises(mk.MkError, match="w samples were not recorded"):
            ses.outputs(quantiles=False, w_samples=True)
    print(f"\nIMPORT hand-made: {stats}")
    assert stats["factorisations"] == 13 * len(pb["subsets"])
    T = pb["coords_test"].shape[0]
    subs = {s: kr.SubsetRef(pb["subsets"][s]["coords"], pb["coords_test"], False) for s in (0, 1)}
    bad, worst = [], 0.0
    for s in (0, 1):
        assert samples[s].tobytes() == out["samples"][s].tobytes()
        for k in range(24):
            ref = _state_ref("E1", pb, cfg, samples, ws, s, k, subs=subs)
            b, f = kr.judge(out["w_pred_samples"][s][:, k].reshape(T, 1), ref)
            bad += [f"subset {s} state {k}: {x}" for x in b]
            worst = max(worst, f["hard_slack"])
    print(f"IMPORT hand-made: largest |dev - ref| / hard {worst:.1e} over 48 states")
    assert not bad, "\n".join(bad[:12] + [f"... {len(bad)} in all"])


# ---------------------------------------------------------------- 5. a chain born on the CPU
def test_a_chain_born_on_the_cpu(mk, monkeypatch):
    """oracle.spmvglm.fit_subset's chain (n_s = 60, q = 2, 40 iterations) imported into a device session that
    never ran: the kriging draws agree with the oracle's to 1e-8 absolute."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    q, p, ns, n_test = 2, 4, 60, 12
    d = mk.synthetic.generate(ns, q=q, n_test=n_test, seed=31)
    kw = dict(n_batch=4, batch_length=10, burn_in=21, seed=9)
    sub = dict(coords=d["coords"], y=d["y"], weights=np.ones(ns * q), x=d["x"])
    ocfg = om.Config(q, p, beta_starting=np.zeros(p), beta_tuning=np.full(p, 0.05), **kw)
    ref = om.fit_subset(sub["coords"], sub["y"], sub["weights"], sub["x"], ocfg, subset=5, coords_test=d["coords_test"],
                        record_w=True)
    cfg = mk.SamplerConfig(q, p, np.zeros(p), np.full(p, 0.05), predict_tile=TILE, **kw)
    with mk.Session([sub], cfg, subset_base=5, record_w=True) as ses:
        ses.import_chain([ref["samples"]], [ref["w_samples"].T.copy()])
        ses.set_test_sites(d["coords_test"])
        out = ses.outputs(samples=True, w_samples=True, w_pred_samples=True)
    assert out["samples"][0].tobytes() == np.ascontiguousarray(ref["samples"]).tobytes()
    diff = np.abs(out["w_pred_samples"][0].T - ref["w_pred"])
    print(f"\nIMPORT oracle chain: largest |device - oracle| kriging draw {diff.max():.3e}")
    assert diff.max() <= 1e-8
    np.testing.assert_allclose(out["parameters"][0], ref["param_q"], rtol=0, atol=1e-8)


# ---------------------------------------------------------------- 6. the sinks are wired
def test_the_sinks_are_wired(mk, monkeypatch):
    """An imported L1 session with x_test: maps against maps_ref on its own draws (test_gpu_maps.py's bars),
    criteria(thin=2) against crit_ref at 1e-9 and against the live session's replay route, bit for bit
    (k_crit_replay recomputes eta from X, beta and w, which are the same bytes)."""
    r = _live(mk, monkeypatch, "L1")
    pb, cfg, a = r["pb"], r["cfg"], r["out"]
    T, q, p = pb["coords_test"].shape[0], cfg.q, cfg.p
    rng = np.random.default_rng(8)
    xt = np.zeros((T * q, p))
    xc = rng.standard_normal((T, q))
    for h in range(q):
        xt[h::q, 2 * h] = 1.0
        xt[h::q, 2 * h + 1] = xc[:, h]
    thr = (0.2, 0.5, 0.8, 0.3141592653589793)
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    with mk.Session(pb["subsets"], cfg, coords_test=pb["coords_test"], subset_base=BASE, record_w=True, x_test=xt) as ses:
        ses.import_chain(a["samples"], a["w_samples"])
        ses.set_maps(thr)
        out = ses.outputs(quantiles=False, samples=True, w_samples=True, w_pred_samples=True)
        maps = ses.maps()
        crit = ses.criteria(thin=2, pointwise=True)
        with pytest.raises(mk.MkError, match="in-chain criteria"):
            mk._lib.check(ses._lib.mk_session_set_criteria(ses._h, 1))
    for s, sb in enumerate(pb["subsets"]):
        ref = map_ref(out["samples"][s], out["w_pred_samples"][s], xt, p, "logit", thr, first=cfg.burn_in)
        pk = map_ref_p(out["samples"][s], out["w_pred_samples"][s], xt, p, "logit", first=cfg.burn_in)
        dev = maps["subsets"][s]
        gap = min(np.abs(pk - u).min() for u in thr)
        print(f"\nIMPORT maps subset {s}: largest difference {np.abs(dev - ref).max():.2e}, nearest p to a threshold {gap:.2e}")
        assert gap > 1e-9, "a restated p lies within the guard of a threshold: change the thresholds"
        assert (np.abs(dev[:, :4] - ref[:, :4]) <= 1e-9 * np.abs(ref[:, :4]) + 1e-12).all()
        assert np.array_equal(dev[:, 4:], ref[:, 4:])
        cref, pw = crit_ref(out["samples"][s], out["w_samples"][s], sb["y"], sb["weights"], sb["x"], p, "logit",
                            (cfg.burn_in, cfg.n_samples), 2)
        cdev, dpw = crit["subsets"][s], crit["pointwise"][s]
        print(f"IMPORT criteria subset {s}: device {cdev}\n  restatement {np.asarray(cref)}")
        for k in (0, 1, 3, 4, 6, 7):
            np.testing.assert_allclose(cdev[k], cref[k], rtol=1e-9, atol=0)
        assert abs(cdev[2] - cref[2]) <= 1e-9 * abs(cref[0]) and abs(cdev[5] - cref[5]) <= 1e-9 * abs(cref[4])
        np.testing.assert_allclose(dpw[:, 0], pw[:, 0], rtol=1e-9, atol=0)
    live = r["crit2"]
    assert crit["subsets"].tobytes() == live["subsets"].tobytes() and crit["total"].tobytes() == live["total"].tobytes()
    for x, y in zip(crit["pointwise"], live["pointwise"]):
        assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------- 7. refusals and the state after import
def test_refusals_and_the_state_after_import(mk, monkeypatch):
    r = _live(mk, monkeypatch, "L1")
    pb, cfg, a = r["pb"], r["cfg"], r["out"]
    lib = mk.load()
    count = lib.mk_session_count()
    kept, n, p = cfg.kept, cfg.n_samples, cfg.p
    sm, ws = a["samples"], a["w_samples"]

    def refused(ses, samples, w_samples, match):
        with pytest.raises(mk.MkError, match=match) as e:
            ses.import_chain(samples, w_samples)
        assert e.value.code == -1 and not ses.imported and ses.iteration == 0

    with mk.Session(pb["subsets"], _cfg(mk, "L1", tile=0), coords_test=pb["coords_test"], subset_base=BASE,
                    record_w=True) as fused:
        refused(fused, sm, ws, "keeps no chain states")
    with mk.Session(pb["subsets"], cfg, coords_test=pb["coords_test"], subset_base=BASE, record_w=True) as ses:
        phi_b = [x.copy() for x in sm]
        phi_b[1][24, p + 3] = cfg.phi_b[0]                          # 0-based row 24: iteration 25; column p + ntri
        refused(ses, phi_b, ws, f"phi of subset {BASE + 1}, iteration 25, column {p + 3} ")
        notpd = [x.copy() for x in sm]
        notpd[0][30, p + 1] = 50.0                                  # K_21 far above sqrt(K_11 K_22)
        refused(ses, notpd, ws, f"K of subset {BASE}, iteration 31, columns {p} .. {p + 2} is not positive definite")
        nan_w = [x.copy() for x in ws]
        nan_w[1][7, 33] = np.nan
        refused(ses, sm, nan_w, f"w_samples of subset {BASE + 1}, iteration 34, row 7 is nan")
        refused(ses, sm, [x[:, -(kept - 1):] for x in ws], f"n_w = {kept - 1} is outside")
        refused(ses, sm, [x[:, -kept:] for x in ws], f"n_w = {kept} must be n_samples = {n}")     # the session records w
        # every refusal left the session as created: it still takes the good chain
        ses.import_chain(sm, ws)
        assert ses.imported and ses.iteration == n
        with pytest.raises(mk.MkError, match="already holds an imported chain"):
            ses.import_chain(sm, ws)
        with pytest.raises(mk.MkError, match="imported chain, which is complete"):
            ses.run(1)
        with pytest.raises(mk.MkError, match="imported chain"):
            ses.chain_state(0)
        with pytest.raises(mk.MkError, match="imported chain"):
            ses.set_lookahead(0)
        with pytest.raises(mk.MkError, match="came without acceptance"):
            ses.outputs(quantiles=False, acceptance=True)
        assert not ses.notpd_counts().any()
        got = ses.outputs(quantiles=False, samples=True)
        assert got["samples"][0].tobytes() == sm[0].tobytes()
    with mk.Session(pb["subsets"], cfg, coords_test=pb["coords_test"], subset_base=BASE, record_w=True) as ran:
        ran.run(1)
        with pytest.raises(mk.MkError, match="has run 1 iterations"):
            ran.import_chain(sm, ws)
    with mk.Session(pb["subsets"], cfg, coords_test=pb["coords_test"], subset_base=BASE, record_w=True) as ses:
        ses.import_chain(sm, ws, a["acceptance"])
        acc = ses.outputs(quantiles=False, acceptance=True)["acceptance"]
        for s in range(len(pb["subsets"])):
            assert acc[s].tobytes() == a["acceptance"][s].tobytes()
    assert lib.mk_session_count() == count


# ---------------------------------------------------------------- 8. save and load
def test_save_and_load_a_fit(mk, monkeypatch, tmp_path):
    """A small spMvGLM fit saved and closed; two load_fits give byte-equal spPredict draws within 2 hard of the
    original fit's, and the original's p.beta.theta.samples byte for byte."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    n, n_test, seed, idx = 129, 40, 21, 3
    d = mk.synthetic.generate(n, q=1, n_test=n_test, seed=seed)
    kw = dict(starting=dict(beta=np.zeros(2), phi=6.0, A=[1.0], w=0.0), tuning=dict(beta=np.full(2, 0.05), phi=1.0, A=0.1, w=0.5),
              priors={"phi.Unif": (4.0, 12.0), "K.IW": (1.0, [[0.1]])}, amcmc={"n.batch": 2, "batch.length": 6})
    path = str(tmp_path / "fit.npz")
    with mk.spMvGLM([(d["y"], d["x"])], d["coords"], np.ones((n, 1)), seed=seed, subset_index=idx, **kw) as fit:
        orig = mk.spPredict(fit, d["coords_test"])["p.w.predictive.samples"]
        samples, w = fit["p.beta.theta.samples"], fit["p.w.samples"]
        fit.save(path)
    draws = []
    for _ in range(2):
        with mk.load_fit(path) as back:
            assert back["p.beta.theta.samples"].tobytes() == samples.tobytes()
            assert back["p.w.samples"].tobytes() == w.tobytes()
            assert back["_session"].imported
            draws.append(mk.spPredict(back, d["coords_test"])["p.w.predictive.samples"])
            diag = mk.spDiag(back, start=3)
            assert np.isfinite(list(diag["DIC"].values())).all()
    assert draws[0].tobytes() == draws[1].tobytes() and draws[0].shape == orig.shape == (n_test, 12)
    sub = kr.SubsetRef(d["coords"], d["coords_test"], False)
    key = philox.make_key(seed, idx)
    worst = 0.0
    for it in range(12):
        row = samples[it]
        ref = kr.predict_state(sub, row[2:3], row[3:4], np.zeros(1), w[:, it], key, it)
        dd = np.abs(draws[0][:, it] - orig[:, it])
        worst = max(worst, float(np.max(dd / (2.0 * ref["hard"]))))
        assert (dd <= 2.0 * ref["hard"]).all(), (it, dd.max(), ref["hard"].min())
        bad, _ = kr.judge(draws[0][:, it].reshape(n_test, 1), ref)
        assert not bad, bad
    print(f"\nIMPORT load_fit: largest |loaded - original| / 2 hard {worst:.1e}")


def test_load_a_range_of_a_saved_session(mk, monkeypatch, tmp_path):
    """load_session(path, subsets=(1, 2)) of a 3-subset file gives the grids of subsets 1-2 of the full load."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    pb = kr.problem("E1")
    subsets = pb["subsets"][:3]
    cfg = _cfg(mk, "E1")
    path = str(tmp_path / "ses.npz")
    with mk.Session(subsets, cfg, subset_base=BASE, record_w=True) as ses:
        ses.run(cfg.n_samples)
        mk.fitfile.save_session(ses, path)
    ct = pb["coords_test"][:64]
    with mk.fitfile.load_session(path) as full:
        assert full.S == 3 and full.imported
        full.set_test_sites(ct)
        whole = full.outputs(w_pred_samples=True)
    with mk.fitfile.load_session(path, subsets=(1, 2)) as part:
        assert part.S == 2
        part.set_test_sites(ct)
        got = part.outputs(w_pred_samples=True)
    for j in range(2):
        for f in ("parameters", "w_predict", "w_pred_samples"):
            assert got[f][j].tobytes() == whole[f][j + 1].tobytes(), (f, j)
