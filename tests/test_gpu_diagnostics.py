"""Chain diagnostics on the device (include/mk.h: ess by Geyer's initial monotone sequence, mcse of
the column mean, split R-hat per chain) against their NumPy restatement tests/diag_ref.py.

Bars.  rtol 1e-9 against the restatement: a sum of <= 16,384 products carries <= ~2e-12 relative
error and the cancellation in tau = -1 + 2 sum Gamma amplifies it by at most ~1e2 on these inputs.
The stopping index of the Gamma sequence is a discontinuity, so every comparison first shows, on
the CPU, that no stop / continue decision of the restatement was closer to zero than 1e-9 (the
stand-alone inputs: every column, asserted; the sessions' own draws: such columns may be left out,
at most 1 % of them).  Bit equality between the fused and the tiled route, between tile_grids and
outputs, and between the node driver and one session: every sum's order depends on the chain's
length only.  The worst rows are exact minima / maxima.

Shapes: subsets of 150 / 163 sites (two 128-tiles with the bordered row) with q = 1 and 64 / 71
with q = 2, 24 test sites with covariates, n_batch = 8, batch_length = 8, burn_in = 17: 48 kept."""
import numpy as np
import pytest

from diag_ref import ar1, diag_ref

pytestmark = pytest.mark.gpu
RTOL = 1e-9
GUARD = 1e-9
N_TEST = 24
KW = dict(n_batch=8, batch_length=8, burn_in=17, seed=9)
KINDS = ("parameters", "w_predict", "p_predict")

_NS = (4, 5, 255, 256, 257, 1251, 4096)
_RHOS = (0.0, 0.5, 0.9, -0.5)
_chains = {}


def _inputs():
    """The AR(1) inputs of every (n, rho) and the long rho = 0.99 case, drawn once in a fixed order from
    default_rng(20250114), with the restatement's answer."""
    if not _chains:
        rng = np.random.default_rng(20250114)
        for n in _NS:
            for rho in _RHOS:
                x = ar1(rng, n, 64, rho)
                _chains[(n, rho)] = (x,) + diag_ref(x)
        x = ar1(rng, 16384, 4, 0.99)
        _chains[(16384, 0.99)] = (x,) + diag_ref(x)
    return _chains


def _compare(mk, key):
    x, ref, aux = _inputs()[key]
    print(f"n = {key[0]}, rho = {key[1]}: smallest |Gamma| at a decision {aux[0].min():.2e}, "
          f"pairs added {int(aux[1].min())} .. {int(aux[1].max())}")
    assert aux[0].min() >= GUARD            # no column's stopping index hangs on rounding
    got = mk.chain_diagnostics(x)
    assert got.shape == ref.shape == (3, x.shape[1])
    print("largest relative differences (ess, mcse, rhat):", np.abs(got / ref - 1).max(axis=1))
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0)
    return got


@pytest.mark.parametrize("rho", _RHOS)
@pytest.mark.parametrize("n", _NS)
def test_kernel_against_restatement(mk, n, rho):
    """n = 4 the minimum, 5 the odd split, 255 / 256 / 257 around the thread count, 1251 the
    reference's kept count, 4096 sixteen strides per thread; the axis argument reads the transpose."""
    got = _compare(mk, (n, rho))
    if n == 257:
        assert np.array_equal(mk.chain_diagnostics(np.ascontiguousarray(_inputs()[(n, rho)][0].T), axis=1), got)


def test_kernel_full_lds_long_memory(mk):
    """16,384 states (the whole 128 KB of LDS) at rho = 0.99: hundreds of lags, dozens of lag blocks,
    before the stop."""
    _compare(mk, (16384, 0.99))
    assert _inputs()[(16384, 0.99)][2][1].min() >= 64       # pairs added: >= 128 lags in every column


def test_edges(mk):
    never = mk.chain_diagnostics(np.full((16, 1), 1.5))
    assert np.array_equal(never[:, 0], [0.0, 0.0, np.inf])
    step = mk.chain_diagnostics(np.array([[1.0], [1.0], [2.0], [2.0]]))
    assert step[2, 0] == np.inf and np.isfinite(step[0, 0]) and step[0, 0] > 0 and np.isfinite(step[1, 0])
    np.testing.assert_allclose(step[:2, 0], diag_ref(np.array([[1.0], [1.0], [2.0], [2.0]]))[0][:2, 0], rtol=RTOL)
    x = ar1(np.random.default_rng(1), 300, 3, 0.5)
    x[123, 1] = np.nan
    got = mk.chain_diagnostics(x)                      # the call returns: the lag loop ends
    assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, [0, 2]]).all()
    x[123, 1] = np.inf
    assert np.isnan(mk.chain_diagnostics(x)[:, 1]).all()
    for n in (3, 16385):
        with pytest.raises(mk.MkError) as e:
            mk.chain_diagnostics(np.zeros((n, 2)))
        assert e.value.code == mk._lib.MK_E_ARG


# ---------------------------------------------------------------- sessions
_CASES = {"q1": ([150, 163], 1), "q2": ([64, 71], 2)}
_OUTS = dict(diagnostics=True, samples=True, w_pred_samples=True, p_pred_samples=True)
_fused = {}


def _problem(mk, sizes, q, seed=9):
    off = np.concatenate([[0], np.cumsum(sizes)])
    d = mk.synthetic.generate(int(off[-1]), q=q, n_test=N_TEST, seed=seed + q)
    subs = []
    for s, m in enumerate(sizes):
        rows = slice(off[s] * q, (off[s] + m) * q)
        subs.append(dict(coords=d["coords"][off[s]:off[s] + m], y=d["y"][rows], weights=np.ones(m * q), x=d["x"][rows]))
    return d, subs


def _cfg(mk, q, predict_tile=0):
    p = 2 * q
    return mk.SamplerConfig(q, p, beta_starting=np.zeros(p), beta_tuning=np.full(p, 0.05), predict_tile=predict_tile, **KW)


def _fused_run(mk, name, monkeypatch):
    """One fused fit per case with exact kriging (MK_KRIG_CHEB=0, so a tiled session kriges the same
    draws), shared and left unchanged by the tests that read it."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    if name not in _fused:
        sizes, q = _CASES[name]
        d, subs = _problem(mk, sizes, q)
        with mk.Session(subs, _cfg(mk, q), coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
            ses.run(64)
            before = ses.kernel_stats(14)["launches"]
            plain = ses.outputs()
            between = ses.kernel_stats(14)["launches"]
            out = ses.outputs(**_OUTS)
            after = ses.kernel_stats(14)
        _fused[name] = dict(d=d, subs=subs, q=q, out=out, plain=plain, launches=(before, between, after))
    return _fused[name]


def _check_against_restatement(out, rows, n_subsets):
    """Every '<kind>_diag' of out against the restatement on the device's own draws (rows: the kept
    rows of `samples`), and the worst rows against the exact minima / maxima."""
    left_out = total = 0
    for s in range(n_subsets):
        draws = dict(parameters=out["samples"][s][rows], w_predict=out["w_pred_samples"][s].T,
                     p_predict=out["p_pred_samples"][s].T)
        for kind in KINDS:
            ref, aux = diag_ref(draws[kind])
            got = out[kind + "_diag"][s]
            assert got.shape == ref.shape
            ok = aux[0] >= GUARD
            left_out += int((~ok).sum())
            total += ok.size
            print(f"subset {s} {kind}: {draws[kind].shape[0]} states, largest relative difference "
                  f"{np.nanmax(np.abs(got[:, ok] / ref[:, ok] - 1)):.2e}, smallest |Gamma| {aux[0].min():.2e}")
            np.testing.assert_allclose(got[:, ok], ref[:, ok], rtol=RTOL, atol=0)
    assert left_out <= 0.01 * total, (left_out, total)
    for kind in KINDS:
        a = np.stack(out[kind + "_diag"])
        assert not np.isnan(a).any()
        worst = np.stack([a[:, 0].min(axis=0), a[:, 1].max(axis=0), a[:, 2].max(axis=0)])
        assert np.array_equal(out[kind + "_diag_worst"], worst), kind


@pytest.mark.parametrize("name", list(_CASES))
def test_fused_session(mk, name, monkeypatch):
    r = _fused_run(mk, name, monkeypatch)
    out, q = r["out"], r["q"]
    assert out["w_predict_diag"][0].shape == out["p_predict_diag"][1].shape == (3, q * N_TEST)
    assert out["parameters_diag_worst"].shape == (3, 2 * q + q * (q + 1) // 2 + q)
    _check_against_restatement(out, slice(KW["burn_in"] - 1, None), 2)
    for f, v in r["plain"].items():        # asking for diagnostics changes nothing else
        for s in range(2):
            assert np.array_equal(out[f][s], v[s]), f
    assert not any(k.endswith("_diag") or k.endswith("_diag_worst") for k in r["plain"])


def test_off_costs_nothing(mk, monkeypatch):
    """Kernel-stats kind 14 counts the diagnostic launches: none until diagnostics are asked for."""
    before, between, after = _fused_run(mk, "q1", monkeypatch)["launches"]
    assert before == 0 and between == 0
    assert after["launches"] > 0 and after["ms"] > 0.0


@pytest.mark.parametrize("name", list(_CASES))
def test_tiled_equals_fused(mk, name, monkeypatch):
    """predict_tile = 16 over the 24 sites: tiles of 16 and 8.  Once through outputs (the sink attached
    for the call), once tile by tile through tile_grids: the fused session's numbers bit for bit."""
    r = _fused_run(mk, name, monkeypatch)
    fused, q, d = r["out"], r["q"], r["d"]
    with mk.Session(r["subs"], _cfg(mk, q, predict_tile=16), coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(64)
        assert ses.predict_tile == 16
        tiled = ses.outputs(**_OUTS)
        tiles = [ses.tile_grids(t0, prob=True, diagnostics=True) for t0 in (0, 16)]
        only_par = ses.outputs(quantiles=False, diagnostics="parameters")
    assert set(only_par) == {"parameters_diag", "parameters_diag_worst"}
    for kind in KINDS:
        for s in range(2):
            assert np.array_equal(tiled[kind + "_diag"][s], fused[kind + "_diag"][s]), (kind, s)
        assert np.array_equal(tiled[kind + "_diag_worst"], fused[kind + "_diag_worst"]), kind
    assert np.array_equal(only_par["parameters_diag_worst"], fused["parameters_diag_worst"])
    for (gw, gp, dg), (c0, c1) in zip(tiles, ((0, 16 * q), (16 * q, 24 * q))):
        assert set(dg) == {k + sfx for k in KINDS[1:] for sfx in ("_diag", "_diag_worst")}
        for kind in KINDS[1:]:
            for s in range(2):
                assert np.array_equal(dg[kind + "_diag"][s], fused[kind + "_diag"][s][:, c0:c1]), (kind, s)
            assert np.array_equal(dg[kind + "_diag_worst"], fused[kind + "_diag_worst"][:, c0:c1]), kind
        for s in range(2):
            assert np.array_equal(gw[s], fused["w_predict"][s][:, c0:c1])
            assert np.array_equal(gp[s], fused["p_predict"][s][:, c0:c1])


def test_kept_window(mk, monkeypatch):
    """A tiled session with set_kept_window(20, 60): the parameters, w and p diagnostics are those of
    exactly these 41 states; asking a tiled session for its draws' diagnostics directly names the sink."""
    r = _fused_run(mk, "q1", monkeypatch)
    d = r["d"]
    with mk.Session(r["subs"], _cfg(mk, 1, predict_tile=16), coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(64)
        ses.set_kept_window(20, 60)
        out = ses.outputs(**_OUTS)
        lib = mk.load()
        db = mk.outbuf.DiagnosticBuffers(2, ses.cfg, N_TEST, {"w_predict_diag"})
        with pytest.raises(mk.MkError) as e:
            mk._lib.check(lib.mk_session_diagnostics(ses._h, db.c))
        assert e.value.code == mk._lib.MK_E_ARG and "mk_session_set_diagnostics" in str(e.value)
    assert out["w_pred_samples"][0].shape == (N_TEST, 41)
    _check_against_restatement(out, slice(19, 60), 2)


def test_spbayes_surface(mk):
    """spDiagnostics(fit, start, end) and spPredict(..., diagnostics=True) are the restatement on the
    fit's own samples and the returned draws of that window (thin only picks what is returned)."""
    n = 80
    d = mk.synthetic.generate(n, q=1, n_test=N_TEST, seed=31)
    starting = {"beta": np.zeros(2), "phi": 3 / 0.5, "A": np.ones(1), "w": 0.0}
    tuning = {"beta": np.full(2, 0.05), "phi": 1.0, "A": 0.1, "w": 0.5}
    priors = {"phi.Unif": (3 / 0.75, 3 / 0.25), "K.IW": (1, 0.1 * np.eye(1))}
    amcmc = {"n.batch": 8, "batch.length": 8, "accept.rate": 0.43}
    with mk.spMvGLM([(d["y"], d["x"])], d["coords"], np.ones((n, 1)), starting, tuning, priors, amcmc, seed=9) as fit:
        got = mk.spDiagnostics(fit, start=17, end=64)
        pred = mk.spPredict(fit, d["coords_test"], pred_covars=d["x_test"], start=17, end=64, diagnostics=True)
        thinned = mk.spPredict(fit, d["coords_test"], pred_covars=d["x_test"], start=17, end=64, thin=2, diagnostics=True)
        with pytest.raises(ValueError):
            mk.spDiagnostics(fit, start=0)
    pairs = [(got, fit["p.beta.theta.samples"][16:64]),
             (pred["w.predictive.diagnostics"], pred["p.w.predictive.samples"].T),
             (pred["y.predictive.diagnostics"], pred["p.y.predictive.samples"].T)]
    for dev, draws in pairs:
        ref, aux = diag_ref(draws)
        assert draws.shape[0] == 48 and dev.shape == ref.shape
        assert aux[0].min() >= GUARD
        np.testing.assert_allclose(dev, ref, rtol=RTOL, atol=0)
    assert thinned["p.w.predictive.samples"].shape == (N_TEST, 24)
    assert np.array_equal(thinned["w.predictive.diagnostics"], pred["w.predictive.diagnostics"])
    assert np.array_equal(thinned["y.predictive.diagnostics"], pred["y.predictive.diagnostics"])


_node = {}


@pytest.mark.parametrize("tile", [0, 16])
def test_node_equals_one_session(mk, tile):
    """Four q = 1 subsets over two blocks of one device, fused and tiled: every per-subset array as one
    session makes it, and the worst rows folded over the two blocks equal the session's."""
    if not _node:
        d, subs = _problem(mk, [150, 163, 140, 129], 1, seed=4)
        _node.update(d=d, subs=subs)
    d, subs = _node["d"], _node["subs"]
    cfg = _cfg(mk, 1, predict_tile=tile)
    with mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(64)
        one = ses.outputs(diagnostics=True)
    got = mk.meta_fit_node(subs, cfg, coords_test=d["coords_test"], devices=(0, 0), x_test=d["x_test"], diagnostics=True)
    for kind in KINDS:
        for s in range(4):
            assert np.array_equal(got[kind + "_diag"][s], one[kind + "_diag"][s]), (kind, s)
        a = np.stack(one[kind + "_diag"])
        assert not np.isnan(a).any()
        worst = np.stack([a[:, 0].min(axis=0), a[:, 1].max(axis=0), a[:, 2].max(axis=0)])
        assert np.array_equal(got[kind + "_diag_worst"], worst), kind
        assert np.array_equal(one[kind + "_diag_worst"], worst), kind
    for s in range(4):
        assert np.array_equal(got["w_predict"][s], one["w_predict"][s])
    plain = mk.meta_fit_node(subs, cfg, coords_test=d["coords_test"], devices=(0, 0), x_test=d["x_test"])
    assert not any("_diag" in k for k in plain)
    assert np.array_equal(plain["result2"], got["result2"]) and np.array_equal(plain["result3"], got["result3"])
