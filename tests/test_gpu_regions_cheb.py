"""Areal prediction on the phi-interpolated replay (include/mk.h "areal prediction", MK_REGIONS_INTERP;
Session.set_regions(..., interpolate=True)) against the exact route of the same session, against the NumPy /
SciPy restatement tests/regions_ref.py, and against the interpolated replay without regions.

Fits (the shapes of tests/test_gpu_regions.py, whose helpers are imported): "lmc" -- q = 2
exponential, one subset of 150 sites (n_pad = 256: two K tiles, a ragged tail, row n_s inside the last 16-deep
chunk), 40 iterations, window 21..40, 179 test sites at spacing 0.03 in regions of 1, 17, 128 and 33; "q1" --
q = 1 exponential, two subsets of 150 and 131 sites in one session (n_s differs under one n_pad), 40 test sites
in regions of 1, 12 and 27; "mat", the existing Matern fit, for the fallback.  MK_KRIG_CHEB = -1 forces the
interpolated replay, as tests/test_gpu_krig_cheb_lmc.py does.

Chunks: MK_REGIONS_CHUNK = B = 3 (chunk boundaries at window states 3, 6, .., 18).  The fixed-seed fits'
recorded phi columns show, and test_the_chunk_length_cuts_runs_both_ways asserts from p.beta.theta.samples, a
pair whose phi run crosses a chunk boundary and a pair whose run starts exactly on one.

Bars.  Interpolated against exact draws, and against the restatement: 1e-8 absolute, the project's bar for
interpolated against exact draws, under two asserted guards -- cond(S) <= 1e4 for every (state, outcome,
region) from the restatement alone, and the reported check <= 1e-12, so cond x check <= 1e-8.  One-site regions
against p_pred_samples of the same interpolated replay: 1e-10 where 1 - s >= 1e-3 (only the node values'
summation order and one rounding of 1 - interp(s) against interp(1 - s) differ).  Everything else is equality
of bits.

Largest figures seen on an MI355X (each test prints its own): check 3.5e-15 ("lmc", E = 14 slots) and 2.7e-15
("q1", E = 13); cond(S) 1.6e2 and 6.7e1; interpolated against exact draws 1.4e-15 and 1.6e-15, against the
restatement 1.9e-15 and 8.9e-16; one-site regions against the p draws 1.6e-15 (smallest 1 - s 9.5e-3); with a
determined site the other regions 1.4e-15.  phi changes at window states 1 3 4 5 7 11 12 13 14 16 17 18 19 and
1 2 5 6 9 10 11 12 13 16 17 18 ("lmc", outcomes 0 and 1), 1 2 3 4 5 6 7 9 16 and 1 3 4 5 6 7 8 9 11 12 13 15
16 17 18 19 ("q1", subsets 0 and 1)."""
import ctypes
import math

import numpy as np
import pytest

from regions_ref import RegionRef
import test_gpu_regions as base
from test_gpu_regions import FIRST, KS_REGIONS, LAST, N_WIN, SEED, THR, _free_bytes, _grid_sites, _reference

pytestmark = pytest.mark.gpu
DRAW_ATOL = 1e-8
ONE_SITE_ATOL = 1e-10
COND_MAX = 1e4
CHECK_MAX = 1e-12
B = 3
OUT_KEYS = ("w_pred_samples", "p_pred_samples", "w_predict", "p_predict")
REGION_KEYS = ("region_samples", "region_predict", "subsets", "singular")
_q1 = {}
_own = {}


@pytest.fixture(autouse=True)
def _forced_interpolation(monkeypatch):
    monkeypatch.setenv("MK_KRIG_CHEB", "-1")
    monkeypatch.setenv("MK_REGIONS_CHUNK", str(B))


def _fit(mk, name):
    """test_gpu_regions' fit of that name, made again for this module: that module's tests count kind 19's
    launches on their session since its creation, so these tests replay on a session of their own."""
    if name not in _own:
        theirs = base._fits.pop(name, None)
        try:
            _own[name] = base._fit(mk, name)
        finally:
            base._fits.pop(name, None)
            if theirs is not None:
                base._fits[name] = theirs
    return _own[name]


def _replay(ses, ct, xt, offsets, wts, interpolate, thr=THR):
    """One replay of the window: (regions' dict or None without offsets, the tile's other outputs, kind 19's
    share of it)."""
    ses.set_test_sites(ct, x_test=xt)
    ses.set_kept_window(FIRST, LAST)
    if offsets is not None:
        ses.set_regions(offsets, wts, thr, interpolate=interpolate)
    before = ses.kernel_stats(KS_REGIONS)
    out = ses.outputs(quantiles=True, w_pred_samples=True, p_pred_samples=True)
    after = ses.kernel_stats(KS_REGIONS)
    rg = ses.regions(samples=True) if offsets is not None else None
    return rg, out, {k: after[k] - before[k] for k in ("launches", "ms")}


def _same_bits(a, b, n_sub=1, what=""):
    for k in REGION_KEYS:
        for i in range(n_sub):
            assert np.array_equal(a[0][k][i], b[0][k][i]), (what, k, i)
    for k in OUT_KEYS:
        for i in range(n_sub):
            assert np.array_equal(a[1][k][i], b[1][k][i]), (what, k, i)


def _lmc(mk):
    """The "lmc" fit with both routes replayed once and the restatement, shared by the tests."""
    f = _fit(mk, "lmc")
    if "cheb" not in f:
        f["exact"] = _replay(f["ses"], f["ct"], f["xt"], f["offsets"], f["wts"], False)
        f["cheb"] = _replay(f["ses"], f["ct"], f["xt"], f["offsets"], f["wts"], True)
        if "ref" not in f:
            f["ref_obj"], f["ref"] = _reference(f, f["ct"], f["xt"], f["offsets"], f["wts"])
    return f


def _q1_case(mk):
    """q = 1, two subsets of 150 and 131 sites: the subsets, the config, the sites and the regions."""
    if not _q1:
        d = mk.synthetic.generate(281, q=1, n_test=1, seed=23)
        subs = [dict(coords=d["coords"][a:b], y=d["y"][a:b], weights=np.ones(b - a), x=d["x"][a:b]) for a, b in ((0, 150), (150, 281))]
        cfg = mk.SamplerConfig(1, 2, beta_starting=np.zeros(2), beta_tuning=np.full(2, 0.05), n_batch=4, batch_length=10,
                               burn_in=1, seed=SEED, predict_tile=256, phi_unif=(np.full(1, 4.0), np.full(1, 12.0)))
        rng = np.random.default_rng(78)
        ct = _grid_sites(40, 0.03, rng)
        xt = mk.synthetic.block_design(rng.standard_normal((40, 1)), 1)
        _q1.update(subs=subs, cfg=cfg, ct=ct, xt=xt, wts=rng.uniform(0.5, 3.0, size=40), offsets=[0, 1, 13, 40])
    return _q1


def _q1_session(mk, c, which, base):
    """Both routes of the subsets `which` in one session: (exact, interpolated, samples, w_samples)."""
    subs = [c["subs"][i] for i in which]
    with mk.Session(subs, c["cfg"], subset_base=base, record_w=True) as ses:
        ses.run(c["cfg"].n_samples)
        chain = ses.outputs(quantiles=False, samples=True, w_samples=True)
        exact = _replay(ses, c["ct"], c["xt"], c["offsets"], c["wts"], False)
        cheb = _replay(ses, c["ct"], c["xt"], c["offsets"], c["wts"], True)
    return exact, cheb, chain["samples"], chain["w_samples"]


def _q1_both(mk):
    c = _q1_case(mk)
    if "both" not in c:
        c["both"] = _q1_session(mk, c, (0, 1), 0)
    return c


def _phi_window(samples, q):
    """phi per window state and outcome, (N_WIN, q): the last q reported columns (exponential)."""
    return np.asarray(samples)[FIRST - 1:LAST, -q:]


def _cuts(phi, chunk):
    """(a run crosses a chunk boundary, a run starts exactly on one) for one pair's window phi."""
    bounds = range(chunk, len(phi), chunk)
    return any(phi[j] == phi[j - 1] for j in bounds), any(phi[j] != phi[j - 1] for j in bounds)


def test_the_chunk_length_cuts_runs_both_ways(mk):
    """B = 3: among the pairs of the two fits some run crosses a chunk boundary and some run starts exactly on
    one -- in each fit, so every parity test below factors a crossing run twice and meets a fresh run at a
    chunk's first state."""
    f = _lmc(mk)
    c = _q1_both(mk)
    pairs = {"lmc": [_phi_window(f["fit"]["p.beta.theta.samples"], 2)[:, h] for h in range(2)],
             "q1": [_phi_window(c["both"][2][s], 1)[:, 0] for s in range(2)]}
    for name, cols in pairs.items():
        cuts = [_cuts(col, B) for col in cols]
        print(name, "runs per pair", [1 + int(np.sum(np.diff(col) != 0.0)) for col in cols], "(crosses, starts on) per pair", cuts)
        assert any(x for x, _ in cuts) and any(y for _, y in cuts), (name, cuts)


def _assert_route_parity(name, exact, cheb, refs, n_sub, q, G):
    """Test 1 of the issue for one fit: refs[i] the restatement's window of subset i."""
    rg_e, rg_c = exact[0], cheb[0]
    assert rg_e["route"] == "exact" and rg_e["check"] == 0.0
    assert rg_c["route"] == "interpolated"
    print(f"{name}: check {rg_c['check']:.3e}")
    assert 0.0 <= rg_c["check"] <= CHECK_MAX
    for i in range(n_sub):
        cond = refs[i]["cond"]
        print(f"{name}[{i}]: largest cond(S) over (state, region, outcome) {cond.max():.3e}")
        assert cond.shape == (N_WIN, G, q) and (cond <= COND_MAX).all(), "the draw bar does not cover these inputs"
        e, c = rg_e["region_samples"][i], rg_c["region_samples"][i]
        assert e.shape == c.shape == refs[i]["draws"].shape == (G * q, N_WIN)          # every region is compared
        err_e, err_r = np.abs(c - e), np.abs(c - refs[i]["draws"])
        print(f"{name}[{i}]: largest |interpolated - exact| per region column {err_e.max(axis=1)}")
        print(f"{name}[{i}]: largest |interpolated - restatement| per region column {err_r.max(axis=1)}")
        assert np.isfinite(c).all() and (err_e <= DRAW_ATOL).all() and (err_r <= DRAW_ATOL).all()
        assert (rg_e["singular"][i] == 0).all() and (rg_c["singular"][i] == 0).all() and (refs[i]["singular"] == 0).all()
    # launches: E node covariances + 1 check + 2 per chunk + 2; E = the largest node count + 3 checks
    chunks = math.ceil(N_WIN / B)
    E = cheb[2]["launches"] - (1 + 2 * chunks + 2)
    print(f"{name}: kind 19 launches {cheb[2]['launches']} (E = {E}), exact route {exact[2]['launches']}")
    assert exact[2]["launches"] == 2 * N_WIN + 2
    assert 10 + 3 <= E <= 32 + 3
    t = rg_c["timing_ms"]
    assert (t > 0.0).all() and t.sum() == pytest.approx(cheb[2]["ms"], rel=1e-6)


def test_interpolated_route_matches_the_exact_route_lmc(mk):
    f = _lmc(mk)
    _assert_route_parity("lmc", f["exact"], f["cheb"], [f["ref"]], 1, 2, 4)


def test_interpolated_route_matches_the_exact_route_q1(mk):
    c = _q1_both(mk)
    exact, cheb, samples, w_samples = c["both"]
    refs = []
    for i in range(2):
        ref = RegionRef(c["subs"][i]["coords"], c["ct"], c["offsets"], c["wts"])
        refs.append(ref.window(samples[i], w_samples[i], 1, 2, SEED, i, FIRST, LAST, c["xt"]))
    _assert_route_parity("q1", exact, cheb, refs, 2, 1, 3)
    assert not np.array_equal(cheb[0]["region_samples"][0], cheb[0]["region_samples"][1])


def test_one_site_regions_are_the_interpolated_marginal_draws(mk):
    f = _lmc(mk)
    n_test = f["ct"].shape[0]
    one_minus_s = 1.0 - f["ref"]["s"]
    print(f"smallest 1 - s over states, sites and outcomes: {one_minus_s.min():.3e}")
    assert (one_minus_s >= 1e-3).all(), "the one-site bar does not cover these sites"
    rg, out, _st = _replay(f["ses"], f["ct"], f["xt"], np.arange(n_test + 1), None, True, ())
    assert rg["route"] == "interpolated"
    dev, p_marg = rg["region_samples"][0], out["p_pred_samples"][0]
    assert dev.shape == p_marg.shape == (n_test * f["q"], N_WIN)
    err = np.abs(dev - p_marg)
    print(f"largest |one-site region - p_pred_samples| {err.max():.3e}")
    assert (err <= ONE_SITE_ATOL).all()
    assert (rg["singular"][0] == 0).all()


def test_nothing_else_moves(mk):
    """The interpolated replay's own outputs with regions attached on the interpolated route are, bit for bit,
    those of the same session with no regions attached (the MEANS flag of the draw kernel changes no output)."""
    f = _lmc(mk)
    ses = f["ses"]
    ses.set_regions(None)
    stats0 = ses.kernel_stats(mk.session.KS_KRIG_CHEB)
    _rg, plain, st = _replay(ses, f["ct"], f["xt"], None, None, False)
    assert ses.kernel_stats(mk.session.KS_KRIG_CHEB)["launches"] == stats0["launches"] + 1     # it was interpolated
    assert st["launches"] == 0
    for k in OUT_KEYS:
        assert np.array_equal(plain[k][0], f["cheb"][1][k][0]), k
    assert not np.array_equal(plain["w_pred_samples"][0], f["exact"][1]["w_pred_samples"][0])   # and not the exact replay's


def test_chunks_do_not_change_a_bit(mk, monkeypatch):
    f = _lmc(mk)
    for chunk in (B + 4, 64):                                      # another chunk length; the whole window in one
        monkeypatch.setenv("MK_REGIONS_CHUNK", str(chunk))
        got = _replay(f["ses"], f["ct"], f["xt"], f["offsets"], f["wts"], True)
        assert got[0]["route"] == "interpolated" and got[0]["check"] == f["cheb"][0]["check"]
        assert got[2]["launches"] - f["cheb"][2]["launches"] == 2 * (math.ceil(N_WIN / min(chunk, N_WIN)) - math.ceil(N_WIN / B))
        _same_bits(got, f["cheb"], what=f"chunk {chunk}")


def test_subsets_do_not_depend_on_the_shard(mk):
    c = _q1_both(mk)
    for i in range(2):
        _exact, alone, _s, _w = _q1_session(mk, c, (i,), i)
        assert alone[0]["route"] == "interpolated"
        for k in REGION_KEYS:
            assert np.array_equal(c["both"][1][0][k][i], alone[0][k][0]), (i, k)


def test_matern_runs_exactly(mk):
    f = _fit(mk, "mat")
    exact = _replay(f["ses"], f["ct"], f["xt"], f["offsets"], f["wts"], False)
    asked = _replay(f["ses"], f["ct"], f["xt"], f["offsets"], f["wts"], True)
    assert asked[0]["route"] == "exact" and asked[0]["check"] == 0.0
    assert asked[2]["launches"] == 2 * N_WIN + 2
    _same_bits(asked, exact, what="matern")


def test_failed_check_and_switched_off_replay_exactly(mk, monkeypatch):
    f = _lmc(mk)
    ses = f["ses"]
    fb0 = ses.kernel_stats(mk.session.KS_KRIG_FALLBACK)["launches"]
    monkeypatch.setenv("MK_KRIG_CHEB_TOL", "-1")                   # no difference is <= -1: the check fails
    failed = _replay(ses, f["ct"], f["xt"], f["offsets"], f["wts"], True)
    monkeypatch.delenv("MK_KRIG_CHEB_TOL")
    assert ses.kernel_stats(mk.session.KS_KRIG_FALLBACK)["launches"] == fb0 + 1
    assert failed[0]["route"] == "exact" and failed[0]["check"] == 0.0
    assert failed[2]["launches"] == 2 * N_WIN + 2                  # the abandoned node launches are not priced
    _same_bits(failed, f["exact"], what="failed check")
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    off = _replay(ses, f["ct"], f["xt"], f["offsets"], f["wts"], True)
    assert ses.kernel_stats(mk.session.KS_KRIG_FALLBACK)["launches"] == fb0 + 1
    assert off[0]["route"] == "exact" and off[0]["check"] == 0.0
    _same_bits(off, f["exact"], what="MK_KRIG_CHEB=0")


def test_a_region_site_on_an_observed_site_is_flagged_on_both_routes(mk):
    f = _lmc(mk)
    q = f["q"]
    ct = f["ct"].copy()
    ct[18 + 40] = f["d"]["coords"][17]                             # site 40 of the 128-site region (region 2)
    exact = _replay(f["ses"], ct, f["xt"], f["offsets"], f["wts"], False)
    cheb = _replay(f["ses"], ct, f["xt"], f["offsets"], f["wts"], True)
    assert cheb[0]["route"] == "interpolated"
    print(f"check with a determined site {cheb[0]['check']:.3e}")
    want = np.zeros(4 * q, dtype=np.int64)
    want[2 * q:3 * q] = N_WIN
    assert np.array_equal(exact[0]["singular"][0], want) and np.array_equal(cheb[0]["singular"][0], want)
    for rg in (exact[0], cheb[0]):
        assert np.isfinite(rg["region_samples"][0]).all() and np.isfinite(rg["subsets"][0]).all()
        assert np.isfinite(rg["region_predict"][0]).all()
    others = np.r_[0:2 * q, 3 * q:4 * q]
    err = np.abs(cheb[0]["region_samples"][0] - exact[0]["region_samples"][0])
    print(f"largest |interpolated - exact|: the other regions {err[others].max():.3e}, the flagged one {err[2 * q:3 * q].max():.3e}")
    assert (err[others] <= DRAW_ATOL).all()


def test_refusals_reset_and_cost_when_off(mk):
    f = _lmc(mk)
    ses, lib = f["ses"], mk.load()
    E = mk._lib.MK_E_ARG
    asked, ran, chk = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()

    def route():
        mk._lib.check(lib.mk_session_regions_route(ses._h, ctypes.byref(asked), ctypes.byref(ran), ctypes.byref(chk)))
        return asked.value, ran.value, chk.value

    ses.set_test_sites(f["ct"], x_test=f["xt"])                    # detaches
    assert lib.mk_session_set_regions_route(ses._h, mk._lib.REGIONS_INTERP) == E
    assert b"no areal prediction asked for" in lib.mk_last_error()
    assert lib.mk_session_regions_route(ses._h, None, None, None) == E
    free0 = _free_bytes(mk)
    ses.set_regions(f["offsets"], f["wts"], THR)
    free_exact = _free_bytes(mk)
    assert route() == (0, 0, 0.0)
    for bad in (2, -1, 7):
        assert lib.mk_session_set_regions_route(ses._h, bad) == E
        assert b"unknown route" in lib.mk_last_error()
    assert route() == (0, 0, 0.0)
    ses.set_regions(f["offsets"], f["wts"], THR, interpolate=True)
    free_interp = _free_bytes(mk)
    assert route() == (1, 0, 0.0)                                  # asked, not run yet
    # attaching costs what it costs today on either route: the factors, draws, grids and planes, and no node,
    # means or chunk buffer (those live inside a replay)
    q, G = f["q"], len(f["offsets"]) - 1
    fsz = int(np.sum(np.diff(f["offsets"]) ** 2))
    n_states = f["fit"]["_n_samples"]                              # burn_in = 1: every iteration is a kept state
    today = 8 * (q * fsz + n_states * G * q + G * q * 200 + (2 + len(THR)) * G * q)
    print(f"free HBM: attach (exact) -{free0 - free_exact}, attach (interpolated) -{free0 - free_interp}, today's buffers {today}")
    assert abs(free_exact - free_interp) <= (2 << 20)
    assert free0 - free_interp <= today + (4 << 20)
    ses.set_kept_window(FIRST, LAST)
    ses.outputs(quantiles=False, w_predict_sum=True)
    assert route()[:2] == (1, 1) and 0.0 < route()[2] <= CHECK_MAX
    assert abs(_free_bytes(mk) - free_interp) <= (2 << 20)         # the replay gave its buffers back
    ses.set_regions(f["offsets"], f["wts"], THR)                   # re-attach: back to the exact route
    assert route() == (0, 0, 0.0)
    ses.set_regions(f["offsets"], f["wts"], THR, interpolate=True)
    ses.set_regions(None)
    assert lib.mk_session_regions_route(ses._h, None, None, None) == E
    assert abs(_free_bytes(mk) - free0) <= (2 << 20)
