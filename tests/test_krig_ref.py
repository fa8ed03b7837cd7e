"""tests/krig_ref.py under test on the CPU, before any device draw is judged against it: the 80-bit
predictor against mpmath and against closed forms, the Philox slots against the oracle's own kriging,
the margin that every geometry of tests/test_gpu_krig_parity.py leaves between LAPACK's error and the
hard bar, and the bars against predictors spoiled in one place."""
import numpy as np
import pytest

from oracle import philox
from oracle import spmvglm as om

import krig_ref as kr

LD = np.longdouble
LD_EPS = float(np.finfo(LD).eps)      # 1.08e-19 for 80-bit


def _small(n=40, n_test=12, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(size=(n, 2)), rng.uniform(size=(n_test, 2)), rng.standard_normal(n)


def test_s_and_m_against_mpmath():
    """40 exponential sites, 12 test sites: s and m from mpmath at 50 digits (its own exp, sqrt and LU
    solve of the float64 coordinates) agree within 64 x 1.08e-19 x kappa -- the order of the problem plus
    margin for the longdouble solves."""
    mp = pytest.importorskip("mpmath")
    if LD_EPS > 2e-19:
        pytest.skip("np.longdouble is not 80-bit here")
    mp.mp.dps = 50
    c, ct, u = _small()
    phi = 6.3
    sub = kr.SubsetRef(c, ct)
    f = sub.at(phi)
    z = kr.forward_solve(f["L"], u.astype(LD)[:, None])[:, 0]
    m = f["X"].T @ z
    n, T = c.shape[0], ct.shape[0]

    def rho(a, b):
        dx, dy = mp.mpf(float(a[0])) - mp.mpf(float(b[0])), mp.mpf(float(a[1])) - mp.mpf(float(b[1]))
        return mp.exp(-mp.mpf(phi) * mp.sqrt(dx * dx + dy * dy))

    R = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            R[i, j] = rho(c[i], c[j])
    um = mp.matrix([mp.mpf(float(v)) for v in u])
    bar = 64 * 1.08e-19 * f["kappa"]
    for t in range(T):
        r = mp.matrix([rho(ct[t], c[i]) for i in range(n)])
        lam = mp.lu_solve(R, r)
        s_ref = sum(r[i] * lam[i] for i in range(n))
        m_ref = sum(um[i] * lam[i] for i in range(n))
        assert float(abs(_mpf(mp, f["s"][t]) - s_ref)) <= bar, t
        assert float(abs(_mpf(mp, m[t]) - m_ref)) <= bar * max(1.0, float(np.linalg.norm(u))), t


def _mpf(mp, x):
    """A longdouble as an mpf, exactly: its float64 head plus the float64 of the remainder."""
    hi = float(x)
    lo = float(x - LD(hi))
    return mp.mpf(hi) + mp.mpf(lo)


def test_a_test_site_on_an_observed_site_and_one_far_away():
    """rho_t = R e_i at observed site i: s = 1 and m = u_i to 1e-17 kappa.  At (50, 50) every
    correlation is exp(-6.3 x 69) = 0 to any precision: s = 0, m = 0 and the draw is A z* exactly."""
    c, ct, u = _small()
    ct = ct.copy()
    ct[4] = c[17]
    ct[9] = [50.0, 50.0]
    sub = kr.SubsetRef(c, ct)
    f = sub.at(6.3)
    z = kr.forward_solve(f["L"], u.astype(LD)[:, None])[:, 0]
    m = f["X"].T @ z
    tol = 1e-17 * f["kappa"]
    assert abs(float(f["s"][4] - 1)) <= tol and abs(float(m[4] - LD(u[17]))) <= tol
    assert float(f["s"][9]) < 1e-300 and abs(float(m[9])) < 1e-150
    key = philox.make_key(5, 2)
    K = 1.7
    ref = kr.predict_state(sub, [K], [6.3], [0.0], np.sqrt(K) * u, key, 7)
    zs = philox.predict_normal(key, np.array([9]), 7)[0]
    assert ref["draw"][9, 0] == np.sqrt(LD(K)) * LD(zs)
    assert ref["draw_lapack"][9, 0] == np.sqrt(K) * zs
    assert not ref["regular"][4] and ref["regular"][9]


def test_matern_arm_is_the_longdouble_reference():
    """corr_longdouble's Matern arm is matern_ref.rho_longdouble (tests/test_matern_ref.py), not float64 kv
    promoted: at nu = 1/2 it is exp(-phi d) to longdouble precision, which float64 cannot be; it is 1 at
    d = 0; and the oracle's kv stays within 1e-11 of it at a general nu."""
    c, ct, _ = _small()
    ct = ct.copy()
    ct[4] = c[17]
    d = kr.dist_longdouble(ct, c)
    r = kr.corr_longdouble(d, 6.3, 0.5, True)
    assert r.dtype == LD and r[4, 17] == 1
    e = np.exp(-LD(6.3) * d)
    assert float(np.max(np.abs(r - e) / e)) <= 64 * LD_EPS
    r = kr.corr_longdouble(d, 6.3, 1.3, True)
    o = om.correlation(d.astype(np.float64), 6.3, 1.3, om.COV_MATERN)
    assert float(np.max(np.abs(o.astype(LD) - r) / r)) <= 1e-11


@pytest.mark.parametrize("q", [1, 2])
def test_one_philox_slot_per_site_outcome_and_iteration(q):
    """fit_subset (the CPU oracle) krigs four far sites with global indices 0, 3, 256 and 260: there
    m = 0 and sd = 1 exactly, so w_pred is A z*, and predict_state -- fed the oracle's recorded K, phi
    and w -- must have drawn the same normal for every (site, outcome, kept iteration): bit for bit at
    q = 1 (sqrt(fl(a^2)) = a), to 4 eps |A|_inf max |z*| at q = 2 (A comes back through a 2 x 2 Cholesky)."""
    n, p = 12, 2 * q
    rng = np.random.default_rng(8)
    coords = rng.uniform(size=(n, 2))
    xcov = rng.standard_normal((n, q))
    X = np.zeros((n * q, p))
    for a in range(q):
        X[a::q, 2 * a], X[a::q, 2 * a + 1] = 1.0, xcov[:, a]
    y = (rng.uniform(size=n * q) < 0.5).astype(float)
    sites = np.array([0, 3, 256, 260])
    ct = np.stack([50.0 + np.arange(4), np.full(4, 50.0)], axis=1)
    cfg = om.Config(q, p, np.zeros(p), np.full(p, 0.05), n_batch=2, batch_length=4, burn_in=5, seed=11)
    fit = om.fit_subset(coords, y, np.ones(n * q), X, cfg, subset=3, coords_test=ct, site_index=sites, record_w=True,
                        quantiles=False)
    sub = kr.SubsetRef(coords, ct)
    key = philox.make_key(cfg.seed, 3)
    ntri = q * (q + 1) // 2
    for k in range(cfg.kept):
        it = cfg.burn_in - 1 + k
        row = fit["samples"][it]
        ref = kr.predict_state(sub, row[p:p + ntri], row[p + ntri:p + ntri + q], np.zeros(q), fit["w_samples"][it], key, it,
                               site_index=sites)
        got = fit["w_pred"][k].reshape(4, q)
        tol = 4 * kr.EPS * ref["normA"] * np.max(np.abs(ref["zstar"]))     # the mix A z* sums q products
        if q == 1:
            assert np.array_equal(ref["draw_lapack"], got)
        else:
            np.testing.assert_allclose(ref["draw_lapack"], got, rtol=0, atol=tol)
        np.testing.assert_allclose(ref["draw"].astype(float), got, rtol=0, atol=tol)
    # and a neighbouring slot is another number
    assert philox.predict_normal(key, np.array([3 * q]), 4)[0] != philox.predict_normal(key, np.array([3 * q + 1]), 4)[0]


# ---- every geometry the GPU tests use, with a synthetic state: u ~ N(0, R_h), A = 1 or a fixed factor
_A2 = np.array([[1.1, 0.0], [-0.6, 0.8]])
_synthetic = {}


def synthetic_state(case):
    """(problem, per subset: SubsetRef, predict_state's ref at a synthetic state, its u), once per case."""
    if case not in _synthetic:
        c = kr.CASES[case]
        q, matern = c["q"], c["model"] == "matern"
        pb = kr.problem(case)
        rng = np.random.default_rng(c["seed"] + 1000)
        A = np.array([[1.0]]) if q == 1 else _A2
        K = A @ A.T
        K_tri = [K[i, j] for j in range(q) for i in range(j, q)]
        phi = [6.3, 7.9][:q]
        nu = [0.6, 0.6][:q]
        out = []
        for i, sb in enumerate(pb["subsets"]):
            sub = kr.SubsetRef(sb["coords"], pb["coords_test"], matern)
            n = sub.n
            U = np.zeros((n, q))
            for h in range(q):
                R = om.correlation(sub.D64, phi[h], nu[h], om.COV_MATERN if matern else om.COV_EXPONENTIAL)
                U[:, h] = np.linalg.cholesky(R) @ rng.standard_normal(n)
            w = (U @ A.T).reshape(-1)
            out.append((sub, kr.predict_state(sub, K_tri, phi, nu, w, philox.make_key(20250114, i), 5), U))
        _synthetic[case] = (pb, out)
    return _synthetic[case]


@pytest.mark.parametrize("case", sorted(kr.CASES))
def test_lapack_stays_a_sixteenth_inside_the_hard_bar(case):
    """At every site of every geometry LAPACK's own error is below 1/16 of the hard bar, so at the
    regular sites the comparative bar (16 x LAPACK's error) is the one that binds; and LAPACK itself
    passes both bars.  The specials are where the case table puts them.
    LAPACK's error is counted beyond what any float64 evaluation loses after the solves: 2 eps max(1, |draw|)
    for the three roundings of A (m + sd z*), and |A|_inf |z*| min(sqrt(2 eps), 2 eps / sd_ref) for storing s
    and 1 - s (an ulp of 1 each).  At E1's two-site subset (N = 3, kappa = 1.03) a sixteenth of the hard
    bar, 3 eps / 16, is below the half ulp of merely storing the draw; from N = 32 on the allowance is
    itself below the sixteenth."""
    pb, out = synthetic_state(case)
    c = kr.CASES[case]
    T = pb["coords_test"].shape[0]
    assert T == (c["n_test"] or 71)
    assert {0, 1, 2, 3, T - 1} <= set(pb["special"]) and (T < 257 or {255, 256} <= set(pb["special"]))
    assert sum(v.startswith("duplicate") for v in pb["special"].values()) == 1
    for i, (sub, ref, _) in enumerate(out):
        errl = np.max(np.abs(ref["draw_lapack"].astype(LD) - ref["draw"]), axis=1).astype(float)
        sdf = ref["sd"].astype(float)
        with np.errstate(divide="ignore"):
            ends = (2 * kr.EPS * np.maximum(1.0, np.max(np.abs(ref["draw"].astype(float)), axis=1)) + ref["normA"] * np.max(
                np.abs(ref["zstar"]) * np.minimum(np.sqrt(2 * kr.EPS), 2 * kr.EPS / sdf), axis=1))
        worst = float(np.max(np.maximum(errl - ends, 0.0) / ref["hard"]))
        singular = int(np.sum(~ref["regular"]))
        print(f"{case} subset {i} n {sub.n}: kappa {ref['kappa']:.2e}, near-singular sites {singular}, "
              f"lapack error / hard bar at most {worst:.2e}, "
              f"regular: lapack {np.max(errl[ref['regular']]):.2e}, floor {np.max(ref['floor'][ref['regular']]):.2e}")
        assert worst < 1.0 / 16.0, (i, int(np.argmax(np.maximum(errl - ends, 0.0) / ref["hard"])))
        assert singular >= 3                     # the d = 0, 1e-9 and 1e-6 copies of this subset's site
        bad, _ = kr.judge(ref["draw_lapack"], ref)
        assert bad == []
    if c.get("cluster"):
        assert max(ref["kappa"] for _, ref, _ in out) > 1e6


def _spoiled(sub, ref, u, what):
    """LAPACK's draw of the synthetic state (q = 1, A = 1) with one operation of a kernel gone wrong."""
    f = sub.at(6.3, 0.0)
    n = sub.n
    zs = ref["zstar"][:, 0]
    g = f["Q64"] @ u
    m = f["P64"] @ g
    s = f["s64"].copy()
    if what == "last row pair dropped":
        m = f["P64"][:, :n - 2 + n % 2] @ g[:n - 2 + n % 2]
    elif what == "fabs for fmax":
        return m + np.sqrt(np.abs(1.0 - s)) * zs
    elif what == "s off by 1e-9":
        s = s + 1e-9
    elif what == "normal of the next site":
        zs = np.roll(zs, 1)
    return m + np.sqrt(np.maximum(1.0 - s, 0.0)) * zs


@pytest.mark.parametrize("what", ["last row pair dropped", "s off by 1e-9", "normal of the next site"])
def test_the_bars_catch_a_predictor_spoiled_in_one_place(what):
    """E1's 127-site subset, A = 1: a mean that loses its last row pair, an s off by 1e-9 (the flat 1e-8
    bar of the oracle tests passes both) and a normal taken from the neighbouring slot each break a bar,
    also as an interpolated arm."""
    pb, out = synthetic_state("E1")
    sub, ref, U = out[0]
    clean = _spoiled(sub, ref, U[:, 0], "nothing")
    assert np.array_equal(clean[:, None], ref["draw_lapack"])
    dev = _spoiled(sub, ref, U[:, 0], what)[:, None]
    for interpolated in (False, True):
        bad, fig = kr.judge(dev, ref, interpolated)
        print(what, "interpolated" if interpolated else "exact", fig["n_bad"], "sites;", bad[:1])
        assert bad, (what, interpolated)


def test_fabs_for_fmax_stays_inside_every_derived_bar():
    """What the bars cannot see.  sqrt(|1 - s|) for sqrt(max(1 - s, 0)) changes a draw only where the
    computed 1 - s is negative, at a d = 0 site, and there by |z*| sqrt(|rounding error of s|) -- what a
    correct kernel gives when the same rounding error comes out positive.  With s at the d = 0 site off
    by -/+ 3e-14 (inside B_s = 2.6e-11 there) both forms pass under either sign: no accuracy bar separates
    them, only `every draw is finite` guards the clamp."""
    pb, out = synthetic_state("E1")
    sub, ref, U = out[0]
    f = sub.at(6.3, 0.0)
    t0 = next(t for t, v in pb["special"].items() if v.startswith("subset 0 ") and v.endswith("+ 0"))
    m = f["P64"] @ (f["Q64"] @ U[:, 0])
    zs = ref["zstar"][:, 0]
    moved = []
    for delta in (-3e-14, 3e-14):
        s = f["s64"].copy()
        s[t0] = 1.0 + delta
        for clamp in (lambda x: np.maximum(x, 0.0), np.abs):
            dev = (m + np.sqrt(clamp(1.0 - s)) * zs)[:, None]
            bad, _ = kr.judge(dev, ref)
            assert bad == [], (delta, bad)
            moved.append(abs(dev[t0, 0] - ref["draw_lapack"][t0, 0]))
    print("d = 0 site", t0, "moved by", moved, "hard bar", ref["hard"][t0])
    assert moved[2] == 0 and 0 < moved[0] == moved[1] == moved[3] < ref["hard"][t0]
