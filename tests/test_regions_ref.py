"""tests/regions_ref.py, the restatement the GPU tests of the areal prediction compare the device with, pinned
on the CPU by cases that can be checked by hand: a region of one site is the marginal kriging draw, two sites
have the 2 x 2 closed form, a region site placed on an observed site is conditionally determined (pivot 0,
zeroed column, v = u there), and over many synthetic states the sample covariance of v - mean approaches S."""
import numpy as np
import pytest

from oracle import philox
from oracle import spmvglm as om
from regions_ref import PIVOT_TOL, RegionRef, chol_pivot, grids, normalise, planes

Q, P = 1, 2


def _setup(n=40, T=6, seed=3):
    rng = np.random.default_rng(seed)
    coords = rng.uniform(size=(n, 2))
    ct = rng.uniform(size=(T, 2))
    xt = np.column_stack([np.ones(T), rng.standard_normal(T)])
    return rng, coords, ct, xt


def _row(beta, K, phi):
    return np.concatenate([beta, [K], [phi]])


def test_one_site_is_the_marginal_formula():
    rng, coords, ct, xt = _setup()
    ref = RegionRef(coords, ct, offsets=range(7))                 # six regions of one site
    w = rng.standard_normal(40)
    key = philox.make_key(11, 2)
    st = ref.state(_row([0.3, -0.2], 1.7, 6.0), w, Q, P, key, 5, xt)
    zeta = philox.predict_normal(key, np.arange(6), 5)
    marg = st["mean"][:, 0] + np.sqrt(1.0 - st["s"][:, 0]) * zeta
    assert np.abs(st["v"][:, 0] - marg).max() < 1e-14
    # r of a one-site region is that site's p: omega = 1
    eta = xt @ np.array([0.3, -0.2]) + np.sqrt(1.7) * marg
    assert np.abs(st["r"][:, 0] - 1.0 / (1.0 + np.exp(-eta))).max() < 1e-14
    assert not st["flagged"].any()


def test_two_sites_closed_form():
    S = np.array([[0.5, 0.2], [0.2, 0.4]])
    L, flagged = chol_pivot(S)
    l11 = np.sqrt(0.5)
    want = np.array([[l11, 0.0], [0.2 / l11, np.sqrt(0.4 - 0.04 / 0.5)]])
    assert not flagged and np.abs(L - want).max() < 1e-15
    # and through RegionRef: L of the region's S equals the closed form of that S
    rng, coords, ct, xt = _setup(T=2)
    ref = RegionRef(coords, ct, offsets=[0, 2])
    f = ref.at(7.0)["fac"][0]
    a, b, c = f["S"][0, 0], f["S"][1, 0], f["S"][1, 1]
    want = np.array([[np.sqrt(a), 0.0], [b / np.sqrt(a), np.sqrt(c - b * b / a)]])
    assert np.abs(f["L"] - want).max() < 1e-14
    # the first site keeps its marginal law: L[0, 0]^2 = 1 - s
    assert abs(f["L"][0, 0] ** 2 - (1.0 - ref.at(7.0)["s"][0])) < 1e-14


def test_site_on_an_observed_site_is_determined():
    rng, coords, ct, xt = _setup(T=3)
    ct[1] = coords[17]                                            # the region's second site is observed site 17
    ref = RegionRef(coords, ct, offsets=[0, 3])
    w = rng.standard_normal(40)
    K = 2.3
    st = ref.state(_row([0.1, 0.4], K, 5.5), w, Q, P, philox.make_key(4, 0), 9, xt)
    f = ref.at(5.5)["fac"][0]
    assert abs(f["S"][1, 1]) < 1e-12 and f["flagged"] and st["flagged"][0, 0]
    assert not f["L"][:, 1].any()                                 # the zeroed column
    assert f["L"][0, 0] > 0.1 and f["L"][2, 2] > 0.1              # the other sites keep their spread
    u17 = w[17] / np.sqrt(K)
    assert abs(st["v"][1, 0] - u17) < 1e-10                       # v = u at that site (kriging interpolates)
    # a tiny positive pivot below the tolerance is zeroed as well, one above it is kept
    L, fl = chol_pivot(np.array([[1.0, 0.0], [0.0, 0.5 * PIVOT_TOL]]))
    assert fl and L[1, 1] == 0.0
    L, fl = chol_pivot(np.array([[1.0, 0.0], [0.0, 4.0 * PIVOT_TOL]]))
    assert not fl and L[1, 1] == pytest.approx(2e-6)


def test_sample_covariance_approaches_S():
    """N = 4,000 synthetic states (the Philox iteration runs 0..N-1 at a fixed phi): C = cov(v - mean) is
    Wishart(S, N - 1) / (N - 1), so sd(C_ij) = sqrt((S_ij^2 + S_ii S_jj) / (N - 1)) <= sqrt(2 S_ii S_jj / (N - 1)).
    The bar is 5 of those standard errors per entry: with 15 distinct entries the chance of a false alarm is
    below 15 x 6e-7."""
    N, m = 4000, 5
    rng, coords, ct, xt = _setup(T=m)
    ref = RegionRef(coords, ct, offsets=[0, m])
    f = ref.at(6.0)["fac"][0]
    key = philox.make_key(99, 1)
    idx = np.arange(m)
    E = np.array([f["L"] @ philox.predict_normal(key, idx, it) for it in range(N)])      # v - mean per state
    C = np.cov(E.T)
    S = f["S"]
    se = np.sqrt((S * S + np.outer(np.diag(S), np.diag(S))) / (N - 1))
    assert (np.abs(C - S) <= 5.0 * se).all(), (np.abs(C - S) / se).max()
    assert (np.abs(E.mean(axis=0)) <= 5.0 * np.sqrt(np.diag(S) / N)).all()


def test_weights_grids_and_planes():
    om_ = normalise([0, 2, 5], [1.0, 3.0, 2.0, 0.0, 2.0], 5)
    assert om_.tolist() == [0.25, 0.75, 0.5, 0.0, 0.5]
    assert normalise([0, 3], None, 3).tolist() == [1.0 / 3.0] * 3
    d = np.array([[0.1, 0.2, 0.3, 0.4], [0.5, 0.5, 0.5, np.nan]])
    g = grids(d[:1])
    assert g.shape == (200, 1) and g[-1, 0] == 0.4 and g[99, 0] == pytest.approx(0.25)
    pl = planes(d, (0.25, 0.4))
    assert pl.shape == (2, 4) and pl[0, 0] == pytest.approx(0.25) and pl[0, 2:].tolist() == [0.5, 0.0]
    assert np.isnan(pl[1]).all()                                  # a non-finite draw: the column's planes are NaN


def test_matern_region_has_unit_diagonal():
    rng, coords, ct, xt = _setup(T=4)
    ref = RegionRef(coords, ct, offsets=[0, 4], matern=True)
    f = ref.at(6.0, 0.7)
    Rgg = f["fac"][0]["S"] + f["X"].T @ f["X"]
    assert np.abs(np.diag(Rgg) - 1.0).max() < 1e-14
    assert np.abs(Rgg - om.correlation(om.distance_matrix(ct, ct), 6.0, 0.7, om.COV_MATERN)).max() < 1e-14
