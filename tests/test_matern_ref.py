"""tests/matern_ref.py under test (CPU only): the longdouble Matern reference that judges the device in
tests/test_gpu_matern.py, against mpmath at 40 digits, against the closed forms of the half-integer
orders, its condition number against a difference quotient, and -- with the reference established -- the
oracle's own float64 correlation (scipy's kv), which every other test compares the device with.

The reference against mpmath (x^nu K_nu(x) / (2^(nu-1) Gamma(nu)), 27 nu x 15 x, x from 1e-9 to 600):
    largest relative error 6.9e-19 (nu = 10, x = 1e-8); the condition asserted is 2^-52 = 2.2e-16.

The oracle (om.correlation, float64 kv) against the reference over every point of the plane
(matern_ref.plane(): 3 candidate designs of 19,900 pairs, 2 kriging designs of 24,000, per nu; the two
kriging designs of 168,000 at three nu; each distinct x once), largest relative error per nu and the x where it is:
    nu                   max rel    x            nu             max rel    x
    0.01                 5.120e-15  1.99673      1.0001         9.802e-15  1.99035
    0.05                 5.287e-15  1.90912      1.1            2.940e-14  1.99351
    0.09999999990000001  6.681e-15  1.99244      1.3            2.305e-14  1.9794
    0.1                  6.431e-15  1.97507      1.5            5.393e-16  4.08003
    0.1000000001         8.732e-14  1.99425      1.9            7.197e-14  1.99896
    0.21                 9.960e-14  2            2.0            9.468e-16  1.98267
    0.4999999999         7.496e-14  1.99673      2.0000001      3.845e-15  1.97903
    0.5                  5.252e-16  27.7071      2.5            7.549e-16  0.078133
    0.5000000001         1.140e-14  1.99206      3.4            3.553e-15  5.55112e-17
    0.7                  1.735e-14  1.98504      3.9            3.314e-15  0.103868
    0.9                  2.138e-14  1.99673      4.0            1.032e-15  1.98267
    0.9999999999         6.283e-15  1.949        6.5            1.728e-15  0.105474
    1.0                  2.282e-15  1.97237      10.0           2.245e-15  1.95868
    1.0000000001         6.722e-15  1.98441
The condition asserted is 1e-11, a tenth of the tightest bar at which a test compares the device with
the oracle (REL = 1e-10, tests/test_gpu_linalg.py).  No point is left out: with x <= 600 and nu <= 10
the smallest rho is 2.9e-264."""
import numpy as np
import pytest

import matern_ref as mr
from oracle import spmvglm as om

LD = np.longdouble
X_SAMPLE = tuple(10.0 ** k for k in range(-9, 0)) + (0.5, 2.0, 10.0, 48.9, 200.0, 600.0)


def test_longdouble_is_wider_than_double():
    """The reference's claim rests on a 64-bit significand."""
    assert np.finfo(LD).eps <= 2.0 ** -63


def _to_mpf(mp, v):
    """A longdouble as an mpf, exactly: its leading 53 bits and the rest."""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))


def test_reference_against_mpmath():
    """rho at the tests' nu list x (the decades 1e-9 .. 1e-1, 0.5, 2, 10, 48.9, 200, 600) against mpmath at
    40 digits: relative error <= 2^-52, so the reference is at least 450 times finer than the 1e-13 it
    judges.  Measured: 6.9e-19 (module docstring).  Gamma alone as well."""
    mpm = pytest.importorskip("mpmath")
    mp = mpm.mp
    old = mp.dps
    mp.dps = 40
    try:
        worst, at = 0.0, None
        x = np.array(X_SAMPLE, dtype=LD)
        for nu in mr.NUS:
            rho, cnd = mr.rho_and_cond(x, nu)
            N = mp.mpf(nu)
            g = mr.gamma_longdouble(nu)
            assert abs(_to_mpf(mp, g) - mp.gamma(N)) / mp.gamma(N) <= 2.0 ** -58, nu
            for xv, rv, cv in zip(X_SAMPLE, rho, cnd):
                X = mp.mpf(xv)
                kn = mp.besselk(N, X)
                ref = X ** N * kn / (mp.mpf(2) ** (N - 1) * mp.gamma(N))
                err = float(abs(_to_mpf(mp, rv) - ref) / ref)
                if err > worst:
                    worst, at = err, (nu, xv)
                cref = X * mp.besselk(abs(N - 1), X) / kn
                assert float(abs(_to_mpf(mp, cv) - cref) / cref) <= 2.0 ** -52, (nu, xv)
        print(f"MATERN_REF mpmath: max rel {worst:.3e} at nu, x = {at}")
        assert worst <= 2.0 ** -52, (worst, at)
    finally:
        mp.dps = old


@pytest.mark.parametrize("nu,poly", [(0.5, lambda x: 1 + 0 * x), (1.5, lambda x: 1 + x), (2.5, lambda x: 1 + x + x * x / 3)])
def test_reference_against_closed_forms(nu, poly):
    """Half-integer orders in longdouble, with or without mpmath: exp(-x), (1 + x) exp(-x),
    (1 + x + x^2 / 3) exp(-x), on the mpmath sample and on a dense grid across the octave boundaries
    (where the reference changes its step and cut-off)."""
    x = np.concatenate([np.array(X_SAMPLE, dtype=LD), np.geomspace(LD(1e-9), LD(600), 4001),
                        LD(2) ** np.arange(-29, 10), np.nextafter(2.0 ** np.arange(-29, 10), 0.0).astype(LD)])
    ref = poly(x) * np.exp(-x)
    err = np.abs(mr.rho_longdouble(x, nu) - ref) / ref
    assert float(np.max(err)) <= 2.0 ** -52, (float(np.max(err)), float(x[np.argmax(err)]))


@pytest.mark.parametrize("nu", [0.05, 0.5, 1.0, 1.0 + 1e-10, 2.5, 10.0])
def test_cond_is_the_log_derivative(nu):
    """cond = -d log rho / d log x: against the central difference of log rho in longdouble (relative step
    1e-5: truncation ~ 1e-10 cond-scale, rounding ~ 1e-19 / 1e-5), to 1e-6."""
    x = np.geomspace(LD(1e-6), LD(600), 200)
    d = LD(1e-5)
    up, dn = mr.rho_longdouble(x * (1 + d), nu), mr.rho_longdouble(x * (1 - d), nu)
    quot = -(np.log(up) - np.log(dn)) / (np.log1p(d) - np.log1p(-d))
    c = mr.cond(x, nu)
    assert float(np.max(np.abs(quot - c) / (1 + c))) <= 1e-6


def test_designs_realise_their_purpose():
    """The coverage that tests/test_gpu_matern.py asserts per case, here without a device."""
    for name in mr.CANDIDATE_DESIGNS + mr.KRIG_DESIGNS + mr.KRIG_LONG_DESIGNS:
        assert mr.coverage_violations(name) == [], name


@pytest.mark.parametrize("nu", mr.NUS)
def test_oracle_correlation_against_reference(nu):
    """om.correlation (float64 scipy kv: the oracle's, and what krig_ref promoted before) over the whole
    plane, no point left out: relative error <= 1e-11.  Measured: <= 1.0e-13, worst at x = 2 where
    scipy's series ends (the table in the module docstring)."""
    names = mr.CANDIDATE_DESIGNS + mr.KRIG_DESIGNS + (mr.KRIG_LONG_DESIGNS if nu in mr.NUS_LONG else ())
    worst, at, count = 0.0, None, 0
    for name in names:
        x = mr.x_of(name)
        xf = np.unique(x[x > 0].astype(np.float64))       # the plane's x as float64: both sides get the same number
        ref = mr.rho_longdouble(xf.astype(LD), nu)
        got = om.correlation(xf, 1.0, nu, om.COV_MATERN)
        assert np.all(np.isfinite(got)) and np.all(got > 0)
        rel = (np.abs(got.astype(LD) - ref) / ref).astype(np.float64)
        count += rel.size
        k = int(np.argmax(rel))
        if rel[k] > worst:
            worst, at = float(rel[k]), float(xf[k])
    print(f"MATERN_ORACLE nu {nu!r}: max rel {worst:.3e} at x {at:.6g} ({count} points)")
    assert worst <= 1e-11, (nu, worst, at)
