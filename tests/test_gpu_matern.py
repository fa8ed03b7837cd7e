"""The device's Matern correlation, element by element, against the longdouble reference of
tests/matern_ref.py (trapezoid quadrature of the integral representation: no formula shared with
mk_corr.hpp's Temme series, CF2, reciprocal tables and Chebyshev tables, nor with scipy's kv; itself
checked against mpmath in tests/test_matern_ref.py), on both routes and both table configurations:

  candidate  k_cov_candidate<MATERN> (matern_tile)     built     the kernel builds its unbounded 100-interval
  kriging    k_pred_PT_matern                                     table itself (mk.correlation_batched's way)
                                                       stored    a session's way: k_matern_table /
                                                                 k_matern_table_list store a table bounded by
                                                                 phi x span, the tile workgroups load it

through mk.correlation_cross_batched, at 27 nu beside every branch point in nu (|mu| = 0.1, mu = +-0.5,
the guards at the integers, long recurrences) and at sites built around the branch points in x
(matern_ref.design: every table edge and x = 2 exactly and one ulp either side, every interval, x < 0.5
down to 1e-9, beyond the table up to 600, duplicated sites, a second 4,096-site chunk).  Every case
asserts from the reference side that its sites realise that (matern_ref.coverage_violations).

Bar per element:  |dev - ref| / ref <= 1e-13 + 2 * 2^-52 * cond(x)   (matern_ref's docstring: 1e-13 is
mk_corr.hpp's own claim, the second term the rounding of x = phi d carried to rho).  Also: R equals its
transpose bit for bit, nothing exceeds 1, everything is finite, a duplicated site gives exactly 1.0, and
the two configurations agree within twice the bar.

Each case prints `MATERN_PARITY route config nu: max rel, max rel / bar, x at that maximum`.  Measured
on an MI355X (max rel / bar; the oracle's column: scipy's kv against the same reference,
tests/test_matern_ref.py):

    nu                    candidate built       candidate stored      kriging built         kriging stored        oracle
                          rel/bar  max rel      rel/bar  max rel      rel/bar  max rel      rel/bar  max rel      max rel
    0.01                  0.124    1.608e-14    0.124    1.608e-14    0.129    1.675e-14    0.129    1.675e-14    5.120e-15
    0.05                  0.126    1.636e-14    0.126    1.636e-14    0.128    1.662e-14    0.128    1.662e-14    5.287e-15
    0.09999999990000001   0.125    1.619e-14    0.125    1.619e-14    0.129    1.669e-14    0.129    1.669e-14    6.681e-15
    0.1                   0.324    3.270e-14    0.324    3.270e-14    0.322    3.254e-14    0.322    3.254e-14    6.431e-15
    0.1000000001          0.124    1.605e-14    0.124    1.605e-14    0.129    1.681e-14    0.129    1.681e-14    8.732e-14
    0.21                  0.128    1.654e-14    0.128    1.654e-14    0.131    1.705e-14    0.131    1.705e-14    9.960e-14
    0.4999999999          0.127    1.636e-14    0.127    1.636e-14    0.127    1.646e-14    0.127    1.646e-14    7.496e-14
    0.5                   0.126    1.623e-14    0.126    1.623e-14    0.125    1.623e-14    0.125    1.623e-14    5.252e-16
    0.5000000001          0.126    1.625e-14    0.126    1.625e-14    0.131    1.693e-14    0.131    1.693e-14    1.140e-14
    0.7                   0.126    1.625e-14    0.126    1.625e-14    0.128    1.661e-14    0.128    1.661e-14    1.735e-14
    0.9                   0.129    1.663e-14    0.129    1.663e-14    0.124    1.603e-14    0.124    1.603e-14    2.138e-14
    0.9999999999          0.127    1.638e-14    0.127    1.638e-14    0.125    1.616e-14    0.125    1.616e-14    6.283e-15
    1.0                   0.127    1.641e-14    0.127    1.641e-14    0.126    1.619e-14    0.126    1.619e-14    2.282e-15
    1.0000000001          0.128    1.650e-14    0.128    1.650e-14    0.126    1.626e-14    0.126    1.626e-14    6.722e-15
    1.0001                0.127    1.638e-14    0.127    1.638e-14    0.130    1.680e-14    0.130    1.680e-14    9.802e-15
    1.1                   0.130    1.676e-14    0.130    1.676e-14    0.124    1.601e-14    0.124    1.601e-14    2.940e-14
    1.3                   0.130    1.680e-14    0.130    1.680e-14    0.124    1.606e-14    0.124    1.606e-14    2.305e-14
    1.5                   0.127    1.637e-14    0.127    1.637e-14    0.127    1.630e-14    0.127    1.630e-14    5.393e-16
    1.9                   0.125    1.610e-14    0.125    1.610e-14    0.128    1.644e-14    0.128    1.644e-14    7.197e-14
    2.0                   0.127    1.635e-14    0.127    1.635e-14    0.125    1.612e-14    0.125    1.612e-14    9.468e-16
    2.0000001             0.128    1.645e-14    0.128    1.645e-14    0.126    1.624e-14    0.126    1.624e-14    3.845e-15
    2.5                   0.137    1.757e-14    0.137    1.757e-14    0.133    1.710e-14    0.133    1.710e-14    7.549e-16
    3.4                   0.159    1.668e-14    0.159    1.668e-14    0.130    1.657e-14    0.130    1.657e-14    3.553e-15
    3.9                   0.220    2.198e-14    0.220    2.198e-14    0.126    1.614e-14    0.126    1.614e-14    3.314e-15
    4.0                   0.142    1.665e-14    0.142    1.665e-14    0.129    1.644e-14    0.129    1.644e-14    1.032e-15
    6.5                   0.316    3.164e-14    0.316    3.164e-14    0.139    1.764e-14    0.139    1.764e-14    1.728e-15
    10.0                  0.411    4.108e-14    0.411    4.108e-14    0.169    2.111e-14    0.169    2.111e-14    2.245e-15
    4,200 test sites (near, mixed):
    0.21                  kriging-long built   rel/bar 0.129    max rel 1.658e-14   at x 60.3557
    0.21                  kriging-long stored  rel/bar 0.129    max rel 1.658e-14   at x 60.3557
    1.0000000001          kriging-long built   rel/bar 0.135    max rel 1.733e-14   at x 65.3201
    1.0000000001          kriging-long stored  rel/bar 0.135    max rel 1.733e-14   at x 65.3201
    3.4                   kriging-long built   rel/bar 0.139    max rel 1.773e-14   at x 65.3201
    3.4                   kriging-long stored  rel/bar 0.139    max rel 1.773e-14   at x 65.3201
    exponential k_pred_PT: max rel / bar 0.202 (kruler), 0.633 (kcloud)

Before the two fixes in mk_corr.hpp that this table follows, the same run gave max rel 3.96e-09 at nu = 0.5,
1.5, 2.5, 6.5 (x = 2.2e-16; 5.4e-13 at x = 1.3e-8), 3.8e-09 at nu = 0.5 + 1e-10, 2.4e-12 at nu = 0.7 -- the
series' E = expm1(e) + 1 for mu < 0 at small x -- and values up to 1 + 31 ulps at nu >= 0.9 as x -> 0.
With MK_CH_N dropped from 12 to 10 on a scratch copy, 13 cases here fail (1.05e-13 .. at the table
edges, nu <= 0.21) while the 1e-10 tests of tests/test_gpu_linalg.py still pass.
"""
import numpy as np
import pytest

import matern_ref as mr

pytestmark = pytest.mark.gpu

LD = np.longdouble


def _coverage(names):
    for name in names:
        assert mr.coverage_violations(name) == [], name


def _run(mk, names, nu, stored, model="matern"):
    """R (candidate designs) or P^T (kriging designs) of the designs `names`, one point set each."""
    ds = [mr.design(n) for n in names]
    coords = np.stack([d["obs"] for d in ds])
    phi = np.array([d["phi"] for d in ds])
    krig = ds[0]["test"] is not None
    R, PT = mk.correlation_cross_batched(coords, phi, nu=None if nu is None else np.full(len(ds), nu), cov_model=model,
                                         coords_test=np.stack([d["test"] for d in ds]) if krig else None,
                                         stored_tables=stored, want_R=not krig)
    return PT if krig else R


def _judge_all(route, config, names, nu, out):
    """Every design's block against the reference; prints the case's record line; returns the violations."""
    bad, worst = [], dict(max_rel=0.0, max_ratio=0.0, x_at_ratio=0.0)
    for name, dev in zip(names, out):
        ref, cnd = mr.reference(name, nu)
        x = mr.x_of(name).astype(np.float64)
        v, fig = mr.judge(dev, ref, cnd, x)
        bad += [f"{route} {config} {name} nu {nu!r}: {m}" for m in v]
        i, j = mr.design(name)["dup"]
        if dev[i, j] != 1.0:
            bad.append(f"{route} {config} {name}: duplicated site ({i}, {j}) gives {dev[i, j]!r}, not 1.0")
        worst["max_rel"] = max(worst["max_rel"], fig["max_rel"])
        if fig["max_ratio"] >= worst["max_ratio"]:
            worst["max_ratio"], worst["x_at_ratio"] = fig["max_ratio"], fig["x_at_ratio"]
    print(f"MATERN_PARITY {route} {config} {nu!r}: max rel {worst['max_rel']:.3e}, max rel/bar {worst['max_ratio']:.3f}, "
          f"x {worst['x_at_ratio']:.17g}")
    return bad


def _agree(route, names, nu, a, b):
    """The two table configurations within twice the bar of each other."""
    bad = []
    for name, da, db in zip(names, a, b):
        ref, cnd = mr.reference(name, nu)
        rel = (np.abs(da.astype(LD) - db.astype(LD)) / ref).astype(np.float64)
        k = ~(rel <= 2.0 * mr.bar(cnd))
        if np.any(k):
            i = tuple(np.argwhere(k)[0])
            bad.append(f"{route} {name} nu {nu!r}: built and stored tables differ by {rel[i]:.3e} at {i} ({int(k.sum())} elements)")
    return bad


@pytest.mark.parametrize("nu", mr.NUS)
def test_candidate_route(mk, nu):
    """k_cov_candidate<MATERN> at 200 sites (two 128-tiles, the border row inside the second), designs
    ruler, cloud and patch, tables built in the kernel and stored by k_matern_table."""
    names = mr.CANDIDATE_DESIGNS
    _coverage(names)
    built, stored = _run(mk, names, nu, False), _run(mk, names, nu, True)
    today = mk.correlation_batched(np.stack([mr.design(n)["obs"] for n in names]), [mr.design(n)["phi"] for n in names],
                                   nu=np.full(len(names), nu), cov_model="matern")
    bad = []
    if not np.array_equal(today, built):
        bad.append("mk.correlation_batched is not the built-in-kernel configuration bit for bit")
    for config, out in (("built", built), ("stored", stored)):
        bad += _judge_all("candidate", config, names, nu, out)
        for name, R in zip(names, out):
            if not np.array_equal(R, R.T):
                bad.append(f"candidate {config} {name}: R differs from its transpose")
            if not np.all(np.diag(R) == 1.0):
                bad.append(f"candidate {config} {name}: diagonal not 1")
    bad += _agree("candidate", names, nu, built, stored)
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("nu", mr.NUS)
def test_kriging_route(mk, nu):
    """k_pred_PT_matern at 40 observed sites (n_pad = 128: eight row groups, the last with padding rows)
    and 600 test sites, designs kruler and kcloud, tables built in the kernel and stored by
    k_matern_table_list."""
    names = mr.KRIG_DESIGNS
    _coverage(names)
    built, stored = _run(mk, names, nu, False), _run(mk, names, nu, True)
    bad = _judge_all("kriging", "built", names, nu, built) + _judge_all("kriging", "stored", names, nu, stored)
    bad += _agree("kriging", names, nu, built, stored)
    assert not bad, "\n".join(bad[:12])


@pytest.mark.parametrize("nu", mr.NUS_LONG)
def test_kriging_route_second_chunk(mk, nu):
    """4,200 test sites: the second 4,096-site chunk of k_pred_PT_matern's compaction.  near: every
    element exact (x < 0.5), so the first chunk's index list fills completely; mixed: exact and
    interpolated elements in both chunks."""
    names = mr.KRIG_LONG_DESIGNS
    _coverage(names)
    built, stored = _run(mk, names, nu, False), _run(mk, names, nu, True)
    bad = _judge_all("kriging-long", "built", names, nu, built) + _judge_all("kriging-long", "stored", names, nu, stored)
    bad += _agree("kriging-long", names, nu, built, stored)
    assert not bad, "\n".join(bad[:12])


def test_kriging_route_exponential(mk):
    """k_pred_PT<EXPONENTIAL> against exp(-phi d) in longdouble: relative error <= 2 eps (1 + x), eps =
    2^-52 (x = phi d carries a relative rounding of 2^-52 into the exponent, exp its own)."""
    names = mr.KRIG_DESIGNS
    _coverage(names)
    out = _run(mk, names, None, False, model="exponential")
    bad = []
    for name, dev in zip(names, out):
        x = mr.x_of(name)
        ref = np.exp(-x)
        rel = (np.abs(dev.astype(LD) - ref) / ref).astype(np.float64)
        b = 2.0 * mr.EPS * (1.0 + x.astype(np.float64))
        k = ~(rel <= b)
        print(f"MATERN_PARITY kriging exponential {name}: max rel {rel.max():.3e}, max rel/bar {(rel / b).max():.3f}")
        if np.any(k) or not np.all(np.isfinite(dev)) or np.any(dev > 1.0):
            bad.append(f"{name}: {int(k.sum())} elements over the bar, max rel/bar {(rel / b).max():.3f}")
        i, j = mr.design(name)["dup"]
        if dev[i, j] != 1.0:
            bad.append(f"{name}: duplicated site gives {dev[i, j]!r}")
    assert not bad, "\n".join(bad)
