"""tests/linalg_ref.py under test on the CPU, before any device result is judged against it: the 80-bit
Cholesky against closed forms, the generators against the streams they restate, and the metrics and
bounds against factors that are right and factors spoiled in one place."""
import numpy as np
import pytest
import scipy.linalg as sla

from oracle import spmvglm as om

import linalg_ref as lr

LD_EPS = float(np.finfo(np.longdouble).eps)


@pytest.mark.parametrize("n", [1, 2, 17, 130])
def test_chol_longdouble_of_min_ij_is_the_triangle_of_ones(n):
    """A_ij = min(i, j) (1-based) = T T^T with T the lower triangle of ones: every intermediate is a small
    integer, so the factor is exact and the log-determinant is exactly 0."""
    i = np.arange(1, n + 1)
    L, ld = lr.chol_longdouble(np.minimum.outer(i, i).astype(float))
    assert L.dtype == np.longdouble
    assert np.array_equal(L, np.tril(np.ones((n, n))))
    assert ld == 0


def test_chol_longdouble_logdet_of_diagonal_plus_rank_one():
    """det(D + u u^T) = det(D) (1 + u^T D^-1 u), evaluated in longdouble.  The bar n^2 eps_longdouble is
    4e-15 for 80-bit, far inside what a double factorisation of this matrix gives (n eps ld ~ 1e-11)."""
    n = 200
    rng = np.random.default_rng(4)
    d = rng.uniform(1.0, 50.0, size=n)
    u = rng.normal(size=n)
    L, ld = lr.chol_longdouble(np.diag(d) + np.outer(u, u))
    dl, ul = d.astype(np.longdouble), u.astype(np.longdouble)
    ref = np.sum(np.log(dl)) + np.log1p(np.sum(ul * ul / dl))
    assert abs(ld - ref) <= n * n * LD_EPS
    A = (np.diag(d) + np.outer(u, u)).astype(np.longdouble)      # the matrix as the factorisation saw it
    assert np.linalg.norm(L @ L.T - A) <= n * LD_EPS * np.linalg.norm(A)
    assert np.max(np.abs(np.triu(L, 1))) == 0


def test_chol_longdouble_refuses_an_indefinite_matrix():
    A = np.eye(5)
    A[3, 3] = -1.0
    with pytest.raises(np.linalg.LinAlgError):
        lr.chol_longdouble(A)


def test_exp_corr_keeps_the_stream_of_the_older_tests():
    """The literal text of _CHOL_RUN (tests/test_gpu_diag_syrk.py, tests/test_gpu_inv_deal.py)."""
    S, n = 5, 37
    rng = np.random.default_rng(11)
    c = rng.uniform(size=(S, n, 2))
    d = np.sqrt(((c[:, :, None, :] - c[:, None, :, :]) ** 2).sum(-1))
    A = np.exp(-(3.0 + rng.uniform(size=(S, 1, 1)) * 6.0) * d)
    assert np.array_equal(lr.exp_corr(S, n, 11), A)
    assert np.array_equal(lr.make_batch(S, n, "exp", 11, pick=(0, 4)), A[[0, 4]])
    assert not np.array_equal(lr.exp_corr(S, n, 12), A)


def test_matern_corr_against_the_oracle():
    S, n, phi, nu = 2, 90, 4.0, 1.9
    A = lr.matern_corr(S, n, 12, phi, nu)
    c = np.random.default_rng(12).uniform(size=(S, n, 2))
    for s in range(S):
        ref = om.correlation(om.distance_matrix(c[s], c[s]), phi, nu, 1)
        np.fill_diagonal(ref, 1.0)
        assert np.max(np.abs(A[s] - ref)) <= 1e-13
        assert np.array_equal(A[s], A[s].T) and np.all(np.diag(A[s]) == 1.0)
        sla.cholesky(A[s], lower=True)
    assert np.array_equal(lr.make_batch(S, n, "matern", 12), A)


def _lapack(A):
    L = sla.cholesky(A, lower=True)
    inv, info = sla.lapack.dpotri(L, lower=1)
    assert info == 0
    return L, 2.0 * np.sum(np.log(np.diag(L))), np.tril(inv) + np.tril(inv, -1).T


@pytest.mark.parametrize("kind,n", [("exp", 60), ("matern", 130)])
def test_metrics_pass_lapack_and_flag_one_spoiled_element(kind, n):
    A = lr.make_batch(1, n, kind, 3)[0]
    L, ld, inv = _lapack(A)
    m = lr.metrics(A, L, ld, inv)
    assert lr.violations(m, kind) == []
    assert m["kappa2"] == pytest.approx(np.linalg.cond(A, 2), rel=1e-6)
    # LAPACK against itself
    assert m["L_vs_lapack"] == 0 and m["ld_vs_lapack"] == 0 and m["inv_vs_lapack"] == 0
    assert m["backward"] == m["backward_lapack"] and m["inv_resid"] == m["inv_resid_lapack"]
    assert m["fwd_L"] == m["fwd_L_lapack"] and 0 < m["fwd_L"] <= (n + 1) * lr.EPS * m["kappa2"]
    assert "fwd_L" not in lr.metrics(A, L, ld, inv, forward=False)

    bad = L.copy()
    bad[n - 9, 7] += 1e-11                            # one element, far below the 1e-10 bar against LAPACK
    v = lr.violations(lr.metrics(A, bad, ld, inv), kind)
    assert any(s.startswith("backward residual") for s in v), v

    bad = L.copy()
    bad[3, 9] = 1e-300                                # a nonzero above the diagonal, invisible to any norm
    v = lr.violations(lr.metrics(A, bad, ld, inv), kind)
    assert any(s.startswith("triu(L, 1)") for s in v), v

    bad = inv.copy()
    bad[5, 2] = np.nextafter(bad[5, 2], np.inf)       # one ulp off symmetry
    v = lr.violations(lr.metrics(A, L, ld, bad), kind)
    assert v == ["inv is not bitwise symmetric"], v

    # a diagonal element of the inverse (stays symmetric).  The residual bar grows with kappa_2, so on
    # the Matern matrix (kappa_2 ~ 1e7 at this size) only a coarse fault shows; the exponential
    # matrices have the 1e-9 bar against LAPACK beside it.
    bad = inv.copy()
    bad[n // 2, n // 2] *= (1.0 + 1e-6) if kind == "exp" else 2.0
    v = lr.violations(lr.metrics(A, L, ld, bad), kind)
    assert any(s.startswith("inverse residual" if kind == "matern" else "|inv - inv_lapack|") for s in v), v

    v = lr.violations(lr.metrics(A, L, float("nan"), inv), kind)
    assert any(s.startswith("ld is not finite") for s in v), v
    v = lr.violations(lr.metrics(A, L, ld + 4 * (n + 1) * lr.EPS * m["kappa2"], inv), kind)
    assert any(s.startswith("log-determinant error") for s in v), v

    bad = L.copy()
    bad[n - 1, n - 1] = -bad[n - 1, n - 1]            # L L^T is unchanged by the sign
    v = lr.violations(lr.metrics(A, bad, ld, inv), kind)
    assert any(s.startswith("diag(L)") for s in v), v


def test_digest_sees_one_bit():
    a = np.linspace(0.0, 1.0, 12).reshape(3, 4)
    b = a.copy()
    b[2, 1] = np.nextafter(b[2, 1], 2.0)
    assert lr.digest(a) == lr.digest(a.copy()) == lr.digest(np.asfortranarray(a))
    assert lr.digest(a) != lr.digest(b)
