"""The PSIS-LOO restatement tests/loo_ref.py on its own, and loo_compare (host NumPy): no device.

The restatement is what tests/test_gpu_loo.py holds the kernels to, so its own properties are pinned here: the
weights are a distribution, smoothing never raises a log-weight above the raw maximum, a constant row has
nothing to smooth, and the generalised-Pareto fit recovers a known shape."""
import numpy as np
import pytest
from scipy.special import logsumexp

from loo_ref import NAMES, gpd_fit, loo_compare_ref, loo_ref, loo_total, psis, tail_length


def _bern(rng, n, N, sd):
    eta = rng.normal(0.3, sd, (n, N))
    y = (np.arange(N) % 2).astype(float)
    return y[None, :] * eta - np.logaddexp(0.0, eta)


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
@pytest.mark.parametrize("n,sd", [(25, 1.0), (100, 3.0), (1251, 3.0)])
def test_weights_are_a_distribution(n, sd, dtype):
    ell = _bern(np.random.default_rng(n), n, 40, sd)
    r, l, khat = psis(ell, dtype)
    assert r.dtype == dtype and khat.dtype == dtype
    lw = r - logsumexp(r, axis=1)[:, None]
    np.testing.assert_allclose(np.exp(lw).sum(axis=1).astype(float), 1.0, rtol=1e-13)
    assert (r <= 0).all()                       # the raw maximum is r = 0: no smoothed value exceeds it
    M = tail_length(n)
    raw = np.sort(-ell.T, axis=1).astype(dtype)
    raw = raw - raw[:, -1:]
    assert np.array_equal(r[:, :n - M], raw[:, :n - M])                    # the body is untouched
    assert (np.diff(r[:, n - M:], axis=1) >= 0).all()                      # the smoothed tail is ordered
    assert np.isfinite(khat).all()


def test_tail_lengths():
    assert [tail_length(n) for n in (25, 26, 48, 100, 1251, 2048, 8192)] == [5, 5, 9, 20, 107, 136, 272]


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_constant_row(dtype):
    ell = np.full((48, 3), -0.625)
    ell[:, 1] = np.random.default_rng(0).normal(-1.0, 0.3, 48)
    rows, pw = loo_ref(ell, dtype=dtype)
    for i in (0, 2):
        assert pw[i, 1] == np.inf
        assert abs(float(pw[i, 0]) + 0.625) <= 4 * np.finfo(np.float64).eps
        assert abs(float(pw[i, 2]) + 0.625) <= 4 * np.finfo(np.float64).eps
    assert np.isfinite(pw[1]).all()
    assert rows[5] == np.inf and rows[6] == 2          # +inf counts as a bad k-hat


def test_constant_tail_with_a_varying_body():
    n = 100
    ell = np.linspace(-1.0, -0.1, n)[:, None].repeat(2, axis=1)
    ell[:tail_length(n) + 3, 0] = -2.5                 # the 20 smallest l (the tail) and three beyond it are equal
    _, pw = loo_ref(ell)
    assert pw[0, 1] == np.inf and np.isfinite(pw[1, 1])
    l = ell[:, 0]
    lw = -l - logsumexp(-l)
    assert abs(pw[0, 0] - logsumexp(l + lw)) <= 1e-14  # nothing smoothed: plain importance sampling


def test_pareto_shape_is_recovered():
    """20,000 generalised-Pareto ratios of shape 0.4 (ratio = 1 + x, x ~ Lomax(1/0.4)): k-hat within 0.05."""
    x = np.random.default_rng(1).pareto(1 / 0.4, 20000)
    full = np.sort(np.log1p(x))                        # above the cap of 8192 states: the fit is called directly
    M = tail_length(x.size)
    k, _ = gpd_fit((np.exp(full[-M:]) - np.exp(full[-M - 1]))[None, :])
    khat = (k[0] * M + 5) / (M + 10)
    print(f"k-hat on 20,000 draws, M = {M}: {khat:.4f}")
    assert abs(khat - 0.4) <= 0.05


def test_rows_and_total():
    rng = np.random.default_rng(5)
    ell = _bern(rng, 64, 30, 3.0)
    rows, pw = loo_ref(ell, lconst=1.5)
    assert len(NAMES) == 8 and rows.shape == (8,) and pw.shape == (30, 3)
    assert rows[0] == pw[:, 0].sum() and rows[4] == pw[:, 2].sum()
    assert rows[1] == rows[4] - rows[0] and rows[2] == -2 * rows[0] and rows[7] == 1.5
    np.testing.assert_allclose(rows[3], np.sqrt(30 * pw[:, 0].var(ddof=1)), rtol=1e-13)
    assert rows[1] > 0                                 # leaving an observation out costs fit
    one, _ = loo_ref(ell[:, :1])
    assert np.isnan(one[3])                            # N = 1: no variance
    ell[7, 3] = np.nan
    bad, bpw = loo_ref(ell)
    assert np.isnan(bpw[3]).all() and np.isnan(bad[:7]).all() and bad[7] == 0.0
    assert np.array_equal(np.delete(bpw, 3, axis=0), np.delete(pw, 3, axis=0))
    tot = loo_total(np.stack([rows, rows]))
    assert tot[0] == 2 * rows[0] and tot[5] == rows[5] and tot[3] == np.sqrt(2 * rows[3] ** 2)


@pytest.mark.parametrize("n", [24, 8193])
def test_state_limits(n):
    with pytest.raises(ValueError):
        loo_ref(np.zeros((n, 2)))


def test_loo_compare(mk):
    rng = np.random.default_rng(11)
    _, a = loo_ref(_bern(rng, 64, 50, 3.0))
    _, b = loo_ref(_bern(rng, 64, 50, 3.0))
    got = mk.loo_compare({"pointwise": a}, {"pointwise": [b[:20], b[20:]]})      # one array, or a list per subset
    diff, se, n_bad = loo_compare_ref(a, b)
    assert list(got) == ["elpd_diff", "se_diff", "n_k_bad"]
    np.testing.assert_allclose(got["elpd_diff"], diff, rtol=1e-13)
    np.testing.assert_allclose(got["se_diff"], se, rtol=1e-13)
    assert got["n_k_bad"] == n_bad and n_bad > 0
    back = mk.loo_compare({"pointwise": b}, {"pointwise": a})
    assert back["elpd_diff"] == -got["elpd_diff"] and back["n_k_bad"] == n_bad


def test_loo_compare_refuses_other_observations(mk):
    rng = np.random.default_rng(12)
    _, a = loo_ref(_bern(rng, 32, 10, 1.0))
    with pytest.raises(ValueError):
        mk.loo_compare({"pointwise": a}, {"pointwise": a[:9]})
    with pytest.raises(ValueError):
        mk.loo_compare({"pointwise": a}, {"total": np.zeros(8)})
