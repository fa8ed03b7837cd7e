"""NumPy / scipy.special restatement of the PSIS-LOO rows of include/mk.h ("leave-one-out"), written from
the definitions there, Vehtari, Gelman and Gabry (2017) and Zhang and Stephens (2009), independently of the
kernels: the whole (observations x states) matrix at once, np.sort, scipy's logsumexp, a two-pass variance.

loo_ref(ell, lconst=0.0, dtype=np.float64):
  ell     n_states x n_obs   the log-likelihood terms, one observation per column
  dtype   np.float64 or np.longdouble (80-bit on x86: eps 1.08e-19) -- every step runs in it
Returns (rows, pointwise): rows = [elpd_loo, p_loo, looic, se_elpd_loo, lppd, k_max, n_k_bad, lconst],
pointwise n_obs x 3 = (elpd_loo_i, k-hat_i, lppd_i), both in dtype.  25 <= n_states <= 8192, else ValueError.

loo_total(rows): the total over subsets' rows (sums; the maximum of k_max; the root of the summed squares of
se_elpd_loo).  loo_compare_ref(a, b): loo_compare's three lines on two pointwise arrays."""
import numpy as np
from scipy.special import logsumexp

NAMES = ["elpd_loo", "p_loo", "looic", "se_elpd_loo", "lppd", "k_max", "n_k_bad", "lconst"]
MIN_STATES, MAX_STATES = 25, 8192


def tail_length(n):
    return min(n // 5, int(np.ceil(3.0 * np.sqrt(n))))


def gpd_fit(x, F=np.float64):
    """Zhang and Stephens' estimate as loo applies it, on rows of ascending exceedances x (N x M): (k, sigma)
    before the prior's shrinkage of k."""
    x = np.asarray(x, F)
    M = x.shape[1]
    G = 30 + int(np.floor(np.sqrt(M)))
    g = np.arange(1, G + 1, dtype=F)
    x_star = x[:, int(np.floor(M / 4 + 0.5)) - 1]
    theta = 1 / x[:, -1:] + (1 - np.sqrt(G / (g - F(0.5))))[None, :] / (3 * x_star)[:, None]        # N x G
    k_g = np.mean(np.log1p(-theta[:, :, None] * x[:, None, :]), axis=2, dtype=F)
    L = M * (np.log(-theta / k_g) - k_g - 1)
    omega = 1 / np.sum(np.exp(L[:, None, :] - L[:, :, None]), axis=2, dtype=F)
    theta_hat = np.sum(theta * omega, axis=1, dtype=F)
    k = np.mean(np.log1p(-theta_hat[:, None] * x), axis=1, dtype=F)
    return k, -k / theta_hat


def psis(ell, F=np.float64):
    """Per observation: (the smoothed log ratios sorted ascending, their l in the same order, k-hat)."""
    L = np.asarray(ell, F).T                                   # N x n
    N, n = L.shape
    M = tail_length(n)
    neg = np.sort(-L, axis=1)                                  # ascending -l: the tail is the last M
    r = neg - neg[:, -1:]
    tail, cut = r[:, n - M:], r[:, n - M - 1]
    varies = tail[:, -1] > tail[:, 0]
    khat = np.full(N, np.inf, dtype=F)
    if varies.any():
        ec = np.exp(cut[varies])
        k, sigma = gpd_fit(np.exp(tail[varies]) - ec[:, None], F)
        kh = (k * M + 5) / (M + 10)
        p = (np.arange(1, M + 1, dtype=F) - F(0.5)) / M
        q = sigma[:, None] * np.expm1(-kh[:, None] * np.log1p(-p)[None, :]) / kh[:, None]
        smooth = np.minimum(np.log(q + ec[:, None]), 0)
        fin = np.isfinite(kh)
        new = np.where(fin[:, None], smooth, tail[varies])
        r = r.copy()
        r[np.flatnonzero(varies)[:, None], np.arange(n - M, n)[None, :]] = new
        khat[varies] = kh
    return r, -neg, khat


def loo_ref(ell, lconst=0.0, dtype=np.float64):
    F = dtype
    E = np.asarray(ell, F)
    if E.ndim != 2:
        raise ValueError("ell is n_states x n_obs")
    n, N = E.shape
    if not (MIN_STATES <= n <= MAX_STATES):
        raise ValueError(f"PSIS-LOO takes {MIN_STATES} .. {MAX_STATES} states, not {n}")
    bad = ~np.isfinite(E).all(axis=0)
    E = np.where(bad[None, :], F(0), E)
    with np.errstate(all="ignore"):
        r, l, khat = psis(E, F)
        lw = r - logsumexp(r, axis=1)[:, None]
        elpd = logsumexp(l + lw, axis=1)
        lppd = logsumexp(l, axis=1) - np.log(F(n))
    pw = np.stack([elpd, khat, lppd], axis=1).astype(F)
    pw[bad] = np.nan
    rows = np.zeros(8, dtype=F)
    e = pw[:, 0]
    rows[0] = e.sum(dtype=F)
    rows[4] = pw[:, 2].sum(dtype=F)
    rows[1] = rows[4] - rows[0]
    rows[2] = -2 * rows[0]
    with np.errstate(all="ignore"):
        dev = e - rows[0] / N                                  # two-pass variance
        rows[3] = np.sqrt(N * (np.sum(dev * dev, dtype=F) / F(N - 1))) if N > 1 else np.nan
        rows[5] = np.fmax.reduce(pw[:, 1], initial=-np.inf)
    rows[6] = np.sum(pw[:, 1] > F(0.7))
    if bad.any():
        rows[:7] = np.nan
    rows[7] = lconst
    return rows, pw


def loo_total(rows):
    rows = np.asarray(rows)
    tot = rows.sum(axis=0)
    tot[5] = np.nan if np.isnan(rows[:, 5]).any() else rows[:, 5].max()
    tot[3] = np.sqrt(np.sum(rows[:, 3] ** 2))
    return tot


def loo_compare_ref(a, b):
    d = np.asarray(a)[:, 0] - np.asarray(b)[:, 0]
    return float(d.sum()), float(np.sqrt(d.size * d.var(ddof=1))), int(np.sum((a[:, 1] > 0.7) | (b[:, 1] > 0.7)))
