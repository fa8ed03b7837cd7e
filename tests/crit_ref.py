"""NumPy / scipy.special restatement of the model-assessment rows of include/mk.h (DIC as spDiag
names its rows for the binomial family, and WAIC), written from the definitions and independently of
the kernels: the whole (observations x states) matrix of likelihood terms at once, a two-pass
variance, scipy's logsumexp and gammaln.

crit_ref(samples, w_samples, y, wt, X, p, link, window, thin):
  samples    n.samples x P   p.beta.theta.samples (beta = the first p columns)
  w_samples  N x n.samples   p.w.samples, N = n_s q observations (location-major)
  y, wt      N               successes and trials
  X          N x p           the design
  link       "logit" | "probit"
  window     (first, last)   1-based, inclusive
  thin       every thin-th state from `first`
Returns (rows, pointwise): rows = [bar.D, D.bar.Omega, pD, DIC, lppd, p.waic, WAIC, lconst],
pointwise N x 2 = (lppd_i, var_k l_ik with the n - 1 denominator)."""
import numpy as np
from scipy.special import gammaln, log_ndtr, logsumexp

NAMES = ["bar.D", "D.bar.Omega", "pD", "DIC", "lppd", "p.waic", "WAIC", "lconst"]


def loglik(y, wt, eta, link):
    """The binomial log-likelihood term with the coefficient dropped; eta broadcasts against y, wt."""
    if link == "probit":
        return y * log_ndtr(eta) + (wt - y) * log_ndtr(-eta)
    if link != "logit":
        raise ValueError(link)
    return y * eta - wt * np.logaddexp(0.0, eta)


def lconst(y, wt):
    return float(np.sum(gammaln(wt + 1.0) - gammaln(y + 1.0) - gammaln(wt - y + 1.0)))


def crit_ref(samples, w_samples, y, wt, X, p, link, window, thin=1):
    samples, w_samples = np.asarray(samples, float), np.asarray(w_samples, float)
    y, wt, X = np.asarray(y, float).ravel(), np.asarray(wt, float).ravel(), np.asarray(X, float)
    first, last = window
    idx = np.arange(first - 1, last, thin)
    n = idx.size
    if n < 2:
        raise ValueError("criteria need >= 2 states")
    beta = samples[idx, :p]                              # n x p
    w = w_samples[:, idx]                                # N x n
    ell = loglik(y[:, None], wt[:, None], X @ beta.T + w, link)      # N x n
    bar_d = float(np.mean(-2.0 * ell.sum(axis=0)))
    eta_hat = X @ beta.mean(axis=0) + w.mean(axis=1)
    d_hat = float(-2.0 * loglik(y, wt, eta_hat, link).sum())
    p_d = bar_d - d_hat
    lppd_i = logsumexp(ell, axis=1) - np.log(n)
    dev = ell - ell.mean(axis=1, keepdims=True)          # two-pass variance
    var_i = (dev * dev).sum(axis=1) / (n - 1)
    lppd, p_waic = float(lppd_i.sum()), float(var_i.sum())
    rows = np.array([bar_d, d_hat, p_d, bar_d + p_d, lppd, p_waic, -2.0 * (lppd - p_waic), lconst(y, wt)])
    return rows, np.stack([lppd_i, var_i], axis=1)
