"""NumPy / scipy.special restatement of the held-out validation rows of include/mk.h (log score, Brier
score, error rate), written from the definitions and independently of the kernels: the whole (states x
columns) matrices at once, scipy's logsumexp, expit / ndtr, xlogy / xlog1py and gammaln.

score_ref(samples, w_pred_samples, x_test, y, wt, p, link, first=1):
  samples          n.samples x P  p.beta.theta.samples (beta = the first p columns)
  w_pred_samples   C x n          the kriging draws of n consecutive iterations, C = q n_test columns
  x_test           C x p          the test rows' covariates
  y, wt            C              held-out successes and trials (wt = 0: not observed)
  first                           1-based iteration of the draws' first column
score_ref_p(p, y, wt):            p is n x C, its rows equally weighted states of p(y = 1)
Both return (row, pointwise): row = [n, lpd, brier, err, lconst], pointwise C x 2 = (pmean_c, lpd_c)."""
import numpy as np
from scipy.special import expit, gammaln, log_ndtr, logsumexp, ndtr, xlog1py, xlogy

NAMES = ["n", "lpd", "brier", "err", "lconst"]


def loglik(y, wt, eta, link):
    """The binomial log-likelihood term with the coefficient dropped; eta broadcasts against y, wt."""
    if link == "probit":
        return y * log_ndtr(eta) + (wt - y) * log_ndtr(-eta)
    if link != "logit":
        raise ValueError(link)
    return y * eta - wt * np.logaddexp(0.0, eta)


def loglik_p(y, wt, p):
    """The same at a probability: y log p + (wt - y) log1p(-p), a zero multiplier giving zero."""
    return xlogy(y, p) + xlog1py(wt - y, -p)


def linkinv(eta, link):
    return ndtr(eta) if link == "probit" else expit(eta)


def lconst(y, wt):
    return float(np.sum(gammaln(wt + 1.0) - gammaln(y + 1.0) - gammaln(wt - y + 1.0)))


def _close(pm, ell, finite, y, wt):
    """pm, ell: n x C matrices of p and of the likelihood terms; finite: C flags (every draw finite)."""
    n = pm.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        pmean = pm.sum(axis=0) / n
        lpd_c = logsumexp(ell, axis=0) - np.log(n)
    bad = ~finite | np.isnan(ell).any(axis=0)
    pmean = np.where(bad, np.nan, pmean)
    lpd_c = np.where(bad, np.nan, lpd_c)
    obs = wt > 0
    n_obs = float(obs.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        brier = float(((pmean[obs] - y[obs] / wt[obs]) ** 2).sum() / n_obs)
        wrong = np.where(pmean[obs] >= 0.5, wt[obs] - y[obs], y[obs])
        err = float(wrong.sum() / wt[obs].sum())
    lpd = float(lpd_c.sum())
    if bad.any():
        lpd = brier = err = np.nan
    return np.array([n_obs, lpd, brier, err, lconst(y, wt)]), np.stack([pmean, lpd_c], axis=1)


def score_ref(samples, w_pred_samples, x_test, y, wt, p, link, first=1):
    samples, w = np.asarray(samples, float), np.asarray(w_pred_samples, float)
    x_test = np.asarray(x_test, float)
    y, wt = np.asarray(y, float).ravel(), np.asarray(wt, float).ravel()
    n = w.shape[1]
    beta = samples[first - 1:first - 1 + n, :p]                  # n x p
    eta = beta @ x_test.T + w.T                                  # n x C
    return _close(linkinv(eta, link), loglik(y[None, :], wt[None, :], eta, link), np.isfinite(eta).all(axis=0), y, wt)


def score_ref_p(p, y, wt):
    p = np.asarray(p, float)
    y, wt = np.asarray(y, float).ravel(), np.asarray(wt, float).ravel()
    with np.errstate(invalid="ignore", divide="ignore"):
        ell = loglik_p(y[None, :], wt[None, :], p)
    return _close(p, ell, np.isfinite(p).all(axis=0), y, wt)
