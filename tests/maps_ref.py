"""NumPy restatement of the posterior maps of include/mk.h (mean, sd and exceedance probabilities of w and
of p(y = 1) per test column), written from the definitions: an explicit loop over the states in time order
for the sums, Welford's recurrence as the header writes it, and p by the restated pred_prob of
tests/score_ref.py (linkinv of x'beta + w).

map_ref(samples, w_pred_samples, x_test, p, link, thresholds, first=1):
  samples          n.samples x P  p.beta.theta.samples (beta = the first p columns)
  w_pred_samples   C x n          the kriging draws of n consecutive iterations, C = q n_test columns
  x_test           C x p          the test rows' covariates
  first                           1-based iteration of the draws' first column
  -> C x (4 + J): w_mean, w_sd, p_mean, p_sd, exc_1..J
map_ref_grid(grid, thresholds):   grid is n x C, its rows equally weighted states
  -> C x (2 + J): mean, sd, exc_1..J
map_ref_p(...) as map_ref: the n x C matrix of restated p_kc (for the exceedance guard)."""
import numpy as np

from score_ref import linkinv

BASE_NAMES = ["w_mean", "w_sd", "p_mean", "p_sd"]


def names(J, base=BASE_NAMES):
    return list(base) + [f"exc_{j + 1}" for j in range(J)]


def moments(v):
    """v: n x C.  (mean, sd) per column: the sum in time order from zero over n; Welford's M2 over n - 1."""
    v = np.asarray(v, float)
    n, C = v.shape
    s, m, M2 = np.zeros(C), np.zeros(C), np.zeros(C)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, n + 1):
            x = v[k - 1]
            s = s + x
            d = x - m
            m = m + d / k
            M2 = M2 + d * (x - m)
        mean = s / n
        sd = np.sqrt(M2 / (n - 1)) if n > 1 else np.full(C, np.nan)
    return mean, sd


def exceedance(p, thresholds):
    """p: n x C.  C x J: the share of states with p > u, strictly."""
    p = np.asarray(p, float)
    n, C = p.shape
    out = np.zeros((C, len(thresholds)))
    with np.errstate(invalid="ignore"):
        for j, u in enumerate(thresholds):
            cnt = np.zeros(C)
            for k in range(n):
                cnt = cnt + (p[k] > u)
            out[:, j] = cnt / n
    return out


def map_ref_grid(grid, thresholds=()):
    g = np.asarray(grid, float)
    mean, sd = moments(g)
    out = np.column_stack([mean, sd, exceedance(g, thresholds)])
    out[~np.isfinite(g).all(axis=0)] = np.nan
    return out


def _eta(samples, w_pred_samples, x_test, p, first):
    samples, w = np.asarray(samples, float), np.asarray(w_pred_samples, float)
    n = w.shape[1]
    beta = samples[first - 1:first - 1 + n, :p]                  # n x p
    return beta @ np.asarray(x_test, float).T + w.T, w.T         # n x C each


def map_ref_p(samples, w_pred_samples, x_test, p, link, first=1):
    return linkinv(_eta(samples, w_pred_samples, x_test, p, first)[0], link)


def map_ref(samples, w_pred_samples, x_test, p, link, thresholds=(), first=1):
    eta, w = _eta(samples, w_pred_samples, x_test, p, first)
    pr = linkinv(eta, link)
    wm, ws = moments(w)
    pm, psd = moments(pr)
    out = np.column_stack([wm, ws, pm, psd, exceedance(pr, thresholds)])
    out[~(np.isfinite(w).all(axis=0) & np.isfinite(eta).all(axis=0))] = np.nan
    return out
