"""NumPy restatement of the cross-outcome outputs of include/mk.h (per test site and pair of outcomes the
draws both = p_a p_b and diff = p_a - p_b, their 200-level grids and the planes), written from the
definitions and from a matrix of p draws alone -- a session's p_pred_samples, which are pred_prob's values
bit for bit, so products, differences and comparisons of them are the device's own numbers.  The planes
are two-pass (mean first, then centred sums), not the device's running recurrences.

  pair_list(q)                         the (a, b), a < b, in column order
  pair_draws(p, q)                     p: C x n (C = q n_test, location-major) -> (both, diff, pa, pb), each n x C2
  pair_grids(p, q)                     -> (both_predict, diff_predict), each 200 x C2
  pair_planes(p, q, thresholds=())     -> C2 x (6 + J): both_mean, both_sd, diff_mean, diff_sd, corr, a_gt_b, joint_1..J
C2 = n_pairs n_test; pair column e = t n_pairs + r (site-major)."""
import numpy as np

from oracle.rstats import PROBS200, r_quantile7

BASE_NAMES = ["both_mean", "both_sd", "diff_mean", "diff_sd", "corr", "a_gt_b"]


def names(J):
    return list(BASE_NAMES) + [f"joint_{j + 1}" for j in range(J)]


def pair_list(q):
    out = []
    for a in range(q - 1):
        for b in range(a + 1, q):
            out.append((a, b))
    return out


def pair_draws(p, q):
    p = np.asarray(p, float)
    C, n = p.shape
    assert C % q == 0
    pl = pair_list(q)
    sites = C // q
    pa = np.empty((n, sites * len(pl)))
    pb = np.empty_like(pa)
    for t in range(sites):
        for r, (a, b) in enumerate(pl):
            pa[:, t * len(pl) + r] = p[t * q + a]
            pb[:, t * len(pl) + r] = p[t * q + b]
    with np.errstate(invalid="ignore"):
        return pa * pb, pa - pb, pa, pb


def pair_grids(p, q):
    both, diff, _pa, _pb = pair_draws(p, q)
    return r_quantile7(both, PROBS200, axis=0), r_quantile7(diff, PROBS200, axis=0)


def _mean_sd(v):
    n = v.shape[0]
    mean = v.sum(axis=0) / n
    sd = np.sqrt(((v - mean) ** 2).sum(axis=0) / (n - 1)) if n > 1 else np.full(v.shape[1], np.nan)
    return mean, sd


def m2_ratio(p):
    """Per column of p (C x n): M2 / (n mean^2), the spread the corr test's guard asks for."""
    p = np.asarray(p, float)
    n = p.shape[1]
    mean = p.sum(axis=1) / n
    return ((p - mean[:, None]) ** 2).sum(axis=1) / (n * mean ** 2)


def pair_planes(p, q, thresholds=()):
    both, diff, pa, pb = pair_draws(p, q)
    n, C2 = pa.shape
    J = len(thresholds)
    out = np.empty((C2, 6 + J))
    with np.errstate(invalid="ignore", divide="ignore"):
        out[:, 0], out[:, 1] = _mean_sd(both)
        out[:, 2], out[:, 3] = _mean_sd(diff)
        da, db = pa - pa.sum(axis=0) / n, pb - pb.sum(axis=0) / n
        corr = (da * db).sum(axis=0) / (np.sqrt((da * da).sum(axis=0)) * np.sqrt((db * db).sum(axis=0)))
        # M2 is 0 exactly when the column never moved (Welford's d is then 0 in every state)
        still = (pa == pa[0]).all(axis=0) | (pb == pb[0]).all(axis=0)
        out[:, 4] = np.where(still | (n < 2), np.nan, corr)
        out[:, 5] = (pa > pb).sum(axis=0) / n
        for j, u in enumerate(thresholds):
            out[:, 6 + j] = ((pa > u) & (pb > u)).sum(axis=0) / n
    out[~(np.isfinite(pa).all(axis=0) & np.isfinite(pb).all(axis=0))] = np.nan
    return out
