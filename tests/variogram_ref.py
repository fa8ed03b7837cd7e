"""Reference for the empirical variogram (include/mk.h "empirical variogram"): a NumPy restatement in
longdouble, every sum by math.fsum.  No code is shared with the device or with the package.

For each unordered pair i < j: d = sqrt(dx^2 + dy^2) in longdouble, k = floor(d s) with the same double
s = n_bins / max_dist the entry point divides once; counted iff k < n_bins.  Per bin the count, the sum of
d and of every product (z_a(i) - z_a(j)) (z_b(i) - z_b(j)), and beside each sum the sum of the terms'
absolute values, which is what a bound on a fixed-order fp64 sum is stated in.  A longdouble term goes into
fsum as its double head and tail, so nothing of its 64 bits is dropped.
"""
import math

import numpy as np

LD = np.longdouble


def outcome_pairs(q):
    """(a, b), a >= b: the lower triangle column by column."""
    return [(a, b) for b in range(q) for a in range(b, q)]


def _fsum(t):
    hi = t.astype(np.float64)
    lo = (t - hi.astype(LD)).astype(np.float64)
    return math.fsum(hi.tolist() + lo.tolist())


def variogram(coords, z, n_bins, max_dist):
    """coords (n, 2), z (n, q).  Returns a dict: count [n_bins] (Python ints), n_in (pairs with d s < n_bins),
    sum_d, abs_d [n_bins], sum_zz, abs_zz [T][n_bins] (floats: fsum's correctly rounded sums), dist and gamma
    (NaN where the bin is empty), pairs, and edge_gap: the smallest |d s - round(d s)| over the pairs with d > 0
    (inf when there is none)."""
    coords = np.asarray(coords, dtype=np.float64)
    n = coords.shape[0]
    z = np.asarray(z, dtype=np.float64).reshape(n, -1)
    q = z.shape[1]
    s = LD(float(n_bins) / float(max_dist))
    i, j = np.triu_indices(n, 1)
    x, y = coords[:, 0].astype(LD), coords[:, 1].astype(LD)
    dx, dy = x[i] - x[j], y[i] - y[j]
    d = np.sqrt(dx * dx + dy * dy)
    ks = d * s
    pos = d > 0
    edge_gap = float(np.min(np.abs(ks[pos] - np.rint(ks[pos])))) if pos.any() else math.inf
    k = np.floor(ks)
    inside = k < n_bins
    kk = np.where(inside, k, -1).astype(np.int64)
    pairs = outcome_pairs(q)
    zl = z.astype(LD)
    dz = zl[i] - zl[j]
    count = [0] * n_bins
    sum_d, abs_d = np.zeros(n_bins), np.zeros(n_bins)
    sum_zz, abs_zz = np.zeros((len(pairs), n_bins)), np.zeros((len(pairs), n_bins))
    order = np.argsort(kk, kind="stable")
    bounds = np.searchsorted(kk[order], np.arange(n_bins + 1))
    for b in range(n_bins):
        sel = order[bounds[b]:bounds[b + 1]]
        count[b] = int(sel.size)
        if not sel.size:
            continue
        sum_d[b] = abs_d[b] = _fsum(d[sel])
        for t, (a, c) in enumerate(pairs):
            term = dz[sel, a] * dz[sel, c]
            sum_zz[t, b] = _fsum(term)
            abs_zz[t, b] = _fsum(np.abs(term))
    cnt = np.array(count, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.where(cnt > 0, sum_d / cnt, np.nan)
        gamma = np.where(cnt > 0, sum_zz / (2.0 * cnt), np.nan)
    return {"count": count, "n_in": int(inside.sum()), "sum_d": sum_d, "abs_d": abs_d, "sum_zz": sum_zz,
            "abs_zz": abs_zz, "dist": dist, "gamma": gamma, "pairs": pairs, "edge_gap": edge_gap}


def lattice(m=8):
    """The m x m lattice with spacing 1/m on [0, 1): site (ix, iy) at index ix m + iy.  With m a power of
    two every coordinate, difference, square and sum below is exact in fp64."""
    ix, iy = np.divmod(np.arange(m * m), m)
    return np.column_stack([ix / m, iy / m]), ix, iy
