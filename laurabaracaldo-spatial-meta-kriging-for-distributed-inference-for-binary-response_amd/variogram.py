"""Empirical variograms on device, and a phi prior read from them.

The reference sets phi's start and prior by hand (MK.R:60-63: ``phi = 3/0.5`` and ``Unif(3/0.75, 3/0.25)``,
an effective range of 0.5 on the unit square).  The usual advice for other data is to look at a variogram
of the start-value glm's residuals first; that variogram is an all-pairs job, which mk_variogram_compute
does on the device without subsampling (include/mk.h "empirical variogram").  The same verb gives the
variogram of held-out residuals after a fit -- spatial structure left there is misfit -- and, for q >= 2,
the cross-variograms that are the empirical counterpart of K = A A'.

Only ``variogram`` touches the device; the fit of the exponential model and the suggestion are host code
over at most 64 bins.
"""
import ctypes
import math

import numpy as np

from . import _lib
from ._lib import check, dptr
from .glm import glm_binomial

_GOLD = (math.sqrt(5.0) - 1.0) / 2.0


def tile_edge():
    """Edge of the pair kernel's tiles (MK_VG_EDGE): sizes around it are where its masks change."""
    return int(_lib.load().mk_variogram_tile_edge())


def outcome_pairs(q):
    """The T = q (q + 1) / 2 outcome pairs (a, b), a >= b, in the order of the gamma planes: the lower
    triangle column by column, as A and K are stored."""
    return [(a, b) for b in range(q) for a in range(b, q)]


def variogram(coords, z, n_bins=15, max_dist=None, device=0):
    """Matheron's estimator over all pairs of sites.  coords (n, 2); z (n,), (n, q) or location-major
    (n q,).  max_dist=None takes a third of the bounding box's diagonal (gstat's default).  Bins are
    half-open, [k max_dist / n_bins, (k + 1) max_dist / n_bins).  Returns {'h': mean distance per bin,
    'count', 'gamma': (T, n_bins), 'pairs': the (a, b) of the planes, 'edges': n_bins + 1, 'max_dist',
    'ms': device time of the launches}; an empty bin has count 0 and NaN in h and gamma."""
    lib = _lib.load()
    coords = np.asarray(coords, dtype=np.float64)
    if coords.ndim != 2 or coords.shape[1] != 2:
        raise ValueError(f"error: coords must be n x 2, not {coords.shape}")
    n = coords.shape[0]
    z = np.asarray(z, dtype=np.float64)
    if n < 1 or z.size % n:
        raise ValueError(f"error: z holds {z.size} values for {n} sites")
    q = z.size // n
    z = np.ascontiguousarray(z.reshape(n, q)) if q else z
    if max_dist is None:
        max_dist = float(np.hypot(*(coords.max(axis=0) - coords.min(axis=0)))) / 3.0
    n_bins, max_dist = int(n_bins), float(max_dist)
    T = q * (q + 1) // 2
    nb = max(n_bins, 1)
    count = np.zeros(nb, dtype=np.int64)
    h = np.zeros(nb)
    gamma = np.zeros((max(T, 1), nb))
    cf = np.ascontiguousarray(coords.ravel(order="F"))
    zf = np.ascontiguousarray(z.ravel())
    out = _lib.Variogram(count.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), dptr(h), dptr(gamma), 0.0)
    check(lib.mk_variogram_compute(dptr(cf), n, dptr(zf), q, n_bins, max_dist, ctypes.byref(out), int(device)))
    s = n_bins / max_dist
    return {"h": h, "count": count, "gamma": gamma, "pairs": outcome_pairs(q), "edges": np.arange(n_bins + 1) / s,
            "max_dist": max_dist, "n_bins": n_bins, "ms": float(out.ms)}


def _linkinv(eta, link):
    if link == "probit":
        return 0.5 * np.frompyfunc(math.erfc, 1, 1)(-eta / math.sqrt(2.0)).astype(np.float64)
    return 1.0 / (1.0 + np.exp(-eta))


def pearson_residuals(y, weights, p):
    """(y - wt p) / sqrt(wt p (1 - p)); NaN where wt = 0."""
    y = np.asarray(y, dtype=np.float64).ravel()
    wt = np.broadcast_to(np.asarray(weights, dtype=np.float64), y.shape)
    p = np.asarray(p, dtype=np.float64).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (y - wt * p) / np.sqrt(wt * p * (1.0 - p))
    return np.where(wt > 0, r, np.nan)


def glm_residuals(y, x, weights, link="logit", device=0):
    """Pearson residuals of the start-value glm (glm_binomial's coefficients), location-major like y.
    Rows with wt = 0 give NaN and are the caller's to drop."""
    coef = glm_binomial(y, x, weights, device=device, link=link)[0]
    return pearson_residuals(y, weights, _linkinv(np.asarray(x, dtype=np.float64) @ coef, link))


def _nonneg_fit(g, y, w):
    """min sum w (y - c0 - c g)^2 over c0, c >= 0: the free solution, else the better of the two edges."""
    sw, sg, sy = w.sum(), (w * g).sum(), (w * y).sum()
    sgg, sgy = (w * g * g).sum(), (w * g * y).sum()
    det = sw * sgg - sg * sg
    cands = []
    if det > 0:
        cands.append(((sgg * sy - sg * sgy) / det, (sw * sgy - sg * sy) / det))
    cands.append((0.0, max(sgy / sgg, 0.0) if sgg > 0 else 0.0))
    cands.append((max(sy / sw, 0.0), 0.0))
    best = None
    for c0, c in cands:
        if c0 < 0 or c < 0:
            continue
        sse = float((w * (y - c0 - c * g) ** 2).sum())
        if best is None or sse < best[0]:
            best = (sse, float(c0), float(c))
    return best


def fit_exponential(vg, pair=0, n_grid=512):
    """gamma(h) = c0 + c (1 - exp(-phi h)) by least squares weighted by the bins' counts.  phi is searched
    on a log grid of n_grid (at least 512) values between 3 / (2 max_dist) and 6 / h_1 (h_1 the first
    bin's mean distance), then refined by golden section between the best value's neighbours; c0, c >= 0
    in closed form per phi.  Returns {'nugget', 'psill', 'phi', 'range': 3 / phi, 'sse'}.  Host only."""
    keep = (np.asarray(vg["count"]) > 0) & np.isfinite(vg["gamma"][pair]) & (np.asarray(vg["h"]) > 0)
    h, y, w = vg["h"][keep], vg["gamma"][pair][keep], np.asarray(vg["count"], dtype=np.float64)[keep]
    if h.size < 3:
        raise ValueError(f"error: an exponential fit needs 3 bins with pairs, the variogram has {h.size}")
    lo, hi = 3.0 / (2.0 * float(vg["max_dist"])), 6.0 / float(h[0])
    if not hi > lo:
        hi = 2.0 * lo

    def sse_at(lphi):
        return _nonneg_fit(-np.expm1(-math.exp(lphi) * h), y, w)

    grid = np.linspace(math.log(lo), math.log(hi), max(int(n_grid), 512))
    k = int(np.argmin([sse_at(v)[0] for v in grid]))
    a, b = grid[max(k - 1, 0)], grid[min(k + 1, grid.size - 1)]
    c, d = b - _GOLD * (b - a), a + _GOLD * (b - a)
    fc, fd = sse_at(c)[0], sse_at(d)[0]
    for _ in range(100):
        if fc < fd:
            b, d, fd = d, c, fc
            c = b - _GOLD * (b - a)
            fc = sse_at(c)[0]
        else:
            a, c, fc = c, d, fd
            d = a + _GOLD * (b - a)
            fd = sse_at(d)[0]
    lphi = 0.5 * (a + b)
    best = sse_at(lphi)
    if sse_at(grid[k])[0] < best[0]:         # a flat floor: keep the grid's value
        lphi, best = grid[k], sse_at(grid[k])
    phi = math.exp(lphi)
    return {"nugget": best[1], "psill": best[2], "phi": phi, "range": 3.0 / phi, "sse": best[0]}


def suggest_phi(vg, fits=None):
    """phi's start and uniform prior per outcome, read from the direct variograms: starting = phi-hat and
    unif = (3 / (1.5 r), 3 / (0.5 r)) with r = 3 / phi-hat the fitted effective range -- the reference's
    own ratios: at r = 0.5 this is MK.R:60-63's 6 and (4, 12) exactly.  fits: the outcomes' fit_exponential
    results when they are already at hand.  Returns {'starting': (q,), 'unif': ((q,), (q,)), 'fits'}, the
    shapes SamplerConfig takes as phi_starting and phi_unif.

    This is exploratory.  A response-scale residual variogram of binary data is noisy and attenuated (the
    latent field is seen through one Bernoulli draw per site), so the fitted range is a guide to the prior's
    location and order of magnitude, not an estimate to trust: look at the table before using it."""
    if fits is None:
        diag = [t for t, (a, b) in enumerate(vg["pairs"]) if a == b]
        fits = [fit_exponential(vg, pair=t) for t in diag]
    r = np.array([f["range"] for f in fits], dtype=np.float64)
    return {"starting": np.array([f["phi"] for f in fits], dtype=np.float64), "unif": (3.0 / (1.5 * r), 3.0 / (0.5 * r)),
            "fits": list(fits)}


def residual_variogram(coords_test, y_test, wt_test, pmean, **kw):
    """The variogram of held-out Pearson residuals: pmean is Session.scores(pointwise=True)'s first column
    of a subset, or score_grid's of the combined grid ((q n_test,), location-major like y_test).  Sites
    with an unobserved outcome (wt = 0) are dropped before the call; kw goes to variogram."""
    coords_test = np.asarray(coords_test, dtype=np.float64)
    n = coords_test.shape[0]
    r = pearson_residuals(y_test, wt_test, pmean)
    if n < 1 or r.size % n:
        raise ValueError(f"error: {r.size} held-out values for {n} test sites")
    r = r.reshape(n, r.size // n)
    seen = ~np.isnan(r).any(axis=1)
    return variogram(coords_test[seen], r[seen], **kw)


def table(vg, pair=0):
    """The variogram of one outcome pair as lines of text: bin edges, pairs, mean distance, gamma."""
    a, b = vg["pairs"][pair]
    lines = [f"variogram of outcomes ({a}, {b}): {int(vg['count'].sum())} pairs within {vg['max_dist']:.6g}",
             f"{'from':>10} {'to':>10} {'pairs':>14} {'h':>10} {'gamma':>12}"]
    for k in range(vg["n_bins"]):
        lines.append(f"{vg['edges'][k]:10.4g} {vg['edges'][k + 1]:10.4g} {int(vg['count'][k]):14d} {vg['h'][k]:10.4g} "
                     f"{vg['gamma'][pair][k]:12.5g}")
    return "\n".join(lines)
