"""The host arrays behind an mk_outputs and an mk_diagnostics (include/mk.h) and their way back to the
caller's layouts: one table of field -> shape serves Session.outputs and meta_fit_node."""
import numpy as np

from ._lib import (CRIT_NAMES, LOO_NAMES, MAP_BASE_NAMES, N_CRIT, N_DIAG, N_LEVELS, N_LOO, N_MAP_BASE, N_PAIR_BASE, N_SCORE,
                   PAIR_BASE_NAMES, REGION_BASE_NAMES, SCORE_NAMES, Criteria, Diagnostics, Loo, MapSpec, Maps, Outputs,
                   PairSpec, Pairs, Regions, RegionSpec, Scores, Validation, dptr, iptr)

# The array libmk fills for each mk_outputs field, row-major, in terms of: K subsets, P parameters,
# C = q n_test kriging columns, L levels, n = n_samples, kept states, B amcmc batches, R = P + 1
# acceptance rows, W = sum_i n_part[i] q n (the ragged w samples, flat).  R's column-major matrix is
# the transpose of the trailing two axes: per subset (K first), or one matrix (the sums).
SHAPES = {
    "parameters": ("K", "P", "L"),            # -> K x (200 x P)
    "w_predict": ("K", "C", "L"),             # -> K x (200 x q n_test)
    "samples": ("K", "P", "n"),               # -> K x (n_samples x P)
    "w_samples": ("W",),                      # -> subset i: (n_part[i] q) x n_samples
    "w_pred_samples": ("K", "kept", "C"),     # -> K x ((q n_test) x kept)
    "acceptance": ("K", "R", "B"),            # -> K x (n_batch x R)
    "w_predict_sum": ("C", "L"),              # -> 200 x q n_test
    "p_predict": ("K", "C", "L"),
    "p_pred_samples": ("K", "kept", "C"),
    "p_predict_sum": ("C", "L"),
}
# The same for the fields of mk_diagnostics (D = 3 rows: ess, mcse, rhat), keyed by the name the
# callers see: "<field>_diag" per subset, "<field>_diag_worst" over the call's subsets.
DIAG_SHAPES = {
    "parameters_diag": ("K", "P", "D"),       # -> K x (3 x P)
    "w_predict_diag": ("K", "C", "D"),        # -> K x (3 x q n_test)
    "p_predict_diag": ("K", "C", "D"),
    "parameters_diag_worst": ("P", "D"),      # -> 3 x P
    "w_predict_diag_worst": ("C", "D"),       # -> 3 x q n_test
    "p_predict_diag_worst": ("C", "D"),
}
# which struct a field belongs to, and its member there
STRUCT_OF = {**{f: ("outputs", f) for f in SHAPES},
             **{f: ("diagnostics", f.replace("_diag", "")) for f in DIAG_SHAPES}}


class OutputBuffers:
    """Arrays for the requested `fields` of K subsets (n_part sites each), `kept` states per draw
    array: `.c` is the mk_outputs pointing at them, `.buf[field]` the arrays, and unpack() -- after
    the library call -- the dict Session.outputs documents."""

    def __init__(self, K, cfg, n_part, n_test, kept, fields):
        unknown = set(fields) - set(SHAPES)
        if unknown:
            raise KeyError(f"unknown output fields {sorted(unknown)}")
        self.K, self.q, self.n_samples = int(K), cfg.q, cfg.n_samples
        self.n_part = [int(ns) for ns in n_part]
        dims = dict(K=self.K, P=cfg.P, C=cfg.q * int(n_test), L=N_LEVELS, n=cfg.n_samples, kept=int(kept),
                    B=cfg.n_batch, R=cfg.P + 1, W=sum(self.n_part) * cfg.q * cfg.n_samples)
        self.buf = {f: np.zeros(tuple(dims[d] for d in shape)) for f, shape in SHAPES.items() if f in fields}
        self.c = Outputs()
        for f, a in self.buf.items():
            setattr(self.c, f, dptr(a))


    def _unpack(self, a):
        if a.ndim == 3:
            return [a[i].T.copy() for i in range(self.K)]
        if a.ndim == 2:
            return a.T.copy()
        out, off = [], 0
        for ns in self.n_part:                                # the ragged w samples
            N = ns * self.q
            out.append(a[off:off + N * self.n_samples].reshape(self.n_samples, N).T.copy())
            off += N * self.n_samples
        return out

    def unpack(self):
        return {f: self._unpack(a) for f, a in self.buf.items()}


class DiagnosticBuffers(OutputBuffers):
    """The same for the requested `fields` of DIAG_SHAPES: `.c` is the mk_diagnostics pointing at the
    arrays, unpack() the per-subset lists of 3 x C arrays and the 3 x C worst arrays."""

    def __init__(self, K, cfg, n_test, fields):
        unknown = set(fields) - set(DIAG_SHAPES)
        if unknown:
            raise KeyError(f"unknown diagnostics fields {sorted(unknown)}")
        self.K = int(K)
        dims = dict(K=self.K, P=cfg.P, C=cfg.q * int(n_test), D=N_DIAG)
        self.buf = {f: np.zeros(tuple(dims[d] for d in shape)) for f, shape in DIAG_SHAPES.items() if f in fields}
        self.c = self.struct(self.buf)

    def struct(self, fields):
        """An mk_diagnostics pointing at the arrays of `fields` only (the rest NULL)."""
        c = Diagnostics()
        for f in fields:
            if f in self.buf:
                setattr(c, STRUCT_OF[f][1], dptr(self.buf[f]))
        return c


class CriteriaBuffers:
    """The arrays behind an mk_criteria of K subsets (n_part sites each, q outcomes): `.c` points at
    them; unpack() gives {'subsets': (K, 8), 'total': (8,), 'names': the rows' names} and, with
    pointwise, 'pointwise': per subset an (n_s q) x 2 array, columns lppd_i and M2_i / (n - 1)."""

    def __init__(self, K, q, n_part, pointwise=False):
        self.n_obs = [int(ns) * int(q) for ns in n_part]
        self.subsets = np.zeros((int(K), N_CRIT))
        self.total = np.zeros(N_CRIT)
        self.pointwise = np.zeros(2 * sum(self.n_obs)) if pointwise else None
        self.c = Criteria()
        self.c.subsets, self.c.total, self.c.pointwise = dptr(self.subsets), dptr(self.total), dptr(self.pointwise)

    def unpack(self):
        out = {"subsets": self.subsets.copy(), "total": self.total.copy(), "names": list(CRIT_NAMES)}
        if self.pointwise is not None:
            out["pointwise"], off = [], 0
            for N in self.n_obs:                              # column-major (n_s q) x 2 per subset
                out["pointwise"].append(self.pointwise[off:off + 2 * N].reshape(2, N).T.copy())
                off += 2 * N
        return out


class LooBuffers:
    """The arrays behind an mk_loo of K subsets (n_part sites each, q outcomes): `.c` points at them;
    unpack() gives {'subsets': (K, 8), 'total': (8,), 'names': the rows' names} and, with pointwise,
    'pointwise': per subset an (n_s q) x 3 array, columns elpd_loo_i, k-hat_i and lppd_i."""

    def __init__(self, K, q, n_part, pointwise=False):
        self.n_obs = [int(ns) * int(q) for ns in n_part]
        self.subsets = np.zeros((int(K), N_LOO))
        self.total = np.zeros(N_LOO)
        self.pointwise = np.zeros(3 * sum(self.n_obs)) if pointwise else None
        self.c = Loo()
        self.c.subsets, self.c.total, self.c.pointwise = dptr(self.subsets), dptr(self.total), dptr(self.pointwise)

    def unpack(self):
        out = {"subsets": self.subsets.copy(), "total": self.total.copy(), "names": list(LOO_NAMES)}
        if self.pointwise is not None:
            out["pointwise"], off = [], 0
            for N in self.n_obs:                              # column-major (n_s q) x 3 per subset
                out["pointwise"].append(self.pointwise[off:off + 3 * N].reshape(3, N).T.copy())
                off += 3 * N
        return out


def validation_arrays(y_test, weights_test, C):
    """Held-out data as libmk reads them: (y, wt, the mk_validation pointing at them), each q*n_test
    long, location-major; weights_test broadcasts (1: binary outcomes)."""
    y = np.ascontiguousarray(np.asarray(y_test, dtype=np.float64).reshape(-1))
    if y.shape != (int(C),):
        raise ValueError(f"error: y_test must have q*n_test = {int(C)} entries, not {y.size}")
    wt = np.ascontiguousarray(np.broadcast_to(np.asarray(weights_test, dtype=np.float64), (int(C),)))
    v = Validation()
    v.y_test, v.wt_test = dptr(y), dptr(wt)
    return y, wt, v


class ScoreBuffers:
    """The arrays behind an mk_scores of K subsets with C = q n_test test columns: `.c` points at them;
    unpack() gives {'subsets': (K, 5), 'names': the rows' names} and, with pointwise, 'pointwise': per
    subset a C x 2 array, columns pmean_c and lpd_c; with combined, 'combined' (the combined p grid's
    row by name) and, with pointwise too, 'combined_pointwise' (C x 2)."""

    def __init__(self, K, C, pointwise=False, combined=False):
        self.K, self.C = int(K), int(C)
        self.subsets = np.zeros((self.K, N_SCORE))
        self.pointwise = np.zeros((self.K, 2, self.C)) if pointwise else None
        self.combined = np.zeros(N_SCORE) if combined else None
        self.combined_pointwise = np.zeros((2, self.C)) if combined and pointwise else None
        self.c = Scores()
        self.c.subsets, self.c.pointwise = dptr(self.subsets), dptr(self.pointwise)
        self.c.combined, self.c.combined_pointwise = dptr(self.combined), dptr(self.combined_pointwise)

    def unpack(self):
        out = {"subsets": self.subsets.copy(), "names": list(SCORE_NAMES)}
        if self.pointwise is not None:
            out["pointwise"] = [self.pointwise[i].T.copy() for i in range(self.K)]
        if self.combined is not None:
            out["combined"] = dict(zip(SCORE_NAMES, self.combined.tolist()))
        if self.combined_pointwise is not None:
            out["combined_pointwise"] = self.combined_pointwise.T.copy()
        return out


def map_spec(thresholds):
    """Exceedance thresholds as libmk reads them: (the array, the mk_map_spec pointing at it).  libmk checks
    them (finite, at most MK_MAP_MAXT)."""
    u = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    m = MapSpec()
    m.thresholds, m.n_thresholds = (dptr(u) if u.size else None), int(u.size)
    return u, m


def map_names(J, base=MAP_BASE_NAMES):
    return list(base) + [f"exc_{j + 1}" for j in range(int(J))]


class MapBuffers:
    """The arrays behind an mk_maps of K subsets with C = q n_test test columns and J thresholds: `.c`
    points at them; unpack() gives {'names': w_mean, w_sd, p_mean, p_sd, exc_1..J, 'thresholds', 'subsets':
    per subset a C x (4 + J) array} and, with combined, 'combined' (C x (4 + J))."""

    def __init__(self, K, C, J, subsets=True, combined=False):
        self.K, self.C, self.J = int(K), int(C), int(J)
        n = N_MAP_BASE + self.J
        self.subsets = np.zeros((self.K, n, self.C)) if subsets else None
        self.combined = np.zeros((n, self.C)) if combined else None
        self.c = Maps()
        self.c.subsets, self.c.combined = dptr(self.subsets), dptr(self.combined)

    def unpack(self, thresholds=()):
        out = {"names": map_names(self.J), "thresholds": [float(u) for u in thresholds]}
        if self.subsets is not None:
            out["subsets"] = [self.subsets[i].T.copy() for i in range(self.K)]
        if self.combined is not None:
            out["combined"] = self.combined.T.copy()
        return out


def pair_list(q):
    """The outcome pairs (a, b), a < b, in include/mk.h's order: for a in 0..q-2: for b in a+1..q-1."""
    return [(a, b) for a in range(int(q) - 1) for b in range(a + 1, int(q))]


def pair_spec(thresholds):
    """Joint-exceedance thresholds as libmk reads them: (the array, the mk_pair_spec pointing at it).  libmk
    checks them as it checks the maps' (finite, at most MK_MAP_MAXT)."""
    u = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    m = PairSpec()
    m.n_thresholds, m.thresholds = int(u.size), (dptr(u) if u.size else None)
    return u, m


def pair_names(J):
    return list(PAIR_BASE_NAMES) + [f"joint_{j + 1}" for j in range(int(J))]


class PairBuffers:
    """The arrays behind an mk_pairs of K subsets of a q-outcome fit at n_test sites (C2 = n_pairs n_test
    pair columns, site-major) with J thresholds: `.c` points at them; unpack() gives {'names': both_mean,
    both_sd, diff_mean, diff_sd, corr, a_gt_b, joint_1..J, 'pairs': the (a, b) list, 'thresholds'} and what
    was asked for of 'both_predict' / 'diff_predict' (per subset 200 x C2), 'subsets' (per subset C2 x
    (6 + J)) and, with combined, 'combined_both' / 'combined_diff' (200 x C2)."""

    def __init__(self, K, q, n_test, J, grids=True, planes=True, combined=False):
        self.K, self.q, self.J = int(K), int(q), int(J)
        self.C2 = len(pair_list(q)) * int(n_test)
        g = (self.K, self.C2, N_LEVELS)
        self.both_predict = np.zeros(g) if grids else None
        self.diff_predict = np.zeros(g) if grids else None
        self.planes = np.zeros((self.K, N_PAIR_BASE + self.J, self.C2)) if planes else None
        self.combined_both = np.zeros(g[1:]) if combined else None
        self.combined_diff = np.zeros(g[1:]) if combined else None
        self.c = Pairs()
        for f in ("both_predict", "diff_predict", "planes", "combined_both", "combined_diff"):
            setattr(self.c, f, dptr(getattr(self, f)))

    def unpack(self, thresholds=()):
        out = {"names": pair_names(self.J), "pairs": pair_list(self.q), "thresholds": [float(u) for u in thresholds]}
        for f in ("both_predict", "diff_predict"):
            if getattr(self, f) is not None:
                out[f] = [getattr(self, f)[i].T.copy() for i in range(self.K)]
        if self.planes is not None:
            out["subsets"] = [self.planes[i].T.copy() for i in range(self.K)]
        for f in ("combined_both", "combined_diff"):
            if getattr(self, f) is not None:
                out[f] = getattr(self, f).T.copy()
        return out


def region_spec(offsets, n_test, weights=None, thresholds=()):
    """A region spec as libmk reads it: (offsets int32 [G + 1], weights float64 [n_test] or None, the
    thresholds, the mk_region_spec pointing at them).  libmk checks all of it (include/mk.h "areal
    prediction") and names the offending index."""
    off = np.ascontiguousarray(np.asarray(offsets).reshape(-1), dtype=np.int32)
    if off.size < 2:
        raise ValueError("error: offsets must hold G + 1 >= 2 entries")
    w = None
    if weights is not None:
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
        if w.size != int(n_test):
            raise ValueError(f"error: weights must hold one entry per test site ({int(n_test)}), not {w.size}")
    u = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1))
    m = RegionSpec()
    m.n_regions, m.offsets, m.weights = int(off.size - 1), iptr(off), dptr(w)
    m.n_thresholds, m.thresholds = int(u.size), (dptr(u) if u.size else None)
    return off, w, u, m


def region_names(J):
    return list(REGION_BASE_NAMES) + [f"exc_{j + 1}" for j in range(int(J))]


class RegionBuffers:
    """The arrays behind an mk_regions of K subsets of a q-outcome fit with G regions (C3 = G q region columns,
    region-major) and J thresholds over `kept` states: `.c` points at them; unpack() gives {'names': mean, sd,
    exc_1..J, 'thresholds', 'region_predict': per subset 200 x C3, 'subsets': per subset C3 x (2 + J),
    'singular': per subset C3 (int32), 'timing_ms': covariance-and-factor, draws, grids-and-planes} and, with
    samples, 'region_samples' (per subset C3 x kept)."""

    def __init__(self, K, q, G, J, kept, samples=False):
        self.K, self.q, self.G, self.J = int(K), int(q), int(G), int(J)
        self.C3 = self.G * self.q
        self.region_predict = np.zeros((self.K, self.C3, N_LEVELS))
        self.planes = np.zeros((self.K, 2 + self.J, self.C3))
        self.region_samples = np.zeros((self.K, int(kept), self.C3)) if samples else None
        self.singular = np.zeros((self.K, self.C3), dtype=np.int32)
        self.timing_ms = np.zeros(3)
        self.c = Regions()
        for f in ("region_predict", "planes", "region_samples", "timing_ms"):
            setattr(self.c, f, dptr(getattr(self, f)))
        self.c.singular = iptr(self.singular)

    def unpack(self, thresholds=()):
        out = {"names": region_names(self.J), "thresholds": [float(u) for u in thresholds],
               "region_predict": [self.region_predict[i].T.copy() for i in range(self.K)],
               "subsets": [self.planes[i].T.copy() for i in range(self.K)],
               "singular": [self.singular[i].copy() for i in range(self.K)], "timing_ms": self.timing_ms.copy()}
        if self.region_samples is not None:
            out["region_samples"] = [self.region_samples[i].T.copy() for i in range(self.K)]
        return out
