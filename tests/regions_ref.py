"""NumPy / SciPy restatement of the areal prediction of include/mk.h (the regional prevalence from kriging
draws that are joint across a region's sites), written from the definitions and from what a fit records --
p.beta.theta.samples and p.w.samples -- alone.  Nothing here touches the device or the library;
tests/test_regions_ref.py pins this module on the CPU.

For one subset, one kept state (row of p.beta.theta.samples: beta | K lower triangle | phi | nu; w = A u
location-major) and region g with sites t_1 < .. < t_m, per outcome h:
    A = chol(K),  u_i = A^-1 w_i,  R_h, P_h, R_h(g,g) by oracle.spmvglm.correlation (unit diagonal),
    X = L_R^-1 P',  z = L_R^-1 u_h            (triangular solves with the Cholesky factor L_R of R_h)
    mean_i = X_i . z,   S = R_h(g,g) - X_g' X_g
    L = chol_pivot(S): a pivot that is not > PIVOT_TOL zeroes that column and flags the factor
    zeta_i = oracle.philox.predict_normal(key, t_i q + h, iteration)
    v_i = mean_i + sum_{j <= i} L[i, j] zeta_j
then w*_i,a = sum_h v_i,h A[a,h], p = linkinv(x_test' beta + w*), r_g,a = sum_i omega_i p_i,a."""
import numpy as np
import scipy.linalg as sla

from oracle import philox
from oracle import spmvglm as om
from oracle.rstats import PROBS200, r_quantile7

from maps_ref import map_ref_grid
from score_ref import linkinv

PIVOT_TOL = 1e-12     # MK_REGION_PIVOT_TOL
MAXM = 128            # MK_REGION_MAXM


def chol_pivot(S, tol=PIVOT_TOL):
    """(L, flagged): the lower Cholesky factor of S in the given order, column by column; a pivot that is not
    > tol zeroes its column (that site is conditionally determined by the ones before it)."""
    S = np.array(S, dtype=np.float64)
    m = S.shape[0]
    L = np.zeros((m, m))
    flagged = False
    for j in range(m):
        piv = S[j, j] - np.dot(L[j, :j], L[j, :j])
        if not piv > tol:
            flagged = True
            continue
        d = np.sqrt(piv)
        L[j, j] = d
        for i in range(j + 1, m):
            L[i, j] = (S[i, j] - np.dot(L[i, :j], L[j, :j])) / d
    return L, flagged


def normalise(offsets, weights, n_test):
    """omega: weight / (the sum of its region's weights, added in index order)."""
    w = np.ones(n_test) if weights is None else np.asarray(weights, float)
    om_ = np.zeros(n_test)
    for g in range(len(offsets) - 1):
        a, b = int(offsets[g]), int(offsets[g + 1])
        s = 0.0
        for t in range(a, b):
            s = s + w[t]
        om_[a:b] = w[a:b] / s
    return om_


def recover_A(K_tri, q):
    K = np.zeros((q, q))
    k = 0
    for j in range(q):
        for i in range(j, q):
            K[i, j] = K[j, i] = K_tri[k]
            k += 1
    return np.sqrt(K) if q == 1 else np.linalg.cholesky(K)


class RegionRef:
    """One subset against fixed test sites and regions.  What depends on (phi, nu) only -- X, the kriging
    variance reduction s and every region's factor -- is memoised: phi repeats across kept states."""

    def __init__(self, coords, coords_test, offsets, weights=None, matern=False):
        self.coords = np.asarray(coords, float)
        self.ct = np.asarray(coords_test, float)
        self.offsets = [int(o) for o in offsets]
        self.G = len(self.offsets) - 1
        self.omega = normalise(self.offsets, weights, self.ct.shape[0])
        self.model = om.COV_MATERN if matern else om.COV_EXPONENTIAL
        self.D = om.distance_matrix(self.coords, self.coords)
        self.Dt = om.distance_matrix(self.ct, self.coords)          # T x n
        self.Dg = [om.distance_matrix(self.ct[a:b], self.ct[a:b]) for a, b in zip(self.offsets[:-1], self.offsets[1:])]
        self._memo = {}

    def at(self, phi, nu=0.0):
        key = (float(phi), float(nu))
        if key not in self._memo:
            R = om.correlation(self.D, phi, nu, self.model)
            np.fill_diagonal(R, 1.0)
            LR = np.linalg.cholesky(R)
            X = sla.solve_triangular(LR, om.correlation(self.Dt, phi, nu, self.model).T, lower=True)     # n x T
            fac = []
            for g, (a, b) in enumerate(zip(self.offsets[:-1], self.offsets[1:])):
                Rgg = om.correlation(self.Dg[g], phi, nu, self.model)
                np.fill_diagonal(Rgg, 1.0)
                S = Rgg - X[:, a:b].T @ X[:, a:b]
                L, flagged = chol_pivot(S)
                ev = np.linalg.eigvalsh(S)
                fac.append(dict(S=S, L=L, flagged=flagged, cond=float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")))
            self._memo[key] = dict(LR=LR, X=X, s=np.einsum("it,it->t", X, X), fac=fac)
        return self._memo[key]

    def state(self, row, w, q, p, key, iteration, x_test, link="logit"):
        """One kept state.  row: its p.beta.theta.samples row; w: its p.w.samples column; iteration 0-based.
        -> dict(r (G, q), flagged (G, q) bool, cond (G, q), v (T, q), mean (T, q), s (T, q), p (T, q))."""
        row = np.asarray(row, float)
        ntri = q * (q + 1) // 2
        T, n = self.ct.shape[0], self.coords.shape[0]
        A = recover_A(row[p:p + ntri], q)
        phi = row[p + ntri:p + ntri + q]
        nu = row[p + ntri + q:p + ntri + 2 * q] if self.model == om.COV_MATERN else np.zeros(q)
        U = sla.solve_triangular(A, np.asarray(w, float).reshape(n, q).T, lower=True).T     # u_i = A^-1 w_i
        idx = (np.arange(T)[:, None] * q + np.arange(q)[None, :]).reshape(-1)
        zeta = philox.predict_normal(key, idx, iteration).reshape(T, q)
        mean, v, s = np.zeros((T, q)), np.zeros((T, q)), np.zeros((T, q))
        flagged, cond = np.zeros((self.G, q), bool), np.zeros((self.G, q))
        for h in range(q):
            f = self.at(phi[h], nu[h])
            z = sla.solve_triangular(f["LR"], U[:, h], lower=True)
            mean[:, h] = f["X"].T @ z
            s[:, h] = f["s"]
            for g, (a, b) in enumerate(zip(self.offsets[:-1], self.offsets[1:])):
                L = f["fac"][g]["L"]
                for i in range(b - a):
                    acc = 0.0
                    for j in range(i + 1):
                        acc = acc + L[i, j] * zeta[a + j, h]
                    v[a + i, h] = mean[a + i, h] + acc
                flagged[g, h], cond[g, h] = f["fac"][g]["flagged"], f["fac"][g]["cond"]
        wstar = v @ A.T                                                                      # T x q
        xt = np.asarray(x_test, float)                                                       # (T q) x p, location-major
        eta = (xt @ row[:p]).reshape(T, q) + wstar
        pr = linkinv(eta, link)
        r = np.zeros((self.G, q))
        for g, (a, b) in enumerate(zip(self.offsets[:-1], self.offsets[1:])):
            for i in range(a, b):
                r[g] = r[g] + self.omega[i] * pr[i]
        # the marginal draw of every site (k_pred_draw's law): the same mean and normal, sd = sqrt(1 - s)
        vm = mean + np.sqrt(np.maximum(1.0 - s, 0.0)) * zeta
        pm = linkinv((xt @ row[:p]).reshape(T, q) + vm @ A.T, link)
        return dict(r=r, flagged=flagged, cond=cond, v=v, mean=mean, s=s, p=pr, p_marginal=pm)

    def window(self, samples, w_samples, q, p, seed, subset, first, last, x_test, link="logit"):
        """Iterations first..last (1-based, inclusive) of a recorded fit: draws (C3, n) with column c = g q + a,
        singular (C3,) counts, cond (n, G, q), s (n, T, q), p (T q, n) the sites' joint draws of p(y = 1) and
        p_marginal (T q, n) their marginal draws (p_pred_samples' law and layout)."""
        key = philox.make_key(seed, subset)
        draws, sing, conds, ss, ps, pms = [], np.zeros(self.G * q, dtype=np.int64), [], [], [], []
        for it in range(first - 1, last):
            st = self.state(samples[it], np.asarray(w_samples)[:, it], q, p, key, it, x_test, link)
            draws.append(st["r"].reshape(-1))
            sing += st["flagged"].reshape(-1)
            conds.append(st["cond"])
            ss.append(st["s"])
            ps.append(st["p"].reshape(-1))
            pms.append(st["p_marginal"].reshape(-1))
        return dict(draws=np.array(draws).T, singular=sing, cond=np.array(conds), s=np.array(ss), p=np.array(ps).T,
                    p_marginal=np.array(pms).T)


def grids(draws):
    """Type-7 quantiles at the 200 levels of draws (C3, n): 200 x C3."""
    return r_quantile7(np.asarray(draws, float).T, PROBS200, axis=0)


def planes(draws, thresholds=()):
    """C3 x (2 + J): mean, sd, exc_1..J of draws (C3, n) by the maps' formulas on values."""
    return map_ref_grid(np.asarray(draws, float).T, thresholds)
