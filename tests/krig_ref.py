"""An 80-bit reference of the kriging predictor, its derived bounds and the hard geometries of
tests/test_gpu_krig_parity.py: nothing here touches the device or the library, and
tests/test_krig_ref.py puts this module itself under test on the CPU.

For one subset, one kept state (K = A A', phi_h, nu_h, w = A u as the session recorded them) and every
test site t (layouts: oracle/spmvglm.py fit_subset section 7), per outcome h
    s_h(t) = rho_h(t)' R_h^-1 rho_h(t),   m_h(t) = rho_h(t)' R_h^-1 u_h,   sd_h = sqrt(max(1 - s_h, 0)),
    draw_t = A (m_t + sd_t z*_t),         z* = oracle/philox.py predict_normal(key, site q + h, iteration)
in np.longdouble (80-bit where the platform has it): distances, exp, the Cholesky factor
(linalg_ref.chol_longdouble), X = L^-1 P', z = L^-1 u, s = colsum(X^2), m = X' z, lambda_t = R^-1 rho_t.
Matern correlations are matern_ref.rho_longdouble (a longdouble quadrature, no kv; 1 at d = 0), so the
reference is 80-bit throughout.  Beside it the same draw in float64 through LAPACK with the oracle's own
expressions: the error scale e_L.

The bounds are derived, not measured (eps = 2^-52, N = n_s + 1 the order the device factors, kappa =
kappa_2(R_h), per site t and outcome h, then the largest over h):
  B_s  = N eps kappa |rho_t| |lambda_t|       forward error of a Cholesky solve, |d lambda| <= N eps kappa
  B_m  = N eps kappa |lambda_t| |u_h|         |lambda|, applied to s = rho' lambda and m = lambda' u
  B_sd = min(sqrt(B_s), B_s / sd_ref)         |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b)
  floor = N eps max(1, |draw_ref|) + eps |A|_inf |lambda_t| |u_h|
                                              the second term: the session records w = A u rounded, the
                                              device krigs its own u
  hard bar (every site):    |dev - ref| <= |A|_inf (B_m + |z*| B_sd) + floor
  comparative bar (regular sites, sd_ref >= 0.05, per subset and state):
                            max_t |dev - ref| <= 16 max(max_t |lapack - ref|, max_t floor)
      16: the largest device-to-LAPACK ratio in the table of tests/test_gpu_linalg_policies.py is 15
      (backward residual 4.87e-15 against 3.25e-16, Matern S = 136), rounded up to a power of two.
      Near-singular sites get the hard bar only: there the sign of a rounding-level 1 - s decides
      between sd = 0 and sd ~ 1e-8, and LAPACK's luck with that sign is not a scale.
  phi-interpolated arms add |A|_inf |z*| tol / (sd_ref + sqrt(tol)) to both bars, tol = 1e-10
      (MK_KRIG_CHEB_TOL's default, mk_krig.hip cheb_tol: the interpolant's checked error in s).
  Matern adds 1e-13 kappa |rho_t| |lambda_t| to B_s and 1e-13 kappa |lambda_t| |u_h| to B_m: the
      device's Matern is within 1e-13 relative of the longdouble reference (tests/test_gpu_matern.py
      asserts it element by element, beside the rounding of x = phi d that N eps covers here)."""
import numpy as np
import scipy.linalg as sla

from oracle import philox
from oracle import spmvglm as om

from linalg_ref import EPS, chol_longdouble
from matern_ref import rho_longdouble

LD = np.longdouble
RATIO = 16.0          # the comparative bar's margin (module docstring)
REGULAR_SD = 0.05     # sites with sd_ref below this get the hard bar only
CHEB_TOL = 1e-10      # MK_KRIG_CHEB_TOL's default
KV_REL = 1e-13        # the device's Matern against matern_ref.rho_longdouble: asserted by tests/test_gpu_matern.py
OFFSETS = (0.0, 1e-9, 1e-6, 1e-3)


# ------------------------------------------------------------------ the 80-bit pieces
def dist_longdouble(c1, c2):
    c1, c2 = np.asarray(c1, dtype=LD), np.asarray(c2, dtype=LD)
    dx = c1[:, None, 0] - c2[None, :, 0]
    dy = c1[:, None, 1] - c2[None, :, 1]
    return np.sqrt(dx * dx + dy * dy)


def corr_longdouble(d, phi, nu, matern):
    """rho(d) in longdouble; Matern: matern_ref.rho_longdouble at x = phi d, 1 at d = 0."""
    if not matern:
        return np.exp(-LD(phi) * d)
    x = LD(phi) * np.asarray(d, dtype=LD)
    out = np.ones(x.shape, dtype=LD)
    m = x > 0
    out[m] = rho_longdouble(x[m], nu)
    return out


def forward_solve(L, B):
    """L^-1 B for lower L, all columns of B per pivot step (longdouble)."""
    B = np.array(B, dtype=LD)
    for j in range(L.shape[0]):
        B[j] /= L[j, j]
        if j + 1 < L.shape[0]:
            B[j + 1:] -= np.multiply.outer(L[j + 1:, j], B[j])
    return B


def back_solve(L, B):
    """L^-T B for lower L (longdouble)."""
    B = np.array(B, dtype=LD)
    for j in range(L.shape[0] - 1, -1, -1):
        B[j] /= L[j, j]
        if j > 0:
            B[:j] -= np.multiply.outer(L[j, :j], B[j])
    return B


def recover_A(K_tri, q, dtype=LD):
    """A from the reported lower triangle of K = A A' (column-major): sqrt for q = 1, else the lower
    Cholesky factor with a positive diagonal."""
    K = np.zeros((q, q), dtype=dtype)
    k = 0
    for j in range(q):
        for i in range(j, q):
            K[i, j] = K[j, i] = K_tri[k]
            k += 1
    if q == 1:
        return np.sqrt(K)
    if dtype is LD:
        return chol_longdouble(K)[0]
    return np.linalg.cholesky(K)


class SubsetRef:
    """Everything that depends on one subset's sites, the test sites and (phi_h, nu_h) only, memoised on
    (phi, nu): phi repeats across kept states whenever a candidate is rejected."""

    def __init__(self, coords, coords_test, matern=False):
        self.coords = np.asarray(coords, dtype=np.float64)
        self.coords_test = np.asarray(coords_test, dtype=np.float64)
        self.matern = bool(matern)
        self.n = self.coords.shape[0]
        self.D = dist_longdouble(self.coords, self.coords)
        self.Dt = dist_longdouble(self.coords_test, self.coords)          # (T, n)
        self.D64 = om.distance_matrix(self.coords, self.coords)
        self.Dt64 = om.distance_matrix(self.coords_test, self.coords)
        self._memo = {}

    def at(self, phi, nu=0.0):
        key = (float(phi), float(nu))
        if key not in self._memo:
            self._memo[key] = self._solve(*key)
        return self._memo[key]

    def _solve(self, phi, nu):
        model = om.COV_MATERN if self.matern else om.COV_EXPONENTIAL
        R = corr_longdouble(self.D, phi, nu, self.matern)
        P = corr_longdouble(self.Dt, phi, nu, self.matern)
        if self.matern:
            np.fill_diagonal(R, LD(1))
        L, _ = chol_longdouble(R)
        X = forward_solve(L, P.T)                                          # (n, T)
        lam = back_solve(L, X)                                             # R^-1 rho_t per column
        R64 = om.correlation(self.D64, phi, nu, model)
        P64 = om.correlation(self.Dt64, phi, nu, model)
        ev = np.linalg.eigvalsh(R64)
        L64 = np.linalg.cholesky(R64)
        X64 = sla.solve_triangular(L64, P64.T, lower=True)
        return dict(L=L, X=X, s=np.sum(X * X, axis=0), lam=lam,
                    rho_norm=np.sqrt(np.sum(P * P, axis=1)).astype(float),
                    lam_norm=np.sqrt(np.sum(lam * lam, axis=0)).astype(float),
                    kappa=float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf"),
                    P64=P64, s64=np.einsum("it,it->t", X64, X64), Q64=om.cho_inverse(L64))


def predict_state(sub, K_tri, phi, nu, w, key, iteration, site_index=None):
    """One subset (a SubsetRef), one kept state: the reference draw, the LAPACK draw and the bars.
    K_tri: the reported lower triangle of K; phi, nu: (q,) (nu ignored unless Matern); w: (n_s q,)
    location-major; key: philox.make_key(seed, subset); iteration: 0-based.  Arrays over the T test
    sites (and the q outcomes where per outcome)."""
    q = len(phi)
    n, T = sub.n, sub.coords_test.shape[0]
    N = n + 1
    site_index = np.arange(T, dtype=np.int64) if site_index is None else np.asarray(site_index, dtype=np.int64)
    idx = (site_index[:, None] * q + np.arange(q)[None, :]).reshape(-1)
    zs64 = philox.predict_normal(key, idx, iteration).reshape(T, q)
    zs = zs64.astype(LD)
    # 80-bit
    A = recover_A(np.asarray(K_tri, dtype=LD), q)
    U = forward_solve(A, np.asarray(w, dtype=LD).reshape(n, q).T).T       # u_i = A^-1 w_i
    m = np.zeros((T, q), dtype=LD)
    s = np.zeros((T, q), dtype=LD)
    Bm = np.zeros((T, q))
    Bs = np.zeros((T, q))
    lam_u = np.zeros((T, q))
    kappa = np.zeros(q)
    for h in range(q):
        f = sub.at(phi[h], nu[h] if sub.matern else 0.0)
        z = forward_solve(f["L"], U[:, h:h + 1])[:, 0]
        m[:, h] = f["X"].T @ z
        s[:, h] = f["s"]
        un = float(np.sqrt(np.sum(U[:, h] * U[:, h])))
        rel = N * EPS + (KV_REL if sub.matern else 0.0)
        Bs[:, h] = rel * f["kappa"] * f["rho_norm"] * f["lam_norm"]
        Bm[:, h] = rel * f["kappa"] * f["lam_norm"] * un
        lam_u[:, h] = f["lam_norm"] * un
        kappa[h] = f["kappa"]
    sd = np.sqrt(np.maximum(LD(1) - s, LD(0)))
    draw = (m + sd * zs) @ A.T
    # float64 through LAPACK, the oracle's expressions (fit_subset section 7 with a fresh g = Q u)
    A64 = recover_A(np.asarray(K_tri, dtype=np.float64), q, dtype=np.float64)
    U64 = sla.solve_triangular(A64, np.asarray(w, dtype=np.float64).reshape(n, q).T, lower=True).T
    m64 = np.zeros((T, q))
    sd64 = np.zeros((T, q))
    for h in range(q):
        f = sub.at(phi[h], nu[h] if sub.matern else 0.0)
        m64[:, h] = f["P64"] @ (f["Q64"] @ U64[:, h])
        sd64[:, h] = np.sqrt(np.maximum(1.0 - f["s64"], 0.0))
    draw64 = (m64 + sd64 * zs64) @ A64.T
    # the bars
    sdf = sd.astype(float)
    with np.errstate(divide="ignore", invalid="ignore"):
        Bsd = np.minimum(np.sqrt(Bs), np.where(sdf > 0, Bs / sdf, np.inf))
    normA = float(np.max(np.sum(np.abs(A.astype(float)), axis=1)))
    absz = np.abs(zs64)
    drawf = draw.astype(float)
    floor = N * EPS * np.maximum(1.0, np.max(np.abs(drawf), axis=1)) + EPS * normA * np.max(lam_u, axis=1)
    hard = normA * np.max(Bm + absz * Bsd, axis=1) + floor
    interp = normA * np.max(absz * CHEB_TOL / (sdf + np.sqrt(CHEB_TOL)), axis=1)
    return dict(draw=draw, draw_lapack=draw64, m=m, s=s, sd=sd, zstar=zs64, A=A, hard=hard, floor=floor, interp=interp,
                regular=np.min(sdf, axis=1) >= REGULAR_SD, kappa=float(np.max(kappa)), normA=normA)


def judge(dev, ref, interpolated=False):
    """A predictor's draws dev (T, q) of one subset and state against predict_state's ref: (violations,
    figures).  figures: the largest |dev - ref| and |lapack - ref| over the regular and over the
    near-singular sites, and the regular sites' comparative scale."""
    dev = np.asarray(dev, dtype=np.float64)
    out = []
    if not np.all(np.isfinite(dev)):
        out.append(f"{int(np.sum(~np.isfinite(dev)))} draws are not finite")
    err = np.max(np.abs(dev.astype(LD) - ref["draw"]), axis=1).astype(float)
    errl = np.max(np.abs(ref["draw_lapack"].astype(LD) - ref["draw"]), axis=1).astype(float)
    extra = ref["interp"] if interpolated else 0.0
    hard = ref["hard"] + extra
    bad = ~(err <= hard)
    for t in np.flatnonzero(bad)[:4]:
        out.append(f"hard bar, site {t}: |dev - ref| {err[t]:.3e} > {hard[t]:.3e} (sd_ref {float(np.min(ref['sd'][t])):.3e}, "
                   f"z* {ref['zstar'][t].tolist()}, lapack {errl[t]:.3e})")
    reg = ref["regular"]
    scale = max(float(np.max(errl[reg], initial=0.0)), float(np.max(ref["floor"][reg], initial=0.0)))
    comp = RATIO * scale + extra
    badc = reg & ~(err <= comp)
    for t in np.flatnonzero(badc)[:4]:
        out.append(f"comparative bar, site {t}: |dev - ref| {err[t]:.3e} > {RATIO:g} x {scale:.3e} "
                   f"(lapack {errl[t]:.3e}, floor {ref['floor'][t]:.3e})")
    fig = dict(kappa=ref["kappa"],
               dev_regular=float(np.max(err[reg], initial=0.0)), lapack_regular=float(np.max(errl[reg], initial=0.0)),
               dev_singular=float(np.max(err[~reg], initial=0.0)), lapack_singular=float(np.max(errl[~reg], initial=0.0)),
               scale=scale, hard_slack=float(np.max(err / hard)), n_bad=int(np.sum(bad) + np.sum(badc)))
    return out, fig


# ------------------------------------------------------------------ the hard geometries
# case -> model, q, subset sizes, test sites, arms (MK_KRIG_CHEB, predict_tile); tests/test_gpu_krig_parity.py
# says what each pins.  cluster: that many sites of the (single) subset inside a 1e-3 box.
CASES = {
    "E1": dict(model="exponential", q=1, sizes=(127, 129, 255, 2), n_test=261, seed=101,
               arms=(("0", 0), ("-1", 0), ("0", 256), ("-1", 256))),
    "E2": dict(model="exponential", q=1, sizes=(513,), n_test=None, n_fill=64, seed=102, arms=(("0", 0), ("-1", 256))),
    "E3": dict(model="exponential", q=1, sizes=(255,), n_test=261, seed=803, cluster=60, arms=(("0", 0), ("-1", 256))),
    "L1": dict(model="exponential", q=2, sizes=(129, 127), n_test=261, seed=104, arms=(("0", 0), ("-1", 256))),
    "M1": dict(model="matern", q=1, sizes=(200, 129), n_test=261, seed=105, arms=(("0", 0), ("0", 256))),
}
_EDGES = (0, 255, 256, -1, 1, 2, 3, 254, 257, 127, 128, 129, 130, 63, 64, 65, 191, 192, 193, 31, 32, 33, 95, 96, 97)


def problem(case):
    """The subsets (coords, y, weights, x as a Session takes them) and the test sites of one case, from
    numpy's generator alone.  Test sites: per subset one observed site with copies at x offsets OFFSETS
    (0: the site itself), (3, 3), (50, 50), one test site duplicated verbatim, the rest uniform on the
    unit square; the specials sit on tile and workgroup edges (indices 0, 255, 256, the last, 1..3, ...).
    Returns dict(subsets, coords_test, special: index -> what it is)."""
    c = CASES[case]
    q = c["q"]
    rng = np.random.default_rng(c["seed"])
    subsets = []
    for n in c["sizes"]:
        xy = rng.uniform(size=(n, 2))
        k = c.get("cluster", 0)
        if k:
            xy[:k] = np.array([0.4, 0.6]) + 1e-3 * rng.uniform(size=(k, 2))
        xcov = rng.standard_normal((n, q))
        X = np.zeros((n * q, 2 * q))
        for a in range(q):
            X[a::q, 2 * a] = 1.0
            X[a::q, 2 * a + 1] = xcov[:, a]
        y = (rng.uniform(size=n * q) < 1.0 / (1.0 + np.exp(-(X @ np.tile([0.5, -0.5], q))))).astype(np.float64)
        subsets.append(dict(coords=xy, y=y, weights=np.ones(n * q), x=X))
    specials = []
    for i, sb in enumerate(subsets):
        # the observed site: the first (inside the cluster where there is one), or the next with room in x
        j = next(j for j in range(sb["coords"].shape[0]) if sb["coords"][j, 0] < 0.9)
        for d in OFFSETS:
            specials.append((sb["coords"][j] + np.array([d, 0.0]), f"subset {i} site {j} + {d:g}"))
    specials.append((np.array([3.0, 3.0]), "(3, 3)"))
    specials.append((np.array([50.0, 50.0]), "(50, 50)"))
    n_test = c["n_test"] if c["n_test"] else c["n_fill"] + len(specials) + 1
    ct = rng.uniform(size=(n_test, 2))
    pos = []
    for e in _EDGES:
        e = e % n_test if e < 0 else e
        if e < n_test and e not in pos:
            pos.append(e)
    # order the specials so that a d = 0 site, a near one and the far ones take the first edges
    order = sorted(range(len(specials)), key=lambda k: (k % 4 if k < len(specials) - 2 else 0.5, k))
    special = {}
    for p, k in zip(pos, order):
        ct[p] = specials[k][0]
        special[p] = specials[k][1]
    p_dup = pos[len(specials)]
    src = next(t for t in range(4, n_test) if t not in special and t != p_dup)
    ct[p_dup] = ct[src]
    special[p_dup] = f"duplicate of test site {src}"
    return dict(subsets=subsets, coords_test=ct, special=special)
