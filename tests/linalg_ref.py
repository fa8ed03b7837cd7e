"""References, inputs, metrics and bounds for the batched Cholesky / inverse tests
(tests/gpu_linalg_run.py, tests/test_gpu_linalg_policies.py): nothing here touches the device or the
library, and tests/test_linalg_ref.py puts this module itself under test on the CPU.

The bounds are derived, not measured (eps = 2^-52, N = n + 1 the order the device factors, with its
bordered row):
  backward residual of the factor   |A - L L^T|_F / |A|_F                 <= N eps
      (Higham, Accuracy and Stability of Numerical Algorithms, Thm 10.3, gamma_{n+1}, Frobenius norm)
  inverse residual                  |A inv - I|_F / (|A|_F |inv|_F)        <= N eps kappa_2(A)
      (dpotri-style inversion from a backward-stable factor)
  forward errors against the 80-bit factorisation: |L - L_ref|_F / |L_ref|_F and |ld - ld_ref|
                                                                           <= N eps kappa_2(A)
  exponential inputs also meet the project's bars against LAPACK: L and ld 1e-10,
  inverse 1e-9, relative."""
import hashlib

import numpy as np
import scipy.linalg as sla

EPS = float(np.finfo(np.float64).eps)
REL_L = 1e-10        # tests/test_gpu_linalg.py's REL
REL_INV = 1e-9       # tests/test_gpu_inv_deal.py's REL
FORWARD_MAX_N = 520  # chol_longdouble takes 0.3 s at this order


def chol_longdouble(A):
    """Right-looking Cholesky of one SPD matrix in np.longdouble (80-bit where the platform has it:
    eps 1.08e-19), column by column.  Returns (L, ld): the lower factor and 2 sum log diag L, both
    longdouble.  Raises numpy.linalg.LinAlgError at a pivot that is not positive."""
    a = np.array(A, dtype=np.longdouble)
    n = a.shape[0]
    if a.shape != (n, n):
        raise ValueError("square matrix expected")
    for j in range(n):
        d = a[j, j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        d = np.sqrt(d)
        a[j, j] = d
        a[j + 1:, j] /= d
        c = a[j + 1:, j]
        a[j + 1:, j + 1:] -= np.multiply.outer(c, c)
    L = np.tril(a)
    return L, 2 * np.sum(np.log(np.diag(L)))


def exp_corr(S, n, seed=11):
    """S exponential correlation matrices of n uniform sites each, decays 3..9: the generator and the
    random stream of _CHOL_RUN (tests/test_gpu_diag_syrk.py, tests/test_gpu_inv_deal.py, seed 11),
    one matrix at a time (no S x n x n x 2 intermediate), same bits."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(size=(S, n, 2))
    dec = 3.0 + rng.uniform(size=(S, 1, 1)) * 6.0
    A = np.empty((S, n, n))
    for s in range(S):
        A[s] = np.exp(-dec[s] * _dist(c[s]))
    return A


def matern_corr(S, n, seed, phi, nu):
    """S Matern correlation matrices (x^nu K_nu(x) / (2^(nu-1) Gamma(nu)), x = phi d, diagonal 1) of n
    sites uniform on the unit square."""
    import scipy.special as ssp
    rng = np.random.default_rng(seed)
    c = rng.uniform(size=(S, n, 2))
    A = np.empty((S, n, n))
    for s in range(S):
        x = phi * _dist(c[s])
        lo = np.tril_indices(n, -1)               # K_nu is the cost: the lower triangle, mirrored
        xl = x[lo]
        m = xl > 0
        rl = np.ones_like(xl)
        rl[m] = np.power(xl[m], nu) / (2.0 ** (nu - 1.0) * ssp.gamma(nu)) * ssp.kv(nu, xl[m])
        r = np.zeros_like(x)
        r[lo] = rl
        r += r.T
        np.fill_diagonal(r, 1.0)
        A[s] = r
    return A


def _dist(c):
    dx = c[:, None, 0] - c[None, :, 0]
    dy = c[:, None, 1] - c[None, :, 1]
    return np.sqrt(dx ** 2 + dy ** 2)


def make_batch(S, n, kind, seed, pick=None):
    """The batch of one case; kind "exp" or "matern" (phi = 4, nu = 1.9, the conditioning of
    configs[1]); pick: keep only these matrices of the batch of S."""
    A = exp_corr(S, n, seed) if kind == "exp" else matern_corr(S, n, seed, 4.0, 1.9)
    return A if pick is None else np.ascontiguousarray(A[list(pick)])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# numpy and scipy each bring an OpenBLAS with a thread pool of its own, and calls that alternate
# between the two leave one pool spinning against the other (measured: 0.3 s per matrix of any size
# instead of milliseconds).  The norms therefore stay out of BLAS, and tests/gpu_linalg_run.py, which
# measures thousands of matrices, runs both libraries single-threaded with one matrix per thread:
# numpy's products and eigenvalues release the interpreter lock, scipy's dpotrf / dpotri are short.
def _fro(x):
    return float(np.sqrt(np.einsum("ij,ij->", x, x)))      # einsum's own loop, not a BLAS dot


def _sym(low):
    return np.tril(low) + np.tril(low, -1).T


def metrics(A, L, ld, inv, forward=None):
    """Every figure the tests assert on, for one matrix: the device's (A, L, ld, inv) and LAPACK's
    dpotrf / dpotri of the same A beside them.  forward (default: n <= FORWARD_MAX_N) adds the forward
    errors against chol_longdouble.  Plain floats and bools (JSON)."""
    A = np.asarray(A, float)
    n = A.shape[0]
    nA = _fro(A)
    eye = np.eye(n)
    Ll, info = sla.lapack.dpotrf(A, lower=1, clean=1)
    if info != 0:
        raise np.linalg.LinAlgError(f"dpotrf info {info}")
    il, info = sla.lapack.dpotri(Ll, lower=1)
    if info != 0:
        raise np.linalg.LinAlgError(f"dpotri info {info}")
    il = _sym(il)
    ldl = float(2.0 * np.sum(np.log(np.diag(Ll))))
    ev = np.linalg.eigvalsh(A)
    m = {
        "n": int(n),
        "kappa2": float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf"),
        "min_pivot_lapack": float(np.min(np.diag(Ll))),
        "backward": _fro(A - L @ L.T) / nA,
        "inv_resid": _fro(A @ inv - eye) / (nA * _fro(inv)),
        "max_upper": float(np.max(np.abs(np.triu(L, 1)))) if n > 1 else 0.0,
        "min_diag": float(np.min(np.diag(L))),
        "inv_symmetric": bool(np.array_equal(inv, inv.T)),
        "ld": float(ld),
        "backward_lapack": _fro(A - Ll @ Ll.T) / nA,
        "inv_resid_lapack": _fro(A @ il - eye) / (nA * _fro(il)),
        "L_vs_lapack": _fro(L - Ll) / _fro(Ll),
        "ld_vs_lapack": abs(float(ld) - ldl) / max(1.0, abs(ldl)),
        "inv_vs_lapack": _fro(inv - il) / _fro(il),
    }
    if forward is None:
        forward = n <= FORWARD_MAX_N
    if forward:
        Lr, ldr = chol_longdouble(A)
        nr = np.linalg.norm(Lr)
        m["fwd_L"] = float(np.linalg.norm(np.asarray(L, np.longdouble) - Lr) / nr)
        m["fwd_L_lapack"] = float(np.linalg.norm(np.asarray(Ll, np.longdouble) - Lr) / nr)
        m["fwd_ld"] = float(abs(np.longdouble(float(ld)) - ldr))
        m["fwd_ld_lapack"] = float(abs(np.longdouble(ldl) - ldr))
    return m


def violations(m, kind):
    """The bounds of the module docstring that the metrics m of one matrix break (empty: none).
    NaNs break the bound they sit in."""
    N = m["n"] + 1
    out = []

    def need(ok, what):
        if not ok:
            out.append(what)

    need(m["max_upper"] == 0.0, f"triu(L, 1) is not zero: max {m['max_upper']:.3e}")
    need(m["min_diag"] > 0.0, f"diag(L) is not positive: min {m['min_diag']:.3e}")
    need(m["inv_symmetric"], "inv is not bitwise symmetric")
    need(np.isfinite(m["ld"]), f"ld is not finite: {m['ld']}")
    need(m["backward"] <= N * EPS, f"backward residual {m['backward']:.3e} > {N * EPS:.3e}")
    need(m["inv_resid"] <= N * EPS * m["kappa2"], f"inverse residual {m['inv_resid']:.3e} > {N * EPS * m['kappa2']:.3e}")
    if kind == "exp":
        need(m["L_vs_lapack"] <= REL_L, f"|L - L_lapack| {m['L_vs_lapack']:.3e} > {REL_L:.0e}")
        need(m["ld_vs_lapack"] <= REL_L, f"|ld - ld_lapack| {m['ld_vs_lapack']:.3e} > {REL_L:.0e}")
        need(m["inv_vs_lapack"] <= REL_INV, f"|inv - inv_lapack| {m['inv_vs_lapack']:.3e} > {REL_INV:.0e}")
    if "fwd_L" in m:
        bar = N * EPS * m["kappa2"]
        need(m["fwd_L"] <= bar, f"forward error of L {m['fwd_L']:.3e} > {bar:.3e}")
        need(m["fwd_ld"] <= bar, f"log-determinant error {m['fwd_ld']:.3e} > {bar:.3e}")
    return out
