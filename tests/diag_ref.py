"""NumPy restatement of the chain diagnostics in include/mk.h (ess by Geyer's initial monotone
sequence, mcse of the column mean, split R-hat): the yardstick of tests/test_gpu_diagnostics.py and
tests/test_diagnostics_host.py.  It restates the formulas, not the kernel's summation order."""
import math

import numpy as np


def diag_ref(x):
    """x: n x C, time along axis 0.  Returns (out, aux): out 3 x C rows ess, mcse, rhat; aux 2 x C rows
    the smallest |Gamma_k| met at a stop / continue decision and the number of pairs added."""
    x = np.asarray(x, float)
    n, C = x.shape
    out = np.empty((3, C))
    aux = np.empty((2, C))
    for c in range(C):
        v = x[:, c]
        if not np.isfinite(v).all():
            out[:, c] = np.nan
            aux[:, c] = (np.inf, 0)
            continue
        m = v.sum() / n
        d = v - m
        c0 = np.dot(d, d) / n
        h = n // 2
        a, b = v[:h], v[n - h:]
        ma, mb = a.sum() / h, b.sum() / h
        va = np.dot(a - ma, a - ma) / (h - 1)
        vb = np.dot(b - mb, b - mb) / (h - 1)
        W = 0.5 * (va + vb)
        B = h * 0.5 * (ma - mb) ** 2
        if c0 == 0.0 or np.all(v == v[0]):          # the column never moved
            out[:, c] = (0.0, 0.0, np.inf)
            aux[:, c] = (np.inf, 0)
            continue
        rhat = math.sqrt(((h - 1) / h * W + B / h) / W) if W > 0 else np.inf
        prev, tau, k, mind = np.inf, -1.0, 0, np.inf
        while 2 * k + 1 <= n - 1:
            g = (np.dot(d[:n - 2 * k], d[2 * k:]) / n + np.dot(d[:n - 2 * k - 1], d[2 * k + 1:]) / n) / c0
            mind = min(mind, abs(g))
            if g <= 0:
                break
            g = min(g, prev)
            prev = g
            tau += 2 * g
            k += 1
        tau = max(tau, 1.0 / math.log10(n))
        ess = n / tau
        out[:, c] = (ess, math.sqrt(c0 * n / (n - 1) / ess), rhat)
        aux[:, c] = (mind, k)
    return out, aux


def ar1(rng, n, C, rho):
    """C stationary AR(1) chains x_i = rho x_{i-1} + e_i of length n (n x C)."""
    e = rng.standard_normal((n, C))
    x = np.empty((n, C))
    x[0] = e[0] / math.sqrt(1 - rho * rho)
    for i in range(1, n):
        x[i] = rho * x[i - 1] + e[i]
    return x
