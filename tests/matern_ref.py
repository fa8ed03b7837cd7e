"""A plain high-precision Matern correlation and the points at which the tests judge with it: nothing
here touches the device, the library, scipy's kv or mpmath, and tests/test_matern_ref.py puts this
module itself under test on the CPU.

    K_nu(x) = int_0^inf exp(-x cosh t) cosh(nu t) dt        (x > 0, any real nu)

by the trapezoid rule in np.longdouble.  The integrand is even and entire, so the rule converges
geometrically: on the strip |Im t| <= a the integrand grows by at most exp(x a^2 / 2), the rule's error
is ~ exp(x a^2 / 2 - 2 pi a / h), least at a = 2 pi / (h x): exp(-2 pi^2 / (h^2 x)).  The step therefore
shrinks like 1 / sqrt(x): per binary octave o = floor(log2 x), h = (1/8) / max(1, sqrt(2^(o+1))), so
h^2 x <= 1/64 and the error term is far below 2^-64 (for x < 1 the strip is limited by |Im t| < pi / 2,
where cosh leaves the right half plane: exp(-pi^2 / h) = e^-79).  The sum carries e^x K_nu (the exponent
is -x (cosh t - 1) = -2 x sinh^2(t / 2)), so nothing underflows before the final exp(-x), and it stops
at the first node T with x_min (cosh T - 1) - nu T >= 60: every term is positive, the terms past T are
below e^-60 of the one at t = 0.  No cancellation anywhere: the error is a few longdouble roundings.

    Gamma(z) = int exp(z t - e^t) dt over the real line, the same rule (h = 1/8) at z >= 2, and
    Gamma(nu) = Gamma(nu + k) / (nu (nu + 1) .. (nu + k - 1)).

Shares nothing with the device's Temme series, Steed's CF2, reciprocal tables or Chebyshev tables
(mk_corr.hpp), nor with scipy's kv.

The bar (judge):  |dev - ref| / ref <= 1e-13 + 2 * 2^-52 * cond(x),  cond = x K_|nu-1|(x) / K_nu(x).
1e-13 is the accuracy mk_corr.hpp claims for its tables (krig_ref.KV_REL builds on it).  The second term:
the device forms x = phi sqrt(dx^2 + dy^2) in fp64 -- five roundings, to first order |dx / x| <= 2 u =
2^-52 -- doubled for a square root or a product one ulp off; cond, the relative condition number of rho in
x (d/dx [x^nu K_nu] = -x^nu K_(nu-1)), carries it to rho: ~ x for large x, < 3 for x <= 2."""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
CLAIM = 1e-13          # mk_corr.hpp's claimed accuracy; krig_ref.KV_REL
_CUT = LD(60)

# the device's table geometry (mk_corr.hpp: MK_CH_NG, MK_CH_NI_MAX, MK_CH_E7), restated: the designs
# below are built around these edges, and the tests assert that they hit them
CH_NG, CH_NI, CH_E7 = 7, 100, 2.384185791015625
EDGES = np.array([0.5 * 1.25 ** g for g in range(CH_NG + 1)] + [CH_E7 + 0.5 * k for k in range(1, CH_NI - CH_NG + 1)])
X_SERIES = 2.0         # below: Temme's series, above: Steed's CF2


# ------------------------------------------------------------------ the quadrature
def gamma_longdouble(z):
    """Gamma(z), z > 0, in longdouble."""
    z = LD(z)
    div = LD(1)
    while z < 2:
        div *= z
        z += 1
    t = np.arange(-8 * 48, 8 * 8 + 1, dtype=LD) / LD(8)       # exp(z t) < e^-96 on the left, e^t > 2900 on the right
    return np.sum(np.exp(z * t - np.exp(t))) / LD(8) / div


def _octave_sums(x, o, nus):
    """e^x K_nu(x) for every nu of nus (a tuple of longdoubles >= 0) at x (1-d longdouble, all in the
    binary octave [2^o, 2^(o+1))): (len(nus), len(x))."""
    x_min = LD(2) ** o
    h = LD(1) / LD(8) / max(LD(1), np.sqrt(LD(2) ** (o + 1)))
    nu_max = max(nus)
    k = 1
    while True:
        T = k * h
        s = np.sinh(T / 2)
        if x_min * 2 * s * s - nu_max * T >= _CUT:
            break
        k += 1
    t = np.arange(k + 1, dtype=LD) * h
    s = np.sinh(t / 2)
    w = np.full(k + 1, h, dtype=LD)
    w[0] = h / 2
    out = np.empty((len(nus), len(x)), dtype=LD)
    c = 2 * s * s
    step = max(1, 2_000_000 // (k + 1))                         # bounded scratch
    for i0 in range(0, len(x), step):
        E = np.exp(-np.multiply.outer(x[i0:i0 + step], c))
        for j, nu in enumerate(nus):
            out[j, i0:i0 + step] = E @ (w * np.cosh(nu * t))
    return out


def kv_scaled(x, nus):
    """e^x K_nu(x) in longdouble for each nu of nus, x any shape, all > 0: (len(nus),) + x.shape."""
    x = np.asarray(x, dtype=LD)
    flat = x.reshape(-1)
    if flat.size and not np.all(flat > 0):
        raise ValueError("kv_scaled takes x > 0")
    nus = tuple(abs(LD(nu)) for nu in nus)
    out = np.empty((len(nus), flat.size), dtype=LD)
    if flat.size:
        oct_ = np.floor(np.log2(flat.astype(np.float64))).astype(np.int64)
        # log2 in float64 may round up across a power of two: the octave of a value just below one
        oct_ -= (flat < LD(2) ** oct_.astype(LD))
        for o in np.unique(oct_):
            m = oct_ == o
            out[:, m] = _octave_sums(flat[m], int(o), nus)
    return out.reshape((len(nus),) + x.shape)


def rho_longdouble(x, nu):
    """Matern rho = x^nu K_nu(x) / (2^(nu-1) Gamma(nu)) in longdouble; x all > 0 (the caller sets rho = 1
    at d = 0), nu > 0 taken at its float64 value."""
    return rho_and_cond(x, nu)[0]


def cond(x, nu):
    """x K_|nu-1|(x) / K_nu(x): the relative condition number of rho in x."""
    return rho_and_cond(x, nu)[1]


def rho_and_cond(x, nu):
    """(rho_longdouble, cond) from one pass over the nodes."""
    x = np.asarray(x, dtype=LD)
    nu = LD(nu)
    k = kv_scaled(x, (nu, nu - 1))
    den = LD(2) ** (nu - 1) * gamma_longdouble(nu)
    return np.power(x, nu) * k[0] * np.exp(-x) / den, x * k[1] / k[0]


# ------------------------------------------------------------------ the plane: nu list and site designs
_D = 1e-10
NUS = (0.01, 0.05, 0.1 - _D, 0.1, 0.1 + _D, 0.21, 0.5 - _D, 0.5, 0.5 + _D, 0.7, 0.9, 1.0 - _D, 1.0, 1.0 + _D, 1.0001, 1.1,
       1.3, 1.5, 1.9, 2.0, 2.0 + 1e-7, 2.5, 3.4, 3.9, 4.0, 6.5, 10.0)
NUS_LONG = (0.21, 1.0 + _D, 3.4)       # the kriging arms of 4,200 test sites
N_OBS, N_KRIG, N_TEST, N_TEST_LONG = 200, 40, 600, 4200
PHI = {"ruler": 8.0, "cloud": 6.5, "patch": 6.5, "near": 6.5, "mixed": 6.5}
_BOX = 0.02


def _ruler_specials():
    """x values the ruler must realise exactly and one ulp either side: every Chebyshev edge of the
    geometric part, the last edge of the table, and the series / continued-fraction switch."""
    xs = []
    for e in list(EDGES[:CH_NG + 1]) + [float(EDGES[-1]), X_SERIES]:
        xs += [np.nextafter(e, 0.0), e, np.nextafter(e, np.inf)]
    return np.array(xs)


def _ruler_positions(rng, n_in, n_out):
    """x-axis positions whose x = 8 * position is a multiple of 2^-20: n_in with x in [0, 50), n_out in
    [50, 600]."""
    xin = rng.integers(0, 50 << 20, size=n_in).astype(np.float64) / (1 << 20)
    xout = rng.integers(50 << 20, 600 << 20, size=n_out, endpoint=True).astype(np.float64) / (1 << 20)
    if n_out:
        xout[0] = 600.0
    return np.concatenate([xin, xout]) / PHI["ruler"]


def _on_axis(pos):
    return np.stack([pos, np.zeros_like(pos)], axis=1)


def _cloud(rng, n_box, n_wide, ladder):
    """n_box sites uniform in a 0.02 box (the last `ladder` of them copies of the first ones moved by
    2e-10 .. in decade steps, so the pairs' x reach down to 1e-9), n_wide uniform on [0, 8]^2."""
    box = rng.uniform(0.0, _BOX, size=(n_box, 2))
    for k in range(ladder):
        box[n_box - 1 - k] = box[k] + np.array([2e-10 * 10.0 ** k, 0.0])
    return np.concatenate([box, rng.uniform(0.0, 8.0, size=(n_wide, 2))])


@functools.lru_cache(maxsize=None)
def design(name):
    """Observed and test sites of one design: dict(phi, obs (n, 2), test (n_test, 2) or None, dup: the
    pair (i, j) of a duplicated site, i observed, j observed (candidate designs) or test).

    candidate route, 200 observed sites (two 128-tiles, the border row inside the second):
      ruler   phi = 8, sites on the x-axis at dyadic positions, x = 8 (a - b): the table edges, x = 2,
              each exactly and one ulp either side (against the site at 0), every interval, beyond the table
      cloud   phi = 6.5, 120 sites in a 0.02 box (a whole diagonal tile of exact elements) and 80 on [0, 8]^2
      patch   phi = 6.5, the unit square: phi x span = 9.2, so a stored table really is shorter
              (22 intervals) than the one built in the kernel (100)
    kriging route, 40 observed sites (n_pad = 128: eight row groups, the last with padding rows):
      kruler, kcloud   600 test sites, the same constructions between observed and test sites
      near    4,200 test sites, observed and test sites all inside the box: every x < 0.5
      mixed   4,200 test sites, cloud-like"""
    rng = np.random.default_rng({"ruler": 11, "cloud": 12, "patch": 13, "kruler": 14, "kcloud": 15, "near": 16,
                                 "mixed": 17}[name])
    if name == "ruler":
        sp = _ruler_specials() / PHI["ruler"]
        pos = np.concatenate([[0.0], sp, _ruler_positions(rng, N_OBS - 2 - len(sp) - 40, 40), [0.0]])
        pos[-1] = pos[40]                                           # the duplicate, across the tile edge
        return dict(phi=PHI["ruler"], obs=_on_axis(pos), test=None, dup=(N_OBS - 1, 40))
    if name == "cloud":
        obs = _cloud(rng, 120, N_OBS - 120, 8)
        obs[130] = obs[3]
        return dict(phi=PHI["cloud"], obs=obs, test=None, dup=(130, 3))
    if name == "patch":
        obs = rng.uniform(size=(N_OBS, 2))
        obs[150] = obs[7]
        return dict(phi=PHI["patch"], obs=obs, test=None, dup=(150, 7))
    if name == "kruler":
        sp = _ruler_specials() / PHI["ruler"]
        obs = np.concatenate([[0.0], _ruler_positions(rng, N_KRIG - 1, 0)])
        test = np.concatenate([sp, _ruler_positions(rng, N_TEST - len(sp) - 120, 120)])
        test[300] = obs[17]
        return dict(phi=PHI["ruler"], obs=_on_axis(obs), test=_on_axis(test), dup=(17, 300))
    if name == "kcloud":
        obs = _cloud(rng, 24, N_KRIG - 24, 0)
        test = _cloud(rng, 360, N_TEST - 360, 0)
        for k in range(8):
            test[k] = obs[k] + np.array([2e-10 * 10.0 ** k, 0.0])
        test[599] = obs[30]
        return dict(phi=PHI["cloud"], obs=obs, test=test, dup=(30, 599))
    if name == "near":
        obs = rng.uniform(0.0, _BOX, size=(N_KRIG, 2))
        test = rng.uniform(0.0, _BOX, size=(N_TEST_LONG, 2))
        test[4100] = obs[39]
        return dict(phi=PHI["near"], obs=obs, test=test, dup=(39, 4100))
    if name == "mixed":
        obs = _cloud(rng, 24, N_KRIG - 24, 0)
        test = _cloud(rng, 2000, N_TEST_LONG - 2000, 0)
        test = test[rng.permutation(N_TEST_LONG)]
        test[4199] = obs[5]
        return dict(phi=PHI["mixed"], obs=obs, test=test, dup=(5, 4199))
    raise KeyError(name)


CANDIDATE_DESIGNS = ("ruler", "cloud", "patch")
KRIG_DESIGNS = ("kruler", "kcloud")
KRIG_LONG_DESIGNS = ("near", "mixed")


def plane():
    """The nu list and the designs of the tests: dict(nus, nus_long, candidate, krig, krig_long)."""
    return dict(nus=NUS, nus_long=NUS_LONG, candidate=CANDIDATE_DESIGNS, krig=KRIG_DESIGNS, krig_long=KRIG_LONG_DESIGNS)


@functools.lru_cache(maxsize=None)
def x_of(name):
    """x = phi d in longdouble from the design's float64 coordinates: (n, n) between the observed sites
    of a candidate design (0 on the diagonal), (n, n_test) from observed to test sites of a kriging one."""
    d = design(name)
    a = np.asarray(d["obs"], dtype=LD)
    b = a if d["test"] is None else np.asarray(d["test"], dtype=LD)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    x = LD(d["phi"]) * np.sqrt(dx * dx + dy * dy)
    x.setflags(write=False)
    return x


def interval_of(x):
    """The device's table interval of x >= 0.5 (cheb_interval), -1 below 0.5, CH_NI and up beyond the table."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x < 0.5, -1, np.searchsorted(EDGES, x, side="right") - 1)


def coverage(name):
    """What the design's x realise, for the tests' coverage assertions (from the reference side)."""
    x = x_of(name)
    if design(name)["test"] is None:
        x = x[np.tril_indices(x.shape[0], -1)]
    x = x.reshape(-1)
    xf = x.astype(np.float64)
    exact = xf.astype(LD) == x
    vals = set(xf[exact].tolist())
    j = interval_of(xf)
    dec = np.floor(np.log10(xf[(xf > 0) & (xf < 0.5)])).astype(int)
    return dict(specials_missing=[v for v in _ruler_specials().tolist() if v not in vals],
                per_interval=np.bincount(j[(j >= 0) & (j < CH_NI)], minlength=CH_NI),
                beyond=int(np.sum(j >= CH_NI)), x_max=float(np.max(xf)), zeros=int(np.sum(xf == 0.0)),
                below_half=int(np.sum((xf > 0) & (xf < 0.5))), x_min_pos=float(np.min(xf[xf > 0])),
                decades={int(k): int(np.sum(dec == k)) for k in range(-9, 0)}, n=int(xf.size))


def coverage_violations(name):
    """What the design fails to realise of its purpose (design's docstring): [] when all is there.  The
    tests assert this per case, so a change to a design cannot lose coverage silently."""
    cv, d, x = coverage(name), design(name), x_of(name)
    out = []

    def need(ok, what):
        if not ok:
            out.append(f"{name}: {what}")

    need(cv["zeros"] >= 1 and x[d["dup"]] == 0, "a duplicated site (x = 0 off the diagonal)")
    if name in ("ruler", "kruler"):
        need(not cv["specials_missing"], f"x values missing: {cv['specials_missing']}")
        need(cv["per_interval"].min() >= 3, f"interval {int(cv['per_interval'].argmin())} holds < 3 values")
        need(cv["beyond"] >= 100 and cv["x_max"] == 600.0, "values beyond the table, up to 600")
        need(cv["below_half"] >= 100, "values below 0.5")
    if name in ("cloud", "kcloud"):
        need(cv["below_half"] >= 5000, f"{cv['below_half']} pairs with x < 0.5")
        need(all(cv["decades"][k] >= 1 for k in range(-9, 0)) and cv["x_min_pos"] >= 1e-9,
             f"x < 0.5 spread over the decades of [1e-9, 0.5): {cv['decades']}")
        need(int(np.sum(cv["per_interval"] >= 3)) >= 90 and cv["beyond"] >= 100,
             "rounded distances in at least 90 of the 100 intervals and beyond the table")
    if name == "cloud":
        need(bool(np.all(x[:120, :120] < 0.5)), "rows and columns 0..119 of the first diagonal tile all exact")
    if name == "patch":
        o = d["obs"]
        x_hi = d["phi"] * float(np.hypot(o[:, 0].max() - o[:, 0].min(), o[:, 1].max() - o[:, 1].min()))
        ni = int(interval_of(x_hi)) + 2                                      # cheb_count
        need(ni < CH_NI // 2, f"a stored table of {ni} intervals")
        need(cv["per_interval"][:int(interval_of(cv["x_max"]))].min() >= 3, "every interval up to the largest x")
        need(cv["below_half"] >= 100, "values below 0.5")
    if name == "near":
        need(cv["below_half"] + cv["zeros"] == cv["n"], "every x < 0.5")
    if name == "mixed":
        late = np.asarray(x[:, 4096:], dtype=np.float64)
        need(np.sum((late > 0) & (late < 0.5)) >= 100 and np.sum((late >= 0.5) & (late < EDGES[-1])) >= 100
             and np.sum(late >= EDGES[-1]) >= 100, "exact and interpolated elements in the second chunk")
        need(cv["per_interval"].min() >= 3, "every interval")
    if name in ("near", "mixed"):
        need(x.shape[1] > 4096 and d["dup"][1] >= 4096, "a second 4,096-site chunk with the duplicate in it")
    return out


@functools.lru_cache(maxsize=8)
def reference(name, nu):
    """(rho, cond) in longdouble over x_of(name): rho = 1 and cond = 0 where x = 0.  Computed once per
    (design, nu) and shared, read-only."""
    x = x_of(name)
    rho = np.ones(x.shape, dtype=LD)
    cnd = np.zeros(x.shape, dtype=LD)
    m = x > 0
    rho[m], cnd[m] = rho_and_cond(x[m], nu)
    rho.setflags(write=False)
    cnd.setflags(write=False)
    return rho, cnd


def bar(cnd):
    """The relative bar per element: 1e-13 + 2 * 2^-52 * cond(x)."""
    return CLAIM + 2.0 * EPS * np.asarray(cnd, dtype=np.float64)


def judge(dev, ref, cnd, x=None):
    """dev (float64) against ref (longdouble) element by element: (violations, figures).  figures: the
    largest relative error, the largest error / bar and the x at each (x given), and the count of
    failing elements."""
    dev = np.asarray(dev, dtype=np.float64)
    out = []
    if dev.shape != ref.shape:
        return [f"shape {dev.shape} against {ref.shape}"], {}
    if not np.all(np.isfinite(dev)):
        out.append(f"{int(np.sum(~np.isfinite(dev)))} elements are not finite")
    if np.any(dev > 1.0):
        out.append(f"{int(np.sum(dev > 1.0))} elements exceed 1")
    rel = (np.abs(dev.astype(LD) - ref) / ref).astype(np.float64)
    rel = np.where(np.isfinite(rel), rel, np.inf)
    b = bar(cnd)
    ratio = rel / b
    bad = ~(rel <= b)
    xs = None if x is None else np.asarray(x, dtype=np.float64)
    for i in np.argwhere(bad)[:4]:
        i = tuple(i)
        at = "" if xs is None else f" x {xs[i]:.17g}"
        out.append(f"element {i}:{at} rel {rel[i]:.3e} > bar {b[i]:.3e} (dev {dev[i]!r}, ref {float(ref[i])!r})")
    i_rel = np.unravel_index(np.argmax(rel), rel.shape)
    i_rat = np.unravel_index(np.argmax(ratio), ratio.shape)
    fig = dict(max_rel=float(rel[i_rel]), max_ratio=float(ratio[i_rat]), n_bad=int(np.sum(bad)),
               x_at_rel=None if xs is None else float(xs[i_rel]), x_at_ratio=None if xs is None else float(xs[i_rat]))
    return out, fig
