"""spMvGLM / spPredict drop-ins (the spBayes surface MK.R:80-89 uses).

Argument names and meaning follow spBayes as called by the reference:

  spMvGLM(formula=list(Y1 ~ X1 - 1, ...), coords, weights = n x q matrix,
          starting = list(beta, phi, A, w[, nu]), tuning = list(beta, phi, A, w[, nu]),
          priors = list("beta.Flat", phi.Unif = list(a, b), K.IW = list(df, S)[, nu.Unif]),
          amcmc = list(n.batch, batch.length, accept.rate), cov.model, n.report)
  spPredict(sp.obj, pred.coords, pred.covars, start, end)

``formula`` is a list of (Y_a, X_a) pairs (Y_a: n responses, X_a: n x p_a
design without intercept handling -- the ``Y ~ X - 1`` form of MK.R:80).
Errors are raised as ValueError / MkError where spBayes would stop().

spMvGLM keeps its device session open with every chain state recorded
(predict_tile mode, burn_in = 1); spPredict then only runs the kriging: it sets
the prediction sites (mk_session_set_test_sites) and replays the kept states of
iterations start..end (mk_session_set_kept_window) -- no refit.  Every kriging
draw has its own Philox stream keyed by the iteration, so the draws equal those of
a fit that fused the kriging into iterations start..end.
"""
import numpy as np

from . import fitfile
from .session import SamplerConfig, Session

PREDICT_TILE = 65536   # test sites per kriging pass in spPredict (device buffers per pass)


def _stack(formula, weights):
    q = len(formula)
    n = np.asarray(formula[0][0]).shape[0]
    ps = [np.asarray(X, float).reshape(n, -1).shape[1] for _, X in formula]
    p = sum(ps)
    y = np.zeros(n * q)
    X = np.zeros((n * q, p))
    off = 0
    for a, (Ya, Xa) in enumerate(formula):
        Ya = np.asarray(Ya, float).reshape(-1)
        Xa = np.asarray(Xa, float).reshape(n, -1)
        if Ya.shape[0] != n:
            raise ValueError("error: every outcome needs the same number of locations")
        y[a::q] = Ya
        X[a::q, off:off + ps[a]] = Xa
        off += ps[a]
    w = np.asarray(weights, float)
    w = np.broadcast_to(w, (n, q)) if w.ndim < 2 else w
    if w.shape != (n, q):
        raise ValueError("error: weights must be a n x q matrix")
    return q, p, n, y, X, np.ascontiguousarray(w).reshape(-1)


def _config(q, p, starting, tuning, priors, amcmc, cov_model, burn_in=None, seed=20250114):
    if amcmc is None:
        raise ValueError("error: this build implements the amcmc (adaptive) sampler only, as MK.R:83 uses")
    if "beta" not in starting or "beta" not in tuning:
        raise ValueError("error: beta must be specified in starting and tuning")
    for nm in ("phi", "A", "w"):
        if nm not in starting:
            raise ValueError(f"error: {nm} must be specified in starting")
        if nm not in tuning:
            raise ValueError(f"error: {nm} must be specified in tuning")
    if "phi.Unif" not in priors or "K.IW" not in priors:
        raise ValueError("error: phi.Unif and K.IW must be specified in priors")
    phi_u = priors["phi.Unif"]
    kiw = priors["K.IW"]
    matern = cov_model == "matern"
    if matern and ("nu" not in starting or "nu" not in tuning or "nu.Unif" not in priors):
        raise ValueError("error: nu must be specified in starting, tuning and priors (nu.Unif) for matern")
    return SamplerConfig(
        q, p, beta_starting=starting["beta"], beta_tuning=tuning["beta"], cov_model=cov_model,
        n_batch=amcmc["n.batch"], batch_length=amcmc["batch.length"], accept_rate=amcmc.get("accept.rate", 0.43),
        burn_in=burn_in, phi_starting=np.broadcast_to(np.asarray(starting["phi"], float), (q,)),
        phi_tuning=np.broadcast_to(np.asarray(tuning["phi"], float), (q,)),
        phi_unif=(np.broadcast_to(np.asarray(phi_u[0], float), (q,)), np.broadcast_to(np.asarray(phi_u[1], float), (q,))),
        A_starting=starting["A"], A_tuning=np.broadcast_to(np.asarray(tuning["A"], float), (q * (q + 1) // 2,)),
        w_starting=float(np.asarray(starting["w"]).reshape(-1)[0]), w_tuning=float(np.asarray(tuning["w"]).reshape(-1)[0]),
        nu_starting=None if not matern else np.broadcast_to(np.asarray(starting["nu"], float), (q,)),
        nu_tuning=None if not matern else np.broadcast_to(np.asarray(tuning["nu"], float), (q,)),
        nu_unif=None if not matern else (np.broadcast_to(np.asarray(priors["nu.Unif"][0], float), (q,)),
                                         np.broadcast_to(np.asarray(priors["nu.Unif"][1], float), (q,))),
        K_IW_df=kiw[0], K_IW_S=np.asarray(kiw[1], float).reshape(q, q), seed=seed)


class SpMvGLMFit(dict):
    """Result of spMvGLM: keys 'p.beta.theta.samples' (n.samples x P), 'p.w.samples'
    ((n q) x n.samples), 'acceptance' (n.batch x (p + n_theta + 1)), plus the inputs
    spPredict needs.

    The fit holds its device session (every recorded chain state, for spPredict) until
    ``close()`` -- or the end of a ``with`` block, or garbage collection.  Close fits you no
    longer predict from when fitting many subsets in a loop: each holds its factors in HBM."""

    def save(self, path):
        """The fit into one file (fitfile.save_session): R's save() of an spMvGLM object.  load_fit(path) gives
        an object that serves spPredict and the other sp* calls in a later process, without running the chain."""
        ses = self.get("_session")
        if ses is None:
            raise ValueError("error: the spMvGLM fit was closed; save() needs its session")
        fitfile.save_session(ses, path)

    def close(self):
        ses = self.pop("_session", None)
        if ses is not None:
            ses.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def spMvGLM(formula, coords, weights, starting, tuning, priors, amcmc, cov_model="exponential",
            family="binomial", n_report=10, seed=20250114, device=0, subset_index=0):
    if family != "binomial":
        raise ValueError("error: family must be binomial (the reference's binary response)")
    q, p, n, y, X, wt = _stack(formula, weights)
    coords = np.asarray(coords, float).reshape(n, 2)
    cfg = _config(q, p, starting, tuning, priors, amcmc, cov_model, burn_in=1, seed=seed)
    cfg.predict_tile = PREDICT_TILE          # record every chain state for spPredict
    sub = dict(coords=coords, y=y, weights=wt, x=X)
    ses = Session([sub], cfg, subset_base=subset_index, device=device, record_w=True)
    try:
        ses.run(cfg.n_samples)
        out = ses.outputs(quantiles=False, samples=True, w_samples=True, acceptance=True)
    except Exception:
        ses.close()
        raise
    fit = SpMvGLMFit()
    fit["p.beta.theta.samples"] = out["samples"][0]
    fit["p.w.samples"] = out["w_samples"][0]
    fit["acceptance"] = out["acceptance"][0]
    fit["_session"] = ses                    # closed when the fit object is collected
    fit["_n_samples"] = cfg.n_samples
    return fit


def load_fit(path, device=0):
    """The spMvGLM fit SpMvGLMFit.save wrote, on `device`: the same keys, and a session rebuilt from the file's
    chain (fitfile.load_session), so spPredict, spDiag, spLoo, spDiagnostics, spValidate, spMaps, spPairs and spRegions
    serve it unchanged.  p.beta.theta.samples and p.w.samples are the saved bytes; the kriging draws agree with
    the original fit's to rounding (the record's z is recomputed from w)."""
    a = fitfile.read(path)
    if a["n_part"].shape[0] != 1:
        raise ValueError(f"error: load_fit reads the file of one spMvGLM fit; '{path}' holds {a['n_part'].shape[0]} subsets "
                         "(fitfile.load_session loads those)")
    ses = fitfile.session_from(a, device=device)
    fit = SpMvGLMFit()
    fit["p.beta.theta.samples"] = a["samples"][0]
    fit["p.w.samples"] = a["w_samples"]
    fit["acceptance"] = a["acceptance"][0]
    fit["_session"] = ses
    fit["_n_samples"] = ses.cfg.n_samples
    return fit


def spDiagnostics(sp_obj, start=1, end=None):
    """Chain diagnostics of p.beta.theta.samples over iterations start..end (1-based, inclusive; the
    window a coda user would pass to window()): a 3 x P array, rows ess (Geyer's initial monotone
    sequence), mcse (of the column mean) and split R-hat, computed on the device from the chain the
    fit recorded.  spMvGLM records from iteration 1, so start is where the caller's burn-in ends."""
    ses = sp_obj.get("_session")
    if ses is None:
        raise ValueError("error: the spMvGLM fit was closed; spDiagnostics needs its recorded chain")
    n_samples = sp_obj["_n_samples"]
    end = n_samples if end is None else int(end)
    start = int(start)
    if not (1 <= start <= end <= n_samples):
        raise ValueError("error: invalid start/end")
    ses.set_kept_window(start, end)
    return ses.outputs(quantiles=False, diagnostics="parameters")["parameters_diag"][0]


def spDiag(sp_obj, start=1, end=None, thin=1):
    """spBayes's spDiag for an spMvGLM fit, on the device: {"DIC": {"bar.D", "D.bar.Omega", "pD", "DIC"},
    "WAIC": {"lppd", "p.waic", "WAIC", "lconst"}} over iterations start..end (1-based, inclusive), every
    thin-th, replayed from the chain the fit recorded (p.beta.theta.samples and p.w.samples).  The
    definitions are in include/mk.h; the likelihood drops the binomial coefficient, "lconst" is what
    full-likelihood figures add (-2 lconst to the deviance rows and WAIC, + lconst to lppd)."""
    ses = sp_obj.get("_session")
    if ses is None:
        raise ValueError("error: the spMvGLM fit was closed; spDiag needs its recorded chain")
    n_samples = sp_obj["_n_samples"]
    end = n_samples if end is None else int(end)
    start, thin = int(start), int(thin)
    if not (1 <= start <= end <= n_samples):
        raise ValueError("error: invalid start/end")
    if thin < 1:
        raise ValueError("error: invalid thin")
    ses.set_kept_window(start, end)
    c = ses.criteria(thin=thin)
    row = dict(zip(c["names"], c["subsets"][0].tolist()))
    return {"DIC": {k: row[k] for k in c["names"][:4]}, "WAIC": {k: row[k] for k in c["names"][4:]}}


def spLoo(sp_obj, start=1, end=None, thin=1):
    """PSIS-LOO of an spMvGLM fit (R's loo on the fit's pointwise likelihood), on the device: the rows by name
    -- "elpd_loo", "p_loo", "looic", "se_elpd_loo", "lppd", "k_max", "n_k_bad", "lconst" -- over iterations
    start..end (1-based, inclusive), every thin-th, replayed from the chain the fit recorded, plus "pointwise"
    ((n q) x 3: elpd_loo_i, the Pareto shape k-hat_i, lppd_i).  25 .. 8192 states.  The definitions are in
    include/mk.h; two results go to loo_compare."""
    ses = sp_obj.get("_session")
    if ses is None:
        raise ValueError("error: the spMvGLM fit was closed; spLoo needs its recorded chain")
    n_samples = sp_obj["_n_samples"]
    end = n_samples if end is None else int(end)
    start, thin = int(start), int(thin)
    if not (1 <= start <= end <= n_samples):
        raise ValueError("error: invalid start/end")
    if thin < 1:
        raise ValueError("error: invalid thin")
    ses.set_kept_window(start, end)
    r = ses.loo(thin=thin, pointwise=True)
    res = dict(zip(r["names"], r["subsets"][0].tolist()))
    res["pointwise"] = r["pointwise"][0]
    return res


def spValidate(sp_obj, pred_coords, pred_covars, y, weights=1, start=1, end=None):
    """Held-out validation of an spMvGLM fit, on the device: y ((q n_test), location-major like
    pred_covars' rows) successes of `weights` trials observed at pred_coords are scored against the
    posterior predictive of iterations start..end (1-based, inclusive), kriged from the recorded chain
    in one replay.  Returns the row by name -- "n", "lpd" (log predictive density), "brier", "err"
    (error rate of the rule pmean >= 0.5), "lconst" -- plus "pmean" (the posterior predictive mean of
    p(y = 1) per test column) and "lpd.pointwise".  The definitions are in include/mk.h."""
    ses = sp_obj.get("_session")
    if ses is None:
        raise ValueError("error: the spMvGLM fit was closed; spValidate needs its recorded chain states")
    n_samples = sp_obj["_n_samples"]
    end = n_samples if end is None else int(end)
    start = int(start)
    if not (1 <= start <= end <= n_samples):
        raise ValueError("error: invalid start/end")
    ct = np.asarray(pred_coords, float).reshape(-1, 2)
    xt = np.asarray(pred_covars, float)
    if xt.ndim != 2 or xt.shape[0] != ses.q * ct.shape[0]:
        raise ValueError("error: pred.covars must have one row per prediction site and outcome (q * n rows)")
    ses.set_test_sites(ct, x_test=pred_covars)
    ses.set_kept_window(start, end)
    ses.set_validation(y, weights)
    try:
        ses.outputs(quantiles=False, w_predict_sum=True)      # the one replay of the window
        sc = ses.scores(pointwise=True)
    finally:
        ses.set_validation(None)
    res = dict(zip(sc["names"], sc["subsets"][0].tolist()))
    res["pmean"] = sc["pointwise"][0][:, 0].copy()
    res["lpd.pointwise"] = sc["pointwise"][0][:, 1].copy()
    return res


def spMaps(sp_obj, pred_coords, pred_covars, thresholds=(), start=1, end=None):
    """Posterior maps of an spMvGLM fit at pred_coords, on the device: per prediction column ((q n_test),
    location-major like pred_covars' rows) the posterior mean and sd of w and of p(y = 1) and, per
    threshold u (probability scale), the posterior probability that p > u, over iterations start..end
    (1-based, inclusive), kriged from the recorded chain in one replay -- the draws never leave the
    device.  Returns {"w.mean", "w.sd", "p.mean", "p.sd"} (each q n_test) plus "exceedance" ((q n_test) x
    J) and "thresholds".  The definitions are in include/mk.h."""
    ses = sp_obj.get("_session")
    if ses is None:
        raise ValueError("error: the spMvGLM fit was closed; spMaps needs its recorded chain states")
    n_samples = sp_obj["_n_samples"]
    end = n_samples if end is None else int(end)
    start = int(start)
    if not (1 <= start <= end <= n_samples):
        raise ValueError("error: invalid start/end")
    ct = np.asarray(pred_coords, float).reshape(-1, 2)
    xt = np.asarray(pred_covars, float)
    if xt.ndim != 2 or xt.shape[0] != ses.q * ct.shape[0]:
        raise ValueError("error: pred.covars must have one row per prediction site and outcome (q * n rows)")
    ses.set_test_sites(ct, x_test=pred_covars)
    ses.set_kept_window(start, end)
    ses.set_maps(thresholds)
    try:
        ses.outputs(quantiles=False, w_predict_sum=True)      # the one replay of the window
        m = ses.maps()
    finally:
        ses.set_maps(None)
    pl = m["subsets"][0]
    res = {k.replace("_", "."): pl[:, i].copy() for i, k in enumerate(m["names"][:4])}
    res["exceedance"] = pl[:, 4:].copy()
    res["thresholds"] = m["thresholds"]
    return res


def spPairs(sp_obj, pred_coords, pred_covars, thresholds=(), start=1, end=None):
    """Cross-outcome prediction of a multivariate (q >= 2) spMvGLM fit at pred_coords, on the device: per
    site and pair of outcomes (a, b), a < b -- columns site-major, the pairs in the order "pairs" lists -- the
    200-level grids "both.predict" of p_a p_b = P(y_a = 1, y_b = 1) and "diff.predict" of p_a - p_b (each 200 x
    C2), "both.mean", "both.sd", "diff.mean", "diff.sd", "corr" (the posterior correlation of p_a and p_b) and
    "a.gt.b" (P(p_a > p_b)) (each C2), and "joint" (C2 x J): the posterior probability that both p_a and p_b
    exceed each threshold; over iterations start..end (1-based, inclusive), kriged from the recorded chain
    in one replay -- the draws never leave the device.  The definitions are in include/mk.h."""
    ses = sp_obj.get("_session")
    if ses is None:
        raise ValueError("error: the spMvGLM fit was closed; spPairs needs its recorded chain states")
    if ses.q < 2:
        raise ValueError("error: spPairs needs a fit with q >= 2 outcomes")
    n_samples = sp_obj["_n_samples"]
    end = n_samples if end is None else int(end)
    start = int(start)
    if not (1 <= start <= end <= n_samples):
        raise ValueError("error: invalid start/end")
    ct = np.asarray(pred_coords, float).reshape(-1, 2)
    xt = np.asarray(pred_covars, float)
    if xt.ndim != 2 or xt.shape[0] != ses.q * ct.shape[0]:
        raise ValueError("error: pred.covars must have one row per prediction site and outcome (q * n rows)")
    ses.set_test_sites(ct, x_test=pred_covars)
    ses.set_kept_window(start, end)
    ses.set_pairs(thresholds)
    try:
        ses.outputs(quantiles=False, w_predict_sum=True)      # the one replay of the window
        m = ses.pairs()
    finally:
        ses.set_pairs(None)
    pl = m["subsets"][0]
    res = {"both.predict": m["both_predict"][0], "diff.predict": m["diff_predict"][0]}
    res.update({k.replace("_", "."): pl[:, i].copy() for i, k in enumerate(m["names"][:6])})
    res["joint"] = pl[:, 6:].copy()
    res["pairs"], res["thresholds"] = m["pairs"], m["thresholds"]
    return res


def spRegions(sp_obj, pred_coords, pred_covars, region, weights=None, thresholds=(), start=1, end=None, samples=False,
              interpolate=False):
    """Areal prediction of an spMvGLM fit, on the device: `region` is an integer label per prediction site; per
    region (in ascending label order, "region.labels") and outcome a -- region column g q + a -- the prevalence
    r = sum_i omega_i p_i,a over the region's sites (omega: `weights` normalised within the region, default
    equal) drawn jointly across the sites per kept state.  Returns "region.predict" (200 x C3: its 200-level
    grid), "region.mean", "region.sd" (each C3), "region.exceed" (C3 x J: the posterior probability that r
    exceeds each threshold), "region.singular" (C3: kept states whose joint covariance factor was flagged),
    "region.labels", "thresholds" and, with samples=True, "region.samples" (C3 x kept); over iterations
    start..end (1-based, inclusive), kriged from the recorded chain in one replay.  A region holds at most 128
    sites.  The sites are sorted by label (stable) for the replay.  interpolate=True serves the regions from the
    phi-interpolated replay where it applies (Session.set_regions); "region.route" names the route that ran and
    "region.check" its check.  The definitions are in include/mk.h."""
    ses = sp_obj.get("_session")
    if ses is None:
        raise ValueError("error: the spMvGLM fit was closed; spRegions needs its recorded chain states")
    n_samples = sp_obj["_n_samples"]
    end = n_samples if end is None else int(end)
    start = int(start)
    if not (1 <= start <= end <= n_samples):
        raise ValueError("error: invalid start/end")
    ct = np.asarray(pred_coords, float).reshape(-1, 2)
    n = ct.shape[0]
    xt = np.asarray(pred_covars, float)
    if xt.ndim != 2 or xt.shape[0] != ses.q * n:
        raise ValueError("error: pred.covars must have one row per prediction site and outcome (q * n rows)")
    lab = np.asarray(region).reshape(-1)
    if lab.shape[0] != n or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError("error: region must hold one integer label per prediction site")
    order = np.argsort(lab, kind="stable")
    labels, counts = np.unique(lab, return_counts=True)
    offsets = np.concatenate([[0], np.cumsum(counts)])
    rows = (order[:, None] * ses.q + np.arange(ses.q)[None, :]).reshape(-1)
    w = None
    if weights is not None:
        w = np.asarray(weights, float).reshape(-1)
        if w.shape[0] != n:
            raise ValueError("error: weights must hold one entry per prediction site")
        w = w[order]
    ses.set_test_sites(ct[order], x_test=xt[rows])
    ses.set_kept_window(start, end)
    ses.set_regions(offsets, w, thresholds, interpolate=interpolate)
    try:
        ses.outputs(quantiles=False, w_predict_sum=True)      # the one replay of the window
        m = ses.regions(samples=samples)
    finally:
        ses.set_regions(None)
    pl = m["subsets"][0]
    res = {"region.predict": m["region_predict"][0], "region.mean": pl[:, 0].copy(), "region.sd": pl[:, 1].copy(),
           "region.exceed": pl[:, 2:].copy(), "region.singular": m["singular"][0], "region.labels": labels.tolist(),
           "thresholds": m["thresholds"], "region.route": m["route"], "region.check": m["check"]}
    if samples:
        res["region.samples"] = m["region_samples"][0]
    return res


def spPredict(sp_obj, pred_coords, pred_covars=None, start=1, end=None, thin=1, diagnostics=False):
    """p.w.predictive.samples ((q n_test) x kept) for kept iterations start..end (1-based,
    inclusive; every thin-th), kriged from the chain states spMvGLM recorded (no refit).
    With pred_covars ((q n_test) x p, location-major rows) also p.y.predictive.samples: spBayes's
    binomial prediction linkinv(x(s)' beta + w(s)), beta and w(s) of the same iteration.
    diagnostics=True: also "w.predictive.diagnostics" and, with covariates, "y.predictive.diagnostics"
    (3 x (q n_test): ess, mcse, split R-hat per site) of the draws of iterations start..end, every one
    of them (thin only picks what is returned), from the replay that makes the draws."""
    ses = sp_obj.get("_session")
    if ses is None:
        raise ValueError("error: the spMvGLM fit was closed; spPredict needs its recorded chain states")
    n_samples = sp_obj["_n_samples"]
    end = n_samples if end is None else int(end)
    start = int(start)
    if not (1 <= start <= end <= n_samples):
        raise ValueError("error: invalid start/end")
    ct = np.asarray(pred_coords, float).reshape(-1, 2)
    if pred_covars is not None:
        xt = np.asarray(pred_covars, float)
        if xt.ndim != 2 or xt.shape[0] != ses.q * ct.shape[0]:
            raise ValueError("error: pred.covars must have one row per prediction site and outcome (q * n rows)")
    ses.set_test_sites(ct, x_test=pred_covars)
    ses.set_kept_window(start, end)
    out = ses.outputs(quantiles=False, w_pred_samples=True, p_pred_samples=pred_covars is not None,
                      diagnostics=diagnostics)
    wp = out["w_pred_samples"][0]                  # (q n_test) x (end - start + 1)
    res = {"p.w.predictive.samples": wp[:, ::int(thin)]}
    if pred_covars is not None:
        res["p.y.predictive.samples"] = out["p_pred_samples"][0][:, ::int(thin)]
    if diagnostics:
        res["w.predictive.diagnostics"] = out["w_predict_diag"][0]
        if pred_covars is not None:
            res["y.predictive.diagnostics"] = out["p_predict_diag"][0]
    return res
