"""Meta-kriging workflow around the device path (MetaKriging_BinaryResponse.R).

  partition            MK.R:15-41   random split into n.core subsets (last takes the remainder);
                                    method="R" replays R's own sample()/setdiff stream
  partitioned_spMvGLM  MK.R:46-96   one subset: glm start values -> spMvGLM -> spPredict -> quantiles
  meta_fit             MK.R:100-114 every subset of a shard at once on one GPU (replaces foreach %dopar%)
  combine              MK.R:119-133 mean of the subsets' 200-quantile grids (device kernel)
  posterior_summary    MK.R:136-165 interpolate to the 996-level grid, resample, p(y=1), summaries
"""
import numpy as np

from ._lib import _ip, check, load
from .glm import glm_binomial
from .post import combine_median
from .post import posterior_summary as _post_summary
from .session import SamplerConfig, Session, combine, map_grid

PROBS200 = None


def r_seq(frm, to, by):
    n = int((to - frm) / by + 1e-10)
    x = frm + np.arange(n + 1, dtype=np.float64) * by
    return np.minimum(x, to)


PROBS200 = r_seq(0.005, 1.0, 0.005)     # MK.R:88
XOUT996 = r_seq(0.005, 1.0, 0.001)      # MK.R:140


def partition(n, n_core, seed=20250114, method="permutation"):
    """MK.R:15-41: n.part = c(rep(floor(n/K), K-1), remainder); random indices without replacement.

    Returns (n_part, index_part) with 0-based index arrays.
    method="R": the index sets R itself draws after `set.seed(seed)` (R >= 3.6 defaults:
    Mersenne-Twister + rejection sampling), via libmk's mk_partition_r -- the reference's
    sample()/setdiff loop (MK.R:29-41), in R's draw order.
    method="permutation": a seeded NumPy permutation split (same distribution, not R's stream)."""
    if method == "R":
        lib = load()
        n_part = np.empty(n_core, dtype=np.int32)
        idx = np.empty(n, dtype=np.int32)
        check(lib.mk_partition_r(int(n), int(n_core), int(seed),
                                 n_part.ctypes.data_as(_ip), idx.ctypes.data_as(_ip)))
        offs = np.concatenate([[0], np.cumsum(n_part)])
        return n_part, [idx[offs[i]:offs[i + 1]].astype(np.int64) - 1 for i in range(n_core)]
    if method != "permutation":
        raise ValueError(f"error: unknown partition method '{method}'")
    per = n // n_core
    n_part = [per] * (n_core - 1) + [n - per * (n_core - 1)]
    perm = np.random.default_rng(seed).permutation(n)
    idx, off = [], 0
    for m in n_part:
        idx.append(perm[off:off + m])
        off += m
    return np.array(n_part, dtype=np.int32), idx


def subset_data(y, x, weight, coords, q, index):
    """Y*.part / X*.part / coords.part for one subset (MK.R:33-39), stacked location-major."""
    rows = (np.asarray(index)[:, None] * q + np.arange(q)[None, :]).reshape(-1)
    w = np.broadcast_to(np.asarray(weight, float), (len(y),))
    return dict(coords=np.asarray(coords, float)[index], y=np.asarray(y, float)[rows],
                weights=np.ascontiguousarray(w[rows]), x=np.asarray(x, float)[rows])


def default_config(q, p, beta_starting, beta_tuning, cov_model="exponential", n_batch=100, batch_length=50,
                   seed=20250114, **kw):
    """The worker's literal settings (MK.R:56-64, 83, 85)."""
    return SamplerConfig(q, p, beta_starting, beta_tuning, cov_model=cov_model, n_batch=n_batch,
                         batch_length=batch_length, accept_rate=0.43, seed=seed, **kw)


def start_values(y, x, weight, q, device=0, link="logit"):
    """MK.R:53-55 on the full data, once, on device: beta.starting and t(chol(vcov))."""
    n_tot = len(y)
    wt = np.broadcast_to(np.asarray(weight, float), (n_tot,))
    coef, vcov, bt = glm_binomial(y, x, wt, device=device, link=link)
    return coef, bt


def r_sample_replace(n, size, seed):
    """sample.int(n, size, replace=TRUE) as R draws it right after set.seed(seed) (1-based),
    e.g. MK.R:141's sampleparIndex with n = length(Xout) = 996."""
    lib = load()
    out = np.empty(int(size), dtype=np.int32)
    check(lib.mk_r_sample_replace(int(seed), int(n), int(size), out.ctypes.data_as(_ip)))
    return out


def meta_fit(y, x, weight, coords, q, index_part, coords_test=None, cfg=None, subset_base=0, device=0,
             cov_model="exponential", n_batch=100, batch_length=50, seed=20250114, x_test=None, diagnostics=False,
             criteria=False, y_test=None, weights_test=1, maps=None, pairs=None, regions=None):
    """All subsets of one shard on one GPU; returns the list `obj` of MK.R:108 for those subsets:
    [{'parameters': 200 x P, 'w.predict': 200 x (q n_test)}, ...]; with x_test (MK.R:87's x.test) each
    also holds 'p.predict' (200 x (q n_test)): the grid of p(y = 1) at the test sites.
    diagnostics=True: each also holds 'parameters.diagnostics' (3 x P: ess, mcse, split R-hat of its kept
    chain) and, with test sites, 'w.predict.diagnostics' / 'p.predict.diagnostics' (3 x (q n_test)).
    criteria=True: each also holds 'criteria', the subset's DIC and WAIC rows by name (bar.D, D.bar.Omega,
    pD, DIC, lppd, p.waic, WAIC, lconst; Session.criteria), accumulated in chain over its kept states.
    y_test (with weights_test trials; needs x_test): each also holds 'scores', the subset's held-out row by
    name (n, lpd, brier, err, lconst; Session.scores) of its posterior predictive at the test sites.
    maps (exceedance thresholds, () for none; needs x_test): each also holds 'maps', the subset's (q n_test) x
    (4 + J) planes, and 'maps.names' (w_mean, w_sd, p_mean, p_sd, exc_1..J; Session.maps).
    pairs (joint-exceedance thresholds, () for none; needs x_test and q >= 2): each also holds 'both.predict' and
    'diff.predict' (200 x C2: the grids of p_a p_b and p_a - p_b per site and outcome pair), 'pairs' (C2 x
    (6 + J) planes), 'pairs.names' (both_mean, both_sd, diff_mean, diff_sd, corr, a_gt_b, joint_1..J) and
    'pairs.list' (the (a, b) in column order; Session.pairs).
    regions (dict(offsets=..., weights=..., thresholds=..., interpolate=...); needs x_test and cfg.predict_tile >= the number of
    test sites): each also holds 'region.predict' (200 x C3: the grid of the regional prevalence per region and
    outcome), 'regions' (C3 x (2 + J) planes), 'regions.names' (mean, sd, exc_1..J) and 'regions.singular'
    (Session.regions; combine_regions combines the grids).  The joint draws need the tiled
    replay (the exact one, or with interpolate=True the phi-interpolated one where it applies), so the session
    is then created without test sites and kriges all of them after the run, in one tile."""
    p = np.asarray(x).shape[1]
    if cfg is None:
        beta0, bt = start_values(y, x, weight, q)
        cfg = default_config(q, p, beta0, bt, cov_model=cov_model, n_batch=n_batch, batch_length=batch_length,
                             seed=seed)
    subsets = [subset_data(y, x, weight, coords, q, idx) for idx in index_part]
    with Session(subsets, cfg, coords_test=None if regions is not None else coords_test, subset_base=subset_base,
                 device=device, x_test=None if regions is not None else x_test, criteria=criteria) as ses:
        if regions is not None:     # a tiled session: the chain states are recorded, the sites come after the run
            ses.run(cfg.n_samples)
            ses.set_test_sites(coords_test, x_test=x_test)
            ses.set_regions(regions["offsets"], regions.get("weights"), regions.get("thresholds", ()),
                            interpolate=regions.get("interpolate", False))
        if y_test is not None:
            ses.set_validation(y_test, weights_test)
        if maps is not None:
            ses.set_maps(maps)
        if pairs is not None:
            ses.set_pairs(pairs)
        if regions is None:
            ses.run(cfg.n_samples)
        out = ses.outputs(diagnostics=diagnostics)
        crit = ses.criteria() if criteria else None
        scores = ses.scores() if y_test is not None else None
        planes = ses.maps() if maps is not None else None
        pr = ses.pairs() if pairs is not None else None
        rg = ses.regions() if regions is not None else None
    res = []
    for i in range(len(subsets)):
        d = {"parameters": out["parameters"][i]}
        if "w_predict" in out:
            d["w.predict"] = out["w_predict"][i]
        if "p_predict" in out:
            d["p.predict"] = out["p_predict"][i]
        for kind in ("parameters", "w_predict", "p_predict"):
            if kind + "_diag" in out:
                d[kind.replace("_", ".") + ".diagnostics"] = out[kind + "_diag"][i]
        if crit is not None:
            d["criteria"] = dict(zip(crit["names"], crit["subsets"][i].tolist()))
        if scores is not None:
            d["scores"] = dict(zip(scores["names"], scores["subsets"][i].tolist()))
        if planes is not None:
            d["maps"], d["maps.names"] = planes["subsets"][i], list(planes["names"])
        if pr is not None:
            d["both.predict"], d["diff.predict"] = pr["both_predict"][i], pr["diff_predict"][i]
            d["pairs"], d["pairs.names"], d["pairs.list"] = pr["subsets"][i], list(pr["names"]), list(pr["pairs"])
        if rg is not None:
            d["region.predict"], d["regions"], d["regions.names"] = rg["region_predict"][i], rg["subsets"][i], list(rg["names"])
            d["regions.singular"], d["regions.thresholds"] = rg["singular"][i], list(rg["thresholds"])
        res.append(d)
    return res


def partitioned_spMvGLM(i, y, x, weight, n, q, n_part, coords_test, x_test, index_part, coords,
                        cov_model="exponential", n_batch=100, batch_length=50, seed=20250114, device=0):
    """MK.R:46-96 for subset i (1-based, as the reference): list(parameters, w.predict), and p.predict
    when x_test (the argument MK.R:87 hands spPredict) is given."""
    return meta_fit(y, x, weight, coords, q, [index_part[i - 1]], coords_test=coords_test, subset_base=i - 1,
                    device=device, cov_model=cov_model, n_batch=n_batch, batch_length=batch_length, seed=seed,
                    x_test=x_test)[0]


def combiner(method, device=0):
    """The combine of a list of grids as a function: "mean" (MK.R:123-133, sequential), "sum" (the
    same without the 1/K) or "median" (Weiszfeld)."""
    if method == "mean":
        return lambda grids: combine(grids, device=device)
    if method == "sum":
        return lambda grids: combine(grids, device=device, mean=False)
    if method == "median":
        return lambda grids: combine_median(grids, device=device)[0]
    raise ValueError(f"error: unknown combine method '{method}'")


def combine_results(obj, device=0, method="mean"):
    """MK.R:123-133: result (200 x P) and result2 (200 x q n_test).  method="median" is the
    Weiszfeld geometric-median extension (the reference averages).
    combine_predictive(obj) gives result3 from the subsets' p.predict grids the same way."""
    comb = combiner(method, device)
    result = comb([o["parameters"] for o in obj])
    result2 = comb([o["w.predict"] for o in obj]) if "w.predict" in obj[0] else None
    return result, result2


def combine_predictive(obj, device=0, method="mean"):
    """result3 (200 x q n_test): the subsets' p.predict grids combined as combine_results combines
    w.predict; None when the subsets were fitted without x_test."""
    if "p.predict" not in obj[0]:
        return None
    return combiner(method, device)([o["p.predict"] for o in obj])


def combine_regions(obj, device=0, method="mean"):
    """The subsets' region.predict grids combined as combine_predictive combines p.predict (200 x C3), and the
    combined grid's planes by map_grid: {'region.predict', 'planes' (C3 x (2 + J)), 'names', 'thresholds'}; None
    when the subsets were fitted without regions."""
    if "region.predict" not in obj[0]:
        return None
    grid = combiner(method, device)([o["region.predict"] for o in obj])
    m = map_grid(grid, obj[0].get("regions.thresholds", ()), device=device)
    return {"region.predict": grid, "planes": m["planes"], "names": m["names"], "thresholds": m["thresholds"]}


def convergence_report(diag, ess_min=100, rhat_max=1.05):
    """Counts over the chain diagnostics Session.outputs / meta_fit_node return with diagnostics=True
    (any dict holding '<kind>_diag' -- a list of 3 x C arrays, rows ess, mcse, rhat -- and / or
    '<kind>_diag_worst', kind in parameters, w_predict, p_predict).  Per kind present: 'chains' counted
    (every subset's columns, or the worst rows when only they are given), 'columns', 'ess_below'
    (ess < ess_min), 'rhat_above' (rhat > rhat_max; a chain that never moved has rhat = inf),
    'not_finite' (chains with a NaN), 'min_ess' / 'max_mcse' / 'max_rhat' over the finite entries and
    the columns 'min_ess_column' / 'max_rhat_column' (0-based) where they occur.  The thresholds are
    the caller's: common working values, not pass / fail rules of the library."""
    rep = {}
    for kind in ("parameters", "w_predict", "p_predict"):
        per, worst = diag.get(kind + "_diag"), diag.get(kind + "_diag_worst")
        if per is None and worst is None:
            continue
        a = np.stack([np.asarray(x, float) for x in per]) if per is not None else np.asarray(worst, float)[None]
        if worst is None:       # min ess, max mcse, max rhat; a NaN in any subset stays
            worst = np.where(np.isnan(a).any(axis=0), np.nan,
                             np.stack([a[:, 0].min(axis=0), a[:, 1].max(axis=0), a[:, 2].max(axis=0)]))
        worst = np.asarray(worst, float)
        ess, rhat = a[:, 0], a[:, 2]
        r = dict(chains=int(ess.size), columns=int(a.shape[2]), ess_below=int((ess < ess_min).sum()),
                 rhat_above=int((rhat > rhat_max).sum()), not_finite=int(np.isnan(a).any(axis=1).sum()))
        for name, row, pick in (("min_ess", 0, np.nanargmin), ("max_mcse", 1, np.nanargmax), ("max_rhat", 2, np.nanargmax)):
            ok = not np.isnan(worst[row]).all()
            col = int(pick(worst[row])) if ok else None
            r[name] = float(worst[row][col]) if ok else None
            if name != "max_mcse":
                r[name + "_column"] = col
        rep[kind] = r
    return rep


def median_subset_row(scores):
    """The row (by name) of the subset whose lpd is the median of the K subsets' (of an even K the better of
    the two middle ones; subsets with a NaN lpd last): the "typical subset posterior" the combined one is compared
    with."""
    lpd = np.asarray(scores["subsets"])[:, 1]
    order = np.argsort(np.where(np.isnan(lpd), np.inf, -lpd), kind="stable")      # best first, NaN last
    i = int(order[(len(order) - 1) // 2])
    row = dict(zip(scores["names"], np.asarray(scores["subsets"])[i].tolist()))
    row["subset"] = i
    return row


def validation_report(pmean, y, weights=1, bins=10):
    """Host-side companions of the held-out scores, from a pointwise pmean (NumPy): 'auc', the area under
    the ROC curve by the Mann-Whitney statistic with ties counted half, over the columns with weights = 1
    (None unless both outcomes occur there); and the reliability table over `bins` equal-width bins of
    pmean on the columns with weights > 0 -- 'bin_edges', and per bin 'count', 'mean_pmean' and
    'mean_observed' (the mean of y / weights; NaN for an empty bin)."""
    pm = np.asarray(pmean, dtype=np.float64).reshape(-1)
    yv = np.asarray(y, dtype=np.float64).reshape(-1)
    wt = np.broadcast_to(np.asarray(weights, dtype=np.float64), pm.shape)
    if yv.shape != pm.shape:
        raise ValueError("error: pmean and y must have the same length")
    one = (wt == 1.0) & np.isfinite(pm)
    pos, neg = pm[one & (yv == 1.0)], pm[one & (yv == 0.0)]
    auc = None
    if pos.size and neg.size:
        allv = np.concatenate([pos, neg])
        order = np.argsort(allv, kind="stable")
        ranks = np.empty(allv.size)
        sv = allv[order]
        start = np.flatnonzero(np.concatenate([[True], sv[1:] != sv[:-1]]))
        end = np.concatenate([start[1:], [sv.size]])
        for a, b in zip(start, end):                          # mid-ranks: ties count half
            ranks[order[a:b]] = 0.5 * (a + b - 1) + 1.0
        auc = float((ranks[:pos.size].sum() - pos.size * (pos.size + 1) / 2.0) / (pos.size * neg.size))
    obs = (wt > 0.0) & np.isfinite(pm)
    edges = np.linspace(0.0, 1.0, int(bins) + 1)
    which = np.clip(np.digitize(pm[obs], edges[1:-1]), 0, int(bins) - 1)
    count = np.bincount(which, minlength=int(bins)).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_p = np.bincount(which, weights=pm[obs], minlength=int(bins)) / count
        mean_o = np.bincount(which, weights=yv[obs] / wt[obs], minlength=int(bins)) / count
    return dict(auc=auc, bin_edges=edges, count=count, mean_pmean=mean_p, mean_observed=mean_o)


def posterior_summary(result, result2, x_test, q=None, samplesize=1000, seed=20250114, device=0, rng="philox",
                      index=None, link="logit"):
    """MK.R:136-165 on device: interpolate both combined grids to Xout (996 levels), one shared
    resample index vector (comonotone draws, MK.R:141), p(y=1) = logistic(x.test B + w) and the
    median / 2.5% / 97.5% summaries (post.posterior_summary).  rng="R": sampleparIndex is R's
    sample(seq(1, length(Xout), 1), samplesize, replace=TRUE) right after set.seed(seed);
    index: a 1-based index vector drawn by the caller (R's own stream)."""
    return _post_summary(result, result2, x_test, samplesize=samplesize, seed=seed, device=device, rng=rng,
                         index=index, link=link)


def reference_flow(d, K, q, cov_model="exponential", n_batch=100, batch_length=50, seed=20250114, devices=(0,),
                   method="mean", predict_tile=0, partition_method="R", samplesize=1000, progress=None,
                   predictive=False, diagnostics=False, criteria=False, validate=False, maps=None, pairs=None):
    """The reference script end to end in one process over the GPUs in `devices` (mk_meta_fit: the
    subsets sharded over them in-library, the combine device to device):

      partition                 MK.R:15-41    mk_partition_r (R's own index sets after set.seed)
      glm start values          MK.R:53-55    device IRLS on the full data, once
      foreach %dopar% worker    MK.R:100-114  every subset's spMvGLM + spPredict + 200-level grids
      combine                   MK.R:119-133  sequential mean (or Weiszfeld median), per test-site
                                              tile when predict_tile > 0 (configs[4])
      resample, p(y=1), quant.  MK.R:136-165  posterior_summary

    d: synthetic.generate output.  progress(iterations, n_samples) is called between amcmc batches
    (return True to stop).  predictive=True hands d["x_test"] to the fit as MK.R:87's x.test: every
    subset's grids of p(y = 1) at the test sites are made and combined too, summary["result3"].
    diagnostics=True: the worst-over-subsets chain diagnostics come back as summary["diagnostics"]
    (the '*_diag_worst' arrays of meta_fit_node; convergence_report reads them).
    criteria=True: the DIC and WAIC rows summed over the K subsets come back by name as
    summary["criteria"] (meta_fit_node's 'criteria' total).
    validate=True (implies predictive): d["y_test"] is scored at the test sites; summary["validation"]
    holds 'combined' (the combined p grid's row by name), 'subsets' (K x 5), 'names', 'median_subset'
    (the row of the subset whose lpd is the median of the K) and 'report' (validation_report of the
    combined grid's pmean: AUC and the reliability table).
    maps (exceedance thresholds, () for none; implies predictive): summary["maps"] holds 'names', 'thresholds'
    and 'combined' ((q n_test) x (4 + J): the combined grids' mean, sd and exceedance planes, meta_fit_node's
    'maps_combined') and 'subsets' (per subset the same planes of its own posterior).
    pairs (joint-exceedance thresholds, () for none; implies predictive; q >= 2): summary["pairs"] holds
    meta_fit_node's 'pairs' dict (names, pairs, thresholds and per subset the grids and planes) plus
    'result_both' / 'result_diff' (200 x C2: the combined grids of p_a p_b and p_a - p_b) and 'combined'
    (meta_fit_node's 'pairs_combined': map_grid's planes of the two combined grids).
    Returns (phases, result, result2, summary, cfg) -- phases in seconds of
    wall clock: set-up (partition, glm, subset slicing), the chains (to the last batch boundary),
    quantiles + combine, post-processing, and the whole."""
    import time
    from .node import meta_fit_node
    t = {}
    n = len(d["coords"])
    t0 = time.perf_counter()
    n_part, index_part = partition(n, K, seed=seed, method=partition_method)                 # MK.R:15-41
    beta0, bt = start_values(d["y"], d["x"], 1.0, q, device=int(devices[0]))                 # MK.R:53-55
    p = d["x"].shape[1]
    cfg = SamplerConfig(q, p, beta0, bt, cov_model=cov_model, n_batch=n_batch, batch_length=batch_length, seed=seed,
                        predict_tile=predict_tile)
    subs = [subset_data(d["y"], d["x"], 1.0, d["coords"], q, index_part[i]) for i in range(K)]
    t["setup_s"] = time.perf_counter() - t0
    t1 = time.perf_counter()
    stamp = {}

    def _progress(it, n_samples):
        if it >= n_samples:
            stamp["chains"] = time.perf_counter()
        return bool(progress(it, n_samples)) if progress is not None else False

    fit = meta_fit_node(subs, cfg, coords_test=d["coords_test"], devices=devices, method=method, per_subset=False,
                        progress=_progress, x_test=d["x_test"] if predictive or validate or maps is not None or pairs is not None else None,
                        diagnostics=diagnostics, criteria=criteria,
                        validation=dict(y_test=d["y_test"], pointwise=True) if validate else None,
                        maps=maps, pairs=pairs)                                              # MK.R:100-133
    t3 = time.perf_counter()
    t["chains_s"] = stamp.get("chains", t3) - t1
    t["quantiles_combine_s"] = t3 - stamp.get("chains", t3)
    t2 = time.perf_counter()
    summ = posterior_summary(fit["result"], fit["result2"], d["x_test"], samplesize=samplesize, seed=seed,
                             device=int(devices[0]))                                         # MK.R:136-165
    t["post_s"] = time.perf_counter() - t2
    if "result3" in fit:
        summ["result3"] = fit["result3"]
    if diagnostics:
        summ["diagnostics"] = {k: v for k, v in fit.items() if k.endswith("_diag_worst")}
    if criteria:
        summ["criteria"] = dict(zip(fit["criteria"]["names"], fit["criteria"]["total"].tolist()))
    if maps is not None:
        summ["maps"] = dict(fit["maps"], combined=fit["maps_combined"])
    if pairs is not None:
        summ["pairs"] = dict(fit["pairs"], result_both=fit["result_both"], result_diff=fit["result_diff"],
                             combined=fit["pairs_combined"])
    if validate:
        sc = fit["scores"]
        summ["validation"] = dict(combined=sc["combined"], subsets=sc["subsets"], names=sc["names"],
                                  median_subset=median_subset_row(sc),
                                  report=validation_report(sc["combined_pointwise"][:, 0], d["y_test"]))
    t["end_to_end_s"] = time.perf_counter() - t0
    t["exchange"] = fit["exchange"]          # the combine's all-to-all: "rccl" (distinct GPUs) or "copy"
    t["comm_ranks"] = fit["comm_ranks"]      # ranks RCCL's communicators hold (copies: device blocks)
    return t, fit["result"], fit["result2"], summ, cfg
