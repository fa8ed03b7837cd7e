"""The whole node in one call: mk_meta_fit (include/mk.h) -- MK.R:100-133 without a cluster.

The K subsets are cut into len(devices) balanced contiguous blocks, one session per device on
its own host thread inside libmk, every chain keyed by its global subset index (so equal to the
one-device chain).  The chains advance one amcmc batch at a time on every device; between
batches libmk calls ``progress(iterations, n_samples)`` on this thread (spBayes's n.report lines;
return True to stop: MkError with code MK_E_INTERRUPT, every device freed).  The combine runs
device to device: an all-to-all of column blocks (RCCL over xGMI for distinct devices; device
copies when a device is listed more than once), the sequential mean (MK.R:123-133, bit-identical
to one device) or the Weiszfeld median per column on each block's owner.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import Combined, check
from .outbuf import (CriteriaBuffers, DiagnosticBuffers, MapBuffers, OutputBuffers, PairBuffers, ScoreBuffers, map_spec,
                     pair_spec, validation_arrays)
from .session import PackedProblem, map_grid

N_LEVELS = _lib.N_LEVELS


def meta_fit_node(subsets, cfg, coords_test=None, devices=(0,), subset_base=0, method="mean", per_subset=True,
                  samples=False, w_samples=False, w_pred_samples=False, acceptance=False, w_predict_sum=False,
                  progress=None, record_w=False, max_iter=100, tol=1e-12, x_test=None, p_pred_samples=False,
                  p_predict_sum=False, diagnostics=False, criteria=False, validation=None, maps=None, pairs=None):
    """Fit all subsets over `devices` and combine.  Returns a dict with 'result' (200 x P, MK.R:127),
    'result2' (200 x q n_test, MK.R:133; None without test sites), 'exchange' ('rccl' / 'copy'),
    'comm_ranks' (the ranks the exchange spans: RCCL's own ncclCommCount, or the blocks for copies),
    and per subset (lists, as Session.outputs lays them out) 'parameters' / 'w_predict' when
    per_subset, plus the optional 'samples', 'w_samples', 'w_pred_samples', 'acceptance',
    'w_predict_sum' (the sequential sum of all K w.predict grids).  With x_test ((q n_test) x p, the
    test sites' covariates) also 'result3' (200 x q n_test: the subsets' grids of p(y = 1) =
    linkinv(x.test beta + w) combined as result2 is), per subset 'p_predict', and the optional
    'p_pred_samples' / 'p_predict_sum'.  diagnostics=True (mk_meta_fit_diag) adds, as Session.outputs
    does, the chain diagnostics of all K subsets -- 'parameters_diag', 'w_predict_diag', 'p_predict_diag'
    (per subset 3 x C: ess, mcse, split R-hat) -- and the '*_diag_worst' arrays (3 x C) over all K.
    criteria=True (mk_meta_fit_ex) adds 'criteria': Session.criteria's dict for all K subsets -- 'subsets'
    (K x 8: bar.D, D.bar.Omega, pD, DIC, lppd, p.waic, WAIC, lconst), 'total' (their sums in global
    subset order) and 'names'; criteria="pointwise" also the per-observation pairs.
    validation (mk_meta_fit_val): held-out outcomes at the test sites -- y_test, (y_test, weights_test) or
    a dict with 'y_test' and optionally 'weights_test' and 'pointwise' -- adds 'scores': Session.scores'
    dict for all K subsets ('subsets' K x 5: n, lpd, brier, err, lconst; 'names') plus 'combined', the row
    of the combined p grid result3 by name (score_grid's); with pointwise also the 'pointwise' pairs per
    subset and 'combined_pointwise'.  Needs x_test.
    maps (mk_meta_fit_maps): exceedance thresholds on the probability scale (() for none; None: no maps)
    -- adds 'maps': Session.maps' dict for all K subsets ('names': w_mean, w_sd, p_mean, p_sd, exc_1..J;
    'thresholds'; 'subsets': per subset C x (4 + J)) and 'maps_combined' (C x (4 + J)): the same planes of
    the combined grids, w_mean and w_sd from result2, the others from result3 (map_grid's).  Needs x_test.
    pairs (mk_meta_fit_pairs; q >= 2): joint-exceedance thresholds (() for none; None: no pair outputs) -- adds
    'pairs': Session.pairs' dict for all K subsets, 'result_both' / 'result_diff' (200 x C2: the K subsets'
    grids of p_a p_b and p_a - p_b combined by `method`, on the host copies of all K grids: K 200 C2 8 bytes
    per functional) and 'pairs_combined': {'both': map_grid of result_both with the thresholds, 'diff':
    map_grid of result_diff with the threshold 0 -- its exc_1 is the combined P(p_a > p_b)}.  Needs x_test."""
    lib = _lib.load()
    if method not in ("mean", "median"):
        raise ValueError(f"error: unknown combine method '{method}'")
    pp = PackedProblem(subsets, cfg, coords_test, subset_base, x_test=x_test)
    c, keep = cfg.to_c(device=0, record_w=record_w or w_samples)
    devs = np.ascontiguousarray(devices, dtype=np.int32)
    K, P, q, n_test = pp.S, cfg.P, cfg.q, pp.n_test
    C = q * n_test
    have = n_test > 0
    have_x = pp.x_test is not None and have
    if (p_pred_samples or p_predict_sum) and not have_x:
        raise ValueError("error: p_pred_samples / p_predict_sum need x_test")
    on = dict(parameters=per_subset, w_predict=per_subset and have, samples=samples, w_samples=w_samples,
              w_pred_samples=w_pred_samples and have, acceptance=acceptance, w_predict_sum=w_predict_sum and have,
              p_predict=per_subset and have_x, p_pred_samples=p_pred_samples, p_predict_sum=p_predict_sum)
    ob = OutputBuffers(K, cfg, pp.n_part, n_test, cfg.kept, {f for f, v in on.items() if v})
    cb = Combined()
    result = np.zeros((P, N_LEVELS))
    cb.result = _lib.dptr(result)
    result2 = np.zeros((C, N_LEVELS)) if n_test else None
    cb.result2 = _lib.dptr(result2) if n_test else None
    result3 = np.zeros((C, N_LEVELS)) if have_x else None
    cb.result3 = _lib.dptr(result3)
    cb.method = _lib.MK_COMBINE_MEDIAN if method == "median" else _lib.MK_COMBINE_MEAN
    cb.max_iter, cb.tol = int(max_iter), float(tol)

    def _cb(user, it, n):
        try:
            return 1 if (progress is not None and progress(int(it), int(n))) else 0
        except Exception:       # an exception in the callback stops the fit as an interrupt
            return 1

    fn = _lib.PROGRESS_FN(_cb)
    db = None
    if diagnostics:
        kinds = ["parameters"] + (["w_predict"] if have else []) + (["p_predict"] if have_x else [])
        db = DiagnosticBuffers(K, cfg, n_test, {k + sfx for k in kinds for sfx in ("_diag", "_diag_worst")})
    kb = CriteriaBuffers(K, q, pp.n_part, pointwise=criteria == "pointwise") if criteria else None
    sb = val = None
    if validation is not None:
        if not have_x:
            raise ValueError("error: validation needs test sites and x_test")
        if isinstance(validation, dict):
            vy, vw, vpw = validation["y_test"], validation.get("weights_test", 1), validation.get("pointwise", False)
        elif isinstance(validation, tuple):
            (vy, vw), vpw = validation, False
        else:
            vy, vw, vpw = validation, 1, False
        val = validation_arrays(vy, vw, C)
        sb = ScoreBuffers(K, C, pointwise=bool(vpw), combined=True)
    mb = spec = None
    if maps is not None:
        if not have_x:
            raise ValueError("error: maps need test sites and x_test")
        spec = map_spec(maps)
        mb = MapBuffers(K, C, spec[0].size, combined=True)
    pb = pspec = None
    if pairs is not None:
        if not have_x:
            raise ValueError("error: pairs need test sites and x_test")
        pspec = pair_spec(pairs)
        pb = PairBuffers(K, q, n_test, pspec[0].size, combined=True)
    check(lib.mk_meta_fit_pairs(ctypes.byref(pp.c), ctypes.byref(c), devs.ctypes.data_as(_lib._ip), len(devs), fn, None,
                                ctypes.byref(ob.c), ctypes.byref(cb), ctypes.byref(db.c) if db is not None else None,
                                ctypes.byref(kb.c) if kb is not None else None,
                                ctypes.byref(val[2]) if val is not None else None,
                                ctypes.byref(sb.c) if sb is not None else None,
                                ctypes.byref(spec[1]) if spec is not None else None,
                                ctypes.byref(mb.c) if mb is not None else None,
                                ctypes.byref(pspec[1]) if pspec is not None else None,
                                ctypes.byref(pb.c) if pb is not None else None))
    del keep
    out = {"result": result.T.copy(), "result2": None if result2 is None else result2.T.copy(),
           "exchange": "rccl" if cb.exchange else "copy", "comm_ranks": int(cb.comm_ranks)}
    if result3 is not None:
        out["result3"] = result3.T.copy()
    out.update(ob.unpack())
    if db is not None:
        out.update(db.unpack())
    if kb is not None:
        out["criteria"] = kb.unpack()
    if sb is not None:
        out["scores"] = sb.unpack()
    if mb is not None:
        out["maps"] = mb.unpack(spec[0])
        out["maps_combined"] = out["maps"].pop("combined")
    if pb is not None:
        out["pairs"] = pb.unpack(pspec[0])
        out["result_both"], out["result_diff"] = out["pairs"].pop("combined_both"), out["pairs"].pop("combined_diff")
        dev = int(devs[0])
        out["pairs_combined"] = {"both": map_grid(out["result_both"], pspec[0], device=dev),
                                 "diff": map_grid(out["result_diff"], (0.0,), device=dev)}
    return out
