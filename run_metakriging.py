#!/usr/bin/env python3
"""MetaKriging_BinaryResponse.R end to end on the MI355X path, one process per GPU.

The reference script's flow with its drop-ins (MK.R line numbers):
  data (the driver the reference lacks)   -> synthetic.generate
  partition                      MK.R:15-41             -> metakriging.partition
  glm start values               MK.R:53-55             -> glm_binomial (device, once)
  foreach %dopar% worker         MK.R:100-114           -> Session: every subset of the shard at once
     spMvGLM + spPredict + quantiles  MK.R:80-89
  combine                        MK.R:119-133           -> combine / combine_median / column-sharded (N > 1)
  resample + p(y=1) + summaries  MK.R:136-165           -> posterior_summary (device)

Prints one JSON line with the wall-clock of every phase (rank 0).  Multi-GPU:
  python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 run_metakriging.py ...

  python run_metakriging.py --config 3          # configs[2]: n=500k, K=250, exponential, q=1
"""
import argparse
import os

# before HIP starts: libmk's lookahead schedule runs up to five HIP streams and HIP shares
# hardware queues beyond GPU_MAX_HW_QUEUES (4 by default)
if int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0) < 8:
    os.environ["GPU_MAX_HW_QUEUES"] = "8"
import importlib
import json
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"

# BASELINE.json configs (1-based as in SURVEY.md): n, K, cov, q, n_test, n_batch x batch_length
CONFIGS = {
    1: dict(n=2000, K=5, cov="exponential", q=1, n_test=1000, n_batch=20, batch_length=50),
    2: dict(n=50000, K=50, cov="matern", q=1, n_test=1000, n_batch=100, batch_length=50),
    3: dict(n=500000, K=250, cov="exponential", q=1, n_test=1000, n_batch=100, batch_length=50),
    4: dict(n=100000, K=50, cov="exponential", q=3, n_test=1000, n_batch=100, batch_length=50),
    5: dict(n=500000, K=250, cov="exponential", q=1, n_test=1000000, n_batch=100, batch_length=50,
            predict_tile=65536),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=1, choices=sorted(CONFIGS))
    ap.add_argument("--n", type=int)
    ap.add_argument("--subsets", type=int)
    ap.add_argument("--n-test", type=int)
    ap.add_argument("--n-batch", type=int)
    ap.add_argument("--batch-length", type=int)
    ap.add_argument("--combine", default="mean", choices=["mean", "median"])
    ap.add_argument("--predict-tile", type=int)
    ap.add_argument("--seed", type=int, default=20250114)
    ap.add_argument("--partition", default="R", choices=["R", "permutation"],
                    help="R: the subsets R draws after set.seed(seed) (mk_partition_r)")
    ap.add_argument("--devices", default=None,
                    help="one process, libmk's multi-device driver (mk_meta_fit) over these HIP devices, e.g. "
                         "0,1,2,3,4,5,6,7 (a device may repeat: several shards on one GPU, device-copy exchange)")
    ap.add_argument("--diagnostics", action="store_true",
                    help="chain diagnostics (ess, mcse, split R-hat per kept chain, on the device): one more JSON "
                         "line after the summary, {\"diagnostics\": convergence_report(...)}; one process (plain or "
                         "--devices)")
    ap.add_argument("--criteria", action="store_true",
                    help="model assessment (DIC and WAIC, accumulated on the device over the kept iterations): one "
                         "more JSON line, {\"criteria\": the rows summed over the subsets}; one process (plain or "
                         "--devices)")
    ap.add_argument("--loo", action="store_true",
                    help="PSIS-LOO (leave-one-out elpd and the Pareto shape k-hat per observation, on the device, "
                         "replayed from the recorded chain over the kept iterations): one more JSON line, {\"loo\": "
                         "the total row by name}; one process, plain path")
    ap.add_argument("--validate", action="store_true",
                    help="held-out validation against y.test (log score, Brier score, error rate on the device): "
                         "one more JSON line, {\"validation\": the combined p grid's row, the median subset's row, "
                         "AUC}; several ranks: rank 0 scores the combined grid, per-subset rows are left out")
    ap.add_argument("--maps", default=None, metavar="U1,U2,...",
                    help="posterior maps of the combined posterior, e.g. 0.2,0.5 (at most 8 thresholds on the "
                         "probability scale; '' for none): per test column the mean and sd of w and of p(y = 1) "
                         "and P(p > u) per threshold, made on the device and saved as a (q n_test) x (4 + J) "
                         ".npy (--maps-out); one more JSON line, {\"maps\": the file, the planes' names, per "
                         "threshold the share of sites whose exceedance probability is >= 0.95}")
    ap.add_argument("--maps-out", default="maps_combined.npy", help="where --maps saves the combined planes")
    ap.add_argument("--pairs", default=None, metavar="U1,U2,...",
                    help="cross-outcome prediction of a multivariate config (q >= 2: --config 4), e.g. 0.2,0.5 (at most "
                         "8 thresholds; '' for none): per test site and outcome pair (a, b) the combined 200-level "
                         "grids of p_a p_b (both occur) and p_a - p_b, saved as 200 x C2 .npy, and their planes "
                         "(mean, sd, exceedances; of the difference P(diff > 0)) saved as .npy (--pairs-out is the "
                         "prefix); one more JSON line, {\"pairs\": the files, per pair the share of sites with "
                         "combined P(p_a > p_b) >= 0.95}; one process (plain or --devices)")
    ap.add_argument("--pairs-out", default="pairs", help="prefix of the files --pairs saves")
    ap.add_argument("--variogram", type=int, nargs="?", const=15, default=None, metavar="N_BINS",
                    help="before the fit, the empirical variogram of the start-value glm's Pearson residuals over "
                         "all pairs of sites, on the device (15 bins up to a third of the bounding box's diagonal; "
                         "at most 64): the table per outcome on stderr, saved as n_bins x (4 + T) .npy (from, to, "
                         "pairs, h, gamma per outcome pair; --variogram-out), and one more JSON line, {\"variogram\": "
                         "the exponential fits and the phi start and prior they suggest}; with --validate also the "
                         "variogram of the held-out residuals of the combined grid, {\"heldout_variogram\": ...}: "
                         "structure left there is misfit.  Not with --devices")
    ap.add_argument("--variogram-out", default="variogram.npy", help="where --variogram saves its table")
    ap.add_argument("--phi-from-variogram", action="store_true",
                    help="start phi at the residual variogram's fitted decay and put its uniform prior around the fitted "
                         "range (suggest_phi: the reference's own ratios) instead of MK.R:60-63's 3/0.5 and "
                         "Unif(3/0.75, 3/0.25); implies --variogram.  Off by default: without it nothing about the fit "
                         "changes")
    ap.add_argument("--save-fit", default=None, metavar="DIR",
                    help="after the chain, save the session (data, configuration, p.beta.theta.samples, p.w.samples) as "
                         "DIR/session_0.npz (fitfile.save_session): the session then keeps its chain states and records w "
                         "(a kriging tile even where the config has none) instead of fusing the kriging into the kept "
                         "iterations.  One process; not with --devices.  Off by default: without it nothing about a run "
                         "changes")
    ap.add_argument("--from-fit", default=None, metavar="DIR",
                    help="skip the partition, the start-value glm and the MCMC: load DIR/session_0.npz (--save-fit), "
                         "krige this run's test sites from its recorded chain, combine and summarise as usual.  One "
                         "process; not with --devices")
    ap.add_argument("--checkpoint", default=None, metavar="DIR",
                    help="write the running chain's state to DIR/shard<first subset>.npz (fitfile.save_checkpoint: the "
                         "data, the configuration and everything a later process needs to continue the chain bit for "
                         "bit), once at the end of the chain and, with --checkpoint-every, on the way; each write replaces "
                         "the file atomically.  Not with --devices, --save-fit or --from-fit.  Off by default: without it "
                         "nothing about a run changes")
    ap.add_argument("--checkpoint-every", type=int, default=0, metavar="N",
                    help="with --checkpoint: also write after every N amcmc batches")
    ap.add_argument("--resume", default=None, metavar="DIR",
                    help="continue the chain of DIR/shard<first subset>.npz (--checkpoint) to n.samples instead of "
                         "starting one, then go on with the flow as usual; the file must hold this run's subsets and "
                         "configuration (the first key that differs is named).  Not with --devices, --save-fit or "
                         "--from-fit")
    a = ap.parse_args()
    a.map_thresholds = None if a.maps is None else [float(u) for u in a.maps.split(",") if u.strip()]
    a.pair_thresholds = None if a.pairs is None else [float(u) for u in a.pairs.split(",") if u.strip()]
    c = dict(CONFIGS[a.config])
    for k_arg, k_cfg in [("n", "n"), ("subsets", "K"), ("n_test", "n_test"), ("n_batch", "n_batch"),
                         ("batch_length", "batch_length"), ("predict_tile", "predict_tile")]:
        v = getattr(a, k_arg)
        if v is not None:
            c[k_cfg] = v
    if a.pair_thresholds is not None and c["q"] < 2:
        ap.error(f"--pairs needs a multivariate config: --config {a.config} has q = {c['q']} (--config 4 is q = 3)")
    if a.phi_from_variogram and a.variogram is None:
        a.variogram = 15
    if a.save_fit is not None and a.from_fit is not None:
        ap.error("--save-fit and --from-fit: a run either makes the chain and saves it, or loads it")
    if a.checkpoint_every and a.checkpoint is None:
        ap.error("--checkpoint-every needs --checkpoint DIR")
    if a.checkpoint_every < 0:
        ap.error("--checkpoint-every counts amcmc batches: 0 (the end of the chain alone) or more")
    if (a.checkpoint is not None or a.resume is not None) and (a.devices is not None or a.save_fit is not None or
                                                               a.from_fit is not None):
        ap.error("--checkpoint and --resume run in the plain path (one process per GPU), not with --devices, --save-fit or "
                 "--from-fit")
    if a.devices is not None:
        if a.save_fit is not None or a.from_fit is not None:
            ap.error("--save-fit and --from-fit run in the plain path (one process), not with --devices")
        if a.variogram is not None:
            ap.error("--variogram and --phi-from-variogram run in the plain path (one process per GPU), not with --devices")
        if a.loo:
            ap.error("--loo runs in the plain path (one process), not with --devices")
        return node_main(a, c)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.diagnostics and world > 1:
        ap.error("--diagnostics runs in one process: plain, or over several GPUs with --devices")
    if a.criteria and world > 1:
        ap.error("--criteria runs in one process: plain, or over several GPUs with --devices")
    if a.loo and world > 1:
        ap.error("--loo runs in one process")
    if a.pair_thresholds is not None and world > 1:
        ap.error("--pairs runs in one process: plain, or over several GPUs with --devices")
    if (a.save_fit is not None or a.from_fit is not None) and world > 1:
        ap.error("--save-fit and --from-fit run in one process")
    if a.from_fit is not None and a.variogram is not None:
        ap.error("--variogram looks at the start-value glm's residuals, which --from-fit skips")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # the combined grid of p(y = 1), result3; the pairs need x.test on the device as it does
    need_p = a.validate or a.map_thresholds is not None or a.pair_thresholds is not None
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", rank=rank, world_size=world)
    mk = importlib.import_module(PKG)
    dmod = importlib.import_module(PKG + ".distributed")
    t = {}
    t0 = time.perf_counter()
    q, n, K = c["q"], c["n"], c["K"]
    d = mk.synthetic.generate(n, q=q, n_test=c["n_test"], cov_model=1 if c["cov"] == "matern" else 0, seed=a.seed)
    t["data_s"] = time.perf_counter() - t0

    t1 = time.perf_counter()
    vario, phi_kw = None, {}
    ses = None
    if a.from_fit is None:
        n_part, index_part = mk.partition(n, K, seed=a.seed, method=a.partition)                     # MK.R:15-41
        beta0, bt = mk.start_values(d["y"], d["x"], 1.0, q, device=local)         # MK.R:53-55
        p = d["x"].shape[1]
        if a.variogram is not None:               # every rank: the suggestion is a function of the data alone
            vario = residual_variogram_before(mk, d, q, a, local, report=rank == 0)
            if a.phi_from_variogram:
                phi_kw = dict(phi_starting=vario["suggestion"]["starting"], phi_unif=vario["suggestion"]["unif"])
        # --save-fit: a tiled session (it keeps its chain states) whatever the config's tile
        tile_cfg = c.get("predict_tile", 0) or (65536 if a.save_fit is not None else 0)
        cfg = mk.SamplerConfig(q, p, beta0, bt, cov_model=c["cov"], n_batch=c["n_batch"], batch_length=c["batch_length"],
                               seed=a.seed, predict_tile=tile_cfg, **phi_kw)
        lo, hi = dmod.shard_range(K, world, rank)
        subs = [mk.subset_data(d["y"], d["x"], 1.0, d["coords"], q, index_part[i]) for i in range(lo, hi)]
    else:                                         # the chain of an earlier run: no partition, glm or MCMC
        ses = mk.fitfile.load_session(os.path.join(a.from_fit, "session_0.npz"), device=local, predict_tile=a.predict_tile)
        cfg = ses.cfg
        if cfg.q != q:
            raise SystemExit(f"--from-fit: the file's fit has q = {cfg.q}, --config {a.config} has q = {q}")
        K, lo = ses.S, 0
        c["K"], c["n_batch"], c["batch_length"] = K, cfg.n_batch, cfg.batch_length
        subs = [None] * K                         # only their number is read below
    kept_states = a.save_fit is not None or a.from_fit is not None    # the session takes its test sites after creation
    t["setup_s"] = time.perf_counter() - t1

    t2 = time.perf_counter()
    big = cfg.predict_tile > 0 and cfg.predict_tile < c["n_test"]
    C = q * c["n_test"]
    P = cfg.P
    if subs:
        # one process, fused kriging: x.test goes in as MK.R:87 passes it, p.predict comes out
        x_test = d["x_test"] if ((world == 1 and not big) or need_p) else None   # MK.R:108
        ckpt_file = f"shard{lo}.npz"
        if a.resume is not None:                  # the chain of an earlier process, continued below
            ses = mk.fitfile.load_checkpoint(os.path.join(a.resume, ckpt_file), device=local, data=subs, cfg=cfg,
                                             record_w=a.loo, criteria=a.criteria)
            if rank == 0:
                print(f"resumed at iteration {ses.iteration}/{cfg.n_samples}", file=sys.stderr, flush=True)
        elif not kept_states:
            ses = mk.Session(subs, cfg, coords_test=d["coords_test"], subset_base=lo, device=local, x_test=x_test,
                             criteria=a.criteria, record_w=a.loo)     # --loo replays the recorded chain
        else:     # no test sites at creation: the session keeps every kept state; --criteria replays the recorded chain
            if ses is None:
                ses = mk.Session(subs, cfg, subset_base=lo, device=local, record_w=True)
            ses.set_test_sites(d["coords_test"], x_test=x_test)
        if a.validate and world == 1:             # scored per subset: now (fused) or by the tile replays
            ses.set_validation(d["y_test"])
        if a.pair_thresholds is not None:         # filled now (fused) or by the tile replays
            ses.set_pairs(a.pair_thresholds)
        it = ses.iteration if a.from_fit is None else cfg.n_samples     # > 0 after --resume, mid-batch where it stopped
        while it < cfg.n_samples:                 # progress every n.report = 10 batches (MK.R:84)
            step = cfg.batch_length - it % cfg.batch_length
            ses.run(step)
            it += step
            b = it // cfg.batch_length
            if rank == 0 and b % 10 == 0:
                print(f"batch {b}/{cfg.n_batch}  {time.perf_counter() - t2:.1f}s", file=sys.stderr, flush=True)
            if a.checkpoint is not None and ((a.checkpoint_every and b % a.checkpoint_every == 0) or it == cfg.n_samples):
                os.makedirs(a.checkpoint, exist_ok=True)
                mk.fitfile.save_checkpoint(ses, os.path.join(a.checkpoint, ckpt_file))
        if a.save_fit is not None:
            os.makedirs(a.save_fit, exist_ok=True)
            mk.fitfile.save_session(ses, os.path.join(a.save_fit, "session_0.npz"))
        t3 = time.perf_counter()
        # 1M sites (tiled kriging): the parameter grids now; w.predict tile by tile in the combine
        # one process: the grids to the host for the combine; N > 1: they stay in HBM (shard_grids below)
        # --diagnostics: with the grids when the kriging is fused; tiled: the parameters now, the draws tile by tile
        dg = ("parameters" if big else True) if a.diagnostics else False
        out = (ses.outputs(quantiles=True, w_predict=not big, p_predict=False if big else None, diagnostics=dg)
               if world == 1
               else {"parameters": [], "w_predict": []})
        crit = ses.criteria() if a.criteria else None
        loo = ses.loo() if a.loo else None
        scores = ses.scores() if (a.validate and world == 1 and not big) else None
    else:                                         # K < world: this rank has no subsets, it joins the exchange
        t3 = time.perf_counter()
        out = {"parameters": [], "w_predict": []}
        crit = scores = None
    t["fit_s"] = t3 - t2
    t["predict_quantiles_s"] = time.perf_counter() - t3
    diag = {k: v for k, v in out.items() if "_diag" in k}

    t4 = time.perf_counter()
    result3 = None
    par = np.stack(out["parameters"]) if out["parameters"] else np.zeros((0, 200, P))
    tile = ses.predict_tile if ses is not None else cfg.predict_tile   # the tile in use (HBM may shrink it)

    def tile_grids(t0):                           # this shard's grids of one test-site tile (kriging replay)
        tc = min(tile, c["n_test"] - t0)
        return ses.tile_grids(t0) if ses is not None else np.zeros((0, 200, q * tc))

    if world > 1:
        import torch
        dev = torch.device("cuda", local)

        def shard_grids(which, ncol):   # this shard's (S, 200, ncol) grids, written by libmk into HBM
            g = torch.empty((len(subs), ncol, 200), dtype=torch.float64, device=dev)
            if ses is not None:
                ses.grids_device(which, g.data_ptr())
            return g.transpose(1, 2)

        result = dmod.combine_sharded(shard_grids(0, P), K, dist, method=a.combine, device=dev, gpu=local)   # MK.R:123-127
        if big:   # the exchange runs tile by tile: every rank must replay the same tiles
            tl = torch.tensor([tile, -tile], dtype=torch.int64, device=dev)
            dist.all_reduce(tl, op=dist.ReduceOp.MIN)
            if int(tl[0]) != -int(tl[1]):
                raise SystemExit(f"ranks took different kriging tiles ({int(tl[0])} .. {-int(tl[1])} test sites: HBM "
                                 f"limits differ); pass --predict-tile {int(tl[0])} or less")
        if not big:
            result2 = dmod.combine_sharded(shard_grids(1, C), K, dist, method=a.combine, device=dev, gpu=local)
            if need_p:
                result3 = dmod.combine_sharded(shard_grids(2, C), K, dist, method=a.combine, device=dev, gpu=local)
        else:
            # tiled kriging (cfg5): per test-site tile, the column-sharded exchange + combine of that
            # tile's grids (sequential mean, or the Weiszfeld median per column)
            result2 = dmod.combine_tiles(tile_grids, c["n_test"], tile, q, K, dist, method=a.combine, device=dev,
                                         gpu=local)
            if need_p:          # the p grids of every tile: a second replay (the exchange takes one kind at a time)
                def tile_grids_p(t0):
                    tc = min(tile, c["n_test"] - t0)
                    return ses.tile_grids(t0, prob=True)[1] if ses is not None else np.zeros((0, 200, q * tc))
                result3 = dmod.combine_tiles(tile_grids_p, c["n_test"], tile, q, K, dist, method=a.combine, device=dev,
                                             gpu=local)
    elif not big:
        obj = [{"parameters": out["parameters"][i], "w.predict": out["w_predict"][i]} for i in range(len(subs))]
        result, result2 = mk.combine_results(obj, device=local, method=a.combine)             # MK.R:123-133
        if "p_predict" in out:
            result3 = mk.metakriging.combine_predictive([{"p.predict": g} for g in out["p_predict"]], device=local,
                                                        method=a.combine)
    else:   # tiled kriging (cfg5), one process: every tile's K grids combined as they are replayed
        result = mk.combine_results([{"parameters": g} for g in out["parameters"]], device=local,
                                    method=a.combine)[0]
        result2 = np.zeros((200, C))
        if need_p:
            result3 = np.zeros((200, C))
        if a.diagnostics:    # the worst rows over the subsets, filled tile by tile from each tile's own replay
            diag["w_predict_diag_worst"] = np.zeros((3, C))
        for t0 in range(0, c["n_test"], tile):
            if a.diagnostics or need_p:         # one replay: the grids, the tile's diagnostics and its scores
                res = ses.tile_grids(t0, prob=need_p, diagnostics=a.diagnostics)
                g = res[0] if isinstance(res, tuple) else res
                if a.diagnostics:
                    diag["w_predict_diag_worst"][:, t0 * q:t0 * q + g.shape[2]] = res[-1]["w_predict_diag_worst"]
                if need_p:
                    result3[:, t0 * q:t0 * q + g.shape[2]] = mk.combine_results(
                        [{"parameters": x} for x in res[1]], device=local, method=a.combine)[0]
            else:
                g = tile_grids(t0)
            result2[:, t0 * q:t0 * q + g.shape[2]] = mk.combine_results([{"parameters": x} for x in g], device=local,
                                                                        method=a.combine)[0]
            del g
            print(f"tile {t0 // tile + 1}/{(c['n_test'] + tile - 1) // tile}  {time.perf_counter() - t4:.1f}s",
                  file=sys.stderr, flush=True)
    if a.validate and world == 1 and big:
        scores = ses.scores()                     # every tile has been replayed
    pair_grids = None
    if a.pair_thresholds is not None:             # fused: made now; tiled: every tile has been replayed
        pr = ses.pairs(planes=False)
        comb = mk.metakriging.combiner(a.combine, local)
        pair_grids = (pr["pairs"], comb(pr["both_predict"]), comb(pr["diff_predict"]))
    krig = None
    if ses is not None and big:                   # how this shard's tiles were kriged (any q)
        cheb, fb = (ses.kernel_stats(k) for k in (mk.session.KS_KRIG_CHEB, mk.session.KS_KRIG_FALLBACK))
        n_int = cheb["launches"]
        krig = {"mode": os.environ.get("MK_KRIG_CHEB", "1"), "tile": int(tile),
                "interpolated_tiles": n_int, "fallback_tiles": fb["launches"],
                "exact_evaluations_per_pair_and_tile": cheb["flops"] / (n_int * len(subs) * q) if n_int else None,
                "max_check_difference": cheb["ms"] if n_int else None}
    if ses is not None:
        ses.close()
    t["combine_s"] = time.perf_counter() - t4

    t5 = time.perf_counter()
    summ = None
    if result is not None:
        summ = mk.posterior_summary(result, result2, d["x_test"], samplesize=1000, seed=a.seed, device=local)
    t["post_s"] = time.perf_counter() - t5
    t["end_to_end_s"] = time.perf_counter() - t1
    if rank == 0:
        rec = dict(config=a.config, workload=c, n_gpus=world, combine=a.combine, phases=t,
                   subset_iters_per_s=K * cfg.n_samples / (t["fit_s"]) if world == 1 and a.from_fit is None else None)
        if summ is not None:
            truth = np.concatenate([d["beta_true"], [1.0] if q == 1 else [], [6.0] if q == 1 else []])
            rec["param_median"] = summ["param_quant"][0].tolist()
            rec["param_95ci"] = [summ["param_quant"][1].tolist(), summ["param_quant"][2].tolist()]
            wq = summ["w_quant"]
            rec["w_test_coverage_95"] = float(np.mean((d["w_test_true"] >= wq[1]) & (d["w_test_true"] <= wq[2])))
            rec["truth_beta_phi"] = truth.tolist()
            rec.update(predictive_scores(result3, d))
        if krig is not None:
            rec["kriging_replay"] = krig
        print(json.dumps(rec), flush=True)
        if a.diagnostics:
            print(json.dumps({"diagnostics": mk.convergence_report(diag)}), flush=True)
        if a.criteria:
            print(json.dumps({"criteria": dict(zip(crit["names"], crit["total"].tolist()))}), flush=True)
        if a.loo:
            print(json.dumps({"loo": dict(zip(loo["names"], loo["total"].tolist()))}), flush=True)
        if vario is not None:
            print(json.dumps({"variogram": vario["line"]}), flush=True)
        if a.validate and result3 is not None:
            print(json.dumps({"validation": validation_line(mk, result3, d, scores, local)}), flush=True)
            if a.variogram is not None:
                print(json.dumps({"heldout_variogram": heldout_variogram_line(mk, result3, d, a, local)}), flush=True)
        if a.map_thresholds is not None and result3 is not None:
            w, p = (mk.map_grid(np.asarray(g), u, device=local) for g, u in ((result2, ()), (result3, a.map_thresholds)))
            names = ["w_" + k for k in w["names"]] + ["p_" + k for k in p["names"][:2]] + p["names"][2:]
            print(json.dumps({"maps": maps_line(np.hstack([w["planes"], p["planes"]]), names, a)}), flush=True)
        if pair_grids is not None:
            pl = {"both": mk.map_grid(pair_grids[1], a.pair_thresholds, device=local),
                  "diff": mk.map_grid(pair_grids[2], (0.0,), device=local)}
            print(json.dumps({"pairs": pairs_line(pair_grids[0], pair_grids[1], pair_grids[2], pl, a)}), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def predictive_scores(result3, d):
    """Held-out scores of the combined grid of p(y = 1) (result3, 200 x q n_test; levels 0.005 .. 1):
    the Brier score of its median against y.test, and how often the generating probability
    logistic(x.test beta + w) lies in its 2.5 % .. 97.5 % band."""
    if result3 is None:
        return {}
    med, lo, hi = result3[99], result3[4], result3[194]
    p_true = 1.0 / (1.0 + np.exp(-(d["x_test"] @ d["beta_true"] + d["w_test_true"])))
    return {"p_test_brier": float(np.mean((med - d["y_test"]) ** 2)),
            "p_test_coverage_95": float(np.mean((p_true >= lo) & (p_true <= hi)))}


def validation_line(mk, result3, d, scores, device):
    """The combined p grid's held-out row (score_grid on the device), AUC of its pmean, and -- where the
    per-subset rows exist -- the median subset's row."""
    comb = mk.score_grid(np.asarray(result3), d["y_test"], pointwise=True, device=device)
    rep = mk.validation_report(comb.pop("pointwise")[:, 0], d["y_test"])
    line = {"combined": comb, "auc": rep["auc"]}
    if scores is not None:
        line["median_subset"] = mk.metakriging.median_subset_row(scores)
    return line


def finite_or_none(v):
    """A list for a JSON line: None where a bin is empty (NaN)."""
    return [float(x) if np.isfinite(x) else None for x in v]


def variogram_fits(mk, vg):
    """Per outcome the exponential fit of its direct variogram, and the table on stderr."""
    vmod = importlib.import_module(PKG + ".variogram")
    fits = []
    for t, (i, j) in enumerate(vg["pairs"]):
        if i == j:
            print(vmod.table(vg, pair=t), file=sys.stderr, flush=True)
            fits.append(mk.fit_exponential(vg, pair=t))
    return fits


def residual_variogram_before(mk, d, q, a, device, report):
    """--variogram before the fit: the variogram of the start-value glm's Pearson residuals over all pairs of
    sites, its table (n_bins x (4 + T): from, to, pairs, h, gamma per outcome pair) saved, the fits and the phi
    start and prior they suggest."""
    n = d["coords"].shape[0]
    r = mk.glm_residuals(d["y"], d["x"], 1.0, device=device)
    vg = mk.variogram(d["coords"], r.reshape(n, q), n_bins=a.variogram, device=device)
    if not report:
        return {"suggestion": mk.suggest_phi(vg), "line": None}
    fits = variogram_fits(mk, vg)
    sug = mk.suggest_phi(vg, fits=fits)
    np.save(a.variogram_out, np.column_stack([vg["edges"][:-1], vg["edges"][1:], vg["count"], vg["h"], vg["gamma"].T]))
    line = {"file": a.variogram_out, "n_bins": vg["n_bins"], "max_dist": vg["max_dist"], "pairs": int(vg["count"].sum()),
            "device_ms": vg["ms"], "fits": fits, "phi_starting": sug["starting"].tolist(),
            "phi_unif": [sug["unif"][0].tolist(), sug["unif"][1].tolist()], "used_for_the_fit": bool(a.phi_from_variogram)}
    print(f"suggested phi start {line['phi_starting']} and uniform prior {line['phi_unif']} (exploratory: a residual "
          "variogram of binary data is noisy and attenuated)", file=sys.stderr, flush=True)
    return {"suggestion": sug, "line": line}


def heldout_variogram_line(mk, result3, d, a, device):
    """--variogram with --validate: the variogram of the held-out Pearson residuals of the combined grid's
    pmean (score_grid's pointwise column); spatial structure left in it is misfit."""
    pmean = mk.score_grid(np.asarray(result3), d["y_test"], pointwise=True, device=device)["pointwise"][:, 0]
    vg = mk.residual_variogram(d["coords_test"], d["y_test"], 1.0, pmean, n_bins=a.variogram, device=device)
    fits = variogram_fits(mk, vg)
    return {"n_bins": vg["n_bins"], "max_dist": vg["max_dist"], "pairs": int(vg["count"].sum()), "device_ms": vg["ms"],
            "count": vg["count"].tolist(), "h": finite_or_none(vg["h"]), "gamma": [finite_or_none(g) for g in vg["gamma"]],
            "fits": fits}


def maps_line(planes, names, a):
    """Saves the combined planes ((q n_test) x (4 + J)) and summarises them: per threshold the share of
    test columns whose exceedance probability is >= 0.95."""
    np.save(a.maps_out, planes)
    exc = planes[:, 4:]
    return {"file": a.maps_out, "names": list(names), "thresholds": a.map_thresholds,
            "share_exc_ge_0.95": [float(np.mean(exc[:, j] >= 0.95)) for j in range(exc.shape[1])]}


def pairs_line(pairs, both, diff, planes, a):
    """Saves the combined pair grids (200 x C2 each) and their planes (map_grid's: C2 x (2 + J) of `both`, C2 x 3
    of `diff`, whose last column is the combined P(p_a > p_b)) and summarises them: per outcome pair the share
    of test sites where that probability is >= 0.95."""
    files = {k: f"{a.pairs_out}_{k}.npy" for k in ("both", "diff", "both_planes", "diff_planes")}
    np.save(files["both"], both)
    np.save(files["diff"], diff)
    np.save(files["both_planes"], planes["both"]["planes"])
    np.save(files["diff_planes"], planes["diff"]["planes"])
    gt = planes["diff"]["planes"][:, 2].reshape(-1, len(pairs))      # site-major pair columns
    return {"files": files, "pairs": [list(ab) for ab in pairs], "thresholds": a.pair_thresholds,
            "both_names": planes["both"]["names"], "diff_names": planes["diff"]["names"],
            "share_a_gt_b_ge_0.95": [float(np.mean(gt[:, r] >= 0.95)) for r in range(len(pairs))]}


def node_main(a, c):
    """The script in one process over a device list (mk_meta_fit): shards, combine (mean or median,
    per test-site tile at configs[4]) and post-processing without torch or a second process."""
    mk = importlib.import_module(PKG)
    devices = [int(x) for x in a.devices.split(",")]
    t0 = time.perf_counter()
    q, n, K = c["q"], c["n"], c["K"]
    d = mk.synthetic.generate(n, q=q, n_test=c["n_test"], cov_model=1 if c["cov"] == "matern" else 0, seed=a.seed)
    data_s = time.perf_counter() - t0

    def progress(it, n_samples):
        if it % (10 * c["batch_length"]) == 0:    # n.report = 10 batches (MK.R:84)
            print(f"iterations {it}/{n_samples}  {time.perf_counter() - t0:.1f}s", file=sys.stderr, flush=True)
        return False

    ph, result, result2, summ, cfg = mk.metakriging.reference_flow(
        d, K, q, cov_model=c["cov"], n_batch=c["n_batch"], batch_length=c["batch_length"], seed=a.seed,
        devices=devices, method=a.combine, predict_tile=c.get("predict_tile", 0), partition_method=a.partition,
        progress=progress, predictive=True,     # MK.R:87's x.test: the grids of p(y = 1) and result3
        diagnostics=a.diagnostics, criteria=a.criteria, validate=a.validate, maps=a.map_thresholds,
        pairs=a.pair_thresholds)
    ph["data_s"] = data_s
    rec = dict(config=a.config, workload=c, devices=devices, combine=a.combine, phases=ph,
               subset_iters_per_s=K * cfg.n_samples / ph["chains_s"])
    truth = np.concatenate([d["beta_true"], [1.0] if q == 1 else [], [6.0] if q == 1 else []])
    rec["param_median"] = summ["param_quant"][0].tolist()
    rec["param_95ci"] = [summ["param_quant"][1].tolist(), summ["param_quant"][2].tolist()]
    wq = summ["w_quant"]
    rec["w_test_coverage_95"] = float(np.mean((d["w_test_true"] >= wq[1]) & (d["w_test_true"] <= wq[2])))
    rec["truth_beta_phi"] = truth.tolist()
    rec.update(predictive_scores(summ.get("result3"), d))
    print(json.dumps(rec), flush=True)
    if a.diagnostics:
        print(json.dumps({"diagnostics": mk.convergence_report(summ["diagnostics"])}), flush=True)
    if a.criteria:
        print(json.dumps({"criteria": summ["criteria"]}), flush=True)
    if a.validate:
        v = summ["validation"]
        print(json.dumps({"validation": {"combined": v["combined"], "median_subset": v["median_subset"],
                                         "auc": v["report"]["auc"]}}), flush=True)
    if a.map_thresholds is not None:
        print(json.dumps({"maps": maps_line(summ["maps"]["combined"], summ["maps"]["names"], a)}), flush=True)
    if a.pair_thresholds is not None:
        pr = summ["pairs"]
        print(json.dumps({"pairs": pairs_line(pr["pairs"], pr["result_both"], pr["result_diff"], pr["combined"], a)}),
              flush=True)


if __name__ == "__main__":
    main()
