#!/usr/bin/env python3
"""configs[3]'s per-GPU share with a tiled prediction set, measured on one GPU: the q = 3 LMC of
K = 50 subsets of n_s = 2,000 (exponential), the 7-subset block one rank of an 8-GPU run holds (global
subset indices, so its chains are the node run's), the reference's sampler as written -- 100 x 50 amcmc
iterations, burn.in 3,750, 1,251 kept states (MK.R:57-59, 83, 85) -- and 131,072 held-out sites kriged
through the tiled replay in two tiles of 65,536 (MK.R:87-89).

Run it twice, back to back on one box: MK_KRIG_CHEB=0 (the exact replay: X = W P^T re-run for every
(subset, outcome) pair whose phi_h changed) and the default (the phi-interpolated replay of DESIGN.md
4.7 where the auto rule takes it).  The fit is deterministic (Philox streams keyed by the global subset
index), so both runs replay the same chain.  --save DIR keeps every tile's grids (S x 200 x q T, ~2 GB
per tile: give a scratch directory); --compare DIR reports the largest |difference| to them per tile and
removes them.  One JSON line on stdout, progress on stderr.

    MK_KRIG_CHEB=0 python tools/lmc_share.py --save /tmp/lmc_grids > exact.json
    python tools/lmc_share.py --compare /tmp/lmc_grids > default.json

The first tile's time holds the window's one-time work (the interpolated path's g = W' z of every kept
state); g_pass_s is the first tile's time less the mean of the others.
"""
import argparse
import importlib
import json
import os
import sys
import time

if int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0) < 8:
    os.environ["GPU_MAX_HW_QUEUES"] = "8"
import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--K", type=int, default=50)
    ap.add_argument("--q", type=int, default=3)
    ap.add_argument("--gpus", type=int, default=8, help="node size whose per-GPU share this is")
    ap.add_argument("--rank", type=int, default=-1, help="the share's rank (-1: the first of the largest blocks)")
    ap.add_argument("--n-test", type=int, default=131_072)
    ap.add_argument("--tile", type=int, default=65536)
    ap.add_argument("--n-batch", type=int, default=100)
    ap.add_argument("--batch-length", type=int, default=50)
    ap.add_argument("--save", default=None, metavar="DIR", help="keep every tile's grids there (tile_<i>.npy)")
    ap.add_argument("--compare", default=None, metavar="DIR", help="compare every tile's grids with those, then remove them")
    a = ap.parse_args()
    mk = importlib.import_module(PKG)
    dmod = importlib.import_module(PKG + ".distributed")
    q = a.q
    t = {}
    t0 = time.perf_counter()
    d = mk.synthetic.generate(a.n, q=q, n_test=a.n_test, seed=20250114)
    t["generate_s"] = time.perf_counter() - t0
    t1 = time.perf_counter()
    _, idx = mk.partition(a.n, a.K, seed=20250114, method="R")                   # MK.R:15-41
    beta0, bt = mk.start_values(d["y"], d["x"], 1.0, q)                         # MK.R:53-55
    blocks = [dmod.shard_range(a.K, a.gpus, r) for r in range(a.gpus)]
    rank = a.rank if a.rank >= 0 else max(range(a.gpus), key=lambda r: (blocks[r][1] - blocks[r][0], -r))
    lo, hi = blocks[rank]
    subs = [mk.subset_data(d["y"], d["x"], 1.0, d["coords"], q, idx[i]) for i in range(lo, hi)]
    cfg = mk.SamplerConfig(q, d["x"].shape[1], beta0, bt, n_batch=a.n_batch, batch_length=a.batch_length,
                           seed=20250114, predict_tile=a.tile)
    t["setup_s"] = time.perf_counter() - t1
    for dname in (a.save, a.compare):
        if dname:
            os.makedirs(dname, exist_ok=True)
    per_tile = []
    with mk.Session(subs, cfg, coords_test=d["coords_test"], subset_base=lo) as ses:
        tile = ses.predict_tile                      # the tile in use (HBM may shrink the request)
        ntiles = (a.n_test + tile - 1) // tile
        t2 = time.perf_counter()
        for b in range(cfg.n_batch):                                               # MK.R:80-84
            ses.run(cfg.batch_length)
            if (b + 1) % 20 == 0:
                print(f"lmc share: batch {b + 1}/{cfg.n_batch}, {time.perf_counter() - t2:.1f}s", file=sys.stderr,
                      flush=True)
        t["chains_s"] = time.perf_counter() - t2
        out = ses.outputs(quantiles=False, samples=True)
        # phi_h of the kept window: the last q reported columns
        changes = [int(np.count_nonzero(np.diff(smp[cfg.burn_in - 1:, -q + h]))) for smp in out["samples"]
                   for h in range(q)]
        for ti in range(ntiles):
            t4 = time.perf_counter()
            g = ses.tile_grids(ti * tile)            # (S, 200, q Tc): the replay of the kept states, MK.R:87-89
            t5 = time.perf_counter()
            rec = {"tile": ti, "sites": int(g.shape[2]) // q, "replay_grids_s": t5 - t4,
                   "finite": bool(np.isfinite(g).all())}
            if a.save:
                np.save(os.path.join(a.save, f"tile_{ti}.npy"), g)
            if a.compare:
                path = os.path.join(a.compare, f"tile_{ti}.npy")
                rec["max_abs_diff_to_saved"] = float(np.max(np.abs(g - np.load(path))))
                os.remove(path)
            per_tile.append(rec)
            print(f"lmc share: tile {ti} replay+grids {t5 - t4:.1f}s", file=sys.stderr, flush=True)
            del g
        cheb = ses.kernel_stats(mk.session.KS_KRIG_CHEB)          # tiles kriged by phi interpolation
        fallback = ses.kernel_stats(mk.session.KS_KRIG_FALLBACK)  # tiles whose check sent them to the exact replay
    t["tiles_replay_grids_s"] = sum(p["replay_grids_s"] for p in per_tile)
    t["process_s"] = time.perf_counter() - t0
    pairs = len(subs) * q
    rest = [p["replay_grids_s"] for p in per_tile[1:]]
    rec = {"workload": f"configs[3] per-GPU share: rank {rank} of {a.gpus} (subsets {lo}..{hi - 1}, {hi - lo} of K={a.K}, "
                       f"n_s={len(subs[0]['coords'])}), q={q}, n={a.n}, {a.n_test} test sites in tiles of {tile}, "
                       f"{cfg.n_batch} x {cfg.batch_length} amcmc iterations, burn.in {cfg.burn_in}, {cfg.kept} kept states",
           "krig_mode": os.environ.get("MK_KRIG_CHEB", "1"), "phases_s": t, "per_tile": per_tile, "pairs": pairs,
           "phi_changes_per_pair": changes,
           "interpolated_tiles": cheb["launches"], "fallback_tiles": fallback["launches"],
           "exact_evaluations_per_pair_and_tile": (cheb["flops"] / (cheb["launches"] * pairs)) if cheb["launches"] else None,
           "x_refreshes_per_pair_and_tile_exact": (sum(changes) + pairs) / pairs,
           "max_check_difference": cheb["ms"] if cheb["launches"] else None,
           "g_pass_s": (per_tile[0]["replay_grids_s"] - sum(rest) / len(rest)) if rest else None}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
