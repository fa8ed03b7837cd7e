"""What the areal prediction costs at configs[3]'s per-GPU share (7 subsets x 2,000 sites, q = 3; 1,000 test
sites in 10 regions of 100, 1,251 kept states, J = 3 thresholds): a tiled session runs the chain, attaches the
test sites and the regions, and replays the kept window once (the exact replay: regions switch the
phi-interpolated one off).  From that one replay:

  k_region_cov    covariance and factor of every (dirty pair, region)   mk_regions.timing_ms[0]
  k_region_draw   the regional draws, one launch per kept state         timing_ms[1]
  grids, planes   k_quantiles and k_map_cols on the regional draws      timing_ms[2]
  k_pred_var      the kriging GEMM of the same replay                   kernel-stats kind 9 (profiler on for it)

Kind 19 holds the sum of the first three and must show no launch before the regions are attached.  One JSON
document on stdout and, with --out, in that file.

--interpolate: after that, the same session replays the window --repeats times on each route, interleaved
(exact, interpolated, exact, ..), each replay from a fresh attach so that timing_ms and the launches are that
replay's alone; "routes" then holds per route the wall clock, the three timing parts and kind 19's launches of
every repeat, and for the interpolated route the route that ran, its check, the node count E (the launches less
the check, two per chunk of kept states and the two summaries) and the largest |interpolated - exact| draw.

  python tools/regions_cost.py [--subsets 7] [--n 14000] [--kept 1251] [--interpolate] [--repeats 3]
                               [--out profiles/regions/cost.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"
THRESHOLDS = (0.2, 0.5, 0.8)


def both_routes(mk, ses, offsets, a):
    """--repeats replays per route on the session, interleaved; the profiler stays as main() left it."""
    ks = mk.session.KS_REGIONS
    sites = a.n_test // a.regions
    fsz = a.regions * sites * sites
    env_b = int(os.environ.get("MK_REGIONS_CHUNK") or 0)          # the library's chunk rule (include/mk.h)
    B = max(1, min(a.kept, env_b if env_b > 0 else (1 << 30) // (8 * a.subsets * a.q * fsz)))
    chunks = -(-a.kept // B)
    rec = {"exact": [], "interpolated": [], "chunk_states": B, "chunks": chunks}
    draws = {}
    for _ in range(a.repeats):
        for name, interp in (("exact", False), ("interpolated", True)):
            ses.set_regions(offsets, None, THRESHOLDS, interpolate=interp)
            before = ses.kernel_stats(ks)
            t0 = time.perf_counter()
            ses.outputs(quantiles=False, w_predict_sum=True)
            wall = time.perf_counter() - t0
            rg = ses.regions(samples=True)
            launches = ses.kernel_stats(ks)["launches"] - before["launches"]
            t = rg["timing_ms"].tolist()
            row = {"replay_wall_s": wall, "cov_and_factor_ms": t[0], "draws_ms": t[1], "grids_and_planes_ms": t[2],
                   "launches": launches, "route": rg["route"], "check": rg["check"],
                   "singular_states": int(sum(int(x.sum()) for x in rg["singular"]))}
            if rg["route"] == "interpolated":
                row["nodes_E"] = launches - (1 + 2 * chunks + 2)
            rec[name].append(row)
            draws[name] = rg["region_samples"]
    rec["max_abs_draw_difference"] = float(max(np.abs(x - y).max() for x, y in zip(draws["exact"], draws["interpolated"])))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subsets", type=int, default=7)
    ap.add_argument("--n", type=int, default=14_000)
    ap.add_argument("--q", type=int, default=3)
    ap.add_argument("--n-test", type=int, default=1000)
    ap.add_argument("--regions", type=int, default=10)
    ap.add_argument("--kept", type=int, default=1251)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--interpolate", action="store_true", help="time both routes on the one session")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mk = importlib.import_module(PKG)
    K, q = a.subsets, a.q
    assert a.n_test % a.regions == 0 and a.n_test // a.regions <= 128
    d = mk.synthetic.generate(a.n, q=q, n_test=a.n_test, seed=20250114)
    _, idx = mk.partition(a.n, K, seed=20250114)
    beta0, bt = mk.start_values(d["y"], d["x"], 1.0, q, device=0)
    total = a.warmup + a.kept - 1                    # burn_in = warmup: every later iteration is a kept one
    assert total % 50 == 0, "warmup + kept - 1 must be a multiple of 50"
    cfg = mk.SamplerConfig(q, d["x"].shape[1], beta0, bt, n_batch=total // 50, batch_length=50, burn_in=a.warmup,
                           seed=20250114, predict_tile=1024)
    subs = [mk.subset_data(d["y"], d["x"], 1.0, d["coords"], q, idx[i]) for i in range(K)]
    # districts: vertical strips of the unit square, the sites of a strip in the order they come
    order = np.argsort(d["coords_test"][:, 0], kind="stable")
    rows = (order[:, None] * q + np.arange(q)[None, :]).reshape(-1)
    offsets = np.arange(a.regions + 1) * (a.n_test // a.regions)
    with mk.Session(subs, cfg) as ses:
        t0 = time.perf_counter()
        ses.run(total)
        fit_s = time.perf_counter() - t0
        ses.set_test_sites(d["coords_test"][order], x_test=d["x_test"][rows])
        off = ses.kernel_stats(mk.session.KS_REGIONS)
        ses.set_regions(offsets, None, THRESHOLDS)
        ses.profile(True, kinds=[mk.session.KS_PRED_VAR])
        before = ses.kernel_stats(mk.session.KS_PRED_VAR)
        t0 = time.perf_counter()
        ses.outputs(quantiles=False, w_predict_sum=True)
        replay_s = time.perf_counter() - t0
        pv = ses.kernel_stats(mk.session.KS_PRED_VAR)
        rg = ses.regions()
        kind19 = ses.kernel_stats(mk.session.KS_REGIONS)
        routes = both_routes(mk, ses, offsets, a) if a.interpolate else None
    t = rg["timing_ms"].tolist()
    rec = {"geometry": {"subsets": K, "sites_per_subset": a.n // K, "q": q, "n_test": a.n_test, "regions": a.regions,
                        "sites_per_region": a.n_test // a.regions, "kept_states": a.kept, "thresholds": list(THRESHOLDS)},
           "kind19_before_attaching": off, "kind19": kind19,
           "fit_wall_s": fit_s, "replay_wall_s": replay_s,
           "ms_per_fit": {"k_region_cov": t[0], "k_region_draw": t[1], "grids_and_planes": t[2],
                          "k_pred_var": pv["ms"] - before["ms"]},
           "k_pred_var_launches": pv["launches"] - before["launches"],
           "cov_over_pred_var": t[0] / max(pv["ms"] - before["ms"], 1e-30),
           "singular_states": int(sum(int(x.sum()) for x in rg["singular"])),
           "first_subset_planes": {n: rg["subsets"][0][:, i].tolist() for i, n in enumerate(rg["names"])}}
    if routes is not None:
        rec["routes"] = routes
    text = json.dumps(rec, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
