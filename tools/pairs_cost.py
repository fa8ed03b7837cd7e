"""What the cross-outcome outputs cost at configs[3]'s per-GPU share (7 subsets x 2,000 sites, q = 3, so
three outcome pairs; 1,000 test sites, 1,251 kept states, J = 3 thresholds): a fused session runs the
chain, then on the same draws, --calls times each:

  k_quantiles_pair   mk_session_pairs asking for the grids alone   kernel-stats kind 18 (always timed)
  k_pair_cols        mk_session_pairs asking for the planes alone  kind 18
  k_map_cols         mk_session_maps                               kind 17
  k_quantiles_prob   mk_session_grids(which = 2) into HBM          wall clock of the call (it returns after the
                     stream is idle and copies nothing to the host; no kernel-stats kind covers the quantile kernels)

and sets each new kernel beside the per-column kernel it is modelled on.  Work per functional is n_pairs 2 / q
of the per-column kernel's (two draw columns per pair column): at q = 3 the pair sort, which makes two
functionals, is expected near 2 x k_quantiles_prob, and k_pair_cols near 2 x k_map_cols' reads.  Before
anything is attached, kind 18 must show no launch (after the fit and after an outputs() call).  One JSON
document on stdout and, with --out, in that file.

  python tools/pairs_cost.py [--subsets 7] [--n 14000] [--kept 1251] [--out profiles/pairs/cost.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"
THRESHOLDS = (0.2, 0.5, 0.8)


def timed_calls(ses, kind, call, n):
    """n calls, each with its own launches and milliseconds of the kernel-stats kind."""
    calls, before = [], ses.kernel_stats(kind)
    for _ in range(n):
        call()
        now = ses.kernel_stats(kind)
        calls.append({"launches": now["launches"] - before["launches"], "ms": now["ms"] - before["ms"]})
        before = now
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subsets", type=int, default=7)
    ap.add_argument("--n", type=int, default=14_000)
    ap.add_argument("--q", type=int, default=3)
    ap.add_argument("--n-test", type=int, default=1000)
    ap.add_argument("--kept", type=int, default=1251)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mk = importlib.import_module(PKG)
    K, q, J = a.subsets, a.q, len(THRESHOLDS)
    d = mk.synthetic.generate(a.n, q=q, n_test=a.n_test, seed=20250114)
    _, idx = mk.partition(a.n, K, seed=20250114)
    beta0, bt = mk.start_values(d["y"], d["x"], 1.0, q, device=0)
    total = a.warmup + a.kept - 1                    # burn_in = warmup: every later iteration is a kept one
    assert total % 50 == 0, "warmup + kept - 1 must be a multiple of 50"
    cfg = mk.SamplerConfig(q, d["x"].shape[1], beta0, bt, n_batch=total // 50, batch_length=50, burn_in=a.warmup,
                           seed=20250114)
    subs = [mk.subset_data(d["y"], d["x"], 1.0, d["coords"], q, idx[i]) for i in range(K)]
    C, n_pairs = q * a.n_test, q * (q - 1) // 2
    C2 = n_pairs * a.n_test
    hip = ctypes.CDLL("libamdhip64.so")
    with mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(total)
        ses.outputs()
        off = ses.kernel_stats(mk.session.KS_PAIRS)
        ses.set_pairs(THRESHOLDS)
        ses.set_maps(THRESHOLDS)
        pair_sort = timed_calls(ses, mk.session.KS_PAIRS, lambda: ses.pairs(planes=False), a.calls)
        pair_cols = timed_calls(ses, mk.session.KS_PAIRS, lambda: ses.pairs(grids=False), a.calls)
        map_cols = timed_calls(ses, mk.session.KS_MAPS, ses.maps, a.calls)
        dptr = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(dptr), ctypes.c_size_t(K * C * 200 * 8)) == 0
        prob_sort = []
        for _ in range(a.calls + 1):                 # the first call also sets the kernel's LDS attribute
            t0 = time.perf_counter()
            ses.grids_device(2, dptr.value)
            prob_sort.append({"wall_ms": (time.perf_counter() - t0) * 1e3})
        hip.hipFree(dptr)
        planes = ses.pairs(grids=False)
    best = {k: min(c["ms"] for c in v) for k, v in (("k_quantiles_pair", pair_sort), ("k_pair_cols", pair_cols),
                                                    ("k_map_cols", map_cols))}
    best["k_quantiles_prob_wall"] = min(c["wall_ms"] for c in prob_sort[1:])
    rec = {"geometry": {"subsets": K, "sites_per_subset": a.n // K, "q": q, "pairs": n_pairs, "n_test": a.n_test,
                        "kept_states": a.kept, "columns": C, "pair_columns": C2, "thresholds": list(THRESHOLDS)},
           "kind18_before_attaching": off,
           "k_quantiles_pair": {"calls": pair_sort, "workgroups": K * C2, "functionals": 2},
           "k_pair_cols": {"calls": pair_cols, "algorithmic_bytes_read": K * 8 * a.kept * C,
                           "draw_bytes_requested": K * 16 * a.kept * C2},
           "k_map_cols": {"calls": map_cols, "algorithmic_bytes_read": K * 8 * a.kept * C},
           "k_quantiles_prob": {"calls": prob_sort, "workgroups": K * C,
                                "note": "wall clock of mk_session_grids(which = 2) into HBM; the first call is left out"},
           "best_ms": best,
           "pair_sort_over_prob_sort": best["k_quantiles_pair"] / best["k_quantiles_prob_wall"],
           "pair_cols_over_map_cols": best["k_pair_cols"] / best["k_map_cols"],
           "expected_ratio_per_functional": n_pairs * 2 / q,
           "planes_first_subset_first_pair_column": dict(zip(planes["names"], planes["subsets"][0][0].tolist()))}
    text = json.dumps(rec, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
