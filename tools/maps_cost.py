"""What the posterior maps cost at configs[2] geometry (250 subsets x 2,000 sites, q = 1, 1,000 test
sites, 1,251 kept states, J = 3 thresholds): a fused session runs the chain, maps are asked for and
mk_session_maps is called --calls times; kernel-stats kind 17 (the map launches, always timed) gives each
call's milliseconds, set beside the algorithmic traffic (8 n C bytes per subset read, 8 (4 + J) C written)
as a share of the HBM peak.  Beside them, in the same process and on the same draws, validation data are
attached and mk_session_scores is called as often: kind 16's milliseconds, the figure the maps' is read
against (the two kernels read the same bytes).  The maps run after the fit and add no launch to the chain,
so the chain's step time is not touched.  One JSON document on stdout and, with --out, in that file.

  python tools/maps_cost.py [--subsets 250] [--n 500000] [--kept 1251] [--out profiles/maps/cost.json]
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"
HBM_PEAK = 8.0e12      # bytes / s (MI355X)
THRESHOLDS = (0.2, 0.5, 0.8)


def timed_calls(ses, kind, call, n):
    """n calls, each with its own launches and milliseconds of the kernel-stats kind."""
    calls, before, last = [], ses.kernel_stats(kind), None
    for _ in range(n):
        last = call()
        now = ses.kernel_stats(kind)
        calls.append({"launches": now["launches"] - before["launches"], "ms": now["ms"] - before["ms"]})
        before = now
    return calls, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subsets", type=int, default=250)
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--n-test", type=int, default=1000)
    ap.add_argument("--kept", type=int, default=1251)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mk = importlib.import_module(PKG)
    K, J = a.subsets, len(THRESHOLDS)
    d = mk.synthetic.generate(a.n, q=1, n_test=a.n_test, seed=20250114)
    _, idx = mk.partition(a.n, K, seed=20250114)
    beta0, bt = mk.start_values(d["y"], d["x"], 1.0, 1, device=0)
    total = a.warmup + a.kept - 1                    # burn_in = warmup: every later iteration is a kept one
    assert total % 50 == 0, "warmup + kept - 1 must be a multiple of 50"
    cfg = mk.SamplerConfig(1, 2, beta0, bt, n_batch=total // 50, batch_length=50, burn_in=a.warmup, seed=20250114)
    subs = [mk.subset_data(d["y"], d["x"], 1.0, d["coords"], 1, idx[i]) for i in range(K)]
    with mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
        ses.run(total)
        off = ses.kernel_stats(mk.session.KS_MAPS)
        ses.set_maps(THRESHOLDS)
        ses.set_validation(d["y_test"])
        # alternating would change nothing (each call is one kernel on an idle device); maps first, then scores
        maps_calls, m = timed_calls(ses, mk.session.KS_MAPS, ses.maps, a.calls)
        score_calls, sc = timed_calls(ses, mk.session.KS_SCORE, lambda: ses.scores(pointwise=True), a.calls)
        same = bool((m["subsets"][0][:, 2] == sc["pointwise"][0][:, 0]).all())
        schedule = "lookahead" if ses.lookahead else "sequential"
    C = a.n_test
    bytes_maps = K * (8 * a.kept * C + 8 * (4 + J) * C)
    bytes_scores = K * (8 * a.kept * C + 16 * C)
    best, best_sc = min(c["ms"] for c in maps_calls), min(c["ms"] for c in score_calls)
    rec = {"geometry": {"subsets": K, "sites_per_subset": a.n // K, "q": 1, "n_test": a.n_test, "kept_states": a.kept,
                        "thresholds": list(THRESHOLDS)},
           "schedule": schedule,
           "kind17": {"calls": maps_calls, "best_ms": best, "algorithmic_bytes_per_call": bytes_maps,
                      "GB_per_s": bytes_maps / (best * 1e-3) / 1e9, "share_of_hbm_peak": bytes_maps / (best * 1e-3) / HBM_PEAK,
                      "hbm_peak_bytes_per_s": HBM_PEAK},
           "kind17_before_attaching": off,
           "kind16_same_run": {"calls": score_calls, "best_ms": best_sc, "algorithmic_bytes_per_call": bytes_scores,
                               "note": "mk_session_scores on the same draws: k_score_cols + k_score_finish"},
           "maps_over_scores": best / best_sc,
           "p_mean_equals_scores_pmean_first_subset": same,
           "planes_first_subset_first_column": dict(zip(m["names"], m["subsets"][0][0].tolist()))}
    text = json.dumps(rec, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
