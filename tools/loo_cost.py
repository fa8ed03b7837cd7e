"""What PSIS-LOO costs at configs[2]'s 32-subset share (32 subsets x 2,000 sites, q = 1, 1,251 kept states): a
session without test sites runs the chain with w recorded, then mk_session_loo is called --calls times;
kernel-stats kind 20 (the PSIS-LOO launches, always timed) gives each call's device milliseconds.  Beside it,
kind 15 of mk_session_criteria over the same window: with no in-chain sums that call replays the recorded
chain (k_crit_replay, then two closing launches of a few microseconds), the elementwise floor of reading the
same chain -- what the selection and the fit cost on top is the difference.  One JSON document on stdout and,
with --out, in that file.

  python tools/loo_cost.py [--subsets 32] [--sites 2000] [--kept 1251] [--calls 3] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subsets", type=int, default=32)
    ap.add_argument("--sites", type=int, default=2000)
    ap.add_argument("--kept", type=int, default=1251)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mk = importlib.import_module(PKG)
    K, n = a.subsets, a.subsets * a.sites
    d = mk.synthetic.generate(n, q=1, n_test=8, seed=20250114)
    _, idx = mk.partition(n, K, seed=20250114)
    beta0, bt = mk.start_values(d["y"], d["x"], 1.0, 1, device=0)
    total = a.warmup + a.kept - 1                    # burn_in = warmup: every later iteration is a kept one
    assert total % 50 == 0, "warmup + kept - 1 must be a multiple of 50"
    cfg = mk.SamplerConfig(1, 2, beta0, bt, n_batch=total // 50, batch_length=50, burn_in=a.warmup, seed=20250114)
    subs = [mk.subset_data(d["y"], d["x"], 1.0, d["coords"], 1, idx[i]) for i in range(K)]
    with mk.Session(subs, cfg, record_w=True) as ses:
        t0 = time.perf_counter()
        ses.run(total)
        chain_s = time.perf_counter() - t0
        off = ses.kernel_stats(mk.session.KS_LOO)
        loo_calls, before = [], off
        for _ in range(a.calls):
            t0 = time.perf_counter()
            res = ses.loo()
            host_ms = (time.perf_counter() - t0) * 1e3
            now = ses.kernel_stats(mk.session.KS_LOO)
            loo_calls.append({"launches": now["launches"] - before["launches"], "ms": now["ms"] - before["ms"],
                              "host_ms": host_ms})
            before = now
        crit_calls, before = [], ses.kernel_stats(mk.session.KS_CRIT)
        for _ in range(a.calls):
            crit = ses.criteria()
            now = ses.kernel_stats(mk.session.KS_CRIT)
            crit_calls.append({"launches": now["launches"] - before["launches"], "ms": now["ms"] - before["ms"]})
            before = now
    best, floor = min(c["ms"] for c in loo_calls), min(c["ms"] for c in crit_calls)
    obs = K * a.sites
    rec = {"geometry": {"subsets": K, "sites_per_subset": a.sites, "q": 1, "states": a.kept, "observations": obs},
           "chain_s": chain_s,
           "kind20_before_the_first_call": off,
           "kind20": {"calls": loo_calls, "best_ms": best, "us_per_observation": best * 1e3 / obs,
                      "terms_scratch_bytes": obs // a.sites * ((a.sites + 1 + 127) // 128 * 128) * a.kept * 8},
           "kind15_replay_same_window": {"calls": crit_calls, "best_ms": floor},
           "loo_over_replay": best / floor if floor else None,
           "total_row": dict(zip(res["names"], res["total"].tolist())),
           "lppd_criteria": float(crit["total"][4])}
    text = json.dumps(rec, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
