"""What switching the in-chain model assessment on costs at configs[2] geometry (250 subsets x 2,000
sites, q = 1, 1,000 test sites): two sessions on the same data, criteria on and off, run in
interleaved windows of kept iterations (on, off, on, off, ...), each window timed by the host clock
around mk_session_run (which returns after the device is idle); then kernel-stats kind 15 (the
criteria launches, always timed) per launch beside kind 5 (whole iterations) of the session that
made them.  One JSON document on stdout and, with --out, in that file.

  python tools/criteria_cost.py [--subsets 250] [--n 500000] [--windows 4] [--steps 20] [--out FILE]
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
    ap.add_argument("--subsets", type=int, default=250)
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--n-test", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mk = importlib.import_module(PKG)
    K = a.subsets
    d = mk.synthetic.generate(a.n, q=1, n_test=a.n_test, seed=20250114)
    _, idx = mk.partition(a.n, K, seed=20250114)
    beta0, bt = mk.start_values(d["y"], d["x"], 1.0, 1, device=0)
    post = a.steps                                   # a last window of the `on` session with kind 5 bracketed
    total = a.warmup + a.windows * a.steps + post
    cfg = mk.SamplerConfig(1, 2, beta0, bt, n_batch=(total + 49) // 50, batch_length=50, burn_in=a.warmup + 1,
                           seed=20250114)            # every timed iteration is a kept one (kriging + criteria)
    subs = [mk.subset_data(d["y"], d["x"], 1.0, d["coords"], 1, idx[i]) for i in range(K)]
    ses = {key: mk.Session(subs, cfg, coords_test=d["coords_test"], criteria=(key == "on")) for key in ("on", "off")}
    try:
        for s in ses.values():
            s.run(a.warmup)
        win = {"on": [], "off": []}
        for _ in range(a.windows):
            for key in ("on", "off"):
                t0 = time.perf_counter()
                ses[key].run(a.steps)
                win[key].append((time.perf_counter() - t0) / a.steps * 1e3)
        ses["on"].profile(True, kinds=[mk.session.KS_ITER])
        ses["on"].run(post)
        crit = ses["on"].kernel_stats(mk.session.KS_CRIT)
        it = ses["on"].kernel_stats(mk.session.KS_ITER)
        off = ses["off"].kernel_stats(mk.session.KS_CRIT)
        schedule = "lookahead" if ses["on"].lookahead else "sequential"
    finally:
        for s in ses.values():
            s.close()
    n_s = a.n // K
    n_pad = (n_s + 1 + 127) // 128 * 128
    # bytes one k_crit_accum launch moves: X (p columns), y, wt, w read, six running values read and written
    bytes_launch = K * n_s * 8 * (2 + 3 + 2 * 6)
    mean = {k: sum(v) / len(v) for k, v in win.items()}
    rec = {"geometry": {"subsets": K, "sites_per_subset": n_s, "n_pad": n_pad, "q": 1, "n_test": a.n_test},
           "schedule": schedule,
           "interleaved_windows_ms_per_step": win, "mean_ms_per_step": mean,
           "on_over_off": mean["on"] / mean["off"],
           "window": f"{a.windows} windows of {a.steps} kept iterations per session after {a.warmup} warmup iterations, "
                     "alternating on, off",
           "kind15": {"launches": crit["launches"], "ms": crit["ms"],
                      "us_per_launch": crit["ms"] / max(crit["launches"], 1) * 1e3,
                      "bytes_per_launch": bytes_launch,
                      "GB_per_s": bytes_launch / (crit["ms"] / max(crit["launches"], 1) * 1e-3) / 1e9 if crit["ms"] else None},
           "kind5_ms_per_iteration": it["ms"] / max(it["launches"], 1),
           "kind15_off_session": off}
    text = json.dumps(rec, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
