"""What the held-out scores cost at configs[2] geometry (250 subsets x 2,000 sites, q = 1, 1,000 test
sites, 1,251 kept states): a fused session runs the chain, validation data are attached and
mk_session_scores is called --calls times; kernel-stats kind 16 (the scoring launches, always timed)
gives each call's milliseconds, set beside the algorithmic traffic (8 n C bytes per subset read, 16 C
written) as a share of the HBM peak.  Scoring runs after the fit, so the chain's step time is not
touched; --parent-lib confirms it against a build of the parent commit: a second session on the same
data through that library, the two run in interleaved windows of kept iterations (new, parent, new,
parent, ...), each window timed by the host clock around mk_session_run (which returns after the
device is idle).  One JSON document on stdout and, with --out, in that file.

  python tools/scores_cost.py [--subsets 250] [--n 500000] [--kept 1251] [--parent-lib libmk_parent.so] [--out FILE]
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
HBM_PEAK = 8.0e12      # bytes / s (MI355X)


def other_library_session(mk, path, *args, **kw):
    """A Session whose calls go to the libmk at `path` (a build without the newer entry points binds
    those it has)."""
    binding = importlib.import_module(PKG + "._lib")
    binding.load()
    lib = ctypes.CDLL(path)
    for name, (res, argtypes) in binding.EXPORTS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, argtypes
    lib.mk_set_hw_queues(binding.HW_QUEUES)
    mine, binding._LIB = binding._LIB, lib
    try:
        return mk.Session(*args, **kw)
    finally:
        binding._LIB = mine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--subsets", type=int, default=250)
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--n-test", type=int, default=1000)
    ap.add_argument("--kept", type=int, default=1251)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mk = importlib.import_module(PKG)
    K = a.subsets
    d = mk.synthetic.generate(a.n, q=1, n_test=a.n_test, seed=20250114)
    _, idx = mk.partition(a.n, K, seed=20250114)
    beta0, bt = mk.start_values(d["y"], d["x"], 1.0, 1, device=0)
    total = a.warmup + a.kept - 1                    # burn_in = warmup: every later iteration is a kept one
    assert total % 50 == 0 and a.windows * a.steps <= a.kept - 1, "warmup + kept - 1 must be a multiple of 50"
    cfg = mk.SamplerConfig(1, 2, beta0, bt, n_batch=total // 50, batch_length=50, burn_in=a.warmup, seed=20250114)
    subs = [mk.subset_data(d["y"], d["x"], 1.0, d["coords"], 1, idx[i]) for i in range(K)]
    kw = dict(coords_test=d["coords_test"], x_test=d["x_test"])
    ses = {"new": mk.Session(subs, cfg, **kw)}
    try:
        if a.parent_lib:
            ses["parent"] = other_library_session(mk, os.path.abspath(a.parent_lib), subs, cfg, **kw)
        for s in ses.values():
            s.run(a.warmup)
        win = {key: [] for key in ses}
        for _ in range(a.windows if a.parent_lib else 0):
            for key in ses:
                t0 = time.perf_counter()
                ses[key].run(a.steps)
                win[key].append((time.perf_counter() - t0) / a.steps * 1e3)
        if "parent" in ses:
            ses.pop("parent").close()
        new = ses["new"]
        new.run(total - new.iteration)
        off = new.kernel_stats(mk.session.KS_SCORE)
        new.set_validation(d["y_test"])
        calls, before = [], off
        for _ in range(a.calls):
            sc = new.scores()
            now = new.kernel_stats(mk.session.KS_SCORE)
            calls.append({"launches": now["launches"] - before["launches"], "ms": now["ms"] - before["ms"]})
            before = now
        schedule = "lookahead" if new.lookahead else "sequential"
    finally:
        for s in ses.values():
            s.close()
    C = a.n_test
    bytes_call = K * (8 * a.kept * C + 16 * C)
    best = min(c["ms"] for c in calls)
    rec = {"geometry": {"subsets": K, "sites_per_subset": a.n // K, "q": 1, "n_test": a.n_test, "kept_states": a.kept},
           "schedule": schedule,
           "kind16": {"calls": calls, "best_ms": best, "algorithmic_bytes_per_call": bytes_call,
                      "GB_per_s": bytes_call / (best * 1e-3) / 1e9, "share_of_hbm_peak": bytes_call / (best * 1e-3) / HBM_PEAK,
                      "hbm_peak_bytes_per_s": HBM_PEAK},
           "kind16_before_attaching": off,
           "rows_first_subset": dict(zip(sc["names"], sc["subsets"][0].tolist()))}
    if a.parent_lib:
        mean = {k: sum(v) / len(v) for k, v in win.items()}
        rec["step_time"] = {"interleaved_windows_ms_per_step": win, "mean_ms_per_step": mean,
                            "new_over_parent": mean["new"] / mean["parent"],
                            "window": f"{a.windows} windows of {a.steps} kept iterations per session after {a.warmup} "
                                      "warmup iterations, alternating this build and the parent commit's, no "
                                      "validation data attached"}
    text = json.dumps(rec, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
