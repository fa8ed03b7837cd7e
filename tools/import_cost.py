"""What importing a recorded chain costs (mk_session_import_chain) beside the g pass of the phi-interpolated replay,
which makes the same factorisations over the same window, at two per-GPU shares with 1,251 kept states:

  cfg4   configs[3]'s share   7 subsets x 2,000 sites, q = 3
  cfg3   configs[2]'s share  32 subsets x 2,000 sites, q = 1

Per share: session A runs the chain (tiled, record_w) and hands samples and w_samples to the host; session B is
created anew and imports them.  Reported per share:

  import      mk_session_import_stats: factorisations, ms of the factor refreshes, ms of the k_import_z launches
              (device events), and the wall clock of the whole call (host transposes and uploads included)
  k_import_z  the bytes of W its launches read, counted from the chain's phi runs (per pair, per chunk of 32 states
              and per run inside it, ceil(states / B) passes over the 128-column tiles up to the diagonal), over
              its ms: bytes per second, and that over the HBM peak
  g pass      on session B, MK_KRIG_CHEB=-1: a tile replay that makes G (the g pass, then the nodes and draws) less
              the same replay again (G kept: nodes and draws alone), after a warm-up replay of a shorter window
  ratio       (import's factor ms + z ms) / g pass

One JSON document on stdout and, with --out, in that file.

  python tools/import_cost.py [--shares cfg4,cfg3] [--kept 1251] [--out profiles/import/cost.json]
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
SHARES = {"cfg4": dict(subsets=7, n=14_000, q=3), "cfg3": dict(subsets=32, n=64_000, q=1)}
HBM_PEAK = 8.0e12          # bytes per second
CHUNK, BATCH, NB = 32, 8, 128


def z_bytes(phi, n_part, q, batch):
    """Bytes of W that k_import_z reads for a chain whose kept phi is phi[subset] (kept x q)."""
    total = 0
    for i, ns in enumerate(n_part):
        tiles = -(-int(ns) // NB)
        tri = sum((t + 1) * NB * NB * 8 for t in range(tiles))
        for h in range(q):
            v = phi[i][:, h]
            for c0 in range(0, v.size, CHUNK):
                w = v[c0:c0 + CHUNK]
                cuts = np.flatnonzero(np.diff(w) != 0.0) + 1
                for run in np.diff(np.concatenate([[0], cuts, [w.size]])):
                    total += -(-int(run) // batch) * tri
    return total


def share(mk, name, kept, warmup):
    g = SHARES[name]
    K, q = g["subsets"], g["q"]
    d = mk.synthetic.generate(g["n"], q=q, n_test=256, seed=20250114)
    _, idx = mk.partition(g["n"], K, seed=20250114)
    beta0, bt = mk.start_values(d["y"], d["x"], 1.0, q, device=0)
    total = warmup + kept - 1
    assert total % 50 == 0, "warmup + kept - 1 must be a multiple of 50"
    cfg = mk.SamplerConfig(q, d["x"].shape[1], beta0, bt, n_batch=total // 50, batch_length=50, burn_in=warmup,
                           seed=20250114, predict_tile=1024)
    subs = [mk.subset_data(d["y"], d["x"], 1.0, d["coords"], q, idx[i]) for i in range(K)]
    os.environ["MK_KRIG_CHEB"] = "-1"
    with mk.Session(subs, cfg, record_w=True) as ses:
        t0 = time.perf_counter()
        ses.run(total)
        fit_s = time.perf_counter() - t0
        out = ses.outputs(quantiles=False, samples=True, w_samples=True)
    ntri = q * (q + 1) // 2
    phi = [s[warmup - 1:, cfg.p + ntri:cfg.p + ntri + q] for s in out["samples"]]
    with mk.Session(subs, cfg, record_w=True) as ses:
        t0 = time.perf_counter()
        ses.import_chain(out["samples"], out["w_samples"])
        import_s = time.perf_counter() - t0
        st = ses.import_stats()
        ses.set_test_sites(d["coords_test"])

        def replay():
            t0 = time.perf_counter()
            ses.tile_grids(0)
            return time.perf_counter() - t0

        ses.set_kept_window(warmup + kept // 2, total)   # warm-up: another window's G
        warm = replay()
        ses.set_kept_window(warmup, total)
        with_g, without_g = replay(), replay()
        cheb = ses.kernel_stats(mk.session.KS_KRIG_CHEB)
        fb = ses.kernel_stats(mk.session.KS_KRIG_FALLBACK)
    zb = z_bytes(phi, [s["coords"].shape[0] for s in subs], q, BATCH)
    g_ms = 1e3 * (with_g - without_g)
    rate = zb / (st["ms_z"] * 1e-3)
    return {"geometry": {"subsets": K, "sites_per_subset": g["n"] // K, "q": q, "kept_states": kept, "iterations": total},
            "fit_wall_s": fit_s, "import_wall_s": import_s, "import": st,
            "k_import_z": {"W_bytes_read": zb, "bytes_per_s": rate, "share_of_hbm_peak": rate / HBM_PEAK, "batch": BATCH,
                           "chunk_states": CHUNK},
            "g_pass": {"replay_with_g_s": with_g, "replay_without_g_s": without_g, "g_pass_ms": g_ms, "warm_up_replay_s": warm,
                       "interpolated_tiles": cheb["launches"], "fallback_tiles": fb["launches"]},
            "import_over_g_pass": (st["ms_factor"] + st["ms_z"]) / g_ms,
            "z_over_factor": st["ms_z"] / st["ms_factor"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shares", default="cfg4,cfg3")
    ap.add_argument("--kept", type=int, default=1251)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mk = importlib.import_module(PKG)
    rec = {name: share(mk, name, a.kept, a.warmup) for name in a.shares.split(",")}
    text = json.dumps(rec, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
