"""What a checkpoint and a restore cost (mk_session_checkpoint / mk_session_restore) at the
32-subset share of configs[2]: 32 subsets x 2,000 sites, q = 1, fused kriging at 256 test sites, 100 x 50
iterations.  Session A runs to the cut (half the chain by default) and writes the file; session B is made from the
file.  Reported:

  digest    k_state_digest over the three factor buffers a site-sweep session holds (L, Winv, W): the bytes of the
            regions (each read once) over the device time of one Session.digest() call, against the HBM peak
  restore   the device time of the re-derivation (candidates, Cholesky, inverse, kriging refresh), of the digests and
            the host time of the uploads, beside one sampler iteration of the same session (KS_ITER)
  file      the size of the file at iterations 0, half and all of the chain, with and without record_w: the one
            written here on disk, the others from the layout (the file is uncompressed: the arrays' bytes and a
            few hundred bytes of headers per key)
  windows   subset-iterations per second of 40-step windows on B (resumed) and on A (never stopped), interleaved

One JSON document on stdout and, with --out, in that file.

  python tools/checkpoint_cost.py [--n-batch 100] [--cut 2500] [--out profiles/checkpoint/cost.json]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"
HBM_PEAK = 8.0e12          # bytes per second
K, N, Q, N_TEST, STEP = 32, 64_000, 1, 256, 40


def region_bytes(n_part):
    """Bytes k_state_digest reads of L, Winv and W (their regions below n_s; include/mk.h "checkpoints")."""
    total = 0
    for ns in n_part:
        tri = ns * (ns + 1) // 2
        tiles = sum(m * (m + 1) // 2 for m in (min(128, ns - 128 * k) for k in range(-(-ns // 128))))
        total += 8 * (2 * tri + tiles)
    return total


def file_bytes(mk, cfg, n_part, iteration, record_w, data_bytes):
    n_pad = (max(n_part) + 1 + 127) // 128 * 128
    words = mk.fitfile.checkpoint_words(cfg, n_pad, iteration, N_TEST, record_w, False)
    return int(8 * len(n_part) * (int(words.sum()) + 4 * cfg.q) + data_bytes)


def window(ses):
    t0 = time.perf_counter()
    ses.run(STEP)
    return K * STEP / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-batch", type=int, default=100)
    ap.add_argument("--cut", type=int, default=None)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mk = importlib.import_module(PKG)
    d = mk.synthetic.generate(N, q=Q, n_test=N_TEST, seed=20250114)
    _, idx = mk.partition(N, K, seed=20250114)
    beta0, bt = mk.start_values(d["y"], d["x"], 1.0, Q, device=0)
    cfg = mk.SamplerConfig(Q, d["x"].shape[1], beta0, bt, n_batch=a.n_batch, batch_length=50, seed=20250114)
    cut = cfg.n_samples // 2 if a.cut is None else a.cut
    assert 0 < cut <= cfg.n_samples - a.windows * STEP, "the windows run after the cut"
    subs = [mk.subset_data(d["y"], d["x"], 1.0, d["coords"], Q, idx[i]) for i in range(K)]
    n_part = [s["coords"].shape[0] for s in subs]
    rec = {"geometry": {"subsets": K, "sites_per_subset": N // K, "q": Q, "n_test": N_TEST, "iterations": cfg.n_samples,
                        "cut": cut}}
    with tempfile.TemporaryDirectory() as tmp, \
            mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as A:
        A.profile(True, kinds=[mk.session.KS_ITER])
        t0 = time.perf_counter()
        A.run(cut)
        rec["run_to_cut_s"] = time.perf_counter() - t0
        it = A.kernel_stats(mk.session.KS_ITER)
        iter_ms = it["ms"] / it["launches"]
        # 1. the digest kernel
        A.digest()                                     # warm-up: the kernels' first launch
        k0 = A.kernel_stats(mk.session.KS_CKPT)
        A.digest()
        k1 = A.kernel_stats(mk.session.KS_CKPT)
        ms, nb = k1["ms"] - k0["ms"], region_bytes(n_part)
        rec["digest"] = {"bytes_read": nb, "ms": ms, "launches": k1["launches"] - k0["launches"],
                         "bytes_per_s": nb / (ms * 1e-3), "share_of_hbm_peak": nb / (ms * 1e-3) / HBM_PEAK}
        # 3. the file
        path = os.path.join(tmp, "shard0.npz")
        t0 = time.perf_counter()
        mk.fitfile.save_checkpoint(A, path)
        save_s = time.perf_counter() - t0
        on_disk = os.path.getsize(path)
        arrays = mk.fitfile.read_checkpoint(path)
        data_bytes = sum(v.nbytes for k, v in arrays.items() if not k.startswith("state_") and k != "digests")
        rec["file"] = {"written_at_cut_bytes": on_disk, "save_s": save_s, "layout_at_cut_bytes":
                       file_bytes(mk, cfg, n_part, cut, False, data_bytes),
                       "bytes": {f"iteration_{i}": {"plain": file_bytes(mk, cfg, n_part, i, False, data_bytes),
                                                    "record_w": file_bytes(mk, cfg, n_part, i, True, data_bytes)}
                                 for i in (0, cfg.n_samples // 2, cfg.n_samples)}}
        # 2. the restore
        t0 = time.perf_counter()
        B = mk.fitfile.load_checkpoint(path)
        load_s = time.perf_counter() - t0
        with B:
            rs = B.restore_stats()
            rec["restore"] = dict(rs, load_checkpoint_s=load_s, iteration_ms=iter_ms,
                                  derive_over_iteration=rs["ms_derive"] / iter_ms,
                                  device_total_over_iteration=(rs["ms_derive"] + rs["ms_digest"]) / iter_ms)
            # 4. the windows, interleaved (README's A/B rule)
            wa, wb = [], []
            for _ in range(a.windows):
                wb.append(window(B))
                wa.append(window(A))
            rec["windows_subset_iters_per_s"] = {"resumed": wb, "never_stopped": wa, "resumed_over_never_stopped":
                                                 float(np.median(wb) / np.median(wa))}
            rec["equal_after_windows"] = bool(A.digest().tobytes() == B.digest().tobytes() and all(
                A.chain_state(i)[k].tobytes() == B.chain_state(i)[k].tobytes() for i in range(K) for k in ("beta", "theta", "w")))
    text = json.dumps(rec, indent=1)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
