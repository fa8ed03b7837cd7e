"""The column-strip body of the fused column update's ragged row tile (gemm_tile_cs, mk_gemm.hpp;
MK_RAGGED, default 1) against the row-wave body it replaces there (MK_RAGGED=0) and against the
unfused kernels (MK_CHOL_FUSED=0): every valid element accumulates the same MFMA sequence, only the
wave that owns it changes, so factors, log-determinants, inverses and whole chains are equal bit for
bit.  The switch is read once per process, so each arm of each case runs in its own subprocess (the
arms of a case side by side).

A row tile is ragged when v < 8 of its 16-row blocks hold rows of the valid extent n + 1 (the
bordered row included); the strips take v <= 6.  Orders n + 1 = 256 + r put r valid rows into the
last of three row tiles: r = 1, 16, 17 (v = 1, 1, 2: a block's first row, its last, the next block's
first), 48 (v = 3), 81 (v = 6, the workload's residue: 2,001 = 15 * 128 + 81), 96 (v = 6, full blocks),
97 and 113 (v = 7 and 8: the row-wave body, with padding), 128 (the exact fill).  n = 520 has five tiles
(K up to 384, v = 1), n = 976 eight (residue 81 again, K up to 768)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

REL = 1e-10   # tests/test_gpu_diag_syrk.py's bar on the factor against LAPACK
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"

ARMS = {"ragged1": {"MK_RAGGED": "1"}, "ragged0": {"MK_RAGGED": "0"}, "unfused": {"MK_CHOL_FUSED": "0"}}

# seeded exponential-correlation matrices, as tests/test_gpu_diag_syrk.py takes them (built one matrix
# at a time: S n^2 distances, not S n^2 coordinate pairs).  The whole L, log-det and inverse are
# compared through their digests; the first four factors come back for LAPACK.
_CHOL_RUN = """
import hashlib, importlib, sys, numpy as np
sys.path.insert(0, {root!r})
mk = importlib.import_module({pkg!r})
rng = np.random.default_rng(11)
S, n = {S}, {n}
A = np.empty((S, n, n))
for s in range(S):
    c = rng.uniform(size=(n, 2))
    d = np.sqrt(((c[:, None, :] - c[None, :, :]) ** 2).sum(-1))
    A[s] = np.exp(-(3.0 + rng.uniform() * 6.0) * d)
L, ld, inv = mk.cholesky_batched(A, inverse=True)
dig = [hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest() for x in (L, ld, inv)]
np.savez({path!r}, A=A[:4], L=L[:4], ld=ld, inv=inv[:4], dig=np.array(dig))
"""

# More than 224 subsets: the sequential schedule, whose factorisations are the fused launches; sizes
# 260 .. 459 in steps of 7 mod 200, so n_pad = 512 (four row tiles) and the subsets are ragged among
# themselves: row tile 2 is full, ragged (every v) or the bordered row alone, row tile 3 ragged or all
# padding (v <= 0: the row-wave body, as before).
_CHAIN_RUN = """
import importlib, sys, numpy as np
sys.path.insert(0, {root!r})
mk = importlib.import_module({pkg!r})
S = 226
sizes = [260 + (7 * s) % 200 for s in range(S)]
d = mk.synthetic.generate(sum(sizes), q=1, n_test=24, seed=83)
cfg = mk.SamplerConfig(1, 2, np.zeros(2), np.full(2, 0.05), n_batch=2, batch_length=3, burn_in=4, seed=5)
subs, off = [], 0
for m in sizes:
    subs.append(dict(coords=d["coords"][off:off + m], y=d["y"][off:off + m], weights=np.ones(m), x=d["x"][off:off + m]))
    off += m
with mk.Session(subs, cfg, coords_test=d["coords_test"], record_w=True) as ses:
    assert not ses.lookahead
    ses.run(cfg.n_samples)
    o = ses.outputs(samples=True, w_samples=True)
out = {{}}
for s in range(S):
    out["samples_%d" % s] = o["samples"][s]
    out["w_%d" % s] = o["w_samples"][s]
np.savez({path!r}, **out)
"""


def _arms(tmp_path, tag, script, arms):
    """The arms of one case, each in its own process, side by side -> {arm: {name: array}}."""
    procs = {}
    for arm in arms:
        path = str(tmp_path / f"{tag}_{arm}.npz")
        env = {k: v for k, v in os.environ.items() if k not in ("MK_RAGGED", "MK_CHOL_FUSED")}
        env.update(ARMS[arm])
        procs[arm] = (path, subprocess.Popen([sys.executable, "-c", script.format(root=ROOT, pkg=PKG, path=path)],
                                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    res = {}
    for arm, (path, p) in procs.items():
        try:
            _, err = p.communicate(timeout=240)
        finally:
            if p.poll() is None:
                p.kill()
        assert p.returncode == 0, (arm, err[-4000:])
        z = np.load(path)
        res[arm] = {k: z[k] for k in z.files}
    return res


# S = 136: >= 128 factors, so every fused launch takes 128-tiles.
ORDERS = [256 + r for r in (1, 16, 17, 48, 81, 96, 97, 113, 128)]


@pytest.mark.parametrize("n", [o - 1 for o in ORDERS] + [520, 976],
                         ids=[f"r{o - 256}" for o in ORDERS] + ["n520", "n976"])
def test_factor_logdet_inverse_are_bit_identical(tmp_path, n):
    res = _arms(tmp_path, f"chol{n}", _CHOL_RUN.replace("{S}", "136").replace("{n}", str(n)), list(ARMS))
    a = res["ragged1"]
    for arm in ("ragged0", "unfused"):
        for j, name in enumerate(("L", "ld", "inv")):
            assert a["dig"][j] == res[arm]["dig"][j], (arm, name)
            assert np.array_equal(a[name], res[arm][name]), (arm, name)
    for s in range(4):
        Lr = sla.cholesky(a["A"][s], lower=True)
        assert np.linalg.norm(a["L"][s] - Lr) <= REL * np.linalg.norm(Lr)


def test_ragged_subsets_chain_is_bit_identical(tmp_path):
    """226 subsets of 260 .. 459 sites on the sequential schedule: samples and latent w."""
    res = _arms(tmp_path, "chain", _CHAIN_RUN, ["ragged1", "ragged0"])
    assert res["ragged1"].keys() == res["ragged0"].keys() and len(res["ragged1"]) == 2 * 226
    for k in res["ragged1"]:
        assert np.array_equal(res["ragged1"][k], res["ragged0"][k]), k
