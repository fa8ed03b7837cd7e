"""The balanced SYRK body of the Cholesky's diagonal-tile updates (gemm_syrk_128, mk_gemm.hpp;
MK_DIAG_SYRK, default 1) against the full-square bodies it replaces (MK_DIAG_SYRK=0): every
lower-triangle element accumulates the same MFMA sequence, so factors, log-determinants, inverses
and whole chains are equal bit for bit.  With the switch on the fused launches also deal their extra
jobs after the row jobs (xcd_map_tail): a different placement of the same work, covered by the same
comparisons.  The switch is read once per process, so each arm of each case runs in its own
subprocess.

The three bit-identity tests of tests/test_gpu_linalg.py compare 128-tile runs with 64- and
32-sub-tile runs; the sub-tile instances keep the quadrant body, so with the switch on those tests
also check the new body against the old one."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

REL = 1e-10
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"

# seeded exponential-correlation matrices, as tests/test_gpu_linalg.py's _FUSED_RUN takes them
_CHOL_RUN = """
import importlib, sys, numpy as np
sys.path.insert(0, {root!r})
mk = importlib.import_module({pkg!r})
rng = np.random.default_rng(11)
S, n = {S}, {n}
c = rng.uniform(size=(S, n, 2))
d = np.sqrt(((c[:, :, None, :] - c[:, None, :, :]) ** 2).sum(-1))
A = np.exp(-(3.0 + rng.uniform(size=(S, 1, 1)) * 6.0) * d)
L, ld, inv = mk.cholesky_batched(A, inverse=True)
np.savez({path!r}, A=A[:4], L=L, ld=ld, inv=inv)
"""


def _arms(tmp_path, tag, argv_of, env):
    """Both arms of one case, each in its own process -> {arm: {name: array}}."""
    res = {}
    for arm in ("1", "0"):
        path = str(tmp_path / f"{tag}_syrk{arm}.npz")
        r = subprocess.run(argv_of(path), capture_output=True, text=True, timeout=240,
                           env=dict(os.environ, MK_DIAG_SYRK=arm, **env))
        assert r.returncode == 0, r.stderr[-4000:]
        z = np.load(path)
        res[arm] = {k: z[k] for k in z.files}
    return res


# S = 136: >= 128 factors, so every fused launch (and every unfused update but the last column's)
# takes 128-tiles.
#   n = 300: nt = 3, one fused launch with K = 128, the diagonal launches' corrections by panels 0, 1
#   n = 520: nt = 5, K up to 384, a ragged last tile
#   n = 383: n + 1 = 384 fills the last tile exactly
#   MK_CHOL_FUSED=0: the diagonal tile of k_chol_update<128, 128>
#   S = 8, MK_TILE=64, unsplit: the extra job of k_chol_update_trsm<64>
@pytest.mark.parametrize("S,n,env", [(136, 300, {}), (136, 520, {}), (136, 383, {}),
                                     (136, 520, {"MK_CHOL_FUSED": "0"}),
                                     (8, 520, {"MK_TILE": "64", "MK_CHOL_SPLIT": "0"})],
                         ids=["n300", "n520", "n383", "n520_unfused", "n520_rows64"])
def test_factor_logdet_inverse_are_bit_identical(tmp_path, S, n, env):
    res = _arms(tmp_path, f"chol{n}",
                lambda path: [sys.executable, "-c", _CHOL_RUN.format(root=ROOT, pkg=PKG, S=S, n=n, path=path)], env)
    for k in ("L", "ld", "inv"):
        assert np.array_equal(res["1"][k], res["0"][k]), k
    for s in range(4):
        Lr = sla.cholesky(res["1"]["A"][s], lower=True)
        assert np.linalg.norm(res["1"]["L"][s] - Lr) <= REL * np.linalg.norm(Lr)


def test_chains_are_bit_identical(tmp_path):
    """tests/gpu_tile_run.py under the sequential schedule with 128-tiles forced: samples, latent w,
    kriging draws, the tiled replay and a plain factorisation."""
    env = {"MK_TILE": "128", "MK_SWEEP": "1", "MK_CHOL_SPLIT": "0", "MK_PRED_GEN": "0", "MK_CHOL_DEPTH": "2",
           "MK_LOOKAHEAD": "0"}
    res = _arms(tmp_path, "chain", lambda path: [sys.executable, os.path.join(HERE, "gpu_tile_run.py"), path], env)
    assert res["1"].keys() == res["0"].keys() and len(res["1"]) > 0
    for k in res["1"]:
        assert np.array_equal(res["1"][k], res["0"][k]), k
