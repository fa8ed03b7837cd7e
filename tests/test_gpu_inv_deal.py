"""The dealt body of the 128-tile inverse levels (gemm_deal_128, mk_gemm.hpp; MK_INV_DEAL, default 1)
against the quadrant body with its per-MFMA predicates (MK_INV_DEAL=0) and against the 64-sub-tile
instance, which keeps the quadrant body: every element accumulates the same MFMA sequence and the
skipped blocks are the same, so inverses and whole chains are equal bit for bit.  The switch and
MK_TILE are read once per process, so each arm of each case runs in its own subprocess.

MK_TILE=128 is forced: at these sizes the launch policy would pick 64-sub-tiles and never reach
k_inv_level<128> (launch_trinv, mk_schedule.hip: cholesky_batched(inverse=True) goes through it)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

REL = 1e-9      # tests/test_gpu_linalg.py's bar for the inverse
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"

# seeded exponential-correlation matrices, the generator of tests/test_gpu_diag_syrk.py's _CHOL_RUN
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

# (MK_INV_DEAL, MK_TILE): the new body, the quadrant body with today's predicates, the 64-sub-tiles
ARMS = {"deal": ("1", "128"), "quad": ("0", "128"), "sub64": ("1", "64")}


def _arms(tmp_path, tag, argv_of, env, arms):
    """One process per arm -> {arm: {name: array}}."""
    res = {}
    for arm in arms:
        deal, tile = ARMS[arm]
        path = str(tmp_path / f"{tag}_{arm}.npz")
        r = subprocess.run(argv_of(path), capture_output=True, text=True, timeout=240,
                           env=dict(os.environ, **env, MK_INV_DEAL=deal, MK_TILE=tile))
        assert r.returncode == 0, r.stderr[-4000:]
        z = np.load(path)
        res[arm] = {k: z[k] for k in z.files}
    return res


# S = 8 (padded order n + 1, 128-tiles):
#   n = 200:  nt = 2, level 1 only: the triangular tile is the whole K range, no dense chunk
#   n = 383:  n + 1 fills the last tile exactly; nt = 3, a pair whose B block is absent
#   n = 500:  nt = 4, K of 1 and 2 tiles in both phases, ragged last tile
#   n = 520:  nt = 5, a ragged pair at the top level
#   n = 1000: nt = 8, K of 1 to 4 tiles in both phases, the descending order across several dense
#             tiles before the triangular one
@pytest.mark.parametrize("n", [200, 383, 500, 520, 1000])
def test_inverse_is_bit_identical(tmp_path, n):
    res = _arms(tmp_path, f"inv{n}",
                lambda path: [sys.executable, "-c", _CHOL_RUN.format(root=ROOT, pkg=PKG, S=8, n=n, path=path)], {},
                ("deal", "quad", "sub64"))
    new = res["deal"]
    for other in ("quad", "sub64"):
        for k in ("inv", "L", "ld"):
            assert np.array_equal(new[k], res[other][k]), (other, k)
    for s in range(4):
        # LAPACK dpotri of the LAPACK factor, full symmetric: the reference tests/test_gpu_linalg.py takes
        ref, info = sla.lapack.dpotri(sla.cholesky(new["A"][s], lower=True), lower=1)
        assert info == 0
        ref = np.tril(ref) + np.tril(ref, -1).T
        assert np.linalg.norm(new["inv"][s] - ref) <= REL * np.linalg.norm(ref)


def test_chains_are_bit_identical(tmp_path):
    """tests/gpu_tile_run.py under the sequential schedule with 128-tiles forced (the environment of
    tests/test_gpu_diag_syrk.py's chain test): samples, latent w, kriging draws, the tiled replay."""
    env = {"MK_SWEEP": "1", "MK_CHOL_SPLIT": "0", "MK_PRED_GEN": "0", "MK_CHOL_DEPTH": "2", "MK_LOOKAHEAD": "0"}
    res = _arms(tmp_path, "chain", lambda path: [sys.executable, os.path.join(HERE, "gpu_tile_run.py"), path], env,
                ("deal", "quad"))
    assert res["deal"].keys() == res["quad"].keys() and len(res["deal"]) > 0
    for k in res["deal"]:
        assert np.array_equal(res["deal"][k], res["quad"][k]), k
