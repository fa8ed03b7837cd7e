"""The work-balanced job map of the inverse levels (inv_map_job, csrc/mk_types.hpp; MK_INV_MAP, default 1)
against xcd_map's equal-count cut (MK_INV_MAP=0): the map changes only which workgroup computes which
tile, so inverses and whole chains are equal bit for bit, and the inverse still meets LAPACK's.  The host
side of the map (exact cover of the grid, balance, order) is tests/test_inv_map_host.py's.

MK_INV_MAP and MK_TILE are read once per process, so each arm runs in its own subprocess; one
subprocess computes all the (n, S) cases of its arm.  MK_TILE is forced: 128 reaches k_inv_level<128>
at these sizes (the launch policy would pick sub-tiles), 64 the instance with four workgroups per tile.

n (padded order n + 1, 128-tiles): 200 -> nt = 2, level 1 only; 383 -> nt = 3, a pair whose B block is
absent; 520 -> nt = 5, a ragged pair at the top level; 1000 -> nt = 8, K ranges of 1 to 4 tiles.
S: 1 and 3 are fewer entries than XCDs (one matrix cut over several), 9 and 13 no multiples of 8 (cuts
inside matrices)."""
import functools
import hashlib
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
NS = (200, 383, 520, 1000)
SS = (1, 3, 9, 13)


def _matrices(S, n):
    """Seeded exponential-correlation matrices (the generator of tests/test_gpu_inv_deal.py's _CHOL_RUN)."""
    rng = np.random.default_rng(11)
    c = rng.uniform(size=(S, n, 2))
    d = np.sqrt(((c[:, :, None, :] - c[:, None, :, :]) ** 2).sum(-1))
    return np.exp(-(3.0 + rng.uniform(size=(S, 1, 1)) * 6.0) * d)


# every case in one process: digests of L, ld and inv; the inverses themselves when keep is set
_RUN = """
import hashlib, importlib, sys, numpy as np
sys.path.insert(0, {root!r})
sys.path.insert(0, {here!r})
mk = importlib.import_module({pkg!r})
from test_gpu_inv_map import _matrices
out = {{}}
for n in {ns!r}:
    for S in {ss!r}:
        L, ld, inv = mk.cholesky_batched(_matrices(S, n), inverse=True)
        for name, a in (("L", L), ("ld", ld), ("inv", inv)):
            out[f"{{name}}_{{n}}_{{S}}"] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)
        if {keep}:
            out[f"arr_{{n}}_{{S}}"] = inv
np.savez({path!r}, **out)
"""


@pytest.fixture(scope="module")
def inverses(tmp_path_factory):
    """{(tile, map): npz} -- computed once per tile, both arms."""
    cache = {}

    def get(tile):
        if (tile, "1") not in cache:
            d = tmp_path_factory.mktemp(f"invmap{tile}")
            for arm in ("1", "0"):
                path = str(d / f"arm{arm}.npz")
                code = _RUN.format(root=ROOT, here=HERE, pkg=PKG, ns=NS, ss=SS, keep=arm == "1", path=path)
                r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                                   env=dict(os.environ, MK_INV_MAP=arm, MK_TILE=tile))
                assert r.returncode == 0, r.stderr[-4000:]
                cache[(tile, arm)] = np.load(path)
        return cache[(tile, "1")], cache[(tile, "0")]
    return get


@functools.lru_cache(maxsize=None)
def _lapack(n, S):
    """LAPACK dpotri of the LAPACK factor, full symmetric: the reference tests/test_gpu_linalg.py takes."""
    refs = []
    for a in _matrices(S, n):
        ref, info = sla.lapack.dpotri(sla.cholesky(a, lower=True), lower=1)
        assert info == 0
        refs.append(np.tril(ref) + np.tril(ref, -1).T)
    return refs


@pytest.mark.parametrize("tile", ["128", "64"])
@pytest.mark.parametrize("S", SS)
@pytest.mark.parametrize("n", NS)
def test_inverse_is_bit_identical(inverses, n, S, tile):
    new, old = inverses(tile)
    for name in ("inv", "L", "ld"):
        assert np.array_equal(new[f"{name}_{n}_{S}"], old[f"{name}_{n}_{S}"]), name
    inv = new[f"arr_{n}_{S}"]
    # the digest is of what is checked against LAPACK
    assert np.array_equal(np.frombuffer(hashlib.sha256(np.ascontiguousarray(inv).tobytes()).digest(), np.uint8),
                          new[f"inv_{n}_{S}"])
    assert inv.shape == (S, n, n)
    for s, ref in enumerate(_lapack(n, S)):
        assert np.linalg.norm(inv[s] - ref) <= REL * np.linalg.norm(ref), s


def test_chains_are_bit_identical(tmp_path):
    """tests/gpu_tile_run.py under the sequential schedule with 128-tiles forced (the environment of
    tests/test_gpu_inv_deal.py's chain test): samples, latent w, kriging draws, the tiled replay.  The
    lists of accepted factors are shorter than the grids' maximum here."""
    env = {"MK_SWEEP": "1", "MK_CHOL_SPLIT": "0", "MK_PRED_GEN": "0", "MK_CHOL_DEPTH": "2", "MK_LOOKAHEAD": "0",
           "MK_TILE": "128"}
    res = {}
    for arm in ("1", "0"):
        path = str(tmp_path / f"chain_{arm}.npz")
        r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_tile_run.py"), path], capture_output=True,
                           text=True, timeout=240, env=dict(os.environ, **env, MK_INV_MAP=arm))
        assert r.returncode == 0, r.stderr[-4000:]
        z = np.load(path)
        res[arm] = {k: z[k] for k in z.files}
    assert res["1"].keys() == res["0"].keys() and len(res["1"]) > 0
    for k in res["1"]:
        assert np.array_equal(res["1"][k], res["0"][k]), k
