"""The batched Cholesky, log-determinant and explicit inverse (mk.cholesky_batched, the sampler's own
launch_cholesky / launch_trinv) against references that do not live in this repository's kernels --
LAPACK's dpotrf / dpotri, and an 80-bit factorisation (tests/linalg_ref.py, itself under test in
tests/test_linalg_ref.py) -- on every launch policy, every matrix of every batch.

tile_size() (mk_schedule.hip) is evaluated per launch and the split form is chosen per session
(setup_groups, mk_api.hip), so one table of cases (tests/gpu_linalg_run.py, with what each case pins)
runs under ten arms: the default policy and every switch that selects another body or schedule.  The
switches are read once per process: one child per arm, one test per child.  The bounds are derived
(tests/linalg_ref.py), not measured; the last two tests compare the digests of L, ld and inv across
the arms (mk_gemm.hpp: the same MFMA sequence per element, whatever the tile shape or schedule) and
across batch sizes, so pruning a variant removes an arm, not a test.

Largest values per case, device | LAPACK (MI355X, default arm; kappa_2 on the host):

  kind   S    n     kappa_2   backward             inverse              forward L            forward ld
  exp    3    127   7.42e03   2.84e-16 | 2.06e-16  3.65e-17 | 2.76e-17  7.90e-16 | 1.37e-15  9.02e-14 | 3.25e-14
  exp    3    128   1.85e03   2.99e-16 | 2.07e-16  4.22e-17 | 3.39e-17  6.74e-16 | 1.41e-15  4.13e-14 | 4.39e-14
  exp    3    129   2.01e03   2.73e-16 | 1.90e-16  4.29e-17 | 3.82e-17  5.81e-16 | 5.05e-16  6.86e-14 | 1.85e-14
  exp    136  127   1.47e04   2.95e-16 | 2.16e-16  6.33e-17 | 4.69e-17  7.73e-16 | 1.13e-15  5.17e-14 | 1.45e-14
  exp    136  128   1.24e04   3.01e-16 | 2.08e-16  5.98e-17 | 5.18e-17  7.44e-16 | 1.06e-15  1.39e-14 | 4.15e-14
  exp    136  255   4.14e04   4.78e-16 | 2.98e-16  8.68e-17 | 3.73e-17  2.86e-15 | 3.72e-15  9.45e-14 | 8.40e-14
  exp    136  256   4.64e04   4.87e-16 | 2.93e-16  7.35e-17 | 5.41e-17  2.16e-15 | 2.67e-15  1.25e-13 | 5.12e-14
  exp    136  383   7.62e04   5.58e-16 | 3.55e-16  5.68e-17 | 4.13e-17  3.26e-15 | 5.00e-15  2.67e-13 | 4.15e-13
  exp    136  384   1.12e05   5.66e-16 | 3.58e-16  9.82e-17 | 5.03e-17  3.77e-15 | 6.64e-15  9.25e-14 | 2.49e-13
  exp    136  520   2.30e05   6.08e-16 | 3.51e-16  9.82e-17 | 4.41e-17  3.74e-15 | 7.26e-15  6.25e-14 | 1.72e-13
  exp    72   1000  7.09e05   7.54e-16 | 4.01e-16  1.32e-16 | 3.98e-17  -                    -
  exp    32   1100  2.81e05   7.66e-16 | 3.64e-16  8.41e-17 | 3.36e-17  -                    -
  matern 3    383   4.84e10   9.69e-16 | 3.16e-16  6.29e-17 | 5.00e-17  1.31e-11 | 1.01e-11  2.81e-08 | 7.62e-08
  matern 3    520   1.43e11   1.46e-15 | 3.14e-16  5.02e-17 | 4.32e-17  1.89e-11 | 1.45e-11  7.73e-08 | 1.97e-07
  matern 136  383   1.06e12   4.87e-15 | 3.25e-16  2.28e-16 | 5.00e-17  1.31e-11 | 1.01e-11  2.81e-08 | 7.62e-08
  matern 3    1000  4.34e11   9.28e-16 | 3.22e-16  1.09e-16 | 3.65e-17  -                    -
  exp    136  1000  7.03e05   7.57e-16 | 4.03e-16  1.20e-16 | 4.02e-17  -                    -
  exp    136* 383   7.62e04   5.50e-16 | 3.48e-16  4.68e-17 | 2.86e-17  3.26e-15 | 5.00e-15  2.67e-13 | 4.15e-13

(136*: matrices 0, 68 and 135 of the batch of 136, factored alone.  forward: against the 80-bit
factorisation, matrices 0, S // 2 and S - 1 where n <= 520.)  Every arm gave the default arm's bits, so
these are every arm's values.  The bars: backward (n + 1) eps = 2.8e-14 .. 2.4e-13, the others
(n + 1) eps kappa_2.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_linalg_run as run

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

ARMS = {
    "default": {},
    "tile128": {"MK_TILE": "128"},
    "tile64": {"MK_TILE": "64"},
    "tile32": {"MK_TILE": "32"},
    "unfused": {"MK_CHOL_FUSED": "0"},
    "unsplit": {"MK_CHOL_SPLIT": "0"},
    "split_depth1": {"MK_CHOL_SPLIT": "1", "MK_CHOL_DEPTH": "1"},
    "split_depth3": {"MK_CHOL_SPLIT": "1", "MK_CHOL_DEPTH": "3"},
    "diag_square": {"MK_DIAG_SYRK": "0"},
    "inv_quadrant_tile128": {"MK_INV_DEAL": "0", "MK_TILE": "128"},
}
SWITCHES = sorted({k for env in ARMS.values() for k in env})


@pytest.fixture(scope="module")
def arm_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("linalg_policies")


def _arm(arm_dir, arm):
    """The child's record of one arm; each arm runs once per module run."""
    path = os.path.join(str(arm_dir), arm + ".npz")
    if not os.path.exists(path):
        memo = os.path.join(str(arm_dir), "memo")
        os.makedirs(memo, exist_ok=True)
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(ARMS[arm])
        r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_linalg_run.py"), path + ".part.npz",
                            "full" if arm == "default" else "arms", memo],
                           capture_output=True, text=True, timeout=110, env=env)
        assert r.returncode == 0, r.stderr[-4000:]
        os.replace(path + ".part.npz", path)
    with np.load(path) as z:
        return json.loads(str(z["meta"]))


def _worst(rec, name):
    vals = [m[name] for m in rec["metrics"] if name in m]
    return max(vals) if vals else float("nan")


@pytest.mark.parametrize("arm", list(ARMS))
def test_factor_logdet_inverse_meet_the_bounds(arm_dir, arm):
    """Every matrix of every case: L exactly lower with a positive diagonal, ld finite, inv bitwise
    symmetric; the factor's backward residual within (n + 1) eps and the inverse's residual within
    (n + 1) eps kappa_2 (on LAPACK's own scale, not on the device's); the exponential cases within the
    project's 1e-10 / 1e-9 of LAPACK; matrices 0, S // 2 and S - 1 of the cases with n <= 520 within
    (n + 1) eps kappa_2 of the 80-bit factor and log-determinant."""
    meta = _arm(arm_dir, arm)
    table = run.TABLES["full" if arm == "default" else "arms"]
    assert list(meta) == [run.case_key(c) for c in table]
    broken = {}
    for case in table:
        S, n, kind, seed, pick = case
        rec = meta[run.case_key(case)]
        nb = S if pick is None else len(pick)
        assert len(rec["metrics"]) == len(rec["digests"]) == nb
        fwd = [s for s in range(nb) if "fwd_L" in rec["metrics"][s]]
        assert tuple(fwd) == run.forward_rows(case)
        print(f"{arm} {run.case_key(case)}: kappa2 {_worst(rec, 'kappa2'):.2e}"
              f" backward {_worst(rec, 'backward'):.2e} | {_worst(rec, 'backward_lapack'):.2e}"
              f" inverse {_worst(rec, 'inv_resid'):.2e} | {_worst(rec, 'inv_resid_lapack'):.2e}"
              f" fwd L {_worst(rec, 'fwd_L'):.2e} | {_worst(rec, 'fwd_L_lapack'):.2e}"
              f" fwd ld {_worst(rec, 'fwd_ld'):.2e} | {_worst(rec, 'fwd_ld_lapack'):.2e}"
              f" vs LAPACK L {_worst(rec, 'L_vs_lapack'):.2e} ld {_worst(rec, 'ld_vs_lapack'):.2e}"
              f" inv {_worst(rec, 'inv_vs_lapack'):.2e}")
        # the bounds again, from the metrics: the child's verdict decides only which arrays it keeps
        for s, m in enumerate(rec["metrics"]):
            v = run.lr.violations(m, kind)
            assert v == rec["violations"].get(str(s), [])
            if v:
                broken[f"{run.case_key(case)}[{s}]"] = v
    assert not broken, (f"{len(broken)} matrices break a bound (arrays of the first few: {arm_dir}/{arm}.npz): "
                        + json.dumps(dict(list(broken.items())[:8]), indent=1))


@pytest.mark.timeout(900)     # run alone it starts every arm's child; after the tests above, none
def test_arms_agree_bit_for_bit(arm_dir):
    """For the same (S, n, kind, seed) the SHA-256 of L, of ld and of inv is the same in every arm,
    matrix by matrix."""
    ref = _arm(arm_dir, "default")
    differ = []
    for arm in ARMS:
        meta = _arm(arm_dir, arm)
        assert meta, arm
        for key, rec in meta.items():
            for s, (a, b) in enumerate(zip(rec["digests"], ref[key]["digests"])):
                for name, x, y in zip(("L", "ld", "inv"), a, b):
                    if x != y:
                        differ.append(f"{arm} {key}[{s}] {name}")
    assert not differ, f"{len(differ)} arrays differ from the default arm's: {differ[:12]}"


def test_batch_size_does_not_change_the_bits(arm_dir):
    """Matrices 0, 68 and 135 of the S = 136, n = 383 batch (128-tiles, fused) factored alone as a batch
    of three (64-sub-tiles, split two-stream form): the same L, ld and inv bit for bit -- the README's
    claim that sharding does not change a chain, at the kernel."""
    meta = _arm(arm_dir, "default")
    big = meta[run.case_key((136, 383, "exp", 11, None))]["digests"]
    small = meta[run.case_key((136, 383, "exp", 11, run.PICK))]["digests"]
    assert len(small) == len(run.PICK)
    for i, s in enumerate(run.PICK):
        assert small[i] == big[s], (i, s)
