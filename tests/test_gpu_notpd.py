"""Factorisations that fail (a candidate whose Cholesky fails is a rejection, not an
abort, and the counts are reported).

A. The flag of k_chol_diag (a non-border pivot that is not > 0) through mk_cholesky_batched: negative,
   exactly zero and NaN pivots at the first and last row, the 16-block and 128-tile edges, in tiles
   0 / 1 / 2, for a small batch and for the fused 128-tile launches (136 factors; MK_DIAG_SYRK=1 and 0,
   each in its own process), and the calls that follow a failed one.
B. A start that cannot be factored is an error from mk_session_create: the host refuses a non-finite
   coordinate and two sites at the same coordinates, the device flag refuses what is left.
C. A chain driven through flagged candidates (tests/gpu_notpd_run.py): everything finite, the same bits
   and the same counts on every code path, no more moves than unflagged proposals, and the tiled replay
   equal to the fused kriging."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.linalg as sla

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = "laurabaracaldo-spatial-meta-kriging-for-distributed-inference-for-binary-response_amd"
MK_E_ARG = -1           # include/mk.h: mk_cholesky_batched and mk_session_create, a matrix that is not PD

# (n, j): first and last pivot, 16-block edges inside a tile, tile edges, the last real row beside the
# border row, tiles 0 / 1 / 2
NJ = [(5, 4), (200, 0), (200, 15), (200, 16), (200, 127), (200, 128), (200, 199), (300, 255), (300, 256), (300, 299)]


def base(S, n, seed):
    """Exponential correlation of uniform sites, phi in [4, 10] (test_cholesky_logdet_inverse's matrices)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(size=(S, n, 2))
    d = np.sqrt(((c[:, :, None, :] - c[:, None, :, :]) ** 2).sum(-1))
    return np.exp(-np.linspace(4.0, 10.0, S)[:, None, None] * d)


def spoil(A, s_bad, kind, j):
    """Spoils matrix s_bad of the batch in place; returns the row LAPACK must stop at (0-based)."""
    M = A[s_bad]
    if kind == "neg":        # pivot j = -1 - sum l^2 < 0 whatever the rounding; earlier pivots untouched
        M[j, j] = -1.0
    elif kind == "zero":     # l_10 = 1, pivot 1 = 1 - 1 * 1 = 0 exactly
        assert j == 1
        M[0, 0] = M[0, 1] = M[1, 0] = M[1, 1] = 1.0
    elif kind == "nan":      # l_ji = NaN, pivot j = NaN
        i = j // 2
        assert i < j
        M[j, i] = M[i, j] = np.nan
    else:
        raise ValueError(kind)
    return j


def cases(n_js):
    out = []
    for n, j in n_js:
        out.append((n, j, "neg"))
        if j > 0:
            out.append((n, j, "nan"))
    return out + [(n, 1, "zero") for n in sorted({n for n, _ in n_js})]


def lapack_info(M):
    """dpotrf's info on the lower triangle."""
    return sla.lapack.dpotrf(np.asfortranarray(M), lower=1, clean=0)[1]


def check_fixture(M, kind, row):
    """LAPACK stops at the spoiled row (negative and zero pivots; an optimised dpotrf need not test a
    NaN pivot, so that fixture shows only where its NaNs are)."""
    if kind == "nan":
        assert np.argwhere(np.isnan(M)).tolist() == [[row // 2, row], [row, row // 2]]
        return 0
    info = int(lapack_info(M))
    assert info == row + 1, (kind, row, info)
    return info


def named_matrix(msg):
    m = re.search(r"matrix (\d+) is not positive definite", msg)
    assert m, msg
    return int(m.group(1))


# ---------------------------------------------------------------- A. small batch, in process
@pytest.mark.parametrize("n,j,kind", cases(NJ), ids=lambda v: str(v))
def test_flag_small_batch(mk, n, j, kind):
    """S = 3, s_bad = 1.  The zero pivot rests on rsqrt_sqrt(1.0) returning exactly (1, 1): on the
    MI355X it does (test_zero_pivot_is_exact_on_the_device shows it)."""
    S, s_bad = 3, 1
    A = base(S, n, 100 + n)
    row = spoil(A, s_bad, kind, j)
    check_fixture(A[s_bad], kind, row)                       # the fixture proves itself
    assert all(lapack_info(A[s]) == 0 for s in range(S) if s != s_bad)
    with pytest.raises(mk.MkError) as e:
        mk.cholesky_batched(A, inverse=True)
    assert e.value.code == MK_E_ARG
    assert named_matrix(str(e.value)) == s_bad


@pytest.mark.parametrize("n", [5, 300])
def test_zero_pivot_is_exact_on_the_device(mk, n):
    """What the zero-pivot case supposes, shown on the device: rsqrt_sqrt(1.0) is exactly (1, 1).  Row
    and column 1 are copies of row and column 0 (A[0, 0] = 1), so l_k1 = 0 for k > 1 and nothing after
    pivot 1 can fail.  With A[1, 1] = 1 + 2^-52 the factor must come back with L[1, 0] = 1 and
    L[1, 1] = 2^-26 to the bit (pivot 1 = 2^-52 exactly: l_10^2 = 1); with A[1, 1] = 1 the pivot is 0 and
    only the comparison `> 0` can flag it."""
    A = base(3, n, 7)
    A[1, 1, :] = A[1, 0, :]
    A[1, :, 1] = A[1, :, 0]
    A[1, 1, 1] = 1.0 + 2.0 ** -52
    L, ld = mk.cholesky_batched(A)
    assert L[1, 1, 0] == 1.0 and L[1, 1, 1] == 2.0 ** -26
    assert np.count_nonzero(L[1, 2:, 1]) == 0 and np.isfinite(L).all()
    A[1, 1, 1] = 1.0
    assert lapack_info(A[1]) == 2
    with pytest.raises(mk.MkError) as e:
        mk.cholesky_batched(A)
    assert e.value.code == MK_E_ARG and named_matrix(str(e.value)) == 1


@pytest.mark.parametrize("kind", ["neg", "nan"])
def test_two_spoiled_matrices_name_the_lower_index(mk, kind):
    A = base(3, 300, 5)
    spoil(A, 2, kind, 17)
    spoil(A, 1, kind, 299)
    with pytest.raises(mk.MkError) as e:
        mk.cholesky_batched(A)
    assert e.value.code == MK_E_ARG and named_matrix(str(e.value)) == 1


def after_failure(mk, S, n, s_bad):
    """good, failing, good with the same (S, n): the second good call gets the failed call's buffers
    back (NaN factor slots, W, logdet partials) and must give the first call's bits."""
    A = base(S, n, 9)
    first = mk.cholesky_batched(A, inverse=True)
    B = A.copy()
    spoil(B, s_bad, "nan", 130)
    with pytest.raises(mk.MkError):
        mk.cholesky_batched(B, inverse=True)
    again = mk.cholesky_batched(A, inverse=True)
    for a, b in zip(first, again):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        assert np.array_equal(a, b)


def test_call_after_a_failed_call_small_batch(mk):
    after_failure(mk, 3, 300, 1)


# ---------------------------------------------------------------- A. the fused 128-tile launches
# S = 136 >= 128 factors: k_chol_update_trsm, and with MK_DIAG_SYRK=1 the SYRK diagonal body.  n = 300 pads
# to 384: 320 MB of factor slots.  The switch is read once per process: one child per arm runs every case.
_FUSED_CHILD = """
import importlib, json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {here!r})
import numpy as np
mk = importlib.import_module({pkg!r})
import test_gpu_notpd as T
S, s_bad, n = 136, 77, 300
res = []
good = T.base(S, n, 9)
for n_, j, kind in T.cases([c for c in T.NJ if c[0] == n]) + [(n, 299, "two")]:
    A = good.copy()
    if kind == "two":
        T.spoil(A, 100, "neg", 3); T.spoil(A, s_bad, "nan", j)
        row = j
    else:
        row = T.spoil(A, s_bad, kind, j)
    T.check_fixture(A[s_bad], "nan" if kind == "two" else kind, row)
    rec = dict(j=j, kind=kind, code=0, msg="")
    try:
        mk.cholesky_batched(A, inverse=True)
    except mk.MkError as e:
        rec.update(code=e.code, msg=str(e))
    res.append(rec)
T.after_failure(mk, S, n, s_bad)
json.dump(res, open({path!r}, "w"))
"""


@pytest.mark.parametrize("syrk", ["1", "0"])
def test_flag_fused_launches(tmp_path, syrk):
    path = str(tmp_path / f"fused_{syrk}.json")
    r = subprocess.run([sys.executable, "-c", _FUSED_CHILD.format(root=ROOT, here=HERE, pkg=PKG, path=path)],
                       capture_output=True, text=True, timeout=110, env=dict(os.environ, MK_DIAG_SYRK=syrk))
    assert r.returncode == 0, r.stderr[-4000:]          # includes the call after the failure (after_failure)
    res = json.load(open(path))
    assert len(res) == len(cases([c for c in NJ if c[0] == 300])) + 1
    for rec in res:
        assert rec["code"] == MK_E_ARG, rec
        assert named_matrix(rec["msg"]) == 77, rec      # "two": 77 and 100 are spoiled, the lower is named


# ---------------------------------------------------------------- B. a start that cannot be factored
def _subsets(mk, sizes, q, cov, seed=3):
    d = mk.synthetic.generate(sum(sizes), q=q, n_test=0, seed=seed, cov_model=cov)
    subs, off = [], 0
    for m in sizes:
        rows = slice(off * q, (off + m) * q)
        subs.append(dict(coords=d["coords"][off:off + m].copy(), y=d["y"][rows], weights=np.ones(m * q), x=d["x"][rows]))
        off += m
    return subs


def _cfg(mk, q, cov):
    p = 2 * q
    return mk.SamplerConfig(q, p, np.zeros(p), np.full(p, 0.05), cov_model="matern" if cov else "exponential",
                            n_batch=1, batch_length=3, burn_in=1, seed=5)


def _refused(mk, subs, cfg, pattern):
    """Session(...) raises MkError matching pattern, leaves no session behind, and a good session of
    the same shape runs afterwards."""
    lib = mk.load()
    live = lib.mk_session_count()
    with pytest.raises(mk.MkError) as e:
        mk.Session(subs, cfg)
    assert e.value.code == MK_E_ARG
    assert re.search(pattern, str(e.value)), str(e.value)
    assert lib.mk_session_count() == live
    good = _subsets(mk, [len(s["coords"]) for s in subs], cfg.q, 1 if cfg.cov_model == "matern" else 0)
    with mk.Session(good, cfg) as ses:
        ses.run(cfg.n_samples)
        o = ses.outputs(samples=True)
        assert not ses.notpd_counts().any()
    assert all(np.isfinite(x).all() for x in o["samples"])
    assert lib.mk_session_count() == live


@pytest.mark.parametrize("cov", [0, 1], ids=["exponential", "matern"])
@pytest.mark.parametrize("a,b", [(0, 1), (17, 41)])
def test_repeated_site_is_refused_at_create(mk, cov, a, b):
    """60 sites, site b a copy of site a.  (0, 1): pivot 1 is exactly 0, the device flag would see it
    too; (17, 41): the pivot's sign is rounding, only the host check is sure to."""
    subs = _subsets(mk, [60], 1, cov)
    subs[0]["coords"][b] = subs[0]["coords"][a]
    _refused(mk, subs, _cfg(mk, 1, cov), rf"subset 0: sites {a} and {b} have the same coordinates")


def test_refusal_names_the_bad_subset(mk):
    subs = _subsets(mk, [60, 50, 70], 2, 0)
    subs[2]["coords"][33] = subs[2]["coords"][8]
    _refused(mk, subs, _cfg(mk, 2, 0), r"subset 2: sites 8 and 33 ")


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_coordinate_is_refused_at_create(mk, bad):
    subs = _subsets(mk, [60, 60], 1, 0)
    subs[1]["coords"][7, 1] = bad
    _refused(mk, subs, _cfg(mk, 1, 0), r"subset 1: site 7 has a non-finite coordinate")


def test_sites_that_share_one_coordinate_are_accepted(mk):
    """The host check compares both coordinates: equal x or equal y alone is an ordinary subset."""
    subs = _subsets(mk, [60], 1, 0)
    x0, y0 = subs[0]["coords"][0]
    subs[0]["coords"][1] = (x0, y0 + 1e-3)
    subs[0]["coords"][2] = (x0 + 1e-3, y0)
    cfg = _cfg(mk, 1, 0)
    with mk.Session(subs, cfg) as ses:
        ses.run(cfg.n_samples)
        assert not ses.notpd_counts().any()
        assert np.isfinite(ses.outputs(samples=True)["samples"][0]).all()


@pytest.mark.parametrize("cov", [0, 1], ids=["exponential", "matern"])
def test_device_flag_refuses_a_singular_start_the_host_cannot_see(mk, cov):
    """Two sites one ulp apart at the origin, (0, 0) and (5e-324, 0): different coordinates, so the
    host check passes; d^2 underflows to 0, rho = 1 exactly, pivot 1 = 1 - 1 * 1 = 0, and the flag read
    back in initial_state is what refuses the session."""
    subs = _subsets(mk, [50, 60], 1, cov)
    subs[1]["coords"][0] = (0.0, 0.0)
    subs[1]["coords"][1] = (5e-324, 0.0)
    R = mk.correlation_batched(subs[1]["coords"][None], [6.0], nu=[0.5] if cov else None,
                               cov_model="matern" if cov else "exponential")
    assert R[0, 1, 0] == 1.0
    _refused(mk, subs, _cfg(mk, 1, cov), r"subset 1, outcome 0: .*not positive definite")


# ---------------------------------------------------------------- C. a chain through flagged candidates
# (MK_TILE, MK_SWEEP, MK_CHOL_SPLIT, extra); the first of each schedule is its reference.  MK_SWEEP=1: the site
# sweep agrees with the block sweep only to rounding, and this shard amplifies rounding.
SCHEDULES = {
    "lookahead": (("128", "1", None, {}),
                  ("64", "1", "1", {}),
                  ("32", "1", "1", {}),
                  ("128", "1", None, {"MK_CHOL_FUSED": "0"})),
    "sequential": (("128", "1", None, {"MK_LOOKAHEAD": "0"}),
                   ("64", "3", "1", {"MK_LOOKAHEAD": "0", "MK_CHOL_DEPTH": "1"}),
                   ("128", "1", None, {"MK_LOOKAHEAD": "0", "MK_EARLY_COV": "0"})),
}


def _hostile_run(tmp_path, tag, tile, sweep, split, extra):
    path = str(tmp_path / f"{tag}.npz")
    env = dict(os.environ, MK_TILE=tile, MK_SWEEP=sweep, **extra)
    if split is not None:
        env["MK_CHOL_SPLIT"] = split
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_notpd_run.py"), path], capture_output=True, text=True,
                       timeout=100, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    z = np.load(path)
    return {k: z[k] for k in z.files}, [int(v) for v in open(path + ".notpd").read().split()]


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_chain_through_flagged_candidates(tmp_path, schedule):
    sys.path.insert(0, HERE)
    import gpu_notpd_run as H
    runs = [_hostile_run(tmp_path, f"{schedule}_{i}", *cfg) for i, cfg in enumerate(SCHEDULES[schedule])]
    ref, counts = runs[0]
    # the path was taken, and not by every proposal
    assert len(counts) == len(H.SIZES)
    for c in counts:
        assert 0 < c < H.PROPOSALS, counts
    # 1. everything returned is finite: samples, w, kriging draws, both quantile grids, the chain state
    for k, v in ref.items():
        assert np.isfinite(v).all(), k
    # 2. the same bits and the same flags on every code path of this schedule
    for i, (got, cnt) in enumerate(runs[1:], 1):
        assert cnt == counts, (SCHEDULES[schedule][i], cnt, counts)
        assert got.keys() == ref.keys()
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (SCHEDULES[schedule][i], k)
    # 3. a flagged candidate never moved the chain: accepted phi and nu proposals <= 40 - count
    cfg = H.config(__import__("importlib").import_module(PKG))
    for s, c in enumerate(counts):
        sm = ref[f"samples_{s}"]
        assert sm.shape == (H.N_BATCH * H.BATCH_LENGTH, 2 + 1 + 2)             # beta | K | phi | nu
        moves = 0
        for col, start in ((3, cfg.phi_starting[0]), (4, cfg.nu_starting[0])):
            moves += int(np.count_nonzero(np.diff(np.concatenate([[start], sm[:, col]]))))
        assert moves <= H.PROPOSALS - c, (s, moves, c)
    # 4. the tiled replay factors the kept states again and gives the fused run's kriging draws
    for tile in (64, 32):
        for s in range(len(H.SIZES)):
            assert np.array_equal(ref[f"tiled{tile}_pred_{s}"], ref[f"pred_{s}"]), (tile, s)
            assert np.array_equal(ref[f"tiled{tile}_wq_{s}"], ref[f"wq_{s}"]), (tile, s)
