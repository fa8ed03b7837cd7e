"""Checkpoints (include/mk.h "checkpoints"; csrc/mk_checkpoint.hip): a chain stopped after c iterations, written to a
file, read by a fresh session and continued reports the bytes of the chain that never stopped.

A is the uninterrupted session.  B1 runs c iterations and writes the file (fitfile.save_checkpoint), B2 is made by
fitfile.load_checkpoint and runs the rest.  "Equal" is tobytes() equality of everything _collect() gathers:
samples, w_samples, w_pred_samples, acceptance, the parameter, w_predict and p_predict grids, chain_state(i) of
every subset, notpd_counts() and digest().  No tolerance appears in this file.

Chains: 4 batches x 10 iterations, burn_in = 21 (kept states from iteration 20 on), the geometries of
tests/krig_ref.py, tile 256 under its 261 test sites where tiled."""
import os
import subprocess
import sys

import numpy as np
import pytest

import krig_ref as kr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WIN = dict(n_batch=4, batch_length=10, burn_in=21)
N = 40
SEED, BASE, TILE = 12, 2, 256
_A = {}
_pb = {}


def _problem(case):
    if case not in _pb:
        pb = kr.problem(case)
        q = kr.CASES[case]["q"]
        pb["x_test"] = np.random.default_rng(77).standard_normal((q * pb["coords_test"].shape[0], 2 * q))
        _pb[case] = pb
    return _pb[case]


def _cfg(mk, case, tile=0, n_streams=0):
    c = kr.CASES[case]
    q = c["q"]
    return mk.SamplerConfig(q, 2 * q, np.zeros(2 * q), np.full(2 * q, 0.05), cov_model=c["model"], seed=SEED, predict_tile=tile,
                            n_streams=n_streams, **WIN)


def _session(mk, case, tile=0, criteria=False, lookahead=None, n_streams=0):
    pb = _problem(case)
    return mk.Session(pb["subsets"], _cfg(mk, case, tile, n_streams), coords_test=pb["coords_test"], x_test=pb["x_test"],
                      subset_base=BASE, record_w=True, criteria=criteria, lookahead=lookahead)


def _collect(ses, criteria=False):
    """Everything "equal" compares, name -> array."""
    out = ses.outputs(samples=True, w_samples=True, w_pred_samples=True, acceptance=True)
    assert {"parameters", "w_predict", "p_predict", "samples", "w_samples", "w_pred_samples", "acceptance"} <= set(out)
    got = {}
    for k, v in out.items():
        for i, a in enumerate(v if isinstance(v, (list, tuple)) else [v]):
            got[f"{k}[{i}]"] = np.asarray(a)
    for i in range(ses.S):
        st = ses.chain_state(i)
        for k in ("beta", "theta", "w", "tune", "accept"):
            got[f"chain_state[{i}].{k}"] = st[k]
    got["notpd"] = ses.notpd_counts()
    got["digest"] = ses.digest()
    if criteria:
        cr = ses.criteria(pointwise=True)
        got["criteria.subsets"], got["criteria.total"] = np.asarray(cr["subsets"]), np.asarray(cr["total"])
        for i, a in enumerate(cr["pointwise"]):
            got[f"criteria.pointwise[{i}]"] = np.asarray(a)
    return got


def _uninterrupted(mk, monkeypatch, case, tile=0, cheb="0", criteria=False, lookahead=None, n_streams=0):
    """Session A of a configuration: run once, shared, left unchanged."""
    key = (case, tile, cheb, criteria, lookahead, n_streams)
    if key not in _A:
        monkeypatch.setenv("MK_KRIG_CHEB", cheb)
        with _session(mk, case, tile, criteria, lookahead, n_streams) as ses:
            ses.run(N)
            _A[key] = _collect(ses, criteria)
    return _A[key]


def _write(mk, path, c, case, tile=0, criteria=False, lookahead=None, n_streams=0):
    """B1: c iterations, then the file."""
    with _session(mk, case, tile, criteria, lookahead, n_streams) as ses:
        if c:
            ses.run(c)
        assert ses.iteration == c
        mk.fitfile.save_checkpoint(ses, path)


def _continue(mk, path, criteria=False, **kw):
    """B2: a fresh session from the file, the rest of the chain, everything it reports."""
    with mk.fitfile.load_checkpoint(path, **kw) as ses:
        c = ses.iteration
        if c < N:
            ses.run(N - c)
        return _collect(ses, criteria)


def _same(a, b, what):
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    bad = [k for k in sorted(a) if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    assert not bad, f"{what}: {len(bad)} of {len(a)} differ: {bad[:8]}"


# ---------------------------------------------------------------- 1. every cut point
@pytest.mark.parametrize("c", [0, 15, 20, 25, 40])
def test_cut_anywhere_equals_uninterrupted(mk, monkeypatch, tmp_path, c):
    """E1, fused, the exact refresh: 15 is mid-batch after one adaptation (accept counts non-zero), 20 the batch end
    on the eve of the kept window, 25 inside it (the draws half filled), 0 and 40 the ends.  At 40 no iteration is
    run and the outputs are served from the restored record."""
    a = _uninterrupted(mk, monkeypatch, "E1")
    path = str(tmp_path / "shard.npz")
    _write(mk, path, c, "E1")
    _same(a, _continue(mk, path), f"cut at {c}")


# ---------------------------------------------------------------- 2. every kind of session, cut inside the kept window
KINDS = {
    "E1-fused-tables": ("E1", 0, "-1", False),
    "E1-tiled-exact": ("E1", TILE, "0", False),
    "E1-tiled-interpolated": ("E1", TILE, "-1", False),
    "L1-fused": ("L1", 0, "0", False),
    "L1-tiled": ("L1", TILE, "-1", False),
    "M1-fused": ("M1", 0, "0", False),
    "M1-tiled": ("M1", TILE, "0", False),
    "E1-criteria": ("E1", 0, "0", True),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_session_kind_at_25(mk, monkeypatch, tmp_path, kind):
    case, tile, cheb, crit = KINDS[kind]
    a = _uninterrupted(mk, monkeypatch, case, tile, cheb, crit)
    path = str(tmp_path / "shard.npz")
    _write(mk, path, 25, case, tile, crit)
    _same(a, _continue(mk, path, crit), kind)


def test_second_half_in_a_fresh_process(mk, monkeypatch, tmp_path):
    """The file written here, the rest of the chain in a child process that has seen nothing else."""
    a = _uninterrupted(mk, monkeypatch, "E1")
    path, res = str(tmp_path / "shard.npz"), str(tmp_path / "child.npz")
    _write(mk, path, 25, "E1")
    env = dict(os.environ, MK_KRIG_CHEB="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gpu_checkpoint_run.py"), path, res, str(N)], capture_output=True,
                       text=True, timeout=100, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    with np.load(res, allow_pickle=False) as z:
        b = {k: z[k] for k in z.files}
    _same(a, b, "child process")


# ---------------------------------------------------------------- 3. the schedule
@pytest.mark.parametrize("wrote,reads", [(1, 0), (0, 1)])
def test_written_under_one_schedule_continued_under_the_other(mk, monkeypatch, tmp_path, wrote, reads):
    """Written under lookahead = `wrote`, read by a session made with lookahead = `reads`, equal to A (the
    uninterrupted chain of the schedule that wrote the file).

    The two schedules make the same decisions and round z differently (the lookahead schedule takes z' of an
    accepted candidate from a forward solve, k_border_step, the sequential one from the bordered factor row:
    tests/test_gpu_sampler.py test_lookahead_equals_sequential_schedule holds them to 1e-10), so
    the schedule belongs to what fixes the chain's bytes, and "the schedule is fixed once the chain has started"
    (mk_session_set_lookahead) holds for a restored chain: the restore puts the session on the schedule that wrote
    the state, whatever it was made with -- Session.lookahead says so -- and the chain it continues is A's."""
    a = _uninterrupted(mk, monkeypatch, "E1", lookahead=wrote)
    path = str(tmp_path / "shard.npz")
    _write(mk, path, 25, "E1", lookahead=wrote)
    _same(a, _continue(mk, path, lookahead=reads), f"lookahead {wrote} -> {reads}")
    with mk.fitfile.load_checkpoint(path, lookahead=reads) as ses:
        assert ses.lookahead == bool(wrote) and ses.iteration == 25
        with pytest.raises(mk.MkError, match="fixed once the chain has started"):
            ses.set_lookahead(reads)


@pytest.mark.parametrize("c", [0, 40])
def test_the_ends_keep_the_readers_schedule(mk, monkeypatch, tmp_path, c):
    """At iteration 0 the reader's schedule runs the whole chain, at n.samples none of it: the session stays as it
    was made, and equals the uninterrupted chain of the schedule that ran the iterations."""
    path = str(tmp_path / "shard.npz")
    _write(mk, path, c, "E1", lookahead=1)
    _same(_uninterrupted(mk, monkeypatch, "E1", lookahead=0 if c == 0 else 1), _continue(mk, path, lookahead=0), f"ends, {c}")
    with mk.fitfile.load_checkpoint(path, lookahead=0) as ses:
        assert not ses.lookahead


def test_a_lookahead_state_is_refused_by_several_stream_groups(mk, monkeypatch, tmp_path):
    """Several stream groups run the sequential schedule alone: a state written mid-chain under the lookahead
    schedule would continue there as another chain (to rounding), so it is refused by name; the ends are not."""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    path = str(tmp_path / "shard.npz")
    _write(mk, path, 25, "E1", lookahead=1)
    with pytest.raises(mk.MkError, match=r"written mid-chain \(iteration 25\) under the lookahead schedule.*n_streams <= 1"):
        mk.fitfile.load_checkpoint(path, n_streams=2)
    with mk.fitfile.load_checkpoint(path) as ses:
        assert ses.lookahead and ses.iteration == 25
    _write(mk, path, 0, "E1", lookahead=1)
    with mk.fitfile.load_checkpoint(path, n_streams=2) as ses:
        assert not ses.lookahead and ses.iteration == 0


def test_written_on_one_stream_group_continued_on_two(mk, monkeypatch, tmp_path):
    """n_streams = 1 to n_streams = 2, both on the sequential schedule (several stream groups have no other)."""
    a = _uninterrupted(mk, monkeypatch, "E1", lookahead=0, n_streams=1)
    path = str(tmp_path / "shard.npz")
    _write(mk, path, 25, "E1", lookahead=0, n_streams=1)
    _same(a, _continue(mk, path, n_streams=2), "n_streams 1 -> 2")


# ---------------------------------------------------------------- 4. a range of the subsets
def test_subset_range_continues_alone(mk, monkeypatch, tmp_path):
    a = _uninterrupted(mk, monkeypatch, "E1")
    path = str(tmp_path / "shard.npz")
    _write(mk, path, 25, "E1")
    b = _continue(mk, path, subsets=(1, 2))
    want = {}
    for k, v in a.items():
        if k in ("notpd", "digest"):
            want[k] = v[1:3]
        elif "[" in k:
            i = int(k[k.index("[") + 1:k.index("]")])
            if i in (1, 2):
                want[k.replace(f"[{i}]", f"[{i - 1}]")] = v
    _same(want, b, "subsets (1, 2)")


# ---------------------------------------------------------------- 5. two checkpoints in a row
def test_two_checkpoints_in_a_row(mk, monkeypatch, tmp_path):
    a = _uninterrupted(mk, monkeypatch, "E1")
    p15, p25, own = (str(tmp_path / n) for n in ("c15.npz", "c25.npz", "own25.npz"))
    _write(mk, p15, 15, "E1")
    with mk.fitfile.load_checkpoint(p15) as ses:
        ses.run(10)
        mk.fitfile.save_checkpoint(ses, p25)
    _same(a, _continue(mk, p25), "15, then 25")
    _write(mk, own, 25, "E1")
    with np.load(p25, allow_pickle=False) as z, np.load(own, allow_pickle=False) as w:
        assert set(z.files) == set(w.files)
        bad = [k for k in z.files if z[k].dtype != w[k].dtype or z[k].shape != w[k].shape or z[k].tobytes() != w[k].tobytes()]
    assert not bad, bad


# ---------------------------------------------------------------- 6. a state that is not the chain's
def test_altered_theta_is_caught_by_the_digest(mk, monkeypatch, tmp_path):
    """theta of subset 1 moved in the file (logit phi + 0.3: phi stays inside its support, every host check
    passes).  The factors re-derived from it are not the ones the file's digests were taken of: the restore is
    refused naming the pair and the buffer L, the session is unusable, and nothing has run.  (No device fault is
    involved: two integers are compared on the host.)"""
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    path = str(tmp_path / "shard.npz")
    _write(mk, path, 25, "E1")
    ff = mk.fitfile
    a = ff.read_checkpoint(path)
    a["state_theta"] = a["state_theta"].copy()
    a["state_theta"][1, 1] += 0.3                      # q = 1: theta = log A | logit phi
    cfg = ff.config_from(a)
    state = {k[len("state_"):]: v for k, v in a.items() if k.startswith("state_")}
    state.update(iteration=a["iteration"], words=a["words"], digests=a["digests"], lookahead=a["lookahead"])
    with mk.Session(ff.subsets_of(a), cfg, coords_test=a["coords_test"], x_test=a["x_test"], subset_base=BASE, record_w=True,
                    lookahead=bool(a["lookahead"])) as ses:
        with pytest.raises(mk.MkError, match=rf"subset {BASE + 1}, outcome 0, buffer L\b"):
            ses.restore(state)
        assert ses.iteration == 0
        with pytest.raises(mk.MkError, match="unusable"):
            ses.run(1)
        with pytest.raises(mk.MkError, match="unusable"):
            ses.checkpoint()


# ---------------------------------------------------------------- 7. the launches' own timing
def test_checkpoint_launches_are_counted(mk, monkeypatch):
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    with _session(mk, "E1") as ses:
        ses.run(3)
        assert ses.kernel_stats(mk.session.KS_CKPT)["launches"] == 0
        st = ses.checkpoint()
        ks = ses.kernel_stats(mk.session.KS_CKPT)
        assert ks["launches"] > 0 and ks["ms"] > 0.0
        assert st["digests"].shape == (4, 4) and int(st["iteration"]) == 3
    with _session(mk, "E1") as ses:
        ses.restore(st)
        assert ses.iteration == 3 and ses.kernel_stats(mk.session.KS_CKPT)["launches"] > 0
        rs = ses.restore_stats()
        assert rs["ms_derive"] > 0.0 and rs["ms_digest"] > 0.0
        with pytest.raises(mk.MkError, match="restored before"):
            ses.restore(st)


def test_refusals_name_what_is_wrong(mk, monkeypatch):
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    with _session(mk, "E1") as ses:
        ses.run(3)
        st = ses.checkpoint()
        with pytest.raises(mk.MkError, match="has run 3 iterations"):
            ses.restore(st)
    with _session(mk, "E1") as ses:
        bad = dict(st, iteration=np.array(41))
        with pytest.raises(mk.MkError, match="iteration 41 is outside 0 .. n.samples = 40"):
            ses.restore(bad)
        bad = dict(st, iteration=np.array(4))
        with pytest.raises(mk.MkError, match="field 'samples' has 12 words per subset.* has 16"):
            ses.restore(bad)
        th = st["theta"].copy()
        th[2, 1] = np.nan
        with pytest.raises(mk.MkError, match=rf"subset {BASE + 2}, field 'theta', word 1 is nan"):
            ses.restore(dict(st, theta=th))
        ac = st["acc"].copy()
        ac[0, 5] = 0.5
        with pytest.raises(mk.MkError, match=rf"subset {BASE}, field 'acc', word 5 is 0.5"):
            ses.restore(dict(st, acc=ac))
        assert ses.iteration == 0
        ses.restore(st)                                  # the refusals left the session as created
        assert ses.iteration == 3
