"""The four result sinks of a tiled session -- chain diagnostics, held-out scores, posterior maps and
cross-outcome pairs -- attached at the same time to one kriging replay: each fills what it fills alone, each
prices its own launches, and set_test_sites detaches them all.  What the sinks compute is checked sink by
sink (test_gpu_diagnostics.py, test_gpu_scores.py, test_gpu_maps.py, test_gpu_pairs.py); this test pins what
they share: the per-tile list in the replay, the window / tile bookkeeping and the launch counts.

Shape: q = 2, subsets of 40 and 70 sites, 24 test sites with covariates in tiles of 16 (the last ragged: 8),
32 iterations (n_batch 4 x batch_length 8), burn_in 9: 24 kept states, then the kept window (12, 30): 19 --
neither a power of two, so the pair sort pads.  Exact kriging (MK_KRIG_CHEB=0), as in the per-sink tests.
Every comparison is bit equality (NaNs in the same places): the same chain, the same draws, and a column is
one thread's or one workgroup's work whatever else was attached."""
import numpy as np
import pytest

from test_gpu_pairs import _problem

pytestmark = pytest.mark.gpu
KS_DIAG, KS_SCORE, KS_MAPS, KS_PAIRS = 14, 16, 17, 18
N_TILES = 2                                                          # 24 sites in tiles of 16
MAP_THR, PAIR_THR = (0.3, 0.6), (0.5,)
WINDOW = (12, 30)


def _equal(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _equal(a[k], b[k], f"{what}[{k}]")
    elif isinstance(a, (list, tuple)) and len(a) and isinstance(a[0], np.ndarray):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, f"{what}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), what
    else:
        assert a == b, what


def _diag(out):
    return {k: v for k, v in out.items() if k.endswith("_diag") or k.endswith("_diag_worst")}


def _session(mk, d, subs):
    cfg = mk.SamplerConfig(2, 4, beta_starting=np.zeros(4), beta_tuning=np.full(4, 0.05), n_batch=4, batch_length=8,
                           burn_in=9, seed=9, predict_tile=16)
    return mk.Session(subs, cfg, coords_test=d["coords_test"], x_test=d["x_test"])


def _stats(ses):
    return {k: ses.kernel_stats(k)["launches"] for k in (KS_DIAG, KS_SCORE, KS_MAPS, KS_PAIRS)}


def _alone(ses, d):
    """Each sink attached on its own to a replay of the current kept window."""
    got = {"diag": _diag(ses.outputs(diagnostics=True))}
    ses.set_validation(d["y_test"])
    ses.outputs(quantiles=False, w_predict_sum=True)
    got["scores"] = ses.scores(pointwise=True)
    ses.set_validation(None)
    ses.set_maps(MAP_THR)
    ses.outputs(quantiles=False, w_predict_sum=True)
    got["maps"] = ses.maps()
    ses.set_maps(None)
    ses.set_pairs(PAIR_THR)
    ses.outputs(quantiles=False, w_predict_sum=True)
    got["pairs"] = ses.pairs()
    ses.set_pairs(None)
    return got


def _together(ses):
    """One replay of the current kept window with the sinks that are attached, and the diagnostics sink."""
    got = {"diag": _diag(ses.outputs(diagnostics=True))}
    got["scores"] = ses.scores(pointwise=True)
    got["maps"] = ses.maps()
    got["pairs"] = ses.pairs()
    return got


def test_sinks_together_equal_alone_and_price_their_own(mk, monkeypatch):
    monkeypatch.setenv("MK_KRIG_CHEB", "0")
    d, subs = _problem(mk, [40, 70], 2)
    with _session(mk, d, subs) as ses:
        ses.run(32)
        assert ses.predict_tile == 16
        alone = _alone(ses, d)
        ses.set_kept_window(*WINDOW)
        alone_win = _alone(ses, d)
    with _session(mk, d, subs) as ses:
        ses.run(32)
        ses.set_validation(d["y_test"])
        ses.set_maps(MAP_THR)
        ses.set_pairs(PAIR_THR)
        assert _stats(ses) == {KS_DIAG: 0, KS_SCORE: 0, KS_MAPS: 0, KS_PAIRS: 0}     # attached: nothing launched yet
        both = _together(ses)
        first = _stats(ses)
        ses.set_kept_window(*WINDOW)
        for results in (ses.scores, ses.maps, ses.pairs):                              # another window's tiles
            with pytest.raises(mk.MkError) as e:
                results()
            assert e.value.code == mk._lib.MK_E_ARG and "tile 0 (test sites 0 .. 15)" in str(e.value)
        both_win = _together(ses)
        second = _stats(ses)
        ses.set_test_sites(d["coords_test"], x_test=d["x_test"])
        for results, setter in ((ses.scores, "mk_session_set_validation"), (ses.maps, "mk_session_set_maps"),
                                (ses.pairs, "mk_session_set_pairs")):
            with pytest.raises(mk.MkError) as e:
                results()
            assert e.value.code == mk._lib.MK_E_ARG and setter in str(e.value)
        ses.outputs(quantiles=False, w_predict_sum=True)                               # detached: nothing more launched
        assert _stats(ses) == second
    # (a) what every sink fills beside the others is what it fills alone
    assert set(both["diag"]) >= {"w_predict_diag", "w_predict_diag_worst", "p_predict_diag", "p_predict_diag_worst"}
    assert both["scores"]["pointwise"][0].shape == (48, 2) and both["maps"]["subsets"][0].shape == (48, 4 + len(MAP_THR))
    assert both["pairs"]["both_predict"][0].shape == (200, 24) and both["pairs"]["subsets"][0].shape == (24, 6 + len(PAIR_THR))
    for k in ("diag", "scores", "maps", "pairs"):
        _equal(both[k], alone[k], k)
        _equal(both_win[k], alone_win[k], k + ", kept window")
    assert not np.array_equal(both["maps"]["subsets"][0], both_win["maps"]["subsets"][0], equal_nan=True)
    # (b) launches per replay: diag_to_host once per tile for w and once for p, and once for the parameters;
    # k_score_cols per tile and k_score_finish per scores(); k_map_cols per tile; both pair kernels per tile
    per_replay = {KS_DIAG: 2 * N_TILES + 1, KS_SCORE: N_TILES + 1, KS_MAPS: N_TILES, KS_PAIRS: 2 * N_TILES}
    assert first == per_replay
    assert second == {k: 2 * v for k, v in per_replay.items()}
