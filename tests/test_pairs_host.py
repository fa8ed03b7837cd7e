"""CPU side of the cross-outcome outputs (include/mk.h: per test site and pair of outcomes the grids of
p_a p_b and p_a - p_b and the planes both_mean, both_sd, diff_mean, diff_sd, corr, a_gt_b, joint_j):
tests/pairs_ref.py, the restatement the GPU tests compare the device with, is pinned here against cases
worked by hand, and the binding is checked against the header."""
import ctypes
import os
import re
from math import sqrt

import numpy as np
import pytest

from oracle.rstats import PROBS200
from pairs_ref import BASE_NAMES, m2_ratio, names, pair_draws, pair_grids, pair_list, pair_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mk.h")


def test_pair_order():
    assert pair_list(2) == [(0, 1)]
    assert pair_list(3) == [(0, 1), (0, 2), (1, 2)]
    assert pair_list(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and pair_list(1) == []
    # q = 3, two sites, one state: column t q + h holds 10 t + h; pair columns are site-major
    p = np.array([[0.0], [1.0], [2.0], [10.0], [11.0], [12.0]])
    both, diff, pa, pb = pair_draws(p, 3)
    assert pa[0].tolist() == [0.0, 0.0, 1.0, 10.0, 10.0, 11.0] and pb[0].tolist() == [1.0, 2.0, 2.0, 11.0, 12.0, 12.0]
    assert both[0].tolist() == [0.0, 0.0, 2.0, 110.0, 120.0, 132.0] and diff[0].tolist() == [-1.0, -2.0, -1.0] * 2


def test_four_states_by_hand():
    """p_a = (.1, .2, .3, .4), p_b = (.8, .6, .4, .2) = 1 - 2 p_a: corr -1.
    both = (.08, .12, .12, .08): mean .1, deviations +-.02, sd = sqrt(4 (.02)^2 / 3).
    diff = (-.7, -.4, -.1, .2): mean -.25, deviations +-.45, +-.15, sd = sqrt(.45 / 3).
    p_a > p_b in the last state only.  Both above .25: state 3 only (p_a = .3, p_b = .4); above .4: p_a never
    is (strict); above .15: states 2, 3, 4."""
    p = np.array([[0.1, 0.2, 0.3, 0.4], [0.8, 0.6, 0.4, 0.2]])
    got = pair_planes(p, 2, (0.25, 0.4, 0.15))
    assert got.shape == (1, 9) and names(3) == BASE_NAMES + ["joint_1", "joint_2", "joint_3"]
    np.testing.assert_allclose(got[0, :4], [0.1, sqrt(0.0016 / 3), -0.25, sqrt(0.15)], rtol=1e-13)
    assert got[0, 4] == pytest.approx(-1.0, abs=1e-13)
    assert got[0, 5:].tolist() == [0.25, 0.25, 0.0, 0.75]
    # p_b = 2 p_a: corr +1, p_a never above p_b
    got = pair_planes(np.array([[0.1, 0.2, 0.3, 0.4], [0.2, 0.4, 0.6, 0.8]]), 2)
    assert got.shape == (1, 6) and got[0, 4] == pytest.approx(1.0, abs=1e-13) and got[0, 5] == 0.0
    # the grids: type 7 of four values at level .5 is the middle of the two central order statistics
    both, diff = pair_grids(p, 2)
    assert both.shape == diff.shape == (200, 1)
    k = int(np.argmin(np.abs(PROBS200 - 0.5)))
    assert both[k, 0] == pytest.approx(0.5 * (0.1 * 0.8 + 0.2 * 0.6)) and diff[k, 0] == pytest.approx(-0.25)
    assert both[-1, 0] == max(0.2 * 0.6, 0.3 * 0.4) and diff[-1, 0] == 0.4 - 0.2     # level 1: the largest draw


def test_constant_column_has_no_corr_and_one_state_no_sd():
    p = np.array([[0.3, 0.3, 0.3], [0.1, 0.5, 0.2]])
    got = pair_planes(p, 2, (0.15,))
    assert np.isnan(got[0, 4]) and np.isfinite(np.delete(got[0], 4)).all()
    assert got[0, 5] == 2.0 / 3.0 and got[0, 6] == 2.0 / 3.0
    assert m2_ratio(p)[0] < 1e-30 and m2_ratio(p)[1] > 1e-6
    got = pair_planes(np.array([[0.3], [0.1]]), 2, (0.05,))          # n = 1: no sd, no corr
    assert got[0, 0] == 0.3 * 0.1 and np.isnan(got[0, [1, 3, 4]]).all() and got[0, 5:].tolist() == [1.0, 1.0]
    # a NaN draw in outcome 1 of q = 3 poisons the pairs (0, 1) and (1, 2) of that site only
    p = np.full((6, 3), 0.5) + np.arange(18).reshape(6, 3) / 100.0
    p[4, 1] = np.nan
    got = pair_planes(p, 3, (0.5,))
    assert np.isnan(got[[3, 5]]).all() and np.isfinite(got[[0, 1, 2, 4]]).all()


def test_pair_structs_and_entry_points_match_header(mk):
    binding = __import__(mk.__name__ + "._lib", fromlist=["x"])
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for cname, py, want in (("mk_pair_spec", binding.PairSpec, ["n_thresholds", "thresholds"]),
                            ("mk_pairs", binding.Pairs, ["both_predict", "diff_predict", "planes", "combined_both",
                                                         "combined_diff"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        fields = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*;", body)
        assert fields == [f[0] for f in py._fields_] == want
    assert int(re.search(r"#define MK_N_PAIR_BASE (\d+)", src).group(1)) == binding.N_PAIR_BASE == len(BASE_NAMES)
    assert binding.PAIR_BASE_NAMES == BASE_NAMES
    lib = mk.load()
    for name, n in (("mk_session_set_pairs", 2), ("mk_session_pairs", 2), ("mk_meta_fit_pairs", 16), ("mk_meta_fit_maps", 14)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, flags=re.S)
        assert decl, name
        assert decl.group(1).count(",") + 1 == n == len(binding.EXPORTS[name][1]), name
        assert hasattr(lib, name)
    mp, pr = binding.EXPORTS["mk_meta_fit_maps"][1], binding.EXPORTS["mk_meta_fit_pairs"][1]
    assert pr[:len(mp)] == mp and len(pr) == len(mp) + 2        # mk_meta_fit_maps' arguments plus two
    assert mk.session.KS_PAIRS == 18 and mk.session.KS_MAPS == 17
    outbuf = __import__(mk.__name__ + ".outbuf", fromlist=["x"])
    assert outbuf.pair_list(3) == pair_list(3) and outbuf.pair_names(2) == names(2)
    pb = outbuf.PairBuffers(2, 3, 5, 1, combined=True)
    assert pb.both_predict.shape == pb.diff_predict.shape == (2, 15, 200) and pb.planes.shape == (2, 7, 15)
    assert pb.combined_both.shape == (15, 200)
    got = pb.unpack((0.2,))
    assert got["pairs"] == pair_list(3) and got["subsets"][1].shape == (15, 7) and got["both_predict"][0].shape == (200, 15)
    assert got["combined_diff"].shape == (200, 15) and got["thresholds"] == [0.2]


def _tiny(mk, q):
    d = mk.synthetic.generate(20, q=q, n_test=2, seed=1)
    p = d["x"].shape[1]
    cfg = mk.SamplerConfig(q, p, np.zeros(p), np.full(p, 0.1), n_batch=1, batch_length=2, burn_in=1)
    return d, cfg, dict(coords=d["coords"], y=d["y"], weights=np.ones(20 * q), x=d["x"])


def test_pairs_fail_loudly_without_gpu(mk):
    """Null handles are argument errors anywhere; so are q = 1, a NaN threshold and nine thresholds, before
    any device is looked for.  Without a device the session route raises MkError and leaves no session."""
    lib = mk.load()
    binding = __import__(mk.__name__ + "._lib", fromlist=["x"])
    sp, pr = binding.PairSpec(), binding.Pairs()
    assert lib.mk_session_set_pairs(None, ctypes.byref(sp)) == binding.MK_E_ARG
    assert lib.mk_session_set_pairs(None, None) == binding.MK_E_ARG
    assert lib.mk_session_pairs(None, ctypes.byref(pr)) == binding.MK_E_ARG
    d, cfg, sub = _tiny(mk, 2)
    for bad, what in (((0.2, np.nan), "threshold 1 "), ((np.inf,), "threshold 0 "), (np.linspace(0.1, 0.9, 9), "n_thresholds = 9")):
        with pytest.raises(mk.MkError) as e:
            mk.meta_fit_node([sub], cfg, coords_test=d["coords_test"], x_test=d["x_test"], devices=[0], pairs=bad)
        assert e.value.code == binding.MK_E_ARG and what in str(e.value)
    with pytest.raises(ValueError):
        mk.meta_fit_node([sub], cfg, coords_test=d["coords_test"], devices=[0], pairs=(0.5,))     # no x_test
    d1, cfg1, sub1 = _tiny(mk, 1)
    with pytest.raises(mk.MkError) as e:
        mk.meta_fit_node([sub1], cfg1, coords_test=d1["coords_test"], x_test=d1["x_test"], devices=[0], pairs=(0.5,))
    assert e.value.code == binding.MK_E_ARG and "q >= 2" in str(e.value)
    if lib.mk_device_count() == 0:
        with pytest.raises(mk.MkError):
            with mk.Session([sub], cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
                ses.set_pairs((0.5,))
                ses.pairs()
        assert lib.mk_session_count() == 0
        with pytest.raises(mk.MkError) as e:
            mk.meta_fit_node([sub], cfg, coords_test=d["coords_test"], x_test=d["x_test"], devices=[0], pairs=(0.5,))
        assert e.value.code == binding.MK_E_NODEV
