"""CPU side of the posterior maps (include/mk.h: mean, sd and exceedance probabilities of w and of
p(y = 1) per test column): tests/maps_ref.py, the restatement the GPU tests compare the device with, is
pinned here against cases worked by hand, and the binding is checked against the header."""
import ctypes
import os
import re
from math import log, sqrt

import numpy as np
import pytest

from maps_ref import BASE_NAMES, map_ref, map_ref_grid, map_ref_p, names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mk.h")


def test_one_state_has_no_sd():
    """n = 1: the mean is the value, the sd NaN (M2 / 0), exceedance 0 or 1."""
    got = map_ref_grid(np.array([[0.3, 0.7]]), (0.5,))
    assert got.shape == (2, 3)
    assert got[:, 0].tolist() == [0.3, 0.7] and np.isnan(got[:, 1]).all() and got[:, 2].tolist() == [0.0, 1.0]


def test_two_states_by_hand():
    """Values (1, 3).  Sum 4, mean 2.  Welford: k = 1: d = 1, m = 1, M2 = 1 (1 - 1) = 0; k = 2: d = 2,
    m = 1 + 2/2 = 2, M2 = 0 + 2 (3 - 2) = 2; sd = sqrt(2 / 1).  Against u = 1 only the 3 counts (strict): 1/2;
    against u = 3 nothing; against u = 0 both."""
    got = map_ref_grid(np.array([[1.0], [3.0]]), (1.0, 3.0, 0.0))
    np.testing.assert_allclose(got[0], [2.0, sqrt(2.0), 0.5, 0.0, 1.0], rtol=1e-15)
    # three states (2, 4, 9): mean 5, squared deviations 9 + 1 + 16 = 26, sd = sqrt(13)
    got = map_ref_grid(np.array([[2.0], [4.0], [9.0]]))
    np.testing.assert_allclose(got[0], [5.0, sqrt(13.0)], rtol=1e-15)


def test_constant_column_and_value_at_a_threshold():
    """A constant column has sd exactly 0 (every d after the first state is 0); a value equal to a threshold
    is not counted."""
    g = np.full((7, 2), 0.2)
    g[:, 1] = [0.1, 0.2, 0.2, 0.3, 0.2, 0.5, 0.2]
    got = map_ref_grid(g, (0.2,))
    assert got[0, 0] == pytest.approx(0.2, rel=1e-15) and got[0, 1] == 0.0 and got[0, 2] == 0.0
    assert got[1, 2] == 2.0 / 7.0                                  # 0.3 and 0.5 only


def test_nan_draw_makes_a_nan_column():
    g = np.array([[0.1, 0.2, 0.3], [0.4, np.nan, 0.6], [0.7, 0.8, 0.9]])
    got = map_ref_grid(g, (0.5, 0.25))
    assert np.isnan(got[1]).all() and np.isfinite(got[[0, 2]]).all()
    got = map_ref_grid(np.array([[0.1, np.inf]]), (0.5,))          # an infinite level too, and with one state
    assert np.isnan(got[1]).all() and got[0, 0] == 0.1


def test_the_sample_route_by_hand():
    """logit with x = 1, beta = (-ln 3, ln 3) over two states (`first` picks them) and draws w = (0, 0):
    p = (1/4, 3/4), p_mean 1/2, p_sd = sqrt(2 (1/4)^2), one of the two states exceeds 0.5; w_mean 0, w_sd 0.
    Draws (2, 4): w_mean 3, w_sd sqrt(2), eta > 0 in both states.  A NaN draw makes its column NaN."""
    l3 = log(3.0)
    samples = np.array([[9.0, 1.0, 6.0], [-l3, 1.0, 6.0], [l3, 1.0, 6.0]])
    x = np.ones((2, 1))
    w = np.zeros((2, 2))                                          # C x n
    got = map_ref(samples, w, x, 1, "logit", (0.5,), first=2)
    assert got.shape == (2, 5) and names(1) == BASE_NAMES + ["exc_1"]
    np.testing.assert_allclose(got[0], [0.0, 0.0, 0.5, sqrt(0.125), 0.5], rtol=1e-14, atol=1e-16)
    np.testing.assert_allclose(map_ref_p(samples, w, x, 1, "logit", first=2)[:, 0], [0.25, 0.75], rtol=1e-14)
    w2 = np.array([[2.0, 4.0], [0.0, np.nan]])
    got = map_ref(samples, w2, x, 1, "logit", (0.5,), first=2)
    np.testing.assert_allclose(got[0, :2], [3.0, sqrt(2.0)], rtol=1e-15)
    assert got[0, 4] == 1.0 and np.isnan(got[1]).all()             # eta = (2 - ln 3, 4 + ln 3) > 0 twice
    # probit at eta = 0: p = 1/2 in every state, sd 0
    got = map_ref(np.zeros((3, 3)), np.zeros((1, 3)), np.ones((1, 1)), 1, "probit", (0.5, 0.4))
    assert got[0].tolist() == [0.0, 0.0, 0.5, 0.0, 0.0, 1.0]


def test_maps_structs_and_entry_points_match_header(mk):
    binding = __import__(mk.__name__ + "._lib", fromlist=["x"])
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for cname, py, want in (("mk_map_spec", binding.MapSpec, ["thresholds", "n_thresholds"]),
                            ("mk_maps", binding.Maps, ["subsets", "combined"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, flags=re.S).group(1)
        fields = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*;", body)
        assert fields == [f[0] for f in py._fields_] == want
    assert int(re.search(r"#define MK_MAP_MAXT (\d+)", src).group(1)) == binding.MAP_MAXT == 8
    assert int(re.search(r"#define MK_N_MAP_BASE (\d+)", src).group(1)) == binding.N_MAP_BASE == len(binding.MAP_BASE_NAMES)
    assert binding.MAP_BASE_NAMES == BASE_NAMES
    lib = mk.load()
    for name, n in (("mk_session_set_maps", 2), ("mk_session_maps", 2), ("mk_map_grid", 7), ("mk_meta_fit_maps", 14),
                    ("mk_meta_fit_val", 12)):
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, flags=re.S)
        assert decl, name
        assert decl.group(1).count(",") + 1 == n == len(binding.EXPORTS[name][1]), name
        assert hasattr(lib, name)
    val, mp = binding.EXPORTS["mk_meta_fit_val"][1], binding.EXPORTS["mk_meta_fit_maps"][1]
    assert mp[:len(val)] == val and len(mp) == len(val) + 2     # mk_meta_fit_val's arguments plus two
    assert mk.session.KS_MAPS == 17


def test_maps_fail_loudly_without_gpu(mk):
    """Null handles are argument errors anywhere; so are a NaN threshold and nine thresholds, naming the
    index, before any device is touched.  Without a device the session route raises MkError and leaves no
    session."""
    lib = mk.load()
    binding = __import__(mk.__name__ + "._lib", fromlist=["x"])
    sp, mp = binding.MapSpec(), binding.Maps()
    assert lib.mk_session_set_maps(None, ctypes.byref(sp)) == binding.MK_E_ARG
    assert lib.mk_session_set_maps(None, None) == binding.MK_E_ARG
    assert lib.mk_session_maps(None, ctypes.byref(mp)) == binding.MK_E_ARG
    assert lib.mk_map_grid(None, 1, 1, None, 0, None, 0) == binding.MK_E_ARG
    g = np.full((2, 3), 0.5)
    with pytest.raises(mk.MkError) as e:
        mk.map_grid(g, (0.2, 0.5, np.nan))
    assert e.value.code == binding.MK_E_ARG and "threshold 2 " in str(e.value)
    with pytest.raises(mk.MkError) as e:
        mk.map_grid(g, (np.inf,))
    assert e.value.code == binding.MK_E_ARG and "threshold 0 " in str(e.value)
    with pytest.raises(mk.MkError) as e:
        mk.map_grid(g, np.linspace(0.1, 0.9, 9))
    assert e.value.code == binding.MK_E_ARG and "n_thresholds = 9" in str(e.value)
    with pytest.raises(ValueError):
        mk.map_grid(np.zeros(3))
    d = mk.synthetic.generate(20, q=1, n_test=2, seed=1)
    cfg = mk.SamplerConfig(1, 2, [0, 0], [0.1, 0.1], n_batch=1, batch_length=2, burn_in=1)
    sub = dict(coords=d["coords"], y=d["y"], weights=np.ones(20), x=d["x"])
    for bad, what in (((0.2, np.nan), "threshold 1 "), (np.linspace(0.1, 0.9, 9), "n_thresholds = 9")):
        with pytest.raises(mk.MkError) as e:       # the node call checks them before it looks for a device
            mk.meta_fit_node([sub], cfg, coords_test=d["coords_test"], x_test=d["x_test"], devices=[0], maps=bad)
        assert e.value.code == binding.MK_E_ARG and what in str(e.value)
    with pytest.raises(ValueError):
        mk.meta_fit_node([sub], cfg, coords_test=d["coords_test"], devices=[0], maps=(0.5,))      # no x_test
    if lib.mk_device_count() == 0:
        with pytest.raises(mk.MkError):
            with mk.Session([sub], cfg, coords_test=d["coords_test"], x_test=d["x_test"]) as ses:
                ses.set_maps((0.5,))
                ses.maps()
        assert lib.mk_session_count() == 0
        with pytest.raises(mk.MkError):
            mk.map_grid(g, (0.5,))
        with pytest.raises(mk.MkError) as e:
            mk.meta_fit_node([sub], cfg, coords_test=d["coords_test"], x_test=d["x_test"], devices=[0], maps=(0.5,))
        assert e.value.code == binding.MK_E_NODEV
