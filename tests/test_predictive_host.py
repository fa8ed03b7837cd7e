"""Host side of the predictive probabilities (spPredict's p.y.predictive.samples, MK.R:87's x.test):
the covariates reach mk_problem only in the (q n_test) x p shape, and the C ABI, its ctypes mirror
and the R glue name the same entry points and fields.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def _subsets(mk, q, n_test):
    d = mk.synthetic.generate(40, q=q, n_test=n_test, seed=6)
    p = 2 * q
    cfg = mk.SamplerConfig(q, p, np.zeros(p), np.full(p, 0.05), n_batch=1, batch_length=2)
    sub = dict(coords=d["coords"], y=d["y"], weights=np.ones(40 * q), x=d["x"])
    return d, cfg, [sub]


@pytest.mark.parametrize("q", [1, 2])
def test_packed_problem_carries_x_test_only_in_its_shape(mk, q):
    from importlib import import_module
    ses = import_module(mk.__name__ + ".session")
    d, cfg, subs = _subsets(mk, q, 7)
    xt = d["x_test"]
    assert xt.shape == (q * 7, 2 * q)
    pp = ses.PackedProblem(subs, cfg, d["coords_test"], x_test=xt)
    assert bool(pp.c.x_test)
    # column-major, location-major rows: element (row r, column j) at j * (q n_test) + r
    got = np.ctypeslib.as_array(pp.c.x_test, shape=(xt.size,))
    assert np.array_equal(got, xt.ravel(order="F"))
    assert not bool(ses.PackedProblem(subs, cfg, d["coords_test"]).c.x_test)
    for bad in (xt[:-1], xt[:, :1], xt.T, xt.ravel(), np.vstack([xt, xt])):
        with pytest.raises(ValueError):
            ses.PackedProblem(subs, cfg, d["coords_test"], x_test=bad)
    with pytest.raises(ValueError):      # covariates without test sites
        ses.PackedProblem(subs, cfg, None, x_test=xt)


def test_struct_mirrors_keep_the_header_order(mk):
    """New fields are appended: a host built against the earlier header still lays the structs out."""
    h = _read("include", "mk.h")

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), h, re.S).group(1)
        return re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))

    lib = mk._lib
    for cname, cls in (("mk_problem", lib.Problem), ("mk_outputs", lib.Outputs), ("mk_combined", lib.Combined)):
        assert fields(cname) == [f for f, _ in cls._fields_], cname
    assert fields("mk_problem")[-1] == "x_test"
    assert fields("mk_outputs")[-3:] == ["p_predict", "p_pred_samples", "p_predict_sum"]
    assert fields("mk_combined")[-1] == "result3"


def test_header_exports_and_glue_name_the_new_entry_points(mk):
    h, c, r = _read("include", "mk.h"), _read("mkgpu", "src", "mk_r.c"), _read("mkgpu", "R", "mkgpu.R")
    assert re.search(r"int mk_session_set_test_covars\(mk_session\* s, const double\* x_test\);", h)
    assert re.search(r"int mk_session_tile_grids_wp\(mk_session\* s, int32_t t0, double\* out_w, double\* out_p, "
                     r"int32_t device_out\);", h)
    ex = mk._lib.EXPORTS
    assert ex["mk_session_set_test_covars"][1] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    assert len(ex["mk_session_tile_grids_wp"][1]) == 5
    assert "mk_session_set_test_covars(" in c
    assert "p.y.predictive.samples" in r
    # mk_spPredict hands pred.covars to the glue, mk_meta_fit hands x.test on and returns result3
    call = r[r.index('.Call("mk_r_sppredict"'):]
    assert "pred.covars" in call[:call.index(")\n")]
    assert "x.test = NULL" in re.search(r"mk_meta_fit <- function\((.*?)\) \{", r, re.S).group(1)
    assert "result3 = res[[7]]" in r and "o$p.predict" in r


def test_sppredict_rejects_covariates_with_the_wrong_row_count(mk):
    """Checked on the host before anything reaches the device."""
    from importlib import import_module
    sb = import_module(mk.__name__ + ".spbayes")

    class _Ses:
        q = 2

        def set_test_sites(self, *a, **k):
            raise AssertionError("the device must not be reached")

    fit = {"_session": _Ses(), "_n_samples": 12}
    with pytest.raises(ValueError):
        sb.spPredict(fit, np.zeros((5, 2)), pred_covars=np.zeros((9, 4)))
