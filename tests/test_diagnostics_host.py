"""CPU-side checks of the chain-diagnostics surface: the header declares it, the ctypes mirror and
the buffer table match it, convergence_report counts what it says, and the NumPy restatement the GPU
tests are measured against (tests/diag_ref.py) agrees with AR(1) theory."""
import os
import re

import numpy as np
import pytest

from diag_ref import ar1, diag_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mk.h")).read(), flags=re.S)


def test_header_declares_the_entry_points_and_the_struct(mk):
    for fn in ("mk_session_diagnostics", "mk_session_set_diagnostics", "mk_meta_fit_diag", "mk_chain_diagnostics"):
        assert re.search(r"\bint %s\s*\(" % fn, HEADER), fn
        assert fn in mk._lib.EXPORTS
    assert re.search(r"#define MK_N_DIAG 3\b", HEADER) and mk._lib.N_DIAG == 3
    body = re.search(r"typedef struct mk_diagnostics \{(.*?)\} mk_diagnostics;", HEADER, flags=re.S).group(1)
    fields = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*;", body)
    assert fields == ["parameters", "w_predict", "p_predict", "parameters_worst", "w_predict_worst", "p_predict_worst"]
    assert fields == [f[0] for f in mk._lib.Diagnostics._fields_]
    # mk_meta_fit_diag takes mk_meta_fit's arguments and the diagnostics last
    a = mk._lib.EXPORTS["mk_meta_fit"][1]
    b = mk._lib.EXPORTS["mk_meta_fit_diag"][1]
    assert b[:-1] == a and b[-1]._type_ is mk._lib.Diagnostics


def test_buffer_table_covers_the_struct(mk):
    ob = mk.outbuf
    assert {m for s, m in ob.STRUCT_OF.values() if s == "diagnostics"} == {f[0] for f in mk._lib.Diagnostics._fields_}
    assert {m for s, m in ob.STRUCT_OF.values() if s == "outputs"} == {f[0] for f in mk._lib.Outputs._fields_}
    cfg = mk.SamplerConfig(2, 4, np.zeros(4), np.full(4, 0.1), n_batch=2, batch_length=5, burn_in=3)
    db = ob.DiagnosticBuffers(3, cfg, 7, {"parameters_diag", "w_predict_diag_worst"})
    assert db.buf["parameters_diag"].shape == (3, cfg.P, 3) and db.buf["w_predict_diag_worst"].shape == (14, 3)
    assert db.c.parameters and db.c.w_predict_worst and not db.c.w_predict and not db.c.p_predict_worst
    only = db.struct(["w_predict_diag_worst"])
    assert only.w_predict_worst and not only.parameters
    db.buf["parameters_diag"][1, 2] = (5.0, 6.0, 7.0)
    un = db.unpack()
    assert un["parameters_diag"][1].shape == (3, cfg.P) and list(un["parameters_diag"][1][:, 2]) == [5.0, 6.0, 7.0]
    assert un["w_predict_diag_worst"].shape == (3, 14)
    with pytest.raises(KeyError):
        ob.DiagnosticBuffers(3, cfg, 7, {"w_samples_diag"})


def test_convergence_report_counts(mk):
    #                 ess                     mcse                   rhat
    s0 = np.array([[500.0, 80.0, 120.0], [0.01, 0.02, 0.03], [1.00, 1.20, 1.01]])
    s1 = np.array([[99.0, 300.0, np.nan], [0.05, 0.01, np.nan], [1.04, np.inf, np.nan]])
    rep = mk.convergence_report({"parameters_diag": [s0, s1]})
    assert set(rep) == {"parameters"}
    r = rep["parameters"]
    assert r["chains"] == 6 and r["columns"] == 3
    assert r["ess_below"] == 2 and r["rhat_above"] == 2 and r["not_finite"] == 1
    assert r["min_ess"] == 80.0 and r["min_ess_column"] == 1
    assert r["max_rhat"] == np.inf and r["max_rhat_column"] == 1 and r["max_mcse"] == 0.05
    # the worst rows alone, with the caller's own thresholds
    worst = np.array([[99.0, 80.0, np.nan], [0.05, 0.02, np.nan], [1.04, np.inf, np.nan]])
    r = mk.convergence_report({"w_predict_diag_worst": worst}, ess_min=90, rhat_max=1.01)["w_predict"]
    assert r["chains"] == 3 and r["ess_below"] == 1 and r["rhat_above"] == 2 and r["not_finite"] == 1
    assert mk.convergence_report({"result": np.zeros(3)}) == {}


def test_restatement_against_ar1_theory():
    """At n = 4096 the median over 64 columns of ess / (n (1 - rho) / (1 + rho)) lies in [0.9, 1.15]:
    this pins the formulas (not the kernel).  The edge rules of the restatement itself."""
    rng = np.random.default_rng(20250114)
    n = 4096
    for rho in (0.0, 0.5, 0.9, -0.5):
        out, aux = diag_ref(ar1(rng, n, 64, rho))
        ratio = float(np.median(out[0] / (n * (1 - rho) / (1 + rho))))
        print(f"rho = {rho}: median ess / theory {ratio:.3f}, largest rhat {out[2].max():.4f}")
        assert 0.9 <= ratio <= 1.15
        assert out[2].max() < 1.2 and (out[1] > 0).all()
    edge = np.array([[1.5, 1.0, 0.3], [1.5, 1.0, np.nan], [1.5, 2.0, 0.1], [1.5, 2.0, 0.2]])
    out, _ = diag_ref(edge)
    assert list(out[:, 0]) == [0.0, 0.0, np.inf]
    assert out[2, 1] == np.inf and np.isfinite(out[0, 1])
    assert np.isnan(out[:, 2]).all()
