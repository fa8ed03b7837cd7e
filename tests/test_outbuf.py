"""OutputBuffers: the arrays behind an mk_outputs and their unpacking into the layouts
Session.outputs and meta_fit_node return.  No GPU and no library: the buffers are filled here, and
the expected entries are index formulas of include/mk.h's layouts, written out below.

K = 3 subsets of 3 / 5 / 4 sites, q = 2, p = 2 (P = 2 + 3 + 2 = 7), 4 test sites (C = 8), 6 iterations of which
burn_in = 4 keeps 3."""
import ctypes
from importlib import import_module

import numpy as np
import pytest

N_PART, Q, N_TEST, L = [3, 5, 4], 2, 4, 200
ALL = ["parameters", "w_predict", "samples", "w_samples", "w_pred_samples", "acceptance", "w_predict_sum", "p_predict",
       "p_pred_samples", "p_predict_sum"]


@pytest.fixture(scope="module")
def outbuf(mk):
    return import_module(mk.__name__ + ".outbuf")


@pytest.fixture(scope="module")
def cfg(mk):
    return mk.SamplerConfig(Q, 2, beta_starting=np.zeros(2), beta_tuning=np.full(2, 0.05), n_batch=2,
                            batch_length=3, burn_in=4)


def _filled(outbuf, cfg):
    ob = outbuf.OutputBuffers(3, cfg, N_PART, N_TEST, cfg.kept, set(ALL))
    for k, (name, a) in enumerate(ob.buf.items()):
        a[...] = (1000 * k + np.arange(a.size, dtype=np.float64)).reshape(a.shape)
    return ob


def test_every_field_unpacks_by_the_layout_formulas(outbuf, cfg):
    ob = _filled(outbuf, cfg)
    assert set(ob.buf) == set(ALL)
    n, P, C, kept = cfg.n_samples, cfg.P, Q * N_TEST, cfg.kept
    assert (n, P, C, kept) == (6, 7, 8, 3)
    shapes = dict(parameters=(3, P, L), w_predict=(3, C, L), p_predict=(3, C, L), samples=(3, P, n),
                  w_pred_samples=(3, kept, C), p_pred_samples=(3, kept, C), acceptance=(3, P + 1, cfg.n_batch),
                  w_predict_sum=(C, L), p_predict_sum=(C, L), w_samples=(sum(N_PART) * Q * n,))
    for name, shape in shapes.items():
        assert ob.buf[name].shape == shape, name
        # the mk_outputs field points at the buffer
        assert ctypes.cast(getattr(ob.c, name), ctypes.c_void_p).value == ob.buf[name].ctypes.data, name
    buf = {name: a.copy() for name, a in ob.buf.items()}
    out = ob.unpack()
    assert set(out) == set(ALL)
    # per subset: out[name][i][l, c] == buf[i, c, l]
    for name in ("parameters", "w_predict", "p_predict", "samples", "w_pred_samples", "p_pred_samples", "acceptance"):
        _, nc, nl = shapes[name]
        assert isinstance(out[name], list) and len(out[name]) == 3
        for i in range(3):
            assert out[name][i].shape == (nl, nc) and out[name][i].flags.c_contiguous, name
            for c in range(nc):
                for l in range(nl):
                    assert out[name][i][l, c] == buf[name][i, c, l], (name, i, l, c)
    # the sums: out[name][l, c] == buf[c, l]
    for name in ("w_predict_sum", "p_predict_sum"):
        assert out[name].shape == (L, C)
        for c in range(C):
            for l in range(L):
                assert out[name][l, c] == buf[name][c, l], (name, l, c)
    # the ragged w samples: ws[i][k, r] == flat[off_i + r * N_i + k], N_i = n_part[i] * q
    flat, off = buf["w_samples"], 0
    assert len(out["w_samples"]) == 3
    for i, ns in enumerate(N_PART):
        N = ns * Q
        assert out["w_samples"][i].shape == (N, n)
        for k in range(N):
            for r in range(n):
                assert out["w_samples"][i][k, r] == flat[off + r * N + k], (i, k, r)
        off += N * n
    assert off == flat.size


def test_only_the_requested_fields_exist(outbuf, cfg):
    ob = outbuf.OutputBuffers(3, cfg, N_PART, N_TEST, cfg.kept, {"samples", "p_predict_sum"})
    assert set(ob.buf) == set(ob.unpack()) == {"samples", "p_predict_sum"}
    for name in ALL:
        assert bool(getattr(ob.c, name)) == (name in ob.buf), name
    with pytest.raises(KeyError):
        outbuf.OutputBuffers(3, cfg, N_PART, N_TEST, cfg.kept, {"w_predict_total"})


class _NoLib:
    """Stands in for libmk behind a Session made without one: every call succeeds and writes nothing."""

    def __getattr__(self, name):
        return lambda *a: 0


def _session(mk, cfg, x_test):
    ses = mk.Session.__new__(mk.Session)
    ses.cfg, ses.q, ses.p = cfg, cfg.q, cfg.p
    ses.S, ses.n_part, ses.n_test = 3, np.array(N_PART, dtype=np.int32), N_TEST
    ses.x_test = x_test
    ses._lib, ses._h, ses._window = _NoLib(), None, None
    return ses


def test_session_selection_rules(mk, cfg):
    """Which fields Session.outputs turns on: p_predict by default only with covariates, w_predict only
    with the quantiles, and a kept window sizes both draw arrays."""
    plain = _session(mk, cfg, None)
    assert set(plain.outputs()) == {"parameters", "w_predict"}                       # p_predict off without x_test
    with_x = _session(mk, cfg, np.zeros(Q * N_TEST * 2))
    assert set(with_x.outputs()) == {"parameters", "w_predict", "p_predict"}
    assert set(with_x.outputs(quantiles=False, samples=True)) == {"samples"}        # no w_predict, no p_predict
    assert set(with_x.outputs(w_predict=False, p_predict=False)) == {"parameters"}
    draws = with_x.outputs(quantiles=False, w_pred_samples=True, p_pred_samples=True)
    assert draws["w_pred_samples"][0].shape == draws["p_pred_samples"][0].shape == (Q * N_TEST, cfg.kept)
    with_x.set_kept_window(4, 5)                                                       # a window of 2 states
    draws = with_x.outputs(quantiles=False, w_pred_samples=True, p_pred_samples=True)
    assert draws["w_pred_samples"][2].shape == draws["p_pred_samples"][2].shape == (Q * N_TEST, 2)
    no_sites = _session(mk, cfg, None)
    no_sites.n_test = 0
    assert set(no_sites.outputs(w_pred_samples=True, w_predict_sum=True)) == {"parameters"}
