// Chain diagnostics on the host side (include/mk.h: ess, mcse and split R-hat per chain): the launcher
// of k_chain_diag / k_chain_diag_prob (mk_mcmc.hip section 8b), a session's diagnostics of its recorded
// samples and fused kriging draws, the sink a tiled session fills tile by tile from the replay that
// makes the grids, and the stand-alone entry on caller-given chains.  Nothing here runs, and no
// scratch is allocated, unless diagnostics are asked for.
#include <hip/hip_runtime.h>
#include <string>
#include "mk_session.hpp"

using namespace mk;

int mk::launch_chain_diag(unsigned grid, hipStream_t st, const double* data, long subset_stride, long row_stride,
                          int n_rows, int n_cols, double* out, const ProbSrc* ps) {
  if (n_rows < 4 || n_rows > MK_QUANT_MAX)
    return set_err(MK_E_ARG, "chain diagnostics take 4 .. " + std::to_string(MK_QUANT_MAX) + " states per chain, not " +
                                 std::to_string(n_rows));
  const size_t lds = (size_t)n_rows * 8;
  if (ps) {
    HIPCHK(hipFuncSetAttribute((const void*)k_chain_diag_prob, hipFuncAttributeMaxDynamicSharedMemorySize, MK_QUANT_MAX * 8));
    MK_LAUNCH(k_chain_diag_prob, dim3(grid), dim3(256), lds, st, data, subset_stride, row_stride, n_rows, n_cols, out, *ps);
  } else {
    HIPCHK(hipFuncSetAttribute((const void*)k_chain_diag, hipFuncAttributeMaxDynamicSharedMemorySize, MK_QUANT_MAX * 8));
    MK_LAUNCH(k_chain_diag, dim3(grid), dim3(256), lds, st, data, subset_stride, row_stride, n_rows, n_cols, out);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int mk::diag_to_host(mk_session* s, const double* data, long subset_stride, long row_stride, int n_rows, long Ct,
                     const ProbSrc* ps, long col0, long C, double* h_each, double* h_worst) {
  if (!h_each && !h_worst) return 0;
  const int S = s->S;
  hipStream_t st = s->stream;
  if ((long)S * Ct > 0x7fffffffL) return set_err(MK_E_ARG, "too many chains for one diagnostic launch");
  DevBufs scratch;
  double* dd = scratch.get<double>((size_t)S * Ct * MK_N_DIAG);
  double* dw = h_worst ? scratch.get<double>((size_t)Ct * MK_N_DIAG) : nullptr;
  if (!dd || (h_worst && !dw)) return set_err(MK_E_NOMEM, "diagnostics scratch");
  EventTimer t;
  int rc = t.start(st);
  if (!rc) rc = launch_chain_diag((unsigned)(S * Ct), st, data, subset_stride, row_stride, n_rows, (int)Ct, dd, ps);
  if (!rc) rc = t.stop(st);
  if (rc) return rc;
  const size_t row = (size_t)Ct * MK_N_DIAG * 8;   // one subset's block
  if (h_each)
    HIPCHK(hipMemcpy2DAsync(h_each + (size_t)col0 * MK_N_DIAG, (size_t)C * MK_N_DIAG * 8, dd, row, row, S,
                            hipMemcpyDeviceToHost, st));
  if (h_worst) {
    MK_LAUNCH(k_diag_worst, dim3((unsigned)((Ct * MK_N_DIAG + 255) / 256)), dim3(256), 0, st, dd, S, Ct, dw);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_worst + (size_t)col0 * MK_N_DIAG, dw, row, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return t.price(s, KS_DIAG, 1);
}

int mk::tile_diagnostics(mk_session* s, int t0, int n_kept, int Ct) {
  const mk_diagnostics& d = s->diag_sink;
  const Model& md = s->md;
  const long C = (long)s->q * s->n_test_all, col0 = (long)t0 * s->q;
  int rc = diag_to_host(s, md.w_pred, (long)n_kept * Ct, (long)Ct, n_kept, Ct, nullptr, col0, C, d.w_predict,
                        d.w_predict_worst);
  if (rc) return rc;
  if (d.p_predict || d.p_predict_worst) {
    if (!s->d_xt) return set_err(MK_E_ARG, "the diagnostics sink asks for p_predict: that needs x_test");
    const ProbSrc ps = prob_src(s, t0);
    rc = diag_to_host(s, md.w_pred, (long)n_kept * Ct, (long)Ct, n_kept, Ct, &ps, col0, C, d.p_predict, d.p_predict_worst);
  }
  return rc;
}

extern "C" int mk_session_set_diagnostics(mk_session* s, const mk_diagnostics* sink) {
  if (!s) return set_err(MK_E_ARG, "null session");
  if (!sink) {
    s->diag_on = false;
    s->diag_sink = mk_diagnostics{};
    return 0;
  }
  if (!s->tiled)
    return set_err(MK_E_ARG, "a diagnostics sink serves tiled sessions (predict_tile > 0); a fused session's draws stay "
                             "in HBM: mk_session_diagnostics");
  if ((sink->p_predict || sink->p_predict_worst) && !s->d_xt)
    return set_err(MK_E_ARG, "p_predict diagnostics need x_test (mk_problem.x_test or mk_session_set_test_covars)");
  s->diag_sink = *sink;
  s->diag_on = sink->w_predict || sink->w_predict_worst || sink->p_predict || sink->p_predict_worst;
  return 0;
}

extern "C" int mk_session_diagnostics(mk_session* s, mk_diagnostics* o) {
  if (!s || !o) return set_err(MK_E_ARG, "null session/diagnostics");
  if (s->poisoned) return poisoned_err(s);
  const Model& md = s->md;
  const bool want_w = o->w_predict || o->w_predict_worst, want_p = o->p_predict || o->p_predict_worst;
  if (s->iter < md.n_samples) return set_err(MK_E_ARG, "chain diagnostics need all n.samples iterations");
  if ((want_w || want_p) && s->tiled)
    return set_err(MK_E_ARG, "a tiled session's kriging draws exist one tile at a time: attach a sink with "
                             "mk_session_set_diagnostics and the tile replays fill it");
  if ((want_w || want_p) && md.n_test < 1) return set_err(MK_E_ARG, "the session has no test sites");
  if (want_p && !s->d_xt)
    return set_err(MK_E_ARG, "p_predict diagnostics need x_test (mk_problem.x_test or mk_session_set_test_covars)");
  MK_ENTRY_DEVICE(s->device);
  const int P = s->P;
  int rc;
  if (o->parameters || o->parameters_worst) {
    if (!md.samples) return set_err(MK_E_ARG, "samples were not recorded (record_samples = 0)");
    const int n = s->win_n < 0 ? md.n_kept : s->win_n;
    rc = diag_to_host(s, md.samples + (long)(md.kept0 + s->win_lo) * P, (long)md.n_samples * P, (long)P, n, P, nullptr, 0, P,
                      o->parameters, o->parameters_worst);
    if (rc) return rc;
  }
  const long C = (long)s->q * md.n_test;
  if (want_p) {
    const ProbSrc ps = prob_src(s, 0);
    rc = diag_to_host(s, md.w_pred, (long)md.n_kept * C, C, md.n_kept, C, &ps, 0, C, o->p_predict, o->p_predict_worst);
    if (rc) return rc;
  }
  if (want_w) {
    rc = diag_to_host(s, md.w_pred, (long)md.n_kept * C, C, md.n_kept, C, nullptr, 0, C, o->w_predict, o->w_predict_worst);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int mk_chain_diagnostics(const double* x, int32_t n_rows, int64_t n_cols, double* out, int32_t device) {
  if (!x || !out) return set_err(MK_E_ARG, "null chains/output");
  if (n_cols < 1 || n_cols > 0x7fffffffL) return set_err(MK_E_ARG, "n_cols must be 1 .. 2^31 - 1");
  if (n_rows < 4 || n_rows > MK_QUANT_MAX)
    return set_err(MK_E_ARG, "chain diagnostics take 4 .. " + std::to_string(MK_QUANT_MAX) + " states per chain, not " +
                                 std::to_string(n_rows));
  MK_ENTRY_DEVICE(device);
  DevBufs b;
  double* dx = b.get<double>((size_t)n_rows * n_cols);
  double* dd = b.get<double>((size_t)n_cols * MK_N_DIAG);
  if (!dx || !dd) return set_err(MK_E_NOMEM, "chain diagnostics buffers");
  HIPCHK(hipMemcpy(dx, x, (size_t)n_rows * n_cols * 8, hipMemcpyHostToDevice));
  // column c is the contiguous chain at c * n_rows: n_cols "subsets" of one column each
  const int rc = launch_chain_diag((unsigned)n_cols, 0, dx, (long)n_rows, 1L, n_rows, 1, dd, nullptr);
  if (rc) return rc;
  HIPCHK(hipMemcpy(out, dd, (size_t)n_cols * MK_N_DIAG * 8, hipMemcpyDeviceToHost));
  return 0;
}
