// Parity-test entry points: the sampler's own candidate and Cholesky kernels on caller-given inputs.
#include <hip/hip_runtime.h>
#include <memory>
#include <vector>
#include "mk_gemm.hpp"
#include "mk_session.hpp"

using namespace mk;

// ------------------------------------------------------------------ parity-test entry points
// R (candidate route) and P^T (kriging route) of S point sets by the session's own kernels, each set a
// one-outcome Model assembled here: theta = 0 with Unif(0, 2 phi) / Unif(0, 2 nu) supports gives exactly
// phi and nu (logitInv(0, 0, b) = b - b/2); the border row is u = 0.  stored_tables: the Matern tables
// as a session has them (span / span_pt by the session's expressions, k_matern_table /
// k_matern_table_list store them, the tile workgroups load them); else the span and table pointers
// stay null and the kernels build unbounded tables themselves.
extern "C" int mk_correlation_cross_batched(const double* coords, int32_t S, int32_t n, const double* coords_test,
                                            int32_t n_test, const double* phi, const double* nu, int32_t cov_model,
                                            int32_t stored_tables, double* R_out, double* PT_out, int32_t device) {
  if (!coords || !phi || S < 1 || n < 1 || (!R_out && !PT_out)) return set_err(MK_E_ARG, "bad correlation arguments");
  if (PT_out && (!coords_test || n_test < 1)) return set_err(MK_E_ARG, "P^T needs test sites");
  if (cov_model != MK_COV_EXPONENTIAL && cov_model != MK_COV_MATERN) return set_err(MK_E_ARG, "bad cov_model");
  if (cov_model == MK_COV_MATERN && !nu) return set_err(MK_E_ARG, "matern needs nu");
  for (int s = 0; s < S; ++s)
    if (!(phi[s] > 0.0) || (nu && cov_model == MK_COV_MATERN && !(nu[s] > 0.0)))
      return set_err(MK_E_ARG, "phi and nu must be > 0");
  MK_ENTRY_DEVICE(device);
  const int n_pad = round_up(n + 1, MK_NB), nt = n_pad / MK_NB;
  const bool matern = cov_model == MK_COV_MATERN, stored = matern && stored_tables != 0;
  const int n_theta = matern ? 3 : 2;
  const int nte = PT_out ? n_test : 0;
  const int n_test_pad = round_up(std::max(nte, 1), 256);   // as kriging_buffers: the kernels write ntt * 128 columns
  DevBufs b;
  double* dc = b.get<double>((size_t)S * 2 * n_pad);
  double* dth = b.get<double>((size_t)S * n_theta);
  double* du = b.get<double>((size_t)S * n_pad);
  int* dns = b.get<int>(S);
  int* dcur = b.get<int>(S + 2);                           // [S] slots (0), then the pair list {0} and its count {1}
  double* dL = R_out ? b.get<double>((size_t)S * 2 * n_pad * n_pad) : nullptr;
  double* dr = R_out ? b.get<double>((size_t)S * n * n) : nullptr;
  double* dct = PT_out ? b.get<double>((size_t)S * 2 * n_test_pad) : nullptr;
  double* dPT = PT_out ? b.get<double>((size_t)S * n_pad * n_test_pad) : nullptr;
  double* dspan = stored ? b.get<double>((size_t)2 * S) : nullptr;           // [S] span, [S] span_pt
  double* dtab = stored ? b.get<double>((size_t)2 * S * MK_CH_TAB) : nullptr;   // [S] chtab, [S] chtab_p
  if (!dc || !dth || !du || !dns || !dcur || (R_out && (!dL || !dr)) || (PT_out && (!dct || !dPT)) ||
      (stored && (!dspan || !dtab)))
    return set_err(MK_E_NOMEM, "correlation alloc");
  std::vector<double> hc((size_t)S * 2 * n_pad, 0.0), hct, hspan((size_t)2 * S, 0.0);
  if (PT_out) hct.assign((size_t)S * 2 * n_test_pad, 0.0);
  for (int s = 0; s < S; ++s) {
    const double* cs = coords + (size_t)s * 2 * n;
    for (int r = 0; r < n; ++r) {
      hc[(size_t)s * 2 * n_pad + r] = cs[r];
      hc[(size_t)s * 2 * n_pad + n_pad + r] = cs[n + r];
    }
    double bb[4], tb[4];
    site_bbox(cs, cs + n, n, bb);
    hspan[s] = matern_span(bb);
    if (PT_out) {
      const double* ts = coords_test + (size_t)s * 2 * n_test;
      for (int t = 0; t < n_test; ++t) {
        hct[(size_t)s * 2 * n_test_pad + t] = ts[t];
        hct[(size_t)s * 2 * n_test_pad + n_test_pad + t] = ts[n_test + t];
      }
      site_bbox(ts, ts + n_test, n_test, tb);
      hspan[S + s] = matern_span_pt(bb, tb);
    }
  }
  std::vector<int> hn(S, n), hcur(S + 2, 0);
  hcur[S + 1] = 1;
  HIPCHK(hipMemcpy(dc, hc.data(), hc.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dns, hn.data(), (size_t)S * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dcur, hcur.data(), hcur.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(dth, 0, (size_t)S * n_theta * 8));
  HIPCHK(hipMemset(du, 0, (size_t)S * n_pad * 8));
  if (PT_out) HIPCHK(hipMemcpy(dct, hct.data(), hct.size() * 8, hipMemcpyHostToDevice));
  if (stored) HIPCHK(hipMemcpy(dspan, hspan.data(), hspan.size() * 8, hipMemcpyHostToDevice));
  MatSet ms{};
  ms.L = dL; ms.cur = dcur; ms.ld = n_pad; ms.nt = nt; ms.q = 1;
  const int ntri_tiles = nt * (nt + 1) / 2;
  const int* d_list = dcur + S;
  const int* d_count = dcur + S + 1;
  for (int s = 0; s < S; ++s) {
    Model md{};
    md.S = 1; md.q = 1; md.p = 0; md.n_pad = n_pad; md.Np = n_pad; md.nt = nt; md.ntri = 1; md.n_theta = n_theta;
    md.cov_model = cov_model;
    md.o_A = 0; md.o_phi = 1; md.o_nu = 2; md.o_w = n_theta; md.n_mh_max = n_theta;
    md.phi_a[0] = 0.0; md.phi_b[0] = 2.0 * phi[s];
    md.nu_a[0] = 0.0; md.nu_b[0] = matern ? 2.0 * nu[s] : 1.0;
    md.n_s = dns + s;
    md.coords = dc + (size_t)s * 2 * n_pad;
    md.theta = dth + (size_t)s * n_theta;
    md.u = du + (size_t)s * n_pad;
    if (stored) {
      md.span = dspan + s;
      md.chtab = dtab + (size_t)s * MK_CH_TAB;
      if (PT_out) {
        md.span_pt = dspan + S + s;
        md.chtab_p = dtab + (size_t)(S + s) * MK_CH_TAB;
      }
    }
    if (R_out) {
      MatSet mv = ms;
      mv.L = dL + (size_t)s * 2 * n_pad * n_pad;
      mv.cur = dcur + s;
      if (stored) MK_LAUNCH(k_matern_table, dim3(1), dim3(256), 0, 0, md, 0, 1, 2, 0, nullptr, nullptr);
      MK_LAUNCH(cov_candidate_kernel(cov_model), dim3(xcd_grid_h(1, ntri_tiles)), dim3(256), 0, 0, md, mv, 0, 1,
                         2, 0, nullptr, nullptr);
    }
    if (PT_out) {
      md.n_test = n_test; md.n_test_pad = n_test_pad; md.ntt = n_test_pad / MK_NB;
      md.coords_test = dct + (size_t)s * 2 * n_test_pad;
      md.PT = dPT + (size_t)s * n_pad * n_test_pad;
      if (matern) {
        if (stored) MK_LAUNCH(k_matern_table_list, dim3(1), dim3(256), 0, 0, md, d_list, d_count);
        MK_LAUNCH(k_pred_PT_matern, dim3(n_pad / MK_PT_RB), dim3(256), 0, 0, md, d_list, d_count);
      } else {
        MK_LAUNCH(pred_PT_kernel(cov_model), dim3(n_pad), dim3(256), 0, 0, md, d_list, d_count);
      }
    }
  }
  if (R_out) MK_LAUNCH(k_extract_candidate, dim3(2048), dim3(256), 0, 0, ms, n, S, dr);
  HIPCHK(hipGetLastError());
  if (R_out) HIPCHK(hipMemcpy(R_out, dr, (size_t)S * n * n * 8, hipMemcpyDeviceToHost));
  if (PT_out) {   // rows k < n, columns t < n_test of every set's [n_pad][n_test_pad]
    for (int s = 0; s < S; ++s)
      HIPCHK(hipMemcpy2D(PT_out + (size_t)s * n * n_test, (size_t)n_test * 8, dPT + (size_t)s * n_pad * n_test_pad,
                         (size_t)n_test_pad * 8, (size_t)n_test * 8, n, hipMemcpyDeviceToHost));
  }
  return 0;
}

extern "C" int mk_correlation_batched(const double* coords, int32_t S, int32_t n, const double* phi, const double* nu,
                                      int32_t cov_model, double* R_out, int32_t device) {
  if (!R_out) return set_err(MK_E_ARG, "bad correlation arguments");
  return mk_correlation_cross_batched(coords, S, n, nullptr, 0, phi, nu, cov_model, 0, R_out, nullptr, device);
}

extern "C" int mk_cholesky_batched(const double* A, int32_t S, int32_t n, double* L_out, double* logdet_out,
                                   double* inv_out, int32_t device) {
  if (!A || S < 1 || n < 1) return set_err(MK_E_ARG, "bad cholesky arguments");
  MK_ENTRY_DEVICE(device);
  std::unique_ptr<mk_session> hold(new mk_session());   // frees the session on every return path
  mk_session* s = hold.get();
  s->device = device;
  if (pool_stream(s->owned, &s->stream, device, SK_PLAIN) != hipSuccess) return set_err(MK_E_HIP, "stream");
  const int n_pad = round_up(n + 1, MK_NB), nt = n_pad / MK_NB;
  s->S = S; s->q = 1; s->n_pad = n_pad; s->nt = nt;
  s->n_part.assign(S, n);
  Model& md = s->md;
  md.S = S; md.q = 1; md.nt = nt; md.n_pad = n_pad;
  MatSet& ms = s->ms;
  ms.ld = n_pad; ms.nt = nt; ms.q = 1;
  int rc;
  int* d_ns;
  double* dA;
  if ((rc = s->alloc(&d_ns, S)) || (rc = s->alloc(&md.ld_part, (size_t)S * nt)) || (rc = s->alloc(&md.quad_c, S)) ||
      (rc = s->alloc(&md.info, S)) || (rc = s->alloc(&md.dirty, S)) || (rc = s->alloc(&ms.cur, S)) ||
      (rc = s->alloc(&md.logdetR, S)) || (rc = s->alloc(&md.quad, S)) ||
      (rc = s->alloc(&ms.L, (size_t)S * 2 * n_pad * n_pad)) || (rc = s->alloc(&ms.Winv, (size_t)S * 2 * nt * MK_NB * MK_NB)) ||
      (rc = s->alloc(&ms.Q, (size_t)S * n_pad * n_pad)) || (rc = s->alloc(&ms.W, (size_t)S * n_pad * n_pad)) ||
      (rc = s->alloc(&dA, (size_t)S * n * n)))
    return rc;
  md.n_s = d_ns;
  if ((rc = setup_groups(s, 1))) return rc;
  Group& a = s->all;
  std::vector<int> hn(S, n);
  if (hipMemcpy(d_ns, hn.data(), S * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dA, A, (size_t)S * n * n * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(ms.cur, 0, S * 4) != hipSuccess || hipMemset(md.info, 0, S * 4) != hipSuccess ||
      hipMemset(ms.Winv, 0, (size_t)S * 2 * nt * MK_NB * MK_NB * 8) != hipSuccess)
    return set_err(MK_E_HIP, "cholesky upload");
  if (!set_gemm_lds()) return set_err(MK_E_HIP, "lds attribute");
  MK_LAUNCH(k_load_plain, dim3(2048), dim3(256), 0, s->stream, ms, dA, n, S);
  launch_cholesky(s, a, 0, 1);
  std::vector<double> part((size_t)S * nt);
  std::vector<int> info(S);
  if (hipStreamSynchronize(s->stream) != hipSuccess) return set_err(MK_E_HIP, "cholesky run");
  if (hipMemcpy(info.data(), md.info, S * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return set_err(MK_E_HIP, "info download");
  for (int i = 0; i < S; ++i)
    if (info[i]) return set_err(MK_E_ARG, "matrix " + std::to_string(i) + " is not positive definite");
  MK_LAUNCH(k_theta_init, dim3((S + 63) / 64), dim3(64), 0, s->stream, md, ms, 0, 1);
  double* dL = nullptr;
  if ((rc = s->alloc(&dL, (size_t)S * n * n))) return rc;
  if (L_out) {
    MK_LAUNCH(k_extract_L, dim3(2048), dim3(256), 0, s->stream, ms, n, S, dL, 0);
    if (hipMemcpyAsync(L_out, dL, (size_t)S * n * n * 8, hipMemcpyDeviceToHost, s->stream) != hipSuccess)
      return set_err(MK_E_HIP, "L download");
  }
  if (logdet_out) {
    if (hipMemcpy(part.data(), md.ld_part, part.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
      return set_err(MK_E_HIP, "logdet download");
    for (int i = 0; i < S; ++i) {
      double v = 0.0;
      for (int k = 0; k < nt; ++k) v += part[(size_t)i * nt + k];
      logdet_out[i] = v;
    }
  }
  if (inv_out) {
    MK_LAUNCH(k_dirty_list, dim3(1), dim3(256), 0, s->stream, md, 1, a.d_plist, a.d_pcount, a.d_list,
                       a.d_count);
    const int ntiles = nt * (nt + 1) / 2;
    launch_trinv(s, a, S, a.d_list, a.d_count);
    MK_LAUNCH(k_lauum, dim3(S * ntiles), dim3(256), gb_lds_bytes(128, 128), s->stream, ms, md.n_s, a.d_list, a.d_count);
    MK_LAUNCH(k_extract_L, dim3(2048), dim3(256), 0, s->stream, ms, n, S, dL, 1);
    if (hipMemcpyAsync(inv_out, dL, (size_t)S * n * n * 8, hipMemcpyDeviceToHost, s->stream) != hipSuccess)
      return set_err(MK_E_HIP, "inverse download");
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
  if (e != hipSuccess) return set_err(MK_E_HIP, std::string("cholesky: ") + hipGetErrorString(e));
  return 0;
}
