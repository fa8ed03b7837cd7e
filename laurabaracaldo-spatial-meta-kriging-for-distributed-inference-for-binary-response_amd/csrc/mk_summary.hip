// Stateless entry points: combine, Weiszfeld median, posterior summary, glm start values.  None of
// them takes a session.
#include <hip/hip_runtime.h>
#include <cmath>
#include <vector>
#include "mk_session.hpp"

using namespace mk;

namespace {
// R's seq.default(from, to, by) for by > 0: from + (0:n)*by, n = as.integer(del/by + 1e-10), pmin(x, to).
std::vector<double> r_seq(double from, double to, double by) {
  const int n = (int)((to - from) / by + 1e-10);
  std::vector<double> x(n + 1);
  for (int i = 0; i <= n; ++i) x[i] = std::fmin(from + (double)i * by, to);
  return x;
}
}  // namespace

// ------------------------------------------------------------------ combine
static int combine_host(const double* grids, int32_t K, int64_t G, double* out, int mean, int32_t device) {
  if (!grids || !out || K < 1 || G < 1) return set_err(MK_E_ARG, "bad combine arguments");
  MK_ENTRY_DEVICE(device);
  DevBufs b;
  double* dg = b.get<double>((size_t)K * G);
  double* dout = b.get<double>((size_t)G);
  if (!dg || !dout) return set_err(MK_E_NOMEM, "combine alloc");
  HIPCHK(hipMemcpy(dg, grids, (size_t)K * G * 8, hipMemcpyHostToDevice));
  MK_LAUNCH(k_combine, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, 0, dg, K, (long)G, dout, mean);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, (size_t)G * 8, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int mk_combine(const double* grids, int32_t K, int64_t G, double* out, int32_t device) {
  return combine_host(grids, K, G, out, 1, device);
}

extern "C" int mk_combine_sum(const double* grids, int32_t K, int64_t G, double* out, int32_t device) {
  return combine_host(grids, K, G, out, 0, device);
}

extern "C" int mk_combine_device(const double* d_grids, int32_t K, int64_t G, double* d_out, int32_t mean,
                                 int32_t device, void* stream) {
  if (!d_grids || !d_out || K < 1 || G < 1) return set_err(MK_E_ARG, "bad combine arguments");
  MK_ENTRY_DEVICE(device);
  MK_LAUNCH(k_combine, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_grids, K, (long)G,
                     d_out, mean ? 1 : 0);
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int mk_combine_median(const double* grids, int32_t K, int32_t L, int64_t C, int32_t max_iter, double tol,
                                 double* out, int32_t* iters, int32_t device) {
  if (!grids || !out || K < 1 || L < 1 || L > 256 || C < 1 || max_iter < 1 || !(tol >= 0.0))
    return set_err(MK_E_ARG, "bad combine_median arguments (1 <= n_levels <= 256, max_iter >= 1, tol >= 0)");
  MK_ENTRY_DEVICE(device);
  DevBufs b;
  const size_t G = (size_t)L * C;
  double* dg = b.get<double>((size_t)K * G);
  double* dout = b.get<double>(G);
  int* dit = b.get<int>((size_t)C);
  if (!dg || !dout || !dit) return set_err(MK_E_NOMEM, "combine_median alloc");
  HIPCHK(hipMemcpy(dg, grids, (size_t)K * G * 8, hipMemcpyHostToDevice));
  MK_LAUNCH(k_weiszfeld, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, 0, dg, K, L, (long)C, max_iter, tol, dout,
                     dit);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, G * 8, hipMemcpyDeviceToHost));
  if (iters) HIPCHK(hipMemcpy(iters, dit, (size_t)C * 4, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int mk_combine_median_device(const double* d_grids, int32_t K, int32_t L, int64_t C, int32_t max_iter,
                                        double tol, double* d_out, int32_t* d_iters, int32_t device, void* stream) {
  if (!d_grids || !d_out || K < 1 || L < 1 || L > 256 || C < 1 || max_iter < 1 || !(tol >= 0.0))
    return set_err(MK_E_ARG, "bad combine_median arguments (1 <= n_levels <= 256, max_iter >= 1, tol >= 0)");
  MK_ENTRY_DEVICE(device);
  MK_LAUNCH(k_weiszfeld, dim3((unsigned)((C + 3) / 4)), dim3(256), 0, (hipStream_t)stream, d_grids, K, L, (long)C,
                     max_iter, tol, d_out, d_iters);
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ post-combine steps (MK.R:136-165)
extern "C" int mk_posterior_summary_ex(const double* result, int32_t P, const double* result2, int64_t C,
                                       const double* x_test, int32_t p, int32_t S, uint64_t seed,
                                       const int32_t* index, int32_t link, mk_summary* o, int32_t device) {
  if (!result || !o || P < 1 || C < 0 || p < 0 || p > P || S < 1 || S > MK_QUANT_MAX)
    return set_err(MK_E_ARG, "bad posterior_summary arguments (P >= 1, 0 <= p <= P, 1 <= samplesize <= 16384)");
  if (C > 0 && (!result2 || (p > 0 && !x_test))) return set_err(MK_E_ARG, "result2 / x_test missing");
  if (link != MK_LINK_LOGIT && link != MK_LINK_PROBIT) return set_err(MK_E_ARG, "link must be logit or probit");
  MK_ENTRY_DEVICE(device);
  const int L = MK_N_LEVELS;
  const std::vector<double> xg = r_seq(0.005, 1.0, 0.005);   // allquant levels (MK.R:88)
  const std::vector<double> xo = r_seq(0.005, 1.0, 0.001);   // Xout (MK.R:140)
  const int n = (int)xg.size(), NL = (int)xo.size();
  if (n != L) return set_err(MK_E_ARG, "internal: probs grid");
  // stats/src/approx.c approx1: bisection to x[i] <= v <= x[j], exact hits return y
  std::vector<int> lo(NL), hi(NL), mode(NL);
  std::vector<double> tt(NL, 0.0);
  for (int k = 0; k < NL; ++k) {
    const double v = xo[k];
    int i = 0, j = n - 1;
    while (i < j - 1) {
      const int ij = (i + j) / 2;
      if (v < xg[ij]) j = ij; else i = ij;
    }
    lo[k] = i;
    hi[k] = j;
    if (v == xg[j]) mode[k] = 0;
    else if (v == xg[i]) mode[k] = 1;
    else { mode[k] = 2; tt[k] = (v - xg[i]) / (xg[j] - xg[i]); }
  }
  const double probs3[3] = {0.5, 0.025, 0.975};   // quant.pred (MK.R:163)
  DevBufs b;
  const size_t Cs = (size_t)std::max<int64_t>(C, 1);
  double* d_res = b.get<double>((size_t)L * P);
  double* d_res2 = b.get<double>((size_t)L * Cs);
  double* d_xt = b.get<double>(Cs * std::max(p, 1));
  int* d_idx = b.get<int>(S);
  int* d_lo = b.get<int>(NL);
  int* d_hi = b.get<int>(NL);
  int* d_mode = b.get<int>(NL);
  double* d_t = b.get<double>(NL);
  double* d_spar = b.get<double>((size_t)S * P);
  double* d_sw = b.get<double>((size_t)S * Cs);
  double* d_p = b.get<double>((size_t)S * Cs);
  double* d_q = b.get<double>((size_t)3 * std::max<size_t>(Cs, P));
  double* d_pr = b.get<double>(3);
  if (!d_res || !d_res2 || !d_xt || !d_idx || !d_lo || !d_hi || !d_mode || !d_t || !d_spar || !d_sw || !d_p || !d_q ||
      !d_pr)
    return set_err(MK_E_NOMEM, "posterior_summary alloc");
  hipStream_t st = 0;
  HIPCHK(hipMemcpy(d_res, result, (size_t)L * P * 8, hipMemcpyHostToDevice));
  if (C > 0) HIPCHK(hipMemcpy(d_res2, result2, (size_t)L * C * 8, hipMemcpyHostToDevice));
  if (C > 0 && p > 0) HIPCHK(hipMemcpy(d_xt, x_test, (size_t)C * p * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_lo, lo.data(), NL * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_hi, hi.data(), NL * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_mode, mode.data(), NL * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_t, tt.data(), NL * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_pr, probs3, 3 * 8, hipMemcpyHostToDevice));
  if (index) {   // sampleparIndex drawn by the caller (R: sample(seq(1, length(Xout), 1), ...)), 1-based
    std::vector<int> hidx(S);
    for (int j = 0; j < S; ++j) {
      if (index[j] < 1 || index[j] > NL) return set_err(MK_E_ARG, "index entries must be in 1..length(Xout)");
      hidx[j] = index[j] - 1;
    }
    HIPCHK(hipMemcpy(d_idx, hidx.data(), (size_t)S * 4, hipMemcpyHostToDevice));
  } else {
    MK_LAUNCH(k_post_index, dim3((S + 255) / 256), dim3(256), 0, st, seed, S, NL, d_idx);
  }
  MK_LAUNCH(k_post_interp, dim3((unsigned)(((long)S * P + 255) / 256)), dim3(256), 0, st, d_res, L, (long)P,
                     d_idx, S, d_lo, d_hi, d_mode, d_t, d_spar);
  if (C > 0) {
    const unsigned nb = (unsigned)(((long)S * C + 255) / 256);
    MK_LAUNCH(k_post_interp, dim3(nb), dim3(256), 0, st, d_res2, L, (long)C, d_idx, S, d_lo, d_hi, d_mode, d_t,
                       d_sw);
    MK_LAUNCH(k_post_prob, dim3(nb), dim3(256), 0, st, d_spar, S, d_xt, (long)C, p, d_sw, link, d_p);
  }
  HIPCHK(hipGetLastError());
  if (o->index) HIPCHK(hipMemcpy(o->index, d_idx, (size_t)S * 4, hipMemcpyDeviceToHost));
  if (o->sample_par) HIPCHK(hipMemcpy(o->sample_par, d_spar, (size_t)S * P * 8, hipMemcpyDeviceToHost));
  if (C > 0 && o->sample_w) HIPCHK(hipMemcpy(o->sample_w, d_sw, (size_t)S * C * 8, hipMemcpyDeviceToHost));
  if (C > 0 && o->p_sample) HIPCHK(hipMemcpy(o->p_sample, d_p, (size_t)S * C * 8, hipMemcpyDeviceToHost));
  // type-7 (0.5, 0.025, 0.975) per column: each column is S contiguous rows -> 3 x ncol column-major
  auto quant = [&](const double* src, long ncol, double* dst) -> int {
    const int rq = launch_quantiles((unsigned)ncol, st, src, (long)S, 1L, S, 1, d_pr, 3, d_q);
    if (rq) return rq;
    HIPCHK(hipMemcpy(dst, d_q, (size_t)ncol * 3 * 8, hipMemcpyDeviceToHost));
    return 0;
  };
  int rc;
  if (o->param_quant && (rc = quant(d_spar, P, o->param_quant))) return rc;
  if (C > 0 && o->w_quant && (rc = quant(d_sw, C, o->w_quant))) return rc;
  if (C > 0 && o->p_quant && (rc = quant(d_p, C, o->p_quant))) return rc;
  return 0;
}

extern "C" int mk_posterior_summary(const double* result, int32_t P, const double* result2, int64_t C,
                                    const double* x_test, int32_t p, int32_t S, uint64_t seed, mk_summary* o,
                                    int32_t device) {
  return mk_posterior_summary_ex(result, P, result2, C, x_test, p, S, seed, nullptr, MK_LINK_LOGIT, o, device);
}

// ------------------------------------------------------------------ glm start values (MK.R:53-55)
// p x p symmetric positive definite solve / inverse through a host Cholesky (p <= 8).
static bool chol_small(const std::vector<double>& A, int p, std::vector<double>& Lc) {
  Lc.assign((size_t)p * p, 0.0);
  for (int j = 0; j < p; ++j) {
    double d = A[j + j * p];
    for (int k = 0; k < j; ++k) d -= Lc[j + k * p] * Lc[j + k * p];
    if (!(d > 0.0)) return false;
    d = std::sqrt(d);
    Lc[j + j * p] = d;
    for (int i = j + 1; i < p; ++i) {
      double v = A[i + j * p];
      for (int k = 0; k < j; ++k) v -= Lc[i + k * p] * Lc[j + k * p];
      Lc[i + j * p] = v / d;
    }
  }
  return true;
}
static void chol_solve_small(const std::vector<double>& Lc, int p, const double* b, double* x) {
  std::vector<double> y(p);
  for (int i = 0; i < p; ++i) {
    double v = b[i];
    for (int k = 0; k < i; ++k) v -= Lc[i + k * p] * y[k];
    y[i] = v / Lc[i + i * p];
  }
  for (int i = p - 1; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < p; ++k) v -= Lc[k + i * p] * x[k];
    x[i] = v / Lc[i + i * p];
  }
}

extern "C" int mk_glm_binomial_link(const double* y, const double* weights, const double* x, int64_t n, int32_t p,
                                    int32_t link, double epsilon, int32_t maxit, double* coef, double* vcov,
                                    int32_t* iters, int32_t device) {
  if (!y || !weights || !x || !coef || n < 1 || p < 1 || p > 8 || maxit < 1)
    return set_err(MK_E_ARG, "bad glm arguments (n >= 1, 1 <= p <= 8, maxit >= 1)");
  if (link != MK_LINK_LOGIT && link != MK_LINK_PROBIT) return set_err(MK_E_ARG, "link must be logit or probit");
  MK_ENTRY_DEVICE(device);
  std::vector<double> yp((size_t)n);
  for (int64_t i = 0; i < n; ++i) yp[i] = y[i] / weights[i];     // glm((y/weight) ~ x - 1, ...)  MK.R:53
  const int ntri = p * (p + 1) / 2, NP = 1 + ntri + p;
  const int nblk = (int)std::min<int64_t>(1024, (n + 255) / 256);
  DevBufs b;
  double* d_y = b.get<double>((size_t)n);
  double* d_w = b.get<double>((size_t)n);
  double* d_x = b.get<double>((size_t)n * p);
  double* d_c = b.get<double>(p);
  double* d_part = b.get<double>((size_t)nblk * NP);
  if (!d_y || !d_w || !d_x || !d_c || !d_part) return set_err(MK_E_NOMEM, "glm alloc");
  HIPCHK(hipMemcpy(d_y, yp.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_w, weights, (size_t)n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_x, x, (size_t)n * p * 8, hipMemcpyHostToDevice));
  std::vector<double> part((size_t)nblk * NP), A((size_t)p * p), rhs(p), Lc, c(p, 0.0), A_used;
  double dev = 0.0;
  auto pass = [&](int mode) -> int {
    if (mode == 1) HIPCHK(hipMemcpy(d_c, c.data(), (size_t)p * 8, hipMemcpyHostToDevice));
    MK_LAUNCH(k_glm_pass, dim3(nblk), dim3(256), 0, 0, d_y, d_w, d_x, (long)n, p, d_c, mode, link, d_part);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(part.data(), d_part, part.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> tot(NP, 0.0);
    for (int bk = 0; bk < nblk; ++bk)
      for (int i = 0; i < NP; ++i) tot[i] += part[(size_t)bk * NP + i];
    dev = tot[0];
    int k = 1;
    for (int a = 0; a < p; ++a)
      for (int bb = a; bb < p; ++bb, ++k) A[a + bb * p] = A[bb + a * p] = tot[k];
    for (int a = 0; a < p; ++a) rhs[a] = tot[1 + ntri + a];
    return 0;
  };
  int rc = pass(0);
  if (rc) return rc;
  double devold = dev;
  int it = 0;
  for (it = 1; it <= maxit; ++it) {
    if (!chol_small(A, p, Lc)) return set_err(MK_E_ARG, "glm: singular weighted design");
    A_used = A;
    chol_solve_small(Lc, p, rhs.data(), c.data());
    if ((rc = pass(1))) return rc;
    if (std::fabs(dev - devold) / (std::fabs(dev) + 0.1) < epsilon) break;
    devold = dev;
  }
  if (it > maxit) it = maxit;
  for (int j = 0; j < p; ++j) coef[j] = c[j];
  if (vcov) {   // chol2inv of the final fit's weighted design = (X'WX)^-1 at the weights that produced coef
    if (!chol_small(A_used, p, Lc)) return set_err(MK_E_ARG, "glm: singular weighted design");
    std::vector<double> e(p), col(p);
    for (int j = 0; j < p; ++j) {
      std::fill(e.begin(), e.end(), 0.0);
      e[j] = 1.0;
      chol_solve_small(Lc, p, e.data(), col.data());
      for (int i = 0; i < p; ++i) vcov[i + j * p] = col[i];
    }
  }
  if (iters) *iters = it;
  return 0;
}

extern "C" int mk_glm_binomial(const double* y, const double* weights, const double* x, int64_t n, int32_t p,
                               double epsilon, int32_t maxit, double* coef, double* vcov, int32_t* iters,
                               int32_t device) {
  return mk_glm_binomial_link(y, weights, x, n, p, MK_LINK_LOGIT, epsilon, maxit, coef, vcov, iters, device);
}
