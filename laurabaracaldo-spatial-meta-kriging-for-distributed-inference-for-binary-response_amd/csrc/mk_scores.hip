// Held-out validation on the device (include/mk.h "held-out validation": log score, Brier score and
// error rate per subset, and of a combined grid of probabilities): the kernels, a session's data and
// pair buffer, and the entry points.  Nothing here runs, and nothing is allocated, unless validation
// data are attached (or mk_score_grid is called).
//
// k_score_cols: one thread owns one column c (a test site x outcome) of one subset and walks its n
// states in time order.  The session form reads the kriging draw w_kc -- row k of the draw buffer, so
// the threads of a workgroup read consecutive doubles of one row -- and makes eta_kc (pred_eta) and
// p_kc (pred_linkinv) from it: pred_prob's two halves, so p is the p of the p draws bit for bit.  The grid
// form reads p_kc.  Per column it keeps the running sum of p and the streaming log-sum-exp of the
// likelihood terms (score_lse: crit_update's running maximum and scaled sum, with -inf terms adding
// nothing) and writes the pair (pmean_c, lpd_c).  A column is one thread's serial work: nothing in it
// depends on the tile, the stream group or the workgroup it ran in.  The draws are read once: 8 n C bytes
// per subset, 16 C written.
// k_score_finish: one workgroup per subset; thread t adds columns t, t + 256, ... in turn, then the
// fixed tree of block_sum<256> -- an order fixed by C = q n_test alone.  The closing formulas are plain
// quotients (the library is built without FMA contraction).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <string>
#include "mk_session.hpp"

namespace mk {

// State k (0-based) with likelihood term l <= 0 into log sum_k exp(l_k) = mx + log(sm).  A term of -inf
// adds nothing; while every term so far was -inf, mx stays -inf and the sum is -inf whatever sm holds.
__device__ inline void score_lse(double& mx, double& sm, double l, int k) {
  if (k == 0) {
    mx = l;
    sm = 1.0;
  } else if (l > mx) {
    sm = fma(sm, exp(mx - l), 1.0);
    mx = l;
  } else if (l > -INFINITY) {
    sm = sm + exp(l - mx);
  }
}

// The grid form's likelihood term at probability p: y log p + (wt - y) log1p(-p), a term whose
// multiplier is 0 contributing 0.
__device__ inline double score_loglik_p(double y, double wt, double p) {
  const double a = y > 0.0 ? y * log(p) : 0.0;
  const double b = wt - y > 0.0 ? (wt - y) * log1p(-p) : 0.0;
  return a + b;
}

// Grid (ceil(n_cols / 256), S).  State k of column c of subset s is data[s * subset_stride + k * row_stride +
// c * col_stride]: a draw buffer [S][n][n_cols] has col_stride 1; a column-major n x n_cols matrix of p has
// row_stride 1 and col_stride n.  y, wt: [C]; the column is col0 + c of them and of the planes of pw
// ([S][2][C]: pmean, lpd).  ps (session form): as k_chain_diag_prob takes it.
template <bool GRID>
__global__ __launch_bounds__(256) void k_score_cols(const double* __restrict__ data, long subset_stride, long row_stride,
                                                    long col_stride, int n, int n_cols, ProbSrc ps,
                                                    const double* __restrict__ y, const double* __restrict__ wt, long col0,
                                                    long C, double* __restrict__ pw) {
  const int s = blockIdx.y;
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cols) return;
  const double* src = data + (long)s * subset_stride + c * col_stride;
  const double* beta = GRID ? nullptr : ps.samples + (long)s * ps.subset_stride;
  const double* xrow = GRID ? nullptr : ps.x + ps.x_off + c;
  const double yv = y[col0 + c], wv = wt[col0 + c];
  double sp = 0.0, mx = 0.0, sm = 0.0;
  bool bad = false;
  for (int k = 0; k < n; ++k) {
    const double v = src[(long)k * row_stride];
    double p, l;
    if (GRID) {
      p = v;
      l = score_loglik_p(yv, wv, p);
      bad = bad || !isfinite(p);
    } else {
      const double eta = pred_eta(xrow, ps.ldx, beta + (long)k * ps.row_stride, ps.p, v);
      p = pred_linkinv(eta, ps.link);
      l = loglik_term(yv, wv, eta, ps.link);
      bad = bad || !isfinite(eta);
    }
    bad = bad || l != l;
    sp = sp + p;
    score_lse(mx, sm, l, k);
  }
  const double dn = (double)n;
  double* o = pw + (long)s * 2 * C + col0 + c;
  o[0] = bad ? NAN : sp / dn;
  o[C] = bad ? NAN : mx + log(sm) - log(dn);
}

// The MK_N_SCORE rows of subset blockIdx.x from its pairs pw [S][2][C] and the data y, wt [C].
__global__ __launch_bounds__(256) void k_score_finish(const double* __restrict__ pw, const double* __restrict__ y,
                                                      const double* __restrict__ wt, long C, double* __restrict__ rows) {
  __shared__ double red[8];
  const int s = blockIdx.x, tid = threadIdx.x;
  const double* pm = pw + (long)s * 2 * C;
  const double* lp = pm + C;
  double tn = 0.0, tl = 0.0, tb = 0.0, te = 0.0, tw = 0.0, tc = 0.0, tbad = 0.0;
  for (long c = tid; c < C; c += 256) {
    const double m = pm[c], l = lp[c], yv = y[c], wv = wt[c];
    tl = tl + l;
    tc = tc + (lgamma(wv + 1.0) - lgamma(yv + 1.0) - lgamma(wv - yv + 1.0));
    if (m != m || l != l) tbad = tbad + 1.0;
    if (wv > 0.0) {
      const double d = m - yv / wv;
      tn = tn + 1.0;
      tb = tb + d * d;
      te = te + (m >= 0.5 ? wv - yv : yv);
      tw = tw + wv;
    }
  }
  const double n = block_sum<256>(tn, red);
  const double lpd = block_sum<256>(tl, red);
  const double sq = block_sum<256>(tb, red);
  const double wrong = block_sum<256>(te, red);
  const double trials = block_sum<256>(tw, red);
  const double lconst = block_sum<256>(tc, red);
  const double bad = block_sum<256>(tbad, red);
  if (tid != 0) return;
  double* o = rows + (long)s * MK_N_SCORE;
  o[0] = n;
  o[1] = lpd;
  o[2] = sq / n;
  o[3] = wrong / trials;
  if (bad != 0.0) o[1] = o[2] = o[3] = NAN;
  o[4] = lconst;
}

}  // namespace mk

using namespace mk;

// ------------------------------------------------------------------ host side
namespace {
const SinkWords kWords = {"null session/scores", "no validation data attached (mk_session_set_validation)",
                          "held-out scores need all n.samples iterations", "held-out scores",
                          "the validation data were attached"};

// First index whose (y, wt) is not a count of successes in a count of trials, or -1.
long first_bad(const double* y, const double* wt, long C) {
  for (long c = 0; c < C; ++c)
    if (!std::isfinite(y[c]) || !std::isfinite(wt[c]) || wt[c] < 0.0 || y[c] < 0.0 || y[c] > wt[c]) return c;
  return -1;
}

int bad_entry(const double* y, const double* wt, long c) {
  return set_err(MK_E_ARG, "validation data: entry " + std::to_string(c) + " has y = " + std::to_string(y[c]) + ", wt = " +
                               std::to_string(wt[c]) + "; every entry must be finite with wt >= 0 and 0 <= y <= wt");
}

// The session form of k_score_cols on the draws in md.w_pred ([S][n][Ct], test row t0 * q first) into
// pw ([S][2][C]).  Not waited for.
int launch_session_cols(mk_session* s, int t0, int n, long Ct, double* pw) {
  const Model& md = s->md;
  const long C = (long)s->q * s->n_test_all;
  hipStream_t st = s->stream;
  const ProbSrc ps = prob_src(s, t0);
  MK_LAUNCH(k_score_cols<false>, dim3((unsigned)((Ct + 255) / 256), s->S), dim3(256), 0, st, (const double*)md.w_pred,
            (long)n * Ct, Ct, 1L, n, (int)Ct, ps, (const double*)s->val.y, (const double*)s->val.wt, (long)t0 * s->q, C, pw);
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace

void mk::validation_detach(mk_session* s) {
  Validation& v = s->val;
  s->release(v.y);
  s->release(v.wt);
  s->release(v.pw);
  v = Validation{};
}

int mk::tile_scores(mk_session* s, int t0, int n_kept, int Ct) {
  Validation& v = s->val;
  if (!s->d_xt) return set_err(MK_E_ARG, "held-out scores need x_test");
  v.fill.begin(s->win_lo, n_kept);
  EventTimer t;
  int rc = t.start(s->stream);
  if (!rc) rc = launch_session_cols(s, t0, n_kept, Ct, v.pw);
  if (!rc) rc = t.stop(s->stream);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(s->stream));
  if ((rc = t.price(s, KS_SCORE, 1))) return rc;
  v.fill.mark(t0);
  return 0;
}

extern "C" int mk_session_set_validation(mk_session* s, const mk_validation* val) {
  if (!s) return set_err(MK_E_ARG, "null session");
  MK_ENTRY_DEVICE(s->device);
  HIPCHK(hipStreamSynchronize(s->stream));
  validation_detach(s);
  if (!val) return 0;
  if (!val->y_test || !val->wt_test) return set_err(MK_E_ARG, "validation data need y_test and wt_test");
  if (s->n_test_all < 1) return set_err(MK_E_ARG, "validation data need test sites: the session has none");
  if (!s->d_xt)
    return set_err(MK_E_ARG, "validation data need x_test (mk_problem.x_test or mk_session_set_test_covars)");
  if (!s->md.samples) return set_err(MK_E_ARG, "held-out scores read beta from the recorded samples (record_samples = 0)");
  const long C = (long)s->q * s->n_test_all;
  const long b = first_bad(val->y_test, val->wt_test, C);
  if (b >= 0) return bad_entry(val->y_test, val->wt_test, b);
  Validation& v = s->val;
  int rc;
  if ((rc = s->alloc(&v.y, (size_t)C)) || (rc = s->alloc(&v.wt, (size_t)C)) ||
      (s->tiled && (rc = s->alloc(&v.pw, (size_t)s->S * 2 * C)))) {
    validation_detach(s);
    if (rc == MK_E_NOMEM)
      return sink_nomem("the held-out score buffer (16 bytes per subset and test column: ", (size_t)s->S * 2 * C * 8,
                        "does not", "or a budget MK_KRIG_MEM_GB, leaves room");
    return rc;
  }
  HIPCHK(hipMemcpy(v.y, val->y_test, (size_t)C * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(v.wt, val->wt_test, (size_t)C * 8, hipMemcpyHostToDevice));
  if (s->tiled) v.fill.attach(s->n_test_all, s->pred_tile);
  v.on = true;
  return 0;
}

extern "C" int mk_session_scores(mk_session* s, mk_scores* o) {
  int rc = results_entry(s, o, &mk_session::val, kWords);
  if (rc) return rc;
  const Model& md = s->md;
  Validation& v = s->val;
  MK_ENTRY_DEVICE(s->device);
  const int S = s->S;
  const long C = (long)s->q * s->n_test_all;
  hipStream_t st = s->stream;
  DevBufs scratch;
  double* d_rows = scratch.get<double>((size_t)S * MK_N_SCORE);
  double* d_pw = s->tiled ? v.pw : scratch.get<double>((size_t)S * 2 * C);
  if (!d_rows || !d_pw) return set_err(MK_E_NOMEM, "held-out score scratch");
  EventTimer t;
  if ((rc = t.start(st))) return rc;
  int launches = 1;
  if (!s->tiled) {   // the fused draws [S][n_kept][C], every kept state
    if ((rc = launch_session_cols(s, 0, md.n_kept, C, d_pw))) return rc;
    launches += 1;
  }
  MK_LAUNCH(k_score_finish, dim3(S), dim3(256), 0, st, (const double*)d_pw, (const double*)v.y, (const double*)v.wt, C, d_rows);
  HIPCHK(hipGetLastError());
  if ((rc = t.stop(st))) return rc;
  if (o->subsets) HIPCHK(hipMemcpyAsync(o->subsets, d_rows, (size_t)S * MK_N_SCORE * 8, hipMemcpyDeviceToHost, st));
  // [S][2][C] == per subset (q n_test) x 2 column-major
  if (o->pointwise) HIPCHK(hipMemcpyAsync(o->pointwise, d_pw, (size_t)S * 2 * C * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return t.price(s, KS_SCORE, launches);
}

extern "C" int mk_score_grid(const double* p, int32_t n_rows, int64_t n_cols, const double* y, const double* wt,
                             double* pointwise, double* row, int32_t device) {
  if (!p || !y || !wt) return set_err(MK_E_ARG, "null grid/validation data");
  if (n_rows < 1) return set_err(MK_E_ARG, "n_rows must be >= 1");
  if (n_cols < 1 || n_cols > 0x7fffffffL) return set_err(MK_E_ARG, "n_cols must be 1 .. 2^31 - 1");
  const long b = first_bad(y, wt, (long)n_cols);
  if (b >= 0) return bad_entry(y, wt, b);
  const long chunk = col_chunk("MK_SCORE_CHUNK", n_rows, (long)n_cols);
  MK_ENTRY_DEVICE(device);
  DevBufs bufs;
  double* d_p = bufs.get<double>((size_t)chunk * n_rows);
  double* d_y = bufs.get<double>((size_t)n_cols);
  double* d_wt = bufs.get<double>((size_t)n_cols);
  double* d_pw = bufs.get<double>((size_t)2 * n_cols);
  double* d_row = bufs.get<double>(MK_N_SCORE);
  if (!d_p || !d_y || !d_wt || !d_pw || !d_row) return set_err(MK_E_NOMEM, "score grid buffers");
  HIPCHK(hipMemcpy(d_y, y, (size_t)n_cols * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_wt, wt, (size_t)n_cols * 8, hipMemcpyHostToDevice));
  const int rc = upload_col_chunks(p, n_rows, (long)n_cols, chunk, d_p, [&](long c0, long nc) {
    MK_LAUNCH(k_score_cols<true>, dim3((unsigned)((nc + 255) / 256), 1), dim3(256), 0, (hipStream_t)0, (const double*)d_p, 0L,
              1L, (long)n_rows, (int)n_rows, (int)nc, ProbSrc{}, (const double*)d_y, (const double*)d_wt, c0, (long)n_cols,
              d_pw);
  });
  if (rc) return rc;
  MK_LAUNCH(k_score_finish, dim3(1), dim3(256), 0, (hipStream_t)0, (const double*)d_pw, (const double*)d_y,
            (const double*)d_wt, (long)n_cols, d_row);
  HIPCHK(hipGetLastError());
  if (pointwise) HIPCHK(hipMemcpy(pointwise, d_pw, (size_t)2 * n_cols * 8, hipMemcpyDeviceToHost));
  if (row) HIPCHK(hipMemcpy(row, d_row, MK_N_SCORE * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}
