// Cross-outcome prediction on the device (include/mk.h "cross-outcome prediction": per test site and pair
// of outcomes (a, b) the draws both = p_a p_b and diff = p_a - p_b of every kept state, their 200-level
// grids, and the planes both_mean, both_sd, diff_mean, diff_sd, corr, a_gt_b, joint_1..J): the two kernels,
// a session's thresholds and buffers, and the entry points.  Nothing here runs, and nothing is allocated,
// unless pairs are asked for.
//
// Both kernels read the kriging draw buffer as the per-column kernels do -- row k of subset s is the draw
// of the window's k-th kept state, Ct = q x sites doubles -- and make p of the pair's two columns t q + a
// and t q + b with pred_prob / pred_eta + pred_linkinv, so p is the p of the p draws bit for bit.  The
// product is __dmul_rn, the difference __dsub_rn: one rounding each whatever the contraction setting, the
// same in the sort and in the planes.  No buffer of pair draws exists.
//
// k_quantiles_pair has k_quantiles_prob's shape: one 256-thread workgroup per (subset, pair column) and
// quant_pow2(n_rows) doubles of dynamic LDS, which it fills, sorts and reads out (quant_sort_readout) twice,
// for both and then for diff; p is recomputed for the second fill (two pred_prob per row against the
// log^2 passes of the sort).
// k_pair_cols has k_map_cols' geometry: one thread per (subset, pair column) walks the states in time
// order with everything in registers -- the two running sums and Welford pairs of both and diff, the
// marginal Welford pairs of p_a and p_b with their co-moment, and 1 + MK_MAP_MAXT counters; the thresholds
// come by value with the unused slots at +inf, so the counting loop has a fixed trip count.  Nothing is
// summed over columns: there is no finish kernel.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <string>
#include "mk_session.hpp"

namespace mk {

// Pair r of q outcomes in the order for a in 0..q-2: for b in a+1..q-1.
__device__ inline void pair_ab(int q, int r, int& a, int& b) {
  a = 0;
  while (r >= q - 1 - a) {
    r -= q - 1 - a;
    ++a;
  }
  b = a + 1 + r;
}

// Grid S * n_pc, dynamic LDS quant_pow2(n_rows) doubles.  Pair column e of the block (n_pc = n_pairs x the
// block's sites) is site e / n_pairs, pair e % n_pairs; its two draw columns are data[s * subset_stride +
// k * row_stride + t q + {a, b}].  out: [S][2][C2][n_probs], both then diff; the column is col0 + e of C2.
// Padding rows (r >= n_rows) are +INFINITY and read nothing.
__global__ __launch_bounds__(256) void k_quantiles_pair(const double* __restrict__ data, long subset_stride,
                                                        long row_stride, int n_rows, int n_pc, int q,
                                                        const double* __restrict__ probs, int n_probs, ProbSrc ps,
                                                        long col0, long C2, double* __restrict__ out) {
  extern __shared__ double v[];
  const int s = blockIdx.x / n_pc, e = blockIdx.x % n_pc;
  const int n_pairs = q * (q - 1) / 2;
  int a, b;
  pair_ab(q, e % n_pairs, a, b);
  const long ca = (long)(e / n_pairs) * q + a, cb = ca + (b - a);
  const double* src = data + (long)s * subset_stride;
  const double* beta = ps.samples + (long)s * ps.subset_stride;
  const double* xa = ps.x + ps.x_off + ca;
  const double* xb = ps.x + ps.x_off + cb;
  const int n2 = quant_pow2(n_rows);
  for (int f = 0; f < 2; ++f) {
    for (int r = threadIdx.x; r < n2; r += 256) {
      double x = INFINITY;
      if (r < n_rows) {
        const double* bt = beta + (long)r * ps.row_stride;
        const double* row = src + (long)r * row_stride;
        const double pa = pred_prob(xa, ps.ldx, bt, ps.p, row[ca], ps.link);
        const double pb = pred_prob(xb, ps.ldx, bt, ps.p, row[cb], ps.link);
        x = f == 0 ? __dmul_rn(pa, pb) : __dsub_rn(pa, pb);
      }
      v[r] = x;
    }
    __syncthreads();
    quant_sort_readout(v, n2, n_rows, probs, n_probs, out + (((long)s * 2 + f) * C2 + col0 + e) * n_probs);
    __syncthreads();   // the read-out is done before the refill
  }
}

// Grid (ceil(n_pc / 256), S).  Addressing as k_quantiles_pair.  planes: [S][MK_N_PAIR_BASE + J][C2]; the
// column is col0 + e.
__global__ __launch_bounds__(256) void k_pair_cols(const double* __restrict__ data, long subset_stride, long row_stride,
                                                   int n, int n_pc, int q, ProbSrc ps, MapThr th, long col0, long C2,
                                                   double* __restrict__ planes) {
  const int s = blockIdx.y;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_pc) return;
  const int n_pairs = q * (q - 1) / 2;
  int a, b;
  pair_ab(q, (int)(e % n_pairs), a, b);
  const long ca = (e / n_pairs) * q + a, cb = ca + (b - a);
  const double* src = data + (long)s * subset_stride;
  const double* beta = ps.samples + (long)s * ps.subset_stride;
  const double* xa = ps.x + ps.x_off + ca;
  const double* xb = ps.x + ps.x_off + cb;
  double sb = 0.0, mb = 0.0, qb = 0.0, sd = 0.0, md = 0.0, qd = 0.0;   // both, diff
  double ma = 0.0, Ma = 0.0, mbb = 0.0, Mb = 0.0, co = 0.0;            // p_a, p_b and their co-moment
  int gt = 0;
  int cnt[MK_MAP_MAXT];
#pragma unroll
  for (int j = 0; j < MK_MAP_MAXT; ++j) cnt[j] = 0;
  bool bad = false;
  for (int k = 0; k < n; ++k) {
    const double* bt = beta + (long)k * ps.row_stride;
    const double* row = src + (long)k * row_stride;
    const double wa = row[ca], wb = row[cb];
    const double ea = pred_eta(xa, ps.ldx, bt, ps.p, wa), eb = pred_eta(xb, ps.ldx, bt, ps.p, wb);
    const double pa = pred_linkinv(ea, ps.link), pb = pred_linkinv(eb, ps.link);
    bad = bad || !isfinite(wa) || !isfinite(wb) || !isfinite(ea) || !isfinite(eb);
    const double dk = (double)(k + 1);
    map_update(sb, mb, qb, __dmul_rn(pa, pb), dk);
    map_update(sd, md, qd, __dsub_rn(pa, pb), dk);
    const double da = pa - ma;   // p_a - m_a,old
    ma = ma + da / dk;
    Ma = Ma + da * (pa - ma);
    const double db = pb - mbb;
    mbb = mbb + db / dk;
    Mb = Mb + db * (pb - mbb);
    co = co + da * (pb - mbb);   // (p_a - m_a,old) (p_b - m_b,new)
    gt += pa > pb ? 1 : 0;
#pragma unroll
    for (int j = 0; j < MK_MAP_MAXT; ++j) cnt[j] += (pa > th.u[j] && pb > th.u[j]) ? 1 : 0;
  }
  const double dn = (double)n;
  double* o = planes + (long)s * (MK_N_PAIR_BASE + th.J) * C2 + col0 + e;
  const bool one = bad || n < 2;
  o[0] = bad ? NAN : sb / dn;
  o[C2] = one ? NAN : sqrt(qb / (dn - 1.0));
  o[2 * C2] = bad ? NAN : sd / dn;
  o[3 * C2] = one ? NAN : sqrt(qd / (dn - 1.0));
  o[4 * C2] = (one || Ma == 0.0 || Mb == 0.0) ? NAN : co / (sqrt(Ma) * sqrt(Mb));
  o[5 * C2] = bad ? NAN : (double)gt / dn;
#pragma unroll
  for (int j = 0; j < MK_MAP_MAXT; ++j)
    if (j < th.J) o[(MK_N_PAIR_BASE + j) * C2] = bad ? NAN : (double)cnt[j] / dn;
}

}  // namespace mk

using namespace mk;

// ------------------------------------------------------------------ host side
namespace {
const SinkWords kWords = {"null session/pairs", "no cross-outcome prediction asked for (mk_session_set_pairs)",
                          "cross-outcome prediction needs all n.samples iterations", "cross-outcome prediction",
                          "the pairs were attached"};

long n_pairs_of(const mk_session* s) { return (long)s->q * (s->q - 1) / 2; }

// The pair kernels on the draws in md.w_pred ([S][n][Ct], test site t0 first): k_quantiles_pair into grids
// ([S][2][C2][200]) and k_pair_cols into planes ([S][6 + J][C2]), either of which may be NULL, timed as
// KS_PAIRS (one launch per kernel).  Returns after the stream is idle.
int session_pairs(mk_session* s, int t0, int n, long Ct, double* grids, double* planes) {
  const Model& md = s->md;
  const long np = n_pairs_of(s), C2 = np * s->n_test_all;
  const long n_pc = Ct / s->q * np, col0 = (long)t0 * np;
  if (col0 + n_pc > C2) return set_err(MK_E_ARG, "cross-outcome prediction: the tile lies outside the test sites");
  hipStream_t st = s->stream;
  const ProbSrc ps = prob_src(s, t0);
  if (grids) {
    HIPCHK(hipFuncSetAttribute((const void*)k_quantiles_pair, hipFuncAttributeMaxDynamicSharedMemorySize, MK_QUANT_MAX * 8));
    if (n < 1 || n > MK_QUANT_MAX)
      return set_err(MK_E_ARG, "quantile summaries take 1 .. " + std::to_string(MK_QUANT_MAX) + " kept samples");
  }
  EventTimer t;
  int rc = t.start(st), kernels = 0;
  if (rc) return rc;
  if (grids) {
    size_t n2 = 1;
    while (n2 < (size_t)n) n2 <<= 1;
    MK_LAUNCH(k_quantiles_pair, dim3((unsigned)(s->S * n_pc)), dim3(256), n2 * 8, st, (const double*)md.w_pred, (long)n * Ct,
              Ct, n, (int)n_pc, s->q, (const double*)s->d_probs, MK_N_LEVELS, ps, col0, C2, grids);
    HIPCHK(hipGetLastError());
    ++kernels;
  }
  if (planes) {
    MK_LAUNCH(k_pair_cols, dim3((unsigned)((n_pc + 255) / 256), s->S), dim3(256), 0, st, (const double*)md.w_pred,
              (long)n * Ct, Ct, n, (int)n_pc, s->q, ps, s->pairs.th, col0, C2, planes);
    HIPCHK(hipGetLastError());
    ++kernels;
  }
  if ((rc = t.stop(st))) return rc;
  HIPCHK(hipStreamSynchronize(st));
  return t.price(s, KS_PAIRS, kernels);
}
}  // namespace

int mk::pair_spec_check(const mk_pair_spec* spec, int q) {
  if (!spec) return set_err(MK_E_ARG, "cross-outcome prediction needs a pair spec");
  const int rc = map_spec_check(spec->thresholds, spec->n_thresholds);
  if (rc) return rc;
  if (q < 2)
    return set_err(MK_E_ARG, "cross-outcome prediction needs q >= 2 outcomes: a q = " + std::to_string(q) + " fit has no pair");
  return 0;
}

void mk::pairs_detach(mk_session* s) {
  s->release(s->pairs.grids);
  s->release(s->pairs.planes);
  s->pairs = Pairs{};
}

int mk::tile_pairs(mk_session* s, int t0, int n_kept, int Ct) {
  Pairs& m = s->pairs;
  if (!s->d_xt) return set_err(MK_E_ARG, "cross-outcome prediction needs x_test");
  m.fill.begin(s->win_lo, n_kept);
  const int rc = session_pairs(s, t0, n_kept, Ct, m.grids, m.planes);
  if (rc) return rc;
  m.fill.mark(t0);
  return 0;
}

extern "C" int mk_session_set_pairs(mk_session* s, const mk_pair_spec* spec) {
  if (!s) return set_err(MK_E_ARG, "null session");
  MapThr th{};
  if (spec) {   // before any device is touched; nothing can be attached in a state these refuse
    int rc = pair_spec_check(spec, s->q);
    if (rc || (rc = map_thresholds(spec->thresholds, spec->n_thresholds, &th))) return rc;
    if (s->n_test_all < 1) return set_err(MK_E_ARG, "cross-outcome prediction needs test sites: the session has none");
    if (!s->d_xt)
      return set_err(MK_E_ARG, "cross-outcome prediction needs x_test (mk_problem.x_test or mk_session_set_test_covars)");
    if (!s->md.samples)
      return set_err(MK_E_ARG, "cross-outcome prediction reads beta from the recorded samples (record_samples = 0)");
  }
  MK_ENTRY_DEVICE(s->device);
  HIPCHK(hipStreamSynchronize(s->stream));
  pairs_detach(s);
  if (!spec) return 0;
  Pairs& m = s->pairs;
  if (s->tiled) {
    const size_t C2 = (size_t)n_pairs_of(s) * s->n_test_all;
    const size_t ng = (size_t)s->S * 2 * C2 * MK_N_LEVELS, npl = (size_t)s->S * (MK_N_PAIR_BASE + th.J) * C2;
    int rc = s->alloc(&m.grids, ng);
    if (!rc) rc = s->alloc(&m.planes, npl);
    if (rc) {
      pairs_detach(s);
      if (rc == MK_E_NOMEM)
        return sink_nomem("the pair grids and planes (" + std::to_string(16 * MK_N_LEVELS + 8 * (MK_N_PAIR_BASE + th.J)) +
                              " bytes per subset and pair column: ",
                          (ng + npl) * 8, "do not", "a budget MK_KRIG_MEM_GB, or fewer test sites per call leave room");
      return rc;
    }
    m.fill.attach(s->n_test_all, s->pred_tile);
  }
  m.th = th;
  m.on = true;
  return 0;
}

extern "C" int mk_session_pairs(mk_session* s, mk_pairs* o) {
  int rc = results_entry(s, o, &mk_session::pairs, kWords);
  if (rc) return rc;
  Pairs& m = s->pairs;
  MK_ENTRY_DEVICE(s->device);
  const long C2 = n_pairs_of(s) * s->n_test_all;
  const size_t G = (size_t)C2 * MK_N_LEVELS, npl = (size_t)(MK_N_PAIR_BASE + m.th.J) * C2;
  hipStream_t st = s->stream;
  const bool want_g = o->both_predict || o->diff_predict;
  DevBufs scratch;
  double* d_grids = m.grids;
  double* d_planes = m.planes;
  if (!s->tiled) {   // the fused draws [S][n_kept][q n_test], every kept state: what is asked for, now
    d_grids = want_g ? scratch.get<double>((size_t)s->S * 2 * G) : nullptr;
    d_planes = o->planes ? scratch.get<double>((size_t)s->S * npl) : nullptr;
    if ((want_g && !d_grids) || (o->planes && !d_planes)) return set_err(MK_E_NOMEM, "cross-outcome scratch");
    if ((d_grids || d_planes) && (rc = session_pairs(s, 0, s->md.n_kept, (long)s->q * s->n_test_all, d_grids, d_planes)))
      return rc;
  }
  // [S][2][C2][200]: per subset and functional 200 x C2 column-major
  double* const h[2] = {o->both_predict, o->diff_predict};
  for (int f = 0; f < 2; ++f)
    if (h[f])
      for (int i = 0; i < s->S; ++i)
        HIPCHK(hipMemcpyAsync(h[f] + (size_t)i * G, d_grids + ((size_t)i * 2 + f) * G, G * 8, hipMemcpyDeviceToHost, st));
  if (o->planes) HIPCHK(hipMemcpyAsync(o->planes, d_planes, (size_t)s->S * npl * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}
