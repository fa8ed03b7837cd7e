// Posterior maps on the device (include/mk.h "posterior maps": per test column the mean and sd of w and
// of p(y = 1) and the probabilities that p exceeds the thresholds; per subset, and of a combined grid):
// the kernel, a session's thresholds and plane buffer, and the entry points.  Nothing here runs, and
// nothing is allocated, unless maps are asked for (or mk_map_grid is called).
//
// k_map_cols has k_score_cols' geometry and addressing: one thread owns one column c (a test site x
// outcome) of one subset and walks its n states in time order.  The session form reads the kriging draw
// w_kc -- row k of the draw buffer, so the threads of a workgroup read consecutive doubles of one row --
// and makes eta_kc (pred_eta) and p_kc (pred_linkinv) from it, so p is the p of the p draws bit for bit.
// The grid form reads the value.  Per value it carries the running sum (the mean is pmean's own
// expression) and a Welford pair (mean, M2) for the sd, and MK_MAP_MAXT exceedance counters, all in
// registers: the thresholds come by value with the unused slots at +inf, so the counting loop has a fixed
// trip count and no register array is indexed at run time.  A column is one thread's serial work: nothing
// in it depends on the tile, the stream group or the workgroup it ran in, and no sum runs over columns, so
// there is no finish kernel.  The draws are read once: 8 n C bytes per subset, 8 (4 + J) C written.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <string>
#include "mk_session.hpp"

namespace mk {

// Grid (ceil(n_cols / 256), S).  State k of column c of subset s is data[s * subset_stride + k * row_stride +
// c * col_stride], as k_score_cols addresses it.  planes: [S][NB + J][C] with NB = 4 (session form: w_mean,
// w_sd, p_mean, p_sd) or 2 (grid form: mean, sd), then exc_1..J; the column is col0 + c of them.
// ps (session form): as k_chain_diag_prob takes it.
template <bool GRID>
__global__ __launch_bounds__(256) void k_map_cols(const double* __restrict__ data, long subset_stride, long row_stride,
                                                  long col_stride, int n, int n_cols, ProbSrc ps, MapThr th, long col0,
                                                  long C, double* __restrict__ planes) {
  constexpr int NB = GRID ? 2 : MK_N_MAP_BASE;
  const int s = blockIdx.y;
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_cols) return;
  const double* src = data + (long)s * subset_stride + c * col_stride;
  const double* beta = GRID ? nullptr : ps.samples + (long)s * ps.subset_stride;
  const double* xrow = GRID ? nullptr : ps.x + ps.x_off + c;
  double sw = 0.0, mw = 0.0, qw = 0.0, sp = 0.0, mp = 0.0, qp = 0.0;
  int cnt[MK_MAP_MAXT];
#pragma unroll
  for (int j = 0; j < MK_MAP_MAXT; ++j) cnt[j] = 0;
  bool bad = false;
  for (int k = 0; k < n; ++k) {
    const double v = src[(long)k * row_stride];
    const double dk = (double)(k + 1);
    double p;
    if (GRID) {
      p = v;
      bad = bad || !isfinite(v);
    } else {
      const double eta = pred_eta(xrow, ps.ldx, beta + (long)k * ps.row_stride, ps.p, v);
      p = pred_linkinv(eta, ps.link);
      bad = bad || !isfinite(v) || !isfinite(eta);
      map_update(sw, mw, qw, v, dk);
    }
    map_update(sp, mp, qp, p, dk);
#pragma unroll
    for (int j = 0; j < MK_MAP_MAXT; ++j) cnt[j] += p > th.u[j] ? 1 : 0;
  }
  const double dn = (double)n;
  double* o = planes + (long)s * (NB + th.J) * C + col0 + c;
  if (!GRID) {
    o[0] = bad ? NAN : sw / dn;
    o[C] = (bad || n < 2) ? NAN : sqrt(qw / (dn - 1.0));
  }
  o[(NB - 2) * C] = bad ? NAN : sp / dn;
  o[(NB - 1) * C] = (bad || n < 2) ? NAN : sqrt(qp / (dn - 1.0));
#pragma unroll
  for (int j = 0; j < MK_MAP_MAXT; ++j)
    if (j < th.J) o[(NB + j) * C] = bad ? NAN : (double)cnt[j] / dn;
}

}  // namespace mk

using namespace mk;

// ------------------------------------------------------------------ host side
namespace {
const SinkWords kWords = {"null session/maps", "no posterior maps asked for (mk_session_set_maps)",
                          "posterior maps need all n.samples iterations", "posterior maps", "the maps were attached"};

// The session form of k_map_cols on the draws in md.w_pred ([S][n][Ct], test row t0 * q first) into
// planes ([S][4 + J][C]), timed as KS_MAPS.  Returns after the stream is idle.
int session_maps(mk_session* s, int t0, int n, long Ct, double* planes) {
  const Model& md = s->md;
  const long C = (long)s->q * s->n_test_all;
  hipStream_t st = s->stream;
  const ProbSrc ps = prob_src(s, t0);
  EventTimer t;
  int rc = t.start(st);
  if (rc) return rc;
  MK_LAUNCH(k_map_cols<false>, dim3((unsigned)((Ct + 255) / 256), s->S), dim3(256), 0, st, (const double*)md.w_pred,
            (long)n * Ct, Ct, 1L, n, (int)Ct, ps, s->maps.th, (long)t0 * s->q, C, planes);
  HIPCHK(hipGetLastError());
  if ((rc = t.stop(st))) return rc;
  HIPCHK(hipStreamSynchronize(st));
  return t.price(s, KS_MAPS, 1);
}
}  // namespace

int mk::launch_map_values(hipStream_t st, const double* data, long subset_stride, long row_stride, int n, int n_cols,
                          int S, const MapThr& th, double* planes) {
  MK_LAUNCH(k_map_cols<true>, dim3((unsigned)((n_cols + 255) / 256), S), dim3(256), 0, st, data, subset_stride, row_stride,
            1L, n, n_cols, ProbSrc{}, th, 0L, (long)n_cols, planes);
  HIPCHK(hipGetLastError());
  return 0;
}

int mk::map_thresholds(const double* thresholds, int J, MapThr* th) {
  if (J < 0 || J > MK_MAP_MAXT)
    return set_err(MK_E_ARG, "posterior maps: n_thresholds = " + std::to_string(J) + " is outside 0 .. " +
                                 std::to_string(MK_MAP_MAXT));
  if (J > 0 && !thresholds) return set_err(MK_E_ARG, "posterior maps: null thresholds with n_thresholds > 0");
  for (int j = 0; j < MK_MAP_MAXT; ++j) {
    if (j < J && !std::isfinite(thresholds[j]))
      return set_err(MK_E_ARG, "posterior maps: threshold " + std::to_string(j) + " is " + std::to_string(thresholds[j]) +
                                   "; every threshold must be finite");
    th->u[j] = j < J ? thresholds[j] : INFINITY;
  }
  th->J = J;
  return 0;
}

int mk::map_spec_check(const double* thresholds, int J) {
  MapThr th{};
  return map_thresholds(thresholds, J, &th);
}

void mk::maps_detach(mk_session* s) {
  s->release(s->maps.planes);
  s->maps = Maps{};
}

int mk::tile_maps(mk_session* s, int t0, int n_kept, int Ct) {
  Maps& m = s->maps;
  if (!s->d_xt) return set_err(MK_E_ARG, "posterior maps need x_test");
  m.fill.begin(s->win_lo, n_kept);
  const int rc = session_maps(s, t0, n_kept, Ct, m.planes);
  if (rc) return rc;
  m.fill.mark(t0);
  return 0;
}

extern "C" int mk_session_set_maps(mk_session* s, const mk_map_spec* spec) {
  if (!s) return set_err(MK_E_ARG, "null session");
  MapThr th{};
  if (spec) {   // before any device is touched
    const int rc = map_thresholds(spec->thresholds, spec->n_thresholds, &th);
    if (rc) return rc;
  }
  MK_ENTRY_DEVICE(s->device);
  HIPCHK(hipStreamSynchronize(s->stream));
  maps_detach(s);
  if (!spec) return 0;
  if (s->n_test_all < 1) return set_err(MK_E_ARG, "posterior maps need test sites: the session has none");
  if (!s->d_xt) return set_err(MK_E_ARG, "posterior maps need x_test (mk_problem.x_test or mk_session_set_test_covars)");
  if (!s->md.samples) return set_err(MK_E_ARG, "posterior maps read beta from the recorded samples (record_samples = 0)");
  Maps& m = s->maps;
  if (s->tiled) {
    const size_t n = (size_t)s->S * (MK_N_MAP_BASE + th.J) * s->q * s->n_test_all;
    const int rc = s->alloc(&m.planes, n);
    if (rc) {
      maps_detach(s);
      if (rc == MK_E_NOMEM)
        return sink_nomem("the posterior-map planes (" + std::to_string(8 * (MK_N_MAP_BASE + th.J)) +
                              " bytes per subset and test column: ",
                          n * 8, "do not", "a budget MK_KRIG_MEM_GB, or fewer thresholds leave room");
      return rc;
    }
    m.fill.attach(s->n_test_all, s->pred_tile);
  }
  m.th = th;
  m.on = true;
  return 0;
}

extern "C" int mk_session_maps(mk_session* s, mk_maps* o) {
  int rc = results_entry(s, o, &mk_session::maps, kWords);
  if (rc) return rc;
  Maps& m = s->maps;
  MK_ENTRY_DEVICE(s->device);
  const long C = (long)s->q * s->n_test_all;
  const size_t len = (size_t)s->S * (MK_N_MAP_BASE + m.th.J) * C;
  hipStream_t st = s->stream;
  DevBufs scratch;
  double* d_planes = m.planes;
  if (!s->tiled) {   // the fused draws [S][n_kept][C], every kept state
    d_planes = scratch.get<double>(len);
    if (!d_planes) return set_err(MK_E_NOMEM, "posterior-map scratch");
    if ((rc = session_maps(s, 0, s->md.n_kept, C, d_planes))) return rc;
  }
  // [S][4 + J][C] == per subset (q n_test) x (4 + J) column-major
  if (o->subsets) HIPCHK(hipMemcpyAsync(o->subsets, d_planes, len * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int mk_map_grid(const double* grid, int32_t n_rows, int64_t n_cols, const double* thresholds,
                           int32_t n_thresholds, double* out, int32_t device) {
  if (!grid || !out) return set_err(MK_E_ARG, "null grid/out");
  if (n_rows < 1) return set_err(MK_E_ARG, "n_rows must be >= 1");
  if (n_cols < 1 || n_cols > 0x7fffffffL) return set_err(MK_E_ARG, "n_cols must be 1 .. 2^31 - 1");
  MapThr th{};
  int rc = map_thresholds(thresholds, n_thresholds, &th);
  if (rc) return rc;
  const long chunk = col_chunk("MK_MAP_CHUNK", n_rows, (long)n_cols);
  MK_ENTRY_DEVICE(device);
  const size_t len = (size_t)(2 + th.J) * n_cols;
  DevBufs bufs;
  double* d_g = bufs.get<double>((size_t)chunk * n_rows);
  double* d_out = bufs.get<double>(len);
  if (!d_g || !d_out) return set_err(MK_E_NOMEM, "map grid buffers");
  rc = upload_col_chunks(grid, n_rows, (long)n_cols, chunk, d_g, [&](long c0, long nc) {
    MK_LAUNCH(k_map_cols<true>, dim3((unsigned)((nc + 255) / 256), 1), dim3(256), 0, (hipStream_t)0, (const double*)d_g, 0L,
              1L, (long)n_rows, (int)n_rows, (int)nc, ProbSrc{}, th, c0, (long)n_cols, d_out);
  });
  if (rc) return rc;
  HIPCHK(hipMemcpy(out, d_out, len * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}
