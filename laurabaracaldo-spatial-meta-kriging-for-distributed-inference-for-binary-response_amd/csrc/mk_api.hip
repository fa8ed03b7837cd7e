// C ABI (include/mk.h) of a session: error state, device queries, create / run / destroy, getters,
// outputs and the shard interface.  The launch schedule is mk_schedule.hip, kriging mk_krig.hip, the
// stream pool mk_pool.hip; mk_session.hpp holds what they share.
//
// One mk_session = one GPU's shard of subsets resident in HBM.  The shard is split into
// contiguous subset groups, each advanced by its own HIP stream: a group's iteration is a
// fixed sequence of stream-ordered launches with no host synchronisation (data-dependent
// control -- which factors changed -- lives in device work lists), and the groups' streams
// overlap on the GPU, so one group's latency-bound steps (diagonal-tile factorisations,
// the MH decisions, launch tails) run beside another group's MFMA panel updates.  A group
// is a pointer view into the shard's arrays (every array is [subset][...]); the chains do
// not depend on the grouping (RNG streams are keyed by global subset index).
#include <hip/hip_runtime.h>
#include <dirent.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>
#include "mk_session.hpp"

using namespace mk;

static thread_local std::string g_err;

namespace mk {
int set_err(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int host_error(int code, const char* msg) { return set_err(code, msg); }   // for host-only sources

int results_ready(const mk_session* s, const SinkWords& w, bool on, const TileFill& fill) {
  if (s->poisoned) return poisoned_err(s);
  if (!on) return set_err(MK_E_ARG, w.off);
  if (s->iter < s->md.n_samples) return set_err(MK_E_ARG, w.need_iters);
  if (!s->tiled) return 0;
  // the buffer holds the window the tiles were last replayed over
  const long t = fill.first_missing(s->win_lo, s->win_n < 0 ? s->md.n_kept : s->win_n);
  return t < 0 ? 0 : set_err(MK_E_ARG, tile_missing_msg(w.what, w.attached, t, s->pred_tile, s->n_test_all));
}
}  // namespace mk

extern "C" const char* mk_last_error(void) { return g_err.c_str(); }

extern "C" int mk_hip_initialized(void) {
  DIR* d = opendir("/proc/self/fd");
  if (!d) return 0;
  int found = 0;
  char path[64], target[256];
  while (dirent* e = readdir(d)) {
    if (e->d_name[0] == '.') continue;
    std::snprintf(path, sizeof path, "/proc/self/fd/%s", e->d_name);
    const ssize_t n = readlink(path, target, sizeof target - 1);
    if (n <= 0) continue;
    target[n] = 0;
    if (std::strcmp(target, "/dev/kfd") == 0) {
      found = 1;
      break;
    }
  }
  closedir(d);
  return found;
}

extern "C" int mk_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" int mk_device_memory(int32_t device, int64_t* free_bytes, int64_t* total_bytes) {
  MK_ENTRY_DEVICE(device);
  size_t f = 0, t = 0;
  HIPCHK(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = (int64_t)f;
  if (total_bytes) *total_bytes = (int64_t)t;
  return 0;
}

namespace mk {

Model model_view(const Model& m, int s0, int S) {
  Model v = m;
  v.S = S;
  v.subset_base = m.subset_base + s0;
  const long q = m.q, np = m.n_pad, Np = m.Np, s = s0;
  v.n_s = m.n_s + s;
  v.coords = m.coords + s * 2 * np;
  v.y = m.y + s * Np;
  v.wt = m.wt + s * Np;
  v.X = m.X + s * m.p * Np;
  v.beta = m.beta + s * m.p;
  v.theta = m.theta + s * m.n_theta;
  v.w = m.w + s * Np;
  v.eta = m.eta + s * Np;
  v.tune = m.tune + s * m.n_mh_max;
  v.acc = m.acc + s * m.n_mh_max;
  v.u = m.u + s * q * np;
  v.z = m.z + s * q * np;
  v.Z = m.Z + s * q * q * np;
  v.logdetR = m.logdetR + s * q;
  v.quad = m.quad + s * q;
  v.A_full = m.A_full + s * q * q;
  v.Ainv = m.Ainv + s * q * q;
  v.dirty = m.dirty + s * q;
  v.ld_part = m.ld_part + (long)s * m.q * m.nt;   // per (subset, outcome) pair
  v.quad_c = m.quad_c + (long)s * m.q;
  v.info = m.info + (long)s * m.q;
  v.notpd = m.notpd + (long)s * m.q;
  v.sw_delta = m.sw_delta + s * Np;
  v.sw_dll = m.sw_dll + s * Np;
  v.sw_logu = m.sw_logu + s * Np;
  v.sw_acc = m.sw_acc + s * Np;
  v.samples = m.samples + s * m.n_samples * m.P;
  v.acc_hist = m.acc_hist + s * m.n_batch * (m.o_w + 1);
  if (m.w_samples) v.w_samples = m.w_samples + s * m.n_samples * Np;
  v.s_pred = m.s_pred + s * q * m.n_test_pad;
  v.s_part = m.s_part + s * q * m.nt * m.n_test_pad;
  if (m.PT) v.PT = m.PT + s * q * np * m.n_test_pad;
  if (m.XK) v.XK = m.XK + s * q * np * m.n_test_pad;
  v.w_pred = m.w_pred + s * m.n_kept * q * (long)std::max(m.n_test, 1);
  if (m.kz) v.kz = m.kz + s * q * np;
  if (m.kth) v.kth = m.kth + s * m.n_theta;
  if (m.kA) v.kA = m.kA + s * q * q;
  if (m.bacc) v.bacc = m.bacc + s * q * np;
  if (m.zc) v.zc = m.zc + s * q * np;
  if (m.la_nu) v.la_nu = m.la_nu + s * q;
  if (m.span) v.span = m.span + s;
  if (m.span_pt) v.span_pt = m.span_pt + s;
  if (m.chtab) v.chtab = m.chtab + s * q * MK_CH_TAB;
  if (m.chtab_p) v.chtab_p = m.chtab_p + s * q * MK_CH_TAB;
  return v;
}

MatSet matset_view(const MatSet& m, int s0) {
  MatSet v = m;
  const long sq = (long)s0 * m.q, e = (long)m.ld * m.ld, wt = (long)m.nt * MK_NB * MK_NB;
  v.L = m.L + sq * 2 * e;
  v.Winv = m.Winv + sq * 2 * wt;
  v.W = m.W + sq * e;
  if (m.Q) v.Q = m.Q + sq * e;
  if (m.QB) v.QB = m.QB + sq * wt;
  v.cur = m.cur + sq;
  if (m.Y) v.Y = m.Y + sq * e;
  return v;
}

}  // namespace mk

static std::atomic<int> g_live_sessions{0};

mk_session::mk_session() { g_live_sessions.fetch_add(1); }

// Teardown order: drain every stream first (no queued work may still reference an event or a
// buffer), then destroy the events the streams recorded, then the streams (CU-masked and
// priority queues included), then free the memory.
mk_session::~mk_session() {
  g_live_sessions.fetch_sub(1);
  if (device >= 0) hipSetDevice(device);
  for (auto& o : owned) hipStreamSynchronize(o.second);
  for (auto& t : prof.pending) { hipEventDestroy(t.a); hipEventDestroy(t.b); }
  for (auto& t : crit.pending) { hipEventDestroy(t.a); hipEventDestroy(t.b); }
  if (prof.inv_cnt) hipHostFree(prof.inv_cnt);
  for (auto& g : groups) {
    if (g.done) hipEventDestroy(g.done);
    for (hipEvent_t e : g.ev) hipEventDestroy(e);
  }
  if (swept) hipEventDestroy(swept);
  for (hipEvent_t e : cov.ev)
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : kt.ev)
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : la.ev) hipEventDestroy(e);
  pool_return(owned);   // drained above; their waits on the destroyed events are satisfied
  for (void* p_ : allocs) hipFree(p_);
  (void)hipGetLastError();   // teardown errors are not the next call's
}

// What no starting value can factor: a subset with a non-finite coordinate (R is NaN), or with two
// sites at the same place (rho(0) = 1 exactly: two equal rows, R singular at every phi and nu).  The
// device flag (initial_state) sees such a start only where the pivot comes out <= 0 or NaN; a
// duplicate deep in the ordering can leave a pivot of +1e-16 and a finite, meaningless factor.
// Sites sorted by (x, y) per subset; subsets are named by their global index.
static int check_sites(const mk_problem* pr) {
  long off = 0;
  std::vector<int> ord;
  for (int i = 0; i < pr->n_subsets; ++i) {
    const int ns = pr->n_part[i];
    const double *x = pr->coords + 2 * off, *y = x + ns;
    const std::string who = "subset " + std::to_string(pr->subset_base + i);
    for (int r = 0; r < ns; ++r)
      if (!std::isfinite(x[r]) || !std::isfinite(y[r]))
        return set_err(MK_E_ARG, who + ": site " + std::to_string(r) + " has a non-finite coordinate");
    ord.resize(ns);
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int a, int b) {
      return x[a] != x[b] ? x[a] < x[b] : (y[a] != y[b] ? y[a] < y[b] : a < b);
    });
    for (int k = 1; k < ns; ++k) {
      const int a = ord[k - 1], b = ord[k];
      if (x[a] == x[b] && y[a] == y[b])
        return set_err(MK_E_ARG, who + ": sites " + std::to_string(a) + " and " + std::to_string(b) +
                                     " have the same coordinates (a singular correlation matrix)");
    }
    off += ns;
  }
  return 0;
}

static int check_cfg(const mk_problem* pr, const mk_config* c) {
  if (!pr || !c) return set_err(MK_E_ARG, "null problem/config");
  if (pr->n_subsets < 1) return set_err(MK_E_ARG, "n_subsets must be >= 1");
  if (pr->q < 1 || pr->q > MK_QMAX) return set_err(MK_E_ARG, "q must be in [1, 4]");
  if (pr->p < 1) return set_err(MK_E_ARG, "p must be >= 1");
  if (!pr->n_part || !pr->coords || !pr->y || !pr->weights || !pr->x) return set_err(MK_E_ARG, "null data pointer");
  if (pr->n_test < 0 || (pr->n_test > 0 && !pr->coords_test)) return set_err(MK_E_ARG, "bad coords_test");
  if (pr->x_test && pr->n_test == 0) return set_err(MK_E_ARG, "x_test needs test sites (n_test = 0)");
  if (c->cov_model != MK_COV_EXPONENTIAL && c->cov_model != MK_COV_MATERN) return set_err(MK_E_ARG, "cov.model must be exponential or matern");
  if (c->n_batch < 1 || c->batch_length < 1) return set_err(MK_E_ARG, "n.batch and batch.length must be >= 1");
  const int n_samples = c->n_batch * c->batch_length;
  if (c->burn_in < 1 || c->burn_in > n_samples) return set_err(MK_E_ARG, "burn_in must be in [1, n.samples]");
  if (n_samples - c->burn_in + 1 > MK_QUANT_MAX)
    return set_err(MK_E_ARG, "at most " + std::to_string(MK_QUANT_MAX) + " kept samples supported");
  if (c->n_streams < 0 || c->n_streams > 8) return set_err(MK_E_ARG, "n_streams must be in [0, 8]");
  if (c->predict_tile < 0) return set_err(MK_E_ARG, "predict_tile must be >= 0");
  if (c->link != MK_LINK_LOGIT && c->link != MK_LINK_PROBIT) return set_err(MK_E_ARG, "link must be logit or probit");
  if (!c->beta_starting || !c->beta_tuning || !c->phi_starting || !c->phi_tuning || !c->A_starting || !c->A_tuning ||
      !c->phi_unif_a || !c->phi_unif_b || !c->K_IW_S)
    return set_err(MK_E_ARG, "null starting/tuning/prior array");
  if (c->cov_model == MK_COV_MATERN && (!c->nu_starting || !c->nu_tuning || !c->nu_unif_a || !c->nu_unif_b))
    return set_err(MK_E_ARG, "matern needs nu starting/tuning/prior");
  for (int i = 0; i < pr->n_subsets; ++i)
    if (pr->n_part[i] < 1) return set_err(MK_E_ARG, "every subset needs >= 1 site");
  for (int h = 0; h < pr->q; ++h) {
    if (!(c->phi_unif_a[h] < c->phi_starting[h] && c->phi_starting[h] < c->phi_unif_b[h]))
      return set_err(MK_E_ARG, "phi starting value outside phi.Unif support");
  }
  return check_sites(pr);
}

// Work lists for `ng` run groups + the whole-shard view (last): list/plist per pair, 2 counts per view.
int mk::setup_groups(mk_session* s, int n_groups) {
  const int S = s->S, q = s->q;
  const int G = std::max(1, std::min(n_groups, S));
  int *lists = nullptr, *counts = nullptr;
  int rc;
  if ((rc = s->alloc(&lists, (size_t)4 * S * q)) || (rc = s->alloc(&counts, (size_t)2 * (G + 1)))) return rc;
  s->all.md = s->md;
  s->all.ms = s->ms;
  s->all.stream = s->stream;
  s->all.S = S;
  s->all.s0 = 0;
  s->all.d_list = lists;
  s->all.d_plist = lists + S * q;
  s->all.d_count = counts + 2 * G;
  s->all.d_pcount = counts + 2 * G + 1;
  const int per = (S + G - 1) / G;
  for (int gi = 0; gi < G; ++gi) {
    const int s0 = gi * per, Sg = std::min(per, S - s0);
    if (Sg <= 0) break;
    Group g;
    g.S = Sg;
    g.s0 = s0;
    g.md = model_view(s->md, s0, Sg);
    g.ms = matset_view(s->ms, s0);
    g.d_list = lists + 2 * S * q + s0 * q;
    g.d_plist = lists + 3 * S * q + s0 * q;
    g.d_count = counts + 2 * gi;
    g.d_pcount = counts + 2 * gi + 1;
    if (G == 1) {
      g.stream = s->stream;
    } else if (pool_stream(s->owned, &g.stream, s->device, SK_PLAIN) != hipSuccess) {
      return set_err(MK_E_HIP, "group stream");
    }
    s->groups.push_back(g);
  }
  if (G > 1) {
    for (auto& g : s->groups)
      if (hipEventCreateWithFlags(&g.done, hipEventDisableTiming) != hipSuccess) return set_err(MK_E_HIP, "group event");
    if (hipEventCreateWithFlags(&s->swept, hipEventDisableTiming) != hipSuccess) return set_err(MK_E_HIP, "sweep event");
  }
  // Split Cholesky (launch_cholesky) for small shards on one stream: a bulk-update stream that
  // leaves the first `reserve` CUs (mask bits 0..reserve-1 = reserve/8 CUs on each XCD, measured
  // by tools/cumask_probe.hip) to the diagonal kernels: one CU per diagonal workgroup, 8..64.
  // MK_CHOL_SPLIT=0 / 1 forces it off / on.
  static const int split_env = env_int("MK_CHOL_SPLIT", -1);
  int n_cu = 0;
  if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess)
    return set_err(MK_E_HIP, "device attribute");
  const bool split = G == 1 && s->nt > 2 && (split_env == 1 || (split_env < 0 && (long)S * q * 4 <= n_cu));
  if (split) {
    const int reserve = std::max(8, std::min(64, round_up(S * q, 8)));
    std::vector<uint32_t> mask((n_cu + 31) / 32, 0xffffffffu);
    for (int b = 0; b < reserve && b < n_cu; ++b) mask[b / 32] &= ~(1u << (b % 32));
    Group& g = s->groups[0];
    if (pool_stream(s->owned, &g.bulk, s->device, SK_CUMASK, 0, mask) != hipSuccess)
      return set_err(MK_E_HIP, "bulk stream");
    g.ev.assign(2 * s->nt + 1, nullptr);
    for (auto& e : g.ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return set_err(MK_E_HIP, "cholesky event");
  }
  return 0;
}

// ------------------------------------------------------------------ mk_session_create, step by step
// Stream groups of a session: n_streams (0: one), at most one per subset.
static int group_count(const mk_config* c, int S) {
  return std::max(1, std::min(c->n_streams > 0 ? (int)c->n_streams : 1, S));
}

// CUs that the lookahead schedule's main stream leaves to the candidates' critical chain: MK_LA_MASK,
// by default 32 (4 per XCD, the split Cholesky's reserve) when the process has 8 hardware queues for
// the extra streams, else none (no masked stream).  The switch is read once per process.
static int la_mask_cus() {
  static const int mask_env = env_int("MK_LA_MASK", -1);
  return mask_env >= 0 ? mask_env : (hw_queues() >= 8 ? 32 : 0);
}

// Sizes, offsets, priors and the recording flags, from the problem and the configuration.
static void derive_dims(mk_session* s, const mk_problem* pr, const mk_config* c) {
  const int S = pr->n_subsets, q = pr->q, p = pr->p;
  s->S = S; s->q = q; s->p = p;
  s->matern = c->cov_model == MK_COV_MATERN;
  // MK_PRED_GEN=1: P^T generated inside the kriging GEMM (exponential; no P^T buffer, half the
  // kriging memory, but 0.52 vs 0.74 of fp64 peak: the exp/sqrt per element are recomputed for
  // every row panel).  Default: stored P^T.
  s->pred_gen = !s->matern && env_int("MK_PRED_GEN", 0) != 0;
  s->n_part.assign(pr->n_part, pr->n_part + S);
  s->bbox.assign((size_t)4 * S, 0.0);
  {
    long off = 0;
    for (int i = 0; i < S; ++i) {
      const int ns = pr->n_part[i];
      const double* cs = pr->coords + 2 * off;
      site_bbox(cs, cs + ns, ns, s->bbox.data() + 4 * i);
      off += ns;
    }
  }
  int nmax = 0;
  for (int i = 0; i < S; ++i) nmax = std::max(nmax, (int)pr->n_part[i]);
  const int n_pad = round_up(nmax + 1, MK_NB);
  const int nt = n_pad / MK_NB;
  s->n_pad = n_pad; s->nt = nt;
  const int Np = n_pad * q;
  const int ntri = q * (q + 1) / 2;
  const int n_theta = ntri + q * (s->matern ? 2 : 1);
  const int P = p + n_theta;
  s->P = P;
  const int o_w = p + n_theta;
  const int n_mh_max = o_w + Np;
  const int n_samples = c->n_batch * c->batch_length;
  const int kept0 = c->burn_in - 1;
  const int n_kept = n_samples - kept0;
  // tiled kriging: device kriging buffers hold one tile of test sites; all sites stay in HBM.
  // predict_tile > 0 without test sites records the kept states for a later
  // mk_session_set_test_sites (spPredict after spMvGLM without refitting).
  s->tiled = c->predict_tile > 0 && (pr->n_test == 0 || c->predict_tile < pr->n_test);
  s->tile_req = c->predict_tile;

  Model& md = s->md;
  md.S = S; md.q = q; md.p = p; md.n_pad = n_pad; md.Np = Np; md.nt = nt; md.ntri = ntri; md.n_theta = n_theta;
  md.cov_model = c->cov_model;
  md.link = c->link;
  md.o_A = p; md.o_phi = p + ntri; md.o_nu = p + ntri + q; md.o_w = o_w; md.n_mh_max = n_mh_max;
  md.n_batch = c->n_batch; md.batch_length = c->batch_length; md.n_samples = n_samples;
  md.kept0 = kept0; md.n_kept = n_kept;
  md.subset_base = pr->subset_base;
  md.S_all = S;
  md.t_off = 0;
  md.seed = c->seed;
  md.accept_rate = c->accept_rate;
  md.P = P;
  for (int h = 0; h < q; ++h) {
    md.phi_a[h] = c->phi_unif_a[h]; md.phi_b[h] = c->phi_unif_b[h];
    md.nu_a[h] = s->matern ? c->nu_unif_a[h] : 0.0;
    md.nu_b[h] = s->matern ? c->nu_unif_b[h] : 1.0;
  }
  md.iw_df = c->K_IW_df;
  for (int i = 0; i < q * q; ++i) md.iw_S[i] = c->K_IW_S[i];
  s->record_samples = true;   // needed on device for the parameter quantiles
  s->record_w = c->record_w != 0;
}

// The data, the chain state, the outputs, then the kriging buffers and the Matern table ranges, in
// this order: kriging_buffers halves a tile that does not fit in what the earlier allocations left.
static int alloc_chain_state(mk_session* s, const mk_problem* pr) {
  Model& md = s->md;
  const int S = s->S, q = s->q, p = s->p, n_pad = s->n_pad, nt = s->nt, P = s->P;
  const int Np = md.Np, n_theta = md.n_theta, n_mh_max = md.n_mh_max, o_w = md.o_w;
  const int n_samples = md.n_samples, n_kept = md.n_kept;
  int rc;
  int* d_ns; double *d_coords, *d_y, *d_wt, *d_X;
  if ((rc = s->alloc(&d_ns, S)) || (rc = s->alloc(&d_coords, (size_t)S * 2 * n_pad)) ||
      (rc = s->alloc(&d_y, (size_t)S * Np)) || (rc = s->alloc(&d_wt, (size_t)S * Np)) ||
      (rc = s->alloc(&d_X, (size_t)S * p * Np)))
    return rc;
  md.n_s = d_ns; md.coords = d_coords; md.y = d_y; md.wt = d_wt; md.X = d_X;
  if ((rc = s->alloc(&md.beta, (size_t)S * p)) || (rc = s->alloc(&md.theta, (size_t)S * n_theta)) ||
      (rc = s->alloc(&md.w, (size_t)S * Np)) || (rc = s->alloc(&md.eta, (size_t)S * Np)) ||
      (rc = s->alloc(&md.tune, (size_t)S * n_mh_max)) || (rc = s->alloc(&md.acc, (size_t)S * n_mh_max)) ||
      (rc = s->alloc(&md.u, (size_t)S * q * n_pad)) || (rc = s->alloc(&md.z, (size_t)S * q * n_pad)) ||
      (rc = s->alloc(&md.Z, (size_t)S * q * q * n_pad)) || (rc = s->alloc(&md.logdetR, (size_t)S * q)) ||
      (rc = s->alloc(&md.quad, (size_t)S * q)) || (rc = s->alloc(&md.A_full, (size_t)S * q * q)) ||
      (rc = s->alloc(&md.Ainv, (size_t)S * q * q)) || (rc = s->alloc(&md.dirty, (size_t)S * q)) ||
      (rc = s->alloc(&md.ld_part, (size_t)S * q * nt)) || (rc = s->alloc(&md.quad_c, (size_t)S * q)) ||
      (rc = s->alloc(&md.info, (size_t)S * q)) || (rc = s->alloc(&md.notpd, (size_t)S * q)) ||
      (rc = s->alloc(&md.sw_delta, (size_t)S * Np)) ||
      (rc = s->alloc(&md.sw_dll, (size_t)S * Np)) || (rc = s->alloc(&md.sw_logu, (size_t)S * Np)) ||
      (rc = s->alloc(&md.sw_acc, (size_t)S * Np)) || (rc = s->alloc(&md.samples, (size_t)S * n_samples * P)) ||
      (rc = s->alloc(&md.acc_hist, (size_t)S * md.n_batch * (o_w + 1))))
    return rc;
  if (s->record_w && (rc = s->alloc(&md.w_samples, (size_t)S * n_samples * Np))) return rc;
  if (s->tiled && ((rc = s->alloc(&md.kz, (size_t)n_kept * S * q * n_pad)) ||
                   (rc = s->alloc(&md.kth, (size_t)n_kept * S * n_theta)) ||
                   (rc = s->alloc(&md.kA, (size_t)n_kept * S * q * q)) ||
                   (rc = s->alloc(&s->d_slist, (size_t)q * S)) || (rc = s->alloc(&s->d_scount, (size_t)q))))
    return rc;
  if ((rc = kriging_buffers(s, pr->n_test, pr->coords_test))) return rc;
  {   // Matern candidate tables (k_cov_candidate): bounding-box diagonal of every subset
    double* d_span = nullptr;
    if ((rc = s->alloc(&d_span, (size_t)S))) return rc;
    std::vector<double> hs(S);
    for (int i = 0; i < S; ++i) hs[i] = matern_span(s->bbox.data() + 4 * i);
    HIPCHK(hipMemcpy(d_span, hs.data(), (size_t)S * 8, hipMemcpyHostToDevice));
    md.span = d_span;
    if (s->matern && ((rc = s->alloc(&md.chtab, (size_t)S * q * MK_CH_TAB)) ||
                      (rc = s->alloc(&md.chtab_p, (size_t)S * q * MK_CH_TAB))))
      return rc;
  }
  return 0;
}

// The latent sweep of this session (launch_sweep), into s->sweep.
// MK_SWEEP (tests and measurements): 1 the 64-site-block kernel (k_sweep: the fallback for subsets
// too large for the site sweep), 2 the multi-workgroup kernel (k_sweep_mg + the k_sweep fallback;
// where its grid fits the chip at once, else split launches), 3 split launches.
// 0 (default): the one-pass site sweep (k_sweep_site; W read once, no Q_BB tiles, no inter-workgroup
// waits) wherever it fits -- n_pad <= 4096 (q = 4: not instantiated) and the sites' data in LDS
// (configs[3]: n_s = 2,000, q = 3 takes 152 KB) -- except multi-outcome small shards (q >= 2, <= 16
// subsets: one workgroup per subset is the iteration's longest chain there), which take the
// multi-workgroup kernel on either schedule.
// Measured (subset-iters/s, 40-step windows, profiles/r04/knobs, r04e): configs[2] 250 subsets block
// sweep 10,143 / site pair 10,527; configs[1] 15,198 / 15,626; configs[3] (q = 3, 50 subsets) block
// 3,016 / site 3,106; configs[3]'s 7-subset share split launches 1,476 / site 1,340 / block 1,107
// (lookahead schedule).  q = 1 runs the lean pair form (k_sweep_site LN > 0: 250 subsets 10,452 ->
// 10,567-10,622, 32 subsets 7,832 -> 7,957-8,067).
static int plan_sweep(mk_session* s, const mk_config* c) {
  const int S = s->S, q = s->q, n_pad = s->n_pad, nt = s->nt;
  const int nmax = *std::max_element(s->n_part.begin(), s->n_part.end());
  int rc;
  HIPCHK(hipFuncSetAttribute(sweep_kernel(q, false), hipFuncAttributeMaxDynamicSharedMemorySize,
                             q * (64 * 64 + 2 * 64) * 8));
  s->sweep.mg_lds = (size_t)q * (64 * 64 + 2 * 64) * 8 + 4 * MK_NB * 8;
  const void* fn = sweep_kernel(q, true);
  HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->sweep.mg_lds));
  int per_cu = 0, n_cu = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, s->sweep.mg_lds));
  HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, s->device));
  const int mode = env_int("MK_SWEEP", 0);
  // the whole grid fits at once (else admission would mostly fall back) -- on the CUs the sweep's
  // stream may use: a one-group session can run the lookahead schedule, whose main stream leaves
  // la_mask_cus() CUs to the candidates' chain
  const int la_mask = group_count(c, S) == 1 ? la_mask_cus() : 0;
  const bool coop_fits = (long)xcd_grid(S, nt) <= (long)per_cu * std::max(1, n_cu - la_mask) && nt <= 32;
  const bool small_multi = q >= 2 && S <= 16;
  const bool site_fits = sweep_site_kernel(q, n_pad <= 8 * MK_SS_T ? 1 : 2) != nullptr && n_pad <= 16 * MK_SS_T &&
                         sweep_site_lds_bytes(nmax, q, q == 1) <= 156 * 1024;
  const bool site = mode == 0 && !small_multi && site_fits;
  const bool multi = (mode == 0 && !site && small_multi) || mode == 2 || mode == 3;
  s->sweep.coop = multi && mode != 3 && coop_fits;
  s->sweep.split = multi && !s->sweep.coop && nt <= 32;   // k_sweep_step sums <= 32 tile partials
  if (site) {
    s->sweep.site = n_pad <= 8 * MK_SS_T ? 1 : 2;
    bool all_even = true;
    for (int i = 0; i < S; ++i) all_even = all_even && (s->n_part[i] % 2 == 0);
    s->sweep.lean = q == 1 ? (all_even ? 2 : 1) : 0;
    s->sweep.site_lds = sweep_site_lds_bytes(nmax, q, s->sweep.lean);
    HIPCHK(hipFuncSetAttribute(sweep_site_kernel(q, s->sweep.site, s->sweep.lean),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)s->sweep.site_lds));
  }
  if (s->sweep.split) {
    HIPCHK(hipFuncSetAttribute(sweep_step_kernel(q), hipFuncAttributeMaxDynamicSharedMemorySize,
                               q * (64 * 64 + 2 * 64) * 8 + 4 * MK_NB * 8));
    if ((rc = s->alloc(&s->sweep.sp_part, (size_t)S * 2 * nt * q * 64))) return rc;
  }
  if (s->sweep.coop) {
    if ((rc = s->alloc(&s->sweep.sw_part, (size_t)S * 2 * nt * q * 64)) ||
        (rc = s->alloc(&s->sweep.sw_cnt, (size_t)S * (n_pad / 64 + 1))) || (rc = s->alloc(&s->sweep.sw_xcc, (size_t)S * nt)) ||
        (rc = s->alloc(&s->sweep.sw_err, 2)))
      return rc;
    s->sweep.sw_adm = s->sweep.sw_cnt + (size_t)S * (n_pad / 64);
    s->sweep.adm_spins = env_int("MK_ADM_SPINS", MK_ADM_SPINS);
    HIPCHK(hipMemsetAsync(s->sweep.sw_err, 0, 2 * sizeof(int), s->stream));
  }
  return 0;
}

// The factor slots, W and the inverse's tiles; for one stream group the lookahead schedule's buffers too.
static int alloc_factors(mk_session* s, const mk_config* c) {
  Model& md = s->md;
  MatSet& ms = s->ms;
  const int S = s->S, q = s->q, n_pad = s->n_pad, nt = s->nt;
  int rc;
  ms.ld = n_pad; ms.nt = nt; ms.q = q;
  if ((rc = s->alloc(&ms.L, (size_t)S * q * 2 * n_pad * n_pad)) ||
      (rc = s->alloc(&ms.Winv, (size_t)S * q * 2 * nt * MK_NB * MK_NB)) ||
      (rc = s->alloc(&ms.W, (size_t)S * q * n_pad * n_pad)) ||
      (!s->sweep.site && (rc = s->alloc(&ms.QB, (size_t)S * q * nt * MK_NB * MK_NB))) ||   // Q_BB: block sweeps only
      (rc = s->alloc(&ms.cur, (size_t)S * q)) ||
      (rc = s->alloc(&s->d_probs, MK_N_LEVELS)))
    return rc;
  // lookahead schedule buffers (run_iteration_la): one stream group (either covariance model)
  s->la.ok = group_count(c, S) == 1;
  if (s->la.ok) {
    if ((rc = s->alloc(&md.bacc, (size_t)S * q * n_pad)) || (rc = s->alloc(&md.zc, (size_t)S * q * n_pad)) ||
        (rc = s->alloc(&ms.Y, (size_t)S * q * n_pad * n_pad)) || (rc = s->alloc(&md.la_nu, (size_t)S * q)))
      return rc;
    HIPCHK(hipMemset(md.la_nu, 0, (size_t)S * q * sizeof(int)));
    s->la.ev.assign(nt + 5, nullptr);
    for (auto& e : s->la.ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return set_err(MK_E_HIP, "lookahead event");
  }
  return 0;
}

// The data from R's layout (per subset, unpadded) into the padded device layout.
static int stage_inputs(mk_session* s, const mk_problem* pr) {
  const Model& md = s->md;
  const int S = s->S, q = s->q, p = s->p, n_pad = s->n_pad, Np = md.Np;
  std::vector<double> hc((size_t)S * 2 * n_pad, 0.0), hy((size_t)S * Np, 0.0), hw((size_t)S * Np, 0.0),
      hX((size_t)S * p * Np, 0.0);
  {
    long off_site = 0;
    for (int i = 0; i < S; ++i) {
      const int ns = pr->n_part[i];
      const double* cs = pr->coords + 2 * off_site;
      for (int r = 0; r < ns; ++r) {
        hc[(size_t)i * 2 * n_pad + r] = cs[r];
        hc[(size_t)i * 2 * n_pad + n_pad + r] = cs[ns + r];
      }
      const double* ys = pr->y + off_site * q;
      const double* ws = pr->weights + off_site * q;
      for (int k = 0; k < ns * q; ++k) {
        hy[(size_t)i * Np + k] = ys[k];
        hw[(size_t)i * Np + k] = ws[k];
      }
      const double* xs = pr->x + off_site * q * p;
      for (int j = 0; j < p; ++j)
        for (int k = 0; k < ns * q; ++k) hX[((size_t)i * p + j) * Np + k] = xs[(size_t)j * ns * q + k];
      off_site += ns;
    }
  }
  HIPCHK(hipMemcpy((void*)md.n_s, pr->n_part, S * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy((void*)md.coords, hc.data(), hc.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy((void*)md.y, hy.data(), hy.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy((void*)md.wt, hw.data(), hw.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy((void*)md.X, hX.data(), hX.size() * 8, hipMemcpyHostToDevice));
  return 0;
}

// Starting values, identical for every subset (MK.R:54-62), and the state they start from.
static int starting_values(mk_session* s, const mk_config* c) {
  Model& md = s->md;
  const int S = s->S, q = s->q, p = s->p, n_pad = s->n_pad;
  const int Np = md.Np, ntri = md.ntri, n_theta = md.n_theta, n_mh_max = md.n_mh_max, o_w = md.o_w;
  std::vector<double> hb((size_t)S * p), hth((size_t)S * n_theta), hwv((size_t)S * Np, 0.0),
      htune((size_t)S * n_mh_max, 0.0), hA((size_t)S * q * q), hAi((size_t)S * q * q);
  std::vector<double> th0(n_theta), A0(q * q, 0.0), Ai0(q * q, 0.0), tune0(o_w);
  {
    int k = 0;
    for (int j = 0; j < q; ++j)
      for (int i = j; i < q; ++i, ++k) {
        const double a = c->A_starting[k];
        if (i == j && !(a > 0.0)) { return set_err(MK_E_ARG, "A starting diagonal must be > 0"); }
        th0[k] = (i == j) ? std::log(a) : a;
        A0[i + j * q] = a;
      }
    for (int h = 0; h < q; ++h) {
      const double ph = c->phi_starting[h];
      th0[ntri + h] = std::log((ph - md.phi_a[h]) / (md.phi_b[h] - ph));
      if (s->matern) {
        const double nv = c->nu_starting[h];
        if (!(md.nu_a[h] < nv && nv < md.nu_b[h])) { return set_err(MK_E_ARG, "nu starting value outside nu.Unif support"); }
        th0[ntri + q + h] = std::log((nv - md.nu_a[h]) / (md.nu_b[h] - nv));
      }
    }
    for (int cc = 0; cc < q; ++cc)
      for (int r = 0; r < q; ++r) {
        if (r < cc) continue;
        double sum = (r == cc) ? 1.0 : 0.0;
        for (int m = cc; m < r; ++m) sum -= A0[r + m * q] * Ai0[m + cc * q];
        Ai0[r + cc * q] = sum / A0[r + r * q];
      }
    for (int j = 0; j < p; ++j) {
      if (!(c->beta_tuning[j] > 0.0)) { return set_err(MK_E_ARG, "beta tuning must be > 0"); }
      tune0[j] = std::log(std::sqrt(c->beta_tuning[j]));
    }
    for (int k2 = 0; k2 < ntri; ++k2) tune0[p + k2] = std::log(std::sqrt(c->A_tuning[k2]));
    for (int h = 0; h < q; ++h) {
      tune0[p + ntri + h] = std::log(std::sqrt(c->phi_tuning[h]));
      if (s->matern) tune0[p + ntri + q + h] = std::log(std::sqrt(c->nu_tuning[h]));
    }
  }
  const double tw = std::log(std::sqrt(c->w_tuning));
  for (int i = 0; i < S; ++i) {
    for (int j = 0; j < p; ++j) hb[(size_t)i * p + j] = c->beta_starting[j];
    for (int k = 0; k < n_theta; ++k) hth[(size_t)i * n_theta + k] = th0[k];
    for (int k = 0; k < s->n_part[i] * q; ++k) {
      hwv[(size_t)i * Np + k] = c->w_starting;
      htune[(size_t)i * n_mh_max + o_w + k] = tw;
    }
    for (int k = 0; k < o_w; ++k) htune[(size_t)i * n_mh_max + k] = tune0[k];
    for (int k = 0; k < q * q; ++k) { hA[(size_t)i * q * q + k] = A0[k]; hAi[(size_t)i * q * q + k] = Ai0[k]; }
  }
  HIPCHK(hipMemcpy(md.beta, hb.data(), hb.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(md.theta, hth.data(), hth.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(md.w, hwv.data(), hwv.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(md.tune, htune.data(), htune.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(md.A_full, hA.data(), hA.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(md.Ainv, hAi.data(), hAi.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemsetAsync(md.acc, 0, (size_t)S * n_mh_max * 8, s->stream));
  HIPCHK(hipMemsetAsync(md.dirty, 0, (size_t)S * q * 4, s->stream));
  HIPCHK(hipMemsetAsync(md.notpd, 0, (size_t)S * q * sizeof(long long), s->stream));
  HIPCHK(hipMemsetAsync(md.u, 0, (size_t)S * q * n_pad * 8, s->stream));
  HIPCHK(hipMemsetAsync(md.z, 0, (size_t)S * q * n_pad * 8, s->stream));
  HIPCHK(hipMemsetAsync(md.Z, 0, (size_t)S * q * q * n_pad * 8, s->stream));
  {
    std::vector<double> probs(MK_N_LEVELS);
    // seq(0.005, 1, 0.005): from + (0:n)*by, pmin(x, to)  (MK.R:88)
    for (int i = 0; i < MK_N_LEVELS; ++i) probs[i] = std::fmin(0.005 + (double)i * 0.005, 1.0);
    HIPCHK(hipMemcpy(s->d_probs, probs.data(), MK_N_LEVELS * 8, hipMemcpyHostToDevice));
  }
  return 0;
}

// The factor slots, W and the diagonal inverses as the initial factorisation expects them.  Run before
// and after krig_tables, whose exact evaluations use these buffers as scratch.
static int reset_factor_state(mk_session* s) {
  const size_t SQ = (size_t)s->S * s->q;
  HIPCHK(hipMemsetAsync(s->ms.cur, 0, SQ * 4, s->stream));
  HIPCHK(hipMemsetAsync(s->md.info, 0, SQ * 4, s->stream));
  HIPCHK(hipMemsetAsync(s->ms.W, 0, SQ * s->n_pad * s->n_pad * 8, s->stream));
  // upper triangles of the Winv tiles stay zero (k_chol_diag writes the lower triangles only)
  HIPCHK(hipMemsetAsync(s->ms.Winv, 0, SQ * 2 * s->nt * MK_NB * MK_NB * 8, s->stream));
  return 0;
}

// Initial state: eta, u, every R_h factored at the starting values, W, z (whole shard); the statistics
// start from here.
static int initial_state(mk_session* s) {
  Model& md = s->md;
  MatSet& ms = s->ms;
  const int S = s->S, q = s->q;
  Group& a = s->all;
  MK_LAUNCH(k_init_state, dim3(S), dim3(256), 0, s->stream, md);
  launch_candidates(md, ms, s->stream, S * q, 0, q, 2, 0);
  launch_cholesky(s, a, 0, q);
  // a start that cannot be factored is an error, not a chain: every later candidate would be compared
  // with a NaN logdetR / quad.  info[] is zero past this point (k_theta_init leaves it alone).
  {
    std::vector<int> info((size_t)S * q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipMemcpy(info.data(), md.info, info.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int sh = 0; sh < S * q; ++sh)
      if (info[sh])
        return set_err(MK_E_ARG, "subset " + std::to_string(md.subset_base + sh / q) + ", outcome " + std::to_string(sh % q) +
                                     ": the correlation matrix at the starting values is not positive definite "
                                     "(coincident or non-finite sites?)");
  }
  MK_LAUNCH(k_theta_init, dim3((S * q + 63) / 64), dim3(64), 0, s->stream, md, ms, 0, q);
  MK_LAUNCH(k_dirty_list, dim3(1), dim3(256), 0, s->stream, md, 0, a.d_list, a.d_count, a.d_plist, a.d_pcount);
  launch_inverse(s, a);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s->stream));
  drain_timers(s);
  for (auto& st : s->prof.stats) st = Stat();
  if (s->kt.on) {   // the tables: exact evaluations and the largest set-up check difference
    s->prof.stats[KS_KRIG_CHEB].flops = s->kt.evals;
    s->prof.stats[KS_KRIG_CHEB].ms = s->kt.check;
  } else if (s->kt.fail) {
    s->prof.stats[KS_KRIG_FALLBACK].launches = s->kt.fail;
    s->prof.stats[KS_KRIG_FALLBACK].ms = s->kt.check;
  }
  return 0;
}

int mk::chain_reinit(mk_session* s) {
  int rc;
  if ((rc = reset_factor_state(s))) return rc;
  return initial_state(s);
}

extern "C" int mk_session_create(const mk_problem* pr, const mk_config* c, mk_session** out) {
  if (!out) return set_err(MK_E_ARG, "null out");
  *out = nullptr;
  int rc = check_cfg(pr, c);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return set_err(MK_E_NODEV, "no HIP device");
  if (c->device < 0 || c->device >= ndev) return set_err(MK_E_ARG, "bad device ordinal");
  MK_ENTRY_DEVICE(c->device);
  // the guard owns the session until it is handed out: every early return (allocation failure,
  // HIPCHK, argument error) frees the session and every device buffer allocated so far
  std::unique_ptr<mk_session> hold(new mk_session());
  mk_session* s = hold.get();
  s->device = c->device;
  if (pool_stream(s->owned, &s->stream, s->device, SK_PLAIN) != hipSuccess) return set_err(MK_E_HIP, "stream");
  derive_dims(s, pr, c);
  // the steps' order fixes the order of the device allocations, which kriging_buffers depends on
  if ((rc = alloc_chain_state(s, pr)) || (rc = plan_sweep(s, c)) || (rc = alloc_factors(s, c)) ||
      (rc = setup_groups(s, group_count(c, s->S))) || (rc = stage_inputs(s, pr)) || (rc = starting_values(s, c)) ||
      (rc = reset_factor_state(s)))
    return rc;
  if (!set_gemm_lds()) return set_err(MK_E_HIP, "lds attribute");
  // fused kriging tables before the initial factorisation: their evaluation uses the factor slots and
  // W as scratch
  if ((rc = krig_tables(s)) || (rc = reset_factor_state(s)) || (rc = initial_state(s))) return rc;
  // the test sites' covariates last: the kriging tile was sized from the HBM the allocations above left
  if (pr->x_test && (rc = set_test_covars(s, pr->x_test))) return rc;
  // default schedule: lookahead where eligible; MK_LOOKAHEAD=0 / 1 overrides (mk_session_set_lookahead too)
  static const int la_env = env_int("MK_LOOKAHEAD", -1);
  s->la.on = s->la.ok && (la_env == 1 || (la_env < 0 && la_auto(s)));
  *out = hold.release();
  return 0;
}

extern "C" int mk_session_run(mk_session* s, int32_t n_iter) {
  if (!s) return set_err(MK_E_ARG, "null session");
  if (s->poisoned) return poisoned_err(s);
  if (s->imp.done)
    return set_err(MK_E_ARG, "the session holds an imported chain, which is complete: mk_session_run cannot continue it");
  MK_ENTRY_DEVICE(s->device);
  if (n_iter < 0 || s->iter + n_iter > s->md.n_samples) return set_err(MK_E_ARG, "n_iter beyond n.samples");
  if (s->la.on && !s->la.c) {
    // the candidates' factorisation is the critical chain: its stream gets the device's highest
    // priority, so its small diagonal / trsm grids are dispatched ahead of the main stream's
    // inverse and sweep workgroups as CUs free up (a plain stream where the device reports no range)
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess) {
      if (pool_stream(s->owned, &s->la.c, s->device, SK_PRIO, hi) != hipSuccess)
        return set_err(MK_E_HIP, "lookahead stream");
    } else if (pool_stream(s->owned, &s->la.c, s->device, SK_PLAIN) != hipSuccess) {
      return set_err(MK_E_HIP, "lookahead stream");
    }
    // Two more streams when the process has the hardware queues for them (HIP maps streams onto
    // GPU_MAX_HW_QUEUES queues, default 4, shared round-robin beyond that -- a shared queue
    // serialises the split Cholesky's streams: measured 5,427 -> 4,087 subset-iters/s at 32
    // subsets; the package and bench.py set 8 before HIP starts):
    //  * la.k: the kept iterations' kriging refresh beside the sweep (sessions with fused test sites);
    //  * la.m: the iterations' main-stream work on a stream that leaves the first la_mask_cus() CUs
    //    (default 32: 4 per XCD, the split Cholesky's reserve) to the candidates' critical chain --
    //    its diagonal-tile workgroups take a whole CU's LDS and otherwise wait behind the inverse
    //    and kriging GEMMs (32 / 63 / 125 subsets: 6,669 -> 6,921, 7,550 -> 7,645, 8,062 -> 8,211).
    if (hw_queues() >= 8 && s->md.n_test > 0 && !s->tiled &&
        pool_stream(s->owned, &s->la.k, s->device, SK_PLAIN) != hipSuccess)
      return set_err(MK_E_HIP, "lookahead kriging stream");
    const int mask_cu = la_mask_cus();
    int n_cu = 0;
    if (mask_cu > 0 && hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, s->device) == hipSuccess) {
      std::vector<uint32_t> mask((n_cu + 31) / 32, 0xffffffffu);
      for (int b = 0; b < mask_cu && b < n_cu; ++b) mask[b / 32] &= ~(1u << (b % 32));
      if (pool_stream(s->owned, &s->la.m, s->device, SK_CUMASK, 0, mask) != hipSuccess)
        return set_err(MK_E_HIP, "lookahead main stream");
    }
  }
  static const int early_cov = env_int("MK_EARLY_COV", 1);
  // (the inverse must have its own scratch Y: without it, it works in the free factor slots)
  if (early_cov && !s->la.on && s->groups.size() == 1 && s->ms.Y && !s->cov.st) {
    if (pool_stream(s->owned, &s->cov.st, s->device, SK_PLAIN) != hipSuccess) return set_err(MK_E_HIP, "covariance stream");
    for (auto& e : s->cov.ev)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return set_err(MK_E_HIP, "covariance event");
  }
  const bool swap_m = s->la.on && s->la.m;
  if (swap_m) {   // the iterations' main-stream work on la.m, after everything queued on the session stream
    hipEventRecord(s->la.ev[s->nt + 1], s->stream);
    hipStreamWaitEvent(s->la.m, s->la.ev[s->nt + 1], 0);
    s->groups[0].stream = s->la.m;
  }
  const auto t0 = std::chrono::steady_clock::now();
  s->launch_err = hipSuccess;
  hipError_t le = hipSuccess;
  for (int i = 0; i < n_iter; ++i) {
    s->prof.iter = s->prof.every <= 1 || s->iter % s->prof.every == 0;
    run_iteration(s, s->iter);
    s->iter++;
    le = hipGetLastError();
    if (le == hipSuccess) le = s->launch_err;
    if (le != hipSuccess) break;
  }
  s->prof.iter = true;   // launches outside the iterations (the tiled replay) follow prof alone
  if (swap_m) s->groups[0].stream = s->stream;
  // every stream is drained before an error returns: nothing of this run is left queued
  if (le != hipSuccess) {
    for (hipStream_t st : {s->la.m, s->la.c, s->la.k, s->cov.st}) if (st) (void)hipStreamSynchronize(st);
    s->kt.pending = false;
    for (auto& g : s->groups) (void)hipStreamSynchronize(g.stream);
    crit_drain(s, false);
    return set_err(MK_E_HIP, std::string("kernel launch in iteration ") + std::to_string(s->iter - 1) + ": " +
                                 hipGetErrorString(le));
  }
  if (swap_m) HIPCHK(hipStreamSynchronize(s->la.m));
  for (auto& g : s->groups) HIPCHK(hipStreamSynchronize(g.stream));
  if (s->la.c) HIPCHK(hipStreamSynchronize(s->la.c));   // the next iteration's candidates
  if (s->la.k) HIPCHK(hipStreamSynchronize(s->la.k));
  if (s->kt.pending) {   // the last kept iteration's table draws (side stream)
    HIPCHK(hipEventSynchronize(s->kt.ev[1]));
    s->kt.pending = false;
  }
  crit_drain(s, true);
  if (s->sweep.coop) {
    // the multi-workgroup sweep's barrier time-out (after admission every wait completes: this is the
    // net under that argument): its chain state is then not the sampler's -- the session is
    // poisoned, every later call on it fails
    int e[2] = {0, 0};
    HIPCHK(hipMemcpy(e, s->sweep.sw_err, 2 * sizeof(int), hipMemcpyDeviceToHost));
    if (e[1]) {
      s->prof.stats[KS_SWEEP_FALLBACK].launches += e[1];
      HIPCHK(hipMemset(s->sweep.sw_err + 1, 0, sizeof(int)));
    }
    if (e[0]) {
      s->poisoned = "latent sweep: workgroup barrier timed out (MK_SWEEP=3 avoids the kernel)";
      return set_err(MK_E_HIP, s->poisoned);
    }
  }
  if (s->prof.on) {
    s->prof.stats[KS_ITER].launches += n_iter;
    s->prof.stats[KS_ITER].ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    drain_timers(s);
  }
  return 0;
}

extern "C" int32_t mk_session_iteration(const mk_session* s) { return s ? s->iter : -1; }

extern "C" int32_t mk_session_predict_tile(const mk_session* s) { return (s && s->tiled) ? s->pred_tile : 0; }

// The chain state of one subset after the iterations run so far, in spMvGLM's MH order: beta (p),
// theta (n_theta: A lower-tri col-major with log diagonal | logit phi | logit nu), w (n_s q,
// location-major), tune (p + n_theta + n_s q log proposal sds) and accept (the same, accept counts
// of the current amcmc batch).  Any pointer may be NULL.  A host can resume the chain elsewhere from
// it -- bench.py's CPU baseline times the oracle over the very window the device timed.
extern "C" int mk_session_chain_state(mk_session* s, int32_t subset, double* beta, double* theta, double* w,
                                      double* tune, double* accept) {
  if (!s) return set_err(MK_E_ARG, "null session");
  if (s->poisoned) return poisoned_err(s);
  if (s->imp.done)
    return set_err(MK_E_ARG, "the session holds an imported chain: it has the recorded states, not a sampler's state to resume");
  if (subset < 0 || subset >= s->S) return set_err(MK_E_ARG, "subset out of range");
  MK_ENTRY_DEVICE(s->device);
  const Model& md = s->md;
  const long i = subset, nq = (long)s->n_part[subset] * s->q, nmh = md.o_w + nq;
  HIPCHK(hipStreamSynchronize(s->stream));
  if (beta) HIPCHK(hipMemcpy(beta, md.beta + i * md.p, (size_t)md.p * 8, hipMemcpyDeviceToHost));
  if (theta) HIPCHK(hipMemcpy(theta, md.theta + i * md.n_theta, (size_t)md.n_theta * 8, hipMemcpyDeviceToHost));
  if (w) HIPCHK(hipMemcpy(w, md.w + i * md.Np, (size_t)nq * 8, hipMemcpyDeviceToHost));
  if (tune) HIPCHK(hipMemcpy(tune, md.tune + i * md.n_mh_max, (size_t)nmh * 8, hipMemcpyDeviceToHost));
  if (accept) HIPCHK(hipMemcpy(accept, md.acc + i * md.n_mh_max, (size_t)nmh * 8, hipMemcpyDeviceToHost));
  return 0;
}

// Per (subset, outcome): the phi / nu candidates rejected so far because their factorisation met a
// pivot that is not > 0 (k_theta_mh counts where it reads the flag).
extern "C" int mk_session_notpd_counts(mk_session* s, int64_t* out) {
  if (!s || !out) return set_err(MK_E_ARG, "null session/output");
  if (s->poisoned) return poisoned_err(s);
  MK_ENTRY_DEVICE(s->device);
  static_assert(sizeof(long long) == sizeof(int64_t), "notpd counts are 64-bit");
  HIPCHK(hipStreamSynchronize(s->stream));
  HIPCHK(hipMemcpy(out, s->md.notpd, (size_t)s->S * s->q * sizeof(int64_t), hipMemcpyDeviceToHost));
  return 0;
}


extern "C" int mk_session_set_lookahead(mk_session* s, int32_t mode) {
  if (!s) return set_err(MK_E_ARG, "null session");
  if (mode < -1 || mode > 1) return set_err(MK_E_ARG, "lookahead mode must be -1 (auto), 0 or 1");
  if (s->imp.done)
    return set_err(MK_E_ARG, "the session holds an imported chain: no iteration will run, so there is no schedule to set");
  if (s->iter > 0) return set_err(MK_E_ARG, "the schedule is fixed once the chain has started");
  if (mode == 1 && !s->la.ok)
    return set_err(MK_E_ARG, "lookahead needs the exponential model on one stream group");
  s->la.mode = mode;
  s->la.on = s->la.ok && (mode == 1 || (mode == -1 && la_auto(s)));
  return 0;
}

extern "C" int32_t mk_session_lookahead(const mk_session* s) { return (s && s->la.on) ? 1 : 0; }

extern "C" int mk_session_profile(mk_session* s, int32_t enable) {
  if (!s) return set_err(MK_E_ARG, "null session");
  s->prof.on = enable != 0;
  s->prof.kinds = (enable == 1) ? ~0u : ((uint32_t)enable >> 1);
  return 0;
}

extern "C" int mk_session_profile_every(mk_session* s, int32_t every) {
  if (!s) return set_err(MK_E_ARG, "null session");
  if (every < 1) return set_err(MK_E_ARG, "every must be >= 1");
  s->prof.every = every;
  return 0;
}

extern "C" int mk_session_kernel_stats(const mk_session* s, int32_t which, int64_t* launches, double* total_ms,
                                       double* flops) {
  if (!s || which < 0 || which >= NKSTAT) return set_err(MK_E_ARG, "bad stats query");
  if (launches) *launches = s->prof.stats[which].launches;
  if (total_ms) *total_ms = s->prof.stats[which].ms;
  if (flops) *flops = s->prof.stats[which].flops;
  return 0;
}

// ------------------------------------------------------------------ shard interface (mk_multi.hip)
namespace mk {
int session_info(const mk_session* s, ShardInfo* in) {
  in->device = s->device;
  in->S = s->S;
  in->P = s->P;
  in->q = s->q;
  in->n_test = s->n_test_all;
  in->tiled = s->tiled ? 1 : 0;
  in->pred_tile = s->tiled ? s->pred_tile : s->n_test_all;
  in->n_kept = s->md.n_kept;
  in->stream = s->stream;
  return 0;
}
// The 200-level grids of one kind from the recorded draws into d_out (HBM), on the session stream,
// not waited for: [S][P][200] of the parameters (obj[[i]]$parameters, MK.R:89), or of a fused
// session's kriging draws [S][q n_test][200] -- w.predict, or p = pred_prob(draw), transformed as the
// sort's LDS is filled (no buffer of p draws).
static int launch_grids(mk_session* s, GridKind kind, double* d_out) {
  const Model& md = s->md;
  if (kind == GRID_PARAMETERS)
    return launch_quantiles(s->S * s->P, s->stream, md.samples + (long)md.kept0 * s->P, (long)md.n_samples * s->P,
                            (long)s->P, md.n_kept, s->P, s->d_probs, MK_N_LEVELS, d_out);
  const int C = s->q * md.n_test;
  if (kind == GRID_P)
    return launch_quantiles_prob(s->S * C, s->stream, md.w_pred, (long)md.n_kept * C, (long)C, md.n_kept, C, s->d_probs,
                                 MK_N_LEVELS, d_out, prob_src(s, 0));
  return launch_quantiles(s->S * C, s->stream, md.w_pred, (long)md.n_kept * C, (long)C, md.n_kept, C, s->d_probs,
                          MK_N_LEVELS, d_out);
}
int session_grids(mk_session* s, GridKind kind, double* d_out) {
  MK_ENTRY_DEVICE(s->device);
  if (kind != GRID_PARAMETERS && s->tiled) return set_err(MK_E_ARG, "tiled sessions produce their grids per tile");
  if (kind == GRID_P && !s->d_xt) return set_err(MK_E_ARG, "predictive probabilities need x_test");
  if (s->iter < s->md.n_samples) return set_err(MK_E_ARG, "quantile outputs need all n.samples iterations");
  const int rq = launch_grids(s, kind, d_out);
  if (rq) return rq;
  HIPCHK(hipStreamSynchronize(s->stream));
  return 0;
}
int grids_to_host(mk_session* s, const double* d_grids, long Ct, long col0, long C, double* h_each, double* h_sum,
                  double* dsum) {
  const size_t row = (size_t)Ct * MK_N_LEVELS * 8;   // one subset's block
  hipStream_t st = s->stream;
  if (h_each && Ct == C)   // whole arrays: one flat copy
    HIPCHK(hipMemcpyAsync(h_each, d_grids, (size_t)s->S * row, hipMemcpyDeviceToHost, st));
  else if (h_each)
    HIPCHK(hipMemcpy2DAsync(h_each + (size_t)col0 * MK_N_LEVELS, (size_t)C * MK_N_LEVELS * 8, d_grids, row, row, s->S,
                            hipMemcpyDeviceToHost, st));
  if (h_sum) {   // this shard's term of the combine: sequential sum over its subsets
    MK_LAUNCH(k_combine, dim3((unsigned)((Ct * MK_N_LEVELS + 255) / 256)), dim3(256), 0, st, d_grids, s->S,
              Ct * MK_N_LEVELS, dsum, 0);
    HIPCHK(hipMemcpyAsync(h_sum + (size_t)col0 * MK_N_LEVELS, dsum, row, hipMemcpyDeviceToHost, st));
  }
  return 0;
}
// Tiled session: the grids [S][q Tc][200] of test-site tile [t0, t0 + Tc) into d_out, those of the
// predictive probabilities into d_out_p (either may be NULL; one replay), and the tile's draws
// into o->w_pred_samples / o->p_pred_samples when set.
int session_tile_grids(mk_session* s, int t0, double* d_out, mk_outputs* o, double* d_out_p) {
  MK_ENTRY_DEVICE(s->device);
  if (!s->tiled) return set_err(MK_E_ARG, "not a tiled session");
  if (s->iter < s->md.n_samples) return set_err(MK_E_ARG, "quantile outputs need all n.samples iterations");
  if (t0 < 0 || t0 >= s->n_test_all || t0 % s->pred_tile) return set_err(MK_E_ARG, "bad tile offset");
  return predict_tile(s, t0, d_out, o, d_out_p);
}
}  // namespace mk

extern "C" int mk_session_grids(mk_session* s, int32_t which, double* out, int32_t device_out) {
  if (!s || !out) return set_err(MK_E_ARG, "null session/output");
  if (s->poisoned) return poisoned_err(s);
  if (which < 0 || which > 2) return set_err(MK_E_ARG, "which must be 0 (parameters), 1 (w.predict) or 2 (p.predict)");
  if (which >= 1 && s->tiled) return set_err(MK_E_ARG, "tiled sessions give their kriging grids per tile (mk_session_tile_grids)");
  if (which >= 1 && s->md.n_test < 1) return set_err(MK_E_ARG, "the session has no test sites");
  if (which == 2 && !s->d_xt) return set_err(MK_E_ARG, "p.predict grids need x_test");
  const long C = which == 0 ? (long)s->P : (long)s->q * s->md.n_test;
  MK_ENTRY_DEVICE(s->device);
  DevBufs scratch;
  double* d = out;
  if (!device_out && !(d = scratch.get<double>((size_t)s->S * C * MK_N_LEVELS))) return set_err(MK_E_NOMEM, "grid scratch");
  const int rc = session_grids(s, (GridKind)which, d);
  if (rc) return rc;
  if (!device_out) HIPCHK(hipMemcpy(out, d, (size_t)s->S * C * MK_N_LEVELS * 8, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int mk_session_tile_grids_wp(mk_session* s, int32_t t0, double* out_w, double* out_p, int32_t device_out) {
  if (!s || (!out_w && !out_p)) return set_err(MK_E_ARG, "null session/output");
  if (s->poisoned) return poisoned_err(s);
  if (!s->tiled) return set_err(MK_E_ARG, "tile grids need a session created with predict_tile > 0");
  if (out_p && !s->d_xt) return set_err(MK_E_ARG, "p.predict grids need x_test");
  if (device_out) return session_tile_grids(s, t0, out_w, nullptr, out_p);
  const long Tc = std::min(s->pred_tile, s->n_test_all - t0);
  const size_t n = (size_t)s->S * s->q * std::max(Tc, 1L) * MK_N_LEVELS;
  MK_ENTRY_DEVICE(s->device);
  DevBufs scratch;
  double* dq = out_w ? scratch.get<double>(n) : nullptr;
  double* dqp = out_p ? scratch.get<double>(n) : nullptr;
  if ((out_w && !dq) || (out_p && !dqp)) return set_err(MK_E_NOMEM, "tile grid scratch");
  const int rc = session_tile_grids(s, t0, dq, nullptr, dqp);
  if (rc) return rc;
  const size_t bytes = (size_t)s->S * s->q * Tc * MK_N_LEVELS * 8;
  if (out_w) HIPCHK(hipMemcpy(out_w, dq, bytes, hipMemcpyDeviceToHost));
  if (out_p) HIPCHK(hipMemcpy(out_p, dqp, bytes, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int mk_session_tile_grids(mk_session* s, int32_t t0, double* out, int32_t device_out) {
  if (!s || !out) return set_err(MK_E_ARG, "null session/output");
  return mk_session_tile_grids_wp(s, t0, out, nullptr, device_out);
}

// A downloaded device array, row-major [rows][ld], into the caller's layout: element (r, c), c < cols,
// goes to dst[r * dr + c * dc], and rows >= valid are written as zero (iterations not run yet).  A
// column-major rows x cols destination is dr = 1, dc = rows.
static void host_layout(double* dst, size_t dr, size_t dc, const double* src, int rows, int cols, size_t ld, int valid) {
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) dst[r * dr + c * dc] = r < valid ? src[r * ld + c] : 0.0;
}

extern "C" int mk_session_outputs(mk_session* s, mk_outputs* o) {
  if (!s || !o) return set_err(MK_E_ARG, "null session/outputs");
  if (s->poisoned) return poisoned_err(s);
  MK_ENTRY_DEVICE(s->device);
  Model& md = s->md;
  const int S = s->S, P = s->P, q = s->q;
  const int n_test = md.n_test;
  const bool done = s->iter >= md.n_samples;
  const bool want_p = o->p_predict || o->p_pred_samples || o->p_predict_sum;
  if ((o->parameters || o->w_predict || o->w_pred_samples || want_p) && !done)
    return set_err(MK_E_ARG, "quantile/predictive outputs need all n.samples iterations");
  if (o->acceptance && s->imp.done && !s->imp.acc)
    return set_err(MK_E_ARG, "acceptance: the imported chain came without acceptance rates (mk_chain.acceptance was NULL)");
  if (want_p && !s->d_xt)
    return set_err(MK_E_ARG, "p_predict / p_pred_samples / p_predict_sum need x_test (mk_problem.x_test or "
                             "mk_session_set_test_covars)");
  DevBufs scratch;
  // One kind's grids (parameters, or a fused session's w / p) through scratch of their own to the
  // host; the device layout [S][C][200] == R's 200 x C column-major per subset.
  auto grids = [&](GridKind kind, double* h_each, double* h_sum) -> int {
    const long C = kind == GRID_PARAMETERS ? P : (long)q * n_test;
    double* dq = scratch.get<double>((size_t)S * C * MK_N_LEVELS);
    if (!dq) return set_err(MK_E_NOMEM, "quantile scratch");
    double* dsum = h_sum ? scratch.get<double>((size_t)C * MK_N_LEVELS) : nullptr;
    if (h_sum && !dsum) return set_err(MK_E_NOMEM, "combine scratch");
    const int rq = launch_grids(s, kind, dq);
    return rq ? rq : grids_to_host(s, dq, C, 0, C, h_each, h_sum, dsum);
  };
  int rg;
  if (o->parameters && (rg = grids(GRID_PARAMETERS, o->parameters, nullptr))) return rg;
  // fused: p before w (the same draws, transformed on load)
  if (!s->tiled && (o->p_predict || o->p_predict_sum) && (rg = grids(GRID_P, o->p_predict, o->p_predict_sum))) return rg;
  if (!s->tiled && o->p_pred_samples) {   // per subset C x kept column-major == the device's [kept][C]
    const int C = q * n_test;
    double* dp = scratch.get<double>((size_t)md.n_kept * C);
    if (!dp) return set_err(MK_E_NOMEM, "p draw scratch");
    for (int i = 0; i < S; ++i) {
      const int rc = pred_prob_to_host(s, i, 0, md.n_kept, C, dp, o->p_pred_samples + (size_t)i * md.n_kept * C, (size_t)C);
      if (rc) return rc;
    }
  }
  if (s->tiled && (o->w_predict || o->w_pred_samples || o->w_predict_sum || want_p)) {
    HIPCHK(hipStreamSynchronize(s->stream));
    int rc = predict_tiled(s, o);
    if (rc) return rc;
    if (s->prof.on) drain_timers(s);
  } else if ((o->w_predict || o->w_predict_sum) && n_test > 0) {
    if ((rg = grids(GRID_W, o->w_predict, o->w_predict_sum))) return rg;
  }
  HIPCHK(hipStreamSynchronize(s->stream));
  const int it = s->iter, n = md.n_samples;
  std::vector<double> h;
  if (o->samples) {   // [S][iter][P] -> per subset n_samples x P column-major
    h.resize((size_t)S * n * P);
    HIPCHK(hipMemcpy(h.data(), md.samples, h.size() * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < (size_t)S; ++i) host_layout(o->samples + i * n * P, 1, n, h.data() + i * n * P, n, P, P, it);
  }
  if (o->w_samples) {   // [S][iter][Np] -> per subset N x n_samples column-major: a state's N valid entries are a column
    if (!md.w_samples) return set_err(MK_E_ARG, "w samples were not recorded (record_w = 0)");
    h.resize((size_t)S * n * md.Np);
    HIPCHK(hipMemcpy(h.data(), md.w_samples, h.size() * 8, hipMemcpyDeviceToHost));
    size_t off = 0;
    for (int i = 0; i < S; ++i) {
      const int N = s->n_part[i] * q;
      host_layout(o->w_samples + off, N, 1, h.data() + (size_t)i * n * md.Np, n, N, md.Np, it);
      off += (size_t)N * n;
    }
  }
  // [S][kept][C] == per subset C x kept column-major (p.w.predictive.samples)
  if (o->w_pred_samples && n_test > 0 && !s->tiled)
    HIPCHK(hipMemcpy(o->w_pred_samples, md.w_pred, (size_t)S * md.n_kept * q * n_test * 8, hipMemcpyDeviceToHost));
  if (o->acceptance) {   // [S][batch][nrep] -> per subset n_batch x nrep column-major
    const size_t nb = md.n_batch, nrep = md.o_w + 1;
    h.resize((size_t)S * nb * nrep);
    HIPCHK(hipMemcpy(h.data(), md.acc_hist, h.size() * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < (size_t)S; ++i)
      host_layout(o->acceptance + i * nb * nrep, 1, nb, h.data() + i * nb * nrep, (int)nb, (int)nrep, nrep, (int)nb);
  }
  return 0;
}

extern "C" void mk_session_destroy(mk_session* s) {
  ApiCall call(__func__);
  DeviceGuard dg;
  delete s;
}

extern "C" int32_t mk_session_count(void) { return g_live_sessions.load(); }

extern "C" int mk_fit_predict_batched(const mk_problem* pr, const mk_config* c, mk_outputs* o) {
  mk_session* s = nullptr;
  int rc = mk_session_create(pr, c, &s);
  if (rc) return rc;
  rc = mk_session_run(s, c->n_batch * c->batch_length);
  if (!rc) rc = mk_session_outputs(s, o);
  mk_session_destroy(s);
  return rc;
}

