// What libmk's host sources share: struct mk_session and the functions that cross files.
//
//   mk_api.hip       the C ABI of a session: create / run / destroy, getters, outputs, the shard interface
//   mk_pool.hip      the process-wide stream pool
//   mk_schedule.hip  the per-iteration launch schedule (Cholesky forms, inverse, sweep, lookahead)
//   mk_krig.hip      the kriging buffers, the phi tables and the tiled replay
//   mk_summary.hip   stateless entry points (combine, Weiszfeld, posterior summary, glm): no session
//   mk_parity.hip    parity-test entry points
//   mk_diag.hip      chain diagnostics: the launcher, the session entry points, the tile sink
//   mk_criteria.hip  model assessment (DIC, WAIC): the kernels, the scratch, the session entry points
//   mk_loo.hip       leave-one-out (PSIS-LOO elpd and k-hat per observation): the kernels, the entry points
//   mk_scores.hip    held-out validation (log score, Brier, error rate): the kernels, the entry points
//   mk_maps.hip      posterior maps (mean, sd, exceedance of p(y = 1)): the kernel, the entry points
//   mk_pairs.hip     cross-outcome prediction (co-occurrence and contrast of two outcomes): the kernels, the entry points
//   mk_regions.hip   areal prediction (regional prevalence from joint kriging draws): the kernels, the entry points
//   mk_import.hip    sessions from a recorded chain: the kernels, the upload, the entry points
//   mk_checkpoint.hip  checkpoints: the state out and in, the digest kernel, the entry points
//
// What the six result sinks above share is here and in mk_tilefill.hpp: EventTimer (their launches' price),
// TileFill (which tiles a tiled session's buffer holds, over which kept window), results_entry (the checks a
// results call starts with), upload_col_chunks (the stand-alone grid entries) and sink_nomem.  The list of
// sinks a tile replay fills and mk_session_set_test_sites detaches is in mk_krig.hip (tile_sinks, detach_sinks).
//
// mk_internal.hpp stays the interface towards mk_multi.hip and mk_watch.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>
#include "../../include/mk.h"
#include "mk_kernels.hpp"
#include "mk_internal.hpp"
#include "mk_tilefill.hpp"
#include "mk_regionspec.hpp"
#include "mk_regionchunk.hpp"

namespace mk {
int set_err(int code, const std::string& msg);   // mk_api.hip: sets mk_last_error(), returns code
}

#define HIPCHK(x)                                                                                         \
  do {                                                                                                    \
    hipError_t e_ = (x);                                                                                  \
    if (e_ != hipSuccess) return ::mk::set_err(MK_E_HIP, std::string(#x " -> ") + hipGetErrorString(e_)); \
  } while (0)

// Entry of a C-ABI call that works on `dev`: registered with the stall watchdog, the caller's
// current device restored on every return path (an R or torch host keeps its own device).
#define MK_ENTRY_DEVICE(dev)        \
  ::mk::ApiCall mk_call_(__func__); \
  ::mk::DeviceGuard mk_dg_;         \
  HIPCHK(hipSetDevice(dev))

namespace mk {

static inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// An integer environment switch (dflt when unset or empty).
static inline int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return (v && *v) ? std::atoi(v) : dflt;
}

// Ranges of the Matern Chebyshev tables (Model::span, Model::span_pt), shared by the sessions and the
// parity entry mk_correlation_cross_batched: b = xmin xmax ymin ymax of n sites (zeros when n = 0),
// the bounding-box diagonal of a subset's sites, and the bound on every distance from a subset's
// sites (box b) to the test sites (box t).
static inline void site_bbox(const double* x, const double* y, int n, double* b) {
  b[0] = b[1] = b[2] = b[3] = 0.0;
  for (int r = 0; r < n; ++r) {
    if (r == 0 || x[r] < b[0]) b[0] = x[r];
    if (r == 0 || x[r] > b[1]) b[1] = x[r];
    if (r == 0 || y[r] < b[2]) b[2] = y[r];
    if (r == 0 || y[r] > b[3]) b[3] = y[r];
  }
}
static inline double matern_span(const double* b) { return std::hypot(b[1] - b[0], b[3] - b[2]); }
static inline double matern_span_pt(const double* b, const double* t) {
  return std::hypot(std::fmax(std::fabs(b[1] - t[0]), std::fabs(t[1] - b[0])),
                    std::fmax(std::fabs(b[3] - t[2]), std::fabs(t[3] - b[2])));
}

constexpr int NKSTAT = 22;
// KS_CHOL_UPDATE: the 128-tile panel-update launches (k_chol_update<128>); KS_CHOL_UPDATE_SUB:
// the 64- / 32-sub-tile ones (small grids).  Together: the roofline kernel k_chol_update.
// KS_UPDATE_BUSY: both, with the time of launches that overlap (the split schedule's bulk and
// critical streams) counted once -- the union of their event intervals.
// KS_PRED_VAR: the kriging GEMM k_pred_var; its flops assume every pair is refreshed (an upper
// bound: only the pairs whose factor changed are in the list -- bench_kriging counts exactly).
// KS_COV: the candidates' covariance assembly (k_cov_candidate, with k_matern_table for Matern).
enum { KS_CHOL_UPDATE = 0, KS_CHOL_DIAG, KS_CHOL_TRSM, KS_SWEEP, KS_LAUUM, KS_ITER, KS_INV, KS_CHOL_UPDATE_SUB,
       KS_UPDATE_BUSY, KS_PRED_VAR, KS_COV, KS_SWEEP_FALLBACK, KS_KRIG_CHEB, KS_KRIG_FALLBACK, KS_DIAG, KS_CRIT,
       KS_SCORE, KS_MAPS, KS_PAIRS, KS_REGIONS, KS_LOO, KS_CKPT };
// KS_KRIG_CHEB: tiles kriged by phi interpolation (predict_tile_cheb): launches = tiles, flops = exact
// s evaluations (one per (subset, outcome) pair and node or check point), total_ms = the largest check
// difference seen over all pairs and sites (not a time).  KS_KRIG_FALLBACK: tiles whose check failed
// and were replayed exactly (launches), and total_ms the largest failing difference.
// KS_DIAG: the chain-diagnostic launches (k_chain_diag, k_chain_diag_prob), bracketed by events whether
// or not the profiler is on (a handful per call, each followed by a wait anyway).
// KS_CRIT: the model-assessment launches (k_crit_accum per kept iteration and stream group, k_crit_replay,
// k_crit_finish and k_crit_total per mk_session_criteria), bracketed by events whether or not the profiler
// is on; none are made unless criteria were asked for.
// KS_SCORE: the held-out scoring launches (k_score_cols per tile replay or mk_session_scores, k_score_finish
// per mk_session_scores), bracketed by events whether or not the profiler is on; none are made unless
// validation data were attached.
// KS_MAPS: the posterior-map launches (k_map_cols per tile replay of a tiled session, per mk_session_maps of
// a fused one), bracketed by events whether or not the profiler is on; none are made unless maps were asked
// for.
// KS_PAIRS: the cross-outcome launches (k_quantiles_pair and k_pair_cols per tile replay of a tiled session,
// what mk_session_pairs is asked for of a fused one; launches counts kernels), bracketed by events whether or
// not the profiler is on; none are made unless pairs were asked for.
// KS_REGIONS: the areal-prediction launches (k_region_cov per kept state whose dirty list may hold a pair,
// k_region_draw per kept state, then k_quantiles and k_map_cols per tile replay; on the interpolated route
// k_region_cov_node per node and check slot, k_region_check, and k_region_interp_factor and k_region_draw per
// chunk of kept states in their place; launches counts kernels), bracketed by events whether or not the
// profiler is on; none are made unless regions were attached.
// KS_LOO: the PSIS-LOO launches (k_loo_terms and k_loo_psis per chunk of subsets, k_loo_finish and k_loo_total
// per mk_session_loo), bracketed by events whether or not the profiler is on; none are made unless
// mk_session_loo is called.
// KS_CKPT: the state-digest launches (k_state_digest and k_digest_reduce per factor buffer of a checkpoint, a
// restore or mk_session_digest), bracketed by events whether or not the profiler is on; none are made unless one
// of those calls is.
// KS_SWEEP_FALLBACK: launches = (subset, iteration) sweeps k_sweep_mg refused admission and its
// k_sweep fallback ran (counted on the device, read at the end of every mk_session_run; no timing).

// What a phi-interpolated path returns when the exact path must run instead (not applicable, scratch memory
// short, a check failed); 0 when done, an MK_E_* code (< 0) on an error.
constexpr int MK_CHEB_EXACT = 1;

struct Stat {
  long launches = 0;
  double ms = 0.0, flops = 0.0;
};

struct Timed {
  int which;
  hipEvent_t a, b;
  double flops;
  int cnt = -1;   // >= 0: flops are per listed factor, times the device-side count copied to inv_cnt[cnt]
};

// One stream's share of the shard: views of the shard arrays starting at subset s0.
struct Group {
  Model md{};
  MatSet ms{};
  hipStream_t stream = nullptr;
  int S = 0, s0 = 0;
  int* d_list = nullptr;   // pairs whose factor changed (inverse work list)
  int* d_count = nullptr;
  int* d_plist = nullptr;  // pairs needing a kriging refresh
  int* d_pcount = nullptr;
  hipEvent_t done = nullptr;         // fork-join sweep: this group's pre-sweep work is queued
  hipStream_t bulk = nullptr;        // split Cholesky (launch_cholesky): CU-masked bulk-update stream
  std::vector<hipEvent_t> ev;        // 2 nt + 1 events reused every factorisation
};

// Scoped device scratch (freed on every return path).
struct DevBufs {
  std::vector<void*> p;
  ~DevBufs() {
    for (void* x : p) hipFree(x);
  }
  template <typename T>
  T* get(size_t n) {
    void* x = nullptr;
    if (hipMalloc(&x, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();   // not sticky for the caller's later launch checks
      return nullptr;
    }
    p.push_back(x);
    return (T*)x;
  }
};

// ---- mk_pool.hip: streams by device and kind (plain, high priority, CU-masked with a given mask)
enum { SK_PLAIN = 0, SK_PRIO = 1, SK_CUMASK = 2 };
struct PoolKey {
  int device = -1, kind = SK_PLAIN, prio = 0;
  std::vector<uint32_t> mask;
  bool operator==(const PoolKey& o) const {
    return device == o.device && kind == o.kind && prio == o.prio && mask == o.mask;
  }
};
typedef std::vector<std::pair<PoolKey, hipStream_t>> StreamList;

// ---- the sub-systems of a session, each with the file that owns it

// mk_schedule.hip (run_iteration_la).  Lookahead schedule (one group): iteration t+1's phi
// candidates are factored on c while iteration t's inverse and sweep run on the main stream,
// and their z' = L'^-1 u is solved on the main stream trailing the factorisation panel by panel.
struct Lookahead {
  int mode = -1;               // mk_session_set_lookahead: -1 auto, 0 off, 1 on
  bool ok = false;             // eligible (buffers allocated)
  bool on = false;             // in use
  int next = -1;               // iteration whose candidates are queued on c (-1: none)
  int enq = 0;                 // panels of those candidates enqueued so far
  hipStream_t m = nullptr;     // MK_LA_MASK: CU-masked main stream of the lookahead iterations
  hipStream_t c = nullptr;     // created at the first lookahead run (an unused stream still takes a
                               // hardware queue, GPU_MAX_HW_QUEUES = 4, and slows the split Cholesky)
  hipStream_t k = nullptr;     // kept iterations' kriging refresh beside the sweep
  std::vector<hipEvent_t> ev;  // [nt] panel k final | decided (or adapted) | join | W ready | kriged
};

// mk_schedule.hip (iteration_pre_sweep).  Sequential schedule, one group (MK_EARLY_COV, default on):
// iteration t+1's phi candidates are assembled (without the bordered row) on st beside iteration t's
// sweep; iteration t+1 writes the row once its A step has produced u (k_cand_border) and factors as
// usual -- the same matrices.
struct EarlyCov {
  int pre = -1;                // iteration whose candidates st has assembled (-1: none)
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};   // [0] main stream ready for it, [1] assembled
};

// mk_krig.hip (krig_tables).  Fused kriging from phi tables (exponential, q = 1, one group):
// s(t; phi) at Chebyshev nodes of the prior's phi range, made at session creation; kept iterations
// interpolate them.
struct KrigTables {
  bool on = false;
  int fail = 0;                // set-up checks that failed (the session then refreshes X exactly)
  double check = 0.0, evals = 0.0;
  ChebK tab{};
  double* g = nullptr;         // [S][n_pad] g = W' z of the current kept iteration
  double* z = nullptr;         // [S][n_pad + 2]: its z, then phi and A per subset (k_kt_snap)
  hipEvent_t ev[2] = {nullptr, nullptr};   // [0] snapshot taken, [1] draws done (side stream)
  bool pending = false;        // draws queued on the side stream, not yet waited for
};

// mk_krig.hip (predict_tile_cheb).  Phi-interpolated tiled kriging: the window's g_k = W_k' z_k and
// phi_k per (subset, outcome) pair, kept across tiles (made at the first tile after a run or a window
// change).
struct ChebWindow {
  double* G = nullptr;         // [S q][n_pad][nkp]: g of the window's states (nkp = window rounded up to 8)
  double* phi = nullptr;       // [win][S q]
  double* phit = nullptr;      // [S q][nkp]: phi per state, padded with the last
  std::vector<double> phi_h;
  int iter = -1, lo = -1, n = -1;
};

// mk_api.hip (plan_sweep) chooses, mk_schedule.hip (launch_sweep) launches.  site: the one-pass site
// sweep (default; row pairs per thread, 0: off) with its LDS and lean form; else, for multi-outcome
// small shards, the split-launch multi-workgroup kernel behind its admission consensus, k_sweep
// sweeping the subsets it did not admit (coop), or the split-launch sweep (split: no inter-workgroup
// waits); else the 64-site-block kernel (k_sweep, one workgroup per subset).
struct SweepPlan {
  int site = 0;
  size_t site_lds = 0;
  int lean = 0;                // q = 1: 1 border row by factor, 2 every n_s even (sweep_site_kernel)
  bool split = false;          // k_sweep_step, one launch per 64-site block
  bool coop = false;           // k_sweep_mg (admission consensus) + k_sweep for the subsets not admitted
  size_t mg_lds = 0;
  double* sp_part = nullptr;
  double* sw_part = nullptr;
  int* sw_cnt = nullptr;       // [S][n_pad / 64] block counters, then [S] admission words (sw_adm)
  int* sw_adm = nullptr;
  int adm_spins = MK_ADM_SPINS;
  int* sw_xcc = nullptr;
  int* sw_err = nullptr;
};

// mk_schedule.hip (timed, drain_timers).
struct Profiler {
  bool on = false;
  uint32_t kinds = ~0u;   // kernel kinds bracketed by events while on (bit per KS_ kind)
  int every = 1;          // bracket the launches of every every-th iteration only
  bool iter = true;       // this iteration's launches are bracketed (mk_session_run)
  std::vector<Timed> pending;
  // KS_INV timing: the inverse's work list length lives on the device, so each timed inverse copies
  // its count into a pinned slot in stream order; drain_timers prices the launches with it
  static constexpr int INV_CNT_CAP = 65536;
  int* inv_cnt = nullptr;
  int inv_cnt_used = 0;
  Stat stats[NKSTAT];
};

// mk_criteria.hip.  In-chain model assessment (mk_session_set_criteria): the scratch the kept
// iterations accumulate into (allocated when switched on, never otherwise), the events around their
// launches (priced at the end of every mk_session_run), and the kept window of a session that is not
// tiled (mk_session_set_kept_window; a tiled session's is win_lo / win_n).
struct Criteria {
  bool on = false;
  Crit buf{};
  std::vector<Timed> pending;
  int win_lo = 0, win_n = -1;
};

// mk_scores.hip.  Held-out validation (mk_session_set_validation): the data in HBM and, for a tiled
// session, the pointwise pairs its tile replays fill (allocated when data are attached, never otherwise).
struct Validation {
  bool on = false;
  double* y = nullptr;        // [q n_test_all]
  double* wt = nullptr;       // [q n_test_all]
  double* pw = nullptr;       // tiled: [S][2][q n_test_all], plane 0 pmean_c, plane 1 lpd_c
  TileFill fill;              // tiled: the tiles scored since the data were attached
};

// mk_maps.hip.  Posterior maps (mk_session_set_maps): the thresholds and, for a tiled session, the
// planes its tile replays fill (allocated when maps are asked for, never otherwise).
struct Maps {
  bool on = false;
  MapThr th{};
  double* planes = nullptr;   // tiled: [S][MK_N_MAP_BASE + J][q n_test_all]
  TileFill fill;              // tiled: the tiles filled since the maps were attached
};

// mk_pairs.hip.  Cross-outcome prediction (mk_session_set_pairs): the thresholds and, for a tiled session,
// the grids and planes its tile replays fill (allocated when pairs are asked for, never otherwise).
struct Pairs {
  bool on = false;
  MapThr th{};
  double* grids = nullptr;    // tiled: [S][2][C2][200], both then diff; C2 = n_pairs n_test_all
  double* planes = nullptr;   // tiled: [S][MK_N_PAIR_BASE + J][C2]
  TileFill fill;              // tiled: the tiles filled since the pairs were attached
};

// mk_regions.hip.  Areal prediction (mk_session_set_regions): the plan in HBM, the packed factors of every
// (pair, region) as the replay last refreshed them, and the buffers the replay and tile_regions fill
// (allocated when regions are attached, never otherwise).
struct Regions {
  bool on = false;
  MapThr th{};
  RegionPlan plan;            // host copy (offsets, omega, factor offsets)
  int C3 = 0;                 // region columns G q
  int* offsets = nullptr;     // [G + 1]
  long* foff = nullptr;       // [G + 1]
  double* omega = nullptr;    // [n_test_all]
  double* L = nullptr;        // [S q][foff[G]]: region g's factor m_g x m_g column-major at foff[g]
  int* flag = nullptr;        // [S q][G]: 1 where that factor met a pivot that is not > MK_REGION_PIVOT_TOL
  double* draws = nullptr;    // [S][n][C3], n the replayed window (room for every kept state)
  int* singular = nullptr;    // [S][C3]
  double* grids = nullptr;    // [S][C3][200]
  double* planes = nullptr;   // [S][2 + J][C3]
  TileFill fill;
  struct Ev { int part; hipEvent_t a, b; long launches; };
  std::vector<Ev> pending;    // events of the launches inside the replay loop, priced by tile_regions
  double ms[3] = {0.0, 0.0, 0.0};   // since the attach: covariance and factor | draws | grids and planes
  int route = MK_REGIONS_EXACT;     // asked for (mk_session_set_regions_route)
  int ran = MK_REGIONS_EXACT;       // the route of the last tile replay
  double check = 0.0;               // that replay's largest |interpolant - exact| over the entries of S (0: exact route)
  double dmax = 0.0;                // the largest site-to-site distance inside a region (the node-count rule)
};

// The interpolated route's scratch of one tile replay (regions_interp_begin takes it, the replay's return
// frees it): nothing of it exists while the exact route runs.
struct RegionInterp {
  DevBufs bufs;
  double* Sn = nullptr;       // [E][S q][fsz]: the lower triangle of S at every node and check slot, packed like the factors
  double* means = nullptr;    // [S][n_kept][q n_test]: k_pred_cheb_draw's per-outcome means
  double* Lc = nullptr;       // [S q][B][fsz]: the factors of one chunk's phi runs
  int* flagc = nullptr;       // [S q][B][G]
  int* slot = nullptr;        // [n_kept][S q]
  RegionJob* jobs = nullptr;
  unsigned long long* err = nullptr;
  RegionChunkPlan plan;
  int E = 0;
};

// mk_import.hip.  A chain imported by mk_session_import_chain, and what the import cost.
struct Import {
  bool done = false;           // the record (z, theta, A), samples and w_samples are an imported chain's
  bool acc = false;            // the chain came with acceptance rates
  long factorisations = 0;     // (subset, outcome) factor refreshes
  double ms_factor = 0.0, ms_z = 0.0;
  int batch = 0;               // states per pass over W (k_import_z's B)
};

// mk_checkpoint.hip.  A state restored by mk_session_restore, and what the restore cost.
struct Restore {
  bool done = false;
  double ms_derive = 0.0, ms_digest = 0.0, ms_upload = 0.0;
};

}  // namespace mk

struct mk_session {
  mk_session();
  ~mk_session();   // mk_api.hip: the teardown order
  int device = 0;
  hipStream_t stream = nullptr;   // set-up, outputs and the one-group paths
  mk::StreamList owned;           // every stream of the session (pool_stream), back to the pool at the end
  mk::Model md{};
  mk::MatSet ms{};
  int S = 0, q = 1, p = 0, n_pad = 0, nt = 0, P = 0;
  int iter = 0;
  bool matern = false, record_samples = true, record_w = false;
  bool pred_gen = false;          // kriging P^T generated inside k_pred_var (exponential; no P^T buffer)
  mk::Group all;                  // the whole shard on `stream`
  std::vector<mk::Group> groups;  // the run-time split, one stream each
  hipEvent_t swept = nullptr;     // fork-join sweep (several groups): the whole-shard sweep is queued
  bool tiled = false;             // kriging after the fit over test-site tiles (predict_tile)
  int pred_tile = 0, n_test_all = 0, n_test_pad_all = 0;
  int tile_req = 0;               // predict_tile as configured
  int win_lo = 0, win_n = -1;     // tiled kriging: kept states [win_lo, win_lo + win_n) (-1: all)
  std::vector<double> span_pt_h;  // [S] bound on the subset-site to test-site distances (host copy)
  std::vector<void*> kbufs;       // the kriging buffers (re-sized by mk_session_set_test_sites)
  std::vector<double> bbox;       // [S][4] xmin xmax ymin ymax of each subset's sites (Matern table ranges)
  double* d_ct_all = nullptr;     // all test sites [2][n_test_pad_all] (tiled mode)
  double* d_xt = nullptr;         // x_test of the current test sites, (q n_test_all) x p column-major (NULL: none)
  int* d_slist = nullptr;         // tiled replay: per-outcome subset lists [q][S] + counts [q]
  int* d_run_start = nullptr;     // tiled replay, q = 1: first window state of each subset's pending draws
  int* d_scount = nullptr;
  double* d_probs = nullptr;
  mk::Lookahead la;
  mk::EarlyCov cov;
  mk::KrigTables kt;
  mk::ChebWindow cg;
  mk::SweepPlan sweep;
  mk::Profiler prof;
  mk::Criteria crit;
  mk::Validation val;
  mk::Maps maps;
  mk::Pairs pairs;
  mk::Regions regions;
  mk::Import imp;
  mk::Restore rst;
  std::vector<double> ct_h;      // the current test sites on the host, x then y (the regions' coincidence check)
  mk_diagnostics diag_sink{};           // mk_session_set_diagnostics: filled by every tile replay while diag_on
  bool diag_on = false;
  hipError_t launch_err = hipSuccess;   // first failed kernel launch of a run
  const char* poisoned = nullptr;       // set when a run left the chain in a state that is not the sampler's
  std::vector<int> n_part;
  std::vector<void*> allocs;

  // Free one buffer allocated by alloc().
  void release(void* ptr) {
    if (!ptr) return;
    for (size_t i = 0; i < allocs.size(); ++i)
      if (allocs[i] == ptr) {
        hipFree(ptr);
        allocs.erase(allocs.begin() + (long)i);
        return;
      }
  }
  template <typename T>
  int alloc(T** p_, size_t n) {
    void* ptr = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc(&ptr, n * sizeof(T));
    if (e != hipSuccess) {
      (void)hipGetLastError();   // the failed malloc is sticky in hipGetLastError: clear it for later calls
      return mk::set_err(MK_E_NOMEM, std::string("hipMalloc ") + std::to_string(n * sizeof(T)) + " B");
    }
    allocs.push_back(ptr);
    *p_ = (T*)ptr;
    return 0;
  }
};

namespace mk {

static inline hipEvent_t ev_new() {
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

// Launch helper that optionally brackets a kernel with events on its stream.
template <typename F>
static void timed(mk_session* s, hipStream_t st, int which, double flops, F&& launch, int cnt = -1) {
  if (!s->prof.on || !s->prof.iter || !((s->prof.kinds >> which) & 1u)) {
    launch();
    return;
  }
  Timed t{which, ev_new(), ev_new(), flops, cnt};
  hipEventRecord(t.a, st);
  launch();
  hipEventRecord(t.b, st);
  s->prof.pending.push_back(t);
}

// Events around a sink's launches, bracketed whether or not the profiler is on and destroyed on every
// return path.  start and stop record on the stream; price, once the stream is idle, adds the interval and
// the launches it held to the kernel kind's statistics.
struct EventTimer {
  hipEvent_t a = nullptr, b = nullptr;
  EventTimer() = default;
  EventTimer(const EventTimer&) = delete;
  ~EventTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  int start(hipStream_t st) {
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    HIPCHK(hipEventRecord(a, st));
    return 0;
  }
  int stop(hipStream_t st) {
    HIPCHK(hipEventRecord(b, st));
    return 0;
  }
  int price(mk_session* s, int kind, long launches) const {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    Stat& k = s->prof.stats[kind];
    k.launches += launches;
    k.ms += ms;
    return 0;
  }
};

// A run left the chain in a state that is not the sampler's: every later call on the session fails with this.
static inline int poisoned_err(const mk_session* s) {
  return set_err(MK_E_HIP, std::string("session unusable after an earlier failure: ") + s->poisoned);
}

// A sink's words in the errors of its results entry (mk_session_scores, _maps, _pairs).
struct SinkWords {
  const char* null_args;    // "null session/maps"
  const char* off;          // "no posterior maps asked for (mk_session_set_maps)"
  const char* need_iters;   // "posterior maps need all n.samples iterations"
  const char* what;         // tile_missing_msg's two phrases
  const char* attached;
};
// mk_api.hip.  What a results entry checks before it touches the device: the session usable, the sink on,
// the chain complete and, for a tiled session, every tile replayed over the current kept window.
int results_ready(const mk_session* s, const SinkWords& w, bool on, const TileFill& fill);
template <typename Sink>
int results_entry(const mk_session* s, const void* o, Sink mk_session::*sink, const SinkWords& w) {
  if (!s || !o) return set_err(MK_E_ARG, w.null_args);
  return results_ready(s, w, (s->*sink).on, (s->*sink).fill);
}

// A tiled session's sink buffer did not fit: what ends "... bytes per subset and test column: ", verb is
// "does not" or "do not", remedy what follows "a smaller predict_tile, ".
static inline int sink_nomem(const std::string& what, size_t bytes, const char* verb, const char* remedy) {
  return set_err(MK_E_NOMEM, what + std::to_string(bytes) + " B) " + verb +
                                 " fit in HBM beside the kriging buffers: a smaller predict_tile, " + remedy);
}

// Columns per upload of a stand-alone grid entry (n_rows doubles per column): the environment's count, else
// 256 MiB of the grid; 1 .. n_cols.
static inline long col_chunk(const char* env, long n_rows, long n_cols) {
  const long by_bytes = std::max<long>(1, (256L << 20) / (8L * n_rows));
  const long asked = env_int(env, 0);
  return std::min<long>(asked > 0 ? asked : by_bytes, n_cols);
}
// The host grid h (n_cols columns of n_rows) through the device buffer d (chunk columns), chunk by chunk:
// launch(c0, nc) queues the kernel of columns [c0, c0 + nc) on the null stream, where the next chunk's copy
// returns after it.
template <typename F>
int upload_col_chunks(const double* h, long n_rows, long n_cols, long chunk, double* d, F&& launch) {
  for (long c0 = 0; c0 < n_cols; c0 += chunk) {
    const long nc = std::min<long>(chunk, n_cols - c0);
    HIPCHK(hipMemcpy(d, h + (size_t)c0 * n_rows, (size_t)nc * n_rows * 8, hipMemcpyHostToDevice));
    launch(c0, nc);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

// ---- mk_api.hip
Model model_view(const Model& m, int s0, int S);   // subsets [s0, s0 + S) of the shard's arrays
MatSet matset_view(const MatSet& m, int s0);
int setup_groups(mk_session* s, int n_groups);
// The factors, W, z and the statistics as mk_session_create left them (a failed import used them as scratch).
int chain_reinit(mk_session* s);
// A block of grids [S][Ct][200] in HBM to the host, on the session stream and not waited for: every
// subset's columns into [col0, col0 + Ct) of its [C][200] array at h_each, and their sequential sum
// (k_combine into dsum, Ct * 200 doubles) into the same columns of h_sum ([C][200]).  Either host
// array may be NULL.  A fused session's grids are the block col0 = 0, Ct = C.
int grids_to_host(mk_session* s, const double* d_grids, long Ct, long col0, long C, double* h_each, double* h_sum,
                  double* dsum);

// ---- mk_pool.hip
// A stream of this kind on the current device (hipSetDevice(device) done by the caller), recorded
// in `owned` for the session's destructor; pool_return hands every stream of `owned` back, drained.
hipError_t pool_stream(StreamList& owned, hipStream_t* st, int device, int kind, int prio = 0,
                       const std::vector<uint32_t>& mask = {});
void pool_return(StreamList& owned);
int hw_queues();   // hardware queues of this process's HIP runtime

// ---- mk_schedule.hip
void drain_timers(mk_session* s);
bool set_gemm_lds();
int launch_quantiles(unsigned grid, hipStream_t st, const double* data, long subset_stride, long row_stride,
                     int n_rows, int n_cols, const double* probs, int n_probs, double* out);
int launch_quantiles_prob(unsigned grid, hipStream_t st, const double* data, long subset_stride, long row_stride,
                          int n_rows, int n_cols, const double* probs, int n_probs, double* out, const ProbSrc& ps);
void launch_candidates(const Model& md, const MatSet& ms, hipStream_t st, int n_entries, int h0, int hc, int which,
                       int iter, const int* slist = nullptr, const int* scount = nullptr);
void launch_cholesky(mk_session* s, Group& g, int h0, int hc, const int* slist = nullptr, const int* scount = nullptr,
                     hipStream_t crit = nullptr, hipEvent_t* evP = nullptr, int k_lo = 0, int k_hi = -1);
void launch_trinv(mk_session* s, Group& g, int max_entries, const int* list, const int* count);
void launch_inverse(mk_session* s, Group& g, bool from_zc = false);
void launch_pred_refresh(mk_session* s, Group& g, hipStream_t st = nullptr);
bool la_auto(const mk_session* s);   // the default schedule of this shard is the lookahead one
void run_iteration(mk_session* s, int it);

// ---- mk_krig.hip
int kriging_buffers(mk_session* s, int n_test_all, const double* coords_test);
int krig_tables(mk_session* s);
int predict_tile(mk_session* s, int t0, double* dq, mk_outputs* o, double* dqp = nullptr);
int predict_tiled(mk_session* s, mk_outputs* o);
// x_test (C x p column-major, C = q n_test_all; NULL drops it) of the current test sites into HBM
int set_test_covars(mk_session* s, const double* x_test);
// pred_prob's inputs for the draws in md.w_pred: the window's first kept state, test row t0 * q first
ProbSrc prob_src(const mk_session* s, int t0);
// One subset's p draws to the host: k_pred_prob of its [n_rows][n_cols] block of md.w_pred into
// scratch (n_rows * n_cols doubles), then rows ld_dst apart at dst (stream-ordered, not waited for)
int pred_prob_to_host(mk_session* s, int subset, int t0, int n_rows, int n_cols, double* scratch, double* dst,
                      size_t ld_dst);

// ---- mk_diag.hip
// k_chain_diag (ps == NULL) or k_chain_diag_prob of grid chains, n_rows values each (4 .. MK_QUANT_MAX,
// else MK_E_ARG), addressed as launch_quantiles addresses them; out [grid][3] in HBM.  Not waited for.
int launch_chain_diag(unsigned grid, hipStream_t st, const double* data, long subset_stride, long row_stride,
                      int n_rows, int n_cols, double* out, const ProbSrc* ps);
// The diagnostics of the session's S x Ct chains in a draw or sample buffer to the host: every subset's
// [Ct][3] into columns [col0, col0 + Ct) of its [C][3] array at h_each, the worst rows into the same
// columns of h_worst ([C][3]); either may be NULL.  Timed as KS_DIAG; returns after the stream is idle.
int diag_to_host(mk_session* s, const double* data, long subset_stride, long row_stride, int n_rows, long Ct,
                 const ProbSrc* ps, long col0, long C, double* h_each, double* h_worst);
// The attached sink's share of tile [t0, ..): the draws are in md.w_pred ([S][n_kept][Ct]).
int tile_diagnostics(mk_session* s, int t0, int n_kept, int Ct);

// ---- mk_criteria.hip
// Kept iteration kidx of group g (criteria on): k_crit_accum on the group's stream between two events.
void launch_crit_accum(mk_session* s, Group& g, int kidx);
// The events of the launches above: priced into KS_CRIT (price = false: only destroyed).  The streams are idle.
void crit_drain(mk_session* s, bool price);

// ---- mk_scores.hip
// Attached validation data's share of tile [t0, ..): scores the draws in md.w_pred ([S][n_kept][Ct]) into
// the session's pair buffer.  Timed as KS_SCORE; returns after the stream is idle.
int tile_scores(mk_session* s, int t0, int n_kept, int Ct);
// Frees the validation data and the pair buffer (mk_session_set_test_sites; NULL data).
void validation_detach(mk_session* s);

// ---- mk_maps.hip
// The maps' share of tile [t0, ..): the planes of the draws in md.w_pred ([S][n_kept][Ct]) into the
// session's plane buffer.  Timed as KS_MAPS; returns after the stream is idle.
int tile_maps(mk_session* s, int t0, int n_kept, int Ct);
// Frees the plane buffer and forgets the thresholds (mk_session_set_test_sites; a NULL spec).
void maps_detach(mk_session* s);
// thresholds[0 .. J) into th (the slots past J at +inf); MK_E_ARG naming the index of a non-finite value, or J
// when it is outside 0 .. MK_MAP_MAXT.  Touches no device.
int map_thresholds(const double* thresholds, int J, MapThr* th);
// k_map_cols in its values form on values already in HBM (mk_map_grid's kernel; the regional draws): state k of
// column c of subset s is data[s * subset_stride + k * row_stride + c]; planes [S][2 + J][n_cols].  Not waited for.
int launch_map_values(hipStream_t st, const double* data, long subset_stride, long row_stride, int n, int n_cols, int S,
                      const MapThr& th, double* planes);

// ---- mk_pairs.hip
// The pairs' share of tile [t0, ..): the grids and planes of the tile's pair columns, from the draws in
// md.w_pred ([S][n_kept][Ct]), into the session's buffers.  Timed as KS_PAIRS; returns after the stream is idle.
int tile_pairs(mk_session* s, int t0, int n_kept, int Ct);
// Frees the pair buffers and forgets the thresholds (mk_session_set_test_sites; a NULL spec).
void pairs_detach(mk_session* s);

// ---- mk_regions.hip
// The exact tiled replay's hooks while regions are attached.  regions_begin: before the first kept state of
// tile [t0, t0 + Tc) (clears the flagged-factor counts; MK_E_ARG unless the tile holds every test site).
// regions_state: after launch_pred_refresh of window state j (iteration iter) -- the covariances and factors
// of the pairs on g's dirty list, then that state's regional draws of every subset.
int regions_begin(mk_session* s, int t0, int Tc, int n_kept);
int regions_state(mk_session* s, Group& g, const Model& mt, int iter, int j, int n_kept);
// The phi-interpolated replay's hooks while regions are attached on the interpolated route.  Each returns 0,
// an error (< 0) or, regions_interp_begin alone, MK_CHEB_EXACT.
// regions_interp_begin: regions_begin, then the node, means and factor-chunk buffers of a replay with E slots and
// the chunk plan from the window's phi (s->cg.phi_h); MK_CHEB_EXACT when HBM is short: the tile runs exactly.
// regions_node: after launch_pred_refresh of slot e -- S of the pairs on gp's list into the node buffer.
// regions_check: the interpolant of S against the exact S at the check slots (ck: cheb_eval's nodes), the
// largest |difference| into *emax; waits for the stream.
// regions_interp_draws: per chunk the factors of its phi runs, then the regional draws of its states.
int regions_interp_begin(mk_session* s, RegionInterp& ri, int t0, int Tc, int n_kept, int E);
int regions_node(mk_session* s, const Group& gp, RegionInterp& ri, int e);
int regions_check(mk_session* s, RegionInterp& ri, const ChebK& ck, double* emax);
int regions_interp_draws(mk_session* s, RegionInterp& ri, const Model& mt, const ChebK& ck, int n_kept);
// The regions' share of a tile replay: the grids and planes of the regional draws the replay left, timed as
// KS_REGIONS.  Returns after the stream is idle.
int tile_regions(mk_session* s, int t0, int n_kept, int Ct);
// Frees every region buffer and forgets the spec (mk_session_set_test_sites; a NULL spec).
void regions_detach(mk_session* s);

}  // namespace mk
