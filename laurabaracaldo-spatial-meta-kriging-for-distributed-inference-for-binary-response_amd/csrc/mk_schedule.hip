// The per-iteration launch schedule: the Cholesky forms, the inverse, the latent sweep, the lookahead
// and sequential schedules of one MCMC iteration, and the profiler that brackets their launches.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <vector>
#include "mk_gemm.hpp"
#include "mk_session.hpp"

using namespace mk;

void mk::drain_timers(mk_session* s) {
  std::vector<std::pair<float, float>> upd;   // update launches: [start, end] relative to the first event
  for (auto& t : s->prof.pending) {
    hipEventSynchronize(t.b);
    float ms = 0.f;
    hipEventElapsedTime(&ms, t.a, t.b);
    if (t.cnt >= 0) t.flops *= (double)s->prof.inv_cnt[t.cnt];
    s->prof.stats[t.which].launches += 1;
    s->prof.stats[t.which].ms += ms;
    s->prof.stats[t.which].flops += t.flops;
    if (t.which == KS_CHOL_UPDATE || t.which == KS_CHOL_UPDATE_SUB) {
      float t0 = 0.f;
      hipEventElapsedTime(&t0, s->prof.pending.front().a, t.a);
      upd.push_back({t0, t0 + ms});
      s->prof.stats[KS_UPDATE_BUSY].launches += 1;
      s->prof.stats[KS_UPDATE_BUSY].flops += t.flops;
    }
  }
  std::sort(upd.begin(), upd.end());
  double busy = 0.0, lo = 0.0, hi = -1.0;
  for (auto& iv : upd) {
    if (iv.first > hi) {
      if (hi > lo) busy += hi - lo;
      lo = iv.first;
      hi = iv.second;
    } else {
      hi = std::max(hi, (double)iv.second);
    }
  }
  if (hi > lo) busy += hi - lo;
  s->prof.stats[KS_UPDATE_BUSY].ms += busy;
  for (auto& t : s->prof.pending) {
    hipEventDestroy(t.a);
    hipEventDestroy(t.b);
  }
  s->prof.pending.clear();
  s->prof.inv_cnt_used = 0;
}

// Every tile-GEMM kernel takes gb_lds_bytes(TM, TN) of dynamic LDS: two DMA stages (> 64 KiB at 128 x 128).
static constexpr size_t LDS_128 = gb_lds_bytes(128, 128), LDS_64 = gb_lds_bytes(64, 64),
                        LDS_64x128 = gb_lds_bytes(64, 128), LDS_32 = gb_lds_bytes(32, 32),
                        LDS_32x128 = gb_lds_bytes(32, 128);
// The dynamic-LDS limits of the factorisation, inverse and kriging kernels (the diagonal kernel's too).
bool mk::set_gemm_lds() {
  const std::pair<const void*, size_t> fns[] = {
      {(const void*)k_chol_diag, (size_t)MK_DIAG_LDS_BYTES},
      {(const void*)k_chol_update<128>, LDS_128}, {(const void*)k_chol_update<64>, LDS_64},
      {(const void*)k_chol_trsm<128>, LDS_128},   {(const void*)k_chol_trsm<64>, LDS_64x128},
      {(const void*)k_inv_level<128>, LDS_128},   {(const void*)k_inv_level<64>, LDS_64},
      {(const void*)k_chol_update<32>, LDS_32},   {(const void*)k_chol_trsm<32>, LDS_32x128},
      {(const void*)k_chol_update_trsm<128>, LDS_128}, {(const void*)k_chol_update_trsm<64>, LDS_128},
      {(const void*)k_inv_level<32>, LDS_32},
      {(const void*)k_qblocks, LDS_64},           {(const void*)k_lauum, LDS_128},
      {(const void*)k_pred_var<true>, LDS_128},   {(const void*)k_pred_var<false>, LDS_128}};
  for (const auto& f : fns)
    if (hipFuncSetAttribute(f.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.second) != hipSuccess)
      return false;
  return true;
}

// Type-7 quantiles of n_rows kept values per (subset, column) (k_quantiles): the bitonic sort takes
// the next power of two >= n_rows doubles of dynamic LDS (n_rows <= MK_QUANT_MAX).
int mk::launch_quantiles(unsigned grid, hipStream_t st, const double* data, long subset_stride, long row_stride,
                         int n_rows, int n_cols, const double* probs, int n_probs, double* out) {
  HIPCHK(hipFuncSetAttribute((const void*)k_quantiles, hipFuncAttributeMaxDynamicSharedMemorySize, MK_QUANT_MAX * 8));
  if (n_rows < 1 || n_rows > MK_QUANT_MAX)
    return set_err(MK_E_ARG, "quantile summaries take 1 .. " + std::to_string(MK_QUANT_MAX) + " kept samples");
  size_t n2 = 1;
  while (n2 < (size_t)n_rows) n2 <<= 1;
  MK_LAUNCH(k_quantiles, dim3(grid), dim3(256), n2 * 8, st, data, subset_stride, row_stride, n_rows, n_cols,
                     probs, n_probs, out);
  HIPCHK(hipGetLastError());
  return 0;
}

// The same summary of the predictive probabilities of a kriging draw buffer (k_quantiles_prob): data
// and the shape arguments as launch_quantiles takes them, ps as prob_src makes it.
int mk::launch_quantiles_prob(unsigned grid, hipStream_t st, const double* data, long subset_stride, long row_stride,
                              int n_rows, int n_cols, const double* probs, int n_probs, double* out, const ProbSrc& ps) {
  HIPCHK(hipFuncSetAttribute((const void*)k_quantiles_prob, hipFuncAttributeMaxDynamicSharedMemorySize, MK_QUANT_MAX * 8));
  if (n_rows < 1 || n_rows > MK_QUANT_MAX)
    return set_err(MK_E_ARG, "quantile summaries take 1 .. " + std::to_string(MK_QUANT_MAX) + " kept samples");
  size_t n2 = 1;
  while (n2 < (size_t)n_rows) n2 <<= 1;
  MK_LAUNCH(k_quantiles_prob, dim3(grid), dim3(256), n2 * 8, st, data, subset_stride, row_stride, n_rows, n_cols,
                     probs, n_probs, out, ps);
  HIPCHK(hipGetLastError());
  return 0;
}

// Tile shape of a GEMM launch: 64-sub-tiles (bit-identical, mk_gemm.hpp) when the 128-tile grid
// would leave the chip short of work -- fewer than 256 workgroups (one per CU; 512 before the
// lookahead schedule, whose concurrent chain fills the rest: 32 subsets 6,360 -> 6,546
// subset-iters/s, 250 subsets unchanged; other thresholds: DESIGN.md B.1, B.5).  MK_TILE=128 / 64 /
// 32 forces one shape (tests compare them; 32-sub-tiles were measured no faster than 64 on the last,
// single-tile panels of small shards, so the policy does not pick them).
static int tile_size(long wg128) {
  static const int force = env_int("MK_TILE", 0);
  if (force == 32 || force == 64 || force == 128) return force;
  return wg128 >= 256 ? 128 : 64;
}

// ------------------------------------------------------------------ candidate assembly
// Candidate matrices of n_entries (subset, outcome) entries (k_cov_candidate); Matern sessions
// first store each entry's Chebyshev table (k_matern_table, one workgroup per entry), which the
// tile workgroups then load.
void mk::launch_candidates(const Model& md, const MatSet& ms, hipStream_t st, int n_entries, int h0, int hc, int which,
                           int iter, const int* slist, const int* scount) {
  if (md.cov_model == MK_COV_MATERN && md.chtab)
    MK_LAUNCH(k_matern_table, dim3(n_entries), dim3(256), 0, st, md, h0, hc, which, iter, slist, scount);
  const int ntiles = ms.nt * (ms.nt + 1) / 2;
  MK_LAUNCH(cov_candidate_kernel(md.cov_model), dim3(xcd_grid_h(n_entries, ntiles)),
                     dim3(256), 0, st, md, ms, h0, hc, which, iter, slist, scount);
}

// ------------------------------------------------------------------ Cholesky of all candidates of outcome h
// Candidate tiles are in the free slot (k_cov_candidate, or k_load_plain for the test entry).
// One launch per step covers outcomes h0 .. h0+hc-1 of every subset (hc = q in the sampler).
// Launch pieces of the blocked Cholesky for panel k, tiles [ia, ib), on stream st.

// MK_DIAG_SYRK (default 1, read once per process): the diagonal 128-tiles' updates -- the fused
// launches' extra job, the correction folded into the diagonal launch, and the 128-tile instance of
// k_chol_update -- run the balanced lower-block body (gemm_syrk_128, mk_gemm.hpp), and the fused
// launches deal their (now shorter) extra jobs after the row jobs (xcd_map_tail); 0: the full-square
// bodies in the former order.  An argument of the kernels, so one build serves both arms of an A/B;
// same bits on every element that is read.
static int diag_syrk() {
  static const int on = env_int("MK_DIAG_SYRK", 1);
  return on != 0;
}

// MK_INV_DEAL (default 1, read once per process): the 128-tile inverse levels deal the 16-blocks of
// their triangular K block evenly over the waves and keep the predicates out of the dense chunks
// (gemm_deal_128, mk_gemm.hpp); 0: the quadrant body with a predicate before every MFMA.  An argument
// of the kernel, so one build serves both arms of an A/B; same bits.
static int inv_deal() {
  static const int on = env_int("MK_INV_DEAL", 1);
  return on != 0;
}

// MK_RAGGED (default 1, read once per process): a 128-row job of the fused column update whose row
// tile holds at most six valid 16-row blocks (the last tile of a factor of extent n_s + 1 < n_pad) runs
// its K loop in column strips (gemm_tile_cs, mk_gemm.hpp) and leaves the padding row blocks alone, and
// a launch whose last row tile is ragged in this way for its largest factor deals that tile's jobs
// after the full row jobs and before the extra jobs: longest first (xcd_map_tail2).  0: the row-wave
// body on all eight blocks, in the former order.  An argument of the kernel, so one build serves both
// arms of an A/B; same bits on every valid element.
static int ragged() {
  static const int on = env_int("MK_RAGGED", 1);
  return on != 0;
}
// The kernel's argument: 0 off, 1 the strips, 2 the strips and the order.  The order is per launch, so
// it goes by the group's largest factor (n_pad is cut to the session's largest: its last tile is the
// launch's last row tile); a smaller factor's ragged tile keeps its place among the full row jobs.
static int ragged_arg(mk_session* s, const Group& g) {
  if (!ragged()) return 0;
  int nmax = 0;
  for (int i = g.s0; i < g.s0 + g.S; ++i) nmax = std::max(nmax, (int)s->n_part[i]);
  const int v = (nmax + 1 - (s->nt - 1) * MK_NB + 15) / 16;
  return v >= 1 && v <= CS_VMAX ? 2 : 1;
}

// MK_INV_MAP (default 1, read once per process): the inverse levels' launches cut their tile jobs over
// the XCDs by work and start the longest K ranges first (inv_map_job, mk_types.hpp); 0: xcd_map's cut
// by item count in the matrices' item order, on its own grid.  An argument of the kernel, so one build
// serves both arms of an A/B; only which workgroup computes which tile differs: same bits.
static int inv_map() {
  static const int on = env_int("MK_INV_MAP", 1);
  return on != 0;
}
// Blocks of a level's launch for up to max_entries listed factors on sub sub-tiles per 128-tile.
static int inv_grid(int map, int max_entries, int nt, int sz, int sub) {
  if (map) return inv_map_grid(max_entries, nt, sz, sub);
  return xcd_grid_h(max_entries, (nt + 2 * sz - 1) / (2 * sz) * sz * sz * sub);
}
// Test entry of the map (include/mk.h): the launch grid, and what each of its blocks computes, by the
// kernel's own code on the host.
extern "C" int mk_inv_map_jobs(int32_t map, int32_t count, int32_t max_entries, int32_t nt, int32_t sz, int32_t phase,
                               int32_t sub, int32_t* out, int32_t cap) {
  const int grid = inv_grid(map, max_entries, nt, sz, sub);
  for (int b = 0; out && b < grid && b < cap; ++b) {
    int e, p, i, j, st;
    const bool job = map ? inv_map_job(count, nt, sz, phase, sub, b, &e, &p, &i, &j, &st)
                         : inv_xcd_job(count, nt, sz, phase, sub, b, &e, &p, &i, &j, &st);
    int32_t* o = out + 5 * (long)b;
    o[0] = job ? e : -1, o[1] = job ? p : -1, o[2] = job ? i : -1, o[3] = job ? j : -1, o[4] = job ? st : -1;
  }
  return grid;
}

static void chol_update(mk_session* s, Group& g, hipStream_t st, int h0, int hc, int k, int ia, int ib, int j0, int j1,
                        const int* slist, const int* scount, double flops) {
  const int E = g.S * hc, nti = ib - ia;
  if (nti <= 0) return;
  const int tm = tile_size((long)E * nti);
  if (tm == 32) {
    timed(s, st, KS_CHOL_UPDATE_SUB, flops, [&] {
      MK_LAUNCH(k_chol_update<32>, dim3(xcd_grid_h(E, nti * 16)), dim3(256), LDS_32, st, g.ms, g.S, h0, hc, k, ia,
                         ib, j0, j1, slist, scount, diag_syrk());
    });
  } else if (tm == 64) {
    timed(s, st, KS_CHOL_UPDATE_SUB, flops, [&] {
      MK_LAUNCH(k_chol_update<64>, dim3(xcd_grid_h(E, nti * 4)), dim3(256), LDS_64, st, g.ms, g.S, h0, hc, k, ia,
                         ib, j0, j1, slist, scount, diag_syrk());
    });
  } else {
    timed(s, st, KS_CHOL_UPDATE, flops, [&] {
      MK_LAUNCH(k_chol_update<128>, dim3(xcd_grid_h(E, nti)), dim3(256), LDS_128, st, g.ms, g.S, h0, hc, k, ia,
                         ib, j0, j1, slist, scount, diag_syrk());
    });
  }
}
static void chol_trsm(mk_session* s, Group& g, hipStream_t st, int h0, int hc, int k, int ia, int ib, const int* slist,
                      const int* scount, double flops) {
  const int E = g.S * hc, nti = ib - ia;
  if (nti <= 0) return;
  const int tm = tile_size((long)E * nti);
  timed(s, st, KS_CHOL_TRSM, flops, [&] {
    if (tm == 32)
      MK_LAUNCH(k_chol_trsm<32>, dim3(xcd_grid_h(E, nti * 4)), dim3(256), LDS_32x128, st, g.ms, g.S, h0, hc, k,
                         ia, ib, slist, scount);
    else if (tm == 64)
      MK_LAUNCH(k_chol_trsm<64>, dim3(xcd_grid_h(E, nti * 2)), dim3(256), LDS_64x128, st, g.ms, g.S, h0, hc, k,
                         ia, ib, slist, scount);
    else
      MK_LAUNCH(k_chol_trsm<128>, dim3(xcd_grid_h(E, nti)), dim3(256), LDS_128, st, g.ms, g.S, h0, hc, k, ia, ib,
                         slist, scount);
  });
}
// F(k): column k's update of tiles k+1.. by panels [j0, k) with the panel solve in the epilogue
// (k_chol_update_trsm, 1 <= k < nt - 1), plus (extra) the next diagonal tile's update by panels [0, k).
static void chol_update_trsm(mk_session* s, Group& g, hipStream_t st, int h0, int hc, int k, int j0, int extra,
                             const int* slist, const int* scount, double flops) {
  const int E = g.S * hc, nt = s->nt, nti = nt - (k + 1);
  const int tm = tile_size((long)E * (nti + extra));
  timed(s, st, tm == 128 ? KS_CHOL_UPDATE : KS_CHOL_UPDATE_SUB, flops, [&] {
    if (tm == 128)
      MK_LAUNCH(k_chol_update_trsm<128>, dim3(xcd_grid_h(E, nti + extra)), dim3(256), LDS_128, st, g.ms, g.S, h0, hc,
                k, k + 1, nt, j0, extra, slist, scount, diag_syrk(), g.md.n_s, ragged_arg(s, g));
    else
      MK_LAUNCH(k_chol_update_trsm<64>, dim3(xcd_grid_h(E, 2 * nti + extra)), dim3(256), LDS_128, st, g.ms, g.S, h0,
                hc, k, k + 1, nt, j0, extra, slist, scount, diag_syrk(), g.md.n_s, 0);
  });
}
// cj0 < cj1: the diagonal tile's update by panels [cj0, cj1) first, in the same launch (fused form).
static void chol_diag(mk_session* s, Group& g, hipStream_t st, int h0, int hc, int k, const int* slist,
                      const int* scount, int cj0 = 0, int cj1 = 0, double flops = 0.0) {
  timed(s, st, KS_CHOL_DIAG, flops, [&] {
    MK_LAUNCH(k_chol_diag, dim3(g.S * hc), dim3(256), (size_t)MK_DIAG_LDS_BYTES, st, g.ms, g.md.n_s, h0, hc, k,
                       g.md.ld_part, g.md.quad_c, g.md.info, slist, scount, cj0, cj1, diag_syrk());
  });
}

// Algorithmic flops of the column-k update over panels [j0, j1) (trsm: of panel k) of tiles
// [ia, ib): every (subset, outcome) factor counted over its own valid extent n_s + 1 (the
// bordered row; padding excluded), so ragged subsets (MK.R:18: the last takes the remainder) are
// priced exactly.  Algorithmic, not executed: an off-diagonal tile's update is a GEMM,
// 2 rows cols depth; the diagonal tile's (tile k of column k) a SYRK, cols (cols + 1) depth; the
// panel solve L(i,k) = C(i,k) L(k,k)^-T a triangular solve, rows cols^2 (the kernels skip most of the
// triangle's zero MFMA blocks but not all of them: what they execute is more than this).  With a
// subset list (tiled kriging replay) the active subsets live on the device: the count is then an
// upper bound (every subset).
static double panel_flops(mk_session* s, Group& g, int hc, int k, int ia, int ib, bool trsm, int j0 = 0, int j1 = -1) {
  if (j1 < 0) j1 = k;
  double fl = 0.0;
  for (int i = g.s0; i < g.s0 + g.S; ++i) {
    const double nv = (double)s->n_part[i] + 1.0;
    const double cols = std::fmin((double)MK_NB, std::fmax(0.0, nv - (double)k * MK_NB));
    const double depth = std::fmax(0.0, std::fmin((double)j1 * MK_NB, nv) - (double)j0 * MK_NB);
    const bool diag = ia <= k && k < ib;   // tile k of column k is in [ia, ib)
    const double lo = (double)(diag ? k + 1 : ia) * MK_NB;
    const double rows = std::fmax(0.0, std::fmin(nv, (double)ib * MK_NB) - lo);   // off-diagonal rows
    if (trsm)
      fl += rows * cols * cols;
    else
      fl += 2.0 * rows * cols * depth + (diag ? cols * (cols + 1.0) * depth : 0.0);
  }
  return fl * hc;
}

// Algorithmic flops of one factor's inverse level (k_inv_level, level sz, phase): over the pairs of
// blocks T = tiles [T0, T0+sz), B = [T0+sz, T0+2sz) clipped to the extent n, phase 0 Y = L_BT W_TT is
// a full-by-triangular product (|B| |T|^2), phase 1 W_BT = -W_BB Y a triangular-by-full one (|B|^2 |T|).
// Summed over the levels with the diagonal tiles' inverses (k_chol_diag's) this is n^3 / 3.
static double inv_level_flops(int n, int nt, int sz, int phase) {
  double fl = 0.0;
  for (int T0 = 0; T0 < nt; T0 += 2 * sz) {
    const double t0 = (double)T0 * MK_NB, b0 = (double)(T0 + sz) * MK_NB, b1 = (double)(T0 + 2 * sz) * MK_NB;
    const double bt = std::fmax(0.0, std::fmin((double)n, b0) - t0), bb = std::fmax(0.0, std::fmin((double)n, b1) - b0);
    fl += phase == 0 ? bb * bt * bt : bb * bb * bt;
  }
  return fl;
}

// Cholesky of all candidates of outcomes h0 .. h0+hc-1 (candidate tiles in the free slot), left-
// looking by 128-panels: per column k the update by panels < k, the diagonal tile, the trsm of
// tiles k+1.. .
//
// Sequential form (one stream): U(k; panels 0..k-1), D(k), T(k).  Fused (MK_CHOL_FUSED, default on;
// 0 restores U, D, T): D(0), T(0), then per k >= 1
//   D(k)  the diagonal tile's last panel k-1 (its panels [0, k-1) came with F(k-1); k = 1: panel 0)
//         applied inside the diagonal launch, then the factor,
//   F(k)  tiles k+1.. of column k, update and solve in one launch (C(i,k) stays in registers), plus
//         the next diagonal tile by panels [0, k)
// -- no C(i,k) round trip through HBM between the update and the solve; same bits.  (The split form
// below stays unfused: there F(k) would put the off-diagonal tiles' critical correction after the
// diagonal factor instead of beside the diagonal tile's -- a longer chain; 32 subsets 7,479-7,597 vs
// 8,059-8,078 subset-iters/s)
//
// Split form (small shards, g.bulk set): the update of column c by panels 0..c-2 only needs
// panels that are final two steps earlier, so it runs on the CU-masked bulk stream beside the
// critical chain, which keeps only the rank-128 correction by panel c-1:
//   critical (g.stream, all CUs):  U(k; k-1) [after bulk U(k; 0..k-2)], D(k), T(k)
//   bulk (g.bulk, CUs minus the first `reserve`): U(k+2; 0..k) after T(k)
// The diagonal kernel (one 149 KB-LDS workgroup per matrix) then finds idle CUs at once instead
// of waiting for update workgroups to drain.  Same kernels, same per-element MFMA sequence (the
// accumulator passes through fp64 memory between the two updates): same bits.  (An earlier
// lookahead that moved the full-depth update of the next diagonal tile onto a second stream was
// slower: that update's long K chain sat on the critical path)
//
// crit: the critical stream (default g.stream; the lookahead schedule factors on its own stream).
// evP (optional, nt events): evP[k] is recorded on it once panel k is final (after T(k); the last
// after D(nt-1)), for the border solve that trails the factorisation.
// [k_lo, k_hi): the panels to enqueue (the lookahead schedule enqueues a factorisation in two
// pieces around the main stream's work, so the host does not hold back either stream).
void mk::launch_cholesky(mk_session* s, Group& g, int h0, int hc, const int* slist, const int* scount,
                         hipStream_t crit, hipEvent_t* evP, int k_lo, int k_hi) {
  const int nt = s->nt;
  if (k_hi < 0) k_hi = nt;
  hipStream_t A = crit ? crit : g.stream;
  static const int fused = env_int("MK_CHOL_FUSED", 1);
  if ((slist || !g.bulk) && fused) {
    for (int k = k_lo; k < k_hi; ++k) {
      // X(k) inside D(k): the diagonal tile's last panel (k = 1: panel 0) before it factors
      const int j0 = k >= 2 ? k - 1 : 0;
      chol_diag(s, g, A, h0, hc, k, slist, scount, j0, k, k > 0 ? panel_flops(s, g, hc, k, k, k + 1, false, j0, k) : 0.0);
      if (k == 0 && nt > 1)
        chol_trsm(s, g, A, h0, hc, 0, 1, nt, slist, scount, panel_flops(s, g, hc, 0, 1, nt, true));
      else if (k > 0 && k < nt - 1)
        chol_update_trsm(s, g, A, h0, hc, k, 0, 1, slist, scount,
                         panel_flops(s, g, hc, k, k + 1, nt, false) + panel_flops(s, g, hc, k, k + 1, nt, true) +
                             panel_flops(s, g, hc, k + 1, k + 1, k + 2, false, 0, k));
      if (evP) hipEventRecord(evP[k], A);
    }
    return;
  }
  if (slist || !g.bulk) {
    for (int k = k_lo; k < k_hi; ++k) {
      if (k > 0)
        chol_update(s, g, A, h0, hc, k, k, nt, 0, k, slist, scount, panel_flops(s, g, hc, k, k, nt, false));
      chol_diag(s, g, A, h0, hc, k, slist, scount);
      if (k < nt - 1)
        chol_trsm(s, g, A, h0, hc, k, k + 1, nt, slist, scount, panel_flops(s, g, hc, k, k + 1, nt, true));
      if (evP) hipEventRecord(evP[k], A);
    }
    return;
  }
  // depth d (MK_CHOL_DEPTH, default 2): the bulk update of column c covers panels [0, c-d) and is
  // launched after T(c-d-1), so it has d critical steps to finish; the critical correction is
  // then rank-128d, U(k; k-d..k-1).  Same per-element MFMA sequence for any d (same bits).
  static const int depth_env = env_int("MK_CHOL_DEPTH", 2);
  const int d = std::max(1, std::min(depth_env, 4));
  hipStream_t B = g.bulk;
  hipEvent_t* eT = g.ev.data();                  // eT[k]: T(k) done (critical)
  hipEvent_t* eU = g.ev.data() + nt;             // eU[c]: bulk U(c; 0..c-d-1) done, c = d+1 .. nt-1
  if (k_lo == 0) {
    hipEventRecord(g.ev[2 * nt], A);             // the candidates are on A
    hipStreamWaitEvent(B, g.ev[2 * nt], 0);
  }
  for (int k = k_lo; k < k_hi; ++k) {
    if (k > d) hipStreamWaitEvent(A, eU[k], 0);
    if (k >= 1) {
      const int j0 = std::max(0, k - d);
      chol_update(s, g, A, h0, hc, k, k, nt, j0, k, nullptr, nullptr, panel_flops(s, g, hc, k, k, nt, false, j0, k));
    }
    chol_diag(s, g, A, h0, hc, k, nullptr, nullptr);
    if (k < nt - 1)
      chol_trsm(s, g, A, h0, hc, k, k + 1, nt, nullptr, nullptr, panel_flops(s, g, hc, k, k + 1, nt, true));
    if (evP) hipEventRecord(evP[k], A);
    if (k + d + 1 < nt) {
      const int c = k + d + 1;
      hipEventRecord(eT[k], A);
      hipStreamWaitEvent(B, eT[k], 0);
      chol_update(s, g, B, h0, hc, c, c, nt, 0, c - d, nullptr, nullptr, panel_flops(s, g, hc, c, c, nt, false, 0, c - d));
      hipEventRecord(eU[c], B);
    }
  }
}

// W = L^-1 of the listed pairs: diagonal tiles, then recursive doubling.
void mk::launch_trinv(mk_session* s, Group& g, int max_entries, const int* list, const int* count) {
  const int nt = s->nt;
  MK_LAUNCH(k_inv_copydiag, dim3(max_entries * nt * MK_CD_SPLIT), dim3(256), 0, g.stream, g.ms, list, count);
  // profiled: the listed count in stream order into a pinned slot (drain_timers multiplies the
  // per-factor flops below by it); no slot left -> the launches run untimed
  int cnt = -1;
  if (s->prof.on && s->prof.iter && ((s->prof.kinds >> KS_INV) & 1u)) {
    if (!s->prof.inv_cnt && hipHostMalloc((void**)&s->prof.inv_cnt, Profiler::INV_CNT_CAP * sizeof(int)) != hipSuccess) {
      (void)hipGetLastError();
      s->prof.inv_cnt = nullptr;
    }
    if (s->prof.inv_cnt && s->prof.inv_cnt_used < Profiler::INV_CNT_CAP) {
      cnt = s->prof.inv_cnt_used++;
      hipMemcpyAsync(s->prof.inv_cnt + cnt, count, sizeof(int), hipMemcpyDeviceToHost, g.stream);
    }
  }
  for (int sz = 1; sz < nt; sz *= 2) {
    const int npairs = (nt + 2 * sz - 1) / (2 * sz);
    // the grid is sized for every pair, but only the accepted candidates' factors are in the
    // list (about 40% at the amcmc target rate) and the level's K ranges are uneven: price the
    // launch at an eighth of its 128-tile grid (measured: 32 subsets 1.33 -> 1.16 ms per iteration)
    const int tm = tile_size((long)max_entries * npairs * sz * sz / 8);
    // the map's integers stay below 2^31 at every shape a session can hold (8 (entries + 1) work is
    // 5e8 at nt = 64 with 250 entries); a launch past that keeps xcd_map, a correct placement, and
    // says so once
    const bool fits = inv_map_fits(max_entries, nt, sz);
    if (inv_map() && !fits) {
      static bool said = false;
      if (!said) fprintf(stderr, "libmk: inverse level of %d entries, nt = %d: job map too large, equal-count cut used\n", max_entries, nt);
      said = true;
    }
    const int map = inv_map() && fits;
    for (int phase = 0; phase < 2; ++phase) {
      // per listed factor: the mean over the group's subsets (exact for equal subset sizes)
      double per = 0.0;
      if (cnt >= 0) {
        for (int i = g.s0; i < g.s0 + g.S; ++i) per += inv_level_flops(s->n_part[i], nt, sz, phase);
        per /= std::max(1, g.S);
      }
      const int sub = (MK_NB / tm) * (MK_NB / tm);
      const int grid = inv_grid(map, max_entries, nt, sz, sub);
      auto launch = [&] {
        if (tm == 32)
          MK_LAUNCH(k_inv_level<32>, dim3(grid), dim3(256), LDS_32, g.stream, g.ms, list, count, sz, phase, inv_deal(),
                    map);
        else if (tm == 64)
          MK_LAUNCH(k_inv_level<64>, dim3(grid), dim3(256), LDS_64, g.stream, g.ms, list, count, sz, phase, inv_deal(),
                    map);
        else
          MK_LAUNCH(k_inv_level<128>, dim3(grid), dim3(256), LDS_128, g.stream, g.ms, list, count, sz, phase,
                    inv_deal(), map);
      };
      if (cnt >= 0)
        timed(s, g.stream, KS_INV, per, launch, cnt);
      else
        launch();     // not profiled, or no count slot (untimed: the stats' ms and flops stay paired)
    }
  }
}

// W = L^-1 for the changed factors, diagonal tiles of R^-1, z from the bordered row.
void mk::launch_inverse(mk_session* s, Group& g, bool from_zc) {
  const int nt = s->nt, max_entries = g.S * s->q;
  launch_trinv(s, g, max_entries, g.d_list, g.d_count);
  // the diagonal tiles of R^-1 feed the 64-site-block sweeps only; the site sweep reads W alone
  if (!s->sweep.site)
    timed(s, g.stream, KS_LAUUM, 0.0, [&] {
      MK_LAUNCH(k_qblocks, dim3(xcd_grid_h(max_entries, nt * 2)), dim3(256), LDS_64, g.stream, g.ms, g.md.n_s,
                g.d_list, g.d_count);
    });
  MK_LAUNCH(k_take_border, dim3(max_entries * ((s->n_pad + 255) / 256)), dim3(256), 0, g.stream, g.md, g.ms,
                     g.d_list, g.d_count, from_zc ? (const double*)g.md.zc : nullptr);
}

// Algorithmic flops of k_pred_var over every pair of the group: 2 n_s^2 / 2 per test site (W
// lower-triangular) -- an upper bound, the list holds the pairs whose factor changed.
static double pred_flops(mk_session* s, Group& g) {
  double fl = 0.0;
  for (int i = g.s0; i < g.s0 + g.S; ++i) fl += (double)s->n_part[i] * s->n_part[i] * g.md.n_test;
  return fl * s->q;
}

// Kriging refresh (kept iterations): X = W P^T and s = |X_t|^2 for the pairs in the pred list
// (P^T generated in the GEMM for the exponential model, else stored first by k_pred_PT).
void mk::launch_pred_refresh(mk_session* s, Group& g, hipStream_t st) {
  Model& md = g.md;
  if (md.n_test <= 0) return;
  if (!st) st = g.stream;
  const int nt = s->nt, max_entries = g.S * s->q;
  if (md.cov_model == MK_COV_MATERN && md.chtab_p)
    MK_LAUNCH(k_matern_table_list, dim3(max_entries), dim3(256), 0, st, md, g.d_plist, g.d_pcount);
  if (md.cov_model == MK_COV_MATERN)
    MK_LAUNCH(k_pred_PT_matern, dim3(max_entries * (md.n_pad / MK_PT_RB)), dim3(256), 0, st, md, g.d_plist,
                       g.d_pcount);
  else if (!s->pred_gen)
    MK_LAUNCH(pred_PT_kernel(md.cov_model), dim3(max_entries * md.n_pad), dim3(256), 0, st, md, g.d_plist,
                       g.d_pcount);
  timed(s, st, KS_PRED_VAR, pred_flops(s, g), [&] {
    MK_LAUNCH(s->pred_gen ? k_pred_var<true> : k_pred_var<false>, dim3(pv_grid(max_entries, nt, md.ntt)),
              dim3(256), LDS_128, st, md, g.ms, g.d_plist, g.d_pcount);
  });
  MK_LAUNCH(k_pred_var_reduce, dim3(max_entries * (md.n_test_pad / 256)), dim3(256), 0, st, md, nt,
                     g.d_plist, g.d_pcount);
}

// Default schedule: lookahead for shards of up to 224 (subset, outcome) pairs, where the chains
// leave the chip room to overlap (measured vs sequential: 32 subsets 5,427 -> 6,972, 63 6,174 ->
// 7,719, 125 7,486 -> 8,303, 188 8,071 -> 8,486 subset-iters/s); at 250 subsets both saturate the
// chip and the sequential schedule is as fast (8,572 vs 8,553-8,565) while its panel-update
// launches run alone (roofline timing 0.71 of peak vs 0.52-0.57 beside the main stream's kernels).
// With the lean sweep, at 250 subsets the lookahead schedule gains 0.9 % (10,574-10,579 sequential vs
// 10,660-10,686, three interleaved 40-step windows each, profiles/r04/la250/) but its update launches
// share the chip, so each launch's own rate reads ~0.55 instead of ~0.70 of peak; the sequential
// schedule stays the default there (MK_LOOKAHEAD=1 takes the 0.9 %).
bool mk::la_auto(const mk_session* s) { return (long)s->S * s->q <= 224; }

// The multi-workgroup sweep is a plain launch on either schedule: its admission consensus
// (k_sweep_mg) sweeps a subset only once all its workgroups are resident, and the k_sweep launch
// queued behind it sweeps the rest -- no wait depends on co-residency the hardware does not give
// (how it got there: DESIGN.md 4.3 and 4.6).
static bool use_sweep_mg(const mk_session* s) { return s->sweep.coop; }

// The latent-w sweep: the multi-workgroup kernel when the session chose it (small shard; g is then
// the whole-shard view), else the site sweep or one workgroup per subset; the block sweeps give the
// same bits (mk_mcmc.hip).
static void launch_sweep(mk_session* s, Group& g, int it) {
  const int q = s->q;
  Model md = g.md;
  MatSet ms = g.ms;
  int iter = it;
  hipError_t e = hipSuccess;
  if (s->sweep.site) {
    void* args[] = {&md, &ms, &iter};
    e = hipLaunchKernel(sweep_site_kernel(q, s->sweep.site, s->sweep.lean), dim3(g.S), dim3(MK_SS_T), args,
                        s->sweep.site_lds, g.stream);
    wd_trace(g.stream, "k_sweep_site");
  } else if (use_sweep_mg(s)) {
    hipMemsetAsync(s->sweep.sw_cnt, 0, (size_t)s->S * (s->n_pad / 64 + 1) * sizeof(int), g.stream);   // g: the whole shard
    double* part = s->sweep.sw_part;
    int* cnt = s->sweep.sw_cnt;
    int* xcc = s->sweep.sw_xcc;
    int* err = s->sweep.sw_err;
    int* adm = s->sweep.sw_adm;
    int spins = s->sweep.adm_spins;
    void* args[] = {&md, &ms, &iter, &part, &cnt, &xcc, &err, &adm, &spins};
    e = hipLaunchKernel(sweep_kernel(q, true), dim3(xcd_grid(g.S, s->nt)), dim3(256), args, s->sweep.mg_lds,
                        g.stream);
    wd_trace(g.stream, "k_sweep_mg");
    if (e == hipSuccess) {   // the subsets k_sweep_mg did not admit (normally none: every workgroup returns at once)
      const size_t sw_lds = (size_t)q * (64 * 64 + 2 * 64) * sizeof(double);
      const int* cadm = adm;
      int* fb = s->sweep.sw_err + 1;
      void* fa[] = {&md, &ms, &iter, &cadm, &fb};
      e = hipLaunchKernel(sweep_kernel(q, false), dim3(g.S), dim3(MK_SW_T), fa, sw_lds, g.stream);
      wd_trace(g.stream, "k_sweep(fallback)");
    }
  } else if (s->sweep.split) {   // one launch per 64-site block, ordered by the stream (no waits on the device)
    int nmax = 1;
    for (int i = g.s0; i < g.s0 + g.S; ++i) nmax = std::max(nmax, s->n_part[i]);
    const int nblk = (nmax + 63) / 64, nt = s->nt;
    double* part = s->sweep.sp_part + (long)g.s0 * 2 * nt * q * 64;
    const size_t lds = (size_t)q * (64 * 64 + 2 * 64) * sizeof(double) + 4 * MK_NB * sizeof(double);
    for (int B = 0; B <= nblk && e == hipSuccess; ++B) {
      void* ta[] = {&md, &ms, &iter, &B, &part};
      e = hipLaunchKernel(sweep_step_kernel(q), dim3(g.S * nt), dim3(256), ta, lds, g.stream);
      wd_trace(g.stream, "k_sweep_step");
    }
  } else {
    const size_t sw_lds = (size_t)q * (64 * 64 + 2 * 64) * sizeof(double);
    const int* adm = nullptr;
    int* fb = nullptr;
    void* args[] = {&md, &ms, &iter, &adm, &fb};
    e = hipLaunchKernel(sweep_kernel(q, false), dim3(g.S), dim3(MK_SW_T), args, sw_lds, g.stream);
    wd_trace(g.stream, "k_sweep");
  }
  if (e != hipSuccess && s->launch_err == hipSuccess) s->launch_err = e;
}

// The stream st waits for the table draws queued on the side stream (iteration_post_sweep).
static void kt_wait(mk_session* s, hipStream_t st) {
  if (!s->kt.pending) return;
  hipStreamWaitEvent(st, s->kt.ev[1], 0);
  s->kt.pending = false;
}

// One MCMC iteration of a group, in two halves around the latent sweep (run_iterations).
static void iteration_pre_sweep(mk_session* s, Group& g, int it) {
  Model& md = g.md;
  const int S = g.S, q = s->q;
  const bool kept = it >= md.kept0;
  hipStream_t st = g.stream;
  MK_LAUNCH(k_beta, dim3(S), dim3(256), 0, st, md, it);
  if (q > 1) MK_LAUNCH(k_trmv_Z, dim3(S * q * ((s->n_pad + 255) / 256)), dim3(256), 0, st, md, g.ms);
  MK_LAUNCH(k_Aphase, dim3(S), dim3(256), 0, st, md, it);
  const int nkinds = s->matern ? 2 : 1;
  // the q outcomes' (phi_h, nu_h) steps are independent given u: one batched pass per kind
  for (int which = 0; which < nkinds; ++which) {
    if (which == 0 && s->cov.pre == it) {   // assembled beside the previous sweep: the bordered row now
      hipStreamWaitEvent(st, s->cov.ev[1], 0);
      MK_LAUNCH(k_cand_border, dim3(S * q * ((s->n_pad + 255) / 256)), dim3(256), 0, st, md, g.ms, 0, q);
      s->cov.pre = -1;
    } else {
      timed(s, st, KS_COV, 0.0, [&] { launch_candidates(md, g.ms, st, S * q, 0, q, which, it); });
    }
    launch_cholesky(s, g, 0, q);
    MK_LAUNCH(k_theta_mh, dim3((S * q + 63) / 64), dim3(64), 0, st, md, g.ms, 0, q, which, it);
  }
  MK_LAUNCH(k_dirty_list, dim3(1), dim3(256), 0, st, md, (int)(it == md.kept0), g.d_list, g.d_count,
                     g.d_plist, g.d_pcount);
  kt_wait(s, st);   // the previous kept iteration's draws read W
  launch_inverse(s, g);
  if (kept && !s->tiled && !s->kt.on) launch_pred_refresh(s, g);
  // the next iteration's phi candidates depend only on this iteration's decisions (and on the proposal
  // scale, which adapts after a batch's last iteration): assemble them on cov.st beside the sweep into
  // the free factor slots, which nothing reads from here to the next iteration's Cholesky (the
  // inverse's scratch is Y).  250 subsets, 40-step windows interleaved: 11,075-11,120 vs 11,034-11,063
  // in line (profiles/r06/earlycov; both VALU-heavy, the sweep slows 0.95 -> 1.2 ms, the assembly
  // stretches to 1.9 ms beside it); started at the decision instead, beside the inverse, 11,011-11,029
  // (the inverse 4.65 -> 5.69 ms).
  if (s->cov.st && it + 1 < md.n_samples && (it + 1) % md.batch_length != 0) {
    hipEventRecord(s->cov.ev[0], st);
    hipStreamWaitEvent(s->cov.st, s->cov.ev[0], 0);
    timed(s, s->cov.st, KS_COV, 0.0,
          [&] { launch_candidates(md, g.ms, s->cov.st, S * q, 0, q, MK_CAND_NOBORDER, it + 1); });
    hipEventRecord(s->cov.ev[1], s->cov.st);
    s->cov.pre = it + 1;
  }
}

static void iteration_post_sweep(mk_session* s, Group& g, int it) {
  Model& md = g.md;
  const int S = g.S;
  const bool kept = it >= md.kept0;
  hipStream_t st = g.stream;
  if (s->record_samples) MK_LAUNCH(k_record, dim3((S + 63) / 64), dim3(64), 0, st, md, it);
  if (s->record_w) MK_LAUNCH(k_record_w, dim3((md.Np + 255) / 256, S), dim3(256), 0, st, md, it);
  if (kept && s->crit.on) launch_crit_accum(s, g, it - md.kept0);
  if (kept && md.n_test > 0 && !s->tiled && s->kt.on) {
    // from the phi tables (krig_tables): z, phi and A captured now, then g = W' z and the draws on a
    // side stream -- the lookahead schedule's kriging stream, else the early assembly's stream after its
    // assembly -- beside the next iteration's beta, A and decision steps (W is rewritten only by the next
    // inverse, which waits for them: kt_wait).  At 250 subsets they then overlap the next Cholesky's first
    // columns and slow its diagonal launches (a kept iteration 22.0 ms against 20.0 for a burn-in one,
    // profiles/r06/zg/), but in line costs as much: 40-step windows 11,971-11,988 vs 11,957-11,976, and
    // 8,690-8,730 vs 8,601-8,642 at 32 subsets (profiles/r06/kside/).  With neither side stream
    // (MK_EARLY_COV=0 without lookahead) they run in line.
    double* zs = s->kt.z;
    double* ph = zs + (size_t)S * md.n_pad;
    double* As = ph + S;
    MK_LAUNCH(k_kt_snap, dim3(S), dim3(256), 0, st, md, zs, ph, As);
    hipStream_t side = s->la.k ? s->la.k : (s->cov.st ? s->cov.st : st);
    if (side != st) {
      hipEventRecord(s->kt.ev[0], st);
      hipStreamWaitEvent(side, s->kt.ev[0], 0);
    }
    MK_LAUNCH(k_krig_g, dim3(S * (md.n_pad / 4)), dim3(256), 0, side, md, g.ms, (const double*)zs, s->kt.g, 0, 1);
    MK_LAUNCH(k_pred_tab_draw, dim3(S * ((md.n_test + 255) / 256)), dim3(256), 0, side, md, s->kt.tab, s->kt.g,
              md.coords, (const double*)ph, (const double*)As, it, it - md.kept0);
    if (side != st) {
      hipEventRecord(s->kt.ev[1], side);
      s->kt.pending = true;
    }
    s->prof.stats[KS_KRIG_CHEB].launches += 1;
  } else if (kept && md.n_test > 0 && !s->tiled) {
    const int per = (md.n_test + 3) / 4;
    MK_LAUNCH(k_pred_draw, dim3(S * per), dim3(256), 0, st, md, it, it - md.kept0);
  }
  if (kept && s->tiled) MK_LAUNCH(k_record_kept, dim3(S), dim3(256), 0, st, md, it - md.kept0);
  if ((it + 1) % md.batch_length == 0) MK_LAUNCH(k_adapt, dim3(S), dim3(256), 0, st, md, it / md.batch_length);
}

// Lookahead schedule (exponential model, one group).  The phi proposal of iteration t+1 is known
// once iteration t's phi step has decided (and, at a batch end, adapted), so its candidates
// R(phi'_{t+1}) are assembled and factored on la.c while the main stream runs iteration t's
// inverse, kriging and sweep -- at small shards both chains are latency-bound and overlap.  The
// candidates carry no bordered row (u_{t+1} = A_{t+1}^-1 w_t does not exist yet): after the A step
// the main stream solves z' = L'^-1 u one tile column per launch, each behind the factorisation's
// panel (k_border_step), and |z'|^2 completes the phi ratio (k_border_quad).  The chain is the
// sequential schedule's (same draws, same decisions); z' differs from the bordered factor's row
// by rounding only (tests compare both schedules and the oracle).
// Panels [0, k_hi) of iteration it's candidates (the assembly with the first piece); the rest by
// enqueue_candidates_rest.  The first piece is 3 panels: the GPU needs ~0.2 ms per panel at small
// shards, the host ~10 us per launch for the main stream's ~30.
static int la_head(mk_session* s) { return std::min(3, s->nt); }
static void enqueue_candidates(mk_session* s, Group& g, int it, hipEvent_t after, int k_hi) {
  const int S = g.S, q = s->q, nt = s->nt;
  hipStreamWaitEvent(s->la.c, after, 0);
  timed(s, s->la.c, KS_COV, 0.0,
        [&] { launch_candidates(g.md, g.ms, s->la.c, S * q, 0, q, MK_CAND_NOBORDER, it); });
  launch_cholesky(s, g, 0, q, nullptr, nullptr, s->la.c, s->la.ev.data(), 0, k_hi);
  s->la.next = it;
  s->la.enq = k_hi;
}
static void enqueue_candidates_rest(mk_session* s, Group& g) {
  if (s->la.enq < s->nt) launch_cholesky(s, g, 0, s->q, nullptr, nullptr, s->la.c, s->la.ev.data(), s->la.enq, s->nt);
  s->la.enq = s->nt;
}

static void run_iteration_la(mk_session* s, int it) {
  Group& g = s->groups[0];
  Model& md = g.md;
  const int S = g.S, q = s->q, nt = s->nt;
  hipStream_t M = g.stream;
  hipEvent_t* evP = s->la.ev.data();
  hipEvent_t ev_d = evP[nt];
  if (s->la.next != it) {   // first iteration of the session (or after a tiled replay reused the slots)
    hipEventRecord(ev_d, M);
    enqueue_candidates(s, g, it, ev_d, nt);
  }
  enqueue_candidates_rest(s, g);
  MK_LAUNCH(k_beta, dim3(S), dim3(256), 0, M, md, it);
  if (q > 1) MK_LAUNCH(k_trmv_Z, dim3(S * q * ((s->n_pad + 255) / 256)), dim3(256), 0, M, md, g.ms);
  MK_LAUNCH(k_Aphase, dim3(S), dim3(256), 0, M, md, it);
  for (int k = 0; k < nt; ++k) {   // z' = L'^-1 u, trailing the candidates' panels
    hipStreamWaitEvent(M, evP[k], 0);
    MK_LAUNCH(k_border_step, dim3(xcd_grid_h(S * q, std::max(1, nt - 1 - k))), dim3(256), 0, M, md, g.ms, k);
  }
  MK_LAUNCH(k_border_quad, dim3(S * q), dim3(256), 0, M, md);
  MK_LAUNCH(k_theta_mh, dim3((S * q + 63) / 64), dim3(64), 0, M, md, g.ms, 0, q, 0, it);
  if (s->matern) {
    // the nu step: its candidate R(phi_t, nu') needs this phi decision, so it is factored now, as in
    // the sequential schedule (bordered row: u is known), on the idle high-priority candidate stream
    // (all CUs; the main stream is CU-masked); where it is accepted its border row becomes z
    // (k_nu_border into zc).  The next phi candidates follow on the same stream (they need nu_t).
    hipEventRecord(ev_d, M);
    hipStreamWaitEvent(s->la.c, ev_d, 0);
    timed(s, s->la.c, KS_COV, 0.0, [&] { launch_candidates(md, g.ms, s->la.c, S * q, 0, q, 1, it); });
    launch_cholesky(s, g, 0, q, nullptr, nullptr, s->la.c);
    MK_LAUNCH(k_theta_mh, dim3((S * q + 63) / 64), dim3(64), 0, s->la.c, md, g.ms, 0, q, 1, it);
    MK_LAUNCH(k_nu_border, dim3(S * q * ((s->n_pad + 255) / 256)), dim3(256), 0, s->la.c, md, g.ms);
    hipEventRecord(evP[nt + 4], s->la.c);
    hipStreamWaitEvent(M, evP[nt + 4], 0);
  }
  const bool more = it + 1 < md.n_samples, batch_end = (it + 1) % md.batch_length == 0;
  if (more && !batch_end) {   // the head now; the rest after the main stream's launches
    hipEventRecord(ev_d, M);
    enqueue_candidates(s, g, it + 1, ev_d, la_head(s));
  }
  MK_LAUNCH(k_dirty_list, dim3(1), dim3(256), 0, M, md, (int)(it == md.kept0), g.d_list, g.d_count, g.d_plist,
                     g.d_pcount);
  kt_wait(s, M);   // the previous kept iteration's draws read W
  launch_inverse(s, g, true);
  const bool kept = it >= md.kept0;
  // kept iterations: the kriging refresh (X = W P^T of the changed pairs) only reads W, as the sweep
  // does, and the draws after the sweep are its only consumer -- it runs on la.k beside the sweep
  const bool side = kept && !s->tiled && !s->kt.on && md.n_test > 0 && s->la.k;
  if (side) {
    hipEventRecord(evP[nt + 2], M);
    hipStreamWaitEvent(s->la.k, evP[nt + 2], 0);
    launch_pred_refresh(s, g, s->la.k);
    hipEventRecord(evP[nt + 3], s->la.k);
  } else if (kept && !s->tiled && !s->kt.on) {
    launch_pred_refresh(s, g);
  }
  timed(s, M, KS_SWEEP, 0.0, [&] { launch_sweep(s, g, it); });
  if (side) hipStreamWaitEvent(M, evP[nt + 3], 0);
  iteration_post_sweep(s, g, it);
  if (more && batch_end) {   // the next proposal's scale is the adapted one
    hipEventRecord(ev_d, M);
    enqueue_candidates(s, g, it + 1, ev_d, nt);
  }
  enqueue_candidates_rest(s, g);
  if (!more) s->la.next = -1;
}

// One iteration of the shard.  Each group (stream) runs its own chain of launches; with the
// multi-workgroup sweep and several groups, the groups join for one whole-shard sweep on the
// session stream and fork again (the groups' Cholesky chains overlap each other's latency-bound
// diagonal steps; the sweep is one multi-workgroup launch).  Same kernels, same operands, same bits.
void mk::run_iteration(mk_session* s, int it) {
  if (s->la.on) {
    run_iteration_la(s, it);
    return;
  }
  if (use_sweep_mg(s) && s->groups.size() > 1) {
    for (auto& g : s->groups) {
      hipStreamWaitEvent(g.stream, s->swept, 0);
      iteration_pre_sweep(s, g, it);
      hipEventRecord(g.done, g.stream);
      hipStreamWaitEvent(s->stream, g.done, 0);
    }
    timed(s, s->stream, KS_SWEEP, 0.0, [&] { launch_sweep(s, s->all, it); });
    hipEventRecord(s->swept, s->stream);
    for (auto& g : s->groups) {
      hipStreamWaitEvent(g.stream, s->swept, 0);
      iteration_post_sweep(s, g, it);
    }
    return;
  }
  for (auto& g : s->groups) {
    iteration_pre_sweep(s, g, it);
    timed(s, g.stream, KS_SWEEP, 0.0, [&] { launch_sweep(s, g, it); });
    iteration_post_sweep(s, g, it);
  }
}
