// Device-resident state of one batch of subsets (one GPU's shard).
//
// HBM layout (S local subsets, q outcomes, n_pad = roundup(max n_s + 1, 128)):
//   coords  [S][2][n_pad]            SoA x | y (padding 0)
//   y, wt   [S][Np]                  Np = n_pad*q, location-major (i*q + a), padding 0
//   X       [S][p][Np]               column-major design
//   eta, w  [S][Np]
//   L       [S*q][2][n_pad^2]        accepted / candidate lower Cholesky factors of R_h
//                                    (row n_s of a candidate holds u_h: bordered solve -> z)
//   Winv    [S*q][2][nt][128^2]      inverses of the diagonal 128-tiles of each factor
//   W       [S*q][n_pad^2]           W_h = L_h^-1 of the accepted factor (lower, column-major)
//   QB      [S*q][nt][128^2]         diagonal 128-tiles of R_h^-1 = W'W (rows < n_s)
//   u, z    [S][q][n_pad]            u = (I (x) A^-1) w, z_h = W_h u_h  (so u_h'R_h^-1 u_h = |z_h|^2)
//   Z       [S][q][q][n_pad]         Z_{h,c} = W_h u_c (q > 1 only)
//   bacc,zc [S][q][n_pad]            lookahead: border-solve partial sums, z'_h = L'_h^-1 u_h
//   Y       [S*q][n_pad^2]           lookahead: inverse-level scratch (else the free factor slot)
//   PT, XK  [S*q][n_pad][n_test_pad] kriging: P^T = rho(obs, test) and X = W P^T
// All matrices of one (subset, outcome) pair are contiguous; every kernel finds
// its pair from blockIdx and the cur[] slot table, so no host round trip is
// needed between the steps of an iteration.
#pragma once
#include "../../include/mk.h"
#include "mk_common.hpp"

#define MK_QMAX 4
#define MK_CD_SPLIT 8        // k_inv_copydiag: workgroups per 128-tile (kernel and launch grid)
#define MK_QUANT_MAX 16384   // kept samples per quantile summary (k_quantiles sorts them in 128 KB of LDS)

namespace mk {

struct Model {
  int S, q, p, n_pad, Np, nt, ntri, n_theta, cov_model;
  int link;                               // MK_LINK_LOGIT | MK_LINK_PROBIT
  int o_A, o_phi, o_nu, o_w, n_mh_max;   // MH parameter offsets (spBayes order)
  int n_batch, batch_length, n_samples, kept0, n_kept;
  int n_test, n_test_pad, ntt;
  int subset_base;                        // global index of local subset 0
  int S_all;                              // subsets of the whole shard (stride of the kept-state records)
  int t_off;                              // global index of test site 0 (tiled kriging; 0 when fused)
  uint64_t seed;
  double accept_rate;
  double phi_a[MK_QMAX], phi_b[MK_QMAX], nu_a[MK_QMAX], nu_b[MK_QMAX];
  double iw_df, iw_S[MK_QMAX * MK_QMAX];
  // data
  const int* n_s;
  const double* coords;
  const double* y;
  const double* wt;
  const double* X;
  const double* coords_test;   // [2][n_test_pad]
  const double* span;          // [S] bounding-box diagonal of the subset's sites (Matern tables)
  const double* span_pt;       // [S] bound on the subset-to-test-site distances (Matern kriging tables)
  double* chtab;               // [S*q][MK_CH_TAB] Matern: Chebyshev tables of the pairs' candidates (k_matern_table)
  double* chtab_p;             // [S*q][MK_CH_TAB] Matern: tables of the current (phi, nu), kriging (k_matern_table_list)
  // state
  double* beta;      // [S][p]
  double* theta;     // [S][n_theta]: A lower-tri (log diag) | logit phi | logit nu
  double* w;         // [S][Np]
  double* eta;       // [S][Np]
  double* tune;      // [S][n_mh_max]  log proposal sd
  double* acc;       // [S][n_mh_max]  accept counts within the current batch
  double* u;         // [S][q][n_pad]
  double* z;         // [S][q][n_pad]
  double* Z;         // [S][q][q][n_pad]
  double* logdetR;   // [S][q]
  double* quad;      // [S][q]      u_h' R_h^-1 u_h at the current state
  double* A_full;    // [S][q*q]    current A (col-major)
  double* Ainv;      // [S][q*q]
  int* dirty;        // [S*q]
  // candidate scratch
  double* ld_part;   // [S*q][nt]   logdet partials of the candidate factor (per (subset, outcome) pair)
  double* quad_c;    // [S*q]
  int* info;         // [S*q]       1: the candidate's factorisation met a pivot that is not > 0 (k_chol_diag)
  // sweep scratch
  double* sw_delta;  // [S][Np]
  double* sw_dll;    // [S][Np]
  double* sw_logu;   // [S][Np]
  int* sw_acc;       // [S][Np]
  // outputs
  double* samples;     // [S][n_samples][P]   reported columns beta | K | phi | nu
  double* acc_hist;    // [S][n_batch][p+n_theta+1]  per-batch accept rates (last = mean over w)
  double* w_samples;   // [S][n_samples][Np] or null
  double* s_pred;      // [S][q][n_test_pad]  kriging variance reduction for the current (phi, nu)
  double* s_part;      // [S*q][nt][n_test_pad]
  double* PT;          // [S*q][n_pad][n_test_pad]
  double* XK;          // [S*q][n_test_pad][n_pad]  column t = W rho_t
  double* w_pred;      // [S][n_kept][q*n_test]   (tiled kriging: q*tile)
  // kept chain states for tiled kriging: [n_kept][S_all][...]
  double* kz;          // z_h = W_h u_h   (q*n_pad)
  double* kth;         // theta           (n_theta)
  double* kA;          // A               (q*q)
  // lookahead schedule (mk_api.hip): border solve of the candidate factored ahead of its iteration
  double* bacc;        // [S][q][n_pad]     right-looking partial sums of the border solve
  double* zc;          // [S][q][n_pad]     z'_h = L'_h^-1 u_h of the candidate
  int* la_nu;          // [S*q]             Matern: 1 where this iteration's nu step accepted (k_nu_border)
  int P;               // reported columns
  // candidates rejected for a set info flag since the chain started (k_theta_mh).  Last, so that no
  // other field's offset in the kernels' arguments depends on it.
  long long* notpd;    // [S*q]
};

struct MatSet {
  double* L;
  double* Winv;
  double* W;   // [S*q][ld*ld] inverse factor (persistent)
  double* Q;   // [S*q][ld*ld] full inverse (parity-test entry point only)
  double* QB;  // [S*q][nt][128*128] diagonal tiles of the inverse
  int* cur;    // [S*q]
  double* Y;   // [S*q][ld*ld] inverse-level scratch (lookahead schedule; else the free factor slot)
  int ld, nt, q;
};

// phi-interpolated kriging (mk_mcmc.hip section 11, mk_krig.hip predict_tile_cheb / krig_tables); every
// array is per (subset, outcome) pair sh = s q + h, SQ = S q of them (the fused tables: q = 1)
#define MK_CHEB_MAX 32      // Chebyshev nodes per pair at most
#define MK_CHEB_CHECKS 3    // exact check values per pair and tile: the kept range's ends and middle
#define MK_CHEB_CHECKS_MAX 5
struct ChebK {
  const double* Sn;     // [slot][SQ][T_pad]  exact s at the nodes (slots < nc[sh]) and the check points
  const double* nphi;   // [slot][SQ]         the slots' phi (as the candidate assembly computed it)
  const double* wts;    // [SQ][MK_CHEB_MAX]  barycentric weights
  const int* nc;        // [SQ]               nodes
  int nchk;             // check slots per pair (after the nodes)
  long T_pad;
};

// What turns a kriging draw w(s) into the predictive probability p(y = 1) (pred_prob): beta of the
// draw's kept state and the test row's covariates.  Draw (subset s, window row r, column c) reads
// beta at samples + s*subset_stride + r*row_stride and covariate j at x[x_off + c + j*ldx].
struct ProbSrc {
  const double* samples;   // subset 0's recorded row of the window's first kept state (beta = its first p columns)
  long subset_stride;      // n_samples * P
  long row_stride;         // P
  const double* x;         // x_test on the device, (q n_test_all) x p column-major
  long ldx;                // q * n_test_all
  long x_off;              // the first column's row of x (a tile's t0 * q; 0 when fused)
  int p, link;
};

// The exceedance thresholds of the posterior maps (mk_maps.hip), passed to k_map_cols by value: u[0 .. J)
// as given, the slots past J at +inf (no probability exceeds them), so the kernel counts all
// MK_MAP_MAXT in registers whatever J is.
struct MapThr {
  double u[MK_MAP_MAXT];
  int J;
};

// Model-assessment scratch (mk_criteria.hip; include/mk.h "model assessment").  Per observation
// (subset s, row i of its Np) six running values over the window's states, plane a of subset s at
// acc + (s * MK_CRIT_ACC + a) * Np: 0 the Welford mean of the log-likelihood terms, 1 their M2, 2 the
// running maximum and 3 the scaled sum of the streaming log-sum-exp, 4 a flag (1 once a term was not
// finite), 5 the sum of w.  part: the workgroups' sums of the terms, one per (subset, state, block of
// 256 observations).  sbeta: the sum of beta.
#define MK_CRIT_ACC 6
struct Crit {
  double* acc;     // [S][MK_CRIT_ACC][Np]
  double* part;    // [S][n_cap][nb]
  double* sbeta;   // [S][p]
  int nb;          // ceil(Np / 256)
  int n_cap;       // states the partials have room for
};

__device__ inline long mat_elems(const MatSet& m) { return (long)m.ld * m.ld; }
__device__ inline double* mat_slot(const MatSet& m, int sh, int slot) {
  return m.L + ((long)sh * 2 + slot) * mat_elems(m);
}
__device__ inline double* winv_slot(const MatSet& m, int sh, int slot, int k) {
  return m.Winv + (((long)sh * 2 + slot) * m.nt + k) * (MK_NB * MK_NB);
}
__device__ inline Key subset_key(const Model& md, int s) { return make_key(md.seed, (uint32_t)(md.subset_base + s)); }

// XCD-aware block -> (entry, tile) map.  Blocks are dealt round-robin over the 8 XCDs
// (block b runs on XCD b % 8); the S*T work items are cut into 8 contiguous chunks and XCD x
// takes chunk x in order, so the tiles of one entry (subset) run on one XCD and share its L2
// (its shared panel is fetched once), and every XCD gets an equal share however few entries
// are active (a short list of changed subsets no longer leaves XCDs idle).  S is the number of
// ACTIVE entries; the grid (xcd_grid of the maximum) covers any S up to that maximum.  Speed
// only; any placement is correct.
__host__ __device__ inline bool xcd_map_at(int b, int S, int T, int* s, int* t) {
  const int W = S * T, C = (W + 7) >> 3;
  const int x = b & 7, j = b >> 3;
  if (j >= C) return false;
  const int w = x * C + j;
  if (w >= W) return false;
  *s = w / T;
  *t = w % T;
  return true;
}
__device__ inline bool xcd_map(int S, int T, int* s, int* t) { return xcd_map_at(blockIdx.x, S, T, s, t); }
// The same map with every entry's last item (t = T - 1, T >= 2) dealt after all the others: XCD x
// takes its chunk of the S (T - 1) leading items first, then its chunk of the S last items.  Fits
// the same grid: ceil(S (T-1) / 8) + ceil(S / 8) <= ceil(S / 8) T.
__device__ inline bool xcd_map_tail(int S, int T, int* s, int* t) {
  const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int Wr = S * (T - 1), Cr = (Wr + 7) >> 3, Cs = (S + 7) >> 3;
  if (j < Cr) {
    const int w = x * Cr + j;
    if (w >= Wr) return false;
    *s = w / (T - 1);
    *t = w % (T - 1);
    return true;
  }
  const int e = x * Cs + (j - Cr);
  if (j - Cr >= Cs || e >= S) return false;
  *s = e;
  *t = T - 1;
  return true;
}
// Two tail classes (T >= 3): every entry's items t < T - 2 first, then the items T - 2 of all entries,
// then the items T - 1.  Fits the same grid: ceil(S (T-2) / 8) + 2 ceil(S / 8) <= ceil(S / 8) T.
__device__ inline bool xcd_map_tail2(int S, int T, int* s, int* t) {
  const int x = blockIdx.x & 7;
  int j = blockIdx.x >> 3;
  const int Wr = S * (T - 2), Cr = (Wr + 7) >> 3, Cs = (S + 7) >> 3;
  if (j < Cr) {
    const int w = x * Cr + j;
    if (w >= Wr) return false;
    *s = w / (T - 2);
    *t = w % (T - 2);
    return true;
  }
  j -= Cr;
  if (j >= 2 * Cs) return false;
  const int cls = j >= Cs ? 1 : 0;
  const int e = x * Cs + (j - cls * Cs);
  if (e >= S) return false;
  *s = e;
  *t = T - 2 + cls;
  return true;
}
__host__ inline int xcd_grid(int S, int T) { return 8 * ((S + 7) / 8) * T; }

// ---------------------------------------------------------------- job map of the inverse levels
// A k_inv_level launch (level sz, one phase) is the one GEMM launch whose jobs differ in length: tile
// (i, j) of the pair T = [T0, T0+sz), B = [B0, B0+sz), B0 = T0 + sz, runs a K range of B0 - j tiles in
// phase 0 and of i - B0 + 1 tiles in phase 1, 1 to sz of them.  xcd_map's cut by item count then gives the
// XCDs unequal work, and its item order ends every XCD's share on the longest jobs of its last matrix.
// inv_map_job cuts by work and starts the longest jobs first.
//
// Items.  Tiles with i >= nt do not exist; only the last pair of a matrix can lose rows to that, so a
// matrix is F = nt / (2 sz) whole pairs and one of rl < sz rows (rl = 0: none).  Class k holds the
// tiles whose K range is k tiles: in phase 0 column j = B0 - k of every pair (R = F sz + rl tiles, pair
// by pair, rows ascending), in phase 1 row i = B0 + k - 1 of the pairs that have it (sz tiles each, pair
// by pair, columns ascending) -- so the tiles that share a triangular operand are consecutive.  An
// item is one workgroup's job: a tile, or one of its SUB sub-tiles (adjacent items, each the tile's K
// range on 1 / SUB of its elements; work is counted in these units, k per item of class k).  The
// item sequence of a launch is entry-major and, within a matrix, class-major from k = sz down; all
// matrices of a session have the same nt, hence the same sequence, of SUB sz R items.
//
// Cut.  XCD x (blocks b with b % 8 = x) takes the contiguous run of items whose work midpoint lies in
// the x-th eighth of the launch's work: with c the work before an item of class k and Wt the total,
// x Wt <= 8 c + 4 k < (x + 1) Wt.  Both ends of a run are within sz / 2 of the ideal cut, so an XCD's
// work is within one longest job of the mean; a matrix lies on one XCD, or on two at a cut (the shared
// operands' L2 reuse, above).  The midpoints of one matrix lie inside its own stretch of the work
// line, so a run of width <= ceil(S / 8) matrices touches at most ceil(S / 8) + 1 of them:
// inv_map_grid, which covers any listed count up to max_entries.
//
// Order.  Within its run an XCD takes class sz of all its matrices first, then sz - 1, ...: within a
// class by entry, then in the matrix's order, so the sub-tiles of a tile stay adjacent (a cut may fall
// between two of them).  The blocks past an XCD's run are the last of its blocks, as with xcd_map.
//
// Cost per block: two cuts and one class search, O(sz) integer steps and five divisions; every
// quantity is below 8 (S + 1) Wm, which inv_map_fits checks against 2^31 on the host.
struct InvShape {
  int sz, phase, sub, F, rl;
  // items of class k, items and work of a matrix
  __host__ __device__ int n(int k) const { return sub * (phase == 0 ? F * sz + rl : sz * (F + (rl >= k ? 1 : 0))); }
  __host__ __device__ int items() const { return sub * sz * (F * sz + rl); }
  __host__ __device__ int work() const {
    const int full = sz * (sz + 1) / 2;
    return sub * (phase == 0 ? (F * sz + rl) * full : sz * (F * full + rl * (rl + 1) / 2));
  }
};
__host__ __device__ inline InvShape inv_shape(int nt, int sz, int phase, int sub) {
  InvShape h;
  h.sz = sz;
  h.phase = phase;
  h.sub = sub;
  h.F = nt / (2 * sz);
  const int rem = nt - 2 * sz * h.F;
  h.rl = rem > sz ? rem - sz : 0;
  return h;
}
struct InvPos { int e, k, m; };   // the m-th item of class k of entry e
// The first item whose work midpoint is at or past x eighths of the work of S matrices.
__host__ __device__ inline InvPos inv_map_cut(const InvShape& h, int S, int x) {
  // 8 c + 4 k >= x S Wm: entry x S / 8, and within it the threshold tl on the matrix's own work line
  InvPos q;
  q.e = (x * S) >> 3;
  const int tl = ((x * S) & 7) * h.work();
  int A = 0;   // work before class k
  for (int k = h.sz; k >= 1; --k) {
    const int nk = h.n(k), num = tl - 8 * A - 4 * k;
    // item m of the class has midpoint (8 (A + m k) + 4 k) / 8: the first with 8 k m >= num
    if (nk > 0 && num <= 8 * k * (nk - 1)) {
      q.k = k;
      q.m = num <= 0 ? 0 : (num + 8 * k - 1) / (8 * k);
      return q;
    }
    A += nk * k;
  }
  q.e += 1;   // past the matrix's last midpoint: the next matrix's first item
  q.k = h.sz;
  q.m = 0;
  return q;
}
// Items of class k that a matrix has before position q (q.k, q.m).
__host__ __device__ inline int inv_before(const InvShape& h, const InvPos& q, int k) {
  return k > q.k ? h.n(k) : (k == q.k ? q.m : 0);
}
// Block b of a level's launch over S listed entries -> entry e, pair p, tile (i, j), sub-tile st < SUB.
__host__ __device__ inline bool inv_map_job(int S, int nt, int sz, int phase, int SUB, int b, int* e, int* p, int* i,
                                            int* j, int* st) {
  if (S <= 0) return false;
  const InvShape h = inv_shape(nt, sz, phase, SUB);
  const int x = b & 7;
  int q = b >> 3;   // the item's rank in the XCD's run
  const InvPos a = inv_map_cut(h, S, x), z = inv_map_cut(h, S, x + 1);
  for (int k = sz; k >= 1; --k) {
    const int nk = h.n(k), ba = inv_before(h, a, k);
    const int cnt = (z.e - a.e) * nk + inv_before(h, z, k) - ba;
    if (q >= cnt) {
      q -= cnt;
      continue;
    }
    const int g = a.e * nk + ba + q;   // ordinal among the launch's class-k items
    *e = g / nk;
    *st = g % SUB;
    const int m = g % nk / SUB;        // the tile among the matrix's class-k tiles
    if (phase == 0) {
      const bool last = m >= h.F * sz;   // the short pair's rl rows
      *p = last ? h.F : m / sz;
      *i = 2 * *p * sz + sz + (last ? m - h.F * sz : m % sz);
      *j = 2 * *p * sz + sz - k;
    } else {
      *p = m / sz;
      *i = 2 * *p * sz + sz + k - 1;
      *j = 2 * *p * sz + m % sz;
    }
    return true;
  }
  return false;
}
// The same answer from xcd_map (MK_INV_MAP=0): the matrices' npairs sz^2 tile slots per entry in equal
// counts, clipped tiles (i >= nt) included and dropped here.
__host__ __device__ inline bool inv_xcd_job(int S, int nt, int sz, int phase, int SUB, int b, int* e, int* p, int* i,
                                            int* j, int* st) {
  const int npairs = (nt + 2 * sz - 1) / (2 * sz);
  int t;
  if (!xcd_map_at(b, S, npairs * sz * sz * SUB, e, &t)) return false;
  *st = t % SUB;
  t /= SUB;
  *p = t / (sz * sz);
  t %= sz * sz;
  // consecutive work items share the operand whose K range is the same for all of them:
  // phase 0 a column j (W_TT(j:B0, j)), phase 1 a row i (W_BB(i, B0:i+1))
  *i = 2 * *p * sz + sz + (phase == 0 ? t % sz : t / sz);
  *j = 2 * *p * sz + (phase == 0 ? t / sz : t % sz);
  return *i < nt;
}
__host__ inline bool inv_map_fits(int max_entries, int nt, int sz) {
  const long w = std::max(inv_shape(nt, sz, 0, 16).work(), inv_shape(nt, sz, 1, 16).work());
  return 8L * ((long)max_entries + 1) * w < (1L << 31);
}
__host__ inline int inv_map_grid(int max_entries, int nt, int sz, int SUB) {
  return 8 * ((max_entries + 7) / 8 + 1) * inv_shape(nt, sz, 0, SUB).items();
}


}  // namespace mk
