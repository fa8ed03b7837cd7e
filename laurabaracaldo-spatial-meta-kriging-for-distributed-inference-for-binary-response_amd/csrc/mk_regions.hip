// Areal prediction on the device (include/mk.h "areal prediction": the prevalence of a region, the weighted
// mean of p(y = 1) over its test sites, from kriging draws that are joint across the region's sites): the two
// kernels, a session's plan and buffers, the hooks of the exact tiled replay, those of the phi-interpolated one
// (the opt-in route MK_REGIONS_INTERP, below) and the entry points.  Nothing here runs, and nothing is
// allocated, unless regions are attached.
//
// k_region_cov: one workgroup per (dirty pair, region) right after the replay refreshed X = W P^T.  The
// region's columns of X are k-contiguous in HBM (XK[t * n_pad + row]), so S = R(g,g) - X_g' X_g is
// gemm_tile<128, 128, A k-contiguous, B k-contiguous, NEG, SAME, MASK>: one LDS image serves both fragments,
// the K range is cut at n_s by the mask (row n_s of X carries the bordered row of W), and the 128-column
// window is moved left where it would pass the end of the buffer (w0 = min(t_1, n_test_pad - 128); the
// region then sits at rows and columns d = t_1 - w0 .. d + m of the tile).  Columns of the window outside the
// region only reach accumulator elements nobody reads.  gemm_syrk_128 is not used: it takes an m-contiguous
// panel (section 4.4 has what the launch costs).  The lower triangle then goes to LDS
// (column stride MK_TLD) where the workgroup factors it right-looking, column by column, with the pivot rule
// of the header; the factor is written packed, m x m column-major.
//
// k_region_draw: one workgroup per (subset, region) per kept state.  The means are k_pred_draw's dots (a wave
// per site, the same loads and summation order), the normals its Philox words; thread (i, h) then adds row i
// of L_h times zeta_h, thread (i, a) mixes with A and applies pred_prob, and thread a sums the weighted
// probabilities in site order.
//
// The interpolated route (S_h depends on phi_h alone): k_region_cov_node is k_region_cov's first half, "form S
// in LDS", over the pairs of one node or check slot of cheb_eval, storing the lower triangle; k_region_check is
// k_cheb_check over those triangles; k_region_interp_factor, one workgroup per (pair, phi run, region) of a
// chunk of kept states, interpolates the triangle into LDS and runs k_region_cov's second half, "factor the tile
// in LDS"; k_region_draw<true> then draws a whole chunk, a workgroup per (state, subset, region), reading the
// means k_pred_cheb_draw<Q, true> left and each state's factor through a slot table.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include "mk_session.hpp"
#include "mk_gemm.hpp"

static_assert(mk::REGION_MAXM == MK_REGION_MAXM && MK_REGION_MAXM == MK_NB, "a region is one 128-tile");
static_assert(mk::REGION_MAXT == MK_MAP_MAXT, "mk_regionspec.hpp counts the maps' thresholds");

namespace mk {

struct RegionK {
  const int* offsets;    // [G + 1]
  const long* foff;      // [G + 1]
  const double* omega;   // [n_test]
  double* L;             // [S q][fsz]
  int* flag;             // [S q][G]
  int G;
  long fsz;
};

constexpr int MK_REGION_DRAW_T = 1024;   // threads of k_region_draw's workgroup
constexpr int REGION_LDS_BYTES = MK_NB * MK_TLD * 8;   // the factor's tile; the GEMM's two stages fit inside
static_assert(REGION_LDS_BYTES >= MK_GD_LDS_BYTES, "the GEMM stages share the tile's LDS");

// The interpolated route: cheb_eval's nodes (slots 0 .. nc-1 per pair, then the check slots) with the node
// buffer of S.
struct RegionNodesK {
  const double* Sn;     // [slot][S q][fsz]: lower triangles, region g's m x m column-major at foff[g]
  const double* nphi;   // [slot][S q]
  const double* wts;    // [S q][MK_CHEB_MAX]
  const int* nc;        // [S q]
  int SQ, nchk;
  long fsz;
};

// What k_region_draw<true> reads in place of X, z and the exact route's factors.
struct RegionDrawI {
  const double* means;  // [S][n][q n_test]
  const int* slot;      // [n][S q]
  const double* kA;     // [kept][S][q q]
  const double* L;      // [S q][B][fsz]
  const int* flag;      // [S q][B][G]
  int B, j0, k_lo;
};

// Form S in LDS: T = lower(R(g,g) - X_g' X_g) of pair sh and region g at column stride MK_TLD, rows and
// columns 0 .. m-1.  md: the tile's view with theta of the state (or node slot) whose X is in md.XK.  Ends
// without a barrier.
__device__ inline void region_form_s(const Model& md, const RegionK& rk, int sh, int g, double* lds) {
  const int s = sh / md.q, h = sh % md.q;
  const int ns = md.n_s[s];
  const int t1 = rk.offsets[g], m = rk.offsets[g + 1] - t1;
  const int w0 = min(t1, md.n_test_pad - MK_NB), d = t1 - w0;
  const double* Xg = md.XK + ((long)sh * md.n_test_pad + w0) * md.n_pad;
  Acc acc;
  acc_zero(acc);
  const int K = (ns + GB_K - 1) / GB_K * GB_K;   // <= n_pad; rows >= n_s read as zero (MASK)
  gemm_tile<128, 128, false, false, true, false, true, SKIP_NONE, true>(Xg, md.n_pad, Xg, md.n_pad, K, ns, acc, lds);
  // acc = -X_w' X_w; the GEMM ended with a barrier, so its stages are free: T = lower(R(g,g) + acc)
  const double* th = md.theta + (long)s * md.n_theta;
  const double phi = logit_inv(th[md.ntri + h], md.phi_a[h], md.phi_b[h]);
  const double nu = (md.cov_model == MK_COV_MATERN) ? logit_inv(th[md.ntri + md.q + h], md.nu_a[h], md.nu_b[h]) : 0.0;
  CorrFn rho;
  rho.init(phi, nu, md.cov_model);
  const double* tx = md.coords_test + t1;
  const double* ty = md.coords_test + md.n_test_pad + t1;
  double* T = lds;
#pragma unroll
  for (int bm = 0; bm < 4; ++bm)
#pragma unroll
    for (int bn = 0; bn < 4; ++bn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = acc_row(bm) - d, j = acc_col(bn, r) - d;
        if (j >= 0 && j <= i && i < m) {
          const double rij = (i == j) ? 1.0 : rho(dist2d(tx[i], ty[i], tx[j], ty[j]));
          T[i + j * MK_TLD] = rij + acc.v[bm][bn][r];
        }
      }
}

// Factor the tile in LDS (T: the lower triangle of an m x m matrix at column stride ld, written by this
// workgroup of 256 threads with no barrier since) and write the factor packed, m x m column-major, to L and
// its flag to *flag.  dg [MK_NB] and sflag are the workgroup's.
// Right-looking, column by column: the pivot stays where it is (the diagonal of L goes to dg), so a column
// costs two barriers; in the trailing update a wave owns a column and its lanes walk the rows.
__device__ inline void region_factor(double* T, int ld, int m, double* dg, int* sflag, double* __restrict__ L,
                                     int* __restrict__ flag) {
  if (threadIdx.x == 0) *sflag = 0;
  __syncthreads();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int j = 0; j < m; ++j) {
    const double piv = T[j + j * ld];
    const bool ok = piv > MK_REGION_PIVOT_TOL;   // NaN is not
    const double dj = ok ? sqrt(piv) : 0.0;
    if (tid == 0) {
      dg[j] = dj;
      if (!ok) *sflag = 1;
    }
    for (int i = j + 1 + tid; i < m; i += 256) T[i + j * ld] = ok ? T[i + j * ld] / dj : 0.0;
    __syncthreads();
    if (ok)   // the same for every thread
      for (int c = j + 1 + wave; c < m; c += 4) {
        const double lc = T[c + j * ld];
        for (int i = c + lane; i < m; i += 64) T[i + c * ld] -= T[i + j * ld] * lc;
      }
    __syncthreads();
  }
  for (int x = tid; x < m * m; x += 256) {
    const int i = x % m, j = x / m;
    L[x] = i > j ? T[i + j * ld] : (i == j ? dg[j] : 0.0);
  }
  if (tid == 0) *flag = *sflag;
}

// Grid max_entries * G, dynamic LDS REGION_LDS_BYTES.  md: the tile's view with theta of the state replayed.
__global__ __launch_bounds__(256) void k_region_cov(Model md, RegionK rk, const int* __restrict__ list,
                                                    const int* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int sflag;
  __shared__ double dg[MK_NB];
  const int e = blockIdx.x / rk.G, g = blockIdx.x % rk.G;
  if (e >= *count) return;
  const int sh = list[e];
  region_form_s(md, rk, sh, g, lds);
  region_factor(lds, MK_TLD, rk.offsets[g + 1] - rk.offsets[g], dg, &sflag, rk.L + (long)sh * rk.fsz + rk.foff[g],
                rk.flag + (long)sh * rk.G + g);
}

// The interpolated route's node covariances: k_region_cov's grid, list and LDS over the pairs of one node or
// check slot, storing the lower triangle of S (Sn: that slot's [S q][fsz]) instead of factoring it.
__global__ __launch_bounds__(256) void k_region_cov_node(Model md, RegionK rk, const int* __restrict__ list,
                                                         const int* __restrict__ count, double* __restrict__ Sn) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int e = blockIdx.x / rk.G, g = blockIdx.x % rk.G;
  if (e >= *count) return;
  const int sh = list[e];
  region_form_s(md, rk, sh, g, lds);
  __syncthreads();
  const int m = rk.offsets[g + 1] - rk.offsets[g];
  double* out = Sn + (long)sh * rk.fsz + rk.foff[g];
  for (int x = threadIdx.x; x < m * m; x += 256) {
    const int i = x % m, j = x / m;
    if (i >= j) out[x] = lds[i + j * MK_TLD];
  }
}

// The barycentric coefficients of pair sh at phi (the shape of cheb_s): coef[i] = wts[i] / (phi - phi_i),
// *den their sum in node order, *hit the first node with phi_i == phi (-1: none; its value is then the
// interpolant's).  All threads of the workgroup call it; it begins and ends with a barrier.
__device__ inline void region_bary_coef(const RegionNodesK& nk, int sh, double phi, double* coef, double* den, int* hit) {
  const int nc = nk.nc[sh];
  __syncthreads();
  if ((int)threadIdx.x < nc) coef[threadIdx.x] = nk.wts[(long)sh * MK_CHEB_MAX + threadIdx.x] / (phi - nk.nphi[(long)threadIdx.x * nk.SQ + sh]);
  __syncthreads();
  if (threadIdx.x == 0) {
    double d = 0.0;
    int ht = -1;
    for (int i = 0; i < nc; ++i) {
      if (ht < 0 && phi - nk.nphi[(long)i * nk.SQ + sh] == 0.0) ht = i;
      d += coef[i];
    }
    *den = d;
    *hit = ht;
  }
  __syncthreads();
}

// Entry x of pair sh's packed S from its nodes, with region_bary_coef's coefficients.
__device__ inline double region_bary(const RegionNodesK& nk, int sh, long x, int nc, const double* coef, double den, int hit) {
  const double* f = nk.Sn + (long)sh * nk.fsz + x;
  const long stride = (long)nk.SQ * nk.fsz;
  if (hit >= 0) return f[hit * stride];
  double num = 0.0;
  for (int i = 0; i < nc; ++i) num += coef[i] * f[i * stride];
  return num / den;
}

// The interpolant of S against the exact S at the check slots nc .. nc+nchk-1: the largest |difference| over
// the packed entries and the pairs (grid: S q blocks of ceil(fsz / 256)) into *err (bit pattern of a
// non-negative double; a NaN counts as +inf) -- k_cheb_check over the node buffer of S.
__global__ __launch_bounds__(256) void k_region_check(RegionNodesK nk, unsigned long long* err) {
  __shared__ double coef[MK_CHEB_MAX], red[4], den;
  __shared__ int hit;
  const int nb = (int)((nk.fsz + 255) / 256);
  const int sh = blockIdx.x / nb;
  const long x = (long)(blockIdx.x % nb) * 256 + threadIdx.x;
  const int nc = nk.nc[sh];
  double e = 0.0;
  for (int k = 0; k < nk.nchk; ++k) {
    const int slot = nc + k;
    const double phi = nk.nphi[(long)slot * nk.SQ + sh];
    region_bary_coef(nk, sh, phi, coef, &den, &hit);
    if (x < nk.fsz) {
      const double ex = nk.Sn[((long)slot * nk.SQ + sh) * nk.fsz + x];
      const double d = fabs(region_bary(nk, sh, x, nc, coef, den, hit) - ex);
      if (!(d <= e)) e = (d != d) ? INFINITY : d;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) e = fmax(e, __shfl_xor(e, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    atomicMax(err, (unsigned long long)__double_as_longlong(m));
  }
}

// Interpolate and factor: one workgroup per job (pair, phi of one of its runs, region, factor slot).  The
// region's lower triangle at that phi goes to LDS at column stride ld (dynamic LDS maxm * ld doubles, ld >=
// maxm: small regions' workgroups share a CU), then region_factor writes L and the flag to the slot.
__global__ __launch_bounds__(256) void k_region_interp_factor(RegionK rk, RegionNodesK nk, const RegionJob* __restrict__ jobs,
                                                              int ld, int B, double* __restrict__ Lc,
                                                              int* __restrict__ flagc) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int sflag, hit;
  __shared__ double dg[MK_NB], coef[MK_CHEB_MAX], den;
  const RegionJob jb = jobs[blockIdx.x];
  const int sh = jb.pair, g = jb.region;
  const int m = rk.offsets[g + 1] - rk.offsets[g];
  const int nc = nk.nc[sh];
  region_bary_coef(nk, sh, jb.phi, coef, &den, &hit);
  const long f0 = rk.foff[g];
  for (int x = threadIdx.x; x < m * m; x += 256) {
    const int i = x % m, j = x / m;
    if (i >= j) lds[i + j * ld] = region_bary(nk, sh, f0 + x, nc, coef, den, hit);
  }
  const long at = (long)sh * B + jb.slot;
  region_factor(lds, ld, m, dg, &sflag, Lc + at * rk.fsz + f0, flagc + at * rk.G + g);
}

// INTERP false: grid S * G, MK_REGION_DRAW_T threads (16 waves: the dots are latency-bound, one wave per site
// at a time).  md: the tile's view with z and A of the state replayed (iteration iter, window row j of n);
// ps: prob_src of the tile.  draws: [S][n][C3]; singular: [S][C3].
// INTERP true (the interpolated route): grid nb * S * G for the nb states ri.j0 .. of a chunk, 256 threads;
// the means are read from ri.means, L and the flag through ri.slot, A from the state's record of ri.kA; the
// workgroups of one launch count their flagged factors atomically.  iter and j are unused.
template <bool INTERP>
__global__ __launch_bounds__(INTERP ? 256 : MK_REGION_DRAW_T) void k_region_draw(Model md, RegionK rk, ProbSrc ps, int iter,
                                                                                 int j, int n, double* __restrict__ draws,
                                                                                 int* __restrict__ singular, RegionDrawI ri) {
  constexpr int NT = INTERP ? 256 : MK_REGION_DRAW_T;
  __shared__ double v[MK_QMAX][MK_NB], zeta[MK_QMAX][MK_NB], pw[MK_QMAX][MK_NB];
  const int bx = INTERP ? blockIdx.x % (md.S * rk.G) : blockIdx.x;
  if (INTERP) {
    j = ri.j0 + blockIdx.x / (md.S * rk.G);
    iter = md.kept0 + ri.k_lo + j;
  }
  const int s = bx / rk.G, g = bx % rk.G;
  const int q = md.q, ns = md.n_s[s];
  const int t1 = rk.offsets[g], m = rk.offsets[g + 1] - t1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (INTERP) {
    const double* mu = ri.means + ((long)s * n + j) * q * md.n_test + (long)t1 * q;
    for (int x = tid; x < m * q; x += NT) v[x % q][x / q] = mu[x];
  } else {
    // the means: k_pred_draw's dot, a wave per (site, outcome)
    for (int i = wave; i < m; i += NT / 64)
      for (int h = 0; h < q; ++h) {
        const long sh = (long)s * q + h;
        const double* xk = md.XK + (sh * md.n_test_pad + t1 + i) * md.n_pad;
        const double* zh = md.z + sh * md.n_pad;
        const int np2 = md.n_pad >> 1;
        double a[4] = {0.0, 0.0, 0.0, 0.0};
        for (int base = 0; base < ns; base += 512) {
          d2 xv[4], zv[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int pr = min((base >> 1) + u * 64 + lane, np2 - 1);
            xv[u] = *reinterpret_cast<const d2*>(xk + 2 * pr);
            zv[u] = *reinterpret_cast<const d2*>(zh + 2 * pr);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int r = base + 2 * (u * 64 + lane);
            a[u] += (r < ns) ? xv[u].x * zv[u].x : 0.0;
            a[u] += (r + 1 < ns) ? xv[u].y * zv[u].y : 0.0;
          }
        }
        double acc = (a[0] + a[1]) + (a[2] + a[3]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) v[h][i] = acc;
      }
  }
  const Key key = subset_key(md, s);
  for (int x = tid; x < m * q; x += NT) {
    const int i = x / q, h = x % q;
    zeta[h][i] = predict_normal(key, (uint32_t)((md.t_off + t1 + i) * q + h), (uint32_t)iter);
  }
  __syncthreads();
  // v_{i,h} = mean_{i,h} + sum_{c <= i} L_h[i, c] zeta_{c,h}, c ascending (element (i, h) only reads its own mean)
  for (int x = tid; x < m * q; x += NT) {
    const int i = x % m, h = x / m;
    const long sh = (long)s * q + h;
    const double* L = INTERP ? ri.L + (sh * ri.B + ri.slot[(long)j * md.S * q + sh]) * rk.fsz + rk.foff[g]
                             : rk.L + sh * rk.fsz + rk.foff[g];
    double acc = 0.0;
    for (int c = 0; c <= i; ++c) acc += L[i + (long)c * m] * zeta[h][c];
    v[h][i] = v[h][i] + acc;
  }
  __syncthreads();
  const double* A = INTERP ? ri.kA + ((long)(ri.k_lo + j) * md.S + s) * q * q : md.A_full + (long)s * q * q;
  const double* beta = ps.samples + (long)s * ps.subset_stride + (long)j * ps.row_stride;
  for (int x = tid; x < m * q; x += NT) {
    const int i = x / q, a = x % q;
    double o = 0.0;
    for (int h = 0; h < q; ++h) o += v[h][i] * A[a + h * q];
    const long c = (long)(t1 + i) * q + a;
    pw[a][i] = pred_prob(ps.x + ps.x_off + c, ps.ldx, beta, ps.p, o, ps.link);
  }
  __syncthreads();
  if (tid < q) {
    const int a = tid, C3 = rk.G * q;
    double r = 0.0;
    for (int i = 0; i < m; ++i) r += rk.omega[t1 + i] * pw[a][i];
    draws[((long)s * n + j) * C3 + g * q + a] = r;
    const long sh = (long)s * q + a;
    if (INTERP) {
      if (ri.flag[(sh * ri.B + ri.slot[(long)j * md.S * q + sh]) * rk.G + g]) atomicAdd(&singular[(long)s * C3 + g * q + a], 1);
    } else {
      if (rk.flag[sh * rk.G + g]) singular[(long)s * C3 + g * q + a] += 1;
    }
  }
}

}  // namespace mk

using namespace mk;

// ------------------------------------------------------------------ host side
namespace {
const SinkWords kWords = {"null session/regions", "no areal prediction asked for (mk_session_set_regions)",
                          "areal prediction needs all n.samples iterations", "areal prediction",
                          "the regions were attached"};

RegionK region_k(const Regions& r) {
  RegionK k;
  k.offsets = r.offsets;
  k.foff = r.foff;
  k.omega = r.omega;
  k.L = r.L;
  k.flag = r.flag;
  k.G = r.plan.G;
  k.fsz = r.plan.foff.back();
  return k;
}

void drop_pending(Regions& r) {
  for (auto& e : r.pending) {
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  r.pending.clear();
}

// The events of the replay loop's launches into KS_REGIONS and the per-part times.  The stream is idle.
int price_pending(mk_session* s) {
  Regions& r = s->regions;
  Stat& k = s->prof.stats[KS_REGIONS];
  for (auto& e : r.pending) {
    float ms = 0.f;
    const hipError_t rc = hipEventElapsedTime(&ms, e.a, e.b);
    if (rc != hipSuccess) {
      drop_pending(r);
      return set_err(MK_E_HIP, std::string("areal prediction: event time -> ") + hipGetErrorString(rc));
    }
    r.ms[e.part] += ms;
    k.ms += ms;
    k.launches += e.launches;
  }
  drop_pending(r);
  return 0;
}
}  // namespace

void mk::regions_detach(mk_session* s) {
  Regions& r = s->regions;
  drop_pending(r);
  for (void* b : {(void*)r.offsets, (void*)r.foff, (void*)r.omega, (void*)r.L, (void*)r.flag, (void*)r.draws,
                  (void*)r.singular, (void*)r.grids, (void*)r.planes})
    s->release(b);
  s->regions = Regions{};
}

int mk::regions_begin(mk_session* s, int t0, int Tc, int n_kept) {
  Regions& r = s->regions;
  if (t0 != 0 || Tc != s->n_test_all)
    return set_err(MK_E_ARG, "areal prediction: the regions live in one tile, and this replay's tile does not hold every test site");
  if (!s->d_xt) return set_err(MK_E_ARG, "areal prediction needs x_test");
  if (n_kept > s->md.n_kept) return set_err(MK_E_ARG, "areal prediction: the kept window is longer than the kept states");
  drop_pending(r);   // of a replay that ended in an error
  HIPCHK(hipMemsetAsync(r.singular, 0, (size_t)s->S * r.C3 * sizeof(int), s->stream));
  return 0;
}

int mk::regions_state(mk_session* s, Group& g, const Model& mt, int iter, int j, int n_kept) {
  Regions& r = s->regions;
  hipStream_t st = s->stream;
  const RegionK rk = region_k(r);
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) {
      for (auto& x : ev)
        if (x) (void)hipEventDestroy(x);
      return set_err(MK_E_HIP, "areal prediction: hipEventCreate failed");
    }
  r.pending.push_back({0, ev[0], ev[1], 1});   // owned by the list from here on (drop_pending)
  r.pending.push_back({1, ev[2], ev[3], 1});
  HIPCHK(hipEventRecord(ev[0], st));
  MK_LAUNCH(k_region_cov, dim3((unsigned)(s->S * s->q * rk.G)), dim3(256), REGION_LDS_BYTES, st, mt, rk,
            (const int*)g.d_plist, (const int*)g.d_pcount);
  HIPCHK(hipEventRecord(ev[1], st));
  HIPCHK(hipEventRecord(ev[2], st));
  MK_LAUNCH(k_region_draw<false>, dim3((unsigned)(s->S * rk.G)), dim3(MK_REGION_DRAW_T), 0, st, mt, rk, prob_src(s, 0), iter, j,
            n_kept, r.draws, r.singular, RegionDrawI{});
  HIPCHK(hipEventRecord(ev[3], st));
  HIPCHK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ the interpolated route
namespace {
// The event pair of one launch of timing part `part`, owned by the pending list (drop_pending).
int pending_pair(Regions& r, int part, hipEvent_t* a, hipEvent_t* b) {
  *a = *b = nullptr;
  if (hipEventCreate(a) != hipSuccess || hipEventCreate(b) != hipSuccess) {
    if (*a) (void)hipEventDestroy(*a);
    return set_err(MK_E_HIP, "areal prediction: hipEventCreate failed");
  }
  r.pending.push_back({part, *a, *b, 1});
  return 0;
}

RegionNodesK region_nodes_k(const mk_session* s, const RegionInterp& ri, const ChebK& ck) {
  RegionNodesK nk;
  nk.Sn = ri.Sn;
  nk.nphi = ck.nphi;
  nk.wts = ck.wts;
  nk.nc = ck.nc;
  nk.SQ = s->S * s->q;
  nk.nchk = ck.nchk;
  nk.fsz = s->regions.plan.foff.back();
  return nk;
}

constexpr double REGION_CHUNK_BYTES = 1024.0 * 1024.0 * 1024.0;   // the factor scratch of one chunk at most
}  // namespace

int mk::regions_interp_begin(mk_session* s, RegionInterp& ri, int t0, int Tc, int n_kept, int E) {
  Regions& r = s->regions;
  int rc = regions_begin(s, t0, Tc, n_kept);
  if (rc) return rc;
  hipStream_t st = s->stream;
  const int SQ = s->S * s->q, G = r.plan.G;
  const size_t fsz = (size_t)r.plan.foff.back();
  ri.E = E;
  ri.Sn = ri.bufs.get<double>((size_t)E * SQ * fsz);
  ri.means = ri.bufs.get<double>((size_t)s->S * n_kept * s->q * Tc);
  ri.slot = ri.bufs.get<int>((size_t)n_kept * SQ);
  ri.err = ri.bufs.get<unsigned long long>(1);
  if (!ri.Sn || !ri.means || !ri.slot || !ri.err) return MK_CHEB_EXACT;
  // the longest chunk whose factors fit: the budget's (or MK_REGIONS_CHUNK's), halved while HBM is short
  int B = region_chunk_len(REGION_CHUNK_BYTES, 8.0 * SQ * fsz, n_kept, env_int("MK_REGIONS_CHUNK", 0));
  for (;; B /= 2) {
    void* p = nullptr;
    if (hipMalloc(&p, (size_t)SQ * B * fsz * 8) == hipSuccess) {
      ri.bufs.p.push_back(p);
      ri.Lc = (double*)p;
      break;
    }
    (void)hipGetLastError();
    if (B == 1) return MK_CHEB_EXACT;
  }
  ri.plan = region_chunk_plan(s->cg.phi_h.data(), n_kept, SQ, G, B);
  ri.flagc = ri.bufs.get<int>((size_t)SQ * B * G);
  ri.jobs = ri.bufs.get<RegionJob>(ri.plan.jobs.size());
  if (!ri.flagc || !ri.jobs) return MK_CHEB_EXACT;
  // slots past a pair's last one stay zero and unread, like cheb_eval's rows of Sn
  HIPCHK(hipMemsetAsync(ri.Sn, 0, (size_t)E * SQ * fsz * 8, st));
  HIPCHK(hipMemsetAsync(ri.err, 0, 8, st));
  HIPCHK(hipMemcpyAsync(ri.slot, ri.plan.slot.data(), ri.plan.slot.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ri.jobs, ri.plan.jobs.data(), ri.plan.jobs.size() * sizeof(RegionJob), hipMemcpyHostToDevice, st));
  return 0;
}

int mk::regions_node(mk_session* s, const Group& gp, RegionInterp& ri, int e) {
  Regions& r = s->regions;
  hipStream_t st = s->stream;
  const RegionK rk = region_k(r);
  hipEvent_t a, b;
  const int rc = pending_pair(r, 0, &a, &b);
  if (rc) return rc;
  HIPCHK(hipEventRecord(a, st));
  MK_LAUNCH(k_region_cov_node, dim3((unsigned)(s->S * s->q * rk.G)), dim3(256), REGION_LDS_BYTES, st, gp.md, rk,
            (const int*)gp.d_plist, (const int*)gp.d_pcount, ri.Sn + (size_t)e * s->S * s->q * rk.fsz);
  HIPCHK(hipEventRecord(b, st));
  HIPCHK(hipGetLastError());
  return 0;
}

int mk::regions_check(mk_session* s, RegionInterp& ri, const ChebK& ck, double* emax) {
  Regions& r = s->regions;
  hipStream_t st = s->stream;
  const RegionNodesK nk = region_nodes_k(s, ri, ck);
  hipEvent_t a, b;
  const int rc = pending_pair(r, 0, &a, &b);
  if (rc) return rc;
  HIPCHK(hipEventRecord(a, st));
  MK_LAUNCH(k_region_check, dim3((unsigned)(nk.SQ * ((nk.fsz + 255) / 256))), dim3(256), 0, st, nk, ri.err);
  HIPCHK(hipEventRecord(b, st));
  HIPCHK(hipGetLastError());
  unsigned long long eb = 0;
  HIPCHK(hipMemcpyAsync(&eb, ri.err, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::memcpy(emax, &eb, 8);
  return 0;
}

int mk::regions_interp_draws(mk_session* s, RegionInterp& ri, const Model& mt, const ChebK& ck, int n_kept) {
  Regions& r = s->regions;
  hipStream_t st = s->stream;
  const RegionK rk = region_k(r);
  const RegionNodesK nk = region_nodes_k(s, ri, ck);
  const RegionChunkPlan& pl = ri.plan;
  const int maxm = r.plan.maxm, ld = maxm | 1;   // odd: the factor's row walks spread over the banks
  const int lds_bytes = maxm * ld * 8;
  HIPCHK(hipFuncSetAttribute((const void*)k_region_interp_factor, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
  RegionDrawI di;
  di.means = ri.means;
  di.slot = ri.slot;
  di.kA = s->md.kA;
  di.L = ri.Lc;
  di.flag = ri.flagc;
  di.B = pl.B;
  di.k_lo = s->win_lo;
  const ProbSrc ps = prob_src(s, 0);
  int ahead = 0;
  for (int c = 0; c < pl.chunks; ++c) {
    const int j0 = c * pl.B, nb = std::min(pl.B, n_kept - j0);
    const long nj = pl.joff[(size_t)c + 1] - pl.joff[(size_t)c];
    hipEvent_t a, b;
    int rc = pending_pair(r, 0, &a, &b);
    if (rc) return rc;
    HIPCHK(hipEventRecord(a, st));
    MK_LAUNCH(k_region_interp_factor, dim3((unsigned)nj), dim3(256), lds_bytes, st, rk, nk,
              (const RegionJob*)(ri.jobs + pl.joff[(size_t)c]), ld, pl.B, ri.Lc, ri.flagc);
    HIPCHK(hipEventRecord(b, st));
    if ((rc = pending_pair(r, 1, &a, &b))) return rc;
    di.j0 = j0;
    HIPCHK(hipEventRecord(a, st));
    MK_LAUNCH(k_region_draw<true>, dim3((unsigned)((long)nb * s->S * rk.G)), dim3(256), 0, st, mt, rk, ps, 0, 0, n_kept, r.draws,
              r.singular, di);
    HIPCHK(hipEventRecord(b, st));
    HIPCHK(hipGetLastError());
    // the host stays at most 32 states' worth of launches ahead of the device (predict_tile_cheb's convention)
    if ((ahead += nb) >= 32) {
      HIPCHK(hipStreamSynchronize(st));
      ahead = 0;
    }
  }
  return 0;
}

int mk::tile_regions(mk_session* s, int t0, int n_kept, int Ct) {
  (void)Ct;
  Regions& r = s->regions;
  hipStream_t st = s->stream;
  r.fill.begin(s->win_lo, n_kept);
  EventTimer t;
  int rc = t.start(st);
  if (rc) return rc;
  if ((rc = launch_quantiles((unsigned)(s->S * r.C3), st, r.draws, (long)n_kept * r.C3, (long)r.C3, n_kept, r.C3,
                             s->d_probs, MK_N_LEVELS, r.grids)))
    return rc;
  if ((rc = launch_map_values(st, r.draws, (long)n_kept * r.C3, (long)r.C3, n_kept, r.C3, s->S, r.th, r.planes))) return rc;
  if ((rc = t.stop(st))) return rc;
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, t.a, t.b));
  r.ms[2] += ms;
  if ((rc = t.price(s, KS_REGIONS, 2)) || (rc = price_pending(s))) return rc;
  r.fill.mark(t0);
  return 0;
}

extern "C" int mk_session_set_regions(mk_session* s, const mk_region_spec* spec) {
  if (!s) return set_err(MK_E_ARG, "null session");
  MapThr th{};
  RegionPlan plan;
  if (spec) {   // before any device is touched; nothing can be attached in a state these refuse
    const std::string bad_t = region_thresholds_check(spec->thresholds, spec->n_thresholds);
    if (!bad_t.empty()) return set_err(MK_E_ARG, bad_t);
    int rc = map_thresholds(spec->thresholds, spec->n_thresholds, &th);
    if (rc) return rc;
    if (!s->tiled)
      return set_err(MK_E_ARG, "areal prediction needs the exact tiled replay, and this session was not created with "
                               "predict_tile > 0: create it with predict_tile >= the number of test sites (and attach "
                               "the sites with mk_session_set_test_sites)");
    if (s->n_test_all < 1) return set_err(MK_E_ARG, "areal prediction needs test sites: the session has none");
    if (!s->d_xt)
      return set_err(MK_E_ARG, "areal prediction needs x_test (mk_problem.x_test or mk_session_set_test_covars)");
    if (!s->md.samples)
      return set_err(MK_E_ARG, "areal prediction reads beta from the recorded samples (record_samples = 0)");
    if (s->n_test_all > s->pred_tile)
      return set_err(MK_E_ARG, "areal prediction: the regions live in one tile, and the " + std::to_string(s->n_test_all) +
                                   " test sites exceed the session's tile of " + std::to_string(s->pred_tile) +
                                   " (mk_session_predict_tile): a larger predict_tile, or fewer test sites per call");
    const bool have_ct = (long)s->ct_h.size() == 2L * s->n_test_all;
    const std::string bad = region_plan(spec->n_regions, spec->offsets, s->n_test_all, spec->weights,
                                        have_ct ? s->ct_h.data() : nullptr,
                                        have_ct ? s->ct_h.data() + s->n_test_all : nullptr, &plan);
    if (!bad.empty()) return set_err(MK_E_ARG, bad);
  }
  MK_ENTRY_DEVICE(s->device);
  HIPCHK(hipStreamSynchronize(s->stream));
  regions_detach(s);
  if (!spec) return 0;
  Regions& r = s->regions;
  const int G = plan.G, C3 = G * s->q, J = th.J;
  const size_t fsz = (size_t)plan.foff.back(), SQ = (size_t)s->S * s->q;
  const size_t nd = (size_t)s->S * s->md.n_kept * C3, ng = (size_t)s->S * C3 * MK_N_LEVELS, npl = (size_t)s->S * (2 + J) * C3;
  int rc = s->alloc(&r.offsets, (size_t)G + 1);
  if (!rc) rc = s->alloc(&r.foff, (size_t)G + 1);
  if (!rc) rc = s->alloc(&r.omega, (size_t)s->n_test_all);
  if (!rc) rc = s->alloc(&r.L, SQ * fsz);
  if (!rc) rc = s->alloc(&r.flag, SQ * G);
  if (!rc) rc = s->alloc(&r.draws, nd);
  if (!rc) rc = s->alloc(&r.singular, (size_t)s->S * C3);
  if (!rc) rc = s->alloc(&r.grids, ng);
  if (!rc) rc = s->alloc(&r.planes, npl);
  if (rc) {
    regions_detach(s);
    if (rc == MK_E_NOMEM)
      return sink_nomem("the region factors, draws, grids and planes (" + std::to_string(8 * fsz) +
                            " bytes of factors per pair; in all: ",
                        (SQ * fsz + nd + ng + npl) * 8, "do not", "a budget MK_KRIG_MEM_GB, or fewer or smaller regions leave room");
    return rc;
  }
  HIPCHK(hipFuncSetAttribute((const void*)k_region_cov, hipFuncAttributeMaxDynamicSharedMemorySize, REGION_LDS_BYTES));
  HIPCHK(hipFuncSetAttribute((const void*)k_region_cov_node, hipFuncAttributeMaxDynamicSharedMemorySize, REGION_LDS_BYTES));
  HIPCHK(hipMemcpy(r.offsets, plan.offsets.data(), ((size_t)G + 1) * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(r.foff, plan.foff.data(), ((size_t)G + 1) * sizeof(long), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(r.omega, plan.omega.data(), (size_t)s->n_test_all * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(r.flag, 0, SQ * G * sizeof(int)));
  HIPCHK(hipMemset(r.singular, 0, (size_t)s->S * C3 * sizeof(int)));
  r.fill.attach(s->n_test_all, s->pred_tile);
  r.plan = std::move(plan);
  r.C3 = C3;
  r.th = th;
  r.on = true;
  return 0;
}

extern "C" int mk_session_set_regions_route(mk_session* s, int32_t route) {
  if (!s) return set_err(MK_E_ARG, "null session");
  Regions& r = s->regions;
  if (!r.on) return set_err(MK_E_ARG, std::string(kWords.off) + ": the route belongs to an attached spec");
  if (route != MK_REGIONS_EXACT && route != MK_REGIONS_INTERP)
    return set_err(MK_E_ARG, "areal prediction: unknown route " + std::to_string(route) +
                                 " (MK_REGIONS_EXACT = 0, MK_REGIONS_INTERP = 1)");
  r.route = route;
  // the node-count rule counts the phi range in units of the correlation decay over the largest distance S sees
  r.dmax = 0.0;
  if (route == MK_REGIONS_INTERP && (long)s->ct_h.size() == 2L * s->n_test_all) {
    const double* cx = s->ct_h.data();
    const double* cy = cx + s->n_test_all;
    for (int g = 0; g < r.plan.G; ++g)
      for (int i = r.plan.offsets[g]; i < r.plan.offsets[g + 1]; ++i)
        for (int j = i + 1; j < r.plan.offsets[g + 1]; ++j) r.dmax = std::fmax(r.dmax, std::hypot(cx[i] - cx[j], cy[i] - cy[j]));
  }
  return 0;
}

extern "C" int mk_session_regions_route(mk_session* s, int32_t* asked, int32_t* ran, double* check) {
  if (!s) return set_err(MK_E_ARG, "null session");
  const Regions& r = s->regions;
  if (!r.on) return set_err(MK_E_ARG, kWords.off);
  if (asked) *asked = r.route;
  if (ran) *ran = r.ran;
  if (check) *check = r.check;
  return 0;
}

extern "C" int mk_session_regions(mk_session* s, mk_regions* o) {
  int rc = results_entry(s, o, &mk_session::regions, kWords);
  if (rc) return rc;
  Regions& r = s->regions;
  MK_ENTRY_DEVICE(s->device);
  hipStream_t st = s->stream;
  const size_t S = (size_t)s->S, C3 = (size_t)r.C3, n = (size_t)(s->win_n < 0 ? s->md.n_kept : s->win_n);
  // [S][C3][200] == per subset 200 x C3 column-major; [S][2 + J][C3] == per subset C3 x (2 + J) column-major;
  // [S][n][C3] == per subset C3 x kept column-major
  if (o->region_predict)
    HIPCHK(hipMemcpyAsync(o->region_predict, r.grids, S * C3 * MK_N_LEVELS * 8, hipMemcpyDeviceToHost, st));
  if (o->planes) HIPCHK(hipMemcpyAsync(o->planes, r.planes, S * (2 + r.th.J) * C3 * 8, hipMemcpyDeviceToHost, st));
  if (o->region_samples) HIPCHK(hipMemcpyAsync(o->region_samples, r.draws, S * n * C3 * 8, hipMemcpyDeviceToHost, st));
  if (o->singular) HIPCHK(hipMemcpyAsync(o->singular, r.singular, S * C3 * sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (o->timing_ms)
    for (int i = 0; i < 3; ++i) o->timing_ms[i] = r.ms[i];
  return 0;
}
