// PSIS-LOO on the device (include/mk.h "leave-one-out"): Pareto-smoothed importance-sampling leave-one-out
// elpd and the shape estimate k-hat per observation, from the recorded chain or from a caller's matrix of
// log-likelihood terms.  Nothing here runs, and nothing is allocated, unless it is asked for.
//
// k_loo_terms: the terms l_ik of a chunk of subsets (crit_eta, loglik_term: the criteria's inlines with the
// same operands in the same order).  The recorded w are [subset][iteration][Np]: a workgroup reads a tile of
// 64 observations x 64 states with the observation on the lane (consecutive doubles of one state's row),
// transposes it through LDS (pitch 65 doubles: the transposed read of lane k is at dword 130 k + 2 i, 32
// distinct even banks per half wave) and writes [observation][state] rows with the state on the lane.
// k_loo_psis: one workgroup of 256 threads owns one observation.  Its row goes to LDS padded with +inf to a
// power of two and is sorted ascending in l by a bitonic network: r = -l - max(-l) falls as l rises, so the
// first M sorted entries are the tail, largest r first, and entry M is the cut.  The generalised-Pareto fit
// deals the G values of theta over the four waves, the tail over the lanes (lane j, j + 64, ...; the wave's
// xor-shuffle tree): an order fixed by M alone.  The log-sum-exps take sorted entries t, t + 256, ... per
// thread, then block_sum<256>'s fixed tree.  Two observations with the same terms in another order give the
// same bytes; nothing depends on the chunk or the workgroup an observation ran in.
// k_loo_finish: one workgroup per subset; thread t adds observations t, t + 256, ... in turn, then the fixed
// tree (k_crit_finish's order, fixed by n_s q alone); the variance is two-pass.  k_loo_total: the totals.
// The library is built without FMA contraction or fast-math; every formula is in the order mk.h writes it.
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "mk_session.hpp"

namespace mk {

constexpr int LOO_TILE = 64, LOO_PITCH = LOO_TILE + 1;
constexpr int LOO_MAX_TAIL = 272;   // ceil(3 sqrt(MK_LOO_MAX_STATES))
constexpr int LOO_MAX_G = 48;       // 30 + floor(sqrt(LOO_MAX_TAIL)) = 46

// The terms of subsets s0 + blockIdx.z: states first, first + thin, ... (n of them; 0-based iterations) of
// observations i < n_s q into ell[(blockIdx.z * Np + i) * n + k].  Grid (ceil(Np / 64), ceil(n / 64), subsets).
__global__ __launch_bounds__(256) void k_loo_terms(Model md, int s0, int first, int n, int thin, double* __restrict__ ell) {
  __shared__ double tile[LOO_TILE * LOO_PITCH];
  const int s = s0 + blockIdx.z, tid = threadIdx.x;
  const long Np = md.Np;
  const int nv = md.n_s[s] * md.q;
  const int i0 = blockIdx.x * LOO_TILE, k0 = blockIdx.y * LOO_TILE;
  if (i0 >= nv) return;
  {
    const int li = tid & 63, i = i0 + li;
    const bool mine = i < nv;
    const long o = (long)s * Np + i;
    const double y = mine ? md.y[o] : 0.0, wt = mine ? md.wt[o] : 0.0;
    const double* x = md.X + (long)s * md.p * Np + i;
    for (int lk = tid >> 6; lk < LOO_TILE; lk += 4) {
      const int k = k0 + lk;
      double l = 0.0;
      if (mine && k < n) {
        const long it = (long)s * md.n_samples + first + (long)k * thin;
        const double* beta = md.samples + it * md.P;
        const double w = md.w_samples[it * Np + i];
        l = loglik_term(y, wt, crit_eta(x, Np, beta, md.p, w), md.link);
      }
      tile[lk * LOO_PITCH + li] = l;
    }
  }
  __syncthreads();
  const int lk = tid & 63, k = k0 + lk;
  for (int li = tid >> 6; li < LOO_TILE; li += 4) {
    const int i = i0 + li;
    if (i < nv && k < n) ell[((long)blockIdx.z * Np + i) * n + k] = tile[lk * LOO_PITCH + li];
  }
}

// Where the rows of terms are and where the triples go.  Observation i of subset s (blockIdx.y): its n terms at
// ell + (s * per_subset + i) * n; its triple's value a (elpd_loo_i, k-hat_i, lppd_i) at
// pw[s * subset + a * plane + i0 + i].  Valid observations per subset: n_s[s] q, or nv where n_s is null.
struct LooRows {
  const double* ell;
  long per_subset;
  const int* n_s;
  int q, nv;
  double* pw;
  long plane, subset, i0;
};

// block_sum's tree with fmax (the values are finite or -inf).
template <int NT>
__device__ inline double block_max(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) t = fmax(t, red[w]);
    red[NT / 64] = t;
  }
  __syncthreads();
  return red[NT / 64];
}

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One observation per workgroup: grid (observations, subsets), n2 * 8 bytes of dynamic LDS (n2 the power of
// two >= n).  M: the tail length; G: the fit's grid; jstar: the 0-based position of x* in the ascending tail.
__global__ __launch_bounds__(256) void k_loo_psis(LooRows a, int n, int n2, int M, int G, int jstar) {
  extern __shared__ double row[];
  __shared__ double xs[LOO_MAX_TAIL];
  __shared__ double th[LOO_MAX_G], Lg[LOO_MAX_G], tw[LOO_MAX_G];
  __shared__ double red[8], bc[2];
  const int s = blockIdx.y, tid = threadIdx.x;
  const long i = blockIdx.x;
  const long nv = a.n_s ? (long)a.n_s[s] * a.q : (long)a.nv;
  if (i >= nv) return;
  const double* src = a.ell + ((long)s * a.per_subset + i) * n;
  double* out = a.pw + (long)s * a.subset + a.i0 + i;

  // the row into LDS, padded with +inf; a term that is not finite ends the observation
  double bad = 0.0, mx = -INFINITY;
  for (int k = tid; k < n2; k += 256) {
    double l = INFINITY;
    if (k < n) {
      l = src[k];
      if (!isfinite(l)) bad = 1.0;
      mx = fmax(mx, l);
    }
    row[k] = l;
  }
  bad = block_sum<256>(bad, red);
  if (bad != 0.0) {
    if (tid == 0) {
      out[0] = NAN;
      out[a.plane] = NAN;
      out[2 * a.plane] = NAN;
    }
    return;
  }
  // lppd_i = logsumexp_k(l_k) - log n
  mx = block_max<256>(mx, red);
  double t = 0.0;
  for (int k = tid; k < n; k += 256) t = t + exp(row[k] - mx);
  const double lppd = mx + log(block_sum<256>(t, red)) - log((double)n);

  // ascending in l: a bitonic network over the padded row
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int u = tid; u < (n2 >> 1); u += 256) {
        const int lo = ((u & ~(j - 1)) << 1) | (u & (j - 1)), hi = lo | j;
        const double vl = row[lo], vh = row[hi];
        if ((vl > vh) == ((lo & k) == 0)) {
          row[lo] = vh;
          row[hi] = vl;
        }
      }
    }
  __syncthreads();

  // r of sorted entry e: (-l) - max(-l); the tail is entries 0 .. M - 1 (r descending), the cut entry M
  const double mxr = -row[0];
  const double cut = (-row[M]) - mxr;
  const bool varies = ((-row[0]) - mxr) > ((-row[M - 1]) - mxr);
  double khat = INFINITY;
  bool smoothed = false;
  if (varies) {
    const double ec = exp(cut);
    for (int j = tid; j < M; j += 256) xs[j] = exp((-row[M - 1 - j]) - mxr) - ec;   // ascending
    __syncthreads();
    const double dM = (double)M;
    const double x_last = xs[M - 1], x_star = xs[jstar];
    const int lane = tid & 63;
    for (int g = tid >> 6; g < G; g += 4) {
      const double theta = 1.0 / x_last + (1.0 - sqrt((double)G / ((double)(g + 1) - 0.5))) / (3.0 * x_star);
      double acc = 0.0;
      for (int j = lane; j < M; j += 64) acc = acc + log1p(-theta * xs[j]);
      const double kg = wave_sum(acc) / dM;
      if (lane == 0) {
        th[g] = theta;
        Lg[g] = dM * (log(-theta / kg) - kg - 1.0);
      }
    }
    __syncthreads();
    if (tid < G) {
      double sum = 0.0;
      for (int h = 0; h < G; ++h) sum = sum + exp(Lg[h] - Lg[tid]);
      tw[tid] = th[tid] * (1.0 / sum);
    }
    __syncthreads();
    if (tid == 0) {
      double acc = 0.0;
      for (int g = 0; g < G; ++g) acc = acc + tw[g];
      bc[0] = acc;
    }
    __syncthreads();
    const double theta_hat = bc[0];
    double acc = 0.0;
    for (int j = tid; j < M; j += 256) acc = acc + log1p(-theta_hat * xs[j]);
    const double kk = block_sum<256>(acc, red) / dM;
    const double sigma = -kk / theta_hat;
    khat = (kk * dM + 5.0) / (dM + 10.0);
    if (isfinite(khat)) {
      // the j-th smallest tail value becomes the generalised-Pareto quantile at (j - 1/2) / M, capped at 0
      for (int j = tid; j < M; j += 256) {
        const double p = ((double)(j + 1) - 0.5) / dM;
        const double qv = sigma * expm1(-khat * log1p(-p)) / khat;
        const double v = log(qv + ec);
        xs[j] = v > 0.0 ? 0.0 : v;
      }
      smoothed = true;
      __syncthreads();
    }
  }

  // lw = r - logsumexp(r); elpd_loo_i = logsumexp_k(l_k + lw_k)
  double m = -INFINITY;
  for (int e = tid; e < n; e += 256) {
    const double r = (smoothed && e < M) ? xs[M - 1 - e] : (-row[e]) - mxr;
    m = fmax(m, r);
  }
  m = block_max<256>(m, red);
  t = 0.0;
  for (int e = tid; e < n; e += 256) {
    const double r = (smoothed && e < M) ? xs[M - 1 - e] : (-row[e]) - mxr;
    t = t + exp(r - m);
  }
  const double lse_r = m + log(block_sum<256>(t, red));
  m = -INFINITY;
  for (int e = tid; e < n; e += 256) {
    const double r = (smoothed && e < M) ? xs[M - 1 - e] : (-row[e]) - mxr;
    m = fmax(m, row[e] + (r - lse_r));
  }
  m = block_max<256>(m, red);
  t = 0.0;
  for (int e = tid; e < n; e += 256) {
    const double r = (smoothed && e < M) ? xs[M - 1 - e] : (-row[e]) - mxr;
    t = t + exp((row[e] + (r - lse_r)) - m);
  }
  const double elpd = m + log(block_sum<256>(t, red));
  if (tid == 0) {
    out[0] = elpd;
    out[a.plane] = khat;
    out[2 * a.plane] = lppd;
  }
}

// The triples of subset blockIdx.x (LooRows' pw addressing, i0 = 0) and, where y is not null, its data at
// y + s * ld, wt + s * ld (null: lconst 0).
struct LooFin {
  const double* pw;
  long plane, subset;
  const int* n_s;
  int q, nv;
  const double* y;
  const double* wt;
  long ld;
};

// The eight rows of subset blockIdx.x from its pointwise triples.
__global__ __launch_bounds__(256) void k_loo_finish(LooFin f, double* __restrict__ rows) {
  __shared__ double red[8];
  const int s = blockIdx.x, tid = threadIdx.x;
  const long nv = f.n_s ? (long)f.n_s[s] * f.q : (long)f.nv;
  const double* e = f.pw + (long)s * f.subset;
  const double* kh = e + f.plane;
  const double* lp = e + 2 * f.plane;
  double te = 0.0, tl = 0.0, tn = 0.0, tb = 0.0, tc = 0.0, km = -INFINITY;
  for (long i = tid; i < nv; i += 256) {
    te = te + e[i];
    tl = tl + lp[i];
    if (kh[i] > 0.7) tn = tn + 1.0;
    km = fmax(km, kh[i]);
    if (isnan(lp[i])) tb = tb + 1.0;
    if (f.y) {
      const double y = f.y[(long)s * f.ld + i], wt = f.wt[(long)s * f.ld + i];
      tc = tc + (lgamma(wt + 1.0) - lgamma(y + 1.0) - lgamma(wt - y + 1.0));
    }
  }
  const double elpd = block_sum<256>(te, red);
  const double lppd = block_sum<256>(tl, red);
  const double n_bad = block_sum<256>(tn, red);
  const double bad = block_sum<256>(tb, red);
  const double lconst = block_sum<256>(tc, red);
  const double k_max = block_max<256>(km, red);
  const double dn = (double)nv;
  const double mean = elpd / dn;
  double tv = 0.0;
  for (long i = tid; i < nv; i += 256) {
    const double d = e[i] - mean;
    tv = tv + d * d;
  }
  const double var = block_sum<256>(tv, red) / (dn - 1.0);
  if (tid != 0) return;
  double* o = rows + (long)s * MK_N_LOO;
  o[0] = elpd;
  o[1] = lppd - elpd;
  o[2] = -2.0 * elpd;
  o[3] = sqrt(dn * var);
  o[4] = lppd;
  o[5] = k_max;
  o[6] = n_bad;
  if (bad != 0.0)
    for (int r = 0; r < 7; ++r) o[r] = NAN;
  o[7] = lconst;
}

// The totals over the subsets in subset order (one workgroup): sums, the maximum of k_max (a NaN row makes it
// NaN), the root of the summed squares of se_elpd_loo.
__global__ __launch_bounds__(64) void k_loo_total(const double* __restrict__ rows, int S, double* __restrict__ out) {
  const int r = threadIdx.x;
  if (r >= MK_N_LOO) return;
  double acc = rows[r];
  if (r == 3) acc = acc * acc;
  for (int s = 1; s < S; ++s) {
    const double v = rows[(long)s * MK_N_LOO + r];
    if (r == 5)
      acc = (isnan(v) || v > acc) ? v : acc;
    else if (r == 3)
      acc = acc + v * v;
    else
      acc = acc + v;
  }
  out[r] = r == 3 ? sqrt(acc) : acc;
}

}  // namespace mk

using namespace mk;

// ------------------------------------------------------------------ host side
namespace {

struct LooShape {
  int n2, M, G, jstar;
};

// The tail length, the fit's grid and the position of x* that n states give (include/mk.h).
LooShape loo_shape(int n) {
  LooShape p;
  p.n2 = 1;
  while (p.n2 < n) p.n2 <<= 1;
  p.M = std::min(n / 5, (int)std::ceil(3.0 * std::sqrt((double)n)));
  p.G = 30 + (int)std::floor(std::sqrt((double)p.M));
  p.jstar = (int)std::floor((double)p.M / 4.0 + 0.5) - 1;
  return p;
}

int loo_check_states(long n) {
  if (n < MK_LOO_MIN_STATES)
    return set_err(MK_E_ARG, "PSIS-LOO needs >= " + std::to_string(MK_LOO_MIN_STATES) + " states (a tail of 5), not " +
                                 std::to_string(n));
  if (n > MK_LOO_MAX_STATES)
    return set_err(MK_E_ARG, "PSIS-LOO takes <= " + std::to_string(MK_LOO_MAX_STATES) + " states, not " + std::to_string(n) +
                                 ": a larger thin keeps every thin-th state of the window");
  return 0;
}

int launch_psis(hipStream_t st, const LooRows& rows, long n_obs, int n_subsets, int n, const LooShape& p) {
  HIPCHK(hipFuncSetAttribute((const void*)k_loo_psis, hipFuncAttributeMaxDynamicSharedMemorySize, MK_LOO_MAX_STATES * 8));
  MK_LAUNCH(k_loo_psis, dim3((unsigned)n_obs, (unsigned)n_subsets), dim3(256), (size_t)p.n2 * 8, st, rows, n, p.n2, p.M, p.G,
            p.jstar);
  return 0;
}

}  // namespace

extern "C" int mk_session_loo(mk_session* s, int32_t thin, mk_loo* o) {
  if (!s || !o) return set_err(MK_E_ARG, "null session/loo");
  if (s->poisoned) return poisoned_err(s);
  const Model& md = s->md;
  if (thin < 1) return set_err(MK_E_ARG, "thin must be >= 1");
  if (s->iter < md.n_samples) return set_err(MK_E_ARG, "PSIS-LOO needs all n.samples iterations");
  if (!md.samples || !md.w_samples)
    return set_err(MK_E_ARG, "PSIS-LOO replays the recorded chain: that needs record_samples and record_w");
  const int win_lo = s->tiled ? s->win_lo : s->crit.win_lo, win_n = s->tiled ? s->win_n : s->crit.win_n;
  const int span = win_n < 0 ? md.n_kept : win_n;
  const int n = (span + thin - 1) / thin;
  int rc = loo_check_states(n);
  if (rc) return rc;
  const LooShape p = loo_shape(n);
  MK_ENTRY_DEVICE(s->device);
  const int S = s->S;
  const long Np = md.Np;
  hipStream_t st = s->stream;
  // subsets per chunk of the terms' scratch: the environment's count, else 1 GiB of it; 1 .. S
  const size_t per_subset = (size_t)Np * n * 8;
  const long by_bytes = std::max<long>(1, (long)(((size_t)1 << 30) / per_subset));
  const long asked = env_int("MK_LOO_CHUNK", 0);
  const int chunk = (int)std::min<long>(asked > 0 ? asked : by_bytes, S);
  DevBufs scratch;
  double* d_ell = scratch.get<double>((size_t)chunk * Np * n);
  if (!d_ell)
    return set_err(MK_E_NOMEM, "the PSIS-LOO terms (" + std::to_string(per_subset) + " B per subset, " + std::to_string(chunk) +
                                   " subsets at a time) do not fit in HBM beside the session: a smaller MK_LOO_CHUNK, a larger "
                                   "thin or a shorter kept window leave room");
  double* d_pw = scratch.get<double>((size_t)S * 3 * Np);
  double* d_rows = scratch.get<double>((size_t)(S + 1) * MK_N_LOO);
  if (!d_pw || !d_rows) return set_err(MK_E_NOMEM, "PSIS-LOO scratch");
  EventTimer t;
  if ((rc = t.start(st))) return rc;
  long launches = 2;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int sc = std::min(chunk, S - s0);
    MK_LAUNCH(k_loo_terms, dim3((unsigned)((Np + LOO_TILE - 1) / LOO_TILE), (unsigned)((n + LOO_TILE - 1) / LOO_TILE), (unsigned)sc),
              dim3(256), 0, st, md, s0, md.kept0 + win_lo, n, (int)thin, d_ell);
    const LooRows rows{d_ell, Np, md.n_s + s0, md.q, 0, d_pw + (size_t)s0 * 3 * Np, Np, 3 * Np, 0};
    if ((rc = launch_psis(st, rows, Np, sc, n, p))) return rc;
    launches += 2;
  }
  const LooFin fin{d_pw, Np, 3 * Np, md.n_s, md.q, 0, md.y, md.wt, Np};
  MK_LAUNCH(k_loo_finish, dim3(S), dim3(256), 0, st, fin, d_rows);
  MK_LAUNCH(k_loo_total, dim3(1), dim3(64), 0, st, (const double*)d_rows, S, d_rows + (size_t)S * MK_N_LOO);
  HIPCHK(hipGetLastError());
  if ((rc = t.stop(st))) return rc;
  if (o->subsets) HIPCHK(hipMemcpyAsync(o->subsets, d_rows, (size_t)S * MK_N_LOO * 8, hipMemcpyDeviceToHost, st));
  if (o->total) HIPCHK(hipMemcpyAsync(o->total, d_rows + (size_t)S * MK_N_LOO, MK_N_LOO * 8, hipMemcpyDeviceToHost, st));
  if (o->pointwise) {
    double* h = o->pointwise;
    for (int i = 0; i < S; ++i) {   // subset i: (n_s q) x 3 column-major from its three planes
      const size_t nv = (size_t)s->n_part[i] * s->q;
      HIPCHK(hipMemcpy2DAsync(h, nv * 8, d_pw + (size_t)i * 3 * Np, (size_t)Np * 8, nv * 8, 3, hipMemcpyDeviceToHost, st));
      h += 3 * nv;
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  return t.price(s, KS_LOO, launches);
}

extern "C" int mk_loo_matrix(const double* ell, int64_t n_obs, int32_t n_states, double* pointwise, double* row,
                             int32_t device) {
  if (!ell) return set_err(MK_E_ARG, "null log-likelihood matrix");
  if (n_obs < 1 || n_obs > 0x7fffffffL) return set_err(MK_E_ARG, "n_obs must be 1 .. 2^31 - 1");
  int rc = loo_check_states(n_states);
  if (rc) return rc;
  const int n = n_states;
  const LooShape p = loo_shape(n);
  const long chunk = col_chunk("MK_LOO_CHUNK", n, (long)n_obs);
  MK_ENTRY_DEVICE(device);
  DevBufs bufs;
  double* d_ell = bufs.get<double>((size_t)chunk * n);
  double* d_pw = bufs.get<double>((size_t)3 * n_obs);
  double* d_row = bufs.get<double>(MK_N_LOO);
  if (!d_ell || !d_pw || !d_row) return set_err(MK_E_NOMEM, "PSIS-LOO matrix buffers");
  int lrc = 0;
  rc = upload_col_chunks(ell, n, (long)n_obs, chunk, d_ell, [&](long c0, long nc) {
    const LooRows rows{d_ell, 0, nullptr, 1, (int)nc, d_pw, (long)n_obs, 0, c0};
    const int r = launch_psis((hipStream_t)0, rows, nc, 1, n, p);
    if (r && !lrc) lrc = r;
  });
  if (lrc) return lrc;
  if (rc) return rc;
  const LooFin fin{d_pw, (long)n_obs, 0, nullptr, 1, (int)n_obs, nullptr, nullptr, 0};
  MK_LAUNCH(k_loo_finish, dim3(1), dim3(256), 0, (hipStream_t)0, fin, d_row);
  HIPCHK(hipGetLastError());
  if (pointwise) HIPCHK(hipMemcpy(pointwise, d_pw, (size_t)3 * n_obs * 8, hipMemcpyDeviceToHost));
  if (row) HIPCHK(hipMemcpy(row, d_row, MK_N_LOO * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipDeviceSynchronize());
  return 0;
}
