// Model assessment on the device (include/mk.h "model assessment": spDiag's DIC rows, and WAIC, per
// subset): the kernels, the in-chain scratch and the session entry points.  Nothing here runs, and no
// scratch is allocated, unless criteria are asked for.
//
// One thread owns one observation (subset s, row i < n_s q of its Np).  Per state of the window it
// recomputes eta = x_i' beta + w_i (crit_eta: pred_prob's expression), takes the chain's likelihood
// term l (loglik_term) and updates five running values (crit_update) and the sum of w.  The in-chain
// kernel k_crit_accum keeps them in HBM between the kept iterations; the replay kernel k_crit_replay
// keeps them in registers while it walks the recorded states in time order.  Both call the same
// inlines with the same operands in the same order, so the two routes agree bit for bit.  Every state's
// sum of l over a workgroup's 256 observations (block_sum<256>, a fixed tree) goes to a partial per
// (subset, state, block); k_crit_finish adds a state's partials in block order and the states' D_k by
// thread t taking states t, t + 256, ... in turn and the fixed tree over the threads -- an order that
// depends on n alone.  The sums over observations (D.bar.Omega, lppd, p.waic, lconst) run the same
// way over i, an order fixed by n_pad q alone.  The closing formulas are plain products and
// quotients in the order written in mk.h (no FMA contraction; the updates' fused multiply-adds are
// explicit).
#include <hip/hip_runtime.h>
#include <cmath>
#include <string>
#include "mk_session.hpp"

namespace mk {

// The running values of one observation after k states.
struct CritState {
  double mean, m2;   // Welford: mean of l, sum of squared deviations
  double mx, sm;     // log sum_k exp(l_k) = mx + log(sm)
  double bad;        // 1 once an l was not finite
};

// State k (0-based position in the window) with likelihood term l.
__device__ inline void crit_update(CritState& st, double l, int k) {
  if (k == 0) {
    st.mean = l;
    st.m2 = 0.0;
    st.mx = l;
    st.sm = 1.0;
    st.bad = 0.0;
  } else {
    const double d = l - st.mean;
    st.mean = st.mean + d / (double)(k + 1);
    st.m2 = fma(d, l - st.mean, st.m2);
    if (l > st.mx) {
      st.sm = fma(st.sm, exp(st.mx - l), 1.0);
      st.mx = l;
    } else {
      st.sm = st.sm + exp(l - st.mx);
    }
  }
  if (!isfinite(l)) st.bad = 1.0;
}

// A running sum's state k: the first state sets it.
__device__ inline double crit_add(double cur, double v, int k) { return k == 0 ? v : cur + v; }

// Kept iteration kidx (0-based): grid (nb, S).
__global__ __launch_bounds__(256) void k_crit_accum(Model md, Crit c, int kidx) {
  __shared__ double red[8];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  const long Np = md.Np;
  const int nv = md.n_s[s] * md.q;
  const double* beta = md.beta + (long)s * md.p;
  double l = 0.0;
  if (i < nv) {
    const long o = (long)s * Np + i;
    const double w = md.w[o];
    l = loglik_term(md.y[o], md.wt[o], crit_eta(md.X + (long)s * md.p * Np + i, Np, beta, md.p, w), md.link);
    double* a = c.acc + (long)s * MK_CRIT_ACC * Np + i;
    CritState st{};
    if (kidx > 0) {
      st.mean = a[0];
      st.m2 = a[Np];
      st.mx = a[2 * Np];
      st.sm = a[3 * Np];
      st.bad = a[4 * Np];
    }
    crit_update(st, l, kidx);
    a[0] = st.mean;
    a[Np] = st.m2;
    a[2 * Np] = st.mx;
    a[3 * Np] = st.sm;
    a[4 * Np] = st.bad;
    a[5 * Np] = crit_add(kidx > 0 ? a[5 * Np] : 0.0, w, kidx);
  }
  const double tot = block_sum<256>(l, red);
  if (tid == 0) c.part[((long)s * c.n_cap + kidx) * c.nb + blockIdx.x] = tot;
  if (blockIdx.x == 0 && tid < md.p) {
    double* sb = c.sbeta + (long)s * md.p + tid;
    *sb = crit_add(kidx > 0 ? *sb : 0.0, beta[tid], kidx);
  }
}

// The same from the recorded chain: states first, first + thin, ... (n of them; 0-based iterations),
// beta from samples, w from w_samples.  Grid (nb, S).
__global__ __launch_bounds__(256) void k_crit_replay(Model md, Crit c, int first, int n, int thin) {
  __shared__ double red[8];
  const int s = blockIdx.y, tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
  const long Np = md.Np;
  const int nv = md.n_s[s] * md.q;
  const bool mine = i < nv;
  const long o = (long)s * Np + i;
  const double y = mine ? md.y[o] : 0.0, wt = mine ? md.wt[o] : 0.0;
  const double* x = md.X + (long)s * md.p * Np + i;
  const bool sums_beta = blockIdx.x == 0 && tid < md.p;
  CritState st{};
  double sw = 0.0, sb = 0.0;
  for (int k = 0; k < n; ++k) {
    const long it = (long)s * md.n_samples + first + (long)k * thin;
    const double* beta = md.samples + it * md.P;
    double l = 0.0;
    if (mine) {
      const double w = md.w_samples[it * Np + i];
      l = loglik_term(y, wt, crit_eta(x, Np, beta, md.p, w), md.link);
      crit_update(st, l, k);
      sw = crit_add(sw, w, k);
    }
    const double tot = block_sum<256>(l, red);
    if (tid == 0) c.part[((long)s * c.n_cap + k) * c.nb + blockIdx.x] = tot;
    if (sums_beta) sb = crit_add(sb, beta[tid], k);
  }
  if (mine) {
    double* a = c.acc + (long)s * MK_CRIT_ACC * Np + i;
    a[0] = st.mean;
    a[Np] = st.m2;
    a[2 * Np] = st.mx;
    a[3 * Np] = st.sm;
    a[4 * Np] = st.bad;
    a[5 * Np] = sw;
  }
  if (sums_beta) c.sbeta[(long)s * md.p + tid] = sb;
}

// The eight rows of subset blockIdx.x from the sums of n states; pointwise (optional): [S][2][Np],
// plane 0 lppd_i, plane 1 M2_i / (n - 1), rows i < n_s q.
__global__ __launch_bounds__(256) void k_crit_finish(Model md, Crit c, int n, double* __restrict__ rows,
                                                     double* __restrict__ pointwise) {
  __shared__ double red[8];
  const int s = blockIdx.x, tid = threadIdx.x;
  const long Np = md.Np;
  const int nv = md.n_s[s] * md.q, p = md.p;
  const double dn = (double)n;
  const double* a = c.acc + (long)s * MK_CRIT_ACC * Np;
  const double* sbeta = c.sbeta + (long)s * p;
  // bar.D: a state's partials in block order, then the states
  double t = 0.0;
  for (int k = tid; k < n; k += 256) {
    const double* pk = c.part + ((long)s * c.n_cap + k) * c.nb;
    double d = pk[0];
    for (int b = 1; b < c.nb; ++b) d = d + pk[b];
    t = t + (-2.0 * d);
  }
  const double bar_d = block_sum<256>(t, red) / dn;
  // D.bar.Omega at the window means
  const double* x = md.X + (long)s * p * Np;
  t = 0.0;
  for (int i = tid; i < nv; i += 256) {
    double acc = 0.0;
    for (int j = 0; j < p; ++j) acc = fma(x[(long)j * Np + i], sbeta[j] / dn, acc);
    const double eta = acc + a[5 * Np + i] / dn;
    t = t + loglik_term(md.y[(long)s * Np + i], md.wt[(long)s * Np + i], eta, md.link);
  }
  const double d_hat = -2.0 * block_sum<256>(t, red);
  // lppd, p.waic, lconst, and whether any term was not finite
  const double log_n = log(dn);
  double tl = 0.0, tp = 0.0, tc = 0.0, tb = 0.0;
  for (int i = tid; i < nv; i += 256) {
    const double li = a[2 * Np + i] + log(a[3 * Np + i]) - log_n;
    const double pi = a[Np + i] / (dn - 1.0);
    const double y = md.y[(long)s * Np + i], wt = md.wt[(long)s * Np + i];
    tl = tl + li;
    tp = tp + pi;
    tc = tc + (lgamma(wt + 1.0) - lgamma(y + 1.0) - lgamma(wt - y + 1.0));
    tb = tb + a[4 * Np + i];
    if (pointwise) {
      pointwise[((long)s * 2) * Np + i] = li;
      pointwise[((long)s * 2 + 1) * Np + i] = pi;
    }
  }
  const double lppd = block_sum<256>(tl, red);
  const double p_waic = block_sum<256>(tp, red);
  const double lconst = block_sum<256>(tc, red);
  const double bad = block_sum<256>(tb, red);
  if (tid != 0) return;
  double* o = rows + (long)s * MK_N_CRIT;
  const double p_d = bar_d - d_hat;
  o[0] = bar_d;
  o[1] = d_hat;
  o[2] = p_d;
  o[3] = bar_d + p_d;
  o[4] = lppd;
  o[5] = p_waic;
  o[6] = -2.0 * (lppd - p_waic);
  if (bad != 0.0)
    for (int r = 0; r < 7; ++r) o[r] = NAN;
  o[7] = lconst;
}

// Sums of the rows over the subsets in subset order (one workgroup).
__global__ __launch_bounds__(64) void k_crit_total(const double* __restrict__ rows, int S, double* __restrict__ out) {
  const int r = threadIdx.x;
  if (r >= MK_N_CRIT) return;
  double acc = rows[r];
  for (int s = 1; s < S; ++s) acc = acc + rows[(long)s * MK_N_CRIT + r];
  out[r] = acc;
}

}  // namespace mk

using namespace mk;

// ------------------------------------------------------------------ host side
static Crit crit_view(const Crit& c, const Model& all, int s0) {
  Crit v = c;
  v.acc = c.acc + (long)s0 * MK_CRIT_ACC * all.Np;
  v.part = c.part + (long)s0 * c.n_cap * c.nb;
  v.sbeta = c.sbeta + (long)s0 * all.p;
  return v;
}

void mk::launch_crit_accum(mk_session* s, Group& g, int kidx) {
  const Crit c = crit_view(s->crit.buf, s->md, g.s0);
  if (kidx < 0 || kidx >= c.n_cap) return;
  Timed t{KS_CRIT, ev_new(), ev_new(), 0.0};
  hipEventRecord(t.a, g.stream);
  MK_LAUNCH(k_crit_accum, dim3(c.nb, g.S), dim3(256), 0, g.stream, g.md, c, kidx);
  hipEventRecord(t.b, g.stream);
  s->crit.pending.push_back(t);
}

void mk::crit_drain(mk_session* s, bool price) {
  for (auto& t : s->crit.pending) {
    float ms = 0.f;
    if (price && hipEventSynchronize(t.b) == hipSuccess && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
      s->prof.stats[KS_CRIT].launches += 1;
      s->prof.stats[KS_CRIT].ms += ms;
    }
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  s->crit.pending.clear();
}

extern "C" int mk_session_set_criteria(mk_session* s, int32_t enable) {
  if (!s) return set_err(MK_E_ARG, "null session");
  if (s->imp.done)
    return set_err(MK_E_ARG, "in-chain criteria need the chain to run here: an imported session serves mk_session_criteria "
                             "by replaying its recorded chain (record_w)");
  if (s->iter > 0) return set_err(MK_E_ARG, "in-chain criteria are switched before the first mk_session_run only");
  const bool on = enable != 0;
  if (on == s->crit.on) return 0;
  MK_ENTRY_DEVICE(s->device);
  Crit& c = s->crit.buf;
  if (!on) {
    s->release(c.acc);
    s->release(c.part);
    s->release(c.sbeta);
    c = Crit{};
    s->crit.on = false;
    return 0;
  }
  const Model& md = s->md;
  c.nb = (md.Np + 255) / 256;
  c.n_cap = md.n_kept;
  int rc;
  if ((rc = s->alloc(&c.acc, (size_t)s->S * MK_CRIT_ACC * md.Np)) ||
      (rc = s->alloc(&c.part, (size_t)s->S * c.n_cap * c.nb)) || (rc = s->alloc(&c.sbeta, (size_t)s->S * md.p))) {
    s->release(c.acc);
    s->release(c.part);
    s->release(c.sbeta);
    c = Crit{};
    return rc;
  }
  s->crit.on = true;
  return 0;
}

extern "C" int mk_session_criteria(mk_session* s, int32_t thin, mk_criteria* o) {
  if (!s || !o) return set_err(MK_E_ARG, "null session/criteria");
  if (s->poisoned) return poisoned_err(s);
  const Model& md = s->md;
  if (thin < 1) return set_err(MK_E_ARG, "thin must be >= 1");
  if (s->iter < md.n_samples) return set_err(MK_E_ARG, "criteria need all n.samples iterations");
  const int win_lo = s->tiled ? s->win_lo : s->crit.win_lo, win_n = s->tiled ? s->win_n : s->crit.win_n;
  const bool in_chain = win_n < 0 && thin == 1 && s->crit.on;
  if (!in_chain && (!md.samples || !md.w_samples))
    return set_err(MK_E_ARG, s->crit.on
                                 ? "criteria of a kept window or with thin > 1 replay the recorded chain: that needs "
                                   "record_samples and record_w"
                                 : "criteria need mk_session_set_criteria before the first run, or the recorded chain "
                                   "(record_samples and record_w) to replay");
  const int span = win_n < 0 ? md.n_kept : win_n;
  const int n = in_chain ? md.n_kept : (span + thin - 1) / thin;
  if (n < 2) return set_err(MK_E_ARG, "criteria need >= 2 states, not " + std::to_string(n));
  MK_ENTRY_DEVICE(s->device);
  const int S = s->S;
  hipStream_t st = s->stream;
  DevBufs scratch;
  Crit c = s->crit.buf;
  int launches = 2;
  if (!in_chain) {
    c.nb = (md.Np + 255) / 256;
    c.n_cap = n;
    c.acc = scratch.get<double>((size_t)S * MK_CRIT_ACC * md.Np);
    c.part = scratch.get<double>((size_t)S * n * c.nb);
    c.sbeta = scratch.get<double>((size_t)S * md.p);
    if (!c.acc || !c.part || !c.sbeta) return set_err(MK_E_NOMEM, "criteria scratch");
  }
  double* d_rows = scratch.get<double>((size_t)(S + 1) * MK_N_CRIT);
  double* d_pw = o->pointwise ? scratch.get<double>((size_t)S * 2 * md.Np) : nullptr;
  if (!d_rows || (o->pointwise && !d_pw)) return set_err(MK_E_NOMEM, "criteria scratch");
  EventTimer t;
  int rc = t.start(st);
  if (rc) return rc;
  if (!in_chain) {
    MK_LAUNCH(k_crit_replay, dim3(c.nb, S), dim3(256), 0, st, md, c, md.kept0 + win_lo, n, (int)thin);
    launches += 1;
  }
  MK_LAUNCH(k_crit_finish, dim3(S), dim3(256), 0, st, md, c, n, d_rows, d_pw);
  MK_LAUNCH(k_crit_total, dim3(1), dim3(64), 0, st, (const double*)d_rows, S, d_rows + (size_t)S * MK_N_CRIT);
  HIPCHK(hipGetLastError());
  if ((rc = t.stop(st))) return rc;
  if (o->subsets) HIPCHK(hipMemcpyAsync(o->subsets, d_rows, (size_t)S * MK_N_CRIT * 8, hipMemcpyDeviceToHost, st));
  if (o->total) HIPCHK(hipMemcpyAsync(o->total, d_rows + (size_t)S * MK_N_CRIT, MK_N_CRIT * 8, hipMemcpyDeviceToHost, st));
  if (o->pointwise) {
    double* h = o->pointwise;
    for (int i = 0; i < S; ++i) {   // subset i: (n_s q) x 2 column-major from its two planes
      const size_t nv = (size_t)s->n_part[i] * s->q;
      HIPCHK(hipMemcpy2DAsync(h, nv * 8, d_pw + (size_t)i * 2 * md.Np, (size_t)md.Np * 8, nv * 8, 2, hipMemcpyDeviceToHost, st));
      h += 2 * nv;
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  return t.price(s, KS_CRIT, launches);
}
