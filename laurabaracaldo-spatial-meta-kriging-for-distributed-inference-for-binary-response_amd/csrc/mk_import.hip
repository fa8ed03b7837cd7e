// Sessions from a recorded chain (include/mk.h "sessions from a recorded chain"): the kept-state record
// (z, theta, A) every replay reads, rebuilt on the device from what a fit reports -- samples (beta | K | phi | nu)
// and w_samples (w = A u).  The host checks are mk_importspec.hpp; here are the kernels, the upload and the
// session entry points.
//
// Per kept state k and subset s: A = chol(K) (import_chol, the expressions the host check ran), theta = A's
// lower triangle with log diagonal | logit phi | logit nu, u_i = A^-1 w_i by forward substitution
// (k_import_state).  The factors go through the machinery of the interpolated replay's g pass (mk_krig.hip
// predict_tile_cheb, step 3): k_kept_dirty lists the pairs whose (phi_h, nu_h) differ from the previous state,
// and the candidate, Cholesky and inverse kernels refresh W = L^-1 for those pairs only.  z = W u is
// k_import_z: the pending states of a pair -- those since its W last changed -- are taken together just before
// its W changes again, B of them per pass over W.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <vector>
#define MK_IMPORT_HD __host__ __device__
#include "mk_importspec.hpp"
#include "mk_session.hpp"

using namespace mk;

namespace mk {

// Kept states [c0, c0 + gridDim.x) of every subset (blockIdx.y): the record's theta and A from the samples row,
// and u of every site into U ([state - c0][S][q][n_pad], rows >= n_s zero).  w of (state k, subset s) is at
// wsrc + s * w_sub + (k - c0) * w_state: the device's w_samples, or the staging chunk.
__global__ __launch_bounds__(256) void k_import_state(Model md, int c0, const double* __restrict__ wsrc, long w_sub,
                                                      long w_state, double* __restrict__ U) {
  __shared__ double Ash[MK_QMAX * MK_QMAX];
  const int kc = blockIdx.x, s = blockIdx.y, q = md.q, k = c0 + kc;
  const long row = (long)k * md.S_all + s;
  if (threadIdx.x == 0) {
    const double* smp = md.samples + ((long)s * md.n_samples + md.kept0 + k) * md.P;
    double A[MK_QMAX * MK_QMAX];
    import_chol(smp + md.p, q, A);   // the host check factored this K: every pivot is > 0
    double* th = md.kth + row * md.n_theta;
    int t = 0;
    for (int j = 0; j < q; ++j)
      for (int i = j; i < q; ++i, ++t) th[t] = (i == j) ? log(A[i + j * q]) : A[i + j * q];
    for (int h = 0; h < q; ++h) {
      const double ph = smp[md.p + md.ntri + h];
      th[md.ntri + h] = log((ph - md.phi_a[h]) / (md.phi_b[h] - ph));
      if (md.cov_model == MK_COV_MATERN) {
        const double nv = smp[md.p + md.ntri + q + h];
        th[md.ntri + q + h] = log((nv - md.nu_a[h]) / (md.nu_b[h] - nv));
      }
    }
    for (int i = 0; i < q * q; ++i) {
      md.kA[row * q * q + i] = A[i];
      Ash[i] = A[i];
    }
  }
  __syncthreads();
  const int ns = md.n_s[s];
  const double* w = wsrc + (long)s * w_sub + (long)kc * w_state;
  double* u = U + ((long)kc * md.S + s) * q * md.n_pad;
  for (int i = threadIdx.x; i < md.n_pad; i += 256) {
    double uv[MK_QMAX];
    for (int h = 0; h < q; ++h) {   // forward substitution, h ascending
      double v = 0.0;
      if (i < ns) {
        v = w[(long)i * q + h];
        for (int a = 0; a < h; ++a) v -= Ash[h + a * q] * uv[a];
        v = v / Ash[h + h * q];
      }
      uv[h] = v;
      u[(long)h * md.n_pad + i] = v;
    }
  }
}

// z = W u of the pending states [run_start[sh], j_end) of every listed pair sh (plist == NULL: every pair), B
// states per pass over W.  Grid: SQ x nt workgroups, the row blocks with the longest column range first; a
// workgroup owns 128 rows of one pair, a lane two adjacent rows (16-byte loads along W's columns, which are
// contiguous), and its four waves take the columns c = w mod 4 of every 128-column tile, whose u the workgroup
// stages in LDS.  Row r sums its columns c <= r, c < n_s -- row n_s of W is the chain's bordered row and never
// enters -- per wave in ascending order, then the waves as ((w0 + w1) + w2) + w3: an order that depends on
// nothing but r, so any batching, run length, chunk or shard gives the same bytes.  A lane past the triangle
// selects 0, it does not branch.  Rows >= n_s are written as +0.
template <int B>
__global__ __launch_bounds__(256) void k_import_z(Model md, MatSet ms, const double* __restrict__ U, int c0,
                                                  const int* __restrict__ plist, const int* __restrict__ pcount,
                                                  const int* __restrict__ run_start, int j_end) {
  __shared__ double us[MK_NB * B];          // [column][state]
  __shared__ double part[3 * B * MK_NB];    // waves 1..3: [wave - 1][state][row]
  const int SQ = md.S * md.q, nt = ms.nt;
  const int e = blockIdx.x % SQ, t = nt - 1 - blockIdx.x / SQ;
  if (plist && e >= *pcount) return;
  const int sh = plist ? plist[e] : e;
  const int j0 = run_start[sh];
  if (j0 >= j_end) return;
  const int ns = md.n_s[sh / md.q], n_pad = md.n_pad;
  const long ld = ms.ld;
  const double* Wp = ms.W + (long)sh * ld * ld;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = t * MK_NB + 2 * lane;
  // column tiles up to the diagonal one; none for a row block at or past n_s (its rows are +0)
  const int ct_end = t * MK_NB < ns ? t : -1;
  for (int kb = j0; kb < j_end; kb += B) {
    double a0[B], a1[B];
#pragma unroll
    for (int b = 0; b < B; ++b) a0[b] = a1[b] = 0.0;
    for (int ct = 0; ct <= ct_end; ++ct) {
      __syncthreads();
      for (int idx = threadIdx.x; idx < MK_NB * B; idx += 256) {
        const int b = idx / MK_NB, c = idx % MK_NB;
        const int k = min(kb + b, j_end - 1);   // past the run's end: a state that is computed and not stored
        us[c * B + b] = U[((long)(k - c0) * SQ + sh) * n_pad + ct * MK_NB + c];
      }
      __syncthreads();
      const double* Wc = Wp + (long)(ct * MK_NB) * ld + r;
#pragma unroll 4
      for (int cc = wv; cc < MK_NB; cc += 4) {
        const int c = ct * MK_NB + cc;
        const d2 w2 = *reinterpret_cast<const d2*>(Wc + (long)cc * ld);
        const double v0 = (c <= r && r < ns) ? w2.x : 0.0;
        const double v1 = (c <= r + 1 && r + 1 < ns) ? w2.y : 0.0;
#pragma unroll
        for (int b = 0; b < B; ++b) {
          const double ub = us[cc * B + b];
          a0[b] = fma(v0, ub, a0[b]);
          a1[b] = fma(v1, ub, a1[b]);
        }
      }
    }
    __syncthreads();
    if (wv > 0) {
#pragma unroll
      for (int b = 0; b < B; ++b) {
        part[((wv - 1) * B + b) * MK_NB + 2 * lane] = a0[b];
        part[((wv - 1) * B + b) * MK_NB + 2 * lane + 1] = a1[b];
      }
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (kb + b < j_end) {
          d2 z;
          z.x = ((a0[b] + part[(0 * B + b) * MK_NB + 2 * lane]) + part[(1 * B + b) * MK_NB + 2 * lane]) +
                part[(2 * B + b) * MK_NB + 2 * lane];
          z.y = ((a1[b] + part[(0 * B + b) * MK_NB + 2 * lane + 1]) + part[(1 * B + b) * MK_NB + 2 * lane + 1]) +
                part[(2 * B + b) * MK_NB + 2 * lane + 1];
          *reinterpret_cast<d2*>(md.kz + ((long)(kb + b) * md.S_all * md.q + sh) * n_pad + r) = z;
        }
      }
    }
  }
}

// After the factorisations of kept state j: the listed pairs' pending states start at j (plist == NULL: every
// pair's), a pair whose factorisation met a pivot that is not > 0 notes the first such state in bad (-1: none),
// and the factorisations made are counted.
__global__ __launch_bounds__(256) void k_import_mark(Model md, const int* __restrict__ plist, const int* __restrict__ pcount,
                                                     int* __restrict__ run_start, int j, int* __restrict__ bad,
                                                     unsigned long long* __restrict__ nfact) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int n = plist ? *pcount : md.S * md.q;
  if (e < n) {
    const int sh = plist ? plist[e] : e;
    run_start[sh] = j;
    if (plist && md.info[sh] && bad[sh] < 0) bad[sh] = j;
  }
  if (e == 0 && plist) *nfact += (unsigned long long)n;
}

}  // namespace mk

namespace {

struct ImportEvents {   // the events of one chunk's launches, reused chunk after chunk
  std::vector<hipEvent_t> ev;
  int used = 0;
  ~ImportEvents() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  bool create(int n) {
    for (int i = 0; i < n; ++i) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) return false;
      ev.push_back(e);
    }
    return true;
  }
  void next(hipStream_t st) { (void)hipEventRecord(ev[used++], st); }
};

typedef void (*ImportZKernel)(Model, MatSet, const double*, int, const int*, const int*, const int*, int);

// States per pass over W: 8 (16 accumulators of two rows: 32 VGPRs), or MK_IMPORT_BATCH rounded down to 1, 2, 4 or 8.
ImportZKernel import_z_kernel(int* batch) {
  const int asked = env_int("MK_IMPORT_BATCH", 8);
  const int B = asked >= 8 ? 8 : asked >= 4 ? 4 : asked >= 2 ? 2 : 1;
  *batch = B;
  return B == 8 ? k_import_z<8> : B == 4 ? k_import_z<4> : B == 2 ? k_import_z<2> : k_import_z<1>;
}

int import_nomem(size_t bytes) {
  return sink_nomem("import: the staging buffers of a chunk of kept states (", bytes, "do not",
                    "fewer subsets per session (fitfile.load_session's subsets=), or a session without record_w");
}

// The device side of the import.  An error leaves buffers of the record half written: the caller restores the
// session.
int import_device(mk_session* s, const mk_chain* c) {
  Model& md = s->md;
  const int S = s->S, q = s->q, SQ = S * q, P = s->P, n = md.n_samples, n_kept = md.n_kept, kept0 = md.kept0;
  const int n_pad = md.n_pad, Np = md.Np, nth = md.n_theta, n_w = c->n_w;
  hipStream_t st = s->stream;
  HIPCHK(hipStreamSynchronize(st));
  std::vector<long> woff((size_t)S + 1, 0);
  for (int i = 0; i < S; ++i) woff[(size_t)i + 1] = woff[(size_t)i] + (long)s->n_part[i] * q * n_w;
  // ---- samples ([S][n][P] on the device), w_samples with record_w, acceptance: the caller's values
  std::vector<double> h((size_t)S * n * P);
  for (size_t i = 0; i < (size_t)S; ++i)
    for (int it = 0; it < n; ++it)
      for (int col = 0; col < P; ++col) h[(i * n + it) * P + col] = c->samples[i * n * P + (size_t)col * n + it];
  HIPCHK(hipMemcpy(md.samples, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  if (c->acceptance) {
    const size_t nb = md.n_batch, nrep = md.o_w + 1;
    h.assign((size_t)S * nb * nrep, 0.0);
    for (size_t i = 0; i < (size_t)S; ++i)
      for (size_t b = 0; b < nb; ++b)
        for (size_t col = 0; col < nrep; ++col) h[(i * nb + b) * nrep + col] = c->acceptance[i * nb * nrep + col * nb + b];
    HIPCHK(hipMemcpy(md.acc_hist, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  }
  // the states of a chunk: 32 (the g pass's rule: the host waits for the device every 32 states), fewer where
  // the chunk's staging would pass 256 MiB
  const size_t per_state = (size_t)SQ * n_pad * 8 * (s->record_w ? 1 : 2);
  int cs = (int)std::max<size_t>(1, std::min<size_t>(32, ((size_t)256 << 20) / per_state));
  cs = std::min(cs, n_kept);
  // rows [it0, it0 + cnt) of every subset's w (iterations n - n_w + it0 ..) into hw as [cnt][S][Np] or, one
  // subset, [cnt][Np]; the padding zero
  auto gather = [&](std::vector<double>& hw, int i_lo, int i_hi, int it0, int cnt) {
    const int Sg = i_hi - i_lo;
    hw.assign((size_t)cnt * Sg * Np, 0.0);
    for (int k = 0; k < cnt; ++k)
      for (int i = i_lo; i < i_hi; ++i) {
        const long N = (long)s->n_part[i] * q;
        std::memcpy(hw.data() + ((size_t)k * Sg + (i - i_lo)) * Np, c->w_samples + woff[i] + (long)(it0 + k) * N, (size_t)N * 8);
      }
  };
  std::vector<double> hw;
  if (s->record_w)   // n_w == n: every iteration, into the record itself, through a bounded host buffer
    for (int i = 0; i < S; ++i)
      for (int it0 = 0; it0 < n; it0 += 256) {
        const int cnt = std::min(256, n - it0);
        gather(hw, i, i + 1, it0, cnt);
        HIPCHK(hipMemcpy(md.w_samples + ((size_t)i * n + it0) * Np, hw.data(), hw.size() * 8, hipMemcpyHostToDevice));
      }
  DevBufs scratch;
  double *d_U = nullptr, *d_w = nullptr;
  for (;;) {
    d_U = scratch.get<double>((size_t)cs * SQ * n_pad);
    d_w = s->record_w ? nullptr : scratch.get<double>((size_t)cs * S * Np);
    if (d_U && (s->record_w || d_w)) break;
    for (void* b : scratch.p) hipFree(b);
    scratch.p.clear();
    if (cs == 1) return import_nomem(per_state);
    cs = std::max(1, cs / 2);
  }
  int* d_run = scratch.get<int>((size_t)SQ);
  int* d_bad = scratch.get<int>((size_t)SQ);
  unsigned long long* d_nf = scratch.get<unsigned long long>(1);
  if (!d_run || !d_bad || !d_nf) return import_nomem(per_state * cs);
  HIPCHK(hipMemsetAsync(d_run, 0, (size_t)SQ * sizeof(int), st));
  HIPCHK(hipMemsetAsync(d_bad, 0xff, (size_t)SQ * sizeof(int), st));
  HIPCHK(hipMemsetAsync(d_nf, 0, 8, st));
  HIPCHK(hipMemsetAsync(md.info, 0, (size_t)SQ * sizeof(int), st));
  int B = 0;
  const ImportZKernel kz = import_z_kernel(&B);
  Group g = s->all;
  s->la.next = -1;   // the factor slots are the import's from here on
  s->cov.pre = -1;
  ImportEvents evs;
  if (!evs.create(3 * cs + 1)) return set_err(MK_E_HIP, "import: event");
  double ms_factor = 0.0, ms_z = 0.0;
  std::vector<int> bad((size_t)SQ);
  for (int c0 = 0; c0 < n_kept; c0 += cs) {
    const int cn = std::min(cs, n_kept - c0);
    const double* wsrc = md.w_samples ? md.w_samples + (size_t)(kept0 + c0) * Np : d_w;
    if (!s->record_w) {
      gather(hw, 0, S, n_w - n_kept + c0, cn);
      HIPCHK(hipMemcpy(d_w, hw.data(), hw.size() * 8, hipMemcpyHostToDevice));
    }
    MK_LAUNCH(k_import_state, dim3(cn, S), dim3(256), 0, st, md, c0, wsrc, s->record_w ? (long)n * Np : (long)Np,
              s->record_w ? (long)Np : (long)S * Np, d_U);
    evs.used = 0;
    for (int j = c0; j < c0 + cn; ++j) {
      Model mt = md;
      mt.theta = md.kth + (long)j * S * nth;
      const double* prev = j ? md.kth + (long)(j - 1) * S * nth : nullptr;
      MK_LAUNCH(k_kept_dirty, dim3(1), dim3(256), 0, st, mt, prev, s->d_slist, s->d_scount, g.d_plist, g.d_pcount);
      evs.next(st);
      // the listed pairs' W changes now: their pending states first (none at a chunk's first state)
      if (j > c0) MK_LAUNCH(kz, dim3(SQ * s->nt), dim3(256), 0, st, md, g.ms, d_U, c0, g.d_plist, g.d_pcount, d_run, j);
      evs.next(st);
      for (int hh = 0; hh < q; ++hh) {
        launch_candidates(mt, g.ms, st, S, hh, 1, 2, 0, s->d_slist + hh * S, s->d_scount + hh);
        launch_cholesky(s, g, hh, 1, s->d_slist + hh * S, s->d_scount + hh);
      }
      MK_LAUNCH(k_flip_pairs, dim3((SQ + 255) / 256), dim3(256), 0, st, g.ms, g.d_plist, g.d_pcount);
      launch_trinv(s, g, SQ, g.d_plist, g.d_pcount);
      MK_LAUNCH(k_import_mark, dim3((SQ + 255) / 256), dim3(256), 0, st, md, g.d_plist, g.d_pcount, d_run, j, d_bad, d_nf);
      evs.next(st);
      HIPCHK(hipGetLastError());
    }
    // the chunk's end: every pair's pending states (the next chunk's u replaces this one's)
    MK_LAUNCH(kz, dim3(SQ * s->nt), dim3(256), 0, st, md, g.ms, d_U, c0, (const int*)nullptr, (const int*)nullptr, d_run,
              c0 + cn);
    MK_LAUNCH(k_import_mark, dim3((SQ + 255) / 256), dim3(256), 0, st, md, (const int*)nullptr, (const int*)nullptr, d_run,
              c0 + cn, d_bad, d_nf);
    evs.next(st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(bad.data(), d_bad, (size_t)SQ * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int j = 0; j < cn; ++j) {   // per state: [dirty] e0 [z] e1 [factors] e2
      float a = 0.f, b = 0.f;
      HIPCHK(hipEventElapsedTime(&a, evs.ev[3 * j], evs.ev[3 * j + 1]));
      HIPCHK(hipEventElapsedTime(&b, evs.ev[3 * j + 1], evs.ev[3 * j + 2]));
      ms_z += a;
      ms_factor += b;
    }
    float a = 0.f;
    HIPCHK(hipEventElapsedTime(&a, evs.ev[3 * cn - 1], evs.ev[3 * cn]));
    ms_z += a;
    for (int sh = 0; sh < SQ; ++sh)
      if (bad[sh] >= 0)
        return set_err(MK_E_ARG, "import: subset " + std::to_string(md.subset_base + sh / q) + ", outcome " +
                                     std::to_string(sh % q) + ", iteration " + std::to_string(kept0 + bad[sh] + 1) +
                                     ": the correlation matrix R(phi, nu) of this kept state met a pivot that is not > 0");
  }
  unsigned long long nf = 0;
  HIPCHK(hipMemcpy(&nf, d_nf, 8, hipMemcpyDeviceToHost));
  s->imp.factorisations = (long)nf;
  s->imp.ms_factor = ms_factor;
  s->imp.ms_z = ms_z;
  s->imp.batch = B;
  return 0;
}

}  // namespace

extern "C" int mk_session_import_chain(mk_session* s, const mk_chain* c) {
  if (!s || !c) return set_err(MK_E_ARG, "null session/chain");
  std::string why = import_session_check(s->tiled, s->iter, s->imp.done, s->poisoned != nullptr, s->crit.on);
  if (!why.empty()) return set_err(MK_E_ARG, why);
  const Model& md = s->md;
  ImportDims d;
  d.S = s->S;
  d.subset_base = md.subset_base;
  d.q = s->q;
  d.p = s->p;
  d.n_samples = md.n_samples;
  d.kept0 = md.kept0;
  d.matern = s->matern;
  d.record_w = s->record_w;
  d.n_part = s->n_part.data();
  for (int h = 0; h < s->q; ++h) {
    d.phi_a[h] = md.phi_a[h];
    d.phi_b[h] = md.phi_b[h];
    d.nu_a[h] = md.nu_a[h];
    d.nu_b[h] = md.nu_b[h];
  }
  why = import_chain_check(d, c->samples, c->w_samples, c->n_w);
  if (!why.empty()) return set_err(MK_E_ARG, why);
  MK_ENTRY_DEVICE(s->device);
  const int rc = import_device(s, c);
  if (rc) {   // the session as mk_session_create left it: the factors at the starting values, no flag
    const std::string msg = mk_last_error();
    (void)hipStreamSynchronize(s->stream);
    (void)hipGetLastError();
    if (chain_reinit(s)) {
      s->poisoned = "a failed import could not restore the session's initial state";
      return set_err(MK_E_HIP, s->poisoned);
    }
    return set_err(rc, msg);
  }
  s->imp.done = true;
  s->imp.acc = c->acceptance != nullptr;
  s->iter = md.n_samples;
  return 0;
}

extern "C" int32_t mk_session_imported(const mk_session* s) { return (s && s->imp.done) ? 1 : 0; }

extern "C" int mk_session_import_stats(const mk_session* s, int64_t* factorisations, double* ms_factor, double* ms_z) {
  if (!s) return set_err(MK_E_ARG, "null session");
  if (!s->imp.done) return set_err(MK_E_ARG, "import statistics need an imported session (mk_session_import_chain)");
  if (factorisations) *factorisations = s->imp.factorisations;
  if (ms_factor) *ms_factor = s->imp.ms_factor;
  if (ms_z) *ms_z = s->imp.ms_z;
  return 0;
}
