// Checkpoints (include/mk.h "checkpoints"): the session's state out and in, and the device digest of the factors a
// restore re-derives.  The host checks and the digest's arithmetic are mk_checkpointspec.hpp; here are the kernels,
// the transfers and the entry points.
//
// What is saved is every word a later iteration or output reads that is not a pure function of the data and the
// configuration (the list is in include/mk.h and DESIGN.md 4.11).  What is not saved -- the accepted factors L,
// their diagonal inverses Winv, W = L^-1, the tiles QB, a fused session's P^T, X and s -- is a pure function of
// the restored theta: chain_reinit runs the candidate, Cholesky and inverse kernels on it as mk_session_create
// does on the starting values, launch_pred_refresh rebuilds the kriging buffers of every pair, and the saved state
// is then uploaded over what those launches derived from it (logdetR, quad, z, eta, u carry the rounding of their
// incremental updates).  k_state_digest checks the claim: the digests of the re-derived factors against the ones
// the checkpoint carries.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#define MK_CKPT_HD __host__ __device__
#include "mk_checkpointspec.hpp"
#include "mk_session.hpp"

using namespace mk;

namespace mk {

enum { DG_TRI = 0, DG_TILE_TRI = 1, DG_TILE_QUAD = 2, DG_FLAT = 3 };   // DG_TILE_QUAD: a tile's two diagonal 64-quadrants
constexpr int DG_FLAT_COL = 512;   // words per column of a flat sequence: one 16-byte load per lane

// One buffer of every pair of a launch: pair sh's region starts at base + sh * pair_stride (+ cur[sh] * slot_stride
// where the buffer has two slots), cut into ncol columns (DigestCol).  DG_FLAT: one "pair", n_flat words whose
// first is word idx_off of the sequence.
struct DigestJob {
  const uint64_t* base;
  long pair_stride, slot_stride;
  const int* cur;   // NULL: one slot
  const int* n_s;   // [subset]
  int q, kind, ncol, ld;
  long n_flat;
  uint64_t idx_off;
};

__device__ inline uint64_t digest_block_sum(uint64_t v, uint64_t* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// Stage 1.  Grid (nblk, pairs): workgroup (b, sh) takes the columns b, b + nblk, ... of pair sh's region, a lane
// two adjacent rows per 16-byte load, and writes the sum of its terms to part[sh * nblk + b].  Integer addition
// commutes, so the digest depends on no launch shape.  Loads only; no atomics.
__global__ __launch_bounds__(256) void k_state_digest(DigestJob j, uint64_t* __restrict__ part) {
  __shared__ uint64_t red[256];
  const int sh = blockIdx.y;
  const int ns = j.kind == DG_FLAT ? 0 : j.n_s[sh / j.q];
  const uint64_t* base = j.base + (long)sh * j.pair_stride + (j.cur ? (long)j.cur[sh] * j.slot_stride : 0L);
  uint64_t acc = 0;
  for (int col = blockIdx.x; col < j.ncol; col += gridDim.x) {
    DigestCol c;
    if (j.kind == DG_TRI) {
      c = digest_col_tri(col, ns, j.ld);
    } else if (j.kind == DG_FLAT) {
      const long left = j.n_flat - (long)col * DG_FLAT_COL;
      c.off = (long)col * DG_FLAT_COL;
      c.idx0 = (long)j.idx_off + c.off;
      c.r_lo = 0;
      c.r_hi = left > DG_FLAT_COL ? DG_FLAT_COL : (int)left;
    } else {
      c = digest_col_tile(col, ns, j.kind == DG_TILE_QUAD);
    }
    if (c.r_hi <= c.r_lo) continue;
    for (int r = (c.r_lo & ~1) + 2 * (int)threadIdx.x; r < c.r_hi; r += 512) {
      const ulong2 v = *reinterpret_cast<const ulong2*>(base + c.off + r);
      if (r >= c.r_lo) acc += digest_term(v.x, (uint64_t)(c.idx0 + r));
      if (r + 1 < c.r_hi) acc += digest_term(v.y, (uint64_t)(c.idx0 + r + 1));
    }
  }
  const uint64_t tot = digest_block_sum(acc, red);
  if (threadIdx.x == 0) part[(long)sh * gridDim.x + blockIdx.x] = tot;
}

// Stage 2.  One workgroup per pair: out[sh * stride + slot] = the sum of its nblk partials.
__global__ __launch_bounds__(256) void k_digest_reduce(const uint64_t* __restrict__ part, int nblk, uint64_t* __restrict__ out,
                                                       int stride, int slot) {
  __shared__ uint64_t red[256];
  const int sh = blockIdx.x;
  uint64_t acc = 0;
  for (int b = threadIdx.x; b < nblk; b += 256) acc += part[(long)sh * nblk + b];
  const uint64_t tot = digest_block_sum(acc, red);
  if (threadIdx.x == 0) out[(long)sh * stride + slot] = tot;
}

}  // namespace mk

namespace {

// Workgroups per pair: the chip filled (256 CUs, 8 workgroups each) by the launch's pairs, at most one per column.
int digest_blocks(int pairs, int ncol) { return std::max(1, std::min(ncol, (2048 + pairs - 1) / pairs)); }

// The digests of the four factor buffers of subsets [first, first + count) into h ([count q][MK_CKPT_NDIGEST]), timed
// as KS_CKPT.  *ms (optional) gets the device time.
int session_digests(mk_session* s, int first, int count, uint64_t* h, double* ms = nullptr) {
  const Model& md = s->md;
  const MatSet& ms_ = s->ms;
  const int q = s->q, pairs = count * q, nt = s->nt, ld = s->n_pad;
  const long e = (long)ld * ld, tw = (long)nt * MK_NB * MK_NB;
  hipStream_t st = s->stream;
  const int nb_tri = digest_blocks(pairs, ld), nb_tile = digest_blocks(pairs, nt * MK_NB);
  DevBufs scratch;
  uint64_t* d_part = scratch.get<uint64_t>((size_t)pairs * std::max(nb_tri, nb_tile));
  uint64_t* d_out = scratch.get<uint64_t>((size_t)pairs * MK_CKPT_NDIGEST);
  if (!d_part || !d_out) return set_err(MK_E_NOMEM, "digest scratch");
  HIPCHK(hipMemsetAsync(d_out, 0, (size_t)pairs * MK_CKPT_NDIGEST * 8, st));
  DigestJob j{};
  j.q = q;
  j.n_s = md.n_s + first;
  j.ld = ld;
  const int* cur = ms_.cur + (long)first * q;
  EventTimer tm;
  int rc;
  if ((rc = tm.start(st))) return rc;
  long launches = 0;
  auto run = [&](int slot, int nblk) {
    MK_LAUNCH(k_state_digest, dim3(nblk, pairs), dim3(256), 0, st, j, d_part);
    MK_LAUNCH(k_digest_reduce, dim3(pairs), dim3(256), 0, st, (const uint64_t*)d_part, nblk, d_out, MK_CKPT_NDIGEST, slot);
    launches += 2;
  };
  // the accepted L slot: lower triangle below n_s
  j.base = (const uint64_t*)(ms_.L + (long)first * q * 2 * e);
  j.pair_stride = 2 * e;
  j.slot_stride = e;
  j.cur = cur;
  j.kind = DG_TRI;
  j.ncol = ld;
  run(MK_DIGEST_L, nb_tri);
  // the accepted Winv tiles: their lower triangles below n_s
  j.base = (const uint64_t*)(ms_.Winv + (long)first * q * 2 * tw);
  j.pair_stride = 2 * tw;
  j.slot_stride = tw;
  j.kind = DG_TILE_TRI;
  j.ncol = nt * MK_NB;
  run(MK_DIGEST_WINV, nb_tile);
  // W
  j.base = (const uint64_t*)(ms_.W + (long)first * q * e);
  j.pair_stride = e;
  j.slot_stride = 0;
  j.cur = nullptr;
  j.kind = DG_TRI;
  j.ncol = ld;
  run(MK_DIGEST_W, nb_tri);
  // QB: the diagonal 64-quadrants k_qblocks writes (block sweeps only; a site-sweep session keeps none: 0)
  if (ms_.QB) {
    j.base = (const uint64_t*)(ms_.QB + (long)first * q * tw);
    j.pair_stride = tw;
    j.kind = DG_TILE_QUAD;
    j.ncol = nt * MK_NB;
    run(MK_DIGEST_QB, nb_tile);
  }
  if ((rc = tm.stop(st))) return rc;
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h, d_out, (size_t)pairs * MK_CKPT_NDIGEST * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (ms) {
    float f = 0.f;
    HIPCHK(hipEventElapsedTime(&f, tm.a, tm.b));
    *ms = f;
  }
  return tm.price(s, KS_CKPT, launches);
}

CkptDims dims_of(const mk_session* s) {
  const Model& md = s->md;
  CkptDims d;
  d.S = s->S;
  d.subset_base = md.subset_base;
  d.q = s->q;
  d.p = s->p;
  d.n_pad = s->n_pad;
  d.n_samples = md.n_samples;
  d.batch_length = md.batch_length;
  d.kept0 = md.kept0;
  d.n_test = s->tiled ? 0 : md.n_test;
  d.matern = s->matern;
  d.tiled = s->tiled;
  d.record_w = s->record_w;
  d.criteria = s->crit.on;
  return d;
}

// Field f of subsets [first, first + count) between the host array h ([count] x words) and the device: the first
// `words` words of every subset's `stride` words at dev.
int xfer(bool to_host, void* h, void* dev, long stride, long words, int first, int count) {
  if (words <= 0) return 0;
  char* d = (char*)dev + (size_t)first * stride * 8;
  if (to_host)
    HIPCHK(hipMemcpy2D(h, (size_t)words * 8, d, (size_t)stride * 8, (size_t)words * 8, (size_t)count, hipMemcpyDeviceToHost));
  else
    HIPCHK(hipMemcpy2D(d, (size_t)stride * 8, h, (size_t)words * 8, (size_t)words * 8, (size_t)count, hipMemcpyHostToDevice));
  return 0;
}

// The kept-state record [n_kept][S_all][row]: the first k states of subsets [first, first + count), per subset
// [k][row] on the host.
int xfer_kept(bool to_host, void* h, double* dev, long S_all, long row, long k, int first, int count) {
  if (k <= 0 || row <= 0) return 0;
  for (int i = 0; i < count; ++i) {
    char* hp = (char*)h + (size_t)i * k * row * 8;
    double* d = dev + (size_t)(first + i) * row;
    if (to_host)
      HIPCHK(hipMemcpy2D(hp, (size_t)row * 8, d, (size_t)S_all * row * 8, (size_t)row * 8, (size_t)k, hipMemcpyDeviceToHost));
    else
      HIPCHK(hipMemcpy2D(d, (size_t)S_all * row * 8, hp, (size_t)row * 8, (size_t)row * 8, (size_t)k, hipMemcpyHostToDevice));
  }
  return 0;
}

// The sampler state (fields up to CK_NOTPD), or with `all` the criteria sums and the record too, of subsets
// [first, first + count) after `iteration` iterations.
int xfer_state(mk_session* s, bool to_host, void* const* f, int iteration, int first, int count, bool all) {
  Model& md = s->md;
  const CkptDims d = dims_of(s);
  int64_t w[MK_CKPT_NFIELDS];
  ckpt_layout(d, iteration, w);
  const long q = d.q, np = d.n_pad, Np = d.Np(), nmh = d.nmh();
  int rc;
  if ((rc = xfer(to_host, f[CK_BETA], md.beta, d.p, w[CK_BETA], first, count)) ||
      (rc = xfer(to_host, f[CK_THETA], md.theta, md.n_theta, w[CK_THETA], first, count)) ||
      (rc = xfer(to_host, f[CK_W], md.w, Np, w[CK_W], first, count)) ||
      (rc = xfer(to_host, f[CK_ETA], md.eta, Np, w[CK_ETA], first, count)) ||
      (rc = xfer(to_host, f[CK_TUNE], md.tune, nmh, w[CK_TUNE], first, count)) ||
      (rc = xfer(to_host, f[CK_ACC], md.acc, nmh, w[CK_ACC], first, count)) ||
      (rc = xfer(to_host, f[CK_U], md.u, q * np, w[CK_U], first, count)) ||
      (rc = xfer(to_host, f[CK_Z], md.z, q * np, w[CK_Z], first, count)) ||
      (rc = xfer(to_host, f[CK_ZZ], md.Z, q * q * np, w[CK_ZZ], first, count)) ||
      (rc = xfer(to_host, f[CK_LOGDET], md.logdetR, q, w[CK_LOGDET], first, count)) ||
      (rc = xfer(to_host, f[CK_QUAD], md.quad, q, w[CK_QUAD], first, count)) ||
      (rc = xfer(to_host, f[CK_AFULL], md.A_full, q * q, w[CK_AFULL], first, count)) ||
      (rc = xfer(to_host, f[CK_AINV], md.Ainv, q * q, w[CK_AINV], first, count)) ||
      (rc = xfer(to_host, f[CK_NOTPD], md.notpd, q, w[CK_NOTPD], first, count)))
    return rc;
  if (!all) return 0;
  if (s->crit.on) {
    const Crit& c = s->crit.buf;
    if ((rc = xfer(to_host, f[CK_CRIT_ACC], c.acc, (long)MK_CRIT_ACC * Np, w[CK_CRIT_ACC], first, count)) ||
        (rc = xfer(to_host, f[CK_CRIT_PART], c.part, (long)c.n_cap * c.nb, w[CK_CRIT_PART], first, count)) ||
        (rc = xfer(to_host, f[CK_CRIT_SBETA], c.sbeta, d.p, w[CK_CRIT_SBETA], first, count)))
      return rc;
  }
  const long n = md.n_samples, k = d.kept_done(iteration);
  if ((rc = xfer(to_host, f[CK_SAMPLES], md.samples, n * md.P, w[CK_SAMPLES], first, count)) ||
      (md.w_samples && (rc = xfer(to_host, f[CK_W_SAMPLES], md.w_samples, n * Np, w[CK_W_SAMPLES], first, count))) ||
      (rc = xfer(to_host, f[CK_ACC_HIST], md.acc_hist, (long)md.n_batch * (md.o_w + 1), w[CK_ACC_HIST], first, count)))
    return rc;
  if (s->tiled) {
    if ((rc = xfer_kept(to_host, f[CK_KZ], md.kz, md.S_all, q * np, k, first, count)) ||
        (rc = xfer_kept(to_host, f[CK_KTH], md.kth, md.S_all, md.n_theta, k, first, count)) ||
        (rc = xfer_kept(to_host, f[CK_KA], md.kA, md.S_all, q * q, k, first, count)))
      return rc;
  } else if (md.n_test > 0) {
    if ((rc = xfer(to_host, f[CK_W_PRED], md.w_pred, (long)md.n_kept * q * md.n_test, w[CK_W_PRED], first, count))) return rc;
  }
  return 0;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The device side of a restore.  Returns 0, an error that left the session as created, or an error after
// *poison was set.
int restore_device(mk_session* s, int iteration, const mk_checkpoint* in, const char** poison) {
  const Model& md = s->md;
  const int S = s->S, q = s->q;
  hipStream_t st = s->stream;
  HIPCHK(hipStreamSynchronize(st));
  // the starting state, should the restored theta not factor
  const CkptDims d = dims_of(s);
  int64_t w0[MK_CKPT_NFIELDS];
  ckpt_layout(d, 0, w0);
  std::vector<std::vector<uint64_t>> keep(CK_NOTPD + 1);
  void* kp[MK_CKPT_NFIELDS] = {};
  for (int f = 0; f <= CK_NOTPD; ++f) {
    keep[f].resize((size_t)S * w0[f]);
    kp[f] = keep[f].data();
  }
  int rc;
  if ((rc = xfer_state(s, true, kp, 0, 0, S, false))) return rc;
  auto t0 = std::chrono::steady_clock::now();
  if ((rc = xfer_state(s, false, in->field, iteration, 0, S, true))) {
    *poison = "a restore failed while uploading the state";
    return rc;
  }
  double ms_up = ms_since(t0);
  // the factors of the restored theta, as mk_session_create makes those of the starting values
  EventTimer tm;
  if ((rc = tm.start(st))) return rc;
  rc = chain_reinit(s);
  if (rc) {
    const std::string msg = mk_last_error();
    (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
    if (xfer_state(s, false, kp, 0, 0, S, false) || chain_reinit(s)) {
      *poison = "a failed restore could not bring back the session's initial state";
      return set_err(MK_E_HIP, *poison);
    }
    return set_err(rc, "restore: the restored theta does not factor -- " + msg);
  }
  // a fused session past its first kept iteration holds X = W P^T and s of every pair: both work lists name
  // every pair after chain_reinit
  if (!s->tiled && !s->kt.on && md.n_test > 0 && iteration > md.kept0 && iteration < md.n_samples)
    launch_pred_refresh(s, s->all);
  if ((rc = tm.stop(st))) return rc;
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  float ms_derive = 0.f;
  HIPCHK(hipEventElapsedTime(&ms_derive, tm.a, tm.b));
  // the saved sampler state over what the launches above derived from it (eta, u, logdetR, quad, z)
  t0 = std::chrono::steady_clock::now();
  if ((rc = xfer_state(s, false, in->field, iteration, 0, S, false))) {
    *poison = "a restore failed while uploading the state";
    return rc;
  }
  ms_up += ms_since(t0);
  std::vector<uint64_t> dg((size_t)S * q * MK_CKPT_NDIGEST);
  double ms_dig = 0.0;
  if ((rc = session_digests(s, 0, S, dg.data(), &ms_dig))) {
    *poison = "a restore failed while checking the re-derived factors";
    return rc;
  }
  for (int sh = 0; sh < S * q; ++sh)
    for (int b = 0; b < MK_CKPT_NDIGEST; ++b)
      if (dg[(size_t)sh * MK_CKPT_NDIGEST + b] != in->digests[(size_t)sh * MK_CKPT_NDIGEST + b]) {
        *poison = "a restore re-derived factors that are not the checkpoint's";
        char hex[64];
        std::snprintf(hex, sizeof hex, "%016llx against %016llx", (unsigned long long)dg[(size_t)sh * MK_CKPT_NDIGEST + b],
                      (unsigned long long)in->digests[(size_t)sh * MK_CKPT_NDIGEST + b]);
        return set_err(MK_E_HIP, "restore: subset " + std::to_string(md.subset_base + sh / q) + ", outcome " +
                                     std::to_string(sh % q) + ", buffer " + ckpt_digest_name(b) +
                                     ": the digest of the re-derived factor differs from the checkpoint's (" + hex +
                                     "); the chain is not continued");
      }
  s->rst.done = true;
  s->rst.ms_derive = ms_derive;
  s->rst.ms_digest = ms_dig;
  s->rst.ms_upload = ms_up;
  return 0;
}

}  // namespace

extern "C" int mk_session_checkpoint_layout(const mk_session* s, int32_t iteration, int64_t* words) {
  if (!s || !words) return set_err(MK_E_ARG, "null session/words");
  const int it = iteration < 0 ? s->iter : iteration;
  if (it > s->md.n_samples)
    return set_err(MK_E_ARG, "checkpoint layout: iteration " + std::to_string(it) + " is outside 0 .. n.samples = " +
                                 std::to_string(s->md.n_samples));
  ckpt_layout(dims_of(s), it, words);
  return 0;
}

extern "C" int mk_session_checkpoint(mk_session* s, int32_t first, int32_t count, mk_checkpoint* out) {
  if (!s || !out) return set_err(MK_E_ARG, "null session/checkpoint");
  const std::string why = ckpt_write_check(s->imp.done, s->poisoned != nullptr, s->S, first, count);
  if (!why.empty()) return set_err(MK_E_ARG, why);
  const CkptDims d = dims_of(s);
  int64_t w[MK_CKPT_NFIELDS];
  ckpt_layout(d, s->iter, w);
  for (int f = 0; f < MK_CKPT_NFIELDS; ++f)
    if (w[f] > 0 && !out->field[f])
      return set_err(MK_E_ARG, std::string("checkpoint: field '") + ckpt_field_name(f) + "' is null; the layout has " +
                                   std::to_string((long long)w[f]) + " words per subset");
  if (!out->digests) return set_err(MK_E_ARG, "checkpoint: null digests");
  out->lookahead = s->la.on ? 1 : 0;
  MK_ENTRY_DEVICE(s->device);
  HIPCHK(hipStreamSynchronize(s->stream));
  int rc;
  if ((rc = xfer_state(s, true, out->field, s->iter, first, count, true))) return rc;
  // words no kernel ever wrote (hipMalloc's bytes) are written as zero: eta past a subset's n_s q values and the
  // criteria's planes past them
  const long Np = d.Np();
  for (int i = 0; i < count; ++i) {
    const long nv = (long)s->n_part[first + i] * s->q;
    double* eta = (double*)out->field[CK_ETA] + (size_t)i * Np;
    std::memset(eta + nv, 0, (size_t)(Np - nv) * 8);
    if (w[CK_CRIT_ACC] > 0)
      for (int a = 0; a < MK_CRIT_ACC; ++a) {
        double* pl = (double*)out->field[CK_CRIT_ACC] + ((size_t)i * MK_CRIT_ACC + a) * Np;
        std::memset(pl + nv, 0, (size_t)(Np - nv) * 8);
      }
  }
  return session_digests(s, first, count, out->digests);
}

extern "C" int mk_session_digest(mk_session* s, uint64_t* out) {
  if (!s || !out) return set_err(MK_E_ARG, "null session/output");
  if (s->poisoned) return poisoned_err(s);
  MK_ENTRY_DEVICE(s->device);
  HIPCHK(hipStreamSynchronize(s->stream));
  return session_digests(s, 0, s->S, out);
}

extern "C" int mk_session_restore(mk_session* s, int32_t iteration, const int64_t* words, const mk_checkpoint* in) {
  if (!s || !in) return set_err(MK_E_ARG, "null session/checkpoint");
  std::string why = ckpt_session_check(s->iter + (s->rst.done ? 1 : 0), s->imp.done, s->poisoned != nullptr);
  if (!why.empty()) return set_err(MK_E_ARG, why);
  why = ckpt_restore_check(dims_of(s), iteration, words, in->field, in->digests);
  if (!why.empty()) return set_err(MK_E_ARG, why);
  why = ckpt_schedule_check(in->lookahead, s->la.on ? 1 : 0, s->la.ok, iteration, s->md.n_samples);
  if (!why.empty()) return set_err(MK_E_ARG, why);
  MK_ENTRY_DEVICE(s->device);
  const char* poison = nullptr;
  const int rc = restore_device(s, iteration, in, &poison);
  if (poison) s->poisoned = poison;
  if (rc) return rc;
  // carried schedule state is dropped: the lookahead re-primes its candidates, the early assembly its own
  s->la.next = -1;
  s->cov.pre = -1;
  s->kt.pending = false;
  // a chain that has started keeps its schedule (mk_session_set_lookahead): a state written mid-chain continues
  // on the schedule that wrote it, whatever this session was made with (its streams are made at the first run)
  const bool la = ckpt_schedule(in->lookahead, s->la.on ? 1 : 0, iteration, s->md.n_samples) != 0;
  if (la != s->la.on) {
    s->la.on = la;
    s->la.mode = la ? 1 : 0;
  }
  s->iter = iteration;
  return 0;
}

extern "C" int mk_session_restore_stats(const mk_session* s, double* ms_derive, double* ms_digest, double* ms_upload) {
  if (!s) return set_err(MK_E_ARG, "null session");
  if (!s->rst.done) return set_err(MK_E_ARG, "restore statistics need a restored session (mk_session_restore)");
  if (ms_derive) *ms_derive = s->rst.ms_derive;
  if (ms_digest) *ms_digest = s->rst.ms_digest;
  if (ms_upload) *ms_upload = s->rst.ms_upload;
  return 0;
}

// Words per upload of mk_digest: MK_DIGEST_CHUNK, else 2^25 (256 MiB); even, so that every chunk but the last
// ends on a 16-byte boundary.
static long digest_chunk_words() {
  const long asked = env_int("MK_DIGEST_CHUNK", 0);
  const long c = asked > 0 ? asked : (1L << 25);
  return std::max<long>(2, c & ~1L);
}

extern "C" int mk_digest(const void* words, int64_t n_words, int32_t device, uint64_t* out) {
  if (!out || n_words < 0 || (n_words > 0 && !words)) return set_err(MK_E_ARG, "null words/output or a negative count");
  *out = 0;
  if (n_words == 0) return 0;
  MK_ENTRY_DEVICE(device);
  const long chunk = std::min<long>(digest_chunk_words(), (n_words + 1) & ~1L);
  const int ncol_max = (int)((chunk + DG_FLAT_COL - 1) / DG_FLAT_COL);
  const int nblk_max = digest_blocks(1, ncol_max);
  DevBufs scratch;
  uint64_t* d = scratch.get<uint64_t>((size_t)chunk);   // even: the last lane's pair stays inside
  uint64_t* d_part = scratch.get<uint64_t>((size_t)nblk_max);
  uint64_t* d_out = scratch.get<uint64_t>(1);
  if (!d || !d_part || !d_out) return set_err(MK_E_NOMEM, "digest scratch");
  uint64_t total = 0;
  for (int64_t c0 = 0; c0 < n_words; c0 += chunk) {
    const long nc = (long)std::min<int64_t>(chunk, n_words - c0);
    if (nc & 1) HIPCHK(hipMemset(d + nc, 0, 8));
    HIPCHK(hipMemcpy(d, (const uint64_t*)words + c0, (size_t)nc * 8, hipMemcpyHostToDevice));
    DigestJob j{};
    j.base = d;
    j.q = 1;
    j.kind = DG_FLAT;
    j.ncol = (int)((nc + DG_FLAT_COL - 1) / DG_FLAT_COL);
    j.n_flat = nc;
    j.idx_off = (uint64_t)c0;
    const int nblk = digest_blocks(1, j.ncol);
    MK_LAUNCH(k_state_digest, dim3(nblk, 1), dim3(256), 0, (hipStream_t) nullptr, j, d_part);
    MK_LAUNCH(k_digest_reduce, dim3(1), dim3(256), 0, (hipStream_t) nullptr, (const uint64_t*)d_part, nblk, d_out, 1, 0);
    HIPCHK(hipGetLastError());
    uint64_t one = 0;
    HIPCHK(hipMemcpy(&one, d_out, 8, hipMemcpyDeviceToHost));
    total += one;
  }
  *out = total;
  return 0;
}
