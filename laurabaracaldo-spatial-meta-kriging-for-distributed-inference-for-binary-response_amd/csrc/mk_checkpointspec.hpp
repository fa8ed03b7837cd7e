// Checkpoints (include/mk.h "checkpoints") on the host, before the device is touched: the layout of a session's
// state at an iteration, the session's side of a checkpoint and of a restore, the sizes and values a restore is
// given, and the arithmetic of the state digest (one term, the regions' enumeration).  Each refusal names the
// global subset index, the field, and the expected and given size or the word.  Standard headers and mk.h only,
// so the checks are tested on the host (tests/checkpointspec_test.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include "../../include/mk.h"

namespace mk {

// mk_checkpoint.hip compiles the digest's term and the regions' enumeration for the device too, so the kernel and
// the host's restatement are one expression
#ifndef MK_CKPT_HD
#define MK_CKPT_HD
#endif

enum {
  CK_BETA = 0, CK_THETA, CK_W, CK_ETA, CK_TUNE, CK_ACC, CK_U, CK_Z, CK_ZZ, CK_LOGDET, CK_QUAD, CK_AFULL, CK_AINV, CK_NOTPD,
  CK_CRIT_ACC, CK_CRIT_PART, CK_CRIT_SBETA, CK_SAMPLES, CK_W_SAMPLES, CK_ACC_HIST, CK_KZ, CK_KTH, CK_KA, CK_W_PRED
};
static_assert(CK_W_PRED + 1 == MK_CKPT_NFIELDS, "the fields of include/mk.h");

constexpr int CKPT_NB = 128;         // MK_NB: the factor tile
constexpr int CKPT_CRIT_PLANES = 6;  // MK_CRIT_ACC: running values per observation of the in-chain criteria

inline const char* ckpt_field_name(int f) {
  static const char* const names[MK_CKPT_NFIELDS] = {
      "beta", "theta", "w", "eta", "tune", "acc", "u", "z", "Z", "logdetR", "quad", "A_full", "Ainv", "notpd",
      "crit_acc", "crit_part", "crit_sbeta", "samples", "w_samples", "acc_hist", "kz", "kth", "kA", "w_pred"};
  return (f >= 0 && f < MK_CKPT_NFIELDS) ? names[f] : "?";
}
inline const char* ckpt_digest_name(int b) {
  static const char* const names[MK_CKPT_NDIGEST] = {"L", "Winv", "W", "QB"};
  return (b >= 0 && b < MK_CKPT_NDIGEST) ? names[b] : "?";
}

// What the layout needs of a session's dimensions (mk_checkpoint.hip fills it from the Model).
struct CkptDims {
  int S = 0, subset_base = 0, q = 1, p = 0, n_pad = 0;
  int n_samples = 0, batch_length = 1, kept0 = 0;   // kept states are iterations kept0 .. n_samples - 1 (0-based)
  int n_test = 0;                                   // test sites of a fused session's draws
  bool matern = false, tiled = false, record_w = false, criteria = false;
  int ntri() const { return q * (q + 1) / 2; }
  int n_theta() const { return ntri() + q * (matern ? 2 : 1); }
  int P() const { return p + n_theta(); }
  long Np() const { return (long)n_pad * q; }
  long nmh() const { return P() + Np(); }
  long crit_nb() const { return (Np() + 255) / 256; }
  int kept_done(int iteration) const { return iteration > kept0 ? iteration - kept0 : 0; }
};

// words[f]: 8-byte words per subset of field f after `iteration` iterations.
inline void ckpt_layout(const CkptDims& d, int iteration, int64_t* words) {
  const long q = d.q, np = d.n_pad, Np = d.Np(), k = d.kept_done(iteration), it = iteration;
  words[CK_BETA] = d.p;
  words[CK_THETA] = d.n_theta();
  words[CK_W] = Np;
  words[CK_ETA] = Np;
  words[CK_TUNE] = d.nmh();
  words[CK_ACC] = d.nmh();
  words[CK_U] = q * np;
  words[CK_Z] = q * np;
  words[CK_ZZ] = q * q * np;
  words[CK_LOGDET] = q;
  words[CK_QUAD] = q;
  words[CK_AFULL] = q * q;
  words[CK_AINV] = q * q;
  words[CK_NOTPD] = q;
  words[CK_CRIT_ACC] = (d.criteria && k > 0) ? CKPT_CRIT_PLANES * Np : 0;
  words[CK_CRIT_PART] = d.criteria ? k * d.crit_nb() : 0;
  words[CK_CRIT_SBETA] = (d.criteria && k > 0) ? d.p : 0;
  words[CK_SAMPLES] = it * d.P();
  words[CK_W_SAMPLES] = d.record_w ? it * Np : 0;
  words[CK_ACC_HIST] = (it / d.batch_length) * (d.P() + 1);
  words[CK_KZ] = d.tiled ? k * q * np : 0;
  words[CK_KTH] = d.tiled ? k * d.n_theta() : 0;
  words[CK_KA] = d.tiled ? k * q * q : 0;
  words[CK_W_PRED] = (!d.tiled && d.n_test > 0) ? k * q * d.n_test : 0;
}

// The session's side of mk_session_checkpoint: "" when its state may be written, else the message.
inline std::string ckpt_write_check(bool imported, bool poisoned, int S, int first, int count) {
  if (poisoned) return "checkpoint: the session is unusable after an earlier failure";
  if (imported)
    return "checkpoint: the session holds an imported chain, which has the recorded states and no sampler state; the fit "
           "file (save_session) keeps such a session";
  if (first < 0 || count < 1 || first > S - count)
    return "checkpoint: subsets [" + std::to_string(first) + ", " + std::to_string((long)first + count) +
           ") are outside the session's " + std::to_string(S) + " subsets";
  return "";
}

// The session's side of mk_session_restore.
inline std::string ckpt_session_check(int iterations_run, bool imported, bool poisoned) {
  if (poisoned) return "restore: the session is unusable after an earlier failure";
  if (imported) return "restore: the session holds an imported chain; a state is restored into a session that never ran";
  if (iterations_run > 0)
    return "restore: the session has run " + std::to_string(iterations_run) +
           " iterations (or was restored before); a state is restored into a session as mk_session_create left it";
  return "";
}

// The schedules make the same decisions and round z differently, so the schedule is part of what
// fixes a chain's bytes: "the schedule is fixed once the chain has started" (mk_session_set_lookahead) holds for a
// restored chain too.  The schedule a session continues a state on: its own where no iteration separates the two
// (iteration 0: it runs the whole chain; n.samples: none of it), else the one that wrote the state.
inline int ckpt_schedule(int written_lookahead, int session_lookahead, int iteration, int n_samples) {
  return (iteration <= 0 || iteration >= n_samples) ? (session_lookahead != 0) : (written_lookahead != 0);
}
// "" when the session can run that schedule, else the message: several stream groups have the sequential one alone.
inline std::string ckpt_schedule_check(int written_lookahead, int session_lookahead, bool lookahead_eligible, int iteration,
                                       int n_samples) {
  if (ckpt_schedule(written_lookahead, session_lookahead, iteration, n_samples) == 0 || lookahead_eligible) return "";
  return "restore: the state was written mid-chain (iteration " + std::to_string(iteration) +
         ") under the lookahead schedule, which this session cannot run (several stream groups, n_streams > 1, have the "
         "sequential schedule alone); the two round z differently, so the chain continued here would not be the same "
         "bytes: make the session with n_streams <= 1";
}

// The caller's side: the iteration, the sizes against the layout, the pointers, the values.  fields[f] is
// [S] x words[f]; "" when the state is fine, else the message.
inline std::string ckpt_restore_check(const CkptDims& d, int iteration, const int64_t* words, void* const* fields,
                                      const uint64_t* digests) {
  if (iteration < 0 || iteration > d.n_samples)
    return "restore: iteration " + std::to_string(iteration) + " is outside 0 .. n.samples = " + std::to_string(d.n_samples);
  if (!words || !fields) return "restore: null sizes/fields";
  int64_t want[MK_CKPT_NFIELDS];
  ckpt_layout(d, iteration, want);
  const std::string subs = "subsets " + std::to_string(d.subset_base) + " .. " + std::to_string(d.subset_base + d.S - 1);
  for (int f = 0; f < MK_CKPT_NFIELDS; ++f) {
    if (words[f] != want[f])
      return "restore: " + subs + ", field '" + ckpt_field_name(f) + "' has " + std::to_string((long long)words[f]) +
             " words per subset; the session's layout at iteration " + std::to_string(iteration) + " has " +
             std::to_string((long long)want[f]) + " (n_pad " + std::to_string(d.n_pad) + ", q " + std::to_string(d.q) + ")";
    if (want[f] > 0 && !fields[f])
      return "restore: " + subs + ", field '" + ckpt_field_name(f) + "' is null; the layout has " +
             std::to_string((long long)want[f]) + " words per subset";
  }
  if (!digests) return "restore: null digests";
  const int finite[3] = {CK_THETA, CK_TUNE, CK_W};
  for (int i = 0; i < d.S; ++i) {
    for (int f : finite) {
      const double* a = (const double*)fields[f] + (long)i * want[f];
      for (long j = 0; j < want[f]; ++j)
        if (!std::isfinite(a[j]))
          return "restore: subset " + std::to_string(d.subset_base + i) + ", field '" + ckpt_field_name(f) + "', word " +
                 std::to_string(j) + " is " + std::to_string(a[j]) + "; every value must be finite";
    }
    const double* a = (const double*)fields[CK_ACC] + (long)i * want[CK_ACC];
    for (long j = 0; j < want[CK_ACC]; ++j)
      if (!(a[j] >= 0.0) || !std::isfinite(a[j]) || a[j] != std::floor(a[j]))
        return "restore: subset " + std::to_string(d.subset_base + i) + ", field 'acc', word " + std::to_string(j) + " is " +
               std::to_string(a[j]) + "; an accept count is a non-negative integer";
  }
  return "";
}

// ---------------------------------------------------------------- the state digest
// One term: mix(x + (i + 1) golden), mix the splitmix64 finaliser; the digest is the terms' sum mod 2^64.
MK_CKPT_HD inline uint64_t digest_term(uint64_t x, uint64_t i) {
  uint64_t v = x + (i + 1) * 0x9E3779B97F4A7C15ull;
  v ^= v >> 30;
  v *= 0xBF58476D1CE4E5B9ull;
  v ^= v >> 27;
  v *= 0x94D049BB133111EBull;
  v ^= v >> 31;
  return v;
}

// A region is cut into columns; column j of a buffer holds the rows [r_lo, r_hi) at base + off, and row r of it is
// word idx0 + r of the region's enumeration.  r_hi <= r_lo: the column is outside the region.
struct DigestCol {
  long off, idx0;
  int r_lo, r_hi;
};
// MK_DIGEST_L, MK_DIGEST_W: column j of the ld x ld matrix, rows j .. ns - 1; ld columns.
MK_CKPT_HD inline DigestCol digest_col_tri(int j, int ns, int ld) {
  DigestCol c;
  c.off = (long)j * ld;
  c.idx0 = (long)j * ns - (long)j * (j - 1) / 2 - j;
  c.r_lo = j;
  c.r_hi = j < ns ? ns : 0;
  return c;
}
// MK_DIGEST_WINV (quad = 0) and MK_DIGEST_QB (quad = 1): column j = 128 k + c of the nt 128 x 128 tiles, m the
// tile's rows below n_s.  Winv: rows c .. m - 1 of the tile's lower triangle.  QB holds the two diagonal 64 x 64
// quadrants of a tile alone (k_qblocks computes no other; the rest of the tile is never written): column c lies
// in quadrant c / 64 and holds that quadrant's rows below m.
MK_CKPT_HD inline DigestCol digest_col_tile(int j, int ns, int quad) {
  const int k = j / CKPT_NB, cc = j % CKPT_NB;
  int m = ns - k * CKPT_NB;
  m = m < 0 ? 0 : (m > CKPT_NB ? CKPT_NB : m);
  DigestCol c;
  c.off = (long)k * CKPT_NB * CKPT_NB + (long)cc * CKPT_NB;
  if (!quad) {
    c.r_lo = cc;
    c.r_hi = cc < m ? m : 0;
    // the tiles before k are whole triangles of 128 x 129 / 2
    c.idx0 = (long)k * (CKPT_NB * (CKPT_NB + 1) / 2) + (long)cc * m - (long)cc * (cc - 1) / 2 - cc;
    return c;
  }
  const int h = CKPT_NB / 2, sd = cc / h, r0 = sd * h;
  const int b0 = m < h ? m : h;                   // rows (and columns) of quadrant 0 below n_s
  const int b = sd == 0 ? b0 : (m > h ? m - h : 0);
  c.r_lo = r0;
  c.r_hi = cc < m ? r0 + b : 0;
  // the tiles before k are whole: two quadrants of 64 x 64; inside the tile quadrant 0's b0 x b0 come first
  c.idx0 = (long)k * 2 * h * h + (sd ? (long)b0 * b0 : 0L) + (long)(cc - r0) * b - r0;
  return c;
}
// Words of a region (the digest's m).
inline long digest_region_words(int buffer, int ns) {
  if (buffer == MK_DIGEST_L || buffer == MK_DIGEST_W) return (long)ns * (ns + 1) / 2;
  long m = 0;
  for (int k = 0; k * CKPT_NB < ns; ++k) {
    const long mk = ns - k * CKPT_NB > CKPT_NB ? CKPT_NB : ns - k * CKPT_NB;
    const long h = CKPT_NB / 2, b0 = mk < h ? mk : h, b1 = mk > h ? mk - h : 0;
    m += buffer == MK_DIGEST_QB ? b0 * b0 + b1 * b1 : mk * (mk + 1) / 2;
  }
  return m;
}

}  // namespace mk
