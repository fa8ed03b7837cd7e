// A recorded chain handed to mk_session_import_chain (include/mk.h "sessions from a recorded chain") checked on
// the host, before the device is touched: the session's state, the pointers and n_w, every value finite, every
// kept phi (and nu) strictly inside its prior, every kept K positive definite.  Each refusal names the global
// subset index, the 1-based iteration and the column or row.  Standard headers only, so the checks are tested on
// the host (tests/importspec_test.cpp).
#pragma once
#include <cmath>
#include <string>

namespace mk {

constexpr int IMPORT_QMAX = 4;   // MK_QMAX: outcomes at most

// mk_import.hip compiles import_chol for the device too, so the host's check and the record's A are one expression
#ifndef MK_IMPORT_HD
#define MK_IMPORT_HD
#endif

// What the checks need of a session's dimensions and priors (mk_session_import_chain fills it from the Model).
struct ImportDims {
  int S = 0, subset_base = 0, q = 1, p = 0;
  int n_samples = 0, kept0 = 0;   // kept states are iterations kept0 .. n_samples - 1 (0-based)
  bool matern = false, record_w = false;
  const int* n_part = nullptr;    // [S] sites per subset
  double phi_a[IMPORT_QMAX] = {0, 0, 0, 0}, phi_b[IMPORT_QMAX] = {0, 0, 0, 0};
  double nu_a[IMPORT_QMAX] = {0, 0, 0, 0}, nu_b[IMPORT_QMAX] = {0, 0, 0, 0};
  int ntri() const { return q * (q + 1) / 2; }
  int P() const { return p + ntri() + q * (matern ? 2 : 1); }
  int n_kept() const { return n_samples - kept0; }
};

// The session's side: "" when a chain may be imported into it, else the message.
inline std::string import_session_check(bool tiled, int iteration, bool imported, bool poisoned, bool in_chain_criteria) {
  if (poisoned) return "import: the session is unusable after an earlier failure";
  if (imported) return "import: the session already holds an imported chain (a session takes one import)";
  if (iteration > 0)
    return "import: the session has run " + std::to_string(iteration) +
           " iterations; a chain is imported into a session that never ran";
  if (!tiled)
    return "import: the session keeps no chain states (fused kriging): create it with predict_tile > 0 and no test sites, "
           "or more test sites than the tile";
  if (in_chain_criteria)
    return "import: in-chain criteria cannot be filled by an import; mk_session_criteria replays the recorded chain "
           "(record_w) instead";
  return "";
}

// Lower Cholesky factor of the q x q matrix whose lower triangle (column-major, spBayes' order) is tri: A
// (column-major, q x q) with a positive diagonal; false when a pivot is not > 0 (K is not positive definite).
MK_IMPORT_HD inline bool import_chol(const double* tri, int q, double* A) {
  double K[IMPORT_QMAX * IMPORT_QMAX];
  int k = 0;
  for (int j = 0; j < q; ++j)
    for (int i = j; i < q; ++i, ++k) K[i + j * q] = K[j + i * q] = tri[k];
  for (int i = 0; i < q * q; ++i) A[i] = 0.0;
  for (int j = 0; j < q; ++j) {
    double d = K[j + j * q];
    for (int m = 0; m < j; ++m) d -= A[j + m * q] * A[j + m * q];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    const double piv = std::sqrt(d);
    A[j + j * q] = piv;
    for (int i = j + 1; i < q; ++i) {
      double v = K[i + j * q];
      for (int m = 0; m < j; ++m) v -= A[i + m * q] * A[j + m * q];
      A[i + j * q] = v / piv;
    }
  }
  return true;
}

// samples: [S] x (n_samples x P) column-major; w_samples: [S] x ((n_s q) x n_w) column-major, the last n_w
// iterations.  "" when the chain is fine, else the message.
inline std::string import_chain_check(const ImportDims& d, const double* samples, const double* w_samples, int n_w) {
  if (!samples) return "import: null samples";
  if (!w_samples) return "import: null w_samples";
  const int n = d.n_samples, kept = d.n_kept(), P = d.P(), q = d.q, ntri = d.ntri();
  if (n_w < kept || n_w > n)
    return "import: n_w = " + std::to_string(n_w) + " is outside kept .. n_samples = " + std::to_string(kept) + " .. " +
           std::to_string(n) + " (the w of every kept iteration is needed)";
  if (d.record_w && n_w != n)
    return "import: n_w = " + std::to_string(n_w) + " must be n_samples = " + std::to_string(n) +
           " for a session that records w (record_w)";
  auto where = [&](int i, int it) {
    return "subset " + std::to_string(d.subset_base + i) + ", iteration " + std::to_string(it + 1);
  };
  long woff = 0;
  for (int i = 0; i < d.S; ++i) {
    const double* sm = samples + (long)i * n * P;
    for (int c = 0; c < P; ++c)
      for (int it = 0; it < n; ++it)
        if (!std::isfinite(sm[(long)c * n + it]))
          return "import: samples of " + where(i, it) + ", column " + std::to_string(c) + " is " +
                 std::to_string(sm[(long)c * n + it]) + "; every value must be finite";
    const long N = (long)d.n_part[i] * q;
    const double* wm = w_samples + woff;
    for (int j = 0; j < n_w; ++j)
      for (long r = 0; r < N; ++r)
        if (!std::isfinite(wm[(long)j * N + r]))
          return "import: w_samples of " + where(i, n - n_w + j) + ", row " + std::to_string(r) + " is " +
                 std::to_string(wm[(long)j * N + r]) + "; every value must be finite";
    woff += N * n_w;
    for (int it = d.kept0; it < n; ++it) {
      for (int h = 0; h < q; ++h) {
        const int c = d.p + ntri + h;
        const double phi = sm[(long)c * n + it];
        if (!(phi > d.phi_a[h] && phi < d.phi_b[h]))
          return "import: phi of " + where(i, it) + ", column " + std::to_string(c) + " (outcome " + std::to_string(h) +
                 ") is " + std::to_string(phi) + ", not strictly inside its prior (" + std::to_string(d.phi_a[h]) + ", " +
                 std::to_string(d.phi_b[h]) + "): its logit would be infinite";
        if (d.matern) {
          const int cn = c + q;
          const double nu = sm[(long)cn * n + it];
          if (!(nu > d.nu_a[h] && nu < d.nu_b[h]))
            return "import: nu of " + where(i, it) + ", column " + std::to_string(cn) + " (outcome " + std::to_string(h) +
                   ") is " + std::to_string(nu) + ", not strictly inside its prior (" + std::to_string(d.nu_a[h]) + ", " +
                   std::to_string(d.nu_b[h]) + "): its logit would be infinite";
        }
      }
      double tri[IMPORT_QMAX * (IMPORT_QMAX + 1) / 2], A[IMPORT_QMAX * IMPORT_QMAX];
      for (int k = 0; k < ntri; ++k) tri[k] = sm[(long)(d.p + k) * n + it];
      if (!import_chol(tri, q, A))
        return "import: K of " + where(i, it) + ", columns " + std::to_string(d.p) + " .. " + std::to_string(d.p + ntri - 1) +
               " is not positive definite (its " + std::to_string(q) + " x " + std::to_string(q) +
               " Cholesky met a pivot that is not > 0)";
    }
  }
  return "";
}

}  // namespace mk
