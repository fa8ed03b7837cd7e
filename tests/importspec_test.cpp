// Host test of the import's checks (csrc/mk_importspec.hpp): every refusal and the subset, iteration and column
// or row it names, a valid chain, and the C ABI's struct and prototypes as include/mk.h declares them (checked
// by the compiler: nothing of libmk is linked).  Built by test_import_host.py with the host compiler and
// -fsanitize=address,undefined; prints the first failed check and exits 1, else "ok".
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>
#include "mk_importspec.hpp"
#include "mk.h"

static int failed = 0;
#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      std::printf("line %d: %s is false\n", __LINE__, #x); \
      failed = 1;                                           \
    }                                                       \
  } while (0)

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// the C ABI: field order and types of mk_chain, the three prototypes
static_assert(offsetof(mk_chain, samples) == 0 && offsetof(mk_chain, w_samples) == sizeof(void*), "mk_chain layout");
static_assert(offsetof(mk_chain, n_w) == 2 * sizeof(void*) && offsetof(mk_chain, acceptance) == 3 * sizeof(void*),
              "mk_chain layout");
static_assert(std::is_same<decltype(mk_chain::samples), const double*>::value, "samples");
static_assert(std::is_same<decltype(mk_chain::w_samples), const double*>::value, "w_samples");
static_assert(std::is_same<decltype(mk_chain::n_w), int32_t>::value, "n_w");
static_assert(std::is_same<decltype(mk_chain::acceptance), const double*>::value, "acceptance");
static_assert(std::is_same<decltype(&mk_session_import_chain), int (*)(mk_session*, const mk_chain*)>::value, "import_chain");
static_assert(std::is_same<decltype(&mk_session_imported), int32_t (*)(const mk_session*)>::value, "imported");
static_assert(std::is_same<decltype(&mk_session_import_stats), int (*)(const mk_session*, int64_t*, double*, double*)>::value,
              "import_stats");

// A chain of S subsets: n iterations, q outcomes, p covariates; K = diag-dominant, phi inside (3, 9), nu inside
// (0.2, 2).  samples per subset n x P column-major, w per subset (n_s q) x n_w column-major.
struct Chain {
  mk::ImportDims d;
  std::vector<int> n_part;
  std::vector<double> samples, w;
  int n_w;
  double& at(int i, int it, int c) { return samples[((size_t)i * d.P() + c) * d.n_samples + it]; }
  double& w_at(int i, int j, int r) {
    size_t off = 0;
    for (int k = 0; k < i; ++k) off += (size_t)n_part[k] * d.q * n_w;
    return w[off + (size_t)j * n_part[i] * d.q + r];
  }
};

static Chain make(int q, bool matern, int n_w, bool record_w = false) {
  Chain c;
  c.n_part = {5, 3};
  c.d.S = 2;
  c.d.subset_base = 10;
  c.d.q = q;
  c.d.p = 2;
  c.d.n_samples = 8;
  c.d.kept0 = 4;          // burn_in = 5: iterations 5 .. 8 (1-based) are kept
  c.d.matern = matern;
  c.d.record_w = record_w;
  for (int h = 0; h < q; ++h) {
    c.d.phi_a[h] = 3.0;
    c.d.phi_b[h] = 9.0;
    c.d.nu_a[h] = 0.2;
    c.d.nu_b[h] = 2.0;
  }
  c.n_w = n_w;
  const int P = c.d.P(), n = c.d.n_samples, ntri = c.d.ntri();
  c.samples.assign((size_t)2 * n * P, 0.0);
  for (int i = 0; i < 2; ++i)
    for (int it = 0; it < n; ++it) {
      for (int j = 0; j < c.d.p; ++j) c.at(i, it, j) = 0.1 * j - 0.01 * it;
      int k = 0;
      for (int a = 0; a < q; ++a)
        for (int b = a; b < q; ++b, ++k) c.at(i, it, c.d.p + k) = (a == b) ? 1.0 + 0.1 * a : 0.2;
      for (int h = 0; h < q; ++h) {
        c.at(i, it, c.d.p + ntri + h) = 4.0 + 0.5 * h + 0.1 * it;
        if (matern) c.at(i, it, c.d.p + ntri + q + h) = 0.5 + 0.05 * it;
      }
    }
  size_t nw = 0;
  for (int ns : c.n_part) nw += (size_t)ns * q * n_w;
  c.w.assign(nw, 0.25);
  c.d.n_part = nullptr;   // set by check(): the vector may have moved
  return c;
}

static std::string check(Chain& c) {
  c.d.n_part = c.n_part.data();
  return mk::import_chain_check(c.d, c.samples.data(), c.w.data(), c.n_w);
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // ---- the session's side
  CHECK(mk::import_session_check(true, 0, false, false, false).empty());
  CHECK(has(mk::import_session_check(false, 0, false, false, false), "keeps no chain states (fused kriging)"));
  CHECK(has(mk::import_session_check(true, 3, false, false, false), "has run 3 iterations"));
  CHECK(has(mk::import_session_check(true, 40, true, false, false), "already holds an imported chain"));
  CHECK(has(mk::import_session_check(true, 0, false, true, false), "unusable after an earlier failure"));
  CHECK(has(mk::import_session_check(true, 0, false, false, true), "in-chain criteria"));
  // ---- valid chains: q = 1, q = 3, Matern, the kept columns of w alone and all of them
  for (int q : {1, 3})
    for (bool matern : {false, true})
      for (int n_w : {4, 6, 8}) {
        Chain c = make(q, matern, n_w);
        CHECK(check(c).empty());
      }
  {
    Chain c = make(2, false, 8, true);
    CHECK(check(c).empty());
  }
  // ---- pointers and n_w
  {
    Chain c = make(1, false, 4);
    c.d.n_part = c.n_part.data();
    CHECK(has(mk::import_chain_check(c.d, nullptr, c.w.data(), 4), "null samples"));
    CHECK(has(mk::import_chain_check(c.d, c.samples.data(), nullptr, 4), "null w_samples"));
    CHECK(has(mk::import_chain_check(c.d, c.samples.data(), c.w.data(), 3), "n_w = 3 is outside kept .. n_samples = 4 .. 8"));
    CHECK(has(mk::import_chain_check(c.d, c.samples.data(), c.w.data(), 9), "n_w = 9 is outside"));
    c.d.record_w = true;
    CHECK(has(mk::import_chain_check(c.d, c.samples.data(), c.w.data(), 4), "n_w = 4 must be n_samples = 8"));
  }
  // ---- values that are not finite: samples anywhere (burn-in rows too), w in the supplied columns
  {
    Chain c = make(2, false, 6);
    c.at(1, 2, 3) = nan;
    CHECK(has(check(c), "samples of subset 11, iteration 3, column 3 is nan"));
    c.at(1, 2, 3) = 1.0;
    c.at(0, 7, 0) = inf;
    CHECK(has(check(c), "samples of subset 10, iteration 8, column 0 is inf"));
    c.at(0, 7, 0) = 0.0;
    c.w_at(1, 0, 4) = nan;          // column 0 of 6: iteration 8 - 6 + 0 + 1 = 3
    CHECK(has(check(c), "w_samples of subset 11, iteration 3, row 4 is nan"));
    c.w_at(1, 0, 4) = 0.0;
    c.w_at(0, 5, 9) = -inf;
    CHECK(has(check(c), "w_samples of subset 10, iteration 8, row 9 is -inf"));
  }
  // ---- phi and nu strictly inside their priors, kept rows only
  {
    Chain c = make(2, true, 4);
    const int cphi = c.d.p + c.d.ntri(), cnu = cphi + 2;
    c.at(0, 1, cphi) = 9.0;           // a burn-in row: not read
    CHECK(check(c).empty());
    c.at(1, 6, cphi + 1) = 9.0;       // phi_b itself
    CHECK(has(check(c), "phi of subset 11, iteration 7, column 6 (outcome 1) is 9.0"));
    CHECK(has(check(c), "not strictly inside its prior (3.0"));
    c.at(1, 6, cphi + 1) = 3.0;
    CHECK(has(check(c), "phi of subset 11, iteration 7, column 6"));
    c.at(1, 6, cphi + 1) = 5.0;
    c.at(0, 4, cnu) = 2.0;
    CHECK(has(check(c), "nu of subset 10, iteration 5, column 7 (outcome 0) is 2.0"));
    c.at(0, 4, cnu) = 0.1;
    CHECK(has(check(c), "nu of subset 10, iteration 5, column 7"));
  }
  // ---- K positive definite, kept rows only
  {
    Chain c = make(2, false, 4);
    c.at(0, 0, c.d.p + 1) = 5.0;      // a burn-in row
    CHECK(check(c).empty());
    c.at(1, 5, c.d.p + 1) = 5.0;      // K = [1 5; 5 1.1]: an eigenvalue below zero
    CHECK(has(check(c), "K of subset 11, iteration 6, columns 2 .. 4 is not positive definite"));
    c.at(1, 5, c.d.p + 1) = 0.2;
    c.at(0, 7, c.d.p) = 0.0;          // a zero pivot
    CHECK(has(check(c), "K of subset 10, iteration 8, columns 2 .. 4 is not positive definite"));
    Chain one = make(1, false, 4);
    one.at(0, 4, one.d.p) = -1.0;
    CHECK(has(check(one), "K of subset 10, iteration 5, columns 2 .. 2 is not positive definite"));
  }
  // ---- the factor itself: A A' = K, positive diagonal
  {
    const double tri[6] = {4.0, 2.0, 0.4, 3.0, 0.5, 2.0};
    double A[9];
    CHECK(mk::import_chol(tri, 3, A));
    CHECK(A[0] == 2.0 && A[1] == 1.0 && A[2] == 0.2 && A[3] == 0.0 && A[6] == 0.0 && A[7] == 0.0);
    CHECK(A[4] > 0.0 && A[8] > 0.0);
    CHECK(std::fabs(A[1] * A[1] + A[4] * A[4] - 3.0) < 1e-15 && std::fabs(A[2] * A[1] + A[5] * A[4] - 0.5) < 1e-15);
    CHECK(std::fabs(A[2] * A[2] + A[5] * A[5] + A[8] * A[8] - 2.0) < 1e-15);
  }
  if (!failed) std::printf("ok\n");
  return failed;
}
