// Host test of the checkpoints' checks (csrc/mk_checkpointspec.hpp): the layout arithmetic at S = 1 and 4, q = 1 and
// 2, Matern and not, at iteration 0, mid-batch and n.samples; every refusal and what it names; the digest's term and
// the regions' enumeration against sums worked by hand; and the C ABI's struct and prototypes as include/mk.h
// declares them (checked by the compiler: nothing of libmk is linked).  Built by test_checkpoint_host.py with the
// host compiler and -fsanitize=address,undefined; prints the first failed check and exits 1, else "ok".
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>
#include "mk_checkpointspec.hpp"
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

// the C ABI
static_assert(offsetof(mk_checkpoint, field) == 0, "mk_checkpoint layout");
static_assert(offsetof(mk_checkpoint, digests) == MK_CKPT_NFIELDS * sizeof(void*), "mk_checkpoint layout");
static_assert(offsetof(mk_checkpoint, lookahead) == (MK_CKPT_NFIELDS + 1) * sizeof(void*), "mk_checkpoint layout");
static_assert(std::is_same<decltype(mk_checkpoint::digests), uint64_t*>::value, "digests");
static_assert(std::is_same<decltype(mk_checkpoint::lookahead), int32_t>::value, "lookahead");
static_assert(std::is_same<decltype(&mk_session_checkpoint_layout), int (*)(const mk_session*, int32_t, int64_t*)>::value, "layout");
static_assert(std::is_same<decltype(&mk_session_checkpoint), int (*)(mk_session*, int32_t, int32_t, mk_checkpoint*)>::value,
              "checkpoint");
static_assert(std::is_same<decltype(&mk_session_restore), int (*)(mk_session*, int32_t, const int64_t*, const mk_checkpoint*)>::value,
              "restore");
static_assert(std::is_same<decltype(&mk_session_digest), int (*)(mk_session*, uint64_t*)>::value, "digest");
static_assert(std::is_same<decltype(&mk_digest), int (*)(const void*, int64_t, int32_t, uint64_t*)>::value, "mk_digest");
static_assert(MK_CKPT_NFIELDS == 24 && MK_CKPT_NDIGEST == 4, "constants");

using mk::CkptDims;

static CkptDims dims(int S, int q, bool matern, bool tiled, bool record_w, bool criteria) {
  CkptDims d;
  d.S = S;
  d.subset_base = 10;
  d.q = q;
  d.p = 2 * q;
  d.n_pad = 256;
  d.n_samples = 40;
  d.batch_length = 10;
  d.kept0 = 20;
  d.n_test = tiled ? 0 : 7;
  d.matern = matern;
  d.tiled = tiled;
  d.record_w = record_w;
  d.criteria = criteria;
  return d;
}

// A state of the right sizes, every word a small non-negative integer (fine as theta, tune, w and acc alike).
struct State {
  int64_t words[MK_CKPT_NFIELDS];
  std::vector<std::vector<double>> store;
  void* field[MK_CKPT_NFIELDS];
  std::vector<uint64_t> digests;
  State(const CkptDims& d, int iteration) : store(MK_CKPT_NFIELDS) {
    mk::ckpt_layout(d, iteration, words);
    for (int f = 0; f < MK_CKPT_NFIELDS; ++f) {
      store[f].assign((size_t)d.S * words[f], 1.0);
      field[f] = words[f] ? (void*)store[f].data() : nullptr;
    }
    digests.assign((size_t)d.S * d.q * MK_CKPT_NDIGEST, 0);
  }
  double& at(int f, int subset, long j) { return store[f][(size_t)subset * words[f] + j]; }
};

static void test_layout() {
  for (int S : {1, 4})
    for (int q : {1, 2})
      for (bool matern : {false, true})
        for (bool tiled : {false, true})
          for (bool crit : {false, true})
            for (int it : {0, 15, 20, 21, 40}) {
              const CkptDims d = dims(S, q, matern, tiled, tiled, crit);
              int64_t w[MK_CKPT_NFIELDS];
              mk::ckpt_layout(d, it, w);
              const long ntri = q * (q + 1) / 2, nth = ntri + q * (matern ? 2 : 1), P = 2 * q + nth, Np = 256L * q;
              const long k = it > 20 ? it - 20 : 0;
              CHECK(d.n_theta() == nth && d.P() == P && d.Np() == Np && d.kept_done(it) == k);
              CHECK(w[mk::CK_BETA] == 2 * q && w[mk::CK_THETA] == nth && w[mk::CK_W] == Np && w[mk::CK_ETA] == Np);
              CHECK(w[mk::CK_TUNE] == P + Np && w[mk::CK_ACC] == P + Np);
              CHECK(w[mk::CK_U] == 256L * q && w[mk::CK_Z] == 256L * q && w[mk::CK_ZZ] == 256L * q * q);
              CHECK(w[mk::CK_LOGDET] == q && w[mk::CK_QUAD] == q && w[mk::CK_AFULL] == q * q && w[mk::CK_AINV] == q * q);
              CHECK(w[mk::CK_NOTPD] == q);
              CHECK(w[mk::CK_CRIT_ACC] == ((crit && k) ? 6 * Np : 0) && w[mk::CK_CRIT_PART] == (crit ? k * q : 0));
              CHECK(w[mk::CK_CRIT_SBETA] == ((crit && k) ? 2 * q : 0));
              CHECK(w[mk::CK_SAMPLES] == it * P && w[mk::CK_W_SAMPLES] == (tiled ? it * Np : 0));
              CHECK(w[mk::CK_ACC_HIST] == (it / 10) * (P + 1));
              CHECK(w[mk::CK_KZ] == (tiled ? k * 256 * q : 0) && w[mk::CK_KTH] == (tiled ? k * nth : 0));
              CHECK(w[mk::CK_KA] == (tiled ? k * q * q : 0) && w[mk::CK_W_PRED] == (tiled ? 0 : k * q * 7));
              // a checkpoint at iteration 0 moves no row of the record
              if (it == 0)
                for (int f = mk::CK_CRIT_ACC; f < MK_CKPT_NFIELDS; ++f) CHECK(w[f] == 0);
              // a valid state passes, whatever the number of subsets
              State st(d, it);
              CHECK(mk::ckpt_restore_check(d, it, st.words, st.field, st.digests.data()).empty());
            }
  CHECK(std::string(mk::ckpt_field_name(mk::CK_W_PRED)) == "w_pred" && std::string(mk::ckpt_field_name(0)) == "beta");
  CHECK(std::string(mk::ckpt_digest_name(MK_DIGEST_L)) == "L" && std::string(mk::ckpt_digest_name(MK_DIGEST_QB)) == "QB");
  CHECK(std::string(mk::ckpt_digest_name(MK_DIGEST_WINV)) == "Winv" && std::string(mk::ckpt_digest_name(MK_DIGEST_W)) == "W");
}

static void test_session_refusals() {
  CHECK(mk::ckpt_session_check(0, false, false).empty());
  CHECK(has(mk::ckpt_session_check(7, false, false), "has run 7 iterations"));
  CHECK(has(mk::ckpt_session_check(0, true, false), "imported chain"));
  CHECK(has(mk::ckpt_session_check(0, false, true), "unusable"));
  CHECK(mk::ckpt_write_check(false, false, 4, 0, 4).empty() && mk::ckpt_write_check(false, false, 4, 3, 1).empty());
  CHECK(has(mk::ckpt_write_check(true, false, 4, 0, 4), "imported chain") && has(mk::ckpt_write_check(true, false, 4, 0, 4), "save_session"));
  CHECK(has(mk::ckpt_write_check(false, true, 4, 0, 4), "unusable"));
  CHECK(has(mk::ckpt_write_check(false, false, 4, 3, 2), "subsets [3, 5) are outside the session's 4 subsets"));
  CHECK(has(mk::ckpt_write_check(false, false, 4, -1, 2), "outside") && has(mk::ckpt_write_check(false, false, 4, 0, 0), "outside"));
  CHECK(has(mk::ckpt_write_check(false, false, 4, 1, std::numeric_limits<int>::max()), "outside"));
  // the schedule: a state written mid-chain continues on the schedule that wrote it, the ends on the session's own
  for (int ses : {0, 1}) {
    CHECK(mk::ckpt_schedule(1, ses, 25, 40) == 1 && mk::ckpt_schedule(0, ses, 25, 40) == 0);
    CHECK(mk::ckpt_schedule(1, ses, 1, 40) == 1 && mk::ckpt_schedule(0, ses, 39, 40) == 0);
    CHECK(mk::ckpt_schedule(1, ses, 0, 40) == ses && mk::ckpt_schedule(0, ses, 0, 40) == ses);
    CHECK(mk::ckpt_schedule(1, ses, 40, 40) == ses && mk::ckpt_schedule(0, ses, 40, 40) == ses);
    CHECK(mk::ckpt_schedule_check(1, ses, true, 25, 40).empty() && mk::ckpt_schedule_check(0, ses, true, 25, 40).empty());
  }
  // a session of several stream groups runs the sequential schedule alone
  CHECK(mk::ckpt_schedule_check(0, 0, false, 25, 40).empty());
  CHECK(mk::ckpt_schedule_check(1, 0, false, 0, 40).empty() && mk::ckpt_schedule_check(1, 0, false, 40, 40).empty());
  CHECK(has(mk::ckpt_schedule_check(1, 0, false, 25, 40), "written mid-chain (iteration 25) under the lookahead schedule"));
  CHECK(has(mk::ckpt_schedule_check(1, 0, false, 25, 40), "n_streams <= 1"));
}

static void test_state_refusals() {
  const CkptDims d = dims(4, 2, true, true, true, true);
  {
    State st(d, 25);
    CHECK(has(mk::ckpt_restore_check(d, -1, st.words, st.field, st.digests.data()), "iteration -1 is outside 0 .. n.samples = 40"));
    CHECK(has(mk::ckpt_restore_check(d, 41, st.words, st.field, st.digests.data()), "iteration 41 is outside"));
    CHECK(has(mk::ckpt_restore_check(d, 25, nullptr, st.field, st.digests.data()), "null"));
    CHECK(has(mk::ckpt_restore_check(d, 25, st.words, nullptr, st.digests.data()), "null"));
    CHECK(has(mk::ckpt_restore_check(d, 25, st.words, st.field, nullptr), "null digests"));
    // the sizes of another iteration: the first field that differs is named with both sizes
    const std::string m = mk::ckpt_restore_check(d, 26, st.words, st.field, st.digests.data());
    CHECK(has(m, "subsets 10 .. 13") && has(m, "field 'crit_part'") && has(m, "has 10 words per subset") && has(m, "has 12"));
  }
  for (int f = 0; f < MK_CKPT_NFIELDS; ++f) {   // each size, one word off
    State st(d, 25);
    st.words[f] += 1;
    const std::string m = mk::ckpt_restore_check(d, 25, st.words, st.field, st.digests.data());
    CHECK(has(m, (std::string("field '") + mk::ckpt_field_name(f) + "' has " + std::to_string((long long)st.words[f]) + " words").c_str()));
    CHECK(has(m, (" has " + std::to_string((long long)st.words[f] - 1) + " (n_pad 256, q 2)").c_str()));
  }
  {
    State st(d, 25);
    st.field[mk::CK_KZ] = nullptr;
    CHECK(has(mk::ckpt_restore_check(d, 25, st.words, st.field, st.digests.data()), "field 'kz' is null"));
  }
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (int f : {(int)mk::CK_THETA, (int)mk::CK_TUNE, (int)mk::CK_W})
    for (double v : {inf, -inf, nan}) {
      State st(d, 25);
      st.at(f, 2, 3) = v;
      const std::string m = mk::ckpt_restore_check(d, 25, st.words, st.field, st.digests.data());
      CHECK(has(m, (std::string("subset 12, field '") + mk::ckpt_field_name(f) + "', word 3 is ").c_str()) && has(m, "finite"));
    }
  for (double v : {-1.0, 0.5, inf, nan}) {
    State st(d, 25);
    st.at(mk::CK_ACC, 3, st.words[mk::CK_ACC] - 1) = v;
    const std::string m = mk::ckpt_restore_check(d, 25, st.words, st.field, st.digests.data());
    CHECK(has(m, "subset 13, field 'acc', word ") && has(m, "non-negative integer"));
  }
  {   // what is not checked may hold anything: eta is raw bytes
    State st(d, 25);
    st.at(mk::CK_ETA, 0, 0) = nan;
    st.at(mk::CK_ACC, 0, 0) = 0.0;
    st.at(mk::CK_ACC, 1, 1) = 7.0;
    CHECK(mk::ckpt_restore_check(d, 25, st.words, st.field, st.digests.data()).empty());
  }
}

static uint64_t digest_of(const std::vector<uint64_t>& x) {
  uint64_t d = 0;
  for (size_t i = 0; i < x.size(); ++i) d += mk::digest_term(x[i], i);
  return d;
}

static void test_digest() {
  // x = 0: the stream of splitmix64 seeded with 0
  CHECK(mk::digest_term(0, 0) == 0xE220A8397B1DCDAFull && mk::digest_term(0, 1) == 0x6E789E6AA1B965F4ull);
  CHECK(mk::digest_term(0, 2) == 0x06C45D188009454Full);
  CHECK(digest_of({}) == 0 && digest_of({0, 0}) == 0x509946A41CD733A3ull);
  CHECK(digest_of({0x3FF0000000000000ull}) == 0x88D7C35BBBF3EDEDull);
  CHECK(digest_of({~0ull}) == 0xE4D971771B652C20ull);
  CHECK(digest_of({1, 2, 3}) == 0xEDBE5CA3654F5804ull && digest_of({2, 1, 3}) == 0xF32FAC2652772036ull);
  // the regions' enumeration is dense: every word of a region has its own index 0 .. m - 1, in column order
  for (int ns : {1, 2, 127, 129, 255, 300}) {
    const int ld = 384, nt = 3;
    long next = 0;
    for (int j = 0; j < ld; ++j) {
      const mk::DigestCol c = mk::digest_col_tri(j, ns, ld);
      CHECK(c.off == (long)j * ld);
      for (int r = c.r_lo; r < c.r_hi; ++r) CHECK(c.idx0 + r == next++);
    }
    CHECK(next == mk::digest_region_words(MK_DIGEST_L, ns) && next == (long)ns * (ns + 1) / 2);
    for (int full = 0; full < 2; ++full) {
      next = 0;
      for (int j = 0; j < nt * 128; ++j) {
        const mk::DigestCol c = mk::digest_col_tile(j, ns, full);
        CHECK(c.off == (long)(j / 128) * 128 * 128 + (long)(j % 128) * 128);
        CHECK(c.r_hi <= 128 && (c.r_hi <= c.r_lo || (j / 128) * 128 + c.r_hi <= ns));
        for (int r = c.r_lo; r < c.r_hi; ++r) CHECK(c.idx0 + r == next++);
      }
      CHECK(next == mk::digest_region_words(full ? MK_DIGEST_QB : MK_DIGEST_WINV, ns));
    }
  }
  CHECK(mk::digest_region_words(MK_DIGEST_QB, 130) == 2 * 64 * 64 + 4 && mk::digest_region_words(MK_DIGEST_WINV, 130) == 8256 + 3);
  CHECK(mk::digest_region_words(MK_DIGEST_QB, 70) == 64 * 64 + 6 * 6 && mk::digest_region_words(MK_DIGEST_QB, 64) == 64 * 64);
  {   // QB: quadrant 1 of tile 1 at n_s = 200 (m = 72: quadrant 0 whole, quadrant 1 8 x 8), column 66 of the tile
    const mk::DigestCol c = mk::digest_col_tile(128 + 66, 200, 1);
    CHECK(c.r_lo == 64 && c.r_hi == 72 && c.off == 16384 + 66 * 128 && c.idx0 + 64 == 8192 + 4096 + 2 * 8);
    CHECK(mk::digest_col_tile(128 + 72, 200, 1).r_hi == 0 && mk::digest_col_tile(128 + 63, 200, 1).r_hi == 64);
  }
}

int main() {
  test_layout();
  test_session_refusals();
  test_state_refusals();
  test_digest();
  if (!failed) std::printf("ok\n");
  return failed;
}
