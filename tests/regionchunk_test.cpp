// Host test of the interpolated route's chunk plan (csrc/mk_regionchunk.hpp): the phi runs of every pair inside
// every chunk, the slot table, the job list and the chunk length.  Built by test_regions_cheb_host.py with the
// host compiler and -fsanitize=address,undefined; prints the first failed check and exits 1, else "ok".
#include <cstdio>
#include <vector>
#include "mk_regionchunk.hpp"

static int failed = 0;
#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      std::printf("line %d: %s is false\n", __LINE__, #x); \
      failed = 1;                                           \
    }                                                       \
  } while (0)

// Every state's factor, found through the plan, must be the job of that state's phi: whatever the chunking.
static void check_covers(const mk::RegionChunkPlan& p, const std::vector<double>& phi, int n, int SQ, int G) {
  CHECK((int)p.slot.size() == n * SQ && (int)p.joff.size() == p.chunks + 1 && p.joff.back() == (long)p.jobs.size());
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < SQ; ++i) {
      const int c = j / p.B, sl = p.slot[(size_t)j * SQ + i];
      CHECK(sl >= 0 && sl < p.B);
      for (int g = 0; g < G; ++g) {
        int found = 0;
        for (long k = p.joff[(size_t)c]; k < p.joff[(size_t)c + 1]; ++k) {
          const mk::RegionJob& b = p.jobs[(size_t)k];
          CHECK(b.chunk == c);
          if (b.pair == i && b.region == g && b.slot == sl) {
            ++found;
            CHECK(b.phi == phi[(size_t)j * SQ + i]);
          }
        }
        CHECK(found == 1);
      }
    }
}

int main() {
  using mk::region_chunk_len;
  using mk::region_chunk_plan;
  // 7 states, 2 pairs.  Pair 0: runs 0-2 | 3-4 | 5-6 (a run starts exactly on the boundary of B = 3 and one
  // crosses the boundary at 6 of B = 3); pair 1: one value throughout (it crosses every boundary), except that
  // it returns to an earlier value at state 6, which is a new run.
  const int n = 7, SQ = 2, G = 3;
  const double a = 5.0, b = 6.5, c = 7.25;
  const std::vector<double> phi = {a, c, a, c, a, c, b, c, b, c, a, c, a, b};
  mk::RegionChunkPlan p = region_chunk_plan(phi.data(), n, SQ, G, 3);
  CHECK(p.B == 3 && p.chunks == 3 && p.n == n && p.SQ == SQ && p.G == G);
  // chunk 0: pair 0 one run, pair 1 one run; chunk 1: pair 0 two runs (b b | a), pair 1 one; chunk 2: one each
  CHECK(p.joff == std::vector<long>({0, 2 * G, 5 * G, 7 * G}));
  const int want0[7] = {0, 0, 0, 0, 0, 1, 0}, want1[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < n; ++j) CHECK(p.slot[(size_t)j * SQ] == want0[j] && p.slot[(size_t)j * SQ + 1] == want1[j]);
  CHECK(p.jobs[0].pair == 0 && p.jobs[0].region == 0 && p.jobs[0].slot == 0 && p.jobs[0].phi == a && p.jobs[0].chunk == 0);
  CHECK(p.jobs[(size_t)G].pair == 1 && p.jobs[(size_t)G].phi == c);
  CHECK(p.jobs[(size_t)3 * G].pair == 0 && p.jobs[(size_t)3 * G].slot == 1 && p.jobs[(size_t)3 * G].phi == a);   // chunk 1, second run
  CHECK(p.jobs[(size_t)5 * G].pair == 0 && p.jobs[(size_t)5 * G].phi == a && p.jobs[(size_t)5 * G].slot == 0);   // the crossing run, again
  CHECK(p.jobs[(size_t)6 * G + 2].pair == 1 && p.jobs[(size_t)6 * G + 2].region == 2 && p.jobs[(size_t)6 * G + 2].phi == b);
  for (int B : {1, 2, 3, 4, 6, 7, 8, 100}) {
    const mk::RegionChunkPlan q = region_chunk_plan(phi.data(), n, SQ, G, B);
    CHECK(q.B == (B > n ? n : B) && q.chunks == (n + q.B - 1) / q.B);
    check_covers(q, phi, n, SQ, G);
  }
  // one chunk: the jobs are the runs (pair 0 has 3, pair 1 has 2); chunks of one state: a job per state
  CHECK((long)region_chunk_plan(phi.data(), n, SQ, G, n).jobs.size() == 5L * G);
  CHECK((long)region_chunk_plan(phi.data(), n, SQ, G, 1).jobs.size() == (long)n * SQ * G);
  // degenerate sizes
  CHECK(region_chunk_plan(phi.data(), 1, SQ, G, 0).B == 1);
  CHECK(region_chunk_plan(phi.data(), 0, SQ, G, 5).chunks == 0);
  CHECK(region_chunk_plan(phi.data(), 0, SQ, G, 5).jobs.empty());
  // the chunk length: the budget's share, the override, the clamps
  CHECK(region_chunk_len(1000.0, 100.0, 50, 0) == 10);
  CHECK(region_chunk_len(1000.0, 100.0, 4, 0) == 4);
  CHECK(region_chunk_len(1000.0, 5000.0, 50, 0) == 1);
  CHECK(region_chunk_len(1000.0, 100.0, 50, 7) == 7);
  CHECK(region_chunk_len(1000.0, 100.0, 5, 7) == 5);
  CHECK(region_chunk_len(1000.0, 0.0, 5, 0) == 5);
  CHECK(region_chunk_len(1000.0, 100.0, 50, -3) == 10);
  if (!failed) std::printf("ok\n");
  return failed;
}
