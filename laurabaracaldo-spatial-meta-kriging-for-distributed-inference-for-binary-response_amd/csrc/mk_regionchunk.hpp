// The chunk plan of the areal prediction's interpolated route (include/mk.h "areal prediction"): the kept
// window is cut into chunks of B consecutive states, and inside a chunk every (subset, outcome) pair is cut
// into phi runs -- consecutive states with the same phi_h share one factor per region.  A run that crosses a
// chunk boundary is factored again in the next chunk, so a chunk only reads factors of its own launch.
// Standard headers only, so the plan is tested on the host (tests/regionchunk_test.cpp).
#pragma once
#include <algorithm>
#include <vector>

namespace mk {

struct RegionJob {   // one workgroup of the interpolate-and-factor launch
  int pair, region, slot, chunk;
  double phi;
};

struct RegionChunkPlan {
  int B = 0, n = 0, SQ = 0, G = 0, chunks = 0;
  std::vector<int> slot;         // [n][SQ]: the factor slot (0 .. B-1, within the state's chunk) of that state and pair
  std::vector<RegionJob> jobs;   // chunk-major; within a chunk pair-major, then run, then region
  std::vector<long> joff;        // [chunks + 1]: chunk c's jobs are joff[c] .. joff[c + 1]
};

// States per chunk: what `budget` bytes of factor scratch hold at `per_state` bytes per state, or `asked` when
// that is > 0 (MK_REGIONS_CHUNK); at least 1, at most the window.
inline int region_chunk_len(double budget, double per_state, int n, int asked) {
  double b = asked > 0 ? (double)asked : (per_state > 0.0 ? budget / per_state : (double)n);
  if (!(b >= 1.0)) b = 1.0;
  if (b > (double)std::max(n, 1)) b = (double)std::max(n, 1);
  return (int)b;
}

// phi [n][SQ]: the window's phi per state and pair.  Equal means bit-equal, the replay's own rule for a
// refresh.
inline RegionChunkPlan region_chunk_plan(const double* phi, int n, int SQ, int G, int B) {
  RegionChunkPlan p;
  p.B = std::max(1, std::min(B, std::max(n, 1)));
  p.n = n;
  p.SQ = SQ;
  p.G = G;
  p.chunks = (n + p.B - 1) / p.B;
  p.slot.assign((size_t)std::max(n, 0) * SQ, 0);
  p.joff.assign((size_t)p.chunks + 1, 0);
  for (int c = 0; c < p.chunks; ++c) {
    const int j0 = c * p.B, j1 = std::min(n, j0 + p.B);
    for (int i = 0; i < SQ; ++i) {
      int run = -1;
      for (int j = j0; j < j1; ++j) {
        const double v = phi[(size_t)j * SQ + i];
        if (j == j0 || v != phi[(size_t)(j - 1) * SQ + i]) {
          ++run;
          for (int g = 0; g < G; ++g) p.jobs.push_back(RegionJob{i, g, run, c, v});
        }
        p.slot[(size_t)j * SQ + i] = run;
      }
    }
    p.joff[(size_t)c + 1] = (long)p.jobs.size();
  }
  return p;
}

}  // namespace mk
