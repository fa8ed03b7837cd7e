// Host test of the region spec (csrc/mk_regionspec.hpp): every refusal and the index it names, the normalised
// weights and the packed factor offsets.  Built by test_regions_host.py with the host compiler and
// -fsanitize=address,undefined; prints the first failed check and exits 1, else "ok".
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>
#include "mk_regionspec.hpp"

static int failed = 0;
#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      std::printf("line %d: %s is false\n", __LINE__, #x); \
      failed = 1;                                           \
    }                                                       \
  } while (0)

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main() {
  using mk::RegionPlan;
  using mk::region_plan;
  using mk::region_thresholds_check;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // a good spec: 7 sites in regions of 2, 1 and 4
  const int off[4] = {0, 2, 3, 7};
  const double w[7] = {1.0, 3.0, 5.0, 2.0, 0.0, 2.0, 4.0};
  const double cx[7] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7}, cy[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  RegionPlan p;
  CHECK(region_plan(3, off, 7, w, cx, cy, &p).empty());
  CHECK(p.G == 3 && p.n_test == 7 && p.maxm == 4);
  CHECK(p.offsets == std::vector<int>({0, 2, 3, 7}));
  CHECK(p.foff == std::vector<long>({0, 4, 5, 21}));            // 2^2, 1^2, 4^2
  CHECK(p.omega[0] == 0.25 && p.omega[1] == 0.75 && p.omega[2] == 1.0);
  CHECK(p.omega[3] == 0.25 && p.omega[4] == 0.0 && p.omega[5] == 0.25 && p.omega[6] == 0.5);
  // no weights: equal within the region, added in index order
  RegionPlan e;
  CHECK(region_plan(3, off, 7, nullptr, nullptr, nullptr, &e).empty());
  CHECK(e.omega[0] == 0.5 && e.omega[2] == 1.0 && e.omega[6] == 0.25);
  // the largest region allowed, and one site more
  std::vector<double> ones(129, 1.0);
  const int big[2] = {0, 128}, too_big[2] = {0, 129};
  RegionPlan b;
  CHECK(region_plan(1, big, 128, ones.data(), nullptr, nullptr, &b).empty() && b.maxm == 128 && b.foff[1] == 128L * 128L);
  std::string m = region_plan(1, too_big, 129, ones.data(), nullptr, nullptr, &b);
  CHECK(has(m, "region 0 has 129 sites") && has(m, "at most 128"));
  CHECK(b.maxm == 128);                                         // a refusal leaves the plan alone
  // offsets
  RegionPlan x;
  CHECK(has(region_plan(3, off, 0, w, cx, cy, &x), "needs test sites"));
  CHECK(has(region_plan(0, off, 7, w, cx, cy, &x), "n_regions = 0"));
  CHECK(has(region_plan(3, nullptr, 7, w, cx, cy, &x), "needs offsets"));
  const int o1[4] = {1, 2, 3, 7};
  CHECK(has(region_plan(3, o1, 7, w, cx, cy, &x), "offsets[0] = 1 must be 0"));
  const int o2[4] = {0, 3, 3, 7};
  CHECK(has(region_plan(3, o2, 7, w, cx, cy, &x), "offsets[2] = 3 is not above offsets[1] = 3"));
  const int o3[4] = {0, 4, 2, 7};
  CHECK(has(region_plan(3, o3, 7, w, cx, cy, &x), "offsets[2] = 2 is not above offsets[1] = 4"));
  const int o4[4] = {0, 2, 3, 6};
  CHECK(has(region_plan(3, o4, 7, w, cx, cy, &x), "offsets[3] = 6 must be n_test = 7"));
  const int o5[4] = {0, 2, 3, 9};
  CHECK(has(region_plan(3, o5, 7, w, cx, cy, &x), "offsets[3] = 9 is past the 7 test sites"));
  // weights
  double wb[7] = {1.0, 3.0, 5.0, 2.0, nan, 2.0, 4.0};
  CHECK(has(region_plan(3, off, 7, wb, cx, cy, &x), "weight 4 is"));
  wb[4] = -1.0;
  CHECK(has(region_plan(3, off, 7, wb, cx, cy, &x), "weight 4 is -1"));
  wb[4] = inf;
  CHECK(has(region_plan(3, off, 7, wb, cx, cy, &x), "weight 4 is inf"));
  const double wz[7] = {1.0, 3.0, 0.0, 2.0, 0.0, 2.0, 4.0};
  CHECK(has(region_plan(3, off, 7, wz, cx, cy, &x), "the weights of region 1 sum to 0"));
  // two sites of one region at the same place (sites 3 and 5); the same pair in different regions is fine
  double dx[7] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.4, 0.7};
  CHECK(has(region_plan(3, off, 7, w, dx, cy, &x), "test sites 3 and 5 of region 2 have identical coordinates"));
  dx[5] = 0.6;
  dx[2] = 0.1;                                                   // site 2 (region 1) on site 0 (region 0)
  CHECK(region_plan(3, off, 7, w, dx, cy, &x).empty());
  // thresholds
  const double u[3] = {0.2, nan, 0.5};
  CHECK(region_thresholds_check(u, 1).empty() && region_thresholds_check(nullptr, 0).empty());
  CHECK(has(region_thresholds_check(u, 3), "threshold 1 is"));
  CHECK(has(region_thresholds_check(u, 9), "n_thresholds = 9 is outside 0 .. 8"));
  CHECK(has(region_thresholds_check(u, -1), "n_thresholds = -1"));
  CHECK(has(region_thresholds_check(nullptr, 2), "null thresholds"));
  if (!failed) std::printf("ok\n");
  return failed;
}
