// Host test of the variogram spec (csrc/mk_variogramspec.hpp): every refusal and the index it names, the
// tiles of the triangle dealt exactly once and every unordered pair of sites visited exactly once for n
// around the tile edge, the launch shapes at the sizes where they change.  Built by test_variogram_host.py
// with the host compiler and -fsanitize=address,undefined; prints the first failed check and exits 1, else "ok".
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>
#include "mk_variogramspec.hpp"

static int failed = 0;
#define CHECK(x)                                            \
  do {                                                      \
    if (!(x)) {                                             \
      std::printf("line %d: %s is false\n", __LINE__, #x); \
      failed = 1;                                           \
    }                                                       \
  } while (0)

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

// The kernel's walk over n sites, on the host: the tiles of workgroup g = u mod G, their chunks, rows and
// masked columns.  visits[i * n + j] counts the visits of the pair (i, j).
static bool walk(long n, std::vector<int>* visits) {
  using namespace mk;
  const VgPlan p = vg_plan(n, 1, 15);
  visits->assign((size_t)(n * n), 0);
  std::vector<int> dealt((size_t)(p.nt * p.nt), 0);
  for (int g = 0; g < p.G; ++g)
    for (long u = g; u < p.n_tiles; u += p.G) {
      int I, J;
      vg_tile(u, p.nt, &I, &J);
      if (I < 0 || J < I || J >= p.nt) return false;
      dealt[(size_t)(I * p.nt + J)] += 1;
      for (int c0 = 0; c0 < VG_EDGE; c0 += VG_CHUNK) {
        const long jc = (long)J * VG_EDGE + c0;
        if (jc >= n) break;
        const long nc = n - jc < VG_CHUNK ? n - jc : VG_CHUNK;
        for (int r = 0; r < VG_EDGE; ++r) {
          const long i = (long)I * VG_EDGE + r;
          if (i >= n) continue;
          for (long jj = vg_first_col(i, jc); jj < nc; ++jj) (*visits)[(size_t)(i * n + jc + jj)] += 1;
        }
      }
    }
  for (long I = 0; I < p.nt; ++I)
    for (long J = 0; J < p.nt; ++J)
      if (dealt[(size_t)(I * p.nt + J)] != (J >= I ? 1 : 0)) return false;
  for (long i = 0; i < n; ++i)
    for (long j = 0; j < n; ++j)
      if ((*visits)[(size_t)(i * n + j)] != (j > i ? 1 : 0)) return false;
  return true;
}

int main() {
  using namespace mk;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // the schedule: every tile once, every pair once, no site with itself
  std::vector<int> v;
  const long E = VG_EDGE;
  for (long n : {2L, 3L, (long)VG_CHUNK, (long)VG_CHUNK + 1, E - 1, E, E + 1, 2 * E - 1, 2 * E, 2 * E + 1, 3 * E + 5}) {
    if (!walk(n, &v)) {
      std::printf("walk failed at n = %ld\n", n);
      failed = 1;
    }
  }
  // the tile map on a long triangle: row starts, the last tile, and a full sweep in order
  for (long nt : {1L, 2L, 3L, 7L, 196L, 1954L, 65536L}) {
    int I, J;
    vg_tile(0, nt, &I, &J);
    CHECK(I == 0 && J == 0);
    vg_tile(nt * (nt + 1) / 2 - 1, nt, &I, &J);
    CHECK(I == nt - 1 && J == nt - 1);
    for (long r : {0L, 1L, nt / 3, nt / 2, nt - 2, nt - 1}) {
      if (r < 0 || r >= nt) continue;
      vg_tile(vg_row_start(r, nt), nt, &I, &J);
      CHECK(I == r && J == r);
      vg_tile(vg_row_start(r, nt) + (nt - r) - 1, nt, &I, &J);
      CHECK(I == r && J == nt - 1);
    }
  }
  {
    const long nt = 1954;
    long u = 0;
    bool okay = true;
    for (long i = 0; i < nt && okay; ++i)
      for (long j = i; j < nt; ++j, ++u) {
        int I, J;
        vg_tile(u, nt, &I, &J);
        if (I != i || J != j) {
          okay = false;
          break;
        }
      }
    CHECK(okay && u == nt * (nt + 1) / 2);
  }
  // the number of workgroups is fixed by n alone
  CHECK(vg_plan(2, 1, 15).G == 1 && vg_plan(E + 1, 1, 15).G == 3 && vg_plan(2 * E + 1, 4, 64).G == 6);
  CHECK(vg_plan(500000, 1, 15).G == VG_MAXWG && vg_plan(500000, 3, 64).G == VG_MAXWG);
  CHECK(vg_plan(500000, 1, 15).nt == 1954 && vg_plan(500000, 1, 15).n_tiles == 1954L * 1955L / 2);
  // launch shapes where they change: one pass while it costs no more LDS updates per pair and lane than the
  // split, the widest workgroup that fits
  VgPlan p = vg_plan(1000, 1, 15);
  CHECK(p.W == 256 && p.W0 == 256 && !p.split && p.passes == 1 && p.slots == 2 && p.lds == 128 * 3 * 8 + 256 * 15 * 20);
  CHECK(2 * p.lds <= VG_LDS_BYTES);                       // two workgroups share a CU at gstat's 15 bins
  p = vg_plan(1000, 1, 31);
  CHECK(p.W == 256 && !p.split && p.lds <= VG_LDS_BYTES && p.lds == p.lds0);
  p = vg_plan(1000, 1, 32);                               // one pass would take 128 lanes: 3 x 2 > 2 + 1
  CHECK(p.split && p.passes == 2 && p.W0 == 256 && p.W == 256 && p.slots == 1);
  CHECK(p.lds0 == 128 * 3 * 8 + 256 * 32 * 12 && p.lds == 128 * 3 * 8 + 256 * 32 * 8);
  p = vg_plan(1000, 1, 64);
  CHECK(p.split && p.passes == 2 && p.W0 == 128 && p.W == 256);
  p = vg_plan(1000, 2, 15);
  CHECK(p.W == 256 && !p.split && p.T == 3 && p.slots == 4);
  p = vg_plan(1000, 2, 17);
  CHECK(p.W == 256 && !p.split);
  p = vg_plan(1000, 2, 18);
  CHECK(p.split && p.passes == 4 && p.W0 == 256 && p.W == 256);
  p = vg_plan(1000, 3, 10);
  CHECK(p.W == 256 && !p.split && p.T == 6 && p.slots == 7);
  p = vg_plan(1000, 3, 11);
  CHECK(p.split && p.passes == 7);
  p = vg_plan(1000, 3, 64);
  CHECK(p.split && p.passes == 7 && p.W0 == 128 && p.W == 256 && p.slots == 1);
  p = vg_plan(1000, 4, 6);
  CHECK(p.W == 256 && !p.split && p.T == 10 && p.slots == 11);
  p = vg_plan(1000, 4, 7);
  CHECK(p.split && p.passes == 11 && p.W0 == 256);
  p = vg_plan(1000, 4, 64);
  CHECK(p.split && p.passes == 11 && p.W0 == 128 && p.W == 256);
  for (int q = 1; q <= VG_MAXQ; ++q)
    for (int nb = 1; nb <= VG_MAXBINS; ++nb) {
      p = vg_plan(1000, q, nb);
      const bool fits = p.W >= 64 && p.W <= 256 && p.W0 >= 64 && p.W0 <= 256 && p.lds <= VG_LDS_BYTES && p.lds0 <= VG_LDS_BYTES;
      const bool shaped = p.split ? (p.passes == 1 + p.T && p.slots == 1 && p.lds == vg_lds_bytes(p.W, nb, q, 1, false) &&
                                     p.lds0 == vg_lds_bytes(p.W0, nb, q, 1, true))
                                  : (p.passes == 1 && p.slots == 1 + p.T && p.W == p.W0 && p.lds == p.lds0 &&
                                     p.lds == vg_lds_bytes(p.W, nb, q, 1 + p.T, true));
      if (!fits || !shaped) {
        std::printf("no plan at q = %d, n_bins = %d\n", q, nb);
        failed = 1;
      }
    }
  // outcome pairs: the lower triangle column by column
  int a, b;
  const int want3[6][2] = {{0, 0}, {1, 0}, {2, 0}, {1, 1}, {2, 1}, {2, 2}};
  for (int t = 0; t < 6; ++t) {
    vg_pair(t, 3, &a, &b);
    CHECK(a == want3[t][0] && b == want3[t][1]);
  }
  vg_pair(9, 4, &a, &b);
  CHECK(a == 3 && b == 3);
  vg_pair(0, 1, &a, &b);
  CHECK(a == 0 && b == 0);
  // refusals
  double c[6] = {0.0, 1.0, 2.0, 0.0, 0.5, 1.0};           // 3 sites, column-major
  double z[6] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0};
  long cnt[4];
  double d[4], gm[12];
  CHECK(vg_check(c, 3, z, 1, 4, 1.0, cnt, d, gm).empty() && vg_check(c, 3, z, 2, 4, 1.0, cnt, d, gm).empty());
  CHECK(vg_check(c, 2, z, 1, 1, 1.0, cnt, d, gm).empty() && vg_check(c, 3, z, 1, 64, 1e-300, cnt, d, gm).empty());
  CHECK(has(vg_check(nullptr, 3, z, 1, 4, 1.0, cnt, d, gm), "null coords/z"));
  CHECK(has(vg_check(c, 3, nullptr, 1, 4, 1.0, cnt, d, gm), "null coords/z"));
  CHECK(has(vg_check(c, 3, z, 1, 4, 1.0, nullptr, d, gm), "null count/dist/gamma"));
  CHECK(has(vg_check(c, 3, z, 1, 4, 1.0, cnt, nullptr, gm), "null count/dist/gamma"));
  CHECK(has(vg_check(c, 3, z, 1, 4, 1.0, cnt, d, nullptr), "null count/dist/gamma"));
  CHECK(has(vg_check(c, 1, z, 1, 4, 1.0, cnt, d, gm), "n = 1 sites"));
  CHECK(has(vg_check(c, 0, z, 1, 4, 1.0, cnt, d, gm), "n = 0 sites"));
  CHECK(has(vg_check(c, VG_MAXN + 1, z, 1, 4, 1.0, cnt, d, gm), "is above 16777216"));
  CHECK(has(vg_check(c, 3, z, 0, 4, 1.0, cnt, d, gm), "q = 0 is outside 1 .. 4"));
  CHECK(has(vg_check(c, 3, z, 5, 4, 1.0, cnt, d, gm), "q = 5 is outside 1 .. 4"));
  CHECK(has(vg_check(c, 3, z, 1, 0, 1.0, cnt, d, gm), "n_bins = 0 is outside 1 .. 64"));
  CHECK(has(vg_check(c, 3, z, 1, 65, 1.0, cnt, d, gm), "n_bins = 65 is outside 1 .. 64"));
  CHECK(has(vg_check(c, 3, z, 1, 4, 0.0, cnt, d, gm), "max_dist = 0"));
  CHECK(has(vg_check(c, 3, z, 1, 4, -1.0, cnt, d, gm), "max_dist = -1"));
  CHECK(has(vg_check(c, 3, z, 1, 4, nan, cnt, d, gm), "max_dist = "));
  CHECK(has(vg_check(c, 3, z, 1, 4, inf, cnt, d, gm), "max_dist = inf"));
  c[4] = nan;                                             // site 1, column 1; a later bad z is not the first
  z[5] = inf;
  CHECK(has(vg_check(c, 3, z, 2, 4, 1.0, cnt, d, gm), "coordinate 4 (site 1, column 1)"));
  c[4] = 0.5;
  CHECK(has(vg_check(c, 3, z, 2, 4, 1.0, cnt, d, gm), "z value 5 (site 2, outcome 1) is inf"));
  z[1] = -inf;
  CHECK(has(vg_check(c, 3, z, 2, 4, 1.0, cnt, d, gm), "z value 1 (site 0, outcome 1) is -inf"));
  CHECK(has(vg_check(c, 3, z, 1, 4, 1.0, cnt, d, gm), "z value 1 (site 1, outcome 0)"));
  if (!failed) std::printf("ok\n");
  return failed;
}
