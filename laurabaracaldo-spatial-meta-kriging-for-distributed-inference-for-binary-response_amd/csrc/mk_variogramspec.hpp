// The empirical variogram (include/mk.h "empirical variogram") checked and scheduled on the host: the
// argument checks of mk_variogram_compute, the tiles of the strict upper triangle of the n x n pair
// matrix and their deal to the workgroups, and the shape of a launch (threads, LDS, passes) for a number
// of bins and outcomes.  Standard headers only, so all of it is tested on the host
// (tests/variogramspec_test.cpp); vg_tile is also what the kernel calls.
#pragma once
#include <cmath>
#include <cstddef>
#include <string>

#ifdef __HIPCC__
#define MK_VG_HD __host__ __device__
#else
#define MK_VG_HD
#endif

namespace mk {

constexpr int VG_MAXBINS = 64;        // MK_VG_MAXBINS
constexpr int VG_MAXQ = 4;            // MK_VG_MAXQ
constexpr int VG_EDGE = 256;          // MK_VG_EDGE: tile edge, rows (one per lane at 256 threads) and columns
constexpr int VG_CHUNK = 128;         // columns of a tile staged in LDS at a time
constexpr int VG_MAXWG = 2048;        // workgroups at most: min(tiles, VG_MAXWG), so fixed by n alone
constexpr long VG_MAXN = 1L << 24;    // sites at most: a lane's int32 counts hold (tiles / VG_MAXWG) x 1,024 pairs
constexpr size_t VG_LDS_BYTES = 160 * 1024;   // LDS of a CU: one workgroup may take all of it

// Tile u of the triangle, in row-major order over the tile rows I = 0 .. nt-1 with J = I .. nt-1: row I
// starts at I nt - I (I - 1) / 2.  The root gives I within one; the two loops settle it.
MK_VG_HD inline long vg_row_start(long I, long nt) { return I * nt - I * (I - 1) / 2; }
MK_VG_HD inline void vg_tile(long u, long nt, int* I, int* J) {
  const double b = 2.0 * (double)nt + 1.0;
  long i = (long)((b - sqrt(b * b - 8.0 * (double)u)) * 0.5);
  if (i < 0) i = 0;
  if (i > nt - 1) i = nt - 1;
  while (i + 1 < nt && vg_row_start(i + 1, nt) <= u) ++i;
  while (i > 0 && vg_row_start(i, nt) > u) --i;
  *I = (int)i;
  *J = (int)(i + (u - vg_row_start(i, nt)));
}

// First column of the chunk starting at site jc that row i pairs with (j > i): 0 off the diagonal tiles,
// where jc > i; at or past the chunk's end when the row has nothing in it.
MK_VG_HD inline long vg_first_col(long i, long jc) { return i - jc + 1 > 0 ? i - jc + 1 : 0; }

// A launch: nt tile rows, n_tiles = nt (nt + 1) / 2 tiles dealt u -> workgroup u mod G.  The T = q (q + 1) / 2
// outcome pairs go either all in one pass (split = 0: W threads, per bin and lane an int32 count and 1 + T
// double slots) or in 1 + T passes (split = 1): pass 0 counts and sums the distances (W0 threads, a count and
// one slot), pass 1 + t sums the products of outcome pair t (W threads, one slot, the distance recomputed).
struct VgPlan {
  long nt = 0, n_tiles = 0;
  int G = 0, W = 0, W0 = 0, split = 0, T = 0, passes = 0, slots = 0;
  size_t lds = 0, lds0 = 0;
};

inline size_t vg_lds_bytes(int W, int n_bins, int q, int slots, bool counts) {
  return (size_t)VG_CHUNK * (2 + q) * 8 + (size_t)W * n_bins * (8 * (size_t)slots + (counts ? 4 : 0));
}

// The widest workgroup (256, 128 or 64 lanes) whose lane-private histograms fit the LDS; 0 when none does.
inline int vg_widest(int n_bins, int q, int slots, bool counts) {
  for (int W = 256; W >= 64; W /= 2)
    if (vg_lds_bytes(W, n_bins, q, slots, counts) <= VG_LDS_BYTES) return W;
  return 0;
}

// The cheaper arrangement by LDS updates per pair x (256 / lanes), summed over the passes: (2 + T) 256 / W
// in one pass, 2 x 256 / W0 + T x 256 / W split; ties go to the single pass.  The updates and the waves that
// hide their latency are what the kernel's time is made of.  Every (n_bins, q) allowed
// has a split plan: at 64 bins pass 0 takes 128 lanes x 64 x 12 B = 96 KiB, the others 256 x 64 x 8 B = 128 KiB.
inline VgPlan vg_plan(long n, int q, int n_bins) {
  VgPlan p;
  p.nt = (n + VG_EDGE - 1) / VG_EDGE;
  p.n_tiles = p.nt * (p.nt + 1) / 2;
  p.G = (int)(p.n_tiles < VG_MAXWG ? p.n_tiles : VG_MAXWG);
  p.T = q * (q + 1) / 2;
  const int Wa = vg_widest(n_bins, q, 1 + p.T, true);
  const int W0 = vg_widest(n_bins, q, 1, true), W1 = vg_widest(n_bins, q, 1, false);
  const int cost_one = Wa ? (2 + p.T) * (256 / Wa) : 0, cost_split = 2 * (256 / W0) + p.T * (256 / W1);
  p.split = !Wa || cost_split < cost_one;
  if (p.split) {
    p.W = W1;
    p.W0 = W0;
    p.slots = 1;
    p.passes = 1 + p.T;
    p.lds = vg_lds_bytes(W1, n_bins, q, 1, false);
    p.lds0 = vg_lds_bytes(W0, n_bins, q, 1, true);
  } else {
    p.W = p.W0 = Wa;
    p.slots = 1 + p.T;
    p.passes = 1;
    p.lds = p.lds0 = vg_lds_bytes(Wa, n_bins, q, 1 + p.T, true);
  }
  return p;
}

// Pair t of the T outcome pairs, a >= b, in the lower-triangle column-major order of A and K.
inline void vg_pair(int t, int q, int* a, int* b) {
  for (int c = 0; c < q; ++c) {
    if (t < q - c) {
      *a = c + t;
      *b = c;
      return;
    }
    t -= q - c;
  }
  *a = *b = -1;
}

// The arguments of mk_variogram_compute: "" when they are fine, else the message (naming the first
// offending index of a value that is not finite).  coords n x 2 column-major, z location-major n x q.
inline std::string vg_check(const double* coords, long n, const double* z, int q, int n_bins, double max_dist,
                            const void* count, const void* dist, const void* gamma) {
  if (!coords || !z) return "variogram: null coords/z";
  if (!count || !dist || !gamma) return "variogram: null count/dist/gamma";
  if (n < 2) return "variogram: n = " + std::to_string(n) + " sites; a pair needs 2";
  if (n > VG_MAXN) return "variogram: n = " + std::to_string(n) + " is above " + std::to_string(VG_MAXN);
  if (q < 1 || q > VG_MAXQ) return "variogram: q = " + std::to_string(q) + " is outside 1 .. " + std::to_string(VG_MAXQ);
  if (n_bins < 1 || n_bins > VG_MAXBINS)
    return "variogram: n_bins = " + std::to_string(n_bins) + " is outside 1 .. " + std::to_string(VG_MAXBINS);
  if (!std::isfinite(max_dist) || !(max_dist > 0.0))
    return "variogram: max_dist = " + std::to_string(max_dist) + " must be finite and > 0";
  for (long i = 0; i < 2 * n; ++i)
    if (!std::isfinite(coords[i]))
      return "variogram: coordinate " + std::to_string(i) + " (site " + std::to_string(i % n) + ", column " +
             std::to_string(i / n) + ") is " + std::to_string(coords[i]) + "; every coordinate must be finite";
  for (long i = 0; i < n * q; ++i)
    if (!std::isfinite(z[i]))
      return "variogram: z value " + std::to_string(i) + " (site " + std::to_string(i / q) + ", outcome " +
             std::to_string(i % q) + ") is " + std::to_string(z[i]) + "; every value must be finite";
  return "";
}

}  // namespace mk
