// Empirical (cross-)variograms of all pairs of n sites (include/mk.h "empirical variogram"): a stand-alone
// verb like mk_glm_binomial, on the other side of the fit from the result sinks -- no session, no schedule.
//
// k_vg_pairs walks the tiles of the strict upper triangle of the n x n pair matrix (VG_EDGE x VG_EDGE sites,
// mk_variogramspec.hpp).  The tiles are dealt u -> workgroup u mod G with G = min(tiles, VG_MAXWG): fixed by
// n alone, never by the CU count or the occupancy.  Inside a workgroup each lane owns one row i of the tile
// and visits the tile's columns j in order; what it adds goes into a histogram of its own in LDS, laid out
// [slot][lane]: a wave's lanes are on distinct banks whatever bins they hit (the slot stride is a multiple
// of the bank row) and no two lanes share an address, so there is no atomic of any kind and the order of a
// lane's additions is the order of its (tile, column) visits.  After its last tile the workgroup folds the
// lanes in lane order, one thread per slot, and writes its partial [n_bins][2 + T] to HBM; k_vg_reduce adds
// the partials in workgroup order.  Which workgroup ran when changes nothing: two calls give the same bytes.
//
// The histograms are the price: W lanes x n_bins x (4 + 8 slots) bytes.  vg_plan takes the widest workgroup
// that fits the CU's 160 KiB, with all T outcome pairs in one pass (a count and 1 + T slots) or, when T n_bins
// is large, split: one pass for the counts and the distance sums (a count and one slot) and one per outcome
// pair (one slot; the distance is recomputed), whichever costs fewer LDS updates per pair and lane.  15
// bins, q = 1: 256 lanes x 300 B = 75 KiB, so two workgroups share a CU (the columns are staged VG_CHUNK
// at a time to leave room for that).  Counts are int32 per lane (a lane sees at most
// tiles-per-workgroup x 1,024 pairs, below 2^31 for every n <= VG_MAXN) and int64 from the fold on.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "mk_session.hpp"
#include "mk_variogramspec.hpp"

namespace mk {

constexpr int VG_UNROLL = 4;   // columns in flight per lane; divides VG_CHUNK
static_assert(VG_CHUNK % VG_UNROLL == 0, "the unrolled column loop reads whole groups of the staged chunk");

// TQ >= 1: q = TQ, the counts, the distance sums and all T pairs of outcomes in one pass.  TQ = 0, a split
// pass: pt < 0 the counts and the distance sums; pt >= 0 the outcome pair (pa, pb), plane pt of the T.
// blockDim.x = W in {64, 128, 256}; grid G.  Dynamic LDS: colxy [VG_CHUNK] double2, colz [VG_CHUNK][q],
// hd [n_bins][slots][W] double, and where the pass counts hc [n_bins][W] int.
// partial: [G][n_bins][2 + T] 8-byte words: the count (int64), the distance sum, the T product sums.
template <int TQ>
__global__ __launch_bounds__(256) void k_vg_pairs(const double* __restrict__ cx, const double* __restrict__ cy,
                                                  const double* __restrict__ z, long n, int q, int n_bins, double s,
                                                  long nt, long n_tiles, int pa, int pb, int pt, int T,
                                                  double* __restrict__ partial) {
  constexpr int TT = TQ * (TQ + 1) / 2;
  constexpr int SL = 1 + TT;                                // TQ = 0: the pass's one slot
  extern __shared__ __align__(16) double vg_lds[];
  const int W = blockDim.x, tid = threadIdx.x, G = gridDim.x;
  d2* colxy = (d2*)vg_lds;
  double* colz = vg_lds + 2 * VG_CHUNK;
  double* hd = colz + VG_CHUNK * q;
  int* hc = (int*)(hd + (long)n_bins * SL * W);
  for (int e = tid; e < n_bins * SL * W; e += W) hd[e] = 0.0;
  const bool counts = TQ > 0 || pt < 0;
  if (counts)
    for (int e = tid; e < n_bins * W; e += W) hc[e] = 0;
  const double nb = (double)n_bins;
  for (long u = blockIdx.x; u < n_tiles; u += G) {
    int I, J;
    vg_tile(u, nt, &I, &J);
    const long i0 = (long)I * VG_EDGE, j0 = (long)J * VG_EDGE;
    for (int c0 = 0; c0 < VG_EDGE; c0 += VG_CHUNK) {
      const long jc = j0 + c0;
      if (jc >= n) break;                                   // uniform: the ragged last tile's empty chunk
      const int nc = (int)((n - jc) < VG_CHUNK ? (n - jc) : VG_CHUNK);
      __syncthreads();                                      // the last chunk's readers are done
      for (int t = tid; t < nc; t += W) {
        d2 c;
        c.x = cx[jc + t];
        c.y = cy[jc + t];
        colxy[t] = c;
        for (int a = 0; a < q; ++a) colz[t * q + a] = z[(jc + t) * q + a];
      }
      __syncthreads();
      for (int r = tid; r < VG_EDGE; r += W) {
        const long i = i0 + r;
        if (i >= n) continue;
        // columns of this chunk with j > i: jj > i - jc (diagonal tiles; everything elsewhere, as J > I)
        const long lo = vg_first_col(i, jc);
        if (lo >= nc) continue;
        const int jlo = (int)lo;
        const double xi = cx[i], yi = cy[i];
        double zi[TQ > 0 ? TQ : 2];
        if (TQ > 0) {
#pragma unroll
          for (int a = 0; a < TQ; ++a) zi[a] = z[i * TQ + a];
        } else {
          zi[0] = z[i * q + pa];
          zi[1] = z[i * q + pb];
        }
        // VG_UNROLL columns at a time: their distances first (independent chains hide the square root's
        // latency), then their updates in column order, so a lane's additions keep the order of its visits
        for (int j4 = 0; j4 < nc; j4 += VG_UNROLL) {
          double d[VG_UNROLL], ks[VG_UNROLL];
#pragma unroll
          for (int v = 0; v < VG_UNROLL; ++v) {
            const int jj = j4 + v;                          // < VG_CHUNK: columns >= nc are staged-over leftovers, masked
            const d2 c = colxy[jj];
            const double dx = xi - c.x, dy = yi - c.y;
            d[v] = sqrt(dx * dx + dy * dy);                 // dist2d's expression
            ks[v] = (jj >= jlo && jj < nc) ? d[v] * s : nb;
          }
#pragma unroll
          for (int v = 0; v < VG_UNROLL; ++v) {
            if (!(ks[v] < nb)) continue;
            const int jj = j4 + v, k = (int)ks[v];
            double* h = hd + (long)k * SL * W + tid;
            if (TQ > 0) {
              hc[k * W + tid] += 1;
              h[0] += d[v];
              double dz[TQ > 0 ? TQ : 1];
#pragma unroll
              for (int a = 0; a < TQ; ++a) dz[a] = zi[a] - colz[jj * TQ + a];
              int t = 0;
#pragma unroll
              for (int b = 0; b < TQ; ++b)
#pragma unroll
                for (int a = b; a < TQ; ++a, ++t) h[(1 + t) * W] += dz[a] * dz[b];
            } else if (pt < 0) {
              hc[k * W + tid] += 1;
              h[0] += d[v];
            } else {
              const double da = zi[0] - colz[jj * q + pa], db = zi[1] - colz[jj * q + pb];
              h[0] += da * db;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  // the lanes in lane order, one thread per slot
  double* out = partial + (long)blockIdx.x * n_bins * (2 + T);
  for (int e = tid; e < n_bins * SL; e += W) {
    const int k = e / SL, c = e % SL;
    const double* h = hd + (long)e * W;
    double acc = 0.0;
    for (int l = 0; l < W; ++l) acc += h[l];
    out[k * (2 + T) + (TQ > 0 ? 1 + c : (pt < 0 ? 1 : 2 + pt))] = acc;
  }
  if (counts)
    for (int k = tid; k < n_bins; k += W) {
      long long acc = 0;
      for (int l = 0; l < W; ++l) acc += hc[k * W + l];
      ((long long*)out)[k * (2 + T)] = acc;
    }
}

// One thread per word e of [n_bins][2 + T]: the G partials in workgroup order.
__global__ __launch_bounds__(256) void k_vg_reduce(const double* __restrict__ partial, int G, int words, int stride,
                                                   double* __restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= words) return;
  if (e % stride == 0) {
    long long acc = 0;
    for (int g = 0; g < G; ++g) acc += ((const long long*)partial)[(long)g * words + e];
    ((long long*)out)[e] = acc;
  } else {
    double acc = 0.0;
    for (int g = 0; g < G; ++g) acc += partial[(long)g * words + e];
    out[e] = acc;
  }
}

typedef void (*vg_kernel_t)(const double*, const double*, const double*, long, int, int, double, long, long, int, int,
                            int, int, double*);
static vg_kernel_t vg_kernel(int tq) {
  switch (tq) {
    case 1: return k_vg_pairs<1>;
    case 2: return k_vg_pairs<2>;
    case 3: return k_vg_pairs<3>;
    case 4: return k_vg_pairs<4>;
    default: return k_vg_pairs<0>;
  }
}

}  // namespace mk

using namespace mk;

extern "C" int32_t mk_variogram_tile_edge(void) { return VG_EDGE; }

extern "C" int mk_variogram_compute(const double* coords, int64_t n, const double* z, int32_t q, int32_t n_bins,
                                    double max_dist, mk_variogram* out, int32_t device) {
  if (!out) return set_err(MK_E_ARG, "variogram: null out");
  const std::string bad = vg_check(coords, (long)n, z, q, n_bins, max_dist, out->count, out->dist, out->gamma);
  if (!bad.empty()) return set_err(MK_E_ARG, bad);
  const double s = (double)n_bins / max_dist;
  const VgPlan p = vg_plan((long)n, q, n_bins);
  const int words = n_bins * (2 + p.T);
  MK_ENTRY_DEVICE(device);
  DevBufs bufs;
  double* d_c = bufs.get<double>((size_t)2 * n);
  double* d_z = bufs.get<double>((size_t)n * q);
  double* d_part = bufs.get<double>((size_t)p.G * words);
  double* d_out = bufs.get<double>((size_t)words);
  if (!d_c || !d_z || !d_part || !d_out) return set_err(MK_E_NOMEM, "variogram buffers");
  HIPCHK(hipMemcpy(d_c, coords, (size_t)2 * n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_z, z, (size_t)n * q * 8, hipMemcpyHostToDevice));
  const vg_kernel_t fn = vg_kernel(p.split ? 0 : q);
  HIPCHK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)std::max(p.lds, p.lds0)));
  const hipStream_t st = (hipStream_t)0;
  EventTimer timer;
  int rc = timer.start(st);
  if (rc) return rc;
  for (int t = 0; t < p.passes; ++t) {
    int a = 0, b = 0;                                       // split: pass 0 counts, pass 1 + t is outcome pair t
    if (p.split && t > 0) vg_pair(t - 1, q, &a, &b);
    hipLaunchKernelGGL(fn, dim3((unsigned)p.G), dim3((unsigned)(t ? p.W : p.W0)), t ? p.lds : p.lds0, st,
                       (const double*)d_c, (const double*)(d_c + n), (const double*)d_z, (long)n, (int)q, (int)n_bins, s,
                       p.nt, p.n_tiles, a, b, t - 1, p.T, d_part);
    wd_trace(st, "k_vg_pairs");
  }
  MK_LAUNCH(k_vg_reduce, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, (const double*)d_part, p.G, words,
            2 + p.T, d_out);
  if ((rc = timer.stop(st))) return rc;
  HIPCHK(hipGetLastError());
  std::vector<double> h((size_t)words);
  HIPCHK(hipMemcpy(h.data(), d_out, (size_t)words * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipDeviceSynchronize());
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, timer.a, timer.b));
  out->ms = ms;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int k = 0; k < n_bins; ++k) {
    const double* w = h.data() + (size_t)k * (2 + p.T);
    long long N;
    memcpy(&N, w, 8);
    out->count[k] = (int64_t)N;
    const double dn = (double)N;
    out->dist[k] = N > 0 ? w[1] / dn : nan;
    for (int t = 0; t < p.T; ++t) out->gamma[(size_t)t * n_bins + k] = N > 0 ? w[2 + t] / (2.0 * dn) : nan;
  }
  return 0;
}
