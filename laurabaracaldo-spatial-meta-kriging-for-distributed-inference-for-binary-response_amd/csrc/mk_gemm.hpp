// Batched fp64 tile GEMM on CDNA4 MFMA (v_mfma_f64_16x16x4_f64).
//
// One 256-thread workgroup (4 waves, 2x2) owns one TM x TN output tile (TM, TN in {32, 64, 128});
// each wave owns a (TM/2) x (TN/2) quadrant = BM x BN MFMA blocks of 16x16.  K is streamed in
// chunks of 16 straight from HBM into LDS by global_load_lds (LDS-DMA: no staging registers,
// no ds_write pass), two stages deep: chunk c+1 streams in while chunk c is multiplied, one
// barrier per chunk.  128 x 128 kernels stay within 256 registers (__launch_bounds__(256, 2))
// and 2 x 72 KiB of LDS, so two workgroups share a CU and one's waits hide behind the other's
// MFMAs.
//
// Tile shape and bits: every output element accumulates the same MFMA sequence -- the same
// 16-deep chunks in the same order, four k-steps of 4 per chunk, the same fragment values and
// operand order -- whatever TM x TN tile it belongs to.  A 128-tile split into 64-sub-tiles
// therefore gives bit-identical results; the launch code picks the tile shape from how many
// workgroups the launch would have (small shards: 64-sub-tiles fill the 256 CUs), and the
// chains stay independent of the sharding.
//
// Operands are described by strides so that every product the Cholesky / inverse / kriging
// code needs (NT, NN, TN) is the same kernel body:
//   op(A)(m,k) = A[m + k*sA]  (A_MU)   or  A[m*sA + k]  (!A_MU)
//   op(B)(k,n) = B[k*sB + n]  (B_NU)   or  B[k + n*sB]  (!B_NU)
// LDS images (a DMA wave instruction writes 64 lanes x 16 B = 1 KiB lane-linearly):
//   m-contiguous: [k][m], k-row stride 144 / 80 / 48 doubles (128 / 64 / 32-long operand); one
//     instruction per k-row (a shorter row uses the first lanes).  Every stride is 32 mod 64
//     dwords, so the two 16-lane halves of a ds_read_b64 group hit disjoint banks.
//   k-contiguous: [m][16], the 8 k-pairs of row m XOR-swizzled by (m >> 1) & 7.  One
//     instruction fills 8 rows (lane L: row L>>3, slot L&7 holds pair (L&7)^swz); the
//     swizzle is applied to the SOURCE address, so the image stays lane-linear while a
//     fragment read (16 m x 2 k per half-wave) touches 64 distinct banks.
// The MFMA is issued with (B-fragment, A-fragment) so the accumulator holds
// C^T: lane l, register r of block (bm,bn) is C[m = row0 + 16bm + (l&15)][n = col0 + 16bn +
// (l>>4) + 4r] -- consecutive lanes walk consecutive rows of a column-major C
// (coalesced 128-B stores) instead of consecutive columns.
//
// Two 128 x 128 bodies deal the 16-blocks over the waves differently where a quadrant would leave
// the waves unequal work, with the same MFMA sequence per element (so the same bits):
//   gemm_syrk_128  the diagonal tiles' updates, lower 16-blocks only, nine per wave
//   gemm_deal_128  the inverse levels' products, whose K range holds one triangular 128-deep block:
//                  wave w owns blocks w and 7 - w of the triangular dimension, the dense chunks run
//                  without a predicate and the triangular block's eight chunks are unrolled
#pragma once
#include <type_traits>
#include "mk_common.hpp"

namespace mk {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int GB_K = 16;                       // K chunk (the k-contiguous image assumes 8 pairs per row)
// m-contiguous image k-row stride: 32 mod 64 dwords for every operand length (bank-disjoint halves)
__host__ __device__ constexpr int gb_stride(int len) {
  return len == 256 ? 272 : (len == 128 ? 144 : (len == 64 ? 80 : 48));
}
__host__ __device__ constexpr int gb_img(int len) { return GB_K * gb_stride(len); }   // >= len * GB_K
// dynamic LDS of a TM x TN tile GEMM: two stages of (A image, B image)
__host__ __device__ constexpr int gb_lds_bytes(int tm, int tn) { return 2 * (gb_img(tm) + gb_img(tn)) * 8; }
static_assert(gb_lds_bytes(128, 128) == MK_GD_LDS_BYTES, "mk_common.hpp LDS size");
static_assert(128 * GB_K <= gb_img(128) && 64 * GB_K <= gb_img(64) && 32 * GB_K <= gb_img(32),
              "k-contiguous images fit their slots");

template <int BM, int BN>
struct AccT {
  d4 v[BM][BN];
};
typedef AccT<4, 4> Acc;   // 128 x 128

template <int BM, int BN>
__device__ inline void acc_zero(AccT<BM, BN>& a) {
#pragma unroll
  for (int i = 0; i < BM; ++i)
#pragma unroll
    for (int j = 0; j < BN; ++j) a.v[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
}

__device__ inline int ku_swz(int m) { return (m >> 1) & 7; }

// LDS-DMA wave instructions one dma_chunk issues per wave (4 waves)
template <bool MU, int LEN>
__host__ __device__ constexpr int dma_count() { return MU ? 4 * (LEN > 128 ? LEN / 128 : 1) : (LEN + 31) / 32; }

// DMA one LEN x 16 chunk of op(X) (k = k0 .. k0+15) into an LDS image.
template <bool MU, int LEN>
__device__ inline void dma_chunk(const double* __restrict__ X, long s, int k0, double* img) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (MU) {
    static_assert(!MU || LEN <= 128 || LEN % 128 == 0, "m-contiguous rows of 128-double pieces");
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = w + 4 * j;
#pragma unroll
      for (int pc = 0; pc < (LEN > 128 ? LEN / 128 : 1); ++pc)   // 1 KiB per wave instruction
        if (LEN >= 128 || lane < LEN / 2)
          __builtin_amdgcn_global_load_lds((const void*)(X + (long)(k0 + r) * s + 128 * pc + 2 * lane),
                                           (void*)(img + r * gb_stride(LEN) + 128 * pc), 16, 0, 0);
    }
  } else {
#pragma unroll
    for (int j = 0; j < (LEN + 31) / 32; ++j) {
      const int m8 = (w + 4 * j) * 8;
      const int m = m8 + (lane >> 3);
      const int pr = (lane & 7) ^ ku_swz(m);
      __builtin_amdgcn_global_load_lds((const void*)(X + (long)m * s + k0 + 2 * pr), (void*)(img + m8 * GB_K), 16, 0,
                                       0);
    }
  }
}

template <bool MU, int LEN>
__device__ inline double frag(const double* img, int m, int k) {
  return MU ? img[k * gb_stride(LEN) + m] : img[m * GB_K + 2 * ((k >> 1) ^ ku_swz(m)) + (k & 1)];
}

// Structural zeros (wave-uniform skips; the skipped MFMAs would add exact zeros or feed
// outputs nobody reads, so results are unchanged and the SIMD's matrix pipe goes to the
// co-resident wave instead).  Block indices are absolute within the 128-tile (rb0 / cb0: the
// sub-tile's offset in 16-blocks), so a sub-tile skips exactly what its 128-tile would:
//   SKIP_TRI_B op(B) lower-triangular in (n, k) over one 128-deep K: chunk c only touches
//               output column blocks >= c                             (flag = chunk index c)
//   SKIP_TRI_A  op(A) lower-triangular in (m, k) over the 128-deep K block starting at diag_tile
//               (gemm_tile): chunk c' of that block only touches output row blocks >= c'
//               (flag = c' inside the block, -1 elsewhere)
//   SKIP_TRI_BL op(B) lower-triangular in (k, n) over the 128-deep K block starting at diag_tile:
//               chunk c' of that block only touches output column blocks <= c'
//               (flag = c' inside the block, SKIP_FLAG_NONE elsewhere)
// (A diagonal tile's unread upper 16-blocks are not a skip of this body -- a predicate here leaves
// wave (1,0) with all 16 of its blocks -- but a body of their own: gemm_syrk_128 below.)
enum { SKIP_NONE = 0, SKIP_TRI_B = 2, SKIP_TRI_A = 3, SKIP_TRI_BL = 4 };
constexpr int SKIP_FLAG_NONE = 1 << 20;

// MASK: fragments with chunk-relative k >= kvalid read as zero.
template <int TM, int TN, bool NEG, bool A_MU, bool B_NU, int SKIP, bool MASK>
__device__ inline void mma_chunk(const double* As, const double* Bs, AccT<TM / 32, TN / 32>& acc, int flag,
                                 int kvalid, int rb0, int cb0) {
  constexpr int BM = TM / 32, BN = TN / 32;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wm = w & 1, wn = w >> 1;
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < GB_K / 4; ++ks) {
    const int k = ks * 4 + lk;
    const bool live = !MASK || k < kvalid;
    double ya[BM], xb[BN];
#pragma unroll
    for (int b = 0; b < BM; ++b) {
      const double av = live ? frag<A_MU, TM>(As, wm * (TM / 2) + b * 16 + li, k) : 0.0;
      ya[b] = NEG ? -av : av;
    }
#pragma unroll
    for (int b = 0; b < BN; ++b) xb[b] = live ? frag<B_NU, TN>(Bs, wn * (TN / 2) + b * 16 + li, k) : 0.0;
#pragma unroll
    for (int bm = 0; bm < BM; ++bm)
#pragma unroll
      for (int bn = 0; bn < BN; ++bn) {
        if (SKIP == SKIP_TRI_B && flag > cb0 + wn * BN + bn) continue;
        if (SKIP == SKIP_TRI_A && flag > rb0 + wm * BM + bm) continue;
        if (SKIP == SKIP_TRI_BL && flag < cb0 + wn * BN + bn) continue;
        acc.v[bm][bn] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[bn], ya[bm], acc.v[bm][bn], 0, 0, 0);
      }
  }
}

// acc += (NEG ? -1 : 1) op(A)[TM x K] * op(B)[K x TN], K % GB_K == 0 (MASK: k >= kvalid_total
// read as zero; the chunk's memory must still be addressable).
// REV: K chunks in descending order -- tiles of one launch whose K ranges share their END
// (triangular operands) then stream the same chunks at the same time, so an XCD's L2
// serves the shared panels once.  SAME: op(B) = op(A)^T read from the same memory (A'A
// products, TM == TN): one DMA and one LDS image serve both fragments.
// SKIP (see mma_chunk): SKIP_TRI_B for K = 128; SKIP_TRI_A /
// SKIP_TRI_BL with diag_tile = the K offset of the triangular 128-deep block.
// lds: gb_lds_bytes(TM, TN) of dynamic LDS.  Ends with a barrier (the caller may reuse the LDS).
template <int TM, int TN, bool A_MU, bool B_NU, bool NEG = false, bool REV = false, bool SAME = false,
          int SKIP = SKIP_NONE, bool MASK = false>
__device__ inline void gemm_tile(const double* __restrict__ A, long sA, const double* __restrict__ B, long sB, int K,
                                 int kvalid_total, AccT<TM / 32, TN / 32>& acc, double* lds, int diag_tile = 0,
                                 int rb0 = 0, int cb0 = 0) {
  static_assert(!SAME || TM == TN, "SAME needs a square tile");
  constexpr int STAGE = gb_img(TM) + gb_img(TN);
  if (K <= 0) return;
  const int nch = K / GB_K;
  auto k_of = [&](int c) { return REV ? K - GB_K * (c + 1) : GB_K * c; };
  auto issue = [&](int c) {
    double* st = lds + (c & 1) * STAGE;
    dma_chunk<A_MU, TM>(A, sA, k_of(c), st);
    if (!SAME) dma_chunk<B_NU, TN>(B, sB, k_of(c), st + gb_img(TM));
  };
  issue(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const double* st = lds + (c & 1) * STAGE;
    // the stage chunk c+1 overwrites was last read in iteration c-1, which every wave has left
    if (c + 1 < nch) issue(c + 1);
    const int k0 = k_of(c);
    int flag = diag_tile;
    if (SKIP == SKIP_TRI_B) {
      flag = k0 / GB_K;
    } else if (SKIP == SKIP_TRI_A || SKIP == SKIP_TRI_BL) {
      const int rel = k0 - diag_tile;
      flag = (rel >= 0 && rel < 128) ? rel / GB_K : (SKIP == SKIP_TRI_A ? -1 : SKIP_FLAG_NONE);
    }
    mma_chunk<TM, TN, NEG, A_MU, B_NU, SKIP, MASK>(st, SAME ? st : st + gb_img(TM), acc, flag, kvalid_total - k0,
                                                   rb0, cb0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

// acc += op(A)[TM x K] * B[K x TN] with B GENERATED into LDS rather than streamed: gen(k0, img)
// writes chunk k0's [16][TN] m-contiguous image (k-row stride gb_stride(TN)) with plain LDS stores.
// A streams by LDS-DMA as in gemm_tile; chunk c+1's B is generated while chunk c multiplies (the
// stage it overwrites was last read before the previous barrier).  Same MFMA sequence per element
// as gemm_tile<..., A_MU, B_NU = true> on a stored copy of the same values.
template <int TM, int TN, bool A_MU, class Gen>
__device__ inline void gemm_tile_genb(const double* __restrict__ A, long sA, int K, AccT<TM / 32, TN / 32>& acc,
                                      double* lds, Gen&& gen) {
  constexpr int STAGE = gb_img(TM) + gb_img(TN);
  if (K <= 0) return;
  const int nch = K / GB_K;
  dma_chunk<A_MU, TM>(A, sA, 0, lds);
  gen(0, lds + gb_img(TM));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const double* st = lds + (c & 1) * STAGE;
    if (c + 1 < nch) {
      double* nx = lds + ((c + 1) & 1) * STAGE;
      dma_chunk<A_MU, TM>(A, sA, GB_K * (c + 1), nx);
      gen(GB_K * (c + 1), nx + gb_img(TM));
    }
    mma_chunk<TM, TN, false, A_MU, true, SKIP_NONE, false>(st, st + gb_img(TM), acc, 0, GB_K, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

// Row-wave form of a TM x 128 tile, TM in {128, 64} (k_chol_update_trsm): wave w owns rows
// TM/4 * w .. of all 128 columns (TM/64 x 8 MFMA blocks) instead of a quadrant -- the same MFMA
// sequence per element (same chunks, k-steps, fragment values), so the same bits; what changes is
// which wave holds which rows, and a wave then holds whole rows of C: the operand of a solve
// applied from the right.
// Accumulator: lane l, register r of block (bm, bn) is C[TM/4 w + 16bm + (l & 15)][16bn + (l >> 4) + 4r].
template <int TM>
using AccRW = AccT<TM / 64, 8>;
template <int TM>
__device__ inline int rw_row(int bm) { return (threadIdx.x >> 6) * (TM / 4) + bm * 16 + (threadIdx.x & 15); }
__device__ inline int rw_col(int bn, int r) { return bn * 16 + ((threadIdx.x & 63) >> 4) + 4 * r; }

template <int TM, bool NEG>
__device__ inline void mma_chunk_rw(const double* As, const double* Bs, AccRW<TM>& acc) {
  constexpr int BM = TM / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < GB_K / 4; ++ks) {
    const int k = ks * 4 + lk;
    double ya[BM], xb[8];
#pragma unroll
    for (int b = 0; b < BM; ++b) {
      const double av = frag<true, TM>(As, w * (TM / 4) + b * 16 + li, k);
      ya[b] = NEG ? -av : av;
    }
#pragma unroll
    for (int b = 0; b < 8; ++b) xb[b] = frag<true, 128>(Bs, b * 16 + li, k);
#pragma unroll
    for (int bm = 0; bm < BM; ++bm)
#pragma unroll
      for (int bn = 0; bn < 8; ++bn)
        acc.v[bm][bn] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[bn], ya[bm], acc.v[bm][bn], 0, 0, 0);
  }
}

// gemm_tile<TM, 128, true, true, NEG> in the row-wave form (A m-contiguous, B n-contiguous), K > 0.
template <int TM, bool NEG>
__device__ inline void gemm_tile_rw(const double* __restrict__ A, long sA, const double* __restrict__ B, long sB, int K,
                                    AccRW<TM>& acc, double* lds) {
  constexpr int STAGE = gb_img(TM) + gb_img(128);
  const int nch = K / GB_K;   // K > 0
  auto issue = [&](int c) {
    double* st = lds + (c & 1) * STAGE;
    dma_chunk<true, TM>(A, sA, GB_K * c, st);
    dma_chunk<true, 128>(B, sB, GB_K * c, st + gb_img(TM));
  };
  issue(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const double* st = lds + (c & 1) * STAGE;
    if (c + 1 < nch) issue(c + 1);
    mma_chunk_rw<TM, NEG>(st, st + gb_img(TM), acc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

template <int TM>
__device__ inline void acc_load_rw(AccRW<TM>& acc, const double* C, long ldc) {
#pragma unroll
  for (int bm = 0; bm < TM / 64; ++bm)
#pragma unroll
    for (int bn = 0; bn < 8; ++bn)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc.v[bm][bn][r] = C[rw_row<TM>(bm) + (long)rw_col(bn, r) * ldc];
}

// ---------------------------------------------------------------- column strips: a ragged 128 x 128 row tile
// A row tile of which only the first V < 8 16-row blocks hold valid rows (the last tile of a factor of
// extent n_s + 1 inside n_pad).  In the row-wave form the waves that own padding rows idle, but the
// waves that own valid rows still issue 16 MFMAs per k-step and the chunk barrier ties the workgroup
// to them: the job is no shorter.  Here wave w owns the V valid row blocks of column blocks 2w and
// 2w + 1 -- 2V MFMAs per k-step on every wave, V + 2 fragments -- and the padding row blocks are
// neither loaded, multiplied nor stored.  Per element the MFMA sequence is mma_chunk_rw's (the same
// chunks in the same order, four k-steps with k = 4 ks + (lane >> 4), first operand the column
// block's fragment, second the row block's), so every valid element has the bits gemm_tile_rw gives
// it; what changes is which wave holds which block.
// Accumulator: lane l, register r of block (rb, j) is C[16 rb + (l & 15)][16 (2w + j) + (l >> 4) + 4r]:
// a block's register image does not depend on the wave that holds it, so the strips go back to the
// row-wave layout (cs_to_rw) as a copy of block images through LDS, no transpose.
template <int V>
using AccCS = AccT<V, 2>;
constexpr int CS_VMAX = 6;   // strips where 2V <= 12; V = 7 (14 MFMAs and the relayout against 16) keeps the rows

template <int V, bool NEG>
__device__ inline void mma_chunk_cs(const double* As, const double* Bs, AccCS<V>& acc, int w) {
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < GB_K / 4; ++ks) {
    const int k = ks * 4 + lk;
    double ya[V], xb[2];
#pragma unroll
    for (int b = 0; b < V; ++b) {
      const double av = frag<true, 128>(As, b * 16 + li, k);
      ya[b] = NEG ? -av : av;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) xb[j] = frag<true, 128>(Bs, (2 * w + j) * 16 + li, k);
#pragma unroll
    for (int bm = 0; bm < V; ++bm)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc.v[bm][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[j], ya[bm], acc.v[bm][j], 0, 0, 0);
  }
}

// gemm_tile_rw<128, NEG> on the first V row blocks, K > 0.  w: the wave, wave-uniform.  The A image
// still streams all 128 rows (one DMA instruction per k-row either way).  Ends with a barrier.
template <int V, bool NEG>
__device__ inline void gemm_tile_cs(const double* __restrict__ A, long sA, const double* __restrict__ B, long sB, int K,
                                    AccCS<V>& acc, double* lds, int w) {
  constexpr int STAGE = 2 * gb_img(128);
  const int nch = K / GB_K;   // K > 0
  auto issue = [&](int c) {
    double* st = lds + (c & 1) * STAGE;
    dma_chunk<true, 128>(A, sA, GB_K * c, st);
    dma_chunk<true, 128>(B, sB, GB_K * c, st + gb_img(128));
  };
  issue(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const double* st = lds + (c & 1) * STAGE;
    if (c + 1 < nch) issue(c + 1);
    mma_chunk_cs<V, NEG>(st, st + gb_img(128), acc, w);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

template <int V>
__device__ inline void acc_load_cs(AccCS<V>& acc, const double* C, long ldc, int w) {
  const int li = threadIdx.x & 15, lk = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int bm = 0; bm < V; ++bm)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc.v[bm][j][r] = C[16 * bm + li + (long)(16 * (2 * w + j) + lk + 4 * r) * ldc];
}

// The strips into the row-wave accumulator of the same tile: wave w' receives row blocks 2w' and
// 2w' + 1 of all eight column blocks (zeros where the row block is padding: >= V).  Two rounds, one
// per column block of a strip, each 4 waves x V block images of 2 KiB (lane-linear, 32 B per lane)
// in the LDS the DMA stages have left: at most 56 KiB of gb_lds_bytes(128, 128).  The caller's last
// barrier is behind it; ends with a barrier (the caller may reuse the LDS).
template <int V>
__device__ inline void cs_to_rw(const AccCS<V>& a, AccRW<128>& c, double* lds, int w) {
  static_assert(V >= 1 && V <= 7 && 4 * V * 2048 <= gb_lds_bytes(128, 128), "a round fits the stages' LDS");
  d2* img = (d2*)lds;   // block (rb, source wave ws): d2 index ((rb * 4 + ws) * 64 + lane) * 2
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int bm = 0; bm < V; ++bm) {
      d2* p = img + ((bm * 4 + w) * 64 + lane) * 2;
      p[0] = (d2){a.v[bm][j][0], a.v[bm][j][1]};
      p[1] = (d2){a.v[bm][j][2], a.v[bm][j][3]};
    }
    __syncthreads();
#pragma unroll
    for (int bm = 0; bm < 2; ++bm) {
      const int rb = 2 * w + bm;
      if (rb < V) {   // wave-uniform
#pragma unroll
        for (int ws = 0; ws < 4; ++ws) {
          const d2* p = img + ((rb * 4 + ws) * 64 + lane) * 2;
          const d2 lo = p[0], hi = p[1];
          c.v[bm][2 * ws + j] = (d4){lo[0], lo[1], hi[0], hi[1]};
        }
      } else {
#pragma unroll
        for (int ws = 0; ws < 4; ++ws) c.v[bm][2 * ws + j] = (d4){0.0, 0.0, 0.0, 0.0};
      }
    }
    __syncthreads();
  }
}

// The 128 x 128 form every kernel started from.
template <bool A_MU, bool B_NU, bool NEG = false, bool REV = false, bool SAME = false, int SKIP = SKIP_NONE,
          bool MASK = false>
__device__ inline void gemm_128(const double* __restrict__ A, long sA, const double* __restrict__ B, long sB, int K,
                                int kvalid_total, Acc& acc, double* lds, int diag_tile = 0) {
  gemm_tile<128, 128, A_MU, B_NU, NEG, REV, SAME, SKIP, MASK>(A, sA, B, sB, K, kvalid_total, acc, lds, diag_tile);
}

// Element coordinates of accumulator (bm,bn,r) for this lane (within the TM x TN tile).
template <int TM = 128>
__device__ inline int acc_row(int bm) {
  const int lane = threadIdx.x & 63, wm = (threadIdx.x >> 6) & 1;
  return wm * (TM / 2) + bm * 16 + (lane & 15);
}
template <int TN = 128>
__device__ inline int acc_col(int bn, int r) {
  const int lane = threadIdx.x & 63, wn = threadIdx.x >> 7;
  return wn * (TN / 2) + bn * 16 + (lane >> 4) + 4 * r;
}

// acc = C (column-major, ldc): preload for C -= A B^T updates (no read-modify-write epilogue).
template <int BM, int BN>
__device__ inline void acc_load(AccT<BM, BN>& acc, const double* C, long ldc) {
#pragma unroll
  for (int bm = 0; bm < BM; ++bm)
#pragma unroll
    for (int bn = 0; bn < BN; ++bn)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc.v[bm][bn][r] = C[acc_row<BM * 32>(bm) + (long)acc_col<BN * 32>(bn, r) * ldc];
}

// C = acc (column-major, ldc); optional mirrored store C^T at Ct.  Pure stores only:
// accumulating updates preload C into the accumulators (acc_load) and negate the A
// fragment (gemm_tile<..., NEG>), which keeps the kernels at <= 256 registers (2 waves/SIMD).
template <int BM, int BN>
__device__ inline void store_tile(double* C, long ldc, const AccT<BM, BN>& acc, double* Ct = nullptr) {
#pragma unroll
  for (int bm = 0; bm < BM; ++bm)
#pragma unroll
    for (int bn = 0; bn < BN; ++bn)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = acc_row<BM * 32>(bm), n = acc_col<BN * 32>(bn, r);
        C[m + (long)n * ldc] = acc.v[bm][bn][r];
        if (Ct) Ct[n + (long)m * ldc] = acc.v[bm][bn][r];
      }
}

// ---------------------------------------------------------------- symmetric rank-K update, lower 16-blocks only
// acc -= P P^T for a 128 x K panel P (m-contiguous: op(P)(m, k) = P[m + k*s]) -- the diagonal
// tiles' update, of which only the lower triangle is ever read.  The 36 16-blocks with cb <= rb
// are dealt evenly: wave w owns row blocks w and 7 - w, nine blocks,
//   slot s <= w : block (rb = w,     cb = s)
//   slot s >  w : block (rb = 7 - w, cb = s - w - 1)
// so every wave issues 9 MFMAs per k-step where the quadrant body issues 16 (a skip inside that
// body leaves wave (1,0) with all 16 of its blocks: the workgroup is no shorter), one LDS image
// serves both fragments (half the DMA bytes of two), and no predicate sits in the K loop.  Blocks on
// the diagonal are computed whole.  Slots are indexed statically; rb and cb are wave-uniform scalars
// that only enter LDS and memory addresses.
// Per element the MFMA sequence is mma_chunk's (ascending 16-deep chunks, four k-steps with
// k = 4 ks + (lane >> 4), first operand the column block's fragment, second the negated row
// block's), so every lower-triangle element has the bits gemm_tile<128, 128, true, true, true>
// gives it.  Accumulator: lane l, register r of slot s is C[16 rb + (l & 15)][16 cb + (l >> 4) + 4r].
constexpr int SYRK_SLOTS = 9;
__host__ __device__ constexpr int syrk_rb(int w, int s) { return s <= w ? w : 7 - w; }
__host__ __device__ constexpr int syrk_cb(int w, int s) { return s <= w ? s : s - w - 1; }
// every block with cb <= rb exactly once, nothing else
constexpr bool syrk_cover_exact() {
  int cnt[8][8] = {};
  for (int w = 0; w < 4; ++w)
    for (int s = 0; s < SYRK_SLOTS; ++s) {
      const int rb = syrk_rb(w, s), cb = syrk_cb(w, s);
      if (rb < 0 || rb > 7 || cb < 0 || cb > rb) return false;
      ++cnt[rb][cb];
    }
  for (int rb = 0; rb < 8; ++rb)
    for (int cb = 0; cb < 8; ++cb)
      if (cnt[rb][cb] != (cb <= rb ? 1 : 0)) return false;
  return true;
}
static_assert(syrk_cover_exact(), "the SYRK block map covers the lower 16-blocks exactly once");
// what mma_chunk_syrk relies on: slot 0 is in row block w and slots 4.. in row block 7 - w for every
// wave, and the last slot is the second row block's diagonal block
constexpr bool syrk_rows_static() {
  for (int w = 0; w < 4; ++w) {
    if (syrk_rb(w, 0) != w || syrk_cb(w, SYRK_SLOTS - 1) != 7 - w) return false;
    for (int s = 4; s < SYRK_SLOTS; ++s)
      if (syrk_rb(w, s) != 7 - w) return false;
  }
  return true;
}
static_assert(syrk_rows_static(), "slot 0 / slots 4.. have the same row choice on every wave");

struct AccSyrk {
  d4 v[SYRK_SLOTS];
};
__device__ inline int syrk_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
// Element coordinates of accumulator (s, r) for this lane (within the 128 x 128 tile).
__device__ inline int syrk_row(int w, int s) { return 16 * syrk_rb(w, s) + (threadIdx.x & 15); }
__device__ inline int syrk_col(int w, int s, int r) { return 16 * syrk_cb(w, s) + ((threadIdx.x & 63) >> 4) + 4 * r; }

__device__ inline void mma_chunk_syrk(const double* Ps, AccSyrk& acc, int w) {
  constexpr int LD = gb_stride(128);
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < GB_K / 4; ++ks) {
    const double* row = Ps + (ks * 4 + lk) * LD + li;
    // the two row blocks' fragments; the second is also the last slot's column fragment
    const double p0 = row[16 * w], p1 = row[16 * (7 - w)];
    const double y0 = -p0, y1 = -p1;
    double xb[SYRK_SLOTS];
#pragma unroll
    for (int s = 0; s < SYRK_SLOTS - 1; ++s) xb[s] = row[16 * syrk_cb(w, s)];
    xb[SYRK_SLOTS - 1] = p1;
#pragma unroll
    for (int s = 0; s < SYRK_SLOTS; ++s) {
      const double ya = s == 0 ? y0 : (s >= 4 ? y1 : (s <= w ? y0 : y1));   // a wave-uniform select
      acc.v[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[s], ya, acc.v[s], 0, 0, 0);
    }
  }
}

// K % GB_K == 0.  lds: 2 * gb_img(128) doubles (two stages of the one image).  Ends with a barrier
// (the caller may reuse the LDS).
__device__ inline void gemm_syrk_128(const double* __restrict__ P, long s, int K, AccSyrk& acc, double* lds) {
  constexpr int STAGE = gb_img(128);
  if (K <= 0) return;
  const int nch = K / GB_K;
  const int w = syrk_wave();
  dma_chunk<true, 128>(P, s, 0, lds);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    // the stage chunk c+1 overwrites was last read in iteration c-1, which every wave has left
    if (c + 1 < nch) dma_chunk<true, 128>(P, s, GB_K * (c + 1), lds + ((c + 1) & 1) * STAGE);
    mma_chunk_syrk(lds + (c & 1) * STAGE, acc, w);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

// acc = the nine blocks of C (column-major, ldc); C = acc.
__device__ inline void acc_load_syrk(AccSyrk& acc, const double* C, long ldc) {
  const int w = syrk_wave();
#pragma unroll
  for (int s = 0; s < SYRK_SLOTS; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc.v[s][r] = C[syrk_row(w, s) + (long)syrk_col(w, s, r) * ldc];
}
__device__ inline void store_tile_syrk(double* C, long ldc, const AccSyrk& acc) {
  const int w = syrk_wave();
#pragma unroll
  for (int s = 0; s < SYRK_SLOTS; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) C[syrk_row(w, s) + (long)syrk_col(w, s, r) * ldc] = acc.v[s][r];
}
// The store into a column-major LDS image T (stride tld) that holds the lower triangle and zeros
// above it: elements above the diagonal inside the diagonal blocks are masked, and all 256 threads
// zero the 28 blocks with cb > rb (one element of each per thread).
__device__ inline void store_tile_syrk_lds(double* T, int tld, const AccSyrk& acc) {
  const int w = syrk_wave();
#pragma unroll
  for (int s = 0; s < SYRK_SLOTS; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = syrk_row(w, s), cc = syrk_col(w, s, r);
      T[rr + cc * tld] = rr >= cc ? acc.v[s][r] : 0.0;
    }
  const int zr = threadIdx.x & 15, zc = threadIdx.x >> 4;
#pragma unroll
  for (int rb = 0; rb < 8; ++rb)
#pragma unroll
    for (int cb = rb + 1; cb < 8; ++cb) T[(16 * rb + zr) + (16 * cb + zc) * tld] = 0.0;
}

// ---------------------------------------------------------------- dealt body: one triangular 128-deep K block
// acc += (NEG ? -1 : 1) op(A)[128 x K] * op(B)[K x 128] (A m-contiguous, B k-contiguous, K a multiple
// of 128) where one 128-deep K block is lower-triangular -- the inverse levels' products:
//   row-dealt    (!COL): op(A) lower in (m, k) over the LAST K block, ascending chunks: chunk c' of
//                        that block only touches row blocks >= c'          (gemm_tile's SKIP_TRI_A)
//   column-dealt (COL):  op(B) lower in (k, n) over the FIRST K block, which the descending order
//                        reaches last: chunk c' only touches column blocks <= c'     (SKIP_TRI_BL)
// A skip inside the quadrant body is unbalanced (the waves that own blocks 0-3 of the triangular
// dimension keep 26 of their 32 (block, chunk) pairs, the others 10: the tile costs 26/32 of a dense
// one) and puts a predicate before every MFMA of every chunk.  Here wave w owns the two 16-blocks
// w and 7 - w along the triangular dimension and all eight along the other (2 + 8 fragments and 16
// MFMAs per k-step), so every wave keeps 9 of its 16 (block, chunk) pairs, and the K loop is split:
// the dense chunks run with no predicate, the triangular block's eight chunks are unrolled with c'
// a compile-time constant.  For a given c' at most one of a wave's two blocks depends on w: one
// wave-uniform branch around a group of 8 MFMAs per k-step.
// Per element the MFMA sequence is mma_chunk's (the same chunks in the same order, four k-steps
// with k = 4 ks + (lane >> 4), first operand the B fragment, second the A fragment) and the skipped
// set is SKIP_TRI_A's / SKIP_TRI_BL's, so every element has the bits gemm_tile gives it.
// Accumulator (d: the dealt block, 0 -> w, 1 -> 7 - w; o: the block along the other dimension):
//   row-dealt    v[d][o]: C[16 blk(d) + (l & 15)][16 o + (l >> 4) + 4r]
//   column-dealt v[o][d]: C[16 o + (l & 15)][16 blk(d) + (l >> 4) + 4r]
template <bool COL>
using AccDeal = AccT<COL ? 8 : 2, COL ? 2 : 8>;
__host__ __device__ constexpr int deal_blk(int w, int d) { return d == 0 ? w : 7 - w; }
// is block blk of the triangular dimension touched by chunk cp of the triangular K block?
__host__ __device__ constexpr bool deal_live(bool col, int blk, int cp) { return col ? blk <= cp : blk >= cp; }
// the same for dealt block d of EVERY wave (d = 0: blocks 0..3, d = 1: blocks 4..7): these decide at
// compile time; what is left is one wave-uniform test
__host__ __device__ constexpr bool deal_always(bool col, int d, int cp) {
  return deal_live(col, col ? 4 * d + 3 : 4 * d, cp);
}
__host__ __device__ constexpr bool deal_never(bool col, int d, int cp) {
  return !deal_live(col, col ? 4 * d : 4 * d + 3, cp);
}
// every live (block, chunk) exactly once and nothing else, 9 of 16 per wave, the compile-time
// classes agree with deal_live on every wave, and at most one block per chunk is left to a branch
constexpr bool deal_cover_exact(bool col) {
  int cnt[8][8] = {};
  for (int w = 0; w < 4; ++w) {
    int mine = 0;
    for (int cp = 0; cp < 8; ++cp) {
      int branches = 0;
      for (int d = 0; d < 2; ++d) {
        const int blk = deal_blk(w, d);
        const bool live = deal_live(col, blk, cp);
        if (deal_always(col, d, cp) && !live) return false;
        if (deal_never(col, d, cp) && live) return false;
        if (deal_always(col, d, cp) && deal_never(col, d, cp)) return false;
        if (!deal_always(col, d, cp) && !deal_never(col, d, cp)) ++branches;
        if (live) {
          ++cnt[blk][cp];
          ++mine;
        }
      }
      if (branches > 1) return false;
    }
    if (mine != 9) return false;
  }
  for (int blk = 0; blk < 8; ++blk)
    for (int cp = 0; cp < 8; ++cp)
      if (cnt[blk][cp] != (deal_live(col, blk, cp) ? 1 : 0)) return false;
  return true;
}
static_assert(deal_cover_exact(false) && deal_cover_exact(true),
              "both deals cover the live (block, chunk) pairs exactly once, nine per wave");

// Element coordinates of accumulator (bm, bn, r) for this lane (within the 128 x 128 tile).
template <bool COL>
__device__ inline int deal_row(int w, int bm) { return 16 * (COL ? bm : deal_blk(w, bm)) + (threadIdx.x & 15); }
template <bool COL>
__device__ inline int deal_col(int w, int bn, int r) {
  return 16 * (COL ? deal_blk(w, bn) : bn) + ((threadIdx.x & 63) >> 4) + 4 * r;
}

// CP: the chunk's index c' inside the triangular K block, -1 for a dense chunk.
template <bool COL, bool NEG, int CP>
__device__ inline void mma_chunk_deal(const double* As, const double* Bs, AccDeal<COL>& acc, int w) {
  constexpr int BM = COL ? 8 : 2, BN = COL ? 2 : 8;
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < GB_K / 4; ++ks) {
    const int k = ks * 4 + lk;
    double ya[BM], xb[BN];
#pragma unroll
    for (int b = 0; b < BM; ++b) {
      const double av = frag<true, 128>(As, 16 * (COL ? b : deal_blk(w, b)) + li, k);
      ya[b] = NEG ? -av : av;
    }
#pragma unroll
    for (int b = 0; b < BN; ++b) xb[b] = frag<false, 128>(Bs, 16 * (COL ? deal_blk(w, b) : b) + li, k);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      if (CP >= 0 && deal_never(COL, d, CP)) continue;
      if (CP >= 0 && !deal_always(COL, d, CP) && !deal_live(COL, deal_blk(w, d), CP)) continue;   // wave-uniform
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        if constexpr (COL)
          acc.v[o][d] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[d], ya[o], acc.v[o][d], 0, 0, 0);
        else
          acc.v[d][o] = __builtin_amdgcn_mfma_f64_16x16x4f64(xb[o], ya[d], acc.v[d][o], 0, 0, 0);
      }
    }
  }
}

// K >= 128, K % 128 == 0: K / 16 - 8 dense chunks, then the triangular block's eight (none dense
// when the triangular block is the whole K range).  REV as in gemm_tile; the column deal's
// triangular block is the first, so COL goes with REV and !COL with ascending chunks.
// lds: gb_lds_bytes(128, 128).  Ends with a barrier (the caller may reuse the LDS).
template <bool COL, bool NEG>
__device__ inline void gemm_deal_128(const double* __restrict__ A, long sA, const double* __restrict__ B, long sB, int K,
                                     AccDeal<COL>& acc, double* lds) {
  constexpr bool REV = COL;
  constexpr int IMG = gb_img(128), STAGE = 2 * IMG;
  const int nch = K / GB_K, nd = nch - 128 / GB_K;   // nd is even: a chunk's stage is its parity in either part
  const int w = syrk_wave();
  auto k_of = [&](int c) { return REV ? K - GB_K * (c + 1) : GB_K * c; };
  auto issue = [&](int c) {
    double* st = lds + (c & 1) * STAGE;
    dma_chunk<true, 128>(A, sA, k_of(c), st);
    dma_chunk<false, 128>(B, sB, k_of(c), st + IMG);
  };
  issue(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int c = 0; c < nd; ++c) {
    const double* st = lds + (c & 1) * STAGE;
    // the stage chunk c+1 overwrites was last read in iteration c-1, which every wave has left
    issue(c + 1);
    mma_chunk_deal<COL, NEG, -1>(st, st + IMG, acc, w);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
#define MK_DEAL_TRI(t)                                                              \
  {                                                                                 \
    const double* st = lds + ((t) & 1) * STAGE;                                     \
    if ((t) < 7) issue(nd + (t) + 1);                                               \
    mma_chunk_deal<COL, NEG, REV ? 7 - (t) : (t)>(st, st + IMG, acc, w);            \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                \
    __syncthreads();                                                                \
  }
  MK_DEAL_TRI(0) MK_DEAL_TRI(1) MK_DEAL_TRI(2) MK_DEAL_TRI(3)
  MK_DEAL_TRI(4) MK_DEAL_TRI(5) MK_DEAL_TRI(6) MK_DEAL_TRI(7)
#undef MK_DEAL_TRI
}

// C = acc (column-major, ldc): lanes walk 16 consecutive rows of a column, as in store_tile.
template <bool COL>
__device__ inline void store_tile_deal(double* C, long ldc, const AccDeal<COL>& acc) {
  const int w = syrk_wave();
#pragma unroll
  for (int bm = 0; bm < (COL ? 8 : 2); ++bm)
#pragma unroll
    for (int bn = 0; bn < (COL ? 2 : 8); ++bn)
#pragma unroll
      for (int r = 0; r < 4; ++r) C[deal_row<COL>(w, bm) + (long)deal_col<COL>(w, bn, r) * ldc] = acc.v[bm][bn][r];
}

}  // namespace mk
