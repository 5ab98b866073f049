// What diffmm.hip's and diffrec.hip's output layers share: one 128 x 128 tile of acc = A Bm^T per workgroup on the f32 MFMA
// pipe, the placement of the workgroups on the XCDs, the x0-error epilogue of the two loss kernels with its padded store,
// and the launch grid.  One definition each: the files keep their kernels, what they add to the tile (DiffMM's second
// product and its k acc2 term, DiffRec's chain epilogue), their reductions and their exports.  (gemm.hip's loop serves four
// tile shapes, both transposes, split-K and an unguarded interior path, and stays its own.)
#pragma once
#include "vae_common.h"

namespace chaorec {

constexpr int OT_BM = 128, OT_BN = 128, OT_BK = 16, OT_PAD = 4;   // the tile: waves 2 x 2 of 64 x 64, as gemm.hip's <128, 128>
constexpr int OT_SEG = 64;        // k per segment of a chain (a multiple of OT_BK)

typedef float OtStage[2][OT_BK][OT_BM + OT_PAD];      // one operand's tiles in LDS: k-major, double-buffered (OT_BM == OT_BN)

// Where a thread works: tile (mt, nt) at (m0, n0), its wave's 64 x 64 at (wrow, wcol), the lane's column rr and row half hh
// of a 32 x 32 accumulator.  Workgroups are dealt to the 8 XCDs round-robin: block id -> (id % 8, id / 8), and the workgroups
// of one XCD walk the row tiles of one column tile before the next, so a slice of Bm (W_out) is read into one L2 and A (h,
// 4 MB) stays in all of them.  The deal rounds NT up to 8: `live` is false for a WHOLE workgroup past the last column tile,
// which returns before it reaches a barrier.
struct OutTile {
  int64_t mt, nt, m0, n0;
  int t, wave, wrow, wcol, rr, hh;
  bool live;
};
__device__ __forceinline__ OutTile out_tile_place(int64_t MT, int64_t NT) {
  OutTile tp;
  const int64_t slot = (int64_t)blockIdx.x >> 3;
  tp.nt = (slot / MT) * 8 + ((int64_t)blockIdx.x & 7);
  tp.mt = slot % MT;
  tp.live = tp.nt < NT;
  tp.t = threadIdx.x;
  tp.wave = tp.t >> 6;
  const int lane = tp.t & 63;
  tp.rr = lane & 31;
  tp.hh = lane >> 5;
  tp.wrow = (tp.wave >> 1) * 64;
  tp.wcol = (tp.wave & 1) * 64;
  tp.m0 = tp.mt * OT_BM;
  tp.n0 = tp.nt * OT_BN;
  return tp;
}

// the launch grid of a tile kernel over [M, N]; blocks == 0: too many workgroups
struct OutGrid {
  int64_t MT, NT, blocks;
};
inline OutGrid out_tile_grid(int64_t M, int64_t N) {
  OutGrid g = {(M + OT_BM - 1) / OT_BM, (N + OT_BN - 1) / OT_BN, 0};
  const int64_t blocks = (g.NT + 7) / 8 * g.MT * 8;
  g.blocks = blocks > 0x7fffffff ? 0 : blocks;
  return g;
}

// acc += A[m0 .., 0 .. K) . Bm[n0 .., 0 .. K)^T for the tile of tp; every thread of the workgroup calls.  Both operands
// [rows][k] (rows past M / N read as 0), K a multiple of 4 and rows 16-byte aligned: a float4 is inside or outside.  The K
// loop is gemm.hip's: operand tiles staged k-major in LDS, double-buffered, the k-ascending fmaf chain of
// v_mfma_f32_32x32x2_f32 per element.
// SEGMENTED: the chain is cut into segments of OT_SEG = 64 k.  After every fourth tile the chain's value is added to a
// running sum and the chain restarts from zero; the last, partial segment (zero when K % 64 == 0) is added on return:
// segments in ascending order, the same bits every run.  One chain over K = 1000 rounds a thousand times at the magnitude
// of its growing partial sum and deviated 4 to 5 times as much as torch's blocked fp32 sum (measured against float64 at
// H = 1000: 1.0 to 1.3e-6 of the largest |d_out|, torch 2.5 to 3e-7).  acc is zero on entry.
template <bool SEGMENTED>
__device__ __forceinline__ void out_tile_run(f32x16 (&acc)[2][2], const OutTile &tp, OtStage &As, OtStage &Bs, const float *__restrict__ A,
                                             int64_t lda, const float *__restrict__ Bm, int64_t ldb, int64_t M, int64_t N, int64_t K) {
  f32x16 sum[2][2];
  if constexpr (SEGMENTED) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) sum[i][j] = vae_zero();
  }
  float4 ra[2], rb[2];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int v = tp.t + p * 256, row = v >> 2, k4 = (v & 3) * 4;
      const int64_t gk = k0 + k4;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
      if (tp.m0 + row < M && gk < K) x = *reinterpret_cast<const float4 *>(A + (tp.m0 + row) * lda + gk);
      if (tp.n0 + row < N && gk < K) y = *reinterpret_cast<const float4 *>(Bm + (tp.n0 + row) * ldb + gk);
      ra[p] = x;
      rb[p] = y;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int v = tp.t + p * 256, row = v >> 2, k4 = (v & 3) * 4;
      As[buf][k4 + 0][row] = ra[p].x;
      As[buf][k4 + 1][row] = ra[p].y;
      As[buf][k4 + 2][row] = ra[p].z;
      As[buf][k4 + 3][row] = ra[p].w;
      Bs[buf][k4 + 0][row] = rb[p].x;
      Bs[buf][k4 + 1][row] = rb[p].y;
      Bs[buf][k4 + 2][row] = rb[p].z;
      Bs[buf][k4 + 3][row] = rb[p].w;
    }
  };
  int buf = 0;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int64_t k0 = 0; k0 < K; k0 += OT_BK) {
    const bool more = k0 + OT_BK < K;
    if (more) fetch(k0 + OT_BK);
    float af[OT_BK / 2][2], bf[OT_BK / 2][2];
#pragma unroll
    for (int s = 0; s < OT_BK / 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[s][i] = As[buf][2 * s + tp.hh][tp.wrow + 32 * i + tp.rr];
        bf[s][i] = Bs[buf][2 * s + tp.hh][tp.wcol + 32 * i + tp.rr];
      }
#pragma unroll
    for (int s = 0; s < OT_BK / 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s][i], bf[s][j], acc[i][j], 0, 0, 0);
    if constexpr (SEGMENTED) {
      if (((k0 + OT_BK) % OT_SEG) == 0) {     // a segment is complete: into the running sum, the chain restarts from zero
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            sum[i][j] = sum[i][j] + acc[i][j];
            acc[i][j] = vae_zero();
          }
      }
    }
    if (more) stash(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
  if constexpr (SEGMENTED) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = sum[i][j] + acc[i][j];
  }
}

// The x0-error epilogue on acc = the tile of h W_out^T, in registers; every thread of the workgroup calls (one barrier):
//   err = (acc + bias[i]) - x0[b, i]      (x0 from the bit table: the 32 columns of a lane group are one word)
//   part[b, nt] = the tile's share of sum_i err^2 per row: columns in a fixed butterfly order, then the two column halves
//   acc = c_row[b] err, 0 outside [M, N)
// A product that is to be added to c_b err afterwards starts from zero in a SECOND set of accumulators.  (Continuing the
// chain on c_b err instead would save 64 registers and round 64 times at the magnitude of c_b err, which at small B I is a
// thousand times that of the chain's terms: measured on DiffMM's r F^T, 8 ulp of d_out.)
__device__ __forceinline__ void out_tile_x0_err(f32x16 (&acc)[2][2], const OutTile &tp, float (&Ps)[2][OT_BM], const float *__restrict__ bias,
                                                const uint32_t *__restrict__ bits, int64_t nwords, const float *__restrict__ c_row,
                                                int64_t M, int64_t N, int64_t NT, float *__restrict__ part) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = tp.wrow + 32 * i + vae_row(reg, tp.hh);
      const int64_t gm = tp.m0 + row;
      const float cb = gm < M ? c_row[gm] : 0.f;
      float sq = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t g0 = tp.n0 + tp.wcol + 32 * j, gn = g0 + tp.rr;
        float err = 0.f;
        if (gm < M && gn < N) {
          const uint32_t word = bits[gm * nwords + (g0 >> 5)];
          const float x0 = ((word >> tp.rr) & 1u) ? 1.f : 0.f;
          err = (acc[i][j][reg] + bias[gn]) - x0;
        }
        sq = sq + err * err;
        acc[i][j][reg] = cb * err;
      }
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) sq = sq + __shfl_xor(sq, off, 64);   // within the 32 lanes that hold the row
      if (tp.rr == 0) Ps[tp.wave & 1][row] = sq;
    }
  }
  __syncthreads();
  if (tp.t < OT_BM && tp.m0 + tp.t < M) part[(tp.m0 + tp.t) * NT + tp.nt] = Ps[0][tp.t] + Ps[1][tp.t];
}

// out[m0 .., n0 ..] = acc for the rows below M; columns N .. ldo of a row are written 0 (ldo <= NT * OT_BN)
__device__ __forceinline__ void out_tile_store_padded(const f32x16 (&acc)[2][2], const OutTile &tp, int64_t M, int64_t N,
                                                      float *__restrict__ out, int64_t ldo) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t gn = tp.n0 + tp.wcol + 32 * j + tp.rr;
      if (gn >= ldo) continue;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int64_t gm = tp.m0 + tp.wrow + 32 * i + vae_row(reg, tp.hh);
        if (gm < M) out[gm * ldo + gn] = gn < N ? acc[i][j][reg] : 0.f;
      }
    }
}

}  // namespace chaorec
