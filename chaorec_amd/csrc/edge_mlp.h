// What adagcl.hip and grade.hip share: the row ownership of their per-entry sums and the vgae decoder's 64 x 64 MLP tile.
// One definition each; the two files keep their formulas, their kernel bodies and their exports.
//
// Row ownership, everywhere a row is summed: a wave holds AG_RW = 8 rows, 8 lanes each (lane j of a row takes its entries
// j, j + 8, ..., then a butterfly xor 4, 2, 1); a row with more than AG_LONG = 64 entries is taken by its whole wave
// afterwards (lane j: entries j, j + 64, ...; butterfly xor 32 .. 1).  A sum's order depends on the row's length alone:
// two runs give the same bits.  No atomics on floats.
//
// The MLP tile: logit = w2 . relu(W1 relu(z[a] * z[b]) + b1) + b2 for 64 node pairs per wave on v_mfma_f32_32x32x2_f32 (exact
// fp32 products, k-ascending chain): C[feature][pair] = sum_k W1[feature][k] P[pair][k] -- A = W1 from LDS (16 KB,
// Ws[k][f ^ 32 (k & 1)]: the two k of one instruction sit in different halves of the 64 banks), B = the gathered rows'
// product, formed in registers.  The features are the accumulator's rows, so the w2 dot is a per-lane sum over 32 registers
// and one xor-32 exchange.
#pragma once
#include "vae_common.h"

namespace chaorec {

constexpr int AG_D = 64;
constexpr int AG_RW = 8;           // rows per wave
constexpr int AG_RB = kRowsPerBlock8;      // rows per workgroup
constexpr int AG_LONG = 64;        // a longer row is taken by the whole wave

struct ag2 {
  float a, b;
};

// every lane of the wave calls; n / [beg, end): the lane group's row (beg = end for none).  f(e, row) -> ag2, called once per
// entry.  -> the row's two sums, on every lane of its group
template <class F>
__device__ __forceinline__ ag2 ag_row_reduce(int64_t n, int64_t beg, int64_t end, int lane, F f) {
  const int sub = lane & 7;
  const bool is_long = end - beg > AG_LONG;
  ag2 acc = {0.f, 0.f};
  if (!is_long)
    for (int64_t e = beg + sub; e < end; e += 8) {
      const ag2 t = f(e, n);
      acc.a += t.a;
      acc.b += t.b;
    }
  acc.a = group_sum<8>(acc.a);
  acc.b = group_sum<8>(acc.b);
  unsigned long long mask = __ballot(is_long && sub == 0);
  while (mask) {
    const int src = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const int64_t n_s = __shfl(n, src, 64), b_s = __shfl(beg, src, 64), e_s = __shfl(end, src, 64);
    ag2 t = {0.f, 0.f};
    for (int64_t e = b_s + lane; e < e_s; e += 64) {
      const ag2 x = f(e, n_s);
      t.a += x.a;
      t.b += x.b;
    }
    t.a = wave_sum(t.a);
    t.b = wave_sum(t.b);
    if ((lane >> 3) == (src >> 3)) acc = t;
  }
  return acc;
}

struct EdgeMlpLds {
  float Ws[AG_D * AG_D];      // Ws[k][f ^ 32 (k & 1)] = W1[f][k]
  float b1s[AG_D], w2s[AG_D];
};

// the 256 threads of a workgroup stage one decoder's weights; readable on return
__device__ __forceinline__ void edge_mlp_stage(EdgeMlpLds &s, const float *__restrict__ W1, const float *__restrict__ b1,
                                               const float *__restrict__ w2, int t) {
#pragma unroll
  for (int p = 0; p < AG_D * AG_D / 256; ++p) {
    const int idx = t + 256 * p, k = idx >> 6, f = idx & 63;
    s.Ws[AG_D * k + (f ^ ((k & 1) << 5))] = W1[f * AG_D + k];
  }
  if (t < AG_D) {
    s.b1s[t] = b1[t];
    s.w2s[t] = w2[t];
  }
  __syncthreads();
}

struct EdgeNodes {
  int a, b;       // the pair's two rows of z, both in range
};

// every lane of the wave calls; nodes(slot) -> the pair of the wave's slot 0 .. 63 (called for slots r and 32 + r).
// -> the logit of slot `lane`
template <class F>
__device__ __forceinline__ float edge_mlp_tile(const EdgeMlpLds &s, const float *__restrict__ z, float bias2, int lane, F nodes) {
  const int r = lane & 31, h = lane >> 5;
  float mine = 0.f;
#pragma unroll
  for (int et = 0; et < 2; ++et) {
    const EdgeNodes nd = nodes(32 * et + r);
    const float4 *zr = reinterpret_cast<const float4 *>(z + (int64_t)nd.a * AG_D);
    const float4 *zc = reinterpret_cast<const float4 *>(z + (int64_t)nd.b * AG_D);
    float bf[AG_D / 2];                // P[pair r][k = 2 s + h]
#pragma unroll
    for (int q = 0; q < AG_D / 4; ++q) {
      const float4 a = zr[q], c = zc[q];
      bf[2 * q] = fmaxf(h ? a.y * c.y : a.x * c.x, 0.f);
      bf[2 * q + 1] = fmaxf(h ? a.w * c.w : a.z * c.z, 0.f);
    }
    float tsum = 0.f;
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
      f32x16 acc = vae_zero();
#pragma unroll
      for (int k = 0; k < AG_D / 2; ++k)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s.Ws[AG_D * (2 * k + h) + ((32 * jt + r) ^ (h << 5))], bf[k], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int f = 32 * jt + vae_row(q, h);
        tsum += s.w2s[f] * fmaxf(acc[q] + s.b1s[f], 0.f);
      }
    }
    tsum += __shfl_xor(tsum, 32, 64);
    if (h == et) mine = tsum + bias2;
  }
  return mine;
}

}  // namespace chaorec
