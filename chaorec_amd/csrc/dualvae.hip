// DualVAE (Model/DualVAE.py): the two-sided aspect encoder and the Poisson likelihood with its neighbourhood term, without
// any [B, U], [B, I] or [U, I] buffer.
//
// One kernel family serves both sides.  A SAMPLE is a batch row (an item on the item side, a user on the user side), the
// TABLE is the other side's [N, A, K] tensor (theta / beta), th = tanh(decoder(table)) [N, A, H], zh = tanh(decoder(z))
// [B, A, H], w [N, A] the aspect weights of the table rows.  Per (sample b, table row n, aspect a)
//   s_bna = sigmoid(z_ba . T_na + tanh(zh_ba . th_na)),   p_bn = sum_a w_na s_bna,   nei_ba = sum_n w_na s_bna T_na.
// The forward returns sum_n p_bn, sum_{n in row(b)} log(p_bn + EPS) and nei; the backward receives the gradients g1 [B],
// g2 [B], gN [B, A, K] of the three:
//   d L / d (w s)_bna = q_bna = g1_b + gN_ba . T_na  (+ g2_b / (p_bn + EPS) where n is in row(b)).
// The dense part of q does not need p, so the A aspects are independent launches of one tile pass on the f32 MFMA pipe
// (v_mfma_f32_32x32x2_f32: exact fp32 products, k ascending; K = 25 is padded to 26 by a zero row of the LDS copy); the
// g2 part is sparse and is an owner walk that recomputes the A aspects of one (sample, table row).
// No atomics: partials are added in a fixed order and every output element has one owner; two runs give the same bits.
#include "common.h"
#include "vae_common.h"

namespace chaorec {

constexpr int DV_K = 25;          // latent width (Model/DualVAE.py:37)
constexpr int DV_A = 5;           // aspects (:38)
constexpr int DV_H = 20;          // encoder and decoder hidden width (:48-49)
constexpr int DV_KS = 13;         // MFMA k-steps over K padded to 26
constexpr int DV_HS = 10;         // MFMA k-steps over H
constexpr int DV_AK = DV_A * DV_K, DV_AH = DV_A * DV_H;
constexpr float DV_EPS = 1e-10f;  // (:15)

// ---------------------------------------------------------------------------------------------------------------
// encoder first layer: pre[b, a, :] = bias + sum_{n in row(b)} w[n, a] We_t[n, :].  One workgroup per sample, thread =
// (aspect, column): the 80-byte row We_t[n, :] is gathered once per entry for all A aspects.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void dv_encode_fwd_kernel(const int64_t *__restrict__ ids, int64_t S,
                                                            const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                            const float *__restrict__ We_t, const float *__restrict__ bias,
                                                            const float *__restrict__ w, float *__restrict__ pre) {
  const int t = threadIdx.x;
  if (t >= DV_AH) return;
  const int a = t / DV_H, c = t % DV_H;
  const int64_t b = blockIdx.x, id = ids[b];
  const auto [beg, n_e] = vae_hist_row(rowptr, id, S);
  float acc = 0.f;
  for (int64_t j = 0; j < n_e; ++j) {
    const int64_t n = col[beg + j];
    acc += w[n * DV_A + a] * We_t[n * DV_H + c];
  }
  pre[b * DV_AH + t] = bias[c] + acc;
}

// dWe_t[n, c] = sum_{slots of n} sum_a w[n, a] dpre[slot, a, c]   (lanes 0 .. 19)
// dw[n, a]    = sum_{slots of n} sum_c We_t[n, c] dpre[slot, a, c]  (lanes 32 .. 36): the SPARSE part of d w.
// One wave per table row; every row is written.
__global__ __launch_bounds__(256) void dv_encode_bwd_kernel(int64_t N, const int64_t *__restrict__ tptr, const int32_t *__restrict__ tcol,
                                                            const int64_t *__restrict__ slot_ptr, const int64_t *__restrict__ perm,
                                                            const float *__restrict__ We_t, const float *__restrict__ w,
                                                            const float *__restrict__ dpre, float *__restrict__ dWe_t,
                                                            float *__restrict__ dw) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const bool colw = lane < DV_H, asp = lane >= 32 && lane < 32 + DV_A;
  float wa[DV_A], wrow[DV_H];
#pragma unroll
  for (int a = 0; a < DV_A; ++a) wa[a] = w[n * DV_A + a];
#pragma unroll
  for (int c = 0; c < DV_H; ++c) wrow[c] = We_t[n * DV_H + c];
  float acc = 0.f;
  vae_item_walk(n, tptr, tcol, (const int32_t *)nullptr, slot_ptr, perm, lane, [&](int64_t slot, int) {
    const float *g = dpre + slot * DV_AH;
    if (colw) {
      float v = 0.f;
#pragma unroll
      for (int a = 0; a < DV_A; ++a) v += wa[a] * g[a * DV_H + lane];
      acc += v;
    } else if (asp) {
      float v = 0.f;
#pragma unroll
      for (int c = 0; c < DV_H; ++c) v += wrow[c] * g[(lane - 32) * DV_H + c];
      acc += v;
    }
  });
  if (colw) dWe_t[n * DV_H + lane] = acc;
  if (asp) dw[n * DV_A + (lane - 32)] = acc;
}

// ---------------------------------------------------------------------------------------------------------------
// sample-owned dense passes.  blockIdx = (block of 128 samples, table split, aspect).  Logits TRANSPOSED (A operand =
// the table tile, B operand = the lane's sample), so a lane's accumulator values of a tile belong to ITS sample.
//   BWD = false: psum[split, a, b] = sum_n w s,  pnei[split, b, a, :] = sum_n w s T_n
//   BWD = true : dzp[split, b, a, :] = sum_n dl T_n,  dzhp[split, b, a, :] = sum_n dm th_n  (the dense q)
// Ts row 25 and Hs row 20 are zero: the pad of the k-chain, and what the rows past the width read as an A operand.
// ---------------------------------------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(256) void dv_rows_kernel(const float *__restrict__ z, const float *__restrict__ zh,
                                                      const float *__restrict__ T, const float *__restrict__ th,
                                                      const float *__restrict__ w, int64_t B, int64_t N, int64_t tiles_per_split,
                                                      float *__restrict__ psum, float *__restrict__ pnei,
                                                      const float *__restrict__ g1, const float *__restrict__ gN,
                                                      float *__restrict__ dzp, float *__restrict__ dzhp) {
  constexpr int LD = VAE_TI + 1;
  __shared__ float Ts[DV_K + 1][LD];      // [k][table row]
  __shared__ float Hs[DV_H + 1][LD];      // [h][table row]
  __shared__ float ws[VAE_TI];             // w[n, a] (0 past the end: the column adds nothing)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int a = blockIdx.z;
  const int64_t b = (int64_t)blockIdx.x * VAE_SB + wave * 32 + r;
  const bool live = b < B;
  const int64_t n_tiles = (N + VAE_TI - 1) / VAE_TI;
  const int64_t t_beg = (int64_t)blockIdx.y * tiles_per_split, t_end = min(n_tiles, t_beg + tiles_per_split);
  const int rk = r < DV_K ? r : DV_K, rh = r < DV_H ? r : DV_H;

  float bz[DV_KS], bh[DV_HS], bn[BWD ? DV_KS : 1];
#pragma unroll
  for (int s = 0; s < DV_KS; ++s) {
    const int k = 2 * s + h;
    bz[s] = live && k < DV_K ? z[(b * DV_A + a) * DV_K + k] : 0.f;
    if (BWD) bn[s] = live && k < DV_K ? gN[(b * DV_A + a) * DV_K + k] : 0.f;
  }
#pragma unroll
  for (int s = 0; s < DV_HS; ++s) bh[s] = live ? zh[(b * DV_A + a) * DV_H + 2 * s + h] : 0.f;
  const float my_g1 = BWD && live ? g1[b] : 0.f;
  float ssum = 0.f;
  f32x16 o1 = vae_zero(), o2 = vae_zero();      // nei | dz, dzh

  if (t < LD) {
    Ts[DV_K][t] = 0.f;
    Hs[DV_H][t] = 0.f;
  }
  for (int64_t tile = t_beg; tile < t_end; ++tile) {
    const int64_t n0 = tile * VAE_TI;
    __syncthreads();
    for (int e = t; e < VAE_TI * DV_K; e += 256) {
      const int n = e / DV_K, k = e % DV_K;
      Ts[k][n] = (n0 + n < N) ? T[((n0 + n) * DV_A + a) * DV_K + k] : 0.f;
    }
    for (int e = t; e < VAE_TI * DV_H; e += 256) {
      const int n = e / DV_H, k = e % DV_H;
      Hs[k][n] = (n0 + n < N) ? th[((n0 + n) * DV_A + a) * DV_H + k] : 0.f;
    }
    if (t < VAE_TI) ws[t] = (n0 + t < N) ? w[(n0 + t) * DV_A + a] : 0.f;
    __syncthreads();

#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      f32x16 ad = vae_zero(), am = vae_zero();
#pragma unroll
      for (int s = 0; s < DV_KS; ++s) ad = __builtin_amdgcn_mfma_f32_32x32x2f32(Ts[2 * s + h][32 * jt + r], bz[s], ad, 0, 0, 0);
#pragma unroll
      for (int s = 0; s < DV_HS; ++s) am = __builtin_amdgcn_mfma_f32_32x32x2f32(Hs[2 * s + h][32 * jt + r], bh[s], am, 0, 0, 0);
      if (!BWD) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int n = 32 * jt + vae_row(q, h);
          const float v = ws[n] * sigmoidf_acc(ad[q] + tanhf(am[q]));
          ssum += v;
          o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ts[rk][n], v, o1, 0, 0, 0);
        }
      } else {
        f32x16 an = vae_zero();
#pragma unroll
        for (int s = 0; s < DV_KS; ++s) an = __builtin_amdgcn_mfma_f32_32x32x2f32(Ts[2 * s + h][32 * jt + r], bn[s], an, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int n = 32 * jt + vae_row(q, h);
          const float tm = tanhf(am[q]), sg = sigmoidf_acc(ad[q] + tm);
          const float dl = ws[n] * (my_g1 + an[q]) * (sg * (1.0f - sg));
          const float dm = dl * (1.0f - tm * tm);
          o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Ts[rk][n], dl, o1, 0, 0, 0);
          o2 = __builtin_amdgcn_mfma_f32_32x32x2f32(Hs[rh][n], dm, o2, 0, 0, 0);
        }
      }
    }
  }

  // o1 / o2: row = vae_row(reg, h) (the k or h index), column = the lane's sample
  if (!BWD) {
    const float s2 = __shfl_xor(ssum, 32, 64);     // the two half-waves saw different table rows of the same sample: half 0 first
    if (live && h == 0) psum[((int64_t)blockIdx.y * DV_A + a) * B + b] = ssum + s2;
    if (live) {
      float *out = pnei + (((int64_t)blockIdx.y * B + b) * DV_A + a) * DV_K;
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (vae_row(q, h) < DV_K) out[vae_row(q, h)] = o1[q];
    }
  } else if (live) {
    float *out = dzp + (((int64_t)blockIdx.y * B + b) * DV_A + a) * DV_K;
    float *outh = dzhp + (((int64_t)blockIdx.y * B + b) * DV_A + a) * DV_H;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (vae_row(q, h) < DV_K) out[vae_row(q, h)] = o1[q];
      if (vae_row(q, h) < DV_H) outh[vae_row(q, h)] = o2[q];
    }
  }
}

// the A aspects of one (sample, table row): lane < 25 holds column `lane` of z_ba and T_na, lane < 20 of zh_ba and th_na
// (0 elsewhere) -> s[a], tm[a] = the inner tanh, p = sum_a w_a s_a
__device__ __forceinline__ float dv_pair(const float (&zk)[DV_A], const float (&hk)[DV_A], const float (&tk)[DV_A],
                                         const float (&thk)[DV_A], const float *__restrict__ wrow, float (&s)[DV_A],
                                         float (&tm)[DV_A], float (&wa)[DV_A]) {
  float p = 0.f;
#pragma unroll
  for (int a = 0; a < DV_A; ++a) {
    wa[a] = wrow[a];
    tm[a] = tanhf(wave_sum(hk[a] * thk[a]));
    s[a] = sigmoidf_acc(wave_sum(zk[a] * tk[a]) + tm[a]);
    p += wa[a] * s[a];
  }
  return p;
}

__device__ __forceinline__ void dv_load_row(const float *__restrict__ x25, const float *__restrict__ x20, int64_t row, int lane,
                                            float (&k)[DV_A], float (&hh)[DV_A]) {
#pragma unroll
  for (int a = 0; a < DV_A; ++a) {
    k[a] = lane < DV_K ? x25[(row * DV_A + a) * DV_K + lane] : 0.f;
    hh[a] = lane < DV_H ? x20[(row * DV_A + a) * DV_H + lane] : 0.f;
  }
}

// sum_p[b] and nei[b] from the split partials (fixed order), xlog[b] = sum_{n in row(b)} log(p_bn + EPS): a wave per sample
__global__ __launch_bounds__(64) void dv_fwd_finish_kernel(const int64_t *__restrict__ ids, int64_t B, int64_t S,
                                                           const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const float *__restrict__ z, const float *__restrict__ zh,
                                                           const float *__restrict__ T, const float *__restrict__ th,
                                                           const float *__restrict__ w, const float *__restrict__ psum,
                                                           const float *__restrict__ pnei, int64_t splits, float *__restrict__ sum_p,
                                                           float *__restrict__ xlog, float *__restrict__ nei) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  double sp = 0.0;
  for (int64_t e = lane; e < splits * DV_A; e += 64) sp += (double)psum[e * B + b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sp += __shfl_xor(sp, off, 64);
  for (int e = lane; e < DV_AK; e += 64) {
    float v = 0.f;
    for (int64_t s = 0; s < splits; ++s) v += pnei[(s * B + b) * DV_AK + e];
    nei[b * DV_AK + e] = v;
  }
  float zk[DV_A], hk[DV_A];
  dv_load_row(z, zh, b, lane, zk, hk);
  const int64_t id = ids[b];
  const auto [beg, n_e] = vae_hist_row(rowptr, id, S);
  double part = 0.0;
  for (int64_t j = 0; j < n_e; ++j) {
    const int64_t n = col[beg + j];
    float tk[DV_A], thk[DV_A], s[DV_A], tm[DV_A], wa[DV_A];
    dv_load_row(T, th, n, lane, tk, thk);
    const float p = dv_pair(zk, hk, tk, thk, w + n * DV_A, s, tm, wa);
    part += log((double)(p + DV_EPS));
  }
  if (lane == 0) {
    sum_p[b] = (float)sp;
    xlog[b] = (float)part;
  }
}

// d z_ba, d zh_ba = the splits (ascending) + the history walk with q = g2_b / (p_bn + EPS)
__global__ __launch_bounds__(64) void dv_bwd_finish_kernel(const int64_t *__restrict__ ids, int64_t B, int64_t S,
                                                           const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                           const float *__restrict__ z, const float *__restrict__ zh,
                                                           const float *__restrict__ T, const float *__restrict__ th,
                                                           const float *__restrict__ w, const float *__restrict__ g2,
                                                           const float *__restrict__ dzp, const float *__restrict__ dzhp, int64_t splits,
                                                           float *__restrict__ dz, float *__restrict__ dzh) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  float zk[DV_A], hk[DV_A], vz[DV_A], vh[DV_A];
  dv_load_row(z, zh, b, lane, zk, hk);
#pragma unroll
  for (int a = 0; a < DV_A; ++a) vz[a] = vh[a] = 0.f;
  for (int64_t s = 0; s < splits; ++s)
#pragma unroll
    for (int a = 0; a < DV_A; ++a) {
      if (lane < DV_K) vz[a] += dzp[((s * B + b) * DV_A + a) * DV_K + lane];
      if (lane < DV_H) vh[a] += dzhp[((s * B + b) * DV_A + a) * DV_H + lane];
    }
  const int64_t id = ids[b];
  const auto [beg, n_e] = vae_hist_row(rowptr, id, S);
  const float g = g2[b];
  for (int64_t j = 0; j < n_e; ++j) {
    const int64_t n = col[beg + j];
    float tk[DV_A], thk[DV_A], s[DV_A], tm[DV_A], wa[DV_A];
    dv_load_row(T, th, n, lane, tk, thk);
    const float p = dv_pair(zk, hk, tk, thk, w + n * DV_A, s, tm, wa);
    const float f = g / (p + DV_EPS);
#pragma unroll
    for (int a = 0; a < DV_A; ++a) {
      const float dl = wa[a] * f * (s[a] * (1.0f - s[a]));
      vz[a] += dl * tk[a];
      vh[a] += dl * (1.0f - tm[a] * tm[a]) * thk[a];
    }
  }
#pragma unroll
  for (int a = 0; a < DV_A; ++a) {
    if (lane < DV_K) dz[(b * DV_A + a) * DV_K + lane] = vz[a];
    if (lane < DV_H) dzh[(b * DV_A + a) * DV_H + lane] = vh[a];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// table-owned dense passes: a workgroup owns 64 table rows and loops over ALL sample blocks (128 samples, a wave 32).
// Logits as [sample][table row] (A operand = the sample block, B operand = the table tile): lane & 31 = the table row.
//   SCORES = false, blockIdx = (table block, aspect): d th[n, a, :] = sum_b dm zh_ba, d w[n, a] = sum_b s q (dense q)
//   SCORES = true,  blockIdx = (table block, sample block): out[sample, n] = sum_a w_na s_bna with the weight as given
// Zs column 25 and ZHs column 20 are zero (the k pad; the columns past the width of the B operand of d th).
// ---------------------------------------------------------------------------------------------------------------
template <bool SCORES>
__global__ __launch_bounds__(256) void dv_table_kernel(const float *__restrict__ z, const float *__restrict__ zh,
                                                       const float *__restrict__ T, const float *__restrict__ th,
                                                       const float *__restrict__ w, int64_t B, int64_t N,
                                                       const float *__restrict__ g1, const float *__restrict__ gN,
                                                       float *__restrict__ dth, float *__restrict__ dw, float *__restrict__ scores) {
  constexpr int LW = VAE_TW + 1, LZ = DV_K + 2, LH = DV_H + 1;
  __shared__ float Ws[DV_K + 1][LW];      // [k][table row], row 25 zero
  __shared__ float Hs[DV_H][LW];          // [h][table row]
  __shared__ float Zs[VAE_SB][LZ];         // [sample][k], column 25 zero
  __shared__ float Gs[SCORES ? 1 : VAE_SB][LZ];
  __shared__ float ZHs[VAE_SB][LH];        // [sample][h], column 20 zero
  __shared__ float g1s[VAE_SB];
  __shared__ float wcol[VAE_TW];
  __shared__ float bsum[4][VAE_TW];
  float (*Rs)[33] = reinterpret_cast<float (*)[33]>(&Zs[0][0]);   // [table row][h]: the waves' sums, once Zs is done with
  static_assert(VAE_TW * 33 <= VAE_SB * LZ, "the reduction buffer lives in Zs");
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int64_t n0 = (int64_t)blockIdx.x * VAE_TW;
  const int rh = r < DV_H ? r : DV_H;
  f32x16 acc2[2] = {vae_zero(), vae_zero()};      // d th | the scores
  if (t < VAE_TW) {
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) bsum[wv][t] = 0.f;
  }

  const int a_beg = SCORES ? 0 : (int)blockIdx.y, a_end = SCORES ? DV_A : a_beg + 1;
  const int64_t s_beg = SCORES ? (int64_t)blockIdx.y * VAE_SB : 0, s_end = SCORES ? min(B, s_beg + VAE_SB) : B;
  for (int a = a_beg; a < a_end; ++a) {
    __syncthreads();
    for (int e = t; e < VAE_TW * DV_K; e += 256) {
      const int n = e / DV_K, k = e % DV_K;
      Ws[k][n] = (n0 + n < N) ? T[((n0 + n) * DV_A + a) * DV_K + k] : 0.f;
    }
    for (int e = t; e < VAE_TW * DV_H; e += 256) {
      const int n = e / DV_H, k = e % DV_H;
      Hs[k][n] = (n0 + n < N) ? th[((n0 + n) * DV_A + a) * DV_H + k] : 0.f;
    }
    if (t < VAE_TW) {
      Ws[DV_K][t] = 0.f;
      wcol[t] = (n0 + t < N) ? w[(n0 + t) * DV_A + a] : 0.f;
    }
    for (int64_t s0 = s_beg; s0 < s_end; s0 += VAE_SB) {
      __syncthreads();
      for (int e = t; e < VAE_SB * (DV_K + 1); e += 256) {
        const int row = e / (DV_K + 1), k = e % (DV_K + 1);
        const bool in = s0 + row < B && k < DV_K;
        Zs[row][k] = in ? z[((s0 + row) * DV_A + a) * DV_K + k] : 0.f;
        if (!SCORES) Gs[row][k] = in ? gN[((s0 + row) * DV_A + a) * DV_K + k] : 0.f;
      }
      for (int e = t; e < VAE_SB * (DV_H + 1); e += 256) {
        const int row = e / (DV_H + 1), k = e % (DV_H + 1);
        ZHs[row][k] = (s0 + row < B && k < DV_H) ? zh[((s0 + row) * DV_A + a) * DV_H + k] : 0.f;
      }
      if (!SCORES && t < VAE_SB) g1s[t] = (s0 + t < B) ? g1[s0 + t] : 0.f;      // a sample past the end: q = 0
      __syncthreads();
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const float wl = wcol[32 * jt + r];
        f32x16 ad = vae_zero(), am = vae_zero();
#pragma unroll
        for (int s = 0; s < DV_KS; ++s)
          ad = __builtin_amdgcn_mfma_f32_32x32x2f32(Zs[wave * 32 + r][2 * s + h], Ws[2 * s + h][32 * jt + r], ad, 0, 0, 0);
#pragma unroll
        for (int s = 0; s < DV_HS; ++s)
          am = __builtin_amdgcn_mfma_f32_32x32x2f32(ZHs[wave * 32 + r][2 * s + h], Hs[2 * s + h][32 * jt + r], am, 0, 0, 0);
        if (SCORES) {
#pragma unroll
          for (int q = 0; q < 16; ++q) acc2[jt][q] += wl * sigmoidf_acc(ad[q] + tanhf(am[q]));
        } else {
          f32x16 an = vae_zero();
#pragma unroll
          for (int s = 0; s < DV_KS; ++s)
            an = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[wave * 32 + r][2 * s + h], Ws[2 * s + h][32 * jt + r], an, 0, 0, 0);
          float bk = 0.f;
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int sm = wave * 32 + vae_row(q, h);
            const float tm = tanhf(am[q]), sg = sigmoidf_acc(ad[q] + tm);
            const float qq = g1s[sm] + an[q];
            bk += sg * qq;
            const float dm = wl * qq * (sg * (1.0f - sg)) * (1.0f - tm * tm);
            acc2[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(dm, ZHs[sm][rh], acc2[jt], 0, 0, 0);
          }
          bk += __shfl_xor(bk, 32, 64);
          if (h == 0) bsum[wave][32 * jt + r] += bk;      // (always this lane: an ordered running sum)
        }
      }
    }
  }

  if (SCORES) {
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
      const int64_t n = n0 + 32 * jt + r;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t row = s_beg + wave * 32 + vae_row(q, h);
        if (row < B && n < N) scores[row * N + n] = acc2[jt][q];
      }
    }
    return;
  }

  // waves 0..3 in order; acc2[jt]: row = table row 32 jt + vae_row(reg, h), column = h index r
  const int a = a_beg;
  for (int wv = 0; wv < 4; ++wv) {
    __syncthreads();
    if (wave == wv) {
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          float *dst = &Rs[32 * jt + vae_row(q, h)][r];
          *dst = (wv ? *dst : 0.f) + acc2[jt][q];
        }
    }
  }
  __syncthreads();
  for (int e = t; e < VAE_TW * DV_H; e += 256) {
    const int n = e / DV_H, k = e % DV_H;
    if (n0 + n < N) dth[((n0 + n) * DV_A + a) * DV_H + k] = Rs[n][k];
  }
  if (t < VAE_TW && n0 + t < N) dw[(n0 + t) * DV_A + a] = ((bsum[0][t] + bsum[1][t]) + bsum[2][t]) + bsum[3][t];
}

// the sparse q = g2_b / (p_bn + EPS) of table row n's samples, ADDED to what the dense pass wrote (one owner per row):
// d th[n, a, :] += sum dm zh_ba,  d w[n, a] += sum s_a q.  One wave per table row.
__global__ __launch_bounds__(256) void dv_table_sparse_kernel(int64_t N, const int64_t *__restrict__ tptr, const int32_t *__restrict__ tcol,
                                                              const int64_t *__restrict__ slot_ptr, const int64_t *__restrict__ perm,
                                                              const float *__restrict__ z, const float *__restrict__ zh,
                                                              const float *__restrict__ T, const float *__restrict__ th,
                                                              const float *__restrict__ w, const float *__restrict__ g2,
                                                              float *__restrict__ dth, float *__restrict__ dw) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  float tk[DV_A], thk[DV_A], vh[DV_A], vw[DV_A];
  dv_load_row(T, th, n, lane, tk, thk);
#pragma unroll
  for (int a = 0; a < DV_A; ++a) vh[a] = vw[a] = 0.f;
  bool any = false;
  vae_item_walk(n, tptr, tcol, (const int32_t *)nullptr, slot_ptr, perm, lane, [&](int64_t slot, int) {
    float zk[DV_A], hk[DV_A], s[DV_A], tm[DV_A], wa[DV_A];
    dv_load_row(z, zh, slot, lane, zk, hk);
    const float p = dv_pair(zk, hk, tk, thk, w + n * DV_A, s, tm, wa);
    const float f = g2[slot] / (p + DV_EPS);
#pragma unroll
    for (int a = 0; a < DV_A; ++a) {
      vw[a] += s[a] * f;
      vh[a] += wa[a] * f * (s[a] * (1.0f - s[a])) * (1.0f - tm[a] * tm[a]) * hk[a];
    }
    any = true;
  });
  if (!any) return;
#pragma unroll
  for (int a = 0; a < DV_A; ++a) {
    if (lane < DV_H) dth[(n * DV_A + a) * DV_H + lane] += vh[a];
    if (lane == a) dw[n * DV_A + a] += vw[a];
  }
}

// table[id_b] = z_b, mu_table[id_b] = mu_b; where an id repeats in the batch, the sample at the HIGHEST position writes
// (the last slot of the id's stable-sorted slot list) and the others do not
__global__ __launch_bounds__(128) void dv_writeback_kernel(const int64_t *__restrict__ ids, int64_t S, const int64_t *__restrict__ slot_ptr,
                                                           const int64_t *__restrict__ perm, const float *__restrict__ z,
                                                           const float *__restrict__ mu, float *__restrict__ table,
                                                           float *__restrict__ mu_table) {
  const int64_t b = blockIdx.x, id = ids[b];
  if (id < 0 || id >= S) return;
  const int64_t hi = slot_ptr[id + 1];
  if (hi <= slot_ptr[id] || perm[hi - 1] != b) return;
  const int t = threadIdx.x;
  if (t < DV_AK) {
    table[id * DV_AK + t] = z[b * DV_AK + t];
    mu_table[id * DV_AK + t] = mu[b * DV_AK + t];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// the small Linears' weight and bias gradients, gw[m, n] = sum_r gy[r, m] x[r, n], gb[m] = sum_r gy[r, m] (M, N <= 32,
// R = B * 5 or N * 5 rows): the products are exact in double and the sum is rounded ONCE -- an fp32 chain over 10^3 .. 10^5
// sign-changing terms sits at 1e-6 of the largest element, above what the reference's blocked sums leave.
// blockIdx = (m, row split); thread = (row lane of 8, n lane of 32; n lane 31 sums gy alone for the bias).
// ---------------------------------------------------------------------------------------------------------------
constexpr int DV_GW_ROWS = 2048;      // rows per split
__global__ __launch_bounds__(256) void dv_gw_partial_kernel(const float *__restrict__ gy, const float *__restrict__ x, int64_t R, int M,
                                                            int N, double *__restrict__ partial) {
  __shared__ double red[8][32];
  const int t = threadIdx.x, nl = t & 31, rl = t >> 5, m = blockIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * DV_GW_ROWS, r1 = min(R, r0 + DV_GW_ROWS);
  double acc = 0.0;
  if (nl < N || nl == 31)
    for (int64_t r = r0 + rl; r < r1; r += 8) {
      const double g = (double)gy[r * M + m];
      acc += nl == 31 ? g : g * (double)x[r * N + nl];
    }
  red[rl][nl] = acc;
  __syncthreads();
  if (t < 32) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) v += red[q][t];
    partial[((int64_t)blockIdx.y * M + m) * 32 + t] = v;
  }
}
__global__ __launch_bounds__(32) void dv_gw_finish_kernel(const double *__restrict__ partial, int64_t splits, int M, int N,
                                                          float *__restrict__ gw, float *__restrict__ gb) {
  const int nl = threadIdx.x, m = blockIdx.x;
  double v = 0.0;
  for (int64_t s = 0; s < splits; ++s) v += partial[(s * M + m) * 32 + nl];
  if (nl < N) gw[m * N + nl] = (float)v;
  if (nl == 31) gb[m] = (float)v;
}

// the KL's elements -0.5 (1 + 2 log std - mu^2 - std^2), std = sigmoid(sp), evaluated and summed in double from the fp32
// mu and PRE-sigmoid sp: fp32 log / sigmoid carry a fraction of an ulp of bias that B * 125 like-signed terms do not average
// away, and the scalar's own bound sits below one fp32 ulp.  partial[block]: fixed-order sums.
constexpr int DV_KL_BLOCKS = 64;
__global__ __launch_bounds__(256) void dv_kl_partial_kernel(const float *__restrict__ mu, const float *__restrict__ sp, int64_t n,
                                                            double *__restrict__ partial) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double a = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + t; e < n; e += (int64_t)gridDim.x * 256) {
    const double x = (double)sp[e], m = (double)mu[e];
    const double ls = x >= 0.0 ? -log1p(exp(-x)) : x - log1p(exp(x));      // log sigmoid(x)
    a += -0.5 * (1.0 + 2.0 * ls - m * m - exp(2.0 * ls));
  }
  block_sum_f64(a, red);
  if (t == 0) partial[blockIdx.x] = red[0];
}

// one side's scalars from double sums, each rounded once: out[0] = kl_weight kl - ll + ssl_reg cl, out[1] = kl =
// sum(partial) / (5 B), out[2] = ll = (sum xlog - sum sum_p) / B
__global__ __launch_bounds__(256) void dv_loss_kernel(const double *__restrict__ partial, int n_partial, const float *__restrict__ xlog,
                                                      const float *__restrict__ sum_p, int64_t B, const float *__restrict__ cl,
                                                      float kl_weight, float ssl_reg, float *__restrict__ out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double b = 0.0;
  for (int64_t e = t; e < B; e += 256) b += (double)xlog[e] - (double)sum_p[e];
  block_sum_f64(b, red);
  if (t == 0) {
    double a = 0.0;
    for (int p = 0; p < n_partial; ++p) a += partial[p];
    const double kl = a / (double)(DV_A * B), ll = red[0] / (double)B;
    out[0] = (float)((double)kl_weight * kl - ll + (double)ssl_reg * (double)cl[0]);
    out[1] = (float)kl;
    out[2] = (float)ll;
  }
}

static int dv_shape(const char *what, int32_t k, int32_t a, int32_t hidden) {
  if (k != DV_K || a != DV_A || hidden != DV_H)
    return fail(CHAOREC_E_INVALID, "%s: k=%d a=%d hidden=%d, the kernels tile k=%d a=%d hidden=%d", what, (int)k, (int)a, (int)hidden,
                DV_K, DV_A, DV_H);
  return CHAOREC_OK;
}

}  // namespace chaorec

using namespace chaorec;

extern "C" int64_t chaorec_dualvae_splits(int64_t B, int64_t N) {
  if (B <= 0 || N <= 0) return 1;
  int64_t s, tp;
  vae_split_plan(B, N, DV_A, s, tp);
  return s;
}

extern "C" int chaorec_dualvae_check_shape(int32_t k, int32_t a, int32_t hidden) { return dv_shape("dualvae_check_shape", k, a, hidden); }

extern "C" int chaorec_dualvae_tick(int64_t *state, void *stream) {
  return launch_step_tick("dualvae_tick", state, stream);      // the step the device-drawn epsilon is keyed by
}

extern "C" int chaorec_dualvae_encode_fwd_f32(const int64_t *ids, int64_t B, int64_t S, const int64_t *rowptr, const int32_t *col,
                                              int64_t N, const float *We_t, const float *bias, const float *w, float *pre,
                                              void *stream) {
  if (!ids || !rowptr || !col || !We_t || !bias || !w || !pre) return fail(CHAOREC_E_INVALID, "dualvae_encode_fwd: NULL argument");
  if (B <= 0 || S <= 0 || N <= 0) return fail(CHAOREC_E_INVALID, "dualvae_encode_fwd: B=%lld S=%lld N=%lld", (long long)B, (long long)S, (long long)N);
  hipLaunchKernelGGL(dv_encode_fwd_kernel, dim3((unsigned)B), dim3(128), 0, (hipStream_t)stream, ids, S, rowptr, col, We_t, bias, w, pre);
  return check_launch("dv_encode_fwd_kernel");
}

extern "C" int chaorec_dualvae_encode_bwd_f32(int64_t B, int64_t N, const int64_t *tptr, const int32_t *tcol, const int64_t *slot_ptr,
                                              const int64_t *perm, const float *We_t, const float *w, const float *dpre, float *dWe_t,
                                              float *dw, void *stream) {
  if (!tptr || !tcol || !slot_ptr || !perm || !We_t || !w || !dpre || !dWe_t || !dw)
    return fail(CHAOREC_E_INVALID, "dualvae_encode_bwd: NULL argument");
  if (B <= 0 || N <= 0) return fail(CHAOREC_E_INVALID, "dualvae_encode_bwd: B=%lld N=%lld", (long long)B, (long long)N);
  hipLaunchKernelGGL(dv_encode_bwd_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, N, tptr, tcol, slot_ptr, perm,
                     We_t, w, dpre, dWe_t, dw);
  return check_launch("dv_encode_bwd_kernel");
}

extern "C" int chaorec_dualvae_dense_fwd_f32(const int64_t *ids, int64_t B, int64_t S, const int64_t *rowptr, const int32_t *col,
                                             const float *z, const float *zh, const float *table, const float *th, const float *w,
                                             int64_t N, float *psum, float *pnei, int64_t splits, float *sum_p, float *xlog, float *nei,
                                             void *stream) {
  if (!ids || !rowptr || !col || !z || !zh || !table || !th || !w || !psum || !pnei || !sum_p || !xlog || !nei)
    return fail(CHAOREC_E_INVALID, "dualvae_dense_fwd: NULL argument");
  if (B <= 0 || S <= 0 || N <= 0) return fail(CHAOREC_E_INVALID, "dualvae_dense_fwd: B=%lld S=%lld N=%lld", (long long)B, (long long)S, (long long)N);
  int64_t s, tp;
  vae_split_plan(B, N, DV_A, s, tp);
  if (splits != s) return fail(CHAOREC_E_WORKSPACE, "dualvae_dense_fwd: splits %lld, chaorec_dualvae_splits says %lld", (long long)splits, (long long)s);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((B + VAE_SB - 1) / VAE_SB), (unsigned)s, DV_A);
  hipLaunchKernelGGL((dv_rows_kernel<false>), grid, dim3(256), 0, st, z, zh, table, th, w, B, N, tp, psum, pnei, (const float *)nullptr,
                     (const float *)nullptr, (float *)nullptr, (float *)nullptr);
  int rc = check_launch("dv_rows_kernel<fwd>");
  if (rc) return rc;
  hipLaunchKernelGGL(dv_fwd_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, ids, B, S, rowptr, col, z, zh, table, th, w,
                     (const float *)psum, (const float *)pnei, s, sum_p, xlog, nei);
  return check_launch("dv_fwd_finish_kernel");
}

extern "C" int chaorec_dualvae_dense_bwd_f32(const int64_t *ids, int64_t B, int64_t S, const int64_t *rowptr, const int32_t *col,
                                             const int64_t *tptr, const int32_t *tcol, const int64_t *slot_ptr, const int64_t *perm,
                                             const float *z, const float *zh, const float *table, const float *th, const float *w,
                                             int64_t N, const float *g1, const float *g2, const float *gN, float *dzp, float *dzhp,
                                             int64_t splits, float *dz, float *dzh, float *dth, float *dw, void *stream) {
  if (!ids || !rowptr || !col || !tptr || !tcol || !slot_ptr || !perm || !z || !zh || !table || !th || !w || !g1 || !g2 || !gN || !dzp ||
      !dzhp || !dz || !dzh || !dth || !dw)
    return fail(CHAOREC_E_INVALID, "dualvae_dense_bwd: NULL argument");
  if (B <= 0 || S <= 0 || N <= 0) return fail(CHAOREC_E_INVALID, "dualvae_dense_bwd: B=%lld S=%lld N=%lld", (long long)B, (long long)S, (long long)N);
  int64_t s, tp;
  vae_split_plan(B, N, DV_A, s, tp);
  if (splits != s) return fail(CHAOREC_E_WORKSPACE, "dualvae_dense_bwd: splits %lld, chaorec_dualvae_splits says %lld", (long long)splits, (long long)s);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((B + VAE_SB - 1) / VAE_SB), (unsigned)s, DV_A);
  hipLaunchKernelGGL((dv_rows_kernel<true>), grid, dim3(256), 0, st, z, zh, table, th, w, B, N, tp, (float *)nullptr, (float *)nullptr, g1, gN,
                     dzp, dzhp);
  int rc = check_launch("dv_rows_kernel<bwd>");
  if (rc) return rc;
  hipLaunchKernelGGL(dv_bwd_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, ids, B, S, rowptr, col, z, zh, table, th, w, g2,
                     (const float *)dzp, (const float *)dzhp, s, dz, dzh);
  rc = check_launch("dv_bwd_finish_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL((dv_table_kernel<false>), dim3((unsigned)((N + VAE_TW - 1) / VAE_TW), DV_A), dim3(256), 0, st, z, zh, table, th, w, B, N,
                     g1, gN, dth, dw, (float *)nullptr);
  rc = check_launch("dv_table_kernel<grad>");
  if (rc) return rc;
  hipLaunchKernelGGL(dv_table_sparse_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, N, tptr, tcol, slot_ptr, perm, z, zh, table, th,
                     w, g2, dth, dw);
  return check_launch("dv_table_sparse_kernel");
}

extern "C" int chaorec_dualvae_writeback_f32(const int64_t *ids, int64_t B, int64_t S, const int64_t *slot_ptr, const int64_t *perm,
                                             const float *z, const float *mu, float *table, float *mu_table, void *stream) {
  if (!ids || !slot_ptr || !perm || !z || !mu || !table || !mu_table) return fail(CHAOREC_E_INVALID, "dualvae_writeback: NULL argument");
  if (B <= 0 || S <= 0) return fail(CHAOREC_E_INVALID, "dualvae_writeback: B=%lld S=%lld", (long long)B, (long long)S);
  hipLaunchKernelGGL(dv_writeback_kernel, dim3((unsigned)B), dim3(128), 0, (hipStream_t)stream, ids, S, slot_ptr, perm, z, mu, table, mu_table);
  return check_launch("dv_writeback_kernel");
}

extern "C" int chaorec_dualvae_scores_f32(const float *z, const float *zh, int64_t n_users, const float *table, const float *th,
                                          const float *w, int64_t I, int64_t user_begin, const int64_t *hist_rowptr,
                                          const int64_t *hist_col, float mask_value, float *scores, size_t scores_bytes, void *stream) {
  if (!z || !zh || !table || !th || !w || !hist_rowptr || !hist_col || !scores) return fail(CHAOREC_E_INVALID, "dualvae_scores: NULL argument");
  if (n_users <= 0 || I <= 0 || user_begin < 0)
    return fail(CHAOREC_E_INVALID, "dualvae_scores: n_users=%lld I=%lld user_begin=%lld", (long long)n_users, (long long)I, (long long)user_begin);
  const size_t need = (size_t)n_users * (size_t)I * sizeof(float);
  if (scores_bytes < need || need > (size_t)CHAOREC_DUALVAE_STAGING_BYTES)
    return fail(CHAOREC_E_WORKSPACE, "dualvae_scores: staging of %zu bytes (given %zu, cap %zu)", need, scores_bytes, (size_t)CHAOREC_DUALVAE_STAGING_BYTES);
  const int64_t sblocks = (n_users + VAE_SB - 1) / VAE_SB;
  if (sblocks > 65535) return fail(CHAOREC_E_INVALID, "dualvae_scores: %lld users in one range", (long long)n_users);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((dv_table_kernel<true>), dim3((unsigned)((I + VAE_TW - 1) / VAE_TW), (unsigned)sblocks), dim3(256), 0, st, z, zh, table, th,
                     w, n_users, I, (const float *)nullptr, (const float *)nullptr, (float *)nullptr, (float *)nullptr, scores);
  int rc = check_launch("dv_table_kernel<scores>");
  if (rc) return rc;
  hipLaunchKernelGGL(vae_mask_kernel<>, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, scores, user_begin, user_begin + n_users, I,
                     hist_rowptr, hist_col, mask_value);
  return check_launch("vae_mask_kernel");
}

extern "C" size_t chaorec_dualvae_linear_bwd_workspace_bytes(int64_t R, int32_t M) {
  const int64_t splits = R > 0 ? (R + DV_GW_ROWS - 1) / DV_GW_ROWS : 1;
  return (size_t)splits * (size_t)(M > 0 ? M : 1) * 32 * sizeof(double);
}

extern "C" int chaorec_dualvae_linear_bwd_f32(const float *gy, const float *x, int64_t R, int32_t M, int32_t N, float *gw, float *gb,
                                              void *workspace, size_t workspace_bytes, void *stream) {
  if (!gy || !x || !gw || !gb || !workspace) return fail(CHAOREC_E_INVALID, "dualvae_linear_bwd: NULL argument");
  if (R <= 0 || M < 1 || M > 32 || N < 1 || N > 31)
    return fail(CHAOREC_E_INVALID, "dualvae_linear_bwd: R=%lld M=%d N=%d (1 <= M <= 32, 1 <= N <= 31)", (long long)R, (int)M, (int)N);
  const int64_t splits = (R + DV_GW_ROWS - 1) / DV_GW_ROWS;
  if (splits > 65535) return fail(CHAOREC_E_INVALID, "dualvae_linear_bwd: R=%lld too large", (long long)R);
  if (workspace_bytes < chaorec_dualvae_linear_bwd_workspace_bytes(R, M) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return fail(CHAOREC_E_WORKSPACE, "dualvae_linear_bwd: workspace %zu < %zu (8-byte aligned)", workspace_bytes,
                chaorec_dualvae_linear_bwd_workspace_bytes(R, M));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dv_gw_partial_kernel, dim3((unsigned)M, (unsigned)splits), dim3(256), 0, st, gy, x, R, (int)M, (int)N, (double *)workspace);
  int rc = check_launch("dv_gw_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(dv_gw_finish_kernel, dim3((unsigned)M), dim3(32), 0, st, (const double *)workspace, splits, (int)M, (int)N, gw, gb);
  return check_launch("dv_gw_finish_kernel");
}

extern "C" int chaorec_dualvae_loss_f32(const float *mu, const float *std_pre, int64_t n_kl, const float *xlog, const float *sum_p,
                                        int64_t B, const float *cl, float kl_weight, float ssl_reg, float *out, void *workspace,
                                        size_t workspace_bytes, void *stream) {
  if (!mu || !std_pre || !xlog || !sum_p || !cl || !out || !workspace) return fail(CHAOREC_E_INVALID, "dualvae_loss: NULL argument");
  if (B <= 0 || n_kl <= 0) return fail(CHAOREC_E_INVALID, "dualvae_loss: B=%lld n_kl=%lld", (long long)B, (long long)n_kl);
  if (workspace_bytes < DV_KL_BLOCKS * sizeof(double) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return fail(CHAOREC_E_WORKSPACE, "dualvae_loss: workspace %zu < %zu (8-byte aligned)", workspace_bytes, DV_KL_BLOCKS * sizeof(double));
  int64_t nb = (n_kl + 4095) / 4096;
  if (nb > DV_KL_BLOCKS) nb = DV_KL_BLOCKS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dv_kl_partial_kernel, dim3((unsigned)nb), dim3(256), 0, st, mu, std_pre, n_kl, (double *)workspace);
  int rc = check_launch("dv_kl_partial_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(dv_loss_kernel, dim3(1), dim3(256), 0, st, (const double *)workspace, (int)nb, xlog, sum_p, B, cl, kl_weight, ssl_reg, out);
  return check_launch("dv_loss_kernel");
}
