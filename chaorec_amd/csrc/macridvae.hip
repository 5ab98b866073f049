// MacridVAE (Model/MacridVAE.py): the per-concept history-row encoder and the mixture-of-concepts likelihood without any
// [B, I] or [B, K, I] buffer.
//
// The reference builds, for each of its K = 10 concepts, a [B, I] weighted input, a [B, I] logit matrix and a [B, I]
// probability matrix (Model/MacridVAE.py:100-123).  Here
//   cates, items   one pass over the item rows (normalise, K logits against the normalised cores, Gumbel noise, softmax)
//   a [B, K, 600]  one gather of the 2 400-byte row W1_t[i, :] per (sample, kept entry) feeds all K accumulators
//   likelihood     p_bi = sum_k c_ik exp(l_bik), l = zh_bk . items_i / tau, recomputed tile by tile on the f32 MFMA pipe
//                  (v_mfma_f32_32x32x2_f32: exact fp32 products, k-ascending chain, as multvae.hip).
// |l| <= 1 / tau = 10 (both factors are unit vectors), so exp(l) is in [4.5e-5, 2.2e4]: NO running maximum is kept.
// sum_i p_bi is LINEAR in k, and so is the dense part of every gradient,
//   w_bi r_bik = g n_b exp(l_bik) / (B S_b)  -  g x_bi exp(l_bik) / (B p_bi),      S_b = sum_i p_bi,
// (p_bi cancels in the dense term), so the (sample, concept) pairs are independent ROWS of one MultVAE-like pass: the
// sample-owned passes (S_b, d zh) run over B K rows with the per-(item, k) weight c_ik; the item-owned pass (d items,
// d cates) loops over all rows; the sparse x_bi terms are owner walks that recompute the K logits of one (sample, item).
// No atomics, no memset: partials are added in a fixed order; two runs give the same bits.
#include "common.h"
#include "vae_common.h"

namespace chaorec {

constexpr int MC_D = 64;          // dim_E the kernels tile
constexpr int MC_K = 10;          // kfac (Model/MacridVAE.py:27)
constexpr int MC_H = 600;         // encoder hidden width (:28)
constexpr int MC_H4 = MC_H / 4;
static_assert(MC_D == VAE_D, "the staging helpers move rows of dim_E floats");
constexpr uint64_t MC_SALT_KEEP = 0x6D61637269643031ull, MC_SALT_GUMBEL = 0x6D61637269643032ull, MC_SALT_EPS = 0x6D61637269643033ull;

// the uniform keeps 23 bits here (MultVAE's keeps 24): the streams the goldens were drawn from
constexpr int MC_BITS = 23;
using McKeep = VaeKeep<MC_BITS>;

// Model/MacridVAE.py:135-137: `update` is incremented BEFORE the anneal is read.  state[0] = update, state[1] = the
// count this step's draws are keyed by (the same number).
__global__ void mc_tick_kernel(int64_t *state, float *anneal, float cap, int64_t total) {
  if (threadIdx.x || blockIdx.x) return;
  const int64_t c = state[0] + 1;
  state[0] = c;
  state[1] = c;
  anneal[0] = vae_anneal(c, total, cap);
}

// ---------------------------------------------------------------------------------------------------------------
// concept weights (Model/MacridVAE.py:76-77, :86-94): one wave per item, lane = column
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void mc_load_cores(const float *__restrict__ Kemb, float (*cs)[MC_D], float *cinv) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = wave; k < MC_K; k += 4) {
    const float x = Kemb[k * MC_D + lane];
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(x * x)), 1e-12f);
    cs[k][lane] = x * inv;
    if (lane == 0) cinv[k] = inv;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void mc_concept_fwd_kernel(const float *__restrict__ E, const float *__restrict__ Kemb, int64_t I,
                                                             float inv_tau, const float *__restrict__ gumbel_in, int training,
                                                             uint64_t seed, const int64_t *__restrict__ state,
                                                             float *__restrict__ items, float *__restrict__ cates) {
  __shared__ float cs[MC_K][MC_D];
  __shared__ float cinv[MC_K];
  mc_load_cores(Kemb, cs, cinv);
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= I) return;
  const float x = E[i * MC_D + lane];
  const float it = x / fmaxf(sqrtf(wave_sum(x * x)), 1e-12f);
  items[i * MC_D + lane] = it;
  const uint64_t key = training && !gumbel_in ? draw_key(seed, (uint64_t)state[1], MC_SALT_GUMBEL) : 0;
  float l[MC_K], m = -INFINITY;
#pragma unroll
  for (int k = 0; k < MC_K; ++k) {
    l[k] = wave_sum(it * cs[k][lane]) * inv_tau;
    if (training)      // g = -log(Exp(1)) (F.gumbel_softmax, tau = 1): Exp(1) = -log(u)
      l[k] += gumbel_in ? gumbel_in[i * MC_K + k] : -logf(-logf(draw_uniform<MC_BITS>(key, (uint64_t)i, (uint64_t)k)));
    m = fmaxf(m, l[k]);
  }
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < MC_K; ++k) {
    l[k] = expf(l[k] - m);
    sum += l[k];
  }
  float mine = 0.f;
#pragma unroll
  for (int k = 0; k < MC_K; ++k)
    if (lane == k) mine = l[k] / sum;
  if (lane < MC_K) cates[i * MC_K + lane] = mine;
}

// backward: dE [I, D] and per-workgroup partials of d(normalised cores) [n_blocks, K, D] (64 items per workgroup)
__global__ __launch_bounds__(256) void mc_concept_bwd_kernel(const float *__restrict__ E, const float *__restrict__ Kemb, int64_t I,
                                                             float inv_tau, const float *__restrict__ cates,
                                                             const float *__restrict__ d_items, const float *__restrict__ d_cates,
                                                             float *__restrict__ dE, float *__restrict__ partial) {
  __shared__ float cs[MC_K][MC_D];
  __shared__ float cinv[MC_K];
  __shared__ float red[4][MC_K][MC_D];
  mc_load_cores(Kemb, cs, cinv);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float dc[MC_K];
#pragma unroll
  for (int k = 0; k < MC_K; ++k) dc[k] = 0.f;
  for (int q = wave; q < 64; q += 4) {
    const int64_t i = (int64_t)blockIdx.x * 64 + q;
    if (i >= I) break;
    const float x = E[i * MC_D + lane];
    const float nrm = sqrtf(wave_sum(x * x));
    const float inv = 1.0f / fmaxf(nrm, 1e-12f);
    const float it = x * inv;
    float c[MC_K], g[MC_K], dot = 0.f;
#pragma unroll
    for (int k = 0; k < MC_K; ++k) {
      c[k] = cates[i * MC_K + k];
      g[k] = d_cates[i * MC_K + k];
      dot += c[k] * g[k];
    }
    float dit = d_items[i * MC_D + lane];
#pragma unroll
    for (int k = 0; k < MC_K; ++k) {
      const float t = c[k] * (g[k] - dot) * inv_tau;      // d loss / d (items_i . cores_k)
      dit += t * cs[k][lane];
      dc[k] += t * it;
    }
    const float proj = wave_sum(it * dit);
    dE[i * MC_D + lane] = nrm > 1e-12f ? inv * (dit - it * proj) : inv * dit;
  }
#pragma unroll
  for (int k = 0; k < MC_K; ++k) red[wave][k][lane] = dc[k];
  __syncthreads();
  for (int e = threadIdx.x; e < MC_K * MC_D; e += 256) {
    const int k = e >> 6, d = e & 63;
    partial[(int64_t)blockIdx.x * MC_K * MC_D + e] = ((red[0][k][d] + red[1][k][d]) + red[2][k][d]) + red[3][k][d];
  }
}

// d k_embedding[k, :]: the partials in ascending order, then F.normalize's backward; one wave per concept
__global__ __launch_bounds__(64) void mc_concept_bwd_finish_kernel(const float *__restrict__ Kemb, const float *__restrict__ partial,
                                                                   int64_t n_partial, float *__restrict__ dK) {
  const int lane = threadIdx.x, k = blockIdx.x;
  float v = 0.f;
  for (int64_t p = 0; p < n_partial; ++p) v += partial[p * MC_K * MC_D + k * MC_D + lane];
  const float x = Kemb[k * MC_D + lane];
  const float nrm = sqrtf(wave_sum(x * x));
  const float inv = 1.0f / fmaxf(nrm, 1e-12f);
  const float c = x * inv;
  const float proj = wave_sum(c * v);
  dK[k * MC_D + lane] = nrm > 1e-12f ? inv * (v - c * proj) : inv * v;
}

// ---------------------------------------------------------------------------------------------------------------
// encoder first layer (Model/MacridVAE.py:82-83, :101-105 up to the first Linear): one workgroup per sample, a thread
// one float4 of the 600 columns and all K accumulators; the row W1_t[i, :] is read ONCE per (sample, kept entry)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(192) void mc_encode_fwd_kernel(
    const int64_t *__restrict__ users, int64_t B, int64_t U, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ W1_t, const float *__restrict__ b1, const float *__restrict__ cates, McKeep kf, uint64_t seed,
    const int64_t *__restrict__ state, float *__restrict__ a, float *__restrict__ srow) {
  const int t = threadIdx.x;
  const bool active = t < MC_H4;
  const int c4 = 4 * (active ? t : 0);
  const int64_t b = blockIdx.x;
  const auto [beg, n] = vae_hist_row(rowptr, users[b], U);
  if (kf.training && !kf.keep) kf.key = draw_key(seed, (uint64_t)state[1], MC_SALT_KEEP);
  float4 acc[MC_K];
#pragma unroll
  for (int k = 0; k < MC_K; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t j = 0; j < n; ++j) {
    if (!kf(b, j)) continue;                        // (uniform over the workgroup)
    const int64_t i = col[beg + j];
    const float4 w = *reinterpret_cast<const float4 *>(W1_t + i * MC_H + c4);
#pragma unroll
    for (int k = 0; k < MC_K; ++k) {
      const float c = cates[i * MC_K + k];
      acc[k].x += c * w.x;
      acc[k].y += c * w.y;
      acc[k].z += c * w.z;
      acc[k].w += c * w.w;
    }
  }
  const float sc = vae_row_scale(n, kf.training, kf.keep_prob);
  if (t == 0) srow[b] = sc;
  if (!active) return;
  const float4 bias = *reinterpret_cast<const float4 *>(b1 + c4);
#pragma unroll
  for (int k = 0; k < MC_K; ++k)
    *reinterpret_cast<float4 *>(a + (b * MC_K + k) * MC_H + c4) =
        make_float4(bias.x + sc * acc[k].x, bias.y + sc * acc[k].y, bias.z + sc * acc[k].z, bias.w + sc * acc[k].w);
}

// dW1_t[i, :] = sum_{b, keep_bi} s_b sum_k c_ik da_bk;  dcates[i, k] = sum_{b, keep_bi} s_b W1_t[i, :] . da_bk.
// One workgroup per item; each of the three waves walks on its own and owns 64 float4 columns.
__global__ __launch_bounds__(192) void mc_encode_dw_kernel(
    int64_t I, const int64_t *__restrict__ item_ptr, const int32_t *__restrict__ item_users, const int32_t *__restrict__ item_pos,
    const int64_t *__restrict__ slot_ptr, const int64_t *__restrict__ perm, const float *__restrict__ W1_t,
    const float *__restrict__ cates, McKeep kf, uint64_t seed, const int64_t *__restrict__ state, const float *__restrict__ srow,
    const float *__restrict__ da, float *__restrict__ dW1_t, float *__restrict__ dcates) {
  __shared__ float red[3][MC_K];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool active = t < MC_H4;
  const int c4 = 4 * (active ? t : 0);
  const int64_t i = blockIdx.x;
  if (kf.training && !kf.keep) kf.key = draw_key(seed, (uint64_t)state[1], MC_SALT_KEEP);
  float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active) w = *reinterpret_cast<const float4 *>(W1_t + i * MC_H + c4);
  float c[MC_K], dc[MC_K];
#pragma unroll
  for (int k = 0; k < MC_K; ++k) {
    c[k] = cates[i * MC_K + k];
    dc[k] = 0.f;
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  vae_item_walk(i, item_ptr, item_users, item_pos, slot_ptr, perm, lane, [&](int64_t slot, int pos) {
    if (kf(slot, pos) && active) {
      const float s = srow[slot];
      float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < MC_K; ++k) {
        const float4 g = *reinterpret_cast<const float4 *>(da + (slot * MC_K + k) * MC_H + c4);
        sum.x += c[k] * g.x;
        sum.y += c[k] * g.y;
        sum.z += c[k] * g.z;
        sum.w += c[k] * g.w;
        dc[k] += s * (((w.x * g.x + w.y * g.y) + w.z * g.z) + w.w * g.w);
      }
      acc.x += s * sum.x;
      acc.y += s * sum.y;
      acc.z += s * sum.z;
      acc.w += s * sum.w;
    }
  });
  if (active) *reinterpret_cast<float4 *>(dW1_t + i * MC_H + c4) = acc;
#pragma unroll
  for (int k = 0; k < MC_K; ++k) {
    const float v = wave_sum(dc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (t < MC_K) dcates[i * MC_K + t] = (red[0][t] + red[1][t]) + red[2][t];
}

// column sums of x [rows, cols] (cols % 4 == 0, cols <= 768) by fixed-order partials over 64-row chunks
__global__ __launch_bounds__(192) void mc_colsum_kernel(const float *__restrict__ x, int64_t rows, int cols, float *__restrict__ partial) {
  const int c4 = 4 * threadIdx.x;
  if (c4 >= cols) return;
  const int64_t r0 = (int64_t)blockIdx.x * 64, r1 = min(rows, r0 + 64);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t r = r0; r < r1; ++r) {
    const float4 g = *reinterpret_cast<const float4 *>(x + r * cols + c4);
    v.x += g.x;
    v.y += g.y;
    v.z += g.z;
    v.w += g.w;
  }
  *reinterpret_cast<float4 *>(partial + (int64_t)blockIdx.x * cols + c4) = v;
}
__global__ __launch_bounds__(64) void mc_colsum_finish_kernel(const float *__restrict__ partial, int64_t n_partial, int cols,
                                                              float *__restrict__ out) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= cols) return;
  double v = 0.0;      // (hundreds of chunk sums of one sign pattern: added in double, rounded once)
  for (int64_t p = 0; p < n_partial; ++p) v += (double)partial[p * cols + c];
  out[c] = (float)v;
}

// ---------------------------------------------------------------------------------------------------------------
// likelihood, sample-owned passes.  blockIdx = (block of 128 samples, item split, concept k): a row is one (sample, k).
// Logits TRANSPOSED (A = items tile, B = zh rows), so a lane's 64 accumulator values of a tile belong to ITS row.
// WITH_DZ = false: ps[split, k, b] = sum_{i in split} c_ik exp(l_bik);  true: the dense part of d zh, per split.
// ---------------------------------------------------------------------------------------------------------------
template <bool WITH_DZ>
__global__ __launch_bounds__(256) void mc_rows_kernel(const float *__restrict__ zh, const float *__restrict__ items,
                                                      const float *__restrict__ cates, int64_t B, int64_t I, int64_t tiles_per_split,
                                                      float inv_tau, float *__restrict__ ps, const float *__restrict__ coef,
                                                      const float *__restrict__ gce, float *__restrict__ dzp) {
  constexpr int LD = VAE_TI + 1;
  __shared__ float Ws[MC_D][LD];      // [d][item]
  __shared__ float cs[VAE_TI];         // c_ik of the tile (0 past the end: the column adds nothing)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int k = blockIdx.z;
  const int64_t b = (int64_t)blockIdx.x * VAE_SB + wave * 32 + r;
  const bool live = b < B;
  const int64_t n_tiles = (I + VAE_TI - 1) / VAE_TI;
  const int64_t t_beg = (int64_t)blockIdx.y * tiles_per_split, t_end = min(n_tiles, t_beg + tiles_per_split);

  float bf[MC_D / 2];
#pragma unroll
  for (int s = 0; s < MC_D / 2; ++s) bf[s] = live ? zh[(b * MC_K + k) * MC_D + 2 * s + h] : 0.f;
  float ssum = 0.f;
  const float my_coef = WITH_DZ ? (live ? gce[0] * coef[b] : 0.f) : 0.f;
  f32x16 dz[2] = {vae_zero(), vae_zero()};

  for (int64_t tile = t_beg; tile < t_end; ++tile) {
    const int64_t i0 = tile * VAE_TI;
    __syncthreads();
    vae_stage_transposed<VAE_TI>(Ws, items, i0, I, t);
    if (t < VAE_TI) cs[t] = (i0 + t < I) ? cates[(i0 + t) * MC_K + k] : 0.f;
    __syncthreads();

#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      f32x16 acc = vae_zero();
#pragma unroll
      for (int s = 0; s < MC_D / 2; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[2 * s + h][32 * jt + r], bf[s], acc, 0, 0, 0);
      if (!WITH_DZ) {
#pragma unroll
        for (int q = 0; q < 16; ++q) ssum += cs[32 * jt + vae_row(q, h)] * expf(acc[q] * inv_tau);      // |l| <= 10: no maximum
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = my_coef * (cs[32 * jt + vae_row(q, h)] * expf(acc[q] * inv_tau));
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int item = 32 * jt + vae_row(q, h);
#pragma unroll
          for (int j = 0; j < 2; ++j)
            dz[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[32 * j + r][item], acc[q], dz[j], 0, 0, 0);
        }
      }
    }
  }

  if (!WITH_DZ) {
    const float s2 = __shfl_xor(ssum, 32, 64);     // the two half-waves saw different items of the same row: half 0 first
    if (live && h == 0) ps[((int64_t)blockIdx.y * MC_K + k) * B + b] = ssum + s2;
  } else if (live) {
    vae_store_dz(dzp + (((int64_t)blockIdx.y * B + b) * MC_K + k) * MC_D, dz, h);
  }
}

// the K logits of one (sample, item): lane = column, zk[k] = zh_bk[lane], it = items_i[lane] -> e[k] = exp(l_k), p
__device__ __forceinline__ float mc_pair(const float (&zk)[MC_K], float it, const float *__restrict__ crow, float inv_tau,
                                         float (&e)[MC_K], float (&c)[MC_K]) {
  float p = 0.f;
#pragma unroll
  for (int k = 0; k < MC_K; ++k) {
    c[k] = crow[k];
    e[k] = expf(wave_sum(it * zk[k]) * inv_tau);
    p += c[k] * e[k];
  }
  return p;
}

// S_b from the split partials (fixed order), the history walk sum_{i in hist(u_b)} log p_bi, nll_b, coef_b = n_b / (B S_b)
__global__ __launch_bounds__(64) void mc_lse_finish_kernel(
    const int64_t *__restrict__ users, int64_t B, int64_t U, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ zh, const float *__restrict__ items, const float *__restrict__ cates, float inv_tau,
    const float *__restrict__ ps, int64_t n_ps, float *__restrict__ lse, float *__restrict__ coef, float *__restrict__ nll) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  double s = 0.0;
  for (int64_t sp = lane; sp < n_ps; sp += 64) s += (double)ps[sp * B + b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  float zk[MC_K];
#pragma unroll
  for (int k = 0; k < MC_K; ++k) zk[k] = zh[(b * MC_K + k) * MC_D + lane];
  const auto [beg, n] = vae_hist_row(rowptr, users[b], U);
  double part = 0.0;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t i = col[beg + j];
    float e[MC_K], c[MC_K];
    const float p = mc_pair(zk, items[i * MC_D + lane], cates + i * MC_K, inv_tau, e, c);
    part += log((double)p);
  }
  if (lane == 0) {
    const double l = log(s);
    lse[b] = (float)l;
    coef[b] = (float)((double)n / ((double)B * s));
    nll[b] = (float)((double)n * l - part);
  }
}

// d zh_bk = [sum over splits (ascending) - (g / B) sum_{i in hist(u_b)} c_ik exp(l_bik) items_i / p_bi] / tau
__global__ __launch_bounds__(64) void mc_dz_finish_kernel(
    const int64_t *__restrict__ users, int64_t B, int64_t U, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ zh, const float *__restrict__ items, const float *__restrict__ cates, float inv_tau,
    const float *__restrict__ dzp, int splits, const float *__restrict__ gce, float *__restrict__ dz) {
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  float zk[MC_K], v[MC_K];
#pragma unroll
  for (int k = 0; k < MC_K; ++k) {
    zk[k] = zh[(b * MC_K + k) * MC_D + lane];
    v[k] = 0.f;
  }
  for (int sp = 0; sp < splits; ++sp)
#pragma unroll
    for (int k = 0; k < MC_K; ++k) v[k] += dzp[(((int64_t)sp * B + b) * MC_K + k) * MC_D + lane];
  const auto [beg, n] = vae_hist_row(rowptr, users[b], U);
  const float gB = gce[0] / (float)B;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t i = col[beg + j];
    const float it = items[i * MC_D + lane];
    float e[MC_K], c[MC_K];
    const float p = mc_pair(zk, it, cates + i * MC_K, inv_tau, e, c);
    const float f = gB / p;
#pragma unroll
    for (int k = 0; k < MC_K; ++k) v[k] -= f * (c[k] * e[k]) * it;
  }
#pragma unroll
  for (int k = 0; k < MC_K; ++k) dz[(b * MC_K + k) * MC_D + lane] = v[k] * inv_tau;
}

// ---------------------------------------------------------------------------------------------------------------
// item-owned pass: a workgroup owns 64 items and loops over ALL row blocks (128 rows of zh, a wave 32) and, inside, the
// K concepts.  Logits as [row][item] (A = zh block, B = items tile): lane & 31 = the item.
//   SCORES = false: d items (dense part P^T zh, P straight from the accumulator as the A operand), d cates, then the
//                   sparse x_bi terms by the item walk;
//   SCORES = true : out[row, item] = log p (Model/MacridVAE.py:126), rows = a range of users in eval mode.
// ---------------------------------------------------------------------------------------------------------------
template <bool SCORES>
__global__ __launch_bounds__(256) void mc_items_kernel(
    const float *__restrict__ zh, const float *__restrict__ items, const float *__restrict__ cates, int64_t B, int64_t I, float inv_tau,
    const float *__restrict__ coef, const float *__restrict__ gce, const int64_t *__restrict__ item_ptr,
    const int32_t *__restrict__ item_users, const int64_t *__restrict__ slot_ptr, const int64_t *__restrict__ perm,
    float *__restrict__ d_items, float *__restrict__ d_cates, float *__restrict__ scores) {
  constexpr int LD = MC_D + 1;
  __shared__ float Ws[MC_D][VAE_TW + 1];    // [d][item]
  __shared__ float Zs[VAE_SB][LD];          // [row][d] of the concept in flight
  float (*Rs)[LD] = reinterpret_cast<float (*)[LD]>(&Zs[0][0]);   // [item][d]: the waves' sums, once Zs is done with
  __shared__ float coefs[VAE_SB];
  __shared__ float Cs[MC_K][VAE_TW];
  __shared__ float bsum[SCORES ? 1 : 4][SCORES ? 1 : MC_K][SCORES ? 1 : VAE_TW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int64_t i0 = (int64_t)blockIdx.x * VAE_TW;
  vae_stage_transposed<VAE_TW>(Ws, items, i0, I, t);
  for (int e = t; e < MC_K * VAE_TW; e += 256) {
    const int k = e / VAE_TW, item = e % VAE_TW;
    Cs[k][item] = (i0 + item < I) ? cates[(i0 + item) * MC_K + k] : 0.f;
    if (!SCORES)
#pragma unroll
      for (int w = 0; w < 4; ++w) bsum[w][k][item] = 0.f;
  }
  const float g = SCORES ? 0.f : gce[0];
  f32x16 dw[2][2] = {{vae_zero(), vae_zero()}, {vae_zero(), vae_zero()}};

  for (int64_t s0 = 0; s0 < B; s0 += VAE_SB) {
    f32x16 pr[2] = {vae_zero(), vae_zero()};
    for (int k = 0; k < MC_K; ++k) {
      __syncthreads();
      vae_stage_rows(Zs, zh + k * MC_D, MC_K * MC_D, s0, B, t);
      if (!SCORES && k == 0 && t < VAE_SB) coefs[t] = (s0 + t < B) ? g * coef[s0 + t] : 0.f;     // a row past the end: P = 0
      __syncthreads();
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const float cl = Cs[k][32 * jt + r];
        f32x16 acc = vae_zero();
#pragma unroll
        for (int s = 0; s < MC_D / 2; ++s)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Zs[wave * 32 + r][2 * s + h], Ws[2 * s + h][32 * jt + r], acc, 0, 0, 0);
        if (SCORES) {
#pragma unroll
          for (int q = 0; q < 16; ++q) pr[jt][q] += cl * expf(acc[q] * inv_tau);
        } else {
          float bk = 0.f;
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const float ce = coefs[wave * 32 + vae_row(q, h)] * expf(acc[q] * inv_tau);
            bk += ce;
            acc[q] = ce * cl;
          }
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            const int sm = wave * 32 + vae_row(q, h);
#pragma unroll
            for (int j = 0; j < 2; ++j)
              dw[jt][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[q], Zs[sm][32 * j + r], dw[jt][j], 0, 0, 0);
          }
          bk += __shfl_xor(bk, 32, 64);
          if (h == 0) bsum[wave][k][32 * jt + r] += bk;      // (always this lane: an ordered running sum)
        }
      }
    }
    if (SCORES) {
#pragma unroll
      for (int jt = 0; jt < 2; ++jt) {
        const int64_t i = i0 + 32 * jt + r;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int64_t row = s0 + wave * 32 + vae_row(q, h);
          if (row < B && i < I) scores[row * I + i] = logf(pr[jt][q]);
        }
      }
    }
  }
  if (SCORES) return;

  vae_reduce_waves(Rs, dw, wave, r, h);
  const float gB = g / (float)B;
  for (int it = wave; it < VAE_TW; it += 4) {
    const int64_t i = i0 + it;
    if (i >= I) break;
    const float itv = items[i * MC_D + lane];
    float xz = 0.f, hk[MC_K];
#pragma unroll
    for (int k = 0; k < MC_K; ++k) hk[k] = 0.f;
    vae_item_walk(i, item_ptr, item_users, (const int32_t *)nullptr, slot_ptr, perm, lane, [&](int64_t slot, int) {
      float zk[MC_K], e[MC_K], c[MC_K];
#pragma unroll
      for (int k = 0; k < MC_K; ++k) zk[k] = zh[(slot * MC_K + k) * MC_D + lane];
      const float p = mc_pair(zk, itv, cates + i * MC_K, inv_tau, e, c);
      const float f = 1.0f / p;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < MC_K; ++k) {
        acc += (c[k] * e[k]) * zk[k];
        hk[k] += f * e[k];
      }
      xz += f * acc;
    });
    d_items[i * MC_D + lane] = (Rs[it][lane] - gB * xz) * inv_tau;
    float mine = 0.f;
#pragma unroll
    for (int k = 0; k < MC_K; ++k)
      if (lane == k) mine = (((bsum[0][k][it] + bsum[1][k][it]) + bsum[2][k][it]) + bsum[3][k][it]) - gB * hk[k];
    if (lane < MC_K) d_cates[i * MC_K + lane] = mine;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// exact top-K of each row (K <= 64 <= I), ties to the lowest index: a 4-bit radix search for the K-th largest key (8
// counting passes over the L2-resident row), an ordered compaction of the K winners, a rank-by-counting sort.  A row
// is read 10 times (8 + the count above the key + the compaction), each counting pass with 15 compare-adds per element.
// Keys order by bit pattern, so -0 < +0 and a NaN sorts by its sign and payload (above +inf or below -inf), unlike
// torch.topk, which puts every NaN first; the scores ranked here are logs of positive finite sums and the mask value.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mc_order_key(float x) {      // ascending with the float order
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void mc_topk_kernel(const float *__restrict__ scores, int64_t I, int K, int64_t id_offset,
                                                      int64_t *__restrict__ idx_out, float *__restrict__ val_out) {
  __shared__ int cnt[4][16];
  __shared__ uint32_t sel_key[64];
  __shared__ int sel_idx[64];
  __shared__ int wtot[4][2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t row = blockIdx.x;
  const float *x = scores + row * I;
  uint32_t prefix = 0;      // invariant: at least K keys are >= prefix
  for (int shift = 28; shift >= 0; shift -= 4) {
    int c[15];
#pragma unroll
    for (int j = 0; j < 15; ++j) c[j] = 0;
    for (int64_t e = t; e < I; e += 256) {
      const uint32_t key = mc_order_key(x[e]);
      const uint32_t dg = key >= prefix ? min((key - prefix) >> shift, 15u) : 0u;
#pragma unroll
      for (int j = 0; j < 15; ++j) c[j] += dg >= (uint32_t)(j + 1) ? 1 : 0;
    }
#pragma unroll
    for (int j = 0; j < 15; ++j) {
      int v = c[j];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) cnt[wave][j] = v;
    }
    __syncthreads();
    uint32_t best = 0;
#pragma unroll
    for (int j = 0; j < 15; ++j)
      if (cnt[0][j] + cnt[1][j] + cnt[2][j] + cnt[3][j] >= K) best = j + 1;      // (the counts fall with j)
    prefix += best << shift;
    __syncthreads();
  }
  const uint32_t T = prefix;      // the K-th largest key
  int n_gt = 0;
  for (int64_t e = t; e < I; e += 256) n_gt += mc_order_key(x[e]) > T ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n_gt += __shfl_xor(n_gt, off, 64);
  if (lane == 0) cnt[wave][0] = n_gt;
  __syncthreads();
  n_gt = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0];
  const int need_eq = K - n_gt;
  int run_gt = 0, run_eq = 0;
  for (int64_t base = 0; base < I && (run_gt < n_gt || run_eq < need_eq); base += 256) {
    const int64_t e = base + t;
    const uint32_t key = e < I ? mc_order_key(x[e]) : 0u;
    const bool gt = e < I && key > T, eq = e < I && key == T;
    const unsigned long long bg = __ballot(gt), be = __ballot(eq);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    __syncthreads();                                   // the previous chunk's readers of wtot are done
    if (lane == 0) {
      wtot[wave][0] = __popcll(bg);
      wtot[wave][1] = __popcll(be);
    }
    __syncthreads();
    int pg = run_gt + __popcll(bg & below), pe = run_eq + __popcll(be & below);
    for (int w = 0; w < 4; ++w) {
      if (w < wave) {
        pg += wtot[w][0];
        pe += wtot[w][1];
      }
      run_gt += wtot[w][0];
      run_eq += wtot[w][1];
    }
    if (gt && pg < 64) {
      sel_key[pg] = key;
      sel_idx[pg] = (int)e;
    } else if (eq && pe < need_eq) {
      sel_key[n_gt + pe] = key;
      sel_idx[n_gt + pe] = (int)e;
    }
  }
  __syncthreads();
  if (t < K) {
    const uint32_t mk = sel_key[t];
    const int mi = sel_idx[t];
    int rank = 0;
    for (int j = 0; j < K; ++j) rank += (sel_key[j] > mk || (sel_key[j] == mk && sel_idx[j] < mi)) ? 1 : 0;
    idx_out[row * K + rank] = (int64_t)mi + id_offset;
    val_out[row * K + rank] = x[mi];
  }
}

static int mc_shape(const char *what, int32_t D, int32_t K, int32_t H) {
  if (D != MC_D || K != MC_K || H != MC_H)
    return fail(CHAOREC_E_INVALID, "%s: D=%d K=%d H=%d, the kernels tile D=%d K=%d H=%d", what, (int)D, (int)K, (int)H, MC_D, MC_K, MC_H);
  return CHAOREC_OK;
}

}  // namespace chaorec

using namespace chaorec;

extern "C" int64_t chaorec_macrid_mix_splits(int64_t B, int64_t I) {
  if (B <= 0 || I <= 0) return 1;
  int64_t s, tp;
  vae_split_plan(B, I, MC_K, s, tp);
  return s;
}

extern "C" int chaorec_macrid_check_shape(int32_t D, int32_t K, int32_t H) { return mc_shape("macrid_check_shape", D, K, H); }

extern "C" int chaorec_macrid_tick(int64_t *state, float *anneal, float anneal_cap, int64_t total_anneal_steps, void *stream) {
  if (!state || !anneal) return fail(CHAOREC_E_INVALID, "macrid_tick: NULL argument");
  hipLaunchKernelGGL(mc_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, anneal, anneal_cap, total_anneal_steps);
  return check_launch("mc_tick_kernel");
}

extern "C" int chaorec_macrid_normal_f32(float *out, int64_t n, const int64_t *state, uint64_t seed, float std, void *stream) {
  if (!out || !state) return fail(CHAOREC_E_INVALID, "macrid_normal: NULL argument");
  if (n <= 0) return fail(CHAOREC_E_INVALID, "macrid_normal: n=%lld", (long long)n);
  hipLaunchKernelGGL((vae_normal_kernel<MC_BITS, MC_SALT_EPS>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, n,
                     seed, state, std);
  return check_launch("vae_normal_kernel");
}

extern "C" int chaorec_macrid_concept_fwd_f32(const float *item_emb, const float *k_emb, int64_t I, int32_t D, int32_t K, float tau,
                                              const float *gumbel, const int64_t *state, uint64_t seed, int32_t training,
                                              float *items, float *cates, void *stream) {
  if (!item_emb || !k_emb || !state || !items || !cates) return fail(CHAOREC_E_INVALID, "macrid_concept_fwd: NULL argument");
  int rc = mc_shape("macrid_concept_fwd", D, K, MC_H);
  if (rc) return rc;
  if (I <= 0 || !(tau > 0.f)) return fail(CHAOREC_E_INVALID, "macrid_concept_fwd: I=%lld tau=%g", (long long)I, tau);
  hipLaunchKernelGGL(mc_concept_fwd_kernel, dim3((unsigned)((I + 3) / 4)), dim3(256), 0, (hipStream_t)stream, item_emb, k_emb, I,
                     (float)(1.0 / (double)tau), gumbel, (int)training, seed, state, items, cates);
  return check_launch("mc_concept_fwd_kernel");
}

extern "C" int chaorec_macrid_concept_bwd_f32(const float *item_emb, const float *k_emb, int64_t I, int32_t D, int32_t K, float tau,
                                              const float *cates, const float *d_items, const float *d_cates, float *partial,
                                              int64_t n_partial, float *d_item_emb, float *d_k_emb, void *stream) {
  if (!item_emb || !k_emb || !cates || !d_items || !d_cates || !partial || !d_item_emb || !d_k_emb)
    return fail(CHAOREC_E_INVALID, "macrid_concept_bwd: NULL argument");
  int rc = mc_shape("macrid_concept_bwd", D, K, MC_H);
  if (rc) return rc;
  if (I <= 0 || !(tau > 0.f)) return fail(CHAOREC_E_INVALID, "macrid_concept_bwd: I=%lld tau=%g", (long long)I, tau);
  const int64_t blocks = (I + 63) / 64;
  if (n_partial < blocks) return fail(CHAOREC_E_WORKSPACE, "macrid_concept_bwd: partial blocks %lld < %lld", (long long)n_partial, (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mc_concept_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, item_emb, k_emb, I, (float)(1.0 / (double)tau), cates,
                     d_items, d_cates, d_item_emb, partial);
  rc = check_launch("mc_concept_bwd_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(mc_concept_bwd_finish_kernel, dim3(MC_K), dim3(64), 0, st, k_emb, (const float *)partial, blocks, d_k_emb);
  return check_launch("mc_concept_bwd_finish_kernel");
}

extern "C" int chaorec_macrid_encode_fwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                             const float *W1_t, const float *b1, const float *cates, int32_t K, int32_t H,
                                             const uint8_t *keep, const int64_t *keep_off, const int64_t *state, uint64_t seed,
                                             int32_t training, float keep_prob, float *a, float *srow, void *stream) {
  if (!users || !rowptr || !col || !W1_t || !b1 || !cates || !state || !a || !srow)
    return fail(CHAOREC_E_INVALID, "macrid_encode_fwd: NULL argument");
  int rc = mc_shape("macrid_encode_fwd", MC_D, K, H);
  if (rc) return rc;
  if (B <= 0 || U <= 0) return fail(CHAOREC_E_INVALID, "macrid_encode_fwd: B=%lld U=%lld", (long long)B, (long long)U);
  if ((keep == nullptr) != (keep_off == nullptr)) return fail(CHAOREC_E_INVALID, "macrid_encode_fwd: keep and keep_off go together");
  if (!(keep_prob > 0.f && keep_prob <= 1.f)) return fail(CHAOREC_E_INVALID, "macrid_encode_fwd: keep_prob %g", keep_prob);
  McKeep kf{keep, keep_off, 0, keep_prob, (int)training};
  hipLaunchKernelGGL(mc_encode_fwd_kernel, dim3((unsigned)B), dim3(192), 0, (hipStream_t)stream, users, B, U, rowptr, col, W1_t, b1, cates,
                     kf, seed, state, a, srow);
  return check_launch("mc_encode_fwd_kernel");
}

extern "C" int chaorec_macrid_encode_bwd_f32(int64_t B, int64_t I, const int64_t *item_ptr, const int32_t *item_users,
                                             const int32_t *item_pos, const int64_t *slot_ptr, const int64_t *perm, const float *W1_t,
                                             const float *cates, int32_t K, int32_t H, const uint8_t *keep, const int64_t *keep_off,
                                             const int64_t *state, uint64_t seed, int32_t training, float keep_prob,
                                             const float *srow, const float *da, float *partial, int64_t n_partial, float *dW1_t,
                                             float *db1, float *d_cates, void *stream) {
  if (!item_ptr || !item_users || !item_pos || !slot_ptr || !perm || !W1_t || !cates || !state || !srow || !da || !partial || !dW1_t ||
      !db1 || !d_cates)
    return fail(CHAOREC_E_INVALID, "macrid_encode_bwd: NULL argument");
  int rc = mc_shape("macrid_encode_bwd", MC_D, K, H);
  if (rc) return rc;
  if (B <= 0 || I <= 0) return fail(CHAOREC_E_INVALID, "macrid_encode_bwd: B=%lld I=%lld", (long long)B, (long long)I);
  if ((keep == nullptr) != (keep_off == nullptr)) return fail(CHAOREC_E_INVALID, "macrid_encode_bwd: keep and keep_off go together");
  const int64_t rows = B * MC_K, blocks = (rows + 63) / 64;
  if (n_partial < blocks) return fail(CHAOREC_E_WORKSPACE, "macrid_encode_bwd: partial rows %lld < %lld", (long long)n_partial, (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mc_colsum_kernel, dim3((unsigned)blocks), dim3(192), 0, st, da, rows, MC_H, partial);
  rc = check_launch("mc_colsum_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(mc_colsum_finish_kernel, dim3((MC_H + 63) / 64), dim3(64), 0, st, (const float *)partial, blocks, MC_H, db1);
  rc = check_launch("mc_colsum_finish_kernel");
  if (rc) return rc;
  McKeep kf{keep, keep_off, 0, keep_prob, (int)training};
  hipLaunchKernelGGL(mc_encode_dw_kernel, dim3((unsigned)I), dim3(192), 0, st, I, item_ptr, item_users, item_pos, slot_ptr, perm, W1_t,
                     cates, kf, seed, state, srow, da, dW1_t, d_cates);
  return check_launch("mc_encode_dw_kernel");
}

extern "C" int chaorec_macrid_mix_fwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                          const float *zh, const float *items, const float *cates, int64_t I, int32_t D, int32_t K,
                                          float tau, float *ps, int64_t splits, float *lse, float *coef, float *nll, float *ce,
                                          void *stream) {
  if (!users || !rowptr || !col || !zh || !items || !cates || !ps || !lse || !coef || !nll || !ce)
    return fail(CHAOREC_E_INVALID, "macrid_mix_fwd: NULL argument");
  int rc = mc_shape("macrid_mix_fwd", D, K, MC_H);
  if (rc) return rc;
  if (B <= 0 || U <= 0 || I <= 0 || !(tau > 0.f)) return fail(CHAOREC_E_INVALID, "macrid_mix_fwd: B=%lld U=%lld I=%lld tau=%g", (long long)B, (long long)U, (long long)I, tau);
  int64_t s, tp;
  vae_split_plan(B, I, MC_K, s, tp);
  if (splits != s) return fail(CHAOREC_E_WORKSPACE, "macrid_mix_fwd: splits %lld, chaorec_macrid_mix_splits says %lld", (long long)splits, (long long)s);
  hipStream_t st = (hipStream_t)stream;
  const float inv_tau = (float)(1.0 / (double)tau);
  const dim3 grid((unsigned)((B + VAE_SB - 1) / VAE_SB), (unsigned)s, MC_K);
  hipLaunchKernelGGL((mc_rows_kernel<false>), grid, dim3(256), 0, st, zh, items, cates, B, I, tp, inv_tau, ps, (const float *)nullptr,
                     (const float *)nullptr, (float *)nullptr);
  rc = check_launch("mc_rows_kernel<lse>");
  if (rc) return rc;
  hipLaunchKernelGGL(mc_lse_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, users, B, U, rowptr, col, zh, items, cates, inv_tau,
                     (const float *)ps, s * MC_K, lse, coef, nll);
  rc = check_launch("mc_lse_finish_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(vae_sum_kernel<>, dim3(1), dim3(256), 0, st, (const float *)nll, B, 1.0f / (float)B, ce, 0);
  return check_launch("vae_sum_kernel");
}

extern "C" int chaorec_macrid_mix_bwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                          const int64_t *item_ptr, const int32_t *item_users, const int64_t *slot_ptr,
                                          const int64_t *perm, const float *zh, const float *items, const float *cates, int64_t I,
                                          int32_t D, int32_t K, float tau, const float *coef, const float *gce, float *dzp,
                                          int64_t splits, float *d_zh, float *d_items, float *d_cates, void *stream) {
  if (!users || !rowptr || !col || !item_ptr || !item_users || !slot_ptr || !perm || !zh || !items || !cates || !coef || !gce || !dzp ||
      !d_zh || !d_items || !d_cates)
    return fail(CHAOREC_E_INVALID, "macrid_mix_bwd: NULL argument");
  int rc = mc_shape("macrid_mix_bwd", D, K, MC_H);
  if (rc) return rc;
  if (B <= 0 || U <= 0 || I <= 0 || !(tau > 0.f)) return fail(CHAOREC_E_INVALID, "macrid_mix_bwd: B=%lld U=%lld I=%lld tau=%g", (long long)B, (long long)U, (long long)I, tau);
  int64_t s, tp;
  vae_split_plan(B, I, MC_K, s, tp);
  if (splits != s) return fail(CHAOREC_E_WORKSPACE, "macrid_mix_bwd: splits %lld, chaorec_macrid_mix_splits says %lld", (long long)splits, (long long)s);
  hipStream_t st = (hipStream_t)stream;
  const float inv_tau = (float)(1.0 / (double)tau);
  const dim3 grid((unsigned)((B + VAE_SB - 1) / VAE_SB), (unsigned)s, MC_K);
  hipLaunchKernelGGL((mc_rows_kernel<true>), grid, dim3(256), 0, st, zh, items, cates, B, I, tp, inv_tau, (float *)nullptr, coef, gce, dzp);
  rc = check_launch("mc_rows_kernel<dz>");
  if (rc) return rc;
  hipLaunchKernelGGL(mc_dz_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, users, B, U, rowptr, col, zh, items, cates, inv_tau,
                     (const float *)dzp, (int)s, gce, d_zh);
  rc = check_launch("mc_dz_finish_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL((mc_items_kernel<false>), dim3((unsigned)((I + VAE_TW - 1) / VAE_TW)), dim3(256), 0, st, zh, items, cates, B, I, inv_tau,
                     coef, gce, item_ptr, item_users, slot_ptr, perm, d_items, d_cates, (float *)nullptr);
  return check_launch("mc_items_kernel<grad>");
}

extern "C" int chaorec_macrid_scores_f32(const float *zh, int64_t n_users, const float *items, const float *cates, int64_t I, int32_t D,
                                         int32_t K, float tau, int64_t user_begin, const int64_t *hist_rowptr, const int64_t *hist_col,
                                         float mask_value, float *scores, size_t scores_bytes, void *stream) {
  if (!zh || !items || !cates || !hist_rowptr || !hist_col || !scores) return fail(CHAOREC_E_INVALID, "macrid_scores: NULL argument");
  int rc = mc_shape("macrid_scores", D, K, MC_H);
  if (rc) return rc;
  if (n_users <= 0 || I <= 0 || user_begin < 0 || !(tau > 0.f))
    return fail(CHAOREC_E_INVALID, "macrid_scores: n_users=%lld I=%lld user_begin=%lld tau=%g", (long long)n_users, (long long)I, (long long)user_begin, tau);
  const size_t need = (size_t)n_users * (size_t)I * sizeof(float);
  if (scores_bytes < need || need > (size_t)CHAOREC_MACRID_STAGING_BYTES)
    return fail(CHAOREC_E_WORKSPACE, "macrid_scores: staging of %zu bytes (given %zu, cap %zu)", need, scores_bytes, (size_t)CHAOREC_MACRID_STAGING_BYTES);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((mc_items_kernel<true>), dim3((unsigned)((I + VAE_TW - 1) / VAE_TW)), dim3(256), 0, st, zh, items, cates, n_users, I,
                     (float)(1.0 / (double)tau), (const float *)nullptr, (const float *)nullptr, (const int64_t *)nullptr,
                     (const int32_t *)nullptr, (const int64_t *)nullptr, (const int64_t *)nullptr, (float *)nullptr, (float *)nullptr, scores);
  rc = check_launch("mc_items_kernel<scores>");
  if (rc) return rc;
  hipLaunchKernelGGL(vae_mask_kernel<>, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, scores, user_begin, user_begin + n_users, I,
                     hist_rowptr, hist_col, mask_value);
  return check_launch("vae_mask_kernel");
}

extern "C" int chaorec_macrid_topk_f32(const float *scores, int64_t n_rows, int64_t I, int32_t topk, int64_t id_offset, int64_t *idx,
                                       float *val, void *stream) {
  if (!scores || !idx || !val) return fail(CHAOREC_E_INVALID, "macrid_topk: NULL argument");
  if (n_rows <= 0 || topk < 1 || topk > 64 || I < topk || I > 0x7FFFFFFF)
    return fail(CHAOREC_E_INVALID, "macrid_topk: n_rows=%lld I=%lld topk=%d (1 <= topk <= 64 <= ... <= I)", (long long)n_rows, (long long)I, (int)topk);
  hipLaunchKernelGGL(mc_topk_kernel, dim3((unsigned)n_rows), dim3(256), 0, (hipStream_t)stream, scores, I, (int)topk, id_offset, idx, val);
  return check_launch("mc_topk_kernel");
}
