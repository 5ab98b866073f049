// MultVAE (Model/MultVAE.py): the history-row encoder and the all-items multinomial likelihood without any [B, I] buffer.
//
// The reference builds the dense multi-hot batch (Model/MultVAE.py:144,150), pushes it through Linear(I -> 128)
// (:78-91), decodes z through Linear(64 -> I) (:98-105) and takes log_softmax over all items (:155-156): [B, I] exists
// five times over.  Here a sample's row is a walk over hist(u_b) in the user-history CSR, and the logits are recomputed
// tile by tile on the f32 MFMA pipe (v_mfma_f32_32x32x2_f32: exact fp32 products, k-ascending fmaf chain, as gemm.hip)
// in each of the three passes that need them:
//   lse      (sample-block owned, item splits)  running max + rescaled sum per sample
//   dz       (sample-block owned, item splits)  P Wp with P = n_b softmax / B rebuilt from lse
//   dWp, dbp (item-tile owned, all samples)     P^T z, column sums of P
// No atomics anywhere: partials over item splits and over the waves of a workgroup are added in a fixed order, the
// sparse X parts are owner walks (a sample walks its history row; an item walks its users in the item-major CSR and,
// per user, that user's sample slots from a stable sort of the batch).  Two runs give the same bits.
//
// Layouts: Wq_t [I, 128] row-major (the reference's layers_q.0.weight [128, I] is its transposed view), Wp [I, 64],
// z [B, 64], h = [mu | logvar] [B, 128].  The latent width is 64 whatever dim_E says (p_dims = [64], :38).
#include "common.h"
#include "vae_common.h"

namespace chaorec {

constexpr int MV_D = 64;          // latent width
constexpr int MV_H = 2 * MV_D;    // encoder output [mu | logvar]
static_assert(MV_D == VAE_D, "the staging helpers move rows of the latent width");
constexpr uint64_t MV_SALT_KEEP = 0x6D756C7476616531ull, MV_SALT_EPS = 0x6D756C7476616532ull;

// the uniform keeps 24 bits here (MacridVAE's keeps 23): the streams the goldens were drawn from
constexpr int MV_BITS = 24;
using MvKeep = VaeKeep<MV_BITS>;

// state[0] = update_count (Model/MultVAE.py:29,162), state[1] = the count this step reads; anneal of :145-148
__global__ void mv_tick_kernel(int64_t *state, float *anneal, float cap, int64_t total) {
  if (threadIdx.x || blockIdx.x) return;
  const int64_t c = state[0];
  state[1] = c;
  state[0] = c + 1;
  anneal[0] = vae_anneal(c, total, cap);
}

// partial[g] = sum of squares of chunk g (Model/MultVAE.py:127-136, torch.norm(p) ** 2 per parameter)
__global__ __launch_bounds__(256) void mv_sumsq_kernel(const float *__restrict__ x, int64_t n, int64_t chunk, float *__restrict__ partial) {
  __shared__ double red[256];
  const int64_t beg = (int64_t)blockIdx.x * chunk, end = min(n, beg + chunk);
  double v = 0.0;
  for (int64_t i = beg + threadIdx.x; i < end; i += 256) v += (double)x[i] * (double)x[i];
  block_sum_f64(v, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = (float)red[0];
}

// ---------------------------------------------------------------------------------------------------------------
// encoder forward: one wave per sample; the two half-waves take alternate entries, a lane one float4 of the 128 columns
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mv_encode_fwd_kernel(
    const int64_t *__restrict__ users, int64_t B, int64_t U, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ Wq_t, const float *__restrict__ bq, MvKeep kf, uint64_t seed, const int64_t *__restrict__ state,
    const float *__restrict__ eps_in, float *__restrict__ h_out, float *__restrict__ z, float *__restrict__ eps_out,
    float *__restrict__ klrow) {
  const int lane = threadIdx.x & 63, half = lane >> 5, c4 = (lane & 31) * 4;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const auto [beg, n] = vae_hist_row(rowptr, users[b], U);
  const uint64_t step = (uint64_t)state[1];
  kf.key = draw_key(seed, step, MV_SALT_KEEP);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t j = half; j < n; j += 8) {      // four gathers in flight per half-wave
    float4 w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t jj = j + 2 * q;
      w[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (jj < n && kf(b, jj)) w[q] = *reinterpret_cast<const float4 *>(Wq_t + (int64_t)col[beg + jj] * MV_H + c4);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      acc.x += w[q].x; acc.y += w[q].y; acc.z += w[q].z; acc.w += w[q].w;
    }
  }
  acc.x += __shfl_xor(acc.x, 32, 64);
  acc.y += __shfl_xor(acc.y, 32, 64);
  acc.z += __shfl_xor(acc.z, 32, 64);
  acc.w += __shfl_xor(acc.w, 32, 64);
  const float sc = vae_row_scale(n, kf.training, kf.keep_prob);
  const float4 bias = *reinterpret_cast<const float4 *>(bq + c4);
  float hv[4] = {bias.x + sc * acc.x, bias.y + sc * acc.y, bias.z + sc * acc.z, bias.w + sc * acc.w};
  if (half == 0) *reinterpret_cast<float4 *>(h_out + b * MV_H + c4) = make_float4(hv[0], hv[1], hv[2], hv[3]);
  // epilogue (Model/MultVAE.py:87-91, :113-114): lanes 0-15 hold mu, lanes 16-31 the logvar of the same columns
  const uint64_t ekey = draw_key(seed, step, MV_SALT_EPS);
  double kl = 0.0;
  float zv[4], ev[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float lv = __shfl(hv[q], (lane & 15) + 16, 64), mu = hv[q];
    const int c = c4 + q;                              // (a column of z for lanes 0-15)
    const float e = (lane < 16) ? (eps_in ? eps_in[b * MV_D + c] : draw_normal<MV_BITS>(ekey, (uint64_t)b, (uint64_t)c)) : 0.f;
    ev[q] = e;
    zv[q] = mu + e * expf(0.5f * lv);
    kl += (double)(0.5f * (-lv + expf(lv) + mu * mu - 1.0f));
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) kl += __shfl_xor(kl, off, 64);
  if (lane < 16) {
    *reinterpret_cast<float4 *>(z + b * MV_D + c4) = make_float4(zv[0], zv[1], zv[2], zv[3]);
    *reinterpret_cast<float4 *>(eps_out + b * MV_D + c4) = make_float4(ev[0], ev[1], ev[2], ev[3]);
  }
  if (lane == 0) klrow[b] = (float)kl;
}

// encoder backward, part 1: sdh[b] = s_b * dL/dh_b and per-block column sums of dL/dh (the bias gradient's partials)
__global__ __launch_bounds__(MV_H) void mv_encode_dh_kernel(
    const int64_t *__restrict__ users, int64_t B, int64_t U, const int64_t *__restrict__ rowptr, const float *__restrict__ h,
    const float *__restrict__ eps, const float *__restrict__ gz, const float *__restrict__ gkl, int training, float keep_prob,
    float *__restrict__ sdh, float *__restrict__ partial) {
  const int c = threadIdx.x;
  const float gk = gkl[0] / (float)B;
  float colsum = 0.f;
  for (int q = 0; q < 64; ++q) {
    const int64_t b = (int64_t)blockIdx.x * 64 + q;
    if (b >= B) break;
    const int64_t n = vae_hist_row(rowptr, users[b], U).n;
    const float hv = h[b * MV_H + c];
    float d;
    if (c < MV_D) {
      d = gz[b * MV_D + c] + gk * hv;
    } else {
      const float e = eps[b * MV_D + c - MV_D];
      d = gz[b * MV_D + c - MV_D] * e * expf(0.5f * hv) * 0.5f + gk * 0.5f * (expf(hv) - 1.0f);
    }
    sdh[b * MV_H + c] = vae_row_scale(n, training, keep_prob) * d;
    colsum += d;
  }
  partial[(int64_t)blockIdx.x * MV_H + c] = colsum;
}

__global__ __launch_bounds__(MV_H) void mv_encode_dbias_kernel(const float *__restrict__ partial, int64_t n_partial,
                                                               const float *__restrict__ bq, const float *__restrict__ gsq,
                                                               float *__restrict__ dbq) {
  const int c = threadIdx.x;
  float v = 0.f;
  for (int64_t p = 0; p < n_partial; ++p) v += partial[p * MV_H + c];
  dbq[c] = v + 2.0f * gsq[0] * bq[c];
}

// encoder backward, part 2: dWq_t[i, :] = sum over kept (sample, i) of sdh[sample] + 2 gsq Wq_t[i, :]; one wave per item
__global__ __launch_bounds__(256) void mv_encode_dw_kernel(
    int64_t I, const int64_t *__restrict__ item_ptr, const int32_t *__restrict__ item_users, const int32_t *__restrict__ item_pos,
    const int64_t *__restrict__ slot_ptr, const int64_t *__restrict__ perm, const float *__restrict__ Wq_t, MvKeep kf, uint64_t seed,
    const int64_t *__restrict__ state, const float *__restrict__ sdh, const float *__restrict__ gsq, float *__restrict__ dWq_t) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= I) return;
  kf.key = draw_key(seed, (uint64_t)state[1], MV_SALT_KEEP);
  float2 acc = make_float2(0.f, 0.f);
  vae_item_walk(i, item_ptr, item_users, item_pos, slot_ptr, perm, lane, [&](int64_t slot, int pos) {
    if (kf(slot, pos)) {
      const float2 g = *reinterpret_cast<const float2 *>(sdh + slot * MV_H + 2 * lane);
      acc.x += g.x;
      acc.y += g.y;
    }
  });
  const float r = 2.0f * gsq[0];
  const float2 w = *reinterpret_cast<const float2 *>(Wq_t + i * MV_H + 2 * lane);
  *reinterpret_cast<float2 *>(dWq_t + i * MV_H + 2 * lane) = make_float2(acc.x + r * w.x, acc.y + r * w.y);
}

// ---------------------------------------------------------------------------------------------------------------
// decoder, sample-owned passes.  Workgroup = 128 samples (a wave: 32, lane & 31 = the sample) x a range of 128-item
// tiles.  Logits TRANSPOSED: A = Wp tile (rows = items), B = z (cols = samples), so a lane's 64 accumulator values of a
// tile all belong to ITS sample: the running softmax state is two registers, and P = n softmax / B is already laid
// out as the B operand of dz^T = Wp^T P (the reduction index -- items -- is permuted the same way on both operands).
// WITH_DZ = false: lse partials (m, s); true: dz partials.
// ---------------------------------------------------------------------------------------------------------------
template <bool WITH_DZ>
__global__ __launch_bounds__(256) void mv_decode_rows_kernel(
    const float *__restrict__ z, const float *__restrict__ Wp, const float *__restrict__ bp, int64_t B, int64_t I,
    int64_t tiles_per_split, float *__restrict__ pm, float *__restrict__ ps, const float *__restrict__ lse2,
    const float *__restrict__ cnt, const float *__restrict__ gnll, float *__restrict__ dzp) {
  constexpr int LD = VAE_TI + 1;
  __shared__ float Ws[MV_D][LD];      // [k][item]: A operand of the logits (k-major), A operand of dz^T (d-major)
  __shared__ float bs[VAE_TI];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int64_t b = (int64_t)blockIdx.x * VAE_SB + wave * 32 + r;
  const bool live = b < B;
  const int64_t n_tiles = (I + VAE_TI - 1) / VAE_TI;
  const int64_t t_beg = (int64_t)blockIdx.y * tiles_per_split, t_end = min(n_tiles, t_beg + tiles_per_split);

  float bf[MV_D / 2];
#pragma unroll
  for (int s = 0; s < MV_D / 2; ++s) bf[s] = live ? z[b * MV_D + 2 * s + h] : 0.f;
  float m = -INFINITY, ssum = 0.f;
  // lse as (max M, log of the rescaled sum L): P = exp((x - M) - L) subtracts NEAR values first, as log_softmax does --
  // one rounded lse of size ~1e3 would put 3e-5 into every exponent of the sample.  (A dead lane: M = +inf, P = 0.)
  const float my_m = WITH_DZ ? (live ? lse2[b] : INFINITY) : 0.f;
  const float my_l = WITH_DZ ? (live ? lse2[B + b] : 0.f) : 0.f;
  const float my_coef = WITH_DZ ? (live ? gnll[0] * cnt[b] / (float)B : 0.f) : 0.f;
  f32x16 dz[2] = {vae_zero(), vae_zero()};

  for (int64_t tile = t_beg; tile < t_end; ++tile) {
    const int64_t i0 = tile * VAE_TI;
    __syncthreads();                      // the previous tile's readers are done
    vae_stage_transposed<VAE_TI>(Ws, Wp, i0, I, t);
    if (t < VAE_TI) bs[t] = (i0 + t < I) ? bp[i0 + t] : -INFINITY;      // a column past the end: logit -inf, P = 0
    __syncthreads();

    f32x16 acc[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      acc[jt] = vae_zero();
#pragma unroll
      for (int s = 0; s < MV_D / 2; ++s)
        acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[2 * s + h][32 * jt + r], bf[s], acc[jt], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[jt][q] = acc[jt][q] + bs[32 * jt + vae_row(q, h)];
    }
    if (!WITH_DZ) {
      float tmax = -INFINITY;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int q = 0; q < 16; ++q) tmax = fmaxf(tmax, acc[jt][q]);
      const float mn = fmaxf(m, tmax);
      if (mn > -INFINITY) {
        float add = 0.f;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
          for (int q = 0; q < 16; ++q) add += expf(acc[jt][q] - mn);
        ssum = ssum * expf(m - mn) + add;
        m = mn;
      }
    } else {
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[jt][q] = my_coef * expf((acc[jt][q] - my_m) - my_l);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int item = 32 * jt + vae_row(q, h);
#pragma unroll
          for (int j = 0; j < 2; ++j)
            dz[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[32 * j + r][item], acc[jt][q], dz[j], 0, 0, 0);
        }
      }
    }
  }

  if (!WITH_DZ) {
    // the two half-waves saw different items of the same sample: half 0's partial first
    const float m2 = __shfl_xor(m, 32, 64), s2 = __shfl_xor(ssum, 32, 64);
    const float M = fmaxf(m, m2);
    float S = 0.f;
    if (m > -INFINITY) S += ssum * expf(m - M);
    if (m2 > -INFINITY) S += s2 * expf(m2 - M);
    if (live && h == 0) {
      pm[(int64_t)blockIdx.y * B + b] = M;
      ps[(int64_t)blockIdx.y * B + b] = S;
    }
  } else if (live) {
    vae_store_dz(dzp + ((int64_t)blockIdx.y * B + b) * MV_D, dz, h);
  }
}

// lse_b from the split partials (fixed order) and the history walk: sum_{i in hist(u_b)} logit_bi with the tile's own
// chain (fmaf over k ascending from 0, then + b_i), so every term is one of the values lse was built from.
__global__ __launch_bounds__(64) void mv_decode_lse_finish_kernel(
    const int64_t *__restrict__ users, int64_t B, int64_t U, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ z, const float *__restrict__ Wp, const float *__restrict__ bp, const float *__restrict__ pm,
    const float *__restrict__ ps, int splits, float *__restrict__ lse, float *__restrict__ lse2, float *__restrict__ cnt,
    float *__restrict__ nll) {
  __shared__ float zs[MV_D];
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  zs[lane] = z[b * MV_D + lane];
  float m = -INFINITY, s = 0.f;
  for (int sp = lane; sp < splits; sp += 64) {
    const float m2 = pm[(int64_t)sp * B + b], s2 = ps[(int64_t)sp * B + b];
    const float M = fmaxf(m, m2);
    if (M > -INFINITY) {
      s = s * expf(m - M) + s2 * expf(m2 - M);
      m = M;
    }
  }
  float M = m;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) M = fmaxf(M, __shfl_xor(M, off, 64));
  const float S = wave_sum(m > -INFINITY ? s * expf(m - M) : 0.f);
  const double l = (double)M + log((double)S);
  __syncthreads();
  const auto [beg, n] = vae_hist_row(rowptr, users[b], U);
  double part = 0.0;
  for (int64_t j = lane; j < n; j += 64) {
    const int64_t i = col[beg + j];
    const float4 *w = reinterpret_cast<const float4 *>(Wp + i * MV_D);
    float dot = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < MV_D / 4; ++k4) {
      const float4 x = w[k4];
      dot = fmaf(x.x, zs[4 * k4 + 0], dot);
      dot = fmaf(x.y, zs[4 * k4 + 1], dot);
      dot = fmaf(x.z, zs[4 * k4 + 2], dot);
      dot = fmaf(x.w, zs[4 * k4 + 3], dot);
    }
    part += (double)(dot + bp[i]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
  if (lane == 0) {
    lse[b] = (float)l;
    lse2[b] = M;
    lse2[B + b] = logf(S);
    cnt[b] = (float)n;
    nll[b] = (float)((double)n * l - part);
  }
}

// dz_b = sum over splits (ascending) - (g / B) sum_{i in hist(u_b)} Wp[i, :]
__global__ __launch_bounds__(64) void mv_decode_dz_finish_kernel(
    const int64_t *__restrict__ users, int64_t B, int64_t U, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ Wp, const float *__restrict__ dzp, int splits, const float *__restrict__ gnll, float *__restrict__ dz) {
  const int d = threadIdx.x;
  const int64_t b = blockIdx.x;
  float v = 0.f;
  for (int sp = 0; sp < splits; ++sp) v += dzp[((int64_t)sp * B + b) * MV_D + d];
  const auto [beg, n] = vae_hist_row(rowptr, users[b], U);
  float x = 0.f;
  for (int64_t j = 0; j < n; ++j) x += Wp[(int64_t)col[beg + j] * MV_D + d];
  dz[b * MV_D + d] = v - (gnll[0] / (float)B) * x;
}

// ---------------------------------------------------------------------------------------------------------------
// decoder, item-owned pass: a workgroup owns 64 items and loops over ALL sample blocks (no sum across workgroups).
// Logits as [sample][item] (A = z block, B = Wp tile), so lane & 31 = the item and P^T z takes P straight from the
// accumulator as its A operand (the reduction index -- samples -- permuted alike on the z operand).  The four waves'
// sums are added through LDS in wave order; then the sparse -X^T z / B part (item walk) and 2 gsq Wp.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mv_decode_dw_kernel(
    const float *__restrict__ z, const float *__restrict__ Wp, const float *__restrict__ bp, int64_t B, int64_t I,
    const float *__restrict__ lse2, const float *__restrict__ cnt, const float *__restrict__ gnll, const float *__restrict__ gsq,
    const int64_t *__restrict__ item_ptr, const int32_t *__restrict__ item_users, const int64_t *__restrict__ slot_ptr,
    const int64_t *__restrict__ perm, float *__restrict__ dWp, float *__restrict__ dbp) {
  constexpr int LD = MV_D + 1;
  __shared__ float Ws[MV_D][VAE_TW + 1];    // [k][item]
  __shared__ float Zs[VAE_SB][LD];          // [sample][k]
  float (*Rs)[LD] = reinterpret_cast<float (*)[LD]>(&Zs[0][0]);   // [item][d]: the waves' sums, once Zs is done with
  __shared__ float lsem[VAE_SB], lsel[VAE_SB], coefs[VAE_SB], bsum[4][VAE_TW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int64_t i0 = (int64_t)blockIdx.x * VAE_TW;
  const float g = gnll[0];
  vae_stage_transposed<VAE_TW>(Ws, Wp, i0, I, t);
  float bias[2];
#pragma unroll
  for (int jt = 0; jt < 2; ++jt) bias[jt] = (i0 + 32 * jt + r < I) ? bp[i0 + 32 * jt + r] : -INFINITY;
  f32x16 dw[2][2] = {{vae_zero(), vae_zero()}, {vae_zero(), vae_zero()}};
  float bacc[2] = {0.f, 0.f};

  for (int64_t s0 = 0; s0 < B; s0 += VAE_SB) {
    __syncthreads();
    vae_stage_rows(Zs, z, MV_D, s0, B, t);
    if (t < VAE_SB) {
      const bool live = s0 + t < B;
      lsem[t] = live ? lse2[s0 + t] : INFINITY;           // a sample past the end: P = 0 * exp(-inf) = 0
      lsel[t] = live ? lse2[B + s0 + t] : 0.f;
      coefs[t] = live ? g * cnt[s0 + t] / (float)B : 0.f;
    }
    __syncthreads();
    f32x16 acc[2];
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
      acc[jt] = vae_zero();
#pragma unroll
      for (int s = 0; s < MV_D / 2; ++s)
        acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Zs[wave * 32 + r][2 * s + h], Ws[2 * s + h][32 * jt + r], acc[jt], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int sm = wave * 32 + vae_row(q, h);
        const float p = coefs[sm] * expf(((acc[jt][q] + bias[jt]) - lsem[sm]) - lsel[sm]);
        acc[jt][q] = p;
        bacc[jt] += p;
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int sm = wave * 32 + vae_row(q, h);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          dw[jt][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[jt][q], Zs[sm][32 * j + r], dw[jt][j], 0, 0, 0);
      }
    }
  }
  // the column sums of P per wave (added at the end, waves 0..3 in order), then the waves' dw the same way
#pragma unroll
  for (int jt = 0; jt < 2; ++jt) bacc[jt] += __shfl_xor(bacc[jt], 32, 64);
  if (h == 0) {
    bsum[wave][r] = bacc[0];
    bsum[wave][32 + r] = bacc[1];
  }
  vae_reduce_waves(Rs, dw, wave, r, h);
  const float gB = g / (float)B, reg2 = 2.0f * gsq[0];
  for (int it = wave; it < VAE_TW; it += 4) {
    const int64_t i = i0 + it;
    if (i >= I) break;
    float xz = 0.f, hits = 0.f;
    vae_item_walk(i, item_ptr, item_users, (const int32_t *)nullptr, slot_ptr, perm, lane, [&](int64_t slot, int) {
      xz += z[slot * MV_D + lane];
      hits += 1.0f;
    });
    dWp[i * MV_D + lane] = (Rs[it][lane] - gB * xz) + reg2 * Wp[i * MV_D + lane];
    if (lane == 0)
      dbp[i] = ((((bsum[0][it] + bsum[1][it]) + bsum[2][it]) + bsum[3][it]) - gB * hits) + reg2 * bp[i];
  }
}

}  // namespace chaorec

using namespace chaorec;

extern "C" int64_t chaorec_multvae_decode_splits(int64_t B, int64_t I) {
  if (B <= 0 || I <= 0) return 1;
  int64_t s, tp;
  vae_split_plan(B, I, 1, s, tp);
  return s;
}

extern "C" int chaorec_multvae_tick(int64_t *state, float *anneal, float anneal_cap, int64_t total_anneal_steps, void *stream) {
  if (!state || !anneal) return fail(CHAOREC_E_INVALID, "multvae_tick: NULL argument");
  hipLaunchKernelGGL(mv_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, anneal, anneal_cap, total_anneal_steps);
  return check_launch("mv_tick_kernel");
}

extern "C" int chaorec_multvae_sumsq_f32(const float *x, int64_t n, float *partial, int64_t n_partial, float *out,
                                         int32_t accumulate, void *stream) {
  if (!x || !partial || !out) return fail(CHAOREC_E_INVALID, "multvae_sumsq: NULL argument");
  if (n < 0 || n_partial < 1 || n_partial > 4096) return fail(CHAOREC_E_INVALID, "multvae_sumsq: n=%lld n_partial=%lld", (long long)n, (long long)n_partial);
  const int64_t chunk = (n + n_partial - 1) / n_partial;
  hipLaunchKernelGGL(mv_sumsq_kernel, dim3((unsigned)n_partial), dim3(256), 0, (hipStream_t)stream, x, n, chunk, partial);
  int rc = check_launch("mv_sumsq_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(vae_sum_kernel<>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float *)partial, n_partial, 1.0f, out, (int)accumulate);
  return check_launch("vae_sum_kernel");
}

extern "C" int chaorec_multvae_encode_fwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                              const float *Wq_t, const float *bq, const uint8_t *keep, const int64_t *keep_off,
                                              const float *eps_in, const int64_t *state, uint64_t seed, int32_t training,
                                              float keep_prob, float *h, float *z, float *eps_out, float *klrow, float *kl,
                                              void *stream) {
  if (!users || !rowptr || !col || !Wq_t || !bq || !state || !h || !z || !eps_out || !klrow || !kl)
    return fail(CHAOREC_E_INVALID, "multvae_encode_fwd: NULL argument");
  if (B <= 0 || U <= 0) return fail(CHAOREC_E_INVALID, "multvae_encode_fwd: B=%lld U=%lld", (long long)B, (long long)U);
  if ((keep == nullptr) != (keep_off == nullptr)) return fail(CHAOREC_E_INVALID, "multvae_encode_fwd: keep and keep_off go together");
  if (!(keep_prob > 0.f && keep_prob <= 1.f)) return fail(CHAOREC_E_INVALID, "multvae_encode_fwd: keep_prob %g", keep_prob);
  hipStream_t st = (hipStream_t)stream;
  MvKeep kf{keep, keep_off, 0, keep_prob, (int)training};
  hipLaunchKernelGGL(mv_encode_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, users, B, U, rowptr, col, Wq_t, bq, kf,
                     seed, state, eps_in, h, z, eps_out, klrow);
  int rc = check_launch("mv_encode_fwd_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(vae_sum_kernel<>, dim3(1), dim3(256), 0, st, (const float *)klrow, B, 1.0f / (float)B, kl, 0);
  return check_launch("vae_sum_kernel");
}

extern "C" int chaorec_multvae_encode_bwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, int64_t I,
                                              const int64_t *item_ptr, const int32_t *item_users, const int32_t *item_pos,
                                              const int64_t *slot_ptr, const int64_t *perm, const float *Wq_t, const float *bq,
                                              const uint8_t *keep, const int64_t *keep_off, const int64_t *state, uint64_t seed,
                                              int32_t training, float keep_prob, const float *h, const float *eps,
                                              const float *gz, const float *gkl, const float *gsq, float *sdh, float *partial,
                                              int64_t n_partial, float *dWq_t, float *dbq, void *stream) {
  if (!users || !rowptr || !item_ptr || !item_users || !item_pos || !slot_ptr || !perm || !Wq_t || !bq || !state || !h || !eps ||
      !gz || !gkl || !gsq || !sdh || !partial || !dWq_t || !dbq)
    return fail(CHAOREC_E_INVALID, "multvae_encode_bwd: NULL argument");
  if (B <= 0 || U <= 0 || I <= 0) return fail(CHAOREC_E_INVALID, "multvae_encode_bwd: B=%lld U=%lld I=%lld", (long long)B, (long long)U, (long long)I);
  if ((keep == nullptr) != (keep_off == nullptr)) return fail(CHAOREC_E_INVALID, "multvae_encode_bwd: keep and keep_off go together");
  const int64_t blocks = (B + 63) / 64;
  if (n_partial < blocks) return fail(CHAOREC_E_WORKSPACE, "multvae_encode_bwd: partial rows %lld < %lld", (long long)n_partial, (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mv_encode_dh_kernel, dim3((unsigned)blocks), dim3(MV_H), 0, st, users, B, U, rowptr, h, eps, gz, gkl,
                     (int)training, keep_prob, sdh, partial);
  int rc = check_launch("mv_encode_dh_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(mv_encode_dbias_kernel, dim3(1), dim3(MV_H), 0, st, (const float *)partial, blocks, bq, gsq, dbq);
  rc = check_launch("mv_encode_dbias_kernel");
  if (rc) return rc;
  MvKeep kf{keep, keep_off, 0, keep_prob, (int)training};
  hipLaunchKernelGGL(mv_encode_dw_kernel, dim3((unsigned)((I + 3) / 4)), dim3(256), 0, st, I, item_ptr, item_users, item_pos,
                     slot_ptr, perm, Wq_t, kf, seed, state, (const float *)sdh, gsq, dWq_t);
  return check_launch("mv_encode_dw_kernel");
}

extern "C" int chaorec_multvae_decode_fwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                              const float *z, const float *Wp, const float *bp, int64_t I, float *pm, float *ps,
                                              int64_t splits, float *lse, float *lse2, float *cnt, float *nll, float *neg_ll, void *stream) {
  if (!users || !rowptr || !col || !z || !Wp || !bp || !pm || !ps || !lse || !lse2 || !cnt || !nll || !neg_ll)
    return fail(CHAOREC_E_INVALID, "multvae_decode_fwd: NULL argument");
  if (B <= 0 || U <= 0 || I <= 0) return fail(CHAOREC_E_INVALID, "multvae_decode_fwd: B=%lld U=%lld I=%lld", (long long)B, (long long)U, (long long)I);
  int64_t s, tp;
  vae_split_plan(B, I, 1, s, tp);
  if (splits != s) return fail(CHAOREC_E_WORKSPACE, "multvae_decode_fwd: splits %lld, chaorec_multvae_decode_splits says %lld", (long long)splits, (long long)s);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((B + VAE_SB - 1) / VAE_SB), (unsigned)s);
  hipLaunchKernelGGL((mv_decode_rows_kernel<false>), grid, dim3(256), 0, st, z, Wp, bp, B, I, tp, pm, ps, (const float *)nullptr,
                     (const float *)nullptr, (const float *)nullptr, (float *)nullptr);
  int rc = check_launch("mv_decode_rows_kernel<lse>");
  if (rc) return rc;
  hipLaunchKernelGGL(mv_decode_lse_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, users, B, U, rowptr, col, z, Wp, bp,
                     (const float *)pm, (const float *)ps, (int)s, lse, lse2, cnt, nll);
  rc = check_launch("mv_decode_lse_finish_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(vae_sum_kernel<>, dim3(1), dim3(256), 0, st, (const float *)nll, B, 1.0f / (float)B, neg_ll, 0);
  return check_launch("vae_sum_kernel");
}

extern "C" int chaorec_multvae_decode_bwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                              const int64_t *item_ptr, const int32_t *item_users, const int64_t *slot_ptr,
                                              const int64_t *perm, const float *z, const float *Wp, const float *bp, int64_t I,
                                              const float *lse2, const float *cnt, const float *gnll, const float *gsq, float *dzp,
                                              int64_t splits, float *dz, float *dWp, float *dbp, void *stream) {
  if (!users || !rowptr || !col || !item_ptr || !item_users || !slot_ptr || !perm || !z || !Wp || !bp || !lse2 || !cnt || !gnll ||
      !gsq || !dzp || !dz || !dWp || !dbp)
    return fail(CHAOREC_E_INVALID, "multvae_decode_bwd: NULL argument");
  if (B <= 0 || U <= 0 || I <= 0) return fail(CHAOREC_E_INVALID, "multvae_decode_bwd: B=%lld U=%lld I=%lld", (long long)B, (long long)U, (long long)I);
  int64_t s, tp;
  vae_split_plan(B, I, 1, s, tp);
  if (splits != s) return fail(CHAOREC_E_WORKSPACE, "multvae_decode_bwd: splits %lld, chaorec_multvae_decode_splits says %lld", (long long)splits, (long long)s);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((B + VAE_SB - 1) / VAE_SB), (unsigned)s);
  hipLaunchKernelGGL((mv_decode_rows_kernel<true>), grid, dim3(256), 0, st, z, Wp, bp, B, I, tp, (float *)nullptr, (float *)nullptr,
                     lse2, cnt, gnll, dzp);
  int rc = check_launch("mv_decode_rows_kernel<dz>");
  if (rc) return rc;
  hipLaunchKernelGGL(mv_decode_dz_finish_kernel, dim3((unsigned)B), dim3(64), 0, st, users, B, U, rowptr, col, Wp, (const float *)dzp,
                     (int)s, gnll, dz);
  rc = check_launch("mv_decode_dz_finish_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(mv_decode_dw_kernel, dim3((unsigned)((I + VAE_TW - 1) / VAE_TW)), dim3(256), 0, st, z, Wp, bp, B, I, lse2, cnt, gnll,
                     gsq, item_ptr, item_users, slot_ptr, perm, dWp, dbp);
  return check_launch("mv_decode_dw_kernel");
}
