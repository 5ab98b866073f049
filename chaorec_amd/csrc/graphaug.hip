// GraphAug (Model/GraphAug.py): the per-entry edge sampler of its view learner, the whole-table log-sum-exp of its
// contrastive loss, and the propagate's random-entry term.  gfx950, D = 64.
//
// (a) edge sampler, ViewLearner.forward + build_prob_neighbourhood (Model/GraphAug.py:268-309), forward only (everything
//   is detached there).  W1 [z[row]; z[col]] = P[row] + Q[col] with P = z W1[:, :64]^T, Q = z W1[:, 64:]^T (two N-sized
//   GEMMs on the caller's side), so per stored entry e = (row, col), in fp32 as the reference:
//     logit = b2 + sum_j w2[j] relu((P[row][j] + b1[j]) + Q[col][j])          j ascending, fmaf chain
//     eps   = (-0.9998f u1) + 0.9999f                                          (bias - (1 - bias)) u1 + (1 - bias), bias = 1e-4
//     att   = clamp(sigmoid((log eps - log(1 - eps)) + logit), 0.01, 0.99)
//     u2'   = clamp(u2, 2^-23, 1 - 2^-23)                                      RelaxedBernoulli(0.9, probs = att).rsample()
//     s     = clamp(sigmoid((((log u2' - log1p(-u2')) + log att) - log1p(-att)) / 0.9f), FLT_MIN, 1 - 2^-23)
//     val   = s > 0.2 ? s : +0
//   Row-owned like ag_*: a wave holds GA_RW = 8 rows, 8 lanes each; a lane keeps its row's P + b1 in 64 registers and takes the
//   row's entries j, j + 8, ...; a row longer than GA_LONG = 64 entries is taken by its whole wave afterwards (lane j: entries
//   j, j + 64, ...).  Every entry has one owner and no sum crosses lanes: the same bits every run, no atomics.
//   u1, u2 given fp32 [E], or NULL: draw_uniform<24>(draw_key(seed, state[1], salt 2 view + {0, 1}), 0, e), written to
//   u_out [2, E] if not NULL.  val_t (may be NULL): val_t[tentry[e]] = val[e] -- tentry is a permutation, one store per element.
// (b) log-sum-exp of a batch against a whole table (contrastLoss's denominator, :534-541), no running max (the reference has
//   none; rows arrive normalised, so |<a, t>| inv_temp <= inv_temp):
//     lse[b] = log sum_m exp(<A_b, T_m> inv_temp);  w_bm = g_b inv_temp exp(<A_b, T_m> inv_temp - lse_b)
//     gA_b = sum_m w_bm T_m;  gT_m = sum_b w_bm A_b
//   on v_mfma_f32_32x32x2_f32 (exact fp32 products), shaped like multvae's decoder passes: forward and gA are sample-owned
//   (workgroup = 128 samples, a wave: one 32-row tile, x a split of the 128-row table tiles) and write per-split partials that
//   a finish launch adds in split order; gT is table-owned (a workgroup owns 64 table rows and loops over ALL of B, the four
//   waves' sums added in wave order).  No [B, M] buffer, no float atomics.
// (c) y = act(z + alpha sum_{e in row n} x[col e]) over the CSR of the step's random entries (all of one value): a wave per
//   row, lane = feature, entries in order.  act = LeakyReLU(slope); slope = 1: none.  z may be NULL.
#include <float.h>
#include "vae_common.h"

namespace chaorec {

constexpr int GA_D = 64;
constexpr int GA_RW = 8;           // rows per wave
constexpr int GA_RB = kRowsPerBlock8;      // rows per workgroup
constexpr int GA_LONG = 64;        // a longer row is taken by the whole wave
constexpr uint64_t GA_SALT = 0x6772617068617567ull;
constexpr float GA_P_LO = 1.1920928955078125e-07f, GA_P_HI = 0.99999988079071044921875f;      // 2^-23, 1 - 2^-23
static_assert(GA_D == VAE_D, "the staging helpers move rows of the latent width");

struct GaSample {
  const int32_t *col, *tentry;
  const float *Q, *b1, *w2, *b2p, *u1, *u2;
  float *val, *val_t, *logit_out, *u_out;
  int64_t N, E;
  float b2;
  uint64_t key1, key2;
};

// pb[j] = P[row][j] + b1[j]: the entry's value, stored by its one owner
__device__ __forceinline__ void ga_entry(const GaSample &a, const float (&pb)[GA_D], int64_t e) {
  const float4 *q = reinterpret_cast<const float4 *>(a.Q + (int64_t)clamp_index(a.col[e], a.N) * GA_D);
  float logit = a.b2;
#pragma unroll
  for (int k = 0; k < GA_D / 4; ++k) {
    const float4 x = q[k];
    logit = fmaf(a.w2[4 * k + 0], fmaxf(add_rn(pb[4 * k + 0], x.x), 0.f), logit);
    logit = fmaf(a.w2[4 * k + 1], fmaxf(add_rn(pb[4 * k + 1], x.y), 0.f), logit);
    logit = fmaf(a.w2[4 * k + 2], fmaxf(add_rn(pb[4 * k + 2], x.z), 0.f), logit);
    logit = fmaf(a.w2[4 * k + 3], fmaxf(add_rn(pb[4 * k + 3], x.w), 0.f), logit);
  }
  const float v1 = a.u1 ? a.u1[e] : draw_uniform<24>(a.key1, 0, (uint64_t)e);
  const float v2 = a.u2 ? a.u2[e] : draw_uniform<24>(a.key2, 0, (uint64_t)e);
  if (a.u_out) {
    a.u_out[e] = v1;
    a.u_out[a.E + e] = v2;
  }
  const float eps = add_rn(mul_rn(-0.9998f, v1), 0.9999f);
  const float gate = add_rn(add_rn(logf(eps), -logf(add_rn(1.0f, -eps))), logit);
  const float att = fminf(fmaxf(sigmoidf_acc(gate), 0.01f), 0.99f);
  const float uc = fminf(fmaxf(v2, GA_P_LO), GA_P_HI);
  const float x = add_rn(add_rn(add_rn(logf(uc), -log1pf(-uc)), logf(att)), -log1pf(-att)) / 0.9f;
  const float s = fminf(fmaxf(sigmoidf_acc(x), FLT_MIN), GA_P_HI);
  const float v = s > 0.2f ? s : 0.f;
  a.val[e] = v;
  if (a.logit_out) a.logit_out[e] = logit;
  if (a.val_t) {
    a.val_t[clamp_index((int64_t)a.tentry[e], a.E)] = v;
  }
}

__device__ __forceinline__ void ga_load_row(float (&pb)[GA_D], const float *__restrict__ P, const float *__restrict__ b1, int64_t n) {
  const float4 *p = reinterpret_cast<const float4 *>(P + n * GA_D);
#pragma unroll
  for (int k = 0; k < GA_D / 4; ++k) {
    const float4 x = p[k];
    pb[4 * k + 0] = add_rn(x.x, b1[4 * k + 0]);
    pb[4 * k + 1] = add_rn(x.y, b1[4 * k + 1]);
    pb[4 * k + 2] = add_rn(x.z, b1[4 * k + 2]);
    pb[4 * k + 3] = add_rn(x.w, b1[4 * k + 3]);
  }
}

__global__ __launch_bounds__(256) void ga_sample_kernel(const int64_t *__restrict__ rowptr, const float *__restrict__ P, GaSample a,
                                                        uint64_t seed, const int64_t *__restrict__ state, uint64_t salt) {
  const int lane = threadIdx.x & 63, sub = lane & 7;
  const LaneRow row = lane_group_row(rowptr, a.N);
  const int64_t n = row.n, beg = row.beg, end = min(row.end, a.E);      // (a rowptr past E walks nothing past it)
  a.b2 = a.b2p[0];
  if (!a.u1) a.key1 = draw_key(seed, (uint64_t)state[1], GA_SALT + 2 * salt);
  if (!a.u2) a.key2 = draw_key(seed, (uint64_t)state[1], GA_SALT + 2 * salt + 1);
  const bool is_long = end - beg > GA_LONG;
  float pb[GA_D];
  if (!is_long && end > beg) {
    ga_load_row(pb, P, a.b1, n);
    for (int64_t e = beg + sub; e < end; e += 8) ga_entry(a, pb, e);
  }
  unsigned long long mask = __ballot(is_long && sub == 0);
  while (mask) {
    const int src = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const int64_t n_s = __shfl(n, src, 64), b_s = __shfl(beg, src, 64), e_s = __shfl(end, src, 64);
    ga_load_row(pb, P, a.b1, n_s);
    for (int64_t e = b_s + lane; e < e_s; e += 64) ga_entry(a, pb, e);
  }
}

// ---- (b) ----------------------------------------------------------------------------------------------------------------
// sample-owned passes.  Scores TRANSPOSED (A operand = table tile, B operand = the batch rows), so a lane's 64 accumulator
// values of a tile all belong to ITS sample.  WITH_DA = false: the split's sum of exp; true: the split's gA partial.
template <bool WITH_DA>
__global__ __launch_bounds__(256) void ga_lse_rows_kernel(const float *__restrict__ A, const float *__restrict__ T, int64_t B, int64_t M,
                                                          float inv_temp, int64_t tiles_per_split, float *__restrict__ ps,
                                                          const float *__restrict__ lse, const float *__restrict__ g,
                                                          float *__restrict__ dap) {
  constexpr int LD = VAE_TI + 1;
  __shared__ float Ts[GA_D][LD];      // [k][table row]
  __shared__ float bs[VAE_TI];        // 0, or -inf for a table row past the end: its term is exp(-inf) = 0
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int64_t b = (int64_t)blockIdx.x * VAE_SB + wave * 32 + r;
  const bool live = b < B;
  const int64_t n_tiles = (M + VAE_TI - 1) / VAE_TI;
  const int64_t t_beg = (int64_t)blockIdx.y * tiles_per_split, t_end = min(n_tiles, t_beg + tiles_per_split);

  float bf[GA_D / 2];
#pragma unroll
  for (int s = 0; s < GA_D / 2; ++s) bf[s] = live ? A[b * GA_D + 2 * s + h] : 0.f;
  float ssum = 0.f;
  const float my_lse = WITH_DA ? (live ? lse[b] : INFINITY) : 0.f, my_lo = WITH_DA ? (live ? lse[B + b] : 0.f) : 0.f;
  const float my_coef = WITH_DA ? (live ? g[b] * inv_temp : 0.f) : 0.f;
  f32x16 da[2] = {vae_zero(), vae_zero()};

  for (int64_t tile = t_beg; tile < t_end; ++tile) {
    const int64_t i0 = tile * VAE_TI;
    __syncthreads();
    vae_stage_transposed<VAE_TI>(Ts, T, i0, M, t);
    if (t < VAE_TI) bs[t] = (i0 + t < M) ? 0.f : -INFINITY;
    __syncthreads();
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      f32x16 acc = vae_zero();
#pragma unroll
      for (int s = 0; s < GA_D / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ts[2 * s + h][32 * jt + r], bf[s], acc, 0, 0, 0);
      if (!WITH_DA) {
#pragma unroll
        for (int q = 0; q < 16; ++q) ssum += expf(acc[q] * inv_temp + bs[32 * jt + vae_row(q, h)]);
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = my_coef * expf(((acc[q] * inv_temp + bs[32 * jt + vae_row(q, h)]) - my_lse) - my_lo);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int item = 32 * jt + vae_row(q, h);
#pragma unroll
          for (int j = 0; j < 2; ++j) da[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ts[32 * j + r][item], acc[q], da[j], 0, 0, 0);
        }
      }
    }
  }
  if (!WITH_DA) {
    const float s2 = __shfl_xor(ssum, 32, 64);      // the two half-waves saw different table rows of the same sample
    if (live && h == 0) ps[(int64_t)blockIdx.y * B + b] = ssum + s2;
  } else if (live) {
    vae_store_dz(dap + ((int64_t)blockIdx.y * B + b) * GA_D, da, h);
  }
}

// lse[b] = log of the split partials' sum, split order, in double; lse[B + b] = what rounding it to fp32 lost: the backward
// subtracts the two in turn, so that its exponent (score - lse) does not carry lse's rounding (1e-6 at lse = 20) into every w
__global__ __launch_bounds__(256) void ga_lse_finish_kernel(const float *__restrict__ ps, int64_t B, int splits, float *__restrict__ lse) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int sp = 0; sp < splits; ++sp) s += (double)ps[(int64_t)sp * B + b];
  const double l = log(s);
  lse[b] = (float)l;
  lse[B + b] = (float)(l - (double)(float)l);
}

// gA[b][d] = the split partials' sum, split order
__global__ __launch_bounds__(256) void ga_da_finish_kernel(const float *__restrict__ dap, int64_t n, int splits, float *__restrict__ dA) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v = 0.f;
  for (int sp = 0; sp < splits; ++sp) v += dap[(int64_t)sp * n + i];
  dA[i] = v;
}

// table-owned pass: scores as [sample][table row] (A operand = the batch block, B operand = the table tile), so lane & 31 =
// the table row and w^T A takes w straight from the accumulator as its A operand.
__global__ __launch_bounds__(256) void ga_lse_dt_kernel(const float *__restrict__ A, const float *__restrict__ T, int64_t B, int64_t M,
                                                        float inv_temp, const float *__restrict__ lse, const float *__restrict__ g,
                                                        float *__restrict__ dT) {
  constexpr int LD = GA_D + 1;
  __shared__ float Ts[GA_D][VAE_TW + 1];    // [k][table row]
  __shared__ float As[VAE_SB][LD];          // [sample][k]
  float (*Rs)[LD] = reinterpret_cast<float (*)[LD]>(&As[0][0]);   // [table row][d]: the waves' sums, once As is done with
  __shared__ float lses[VAE_SB], lsel[VAE_SB], coefs[VAE_SB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int64_t i0 = (int64_t)blockIdx.x * VAE_TW;
  vae_stage_transposed<VAE_TW>(Ts, T, i0, M, t);
  float bias[2];
#pragma unroll
  for (int jt = 0; jt < 2; ++jt) bias[jt] = (i0 + 32 * jt + r < M) ? 0.f : -INFINITY;
  f32x16 dw[2][2] = {{vae_zero(), vae_zero()}, {vae_zero(), vae_zero()}};

  for (int64_t s0 = 0; s0 < B; s0 += VAE_SB) {
    __syncthreads();
    vae_stage_rows(As, A, GA_D, s0, B, t);
    if (t < VAE_SB) {
      const bool live = s0 + t < B;
      lses[t] = live ? lse[s0 + t] : INFINITY;          // a sample past the end: w = 0 exp(-inf) = 0
      lsel[t] = live ? lse[B + s0 + t] : 0.f;
      coefs[t] = live ? g[s0 + t] * inv_temp : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int jt = 0; jt < 2; ++jt) {
      f32x16 acc = vae_zero();
#pragma unroll
      for (int s = 0; s < GA_D / 2; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[wave * 32 + r][2 * s + h], Ts[2 * s + h][32 * jt + r], acc, 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int sm = wave * 32 + vae_row(q, h);
        acc[q] = coefs[sm] * expf(((acc[q] * inv_temp + bias[jt]) - lses[sm]) - lsel[sm]);
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int sm = wave * 32 + vae_row(q, h);
#pragma unroll
        for (int j = 0; j < 2; ++j) dw[jt][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[q], As[sm][32 * j + r], dw[jt][j], 0, 0, 0);
      }
    }
  }
  vae_reduce_waves(Rs, dw, wave, r, h);
  for (int it = wave; it < VAE_TW; it += 4) {
    const int64_t i = i0 + it;
    if (i >= M) break;
    dT[i * GA_D + lane] = Rs[it][lane];
  }
}

// ---- (c) ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ga_rand_spmm_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t N,
                                                           int64_t n_cols, const float *__restrict__ x, const float *__restrict__ z,
                                                           float alpha, float slope, float *__restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const int64_t beg = rowptr[n], end = rowptr[n + 1];
  float acc = 0.f;
  for (int64_t e = beg; e < end; ++e) acc += x[(int64_t)clamp_index(col[e], n_cols) * GA_D + lane];
  float v = alpha * acc;
  if (z) v = z[n * GA_D + lane] + v;
  y[n * GA_D + lane] = v > 0.f ? v : slope * v;
}

}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_graphaug_check_shape(int32_t D) {
  if (D != GA_D) return fail(CHAOREC_E_INVALID, "graphaug_check_shape: D=%d, the kernels tile D=%d", (int)D, GA_D);
  return CHAOREC_OK;
}

extern "C" int64_t chaorec_graphaug_rows_per_block(void) { return GA_RB; }
extern "C" int64_t chaorec_graphaug_long_row(void) { return GA_LONG; }

extern "C" int64_t chaorec_graphaug_lse_splits(int64_t B, int64_t M) {
  if (B <= 0 || M <= 0) return 1;
  int64_t s, tp;
  vae_split_plan(B, M, 1, s, tp);
  return s;
}

extern "C" int chaorec_graphaug_sample_f32(const int64_t *rowptr, const int32_t *col, const int32_t *tentry, int64_t N, int64_t E,
                                           const float *P, const float *Q, const float *b1, const float *w2, const float *b2,
                                           const float *u1, const float *u2, uint64_t seed, const int64_t *state, int32_t salt,
                                           float *val, float *val_t, float *logit_out, float *u_out, void *stream) {
  if (!rowptr || !col || !P || !Q || !b1 || !w2 || !b2 || !val) return fail(CHAOREC_E_INVALID, "graphaug_sample: NULL argument");
  if (N <= 0 || E <= 0 || N >= ((int64_t)1 << 31) - GA_RB || E >= ((int64_t)1 << 31) - 256)
    return fail(CHAOREC_E_INVALID, "graphaug_sample: N=%lld E=%lld", (long long)N, (long long)E);
  if (val_t && !tentry) return fail(CHAOREC_E_INVALID, "graphaug_sample: val_t without tentry");
  if ((!u1 || !u2) && !state) return fail(CHAOREC_E_INVALID, "graphaug_sample: neither draws nor a step counter");
  if (salt < 0) return fail(CHAOREC_E_INVALID, "graphaug_sample: salt=%d", (int)salt);
  if ((reinterpret_cast<uintptr_t>(P) & 15) || (reinterpret_cast<uintptr_t>(Q) & 15))
    return fail(CHAOREC_E_INVALID, "graphaug_sample: P and Q must be 16-byte aligned");
  GaSample a;
  a.col = col;
  a.tentry = tentry;
  a.Q = Q;
  a.b1 = b1;
  a.w2 = w2;
  a.u1 = u1;
  a.u2 = u2;
  a.val = val;
  a.val_t = val_t;
  a.logit_out = logit_out;
  a.u_out = u_out;
  a.N = N;
  a.E = E;
  a.b2p = b2;
  a.b2 = 0.f;
  a.key1 = a.key2 = 0;
  hipLaunchKernelGGL(ga_sample_kernel, dim3((unsigned)((N + GA_RB - 1) / GA_RB)), dim3(256), 0, (hipStream_t)stream, rowptr, P, a, seed,
                     state, (uint64_t)salt);
  return check_launch("graphaug_sample");
}

static int ga_lse_check(const char *what, int64_t B, int64_t M, int64_t splits, int64_t &tp) {
  if (B <= 0 || M <= 0 || B >= ((int64_t)1 << 31) - VAE_SB || M >= ((int64_t)1 << 31) - VAE_TI)
    return fail(CHAOREC_E_INVALID, "%s: B=%lld M=%lld", what, (long long)B, (long long)M);
  int64_t s;
  vae_split_plan(B, M, 1, s, tp);
  if (splits != s)
    return fail(CHAOREC_E_WORKSPACE, "%s: splits %lld, chaorec_graphaug_lse_splits says %lld", what, (long long)splits, (long long)s);
  return CHAOREC_OK;
}

extern "C" int chaorec_graphaug_lse_fwd_f32(const float *A, const float *T, int64_t B, int64_t M, float inv_temp, float *part,
                                            int64_t splits, float *lse, void *stream) {
  if (!A || !T || !part || !lse) return fail(CHAOREC_E_INVALID, "graphaug_lse_fwd: NULL argument");
  if ((reinterpret_cast<uintptr_t>(A) & 15) || (reinterpret_cast<uintptr_t>(T) & 15))
    return fail(CHAOREC_E_INVALID, "graphaug_lse_fwd: A and T must be 16-byte aligned");
  int64_t tp;
  if (int rc = ga_lse_check("graphaug_lse_fwd", B, M, splits, tp)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((B + VAE_SB - 1) / VAE_SB), (unsigned)splits);
  hipLaunchKernelGGL((ga_lse_rows_kernel<false>), grid, dim3(256), 0, st, A, T, B, M, inv_temp, tp, part, (const float *)nullptr,
                     (const float *)nullptr, (float *)nullptr);
  hipLaunchKernelGGL(ga_lse_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, part, B, (int)splits, lse);
  return check_launch("graphaug_lse_fwd");
}

extern "C" int chaorec_graphaug_lse_bwd_f32(const float *A, const float *T, int64_t B, int64_t M, float inv_temp, const float *lse,
                                            const float *g, float *part, int64_t splits, float *dA, float *dT, void *stream) {
  if (!A || !T || !lse || !g || !part || !dA || !dT) return fail(CHAOREC_E_INVALID, "graphaug_lse_bwd: NULL argument");
  if ((reinterpret_cast<uintptr_t>(A) & 15) || (reinterpret_cast<uintptr_t>(T) & 15) || (reinterpret_cast<uintptr_t>(part) & 15))
    return fail(CHAOREC_E_INVALID, "graphaug_lse_bwd: A, T and part must be 16-byte aligned");
  int64_t tp;
  if (int rc = ga_lse_check("graphaug_lse_bwd", B, M, splits, tp)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((B + VAE_SB - 1) / VAE_SB), (unsigned)splits);
  hipLaunchKernelGGL((ga_lse_rows_kernel<true>), grid, dim3(256), 0, st, A, T, B, M, inv_temp, tp, (float *)nullptr, lse, g, part);
  hipLaunchKernelGGL(ga_da_finish_kernel, dim3((unsigned)((B * GA_D + 255) / 256)), dim3(256), 0, st, part, B * GA_D, (int)splits, dA);
  hipLaunchKernelGGL(ga_lse_dt_kernel, dim3((unsigned)((M + VAE_TW - 1) / VAE_TW)), dim3(256), 0, st, A, T, B, M, inv_temp, lse, g, dT);
  return check_launch("graphaug_lse_bwd");
}

extern "C" int chaorec_graphaug_rand_spmm_f32(const int64_t *rowptr, const int32_t *col, int64_t n_rows, int64_t n_cols, const float *x,
                                              const float *z, float alpha, float slope, float *y, void *stream) {
  if (!rowptr || !col || !x || !y) return fail(CHAOREC_E_INVALID, "graphaug_rand_spmm: NULL argument");
  if (n_rows <= 0 || n_cols <= 0 || n_rows >= ((int64_t)1 << 33))
    return fail(CHAOREC_E_INVALID, "graphaug_rand_spmm: n_rows=%lld n_cols=%lld", (long long)n_rows, (long long)n_cols);
  hipLaunchKernelGGL(ga_rand_spmm_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rowptr, col, n_rows,
                     n_cols, x, z, alpha, slope, y);
  return check_launch("graphaug_rand_spmm");
}
