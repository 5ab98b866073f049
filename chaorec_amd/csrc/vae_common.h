// What multvae.hip, macridvae.hip and dualvae.hip share (and what graphaug.hip, adagcl.hip and diffmm.hip borrow of it): the
// tile geometry of their MFMA passes, the history-row and item-owner walks, the LDS staging of 64-float rows and the
// fixed-order reductions.  The counter RNG and the step tick are draws.h's, the arithmetic helpers common.h's.  One definition
// each: the three files keep their formulas, their kernel bodies and their exports.  Three things differ between the models ON
// PURPOSE and stay with them: the uniform's bit count (MultVAE 24, MacridVAE and -- through its epsilon -- DualVAE 23),
// the tick kernels (MultVAE reads the counter and then increments it, the other two increment first) and vae_sum_kernel's
// `accumulate` (MultVAE's sum of squares adds one parameter after the other).
// The kernels here are static templates: a file that launches one has its own copy (the link sees no duplicate), a file
// that does not has none -- `template <class = void>` is there for that alone.
#pragma once
#include "draws.h"

namespace chaorec {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int VAE_D = 64;         // floats of a row the staging helpers move (the latent width of MultVAE and MacridVAE)
constexpr int VAE_SB = 128;       // samples (rows) per workgroup: 4 waves x 32
constexpr int VAE_TI = 128;       // items (table rows) per tile of the sample-owned passes
constexpr int VAE_TW = 64;        // items (table rows) per workgroup of the item-owned passes

// row of a 32x32 MFMA accumulator register (C/D layout: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5))
__device__ __forceinline__ int vae_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
__device__ __forceinline__ f32x16 vae_zero() {
  f32x16 v;
#pragma unroll
  for (int q = 0; q < 16; ++q) v[q] = 0.f;
  return v;
}

template <int BITS>
struct VaeKeep {   // is entry j of sample b's history row kept?  given flags (parity tests) or the counter RNG
  const uint8_t *keep;
  const int64_t *keep_off;
  uint64_t key;
  float keep_prob;
  int training;
  __device__ __forceinline__ bool operator()(int64_t b, int64_t j) const {
    if (!training) return true;
    if (keep) return keep[keep_off[b] + j] != 0;
    return draw_uniform<BITS>(key, (uint64_t)b, (uint64_t)j) < keep_prob;
  }
};

// the KL weight min(cap, count / total) of the tick kernels (Model/MultVAE.py:145-148, Model/MacridVAE.py:135-137)
__device__ __forceinline__ float vae_anneal(int64_t count, int64_t total, float cap) {
  const double a = total > 0 ? (double)count / (double)total : (double)cap;
  return (float)(a < (double)cap ? a : (double)cap);
}

// the history row of user u: entries col[beg .. beg + n); n = 0 for an id outside [0, U)
struct VaeHistRow {
  int64_t beg, n;
};
__device__ __forceinline__ VaeHistRow vae_hist_row(const int64_t *__restrict__ rowptr, int64_t u, int64_t U) {
  const bool ok = u >= 0 && u < U;
  const int64_t beg = ok ? rowptr[u] : 0;
  return {beg, ok ? rowptr[u + 1] - beg : 0};
}

// F.normalize's 1 / max(|x|, 1e-12) of a multi-hot row with n ones, times dropout's 1 / keep_prob in training
__device__ __forceinline__ float vae_row_scale(int64_t n, int training, float keep_prob) {
  const float s = 1.0f / fmaxf(sqrtf((float)n), 1e-12f);
  return training ? s / keep_prob : s;
}

// The owner walk: item i's users (item-major CSR, ascending; item_pos: each entry's place in its user's row, or nullptr),
// per user the sample slots perm[slot_ptr[u] .. slot_ptr[u + 1]) (ascending sample number: a stable sort of the batch).
// 64 lanes scan 64 users at a time; the users that are in the batch are then taken one by one, in order, by the WHOLE
// wave: f(slot, pos), users ascending, slots ascending -- that order is what makes two runs give the same bits.
// (DualVAE walks a table row's samples with it: the transposed CSR of whichever side the batch is on, no item_pos.)
template <class F>
__device__ __forceinline__ void vae_item_walk(int64_t i, const int64_t *__restrict__ item_ptr, const int32_t *__restrict__ item_users,
                                              const int32_t *__restrict__ item_pos, const int64_t *__restrict__ slot_ptr,
                                              const int64_t *__restrict__ perm, int lane, F f) {
  const int64_t beg = item_ptr[i], end = item_ptr[i + 1];
  for (int64_t e0 = beg; e0 < end; e0 += 64) {
    const int64_t e = e0 + lane;
    int64_t lo = 0, hi = 0;
    int pos = 0;
    if (e < end) {
      const int64_t u = item_users[e];
      lo = slot_ptr[u];
      hi = slot_ptr[u + 1];
      pos = item_pos ? item_pos[e] : 0;
    }
    unsigned long long mask = __ballot(hi > lo);
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int64_t lo_s = __shfl(lo, src, 64), hi_s = __shfl(hi, src, 64);
      const int pos_s = __shfl(pos, src, 64);
      for (int64_t q = lo_s; q < hi_s; ++q) f(perm[q], pos_s);
    }
  }
}

// LDS staging by the 256 threads of a workgroup, one float4 per thread and pass: rows r0 .. r0 + ROWS of src (VAE_D floats
// each, row r at src + r * VAE_D), zero from r_end on, TRANSPOSED into dst[k][row] ...
template <int ROWS>
__device__ __forceinline__ void vae_stage_transposed(float (*dst)[ROWS + 1], const float *__restrict__ src, int64_t r0, int64_t r_end,
                                                     int t) {
#pragma unroll
  for (int p = 0; p < ROWS * VAE_D / 4 / 256; ++p) {
    const int v = t + p * 256, row = v >> 4, k4 = (v & 15) * 4;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row < r_end) x = *reinterpret_cast<const float4 *>(src + (r0 + row) * VAE_D + k4);
    dst[k4 + 0][row] = x.x;
    dst[k4 + 1][row] = x.y;
    dst[k4 + 2][row] = x.z;
    dst[k4 + 3][row] = x.w;
  }
}
// ... and a block of VAE_SB rows as it is, dst[row][k]; row r at src + r * stride
__device__ __forceinline__ void vae_stage_rows(float (*dst)[VAE_D + 1], const float *__restrict__ src, int64_t stride, int64_t r0,
                                               int64_t r_end, int t) {
#pragma unroll
  for (int p = 0; p < VAE_SB * VAE_D / 4 / 256; ++p) {
    const int v = t + p * 256, row = v >> 4, k4 = (v & 15) * 4;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row < r_end) x = *reinterpret_cast<const float4 *>(src + (r0 + row) * stride + k4);
    dst[row][k4 + 0] = x.x;
    dst[row][k4 + 1] = x.y;
    dst[row][k4 + 2] = x.z;
    dst[row][k4 + 3] = x.w;
  }
}

// a lane's dz^T accumulators (row = d = 32 j + vae_row(reg, h), column = its sample) -> out[0 .. 64)
__device__ __forceinline__ void vae_store_dz(float *__restrict__ out, const f32x16 (&dz)[2], int h) {
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g)     // registers 4g .. 4g+3: d = 32 j + 8 g + 4 h + (0..3)
      *reinterpret_cast<float4 *>(out + 32 * j + 8 * g + 4 * h) =
          make_float4(dz[j][4 * g + 0], dz[j][4 * g + 1], dz[j][4 * g + 2], dz[j][4 * g + 3]);
}

// Rs[item][d] = the four waves' dw, added in wave order 0..3 (every workgroup thread calls; Rs is readable on return).
// dw[jt][j]: row = item 32 jt + vae_row(reg, h), col = d = 32 j + r
__device__ __forceinline__ void vae_reduce_waves(float (*Rs)[VAE_D + 1], const f32x16 (&dw)[2][2], int wave, int r, int h) {
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            float *dst = &Rs[32 * jt + vae_row(q, h)][32 * j + r];
            *dst = (w ? *dst : 0.f) + dw[jt][j][q];
          }
    }
  }
  __syncthreads();
}

// out[0] (+)= sum(in[0..n)) * scale, one workgroup, fixed order, summed in double (the result is one fp32 rounding away
// from the exact sum of its fp32 terms: the loss parts are compared at a few ulp)
template <class = void>
static __global__ __launch_bounds__(256) void vae_sum_kernel(const float *__restrict__ in, int64_t n, float scale, float *__restrict__ out,
                                                             int accumulate) {
  __shared__ double red[256];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) v += (double)in[i];
  block_sum_f64(v, red);
  if (threadIdx.x == 0) out[0] = (float)((accumulate ? (double)out[0] : 0.0) + red[0] * (double)scale);
}

// scores[u - u0, i] = mask for the history entries of users u0 .. u1 (the rankers' masking of seen items): one wave per user
template <class = void>
static __global__ __launch_bounds__(256) void vae_mask_kernel(float *__restrict__ scores, int64_t u0, int64_t u1, int64_t I,
                                                              const int64_t *__restrict__ rowptr, const int64_t *__restrict__ col, float mask) {
  const int lane = threadIdx.x & 63;
  const int64_t u = u0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= u1) return;
  for (int64_t e = rowptr[u] + lane; e < rowptr[u + 1]; e += 64) {
    const int64_t i = col[e];
    if (i >= 0 && i < I) scores[(u - u0) * I + i] = mask;
  }
}

// how the sample-owned passes cut the N / VAE_TI tiles into splits: ~4 workgroups per CU over (sample blocks, groups, splits)
// -- groups = what else the grid runs over (concepts, aspects) --, at most 64 splits, none empty
inline void vae_split_plan(int64_t B, int64_t N, int64_t groups, int64_t &splits, int64_t &tiles_per_split) {
  const int64_t n_tiles = (N + VAE_TI - 1) / VAE_TI, wgs = (B + VAE_SB - 1) / VAE_SB * groups;
  int64_t want = (1024 + wgs - 1) / wgs;
  if (want > 64) want = 64;
  if (want > n_tiles) want = n_tiles;
  if (want < 1) want = 1;
  tiles_per_split = (n_tiles + want - 1) / want;
  if (tiles_per_split < 1) tiles_per_split = 1;
  splits = (n_tiles + tiles_per_split - 1) / tiles_per_split;
  if (splits < 1) splits = 1;
}

}  // namespace chaorec
