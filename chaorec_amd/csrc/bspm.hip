// BSPM (Model/BSPM.py:133-181): the training-free blur / sharpen filter, scored for a tile of B users.  gfx950, fp32.
//
// Everything lives in item space (DESIGN: "BSPM"): P = Rn^T Rn [I, I] as a CSR, X = the tile's rows of Rn, and the ODE state
// is kept TRANSPOSED, Yt [I, B] with the B users of the tile contiguous -- the operand layout of the reference's own product,
// torch.sparse.mm(linear_Filter, r.t()).t().  Three launches of this file around the SpMM's:
//     project    Z[b, :]   = sum_e xval[e] F[item[e], :]                         the IDL term's first factor, [B, m]
//     seed       Y0t[j, :] = beta idlT[j, :] + sum_{i in P_j} P_ji Xt[i, :]      Xt = X^T kept sparse, never dense
//     last_step  scores[b, j] = Yt[j, b] - h (P Yt)[j, b], history = mask_value  the final Euler step, stored [B, I] row-major
// Xt is a tile-local CSR over items: xt_ptr int64 [I + 1], xt_slot int32 (the slot 0 .. B - 1 within the tile, ascending inside
// an item), xt_val f32.
//
// Every output element has one owner and every sum a fixed order (a row's entries in CSR order; a long row's four quarters in
// quarter order): no float atomics, the same bits on every run.
//
// last_step is the model's dense cost (with K_s = 1 it is all of it): nnz(P) gathered rows of B floats.  A workgroup of four
// waves owns a tile of BS_TJ = 32 items x BS_TB = 256 slots: a wave holds a row's 256 slots as 64 lanes x float4 (full 16-byte
// loads of 1 KiB per gathered row), walks the row's entries four gathers in flight and leaves the finished row in LDS; the
// tile is then written transposed, 32 consecutive items (one 128-byte line) per slot and store instruction.  The LDS rows are
// 260 floats apart: the float4 reads of the transposed store (16 lanes of consecutive items) then fall on 64 different banks.
// A row longer than BS_LONG entries would leave three waves waiting for the fourth: its entries are cut into four contiguous
// quarters, one per wave, and the partial rows are added in quarter order through LDS.
#include <math.h>
#include "common.h"

namespace chaorec {

constexpr int BS_TJ = 32;            // items per last_step workgroup
constexpr int BS_TB = 256;           // slots per last_step workgroup: 64 lanes x float4
constexpr int BS_LD = BS_TB + 4;     // LDS row stride in floats
constexpr int BS_WAVES = 4;
constexpr int BS_LONG = 128;         // a longer row of P is shared by the workgroup's four waves
constexpr int BS_MAX_B = 1024;       // the SpMM's limit for the feature width the middle steps run at
constexpr int BS_MAX_M = 128;

__device__ __forceinline__ float4 bs_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 bs_fma4(float s, float4 v, float4 a) {
  return make_float4(fmaf(s, v.x, a.x), fmaf(s, v.y, a.y), fmaf(s, v.z, a.z), fmaf(s, v.w, a.w));
}
__device__ __forceinline__ float4 bs_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ---- project: one wave per slot, lane = columns lane and lane + 64 --------------------------------------------------------
__global__ __launch_bounds__(256) void bs_project_kernel(const int64_t *__restrict__ x_ptr, const int32_t *__restrict__ x_item,
                                                         const float *__restrict__ x_val, int64_t nx, const float *__restrict__ F,
                                                         int64_t I, int B, int m, float *__restrict__ Z) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * BS_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t beg = max((int64_t)0, x_ptr[b]), end = min(x_ptr[b + 1], nx);
  const bool lo = lane < m, hi = lane + 64 < m;
  float a0 = 0.f, a1 = 0.f;
  for (int64_t e = beg; e < end; ++e) {
    const float *row = F + clamp_index((int64_t)x_item[e], I) * m;
    const float v = x_val[e];
    if (lo) a0 = fmaf(v, row[lane], a0);
    if (hi) a1 = fmaf(v, row[lane + 64], a1);
  }
  if (lo) Z[(int64_t)b * m + lane] = a0;
  if (hi) Z[(int64_t)b * m + lane + 64] = a1;
}

// ---- seed: one wave per item row j, its B sums in LDS ----------------------------------------------------------------------
// The wave takes 64 entries of P_j at a time (a lane each), finds those whose item has slots in this tile, and walks them in
// entry order; one entry's slots are distinct, so its lanes update different words, and a wave's LDS accesses keep program order.
__global__ __launch_bounds__(256) void bs_seed_kernel(const int64_t *__restrict__ p_ptr, const int32_t *__restrict__ p_col,
                                                      const float *__restrict__ p_val, int64_t nnz, int64_t I,
                                                      const int64_t *__restrict__ xt_ptr, const int32_t *__restrict__ xt_slot,
                                                      const float *__restrict__ xt_val, int64_t nxt, int B, float beta,
                                                      const float *__restrict__ idlT, float *__restrict__ Y) {
  __shared__ float acc_all[BS_WAVES][BS_MAX_B];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * BS_WAVES + w;
  if (j >= I) return;                      // (a wave leaves whole; nothing below crosses waves)
  float *acc = acc_all[w];
  for (int b = lane; b < B; b += 64) acc[b] = 0.f;
  const int64_t beg = max((int64_t)0, p_ptr[j]), end = min(p_ptr[j + 1], nnz);
  for (int64_t e0 = beg; e0 < end; e0 += 64) {
    const int64_t e = e0 + lane;
    int64_t xb = 0, xe = 0;
    float pv = 0.f;
    if (e < end) {
      const int64_t i = clamp_index((int64_t)p_col[e], I);
      xb = max((int64_t)0, xt_ptr[i]);
      xe = min(xt_ptr[i + 1], nxt);
      pv = p_val[e];
    }
    uint64_t live = __ballot(xe > xb);
    while (live) {
      const int src = __ffsll((unsigned long long)live) - 1;
      live &= live - 1;
      const int64_t sb = __shfl(xb, src, 64), se = __shfl(xe, src, 64);
      const float p = __shfl(pv, src, 64);
      for (int64_t k = sb + lane; k < se; k += 64) {
        const int s = xt_slot[k];
        if (s >= 0 && s < B) acc[s] = fmaf(p, xt_val[k], acc[s]);
      }
    }
  }
  for (int b = lane; b < B; b += 64) {
    const float blur = acc[b];
    Y[j * B + b] = idlT ? add_rn(mul_rn(beta, idlT[j * B + b]), blur) : blur;
  }
}

// ---- last_step ---------------------------------------------------------------------------------------------------------------
// sum over entries [beg, end) of val * Yt[col, c0 + 4 lane ..], in entry order, four gathers in flight
__device__ __forceinline__ float4 bs_row_gather(const int32_t *__restrict__ p_col, const float *__restrict__ p_val, int64_t beg,
                                                int64_t end, int64_t I, const float *__restrict__ Yt, int B, int col0, bool active) {
  float4 acc = bs_zero4();
  if (!active) return acc;
  int64_t e = beg;
  for (; e + 4 <= end; e += 4) {
    const int64_t i0 = clamp_index((int64_t)p_col[e], I), i1 = clamp_index((int64_t)p_col[e + 1], I);
    const int64_t i2 = clamp_index((int64_t)p_col[e + 2], I), i3 = clamp_index((int64_t)p_col[e + 3], I);
    const float4 y0 = bs_ld4(Yt + i0 * B + col0), y1 = bs_ld4(Yt + i1 * B + col0);
    const float4 y2 = bs_ld4(Yt + i2 * B + col0), y3 = bs_ld4(Yt + i3 * B + col0);
    acc = bs_fma4(p_val[e + 3], y3, bs_fma4(p_val[e + 2], y2, bs_fma4(p_val[e + 1], y1, bs_fma4(p_val[e], y0, acc))));
  }
  for (; e < end; ++e) acc = bs_fma4(p_val[e], bs_ld4(Yt + clamp_index((int64_t)p_col[e], I) * B + col0), acc);
  return acc;
}

// y - h * s with the SpMM epilogue's roundings (alpha = -h, beta = 1): the product and the sum round separately
__device__ __forceinline__ float4 bs_step4(float4 y, float h, float4 s) {
  return make_float4(add_rn(mul_rn(-h, s.x), y.x), add_rn(mul_rn(-h, s.y), y.y), add_rn(mul_rn(-h, s.z), y.z), add_rn(mul_rn(-h, s.w), y.w));
}

__global__ __launch_bounds__(256) void bs_last_step_kernel(const int64_t *__restrict__ p_ptr, const int32_t *__restrict__ p_col,
                                                           const float *__restrict__ p_val, int64_t nnz, int64_t I,
                                                           const float *__restrict__ Yt, int B, float h,
                                                           const int64_t *__restrict__ xt_ptr, const int32_t *__restrict__ xt_slot,
                                                           int64_t nxt, float mask_value, float *__restrict__ scores) {
  __shared__ float tile[BS_TJ * BS_LD];
  __shared__ float part[BS_WAVES][BS_TB];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * BS_TJ;
  const int c0 = blockIdx.y * BS_TB;               // first slot of the tile
  const int col0 = c0 + 4 * lane;
  const bool active = col0 < B;                    // (B is a multiple of 4: a float4 is inside or outside)
  const int nj = (int)min((int64_t)BS_TJ, I - j0);

  // rows of at most BS_LONG entries: wave w takes rows w, w + 4, ...
  for (int jl = w; jl < nj; jl += BS_WAVES) {
    const int64_t j = j0 + jl;
    const int64_t beg = max((int64_t)0, p_ptr[j]), end = min(p_ptr[j + 1], nnz);
    if (end - beg > BS_LONG) continue;
    if (!active) continue;
    float4 v = bs_ld4(Yt + j * B + col0);
    if (h != 0.f) v = bs_step4(v, h, bs_row_gather(p_col, p_val, beg, end, I, Yt, B, col0, true));
    *reinterpret_cast<float4 *>(tile + jl * BS_LD + 4 * lane) = v;
  }
  // longer rows, one after the other: a quarter per wave, added in quarter order (the conditions are the workgroup's)
  for (int jl = 0; jl < nj; ++jl) {
    const int64_t j = j0 + jl;
    const int64_t beg = max((int64_t)0, p_ptr[j]), end = min(p_ptr[j + 1], nnz);
    if (end - beg <= BS_LONG) continue;
    const int64_t q = (end - beg + BS_WAVES - 1) / BS_WAVES;
    const int64_t qb = min(beg + w * q, end), qe = min(qb + q, end);
    float4 s = bs_zero4();
    if (h != 0.f) s = bs_row_gather(p_col, p_val, qb, qe, I, Yt, B, col0, active);
    *reinterpret_cast<float4 *>(&part[w][4 * lane]) = s;
    __syncthreads();
    if (w == 0 && active) {
      float4 v = bs_ld4(Yt + j * B + col0);
      if (h != 0.f) {
        float4 sum = bs_ld4(&part[0][4 * lane]);
#pragma unroll
        for (int k = 1; k < BS_WAVES; ++k) {
          const float4 pk = bs_ld4(&part[k][4 * lane]);
          sum = make_float4(sum.x + pk.x, sum.y + pk.y, sum.z + pk.z, sum.w + pk.w);
        }
        v = bs_step4(v, h, sum);
      }
      *reinterpret_cast<float4 *>(tile + jl * BS_LD + 4 * lane) = v;
    }
    __syncthreads();
  }
  __syncthreads();
  // the history mask: the (item, slot) pairs of Xt that fall into this tile
  if (xt_ptr) {
    for (int jl = w; jl < nj; jl += BS_WAVES) {
      const int64_t xb = max((int64_t)0, xt_ptr[j0 + jl]), xe = min(xt_ptr[j0 + jl + 1], nxt);
      for (int64_t k = xb + lane; k < xe; k += 64) {
        const int s = xt_slot[k] - c0;
        if (s >= 0 && s < BS_TB && s + c0 < B) tile[jl * BS_LD + s] = mask_value;
      }
    }
    __syncthreads();
  }
  // transposed store: thread = (item jl, slot quad); a store instruction writes 32 consecutive items of two slots
  const int jl = t & 31;
  if (jl < nj) {
    for (int bq = t >> 5; bq < BS_TB / 4; bq += 8) {
      const int b = c0 + 4 * bq;
      if (b >= B) break;
      const float4 v = bs_ld4(tile + jl * BS_LD + 4 * bq);
      float *out = scores + (int64_t)b * I + j0 + jl;
      out[0] = v.x;
      out[I] = v.y;
      out[2 * I] = v.z;
      out[3 * I] = v.w;
    }
  }
}

static int bs_shape(const char *what, int64_t I, int64_t B, int64_t m) {
  if (I <= 0 || I >= ((int64_t)1 << 31) - BS_TJ)
    return fail(CHAOREC_E_INVALID, "%s: I=%lld", what, (long long)I);
  if (B < 4 || B > BS_MAX_B || B % 4 != 0)
    return fail(CHAOREC_E_INVALID, "%s: B=%lld, the kernels tile a multiple of 4 in [4, %d]", what, (long long)B, BS_MAX_B);
  if (m < 4 || m > BS_MAX_M || m % 4 != 0)
    return fail(CHAOREC_E_INVALID, "%s: m=%lld, the kernels tile a multiple of 4 in [4, %d]", what, (long long)m, BS_MAX_M);
  return CHAOREC_OK;
}

static bool bs_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_bspm_check_shape(int64_t I, int64_t B, int64_t m) { return bs_shape("bspm_check_shape", I, B, m); }

extern "C" int64_t chaorec_bspm_long_row(void) { return BS_LONG; }

extern "C" int chaorec_bspm_project_f32(const int64_t *x_ptr, const int32_t *x_item, const float *x_val, int64_t nx, const float *F,
                                        int64_t I, int64_t B, int64_t m, float *Z, void *stream) {
  if (!x_ptr || !F || !Z || (nx > 0 && (!x_item || !x_val)) || nx < 0) return fail(CHAOREC_E_INVALID, "bspm_project: NULL argument");
  if (int rc = bs_shape("bspm_project", I, B, m)) return rc;
  hipLaunchKernelGGL(bs_project_kernel, dim3((unsigned)((B + BS_WAVES - 1) / BS_WAVES)), dim3(256), 0, (hipStream_t)stream, x_ptr, x_item,
                     x_val, nx, F, I, (int)B, (int)m, Z);
  return check_launch("bspm_project");
}

extern "C" int chaorec_bspm_seed_f32(const int64_t *p_ptr, const int32_t *p_col, const float *p_val, int64_t nnz, int64_t I,
                                     const int64_t *xt_ptr, const int32_t *xt_slot, const float *xt_val, int64_t nxt, int64_t B,
                                     float beta, const float *idlT, float *Y0t, void *stream) {
  if (!p_ptr || !xt_ptr || !Y0t || (nnz > 0 && (!p_col || !p_val)) || (nxt > 0 && (!xt_slot || !xt_val)) || nnz < 0 || nxt < 0)
    return fail(CHAOREC_E_INVALID, "bspm_seed: NULL argument");
  if (int rc = bs_shape("bspm_seed", I, B, 4)) return rc;
  if (!idlT && beta != 0.f) return fail(CHAOREC_E_INVALID, "bspm_seed: beta=%g without idlT", (double)beta);
  hipLaunchKernelGGL(bs_seed_kernel, dim3((unsigned)((I + BS_WAVES - 1) / BS_WAVES)), dim3(256), 0, (hipStream_t)stream, p_ptr, p_col, p_val,
                     nnz, I, xt_ptr, xt_slot, xt_val, nxt, (int)B, beta, idlT, Y0t);
  return check_launch("bspm_seed");
}

extern "C" int chaorec_bspm_last_step_f32(const int64_t *p_ptr, const int32_t *p_col, const float *p_val, int64_t nnz, int64_t I,
                                          const float *Yt, int64_t B, float h, const int64_t *xt_ptr, const int32_t *xt_slot, int64_t nxt,
                                          float mask_value, float *scores, void *stream) {
  if (!p_ptr || !Yt || !scores || (nnz > 0 && (!p_col || !p_val)) || nnz < 0 || nxt < 0 || (xt_ptr && nxt > 0 && !xt_slot))
    return fail(CHAOREC_E_INVALID, "bspm_last_step: NULL argument");
  if (int rc = bs_shape("bspm_last_step", I, B, 4)) return rc;
  if (bs_misaligned(Yt)) return fail(CHAOREC_E_INVALID, "bspm_last_step: Yt must be 16-byte aligned");
  if (Yt == scores) return fail(CHAOREC_E_INVALID, "bspm_last_step: scores must not alias Yt");
  const dim3 grid((unsigned)((I + BS_TJ - 1) / BS_TJ), (unsigned)((B + BS_TB - 1) / BS_TB));
  hipLaunchKernelGGL(bs_last_step_kernel, grid, dim3(256), 0, (hipStream_t)stream, p_ptr, p_col, p_val, nnz, I, Yt, (int)B, h, xt_ptr,
                     xt_slot, nxt, mask_value, scores);
  return check_launch("bspm_last_step");
}
