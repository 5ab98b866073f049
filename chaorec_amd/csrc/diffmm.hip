// DiffMM's diffusion half (Model/DiffMM.py:437-473, 580-592, 624-660): the noised, dropped-out input rows of the denoiser
// straight from the user-history CSR, and the denoiser's output layer with both losses and the complete gradient by the
// layer's output in one pass over the tiles of `out`.  Additive to ABI 16.  fp32, no atomics on floats, no scratch.
//
// (a) dm_rows_kernel      users -> x_in [B, ld] and the bit table of x0 (uint32 [B, ceil(I / 32)]), one wave per row
// (b) dm_out_loss_kernel  d_out = c_b (h W_out^T + b_out - x0) + k (r F^T) on the f32 MFMA pipe, per-row partials of err^2
// (c) dm_reduce_kernel    the row partials in item-tile order -> diff_rows, gc_rows, loss (double, one fixed order)
#include "vae_common.h"

namespace chaorec {

constexpr int DM_ROWS = 4;        // rows per workgroup of (a): one wave each
constexpr int DM_CH = 2048;       // items per pass of a wave over its row: 64 words of the bit table, one per lane
constexpr int DM_BM = 128, DM_BN = 128, DM_BK = 16, DM_PAD = 4;   // (b)'s tile: waves 2 x 2 of 64 x 64, as gemm.hip's <128, 128>
constexpr int DM_D = 64;          // the embedding width of r and F
constexpr int DM_SEG = 64;        // k per segment of the out-layer's chain (a multiple of DM_BK)
constexpr int DM_BITS = 24;       // random bits of a uniform

// (a) Row b of the batch is user u = users[b] (history empty for an id outside [0, U)).  Per pass of DM_CH items the wave
// ORs the row's entries into 64 LDS words (integer OR: any order gives the same word), lane l writes word l of the pass to
// the bit table, and every lane then writes 8 float4 of x_in.  plain: x_in = x0.  Otherwise
//   x_t = fl(fl(a x0) + fl(s n)),  x_in = kept ? fl(2 x_t) : 0
// n = noise[b, i] or normal(seed, step, 2 salt, u, i); kept = keep[b, i] != 0 or uniform(seed, step, 2 salt + 1, u, i) < 1/2:
// the place in the batch is not part of a draw's key.  Columns I .. ld of a row are written 0.  plain == 2: x_in = x_t, no
// dropout and no keep draw (chaorec_diffmm_rows_noised_f32: CF_Diff drops out after its encoder, not before).
template <class = void>
static __global__ __launch_bounds__(64 * DM_ROWS) void dm_rows_kernel(
    const int64_t *__restrict__ users, int64_t B, int64_t U, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    int64_t I, int64_t ld, const float *__restrict__ a_row, const float *__restrict__ s_row, const float *__restrict__ noise,
    const uint8_t *__restrict__ keep, uint64_t seed, uint64_t step, uint64_t salt, int plain, float *__restrict__ x_in,
    uint32_t *__restrict__ bits, int64_t nwords) {
  __shared__ uint32_t words[DM_ROWS][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * DM_ROWS + wave;
  const bool live = b < B;
  const int64_t u = live ? users[b] : -1;
  const VaeHistRow hr = vae_hist_row(rowptr, u, U);
  const float a = (live && plain != 1) ? a_row[b] : 1.f, s = (live && plain != 1) ? s_row[b] : 0.f;
  const uint64_t key_n = draw_key(seed, step, 2 * salt), key_k = draw_key(seed, step, 2 * salt + 1);
  for (int64_t c0 = 0; c0 < ld; c0 += DM_CH) {      // the same trip count for every wave of the workgroup
    words[wave][lane] = 0u;
    __syncthreads();
    for (int64_t e = lane; e < hr.n; e += 64) {
      const int64_t c = (int64_t)col[hr.beg + e] - c0;
      if (c >= 0 && c < DM_CH && c + c0 < I) atomicOr(&words[wave][c >> 5], 1u << (c & 31));
    }
    __syncthreads();
    if (live) {
      const int64_t w = (c0 >> 5) + lane;
      if (w < nwords) bits[b * nwords + w] = words[wave][lane];
#pragma unroll
      for (int p = 0; p < DM_CH / 4 / 64; ++p) {
        const int v = p * 64 + lane;
        const int64_t i0 = c0 + 4 * v;
        if (i0 >= ld) continue;
        const uint32_t word = words[wave][v >> 3];
        float o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t i = i0 + q;
          float x = 0.f;
          if (i < I) {
            const float x0 = ((word >> ((4 * v + q) & 31)) & 1u) ? 1.f : 0.f;
            if (plain == 1) x = x0;
            else {
              const float n = noise ? noise[b * I + i] : draw_normal<DM_BITS>(key_n, (uint64_t)u, (uint64_t)i);
              const bool kept = plain == 2 || (keep ? keep[b * I + i] != 0 : draw_uniform<DM_BITS>(key_k, (uint64_t)u, (uint64_t)i) < 0.5f);
              const float xt = add_rn(mul_rn(a, x0), mul_rn(s, n));
              x = plain == 2 ? xt : (kept ? mul_rn(2.f, xt) : 0.f);
            }
          }
          o[q] = x;
        }
        *reinterpret_cast<float4 *>(x_in + b * ld + i0) = make_float4(o[0], o[1], o[2], o[3]);
      }
    }
    __syncthreads();
  }
}

// (b) One 128 x 128 tile of out = h W_out^T per workgroup.  The K = H loop is gemm.hip's: operand tiles staged k-major in
// LDS, double-buffered, the k-ascending fmaf chain of v_mfma_f32_32x32x2_f32 per element -- in segments of DM_SEG = 64 k: after
// every fourth tile the chain's value is added to a running sum and the chain restarts from zero (segments in ascending order,
// the same bits every run).  One chain over K = 1000 rounds a thousand times at the magnitude of its growing partial sum and
// deviated 4 to 5 times as much as torch's blocked fp32 sum (measured against float64 at H = 1000: 1.0 to 1.3e-6 of the
// largest |d_out|, torch 2.5 to 3e-7); the running sum lives in the accumulators the second chain needs anyway.
// Epilogue, in registers:
//   err = (acc + b_out[i]) - x0[b, i]      (x0 from the bit table: the 32 columns of a lane group are one word)
//   the tile's share of sum_i err^2 per row: columns in a fixed butterfly order, then the two column halves in order
//   acc = c_b err, then 64 more k-steps over (r, F) into a SECOND set of accumulators, acc2 = r_b . F_i from zero,
// and c_b err + k acc2 is stored once.  (Continuing the chain on c_b err instead would save 64 registers and round 64 times at
// the magnitude of c_b err, which at small B I is a thousand times that of the chain's terms: measured, 8 ulp of d_out.)
// Workgroups are dealt to the 8 XCDs round-robin: block id -> (id % 8, id / 8), and the workgroups of one XCD walk the row
// tiles of one column tile before the next, so a slice of W_out is read into one L2 and h, 4 MB, stays in all of them.
template <class = void>
static __global__ __launch_bounds__(256) void dm_out_loss_kernel(
    const float *__restrict__ h, int64_t ldh, const float *__restrict__ W, int64_t ldw, const float *__restrict__ bias,
    const uint32_t *__restrict__ bits, int64_t nwords, const float *__restrict__ r, const float *__restrict__ F,
    const float *__restrict__ c_row, float kf, int64_t B, int64_t I, int64_t H, int64_t MT, int64_t NT,
    float *__restrict__ d_out, int64_t ldd, float *__restrict__ part) {
  __shared__ float As[2][DM_BK][DM_BM + DM_PAD];
  __shared__ float Bs[2][DM_BK][DM_BN + DM_PAD];
  __shared__ float Ps[2][DM_BM];
  const int64_t slot = (int64_t)blockIdx.x >> 3;
  const int64_t nt = (slot / MT) * 8 + ((int64_t)blockIdx.x & 7), mt = slot % MT;
  if (nt >= NT) return;           // the whole workgroup: no barrier has been reached
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int rr = lane & 31, hh = lane >> 5;
  const int wrow = (wave >> 1) * 64, wcol = (wave & 1) * 64;
  const int64_t m0 = mt * DM_BM, n0 = nt * DM_BN;

  f32x16 acc[2][2], acc2[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = acc2[i][j] = vae_zero();

  // acc += A[m0 .., 0 .. K) . Bm[n0 .., 0 .. K)^T; both operands [rows][k], K a multiple of 4, rows 16-byte aligned
  // sum != nullptr: every DM_SEG k, sum += acc and acc = 0 (the caller adds the last, partial segment)
  auto run = [&](f32x16 (&acc)[2][2], f32x16 (*sum)[2], const float *__restrict__ A, int64_t lda, const float *__restrict__ Bm, int64_t ldb,
                 int64_t K) {
    float4 ra[2], rb[2];
    auto fetch = [&](int64_t k0) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int v = t + p * 256, row = v >> 2, k4 = (v & 3) * 4;
        const int64_t gk = k0 + k4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
        if (m0 + row < B && gk < K) x = *reinterpret_cast<const float4 *>(A + (m0 + row) * lda + gk);
        if (n0 + row < I && gk < K) y = *reinterpret_cast<const float4 *>(Bm + (n0 + row) * ldb + gk);
        ra[p] = x;
        rb[p] = y;
      }
    };
    auto stash = [&](int buf) {
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int v = t + p * 256, row = v >> 2, k4 = (v & 3) * 4;
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
    for (int64_t k0 = 0; k0 < K; k0 += DM_BK) {
      const bool more = k0 + DM_BK < K;
      if (more) fetch(k0 + DM_BK);
      float af[DM_BK / 2][2], bf[DM_BK / 2][2];
#pragma unroll
      for (int s = 0; s < DM_BK / 2; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          af[s][i] = As[buf][2 * s + hh][wrow + 32 * i + rr];
          bf[s][i] = Bs[buf][2 * s + hh][wcol + 32 * i + rr];
        }
#pragma unroll
      for (int s = 0; s < DM_BK / 2; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s][i], bf[s][j], acc[i][j], 0, 0, 0);
      if (sum && ((k0 + DM_BK) % DM_SEG) == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            sum[i][j] = sum[i][j] + acc[i][j];
            acc[i][j] = vae_zero();
          }
      }
      if (more) stash(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  };

  run(acc, acc2, h, ldh, W, ldw, H);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = acc2[i][j] + acc[i][j];

  // err, its squares per row, c_b err
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = wrow + 32 * i + vae_row(reg, hh);
      const int64_t gm = m0 + row;
      const float cb = gm < B ? c_row[gm] : 0.f;
      float sq = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t g0 = n0 + wcol + 32 * j, gn = g0 + rr;
        float err = 0.f;
        if (gm < B && gn < I) {
          const uint32_t word = bits[gm * nwords + (g0 >> 5)];
          const float x0 = ((word >> rr) & 1u) ? 1.f : 0.f;
          err = (acc[i][j][reg] + bias[gn]) - x0;
        }
        sq = sq + err * err;
        acc[i][j][reg] = cb * err;
      }
#pragma unroll
      for (int off = 1; off < 32; off <<= 1) sq = sq + __shfl_xor(sq, off, 64);   // within the 32 lanes that hold the row
      if (rr == 0) Ps[wave & 1][row] = sq;
    }
  }
  __syncthreads();
  if (t < DM_BM && m0 + t < B) part[(m0 + t) * NT + nt] = Ps[0][t] + Ps[1][t];

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc2[i][j] = vae_zero();
  run(acc2, nullptr, r, DM_D, F, DM_D, DM_D);

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t gn = n0 + wcol + 32 * j + rr;
      if (gn >= ldd) continue;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int64_t gm = m0 + wrow + 32 * i + vae_row(reg, hh);
        if (gm < B) d_out[gm * ldd + gn] = gn < I ? acc[i][j][reg] + kf * acc2[i][j][reg] : 0.f;
      }
    }
}

// (c) diff_rows[b] = w_b / I sum_tiles part[b, .] (tiles ascending, in double), gc_rows[b] = mean_d r[b, d]^2, loss =
// mean_b diff_rows + e_loss mean_b gc_rows: one workgroup, rows strided per thread, then a tree -- the same order every run.
template <class = void>
static __global__ __launch_bounds__(256) void dm_reduce_kernel(const float *__restrict__ part, int64_t NT, const float *__restrict__ r,
                                                               const double *__restrict__ w, int64_t B, int64_t I, float e_loss,
                                                               double *__restrict__ diff_rows, float *__restrict__ gc_rows,
                                                               float *__restrict__ loss) {
  __shared__ double red[2][256];
  double sd = 0.0, sg = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    double sq = 0.0, g = 0.0;
    for (int64_t n = 0; n < NT; ++n) sq += (double)part[b * NT + n];
    for (int d = 0; d < DM_D; ++d) g += (double)r[b * DM_D + d] * (double)r[b * DM_D + d];
    const double diff = w[b] * (sq / (double)I);
    g /= (double)DM_D;
    diff_rows[b] = diff;
    gc_rows[b] = (float)g;
    sd += diff;
    sg += g;
  }
  red[0][threadIdx.x] = sd;
  red[1][threadIdx.x] = sg;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0][0] / (double)B + (double)e_loss * (red[1][0] / (double)B));
}

static bool dm_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_diffmm_check_shape(int64_t B, int64_t I, int64_t H, int32_t D) {
  if (D != DM_D) return fail(CHAOREC_E_INVALID, "diffmm: dim_E=%d, the kernels tile D=%d", D, DM_D);
  if (B <= 0 || I <= 0 || H <= 0) return fail(CHAOREC_E_INVALID, "diffmm: B=%lld I=%lld H=%lld", (long long)B, (long long)I, (long long)H);
  if (H % 4) return fail(CHAOREC_E_INVALID, "diffmm: H=%lld is no multiple of 4 (rows are read as float4)", (long long)H);
  if (I > ((int64_t)1 << 31) - 256) return fail(CHAOREC_E_INVALID, "diffmm: I=%lld", (long long)I);
  return CHAOREC_OK;
}

extern "C" int chaorec_diffmm_tiles(int32_t *bm, int32_t *bn, int32_t *bk) {
  if (!bm || !bn || !bk) return fail(CHAOREC_E_INVALID, "diffmm_tiles: NULL argument");
  *bm = DM_BM;
  *bn = DM_BN;
  *bk = DM_BK;
  return CHAOREC_OK;
}

extern "C" int64_t chaorec_diffmm_rows_per_block(void) { return DM_ROWS; }

extern "C" int chaorec_diffmm_rows_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                       int64_t I, int64_t ld, const float *a_row, const float *s_row, const float *noise,
                                       const uint8_t *keep, uint64_t seed, uint64_t step, uint32_t salt, int32_t plain,
                                       float *x_in, uint32_t *bits, void *stream) {
  if (!users || !rowptr || !col || !x_in || !bits) return fail(CHAOREC_E_INVALID, "diffmm_rows: NULL argument");
  if (!plain && (!a_row || !s_row)) return fail(CHAOREC_E_INVALID, "diffmm_rows: a_row / s_row missing");
  if (B < 0 || U < 0 || I <= 0 || I > ((int64_t)1 << 31) - 256) return fail(CHAOREC_E_INVALID, "diffmm_rows: B=%lld I=%lld", (long long)B, (long long)I);
  if (ld != (I + 3) / 4 * 4 || !dm_aligned16(x_in)) return fail(CHAOREC_E_INVALID, "diffmm_rows: ld=%lld must be I rounded up to 4, x_in 16-byte aligned", (long long)ld);
  if (B == 0) return CHAOREC_OK;
  hipLaunchKernelGGL(dm_rows_kernel<>, dim3((unsigned)((B + DM_ROWS - 1) / DM_ROWS)), dim3(64 * DM_ROWS), 0, (hipStream_t)stream, users,
                     B, U, rowptr, col, I, ld, a_row, s_row, noise, keep, seed, step, (uint64_t)salt, plain ? 1 : 0, x_in, bits, (I + 31) / 32);
  return check_launch("dm_rows_kernel");
}

extern "C" int chaorec_diffmm_rows_noised_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                              int64_t I, int64_t ld, const float *a_row, const float *s_row, const float *noise,
                                              uint64_t seed, uint64_t step, uint32_t salt, float *x_t, uint32_t *bits, void *stream) {
  if (!users || !rowptr || !col || !x_t || !bits || !a_row || !s_row) return fail(CHAOREC_E_INVALID, "diffmm_rows_noised: NULL argument");
  if (B < 0 || U < 0 || I <= 0 || I > ((int64_t)1 << 31) - 256) return fail(CHAOREC_E_INVALID, "diffmm_rows_noised: B=%lld I=%lld", (long long)B, (long long)I);
  if (ld != (I + 3) / 4 * 4 || !dm_aligned16(x_t)) return fail(CHAOREC_E_INVALID, "diffmm_rows_noised: ld=%lld must be I rounded up to 4, x_t 16-byte aligned", (long long)ld);
  if (B == 0) return CHAOREC_OK;
  hipLaunchKernelGGL(dm_rows_kernel<>, dim3((unsigned)((B + DM_ROWS - 1) / DM_ROWS)), dim3(64 * DM_ROWS), 0, (hipStream_t)stream, users,
                     B, U, rowptr, col, I, ld, a_row, s_row, noise, (const uint8_t *)nullptr, seed, step, (uint64_t)salt, 2, x_t, bits, (I + 31) / 32);
  return check_launch("dm_rows_kernel");
}

extern "C" int chaorec_diffmm_out_loss_f32(const float *h, int64_t ldh, const float *W_out, int64_t ldw, const float *b_out,
                                           const uint32_t *bits, const float *r, const float *F, const double *w,
                                           const float *c_row, float kf, float e_loss, int64_t B, int64_t I, int64_t H,
                                           float *d_out, int64_t ldd, float *part, double *diff_rows, float *gc_rows,
                                           float *loss, void *stream) {
  if (!h || !W_out || !b_out || !bits || !r || !F || !w || !c_row || !d_out || !part || !diff_rows || !gc_rows || !loss)
    return fail(CHAOREC_E_INVALID, "diffmm_out_loss: NULL argument");
  if (int rc = chaorec_diffmm_check_shape(B, I, H, DM_D)) return rc;
  if (ldh < H || ldw < H || (ldh & 3) || (ldw & 3) || ldd < I || !dm_aligned16(h) || !dm_aligned16(W_out) || !dm_aligned16(r) || !dm_aligned16(F))
    return fail(CHAOREC_E_INVALID, "diffmm_out_loss: h, W_out, r, F must be 16-byte aligned with row strides that are multiples of 4");
  const int64_t MT = (B + DM_BM - 1) / DM_BM, NT = (I + DM_BN - 1) / DM_BN;
  if (ldd > NT * DM_BN) return fail(CHAOREC_E_INVALID, "diffmm_out_loss: ldd=%lld past the last item tile", (long long)ldd);
  const int64_t blocks = (NT + 7) / 8 * MT * 8;
  if (blocks > 0x7fffffff) return fail(CHAOREC_E_INVALID, "diffmm_out_loss: %lld workgroups", (long long)blocks);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dm_out_loss_kernel<>, dim3((unsigned)blocks), dim3(256), 0, st, h, ldh, W_out, ldw, b_out, bits, (I + 31) / 32, r, F,
                     c_row, kf, B, I, H, MT, NT, d_out, ldd, part);
  if (int rc = check_launch("dm_out_loss_kernel")) return rc;
  hipLaunchKernelGGL(dm_reduce_kernel<>, dim3(1), dim3(256), 0, st, part, NT, r, w, B, I, e_loss, diff_rows, gc_rows, loss);
  return check_launch("dm_reduce_kernel");
}
