// DiffMM's diffusion half (Model/DiffMM.py:437-473, 580-592, 624-660): the noised, dropped-out input rows of the denoiser
// straight from the user-history CSR, and the denoiser's output layer with both losses and the complete gradient by the
// layer's output in one pass over the tiles of `out`.  Additive to ABI 16.  fp32, no atomics on floats, no scratch.
//
// (a) dm_rows_kernel      users -> x_in [B, ld] and the bit table of x0 (uint32 [B, ceil(I / 32)]), one wave per row
// (b) dm_out_loss_kernel  d_out = c_b (h W_out^T + b_out - x0) + k (r F^T) on the f32 MFMA pipe, per-row partials of err^2
// (c) dm_reduce_kernel    the row partials in item-tile order -> diff_rows, gc_rows, loss (double, one fixed order)
//
// The tile of (b) -- its placement, its K loop and the x0-error epilogue -- is out_tile.h's, shared with diffrec.hip.
#include "out_tile.h"

namespace chaorec {

constexpr int DM_ROWS = 4;        // rows per workgroup of (a): one wave each
constexpr int DM_CH = 2048;       // items per pass of a wave over its row: 64 words of the bit table, one per lane
constexpr int DM_D = 64;          // the embedding width of r and F
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

// (b) One tile of out = h W_out^T per workgroup: out_tile.h's placement, its segmented K = H loop and its x0-error epilogue,
// which leaves acc = c_b err and the row partials.  Then 64 more k-steps over (r, F) into a second set of accumulators,
// acc2 = r_b . F_i from zero and unsegmented (out_tile.h gives the measured reason), and c_b err + k acc2 is stored once.
template <class = void>
static __global__ __launch_bounds__(256) void dm_out_loss_kernel(
    const float *__restrict__ h, int64_t ldh, const float *__restrict__ W, int64_t ldw, const float *__restrict__ bias,
    const uint32_t *__restrict__ bits, int64_t nwords, const float *__restrict__ r, const float *__restrict__ F,
    const float *__restrict__ c_row, float kf, int64_t B, int64_t I, int64_t H, int64_t MT, int64_t NT,
    float *__restrict__ d_out, int64_t ldd, float *__restrict__ part) {
  __shared__ OtStage As, Bs;
  __shared__ float Ps[2][OT_BM];
  const OutTile tp = out_tile_place(MT, NT);
  if (!tp.live) return;           // the whole workgroup: no barrier has been reached

  f32x16 acc[2][2], acc2[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = acc2[i][j] = vae_zero();

  out_tile_run<true>(acc, tp, As, Bs, h, ldh, W, ldw, B, I, H);
  out_tile_x0_err(acc, tp, Ps, bias, bits, nwords, c_row, B, I, NT, part);
  out_tile_run<false>(acc2, tp, As, Bs, r, DM_D, F, DM_D, B, I, DM_D);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = acc[i][j] + kf * acc2[i][j];
  out_tile_store_padded(acc, tp, B, I, d_out, ldd);
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

// Both rows exports: the checks and the launch of (a).  plain as the kernel takes it (2: chaorec_diffmm_rows_noised_f32).
static int dm_rows_launch(const char *name, const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col, int64_t I,
                          int64_t ld, const float *a_row, const float *s_row, const float *noise, const uint8_t *keep, uint64_t seed,
                          uint64_t step, uint32_t salt, int plain, float *x, uint32_t *bits, void *stream) {
  if (!users || !rowptr || !col || !x || !bits) return fail(CHAOREC_E_INVALID, "%s: NULL argument", name);
  if (plain != 1 && (!a_row || !s_row)) return fail(CHAOREC_E_INVALID, "%s: a_row / s_row missing", name);
  if (B < 0 || U < 0 || I <= 0 || I > ((int64_t)1 << 31) - 256) return fail(CHAOREC_E_INVALID, "%s: B=%lld I=%lld", name, (long long)B, (long long)I);
  if (ld != (I + 3) / 4 * 4 || !aligned16(x))
    return fail(CHAOREC_E_INVALID, "%s: ld=%lld must be I rounded up to 4, the rows 16-byte aligned", name, (long long)ld);
  if (B == 0) return CHAOREC_OK;
  hipLaunchKernelGGL(dm_rows_kernel<>, dim3((unsigned)((B + DM_ROWS - 1) / DM_ROWS)), dim3(64 * DM_ROWS), 0, (hipStream_t)stream, users,
                     B, U, rowptr, col, I, ld, a_row, s_row, noise, keep, seed, step, (uint64_t)salt, plain, x, bits, (I + 31) / 32);
  return check_launch("dm_rows_kernel");
}

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
  *bm = OT_BM;
  *bn = OT_BN;
  *bk = OT_BK;
  return CHAOREC_OK;
}

extern "C" int64_t chaorec_diffmm_rows_per_block(void) { return DM_ROWS; }

extern "C" int chaorec_diffmm_rows_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                       int64_t I, int64_t ld, const float *a_row, const float *s_row, const float *noise,
                                       const uint8_t *keep, uint64_t seed, uint64_t step, uint32_t salt, int32_t plain,
                                       float *x_in, uint32_t *bits, void *stream) {
  return dm_rows_launch("diffmm_rows", users, B, U, rowptr, col, I, ld, a_row, s_row, noise, keep, seed, step, salt, plain ? 1 : 0, x_in, bits, stream);
}

extern "C" int chaorec_diffmm_rows_noised_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                              int64_t I, int64_t ld, const float *a_row, const float *s_row, const float *noise,
                                              uint64_t seed, uint64_t step, uint32_t salt, float *x_t, uint32_t *bits, void *stream) {
  return dm_rows_launch("diffmm_rows_noised", users, B, U, rowptr, col, I, ld, a_row, s_row, noise, nullptr, seed, step, salt, 2, x_t, bits, stream);
}

extern "C" int chaorec_diffmm_out_loss_f32(const float *h, int64_t ldh, const float *W_out, int64_t ldw, const float *b_out,
                                           const uint32_t *bits, const float *r, const float *F, const double *w,
                                           const float *c_row, float kf, float e_loss, int64_t B, int64_t I, int64_t H,
                                           float *d_out, int64_t ldd, float *part, double *diff_rows, float *gc_rows,
                                           float *loss, void *stream) {
  if (!h || !W_out || !b_out || !bits || !r || !F || !w || !c_row || !d_out || !part || !diff_rows || !gc_rows || !loss)
    return fail(CHAOREC_E_INVALID, "diffmm_out_loss: NULL argument");
  if (int rc = chaorec_diffmm_check_shape(B, I, H, DM_D)) return rc;
  if (ldh < H || ldw < H || (ldh & 3) || (ldw & 3) || ldd < I || !aligned16(h) || !aligned16(W_out) || !aligned16(r) || !aligned16(F))
    return fail(CHAOREC_E_INVALID, "diffmm_out_loss: h, W_out, r, F must be 16-byte aligned with row strides that are multiples of 4");
  const OutGrid g = out_tile_grid(B, I);
  if (ldd > g.NT * OT_BN) return fail(CHAOREC_E_INVALID, "diffmm_out_loss: ldd=%lld past the last item tile", (long long)ldd);
  if (!g.blocks) return fail(CHAOREC_E_INVALID, "diffmm_out_loss: too many workgroups at B=%lld I=%lld", (long long)B, (long long)I);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dm_out_loss_kernel<>, dim3((unsigned)g.blocks), dim3(256), 0, st, h, ldh, W_out, ldw, b_out, bits, (I + 31) / 32, r, F,
                     c_row, kf, B, I, H, g.MT, g.NT, d_out, ldd, part);
  if (int rc = check_launch("dm_out_loss_kernel")) return rc;
  hipLaunchKernelGGL(dm_reduce_kernel<>, dim3(1), dim3(256), 0, st, part, g.NT, r, w, B, I, e_loss, diff_rows, gc_rows, loss);
  return check_launch("dm_reduce_kernel");
}
