// LightGODE (Model/LightGODE.py:97-146): the alignment + uniformity loss of a batch of B (user, item) pairs and the gradient by
// the gathered rows, with no [B, B] and no [B (B - 1) / 2] buffer.  gfx950, D = 64, fp32.
//
// Per side (users, items), with z_b = e_b / max(|e_b|, 1e-12) the normalised gathered rows, n_b = <z_b, z_b> and
//     e_ij = exp(-2 max(n_i + n_j - 2 <z_i, z_j>, 0))   (i != j; evaluated on rows shifted by a common vector, lg_center)
//     r_i = sum_{j != i} e_ij,   S = 1/2 sum_i r_i,   P = B (B - 1) / 2:
//     unif  = log(S / P)                                              (= pdist(z).pow(2).mul(-2).exp().mean().log())
//     d unif / d z_i = (-4 / S) (r_i z_i - sum_{j != i} e_ij z_j)
//     align = mean_b |x_b - y_b|^2,   d align / d x_b = 2 (x_b - y_b) / B = -d align / d y_b
//     loss  = align + gamma (unif_u + unif_i) / 2
//     d loss / d e_b = (g - z_b <z_b, g>) / max(|e_b|, 1e-12),  g = d loss / d z_b       (F.normalize's backward)
// Four launches:
//   lg_rows:   a wave per sample gathers and normalises its two rows (z, the clamped norm) and sums |x_b - y_b|^2; one more
//              block forms c, a mean of 64 normalised rows of each side, once.
//   lg_center: zc = z - c and n = <zc, zc>; the pair launch works on zc (see the kernel).
//   lg_pairs:  grid (32-row blocks, column splits, side).  A workgroup owns 32 rows i; per step its four waves take 32 columns j
//              each of a 128-column tile staged in LDS.  Scores TRANSPOSED on v_mfma_f32_32x32x2_f32 (A operand = the column
//              tile, B operand = the wave's own rows, exact fp32 products), so a lane's 16 accumulator values all belong to ITS
//              row i: e_ij in place, r_i a running sum, and sum_j e_ij z_j a second product that takes e straight from the
//              accumulator as its B operand and z_j from the same LDS tile.  The four waves' sums are added in wave order, the
//              result is the (split, row) partial.  The symmetry e_ij = e_ji is NOT used: every row has one owner.
//   lg_finish: every workgroup adds the r partials in (row, split) order into S (double, one fixed tree: the same bits in every
//              workgroup), workgroup 0 writes the loss and its parts, and a wave per sample adds its G partials in split order
//              and writes both sides' gradient rows.
// The grid of lg_pairs: 2 ceil(B / 32) row blocks over both sides times as many column splits as bring it to the chip's 256
// CUs (B = 1024: 2 x 32 x 4 = 256 workgroups of two steps each) -- at this size the launch is latency, not throughput.
// The backward adds go * row_grad into the zero-filled table gradients: one owner wave per table row (the first sample with
// that id), repeated ids added in batch order; no float atomics anywhere, the same bits every run.
#include "vae_common.h"

namespace chaorec {

constexpr int LG_D = 64;
constexpr int LG_RB = 32;              // rows per workgroup of lg_pairs (every wave holds all of them)
constexpr int LG_TC = 128;             // columns per step: 4 waves x 32
constexpr int LG_MAX_B = 8192;         // the backward keeps the batch's ids in LDS
constexpr int LG_SCATTER_WAVES = 16;
static_assert(LG_D == VAE_D && LG_TC == VAE_TI, "the staging helper moves 128 rows of the latent width");

// workspace, in floats (every block a multiple of 4 floats from a 16-byte aligned base)
struct LgWs {
  int64_t z, zc, gp, rp, nrm, n2, al, c, total;
  int64_t splits, tiles_per_split;
};
inline LgWs lg_plan(int64_t B) {
  LgWs w;
  const int64_t row_blocks = (B + LG_RB - 1) / LG_RB, tiles = (B + LG_TC - 1) / LG_TC, Bp = (B + 3) / 4 * 4;
  int64_t want = (256 + 2 * row_blocks - 1) / (2 * row_blocks);
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  w.tiles_per_split = (tiles + want - 1) / want;
  w.splits = (tiles + w.tiles_per_split - 1) / w.tiles_per_split;
  w.z = 0;
  w.zc = w.z + 2 * B * LG_D;
  w.gp = w.zc + 2 * B * LG_D;
  w.rp = w.gp + 2 * w.splits * B * LG_D;
  w.nrm = w.rp + 2 * w.splits * Bp;
  w.n2 = w.nrm + 2 * Bp;
  w.al = w.n2 + 2 * Bp;
  w.c = w.al + Bp;
  w.total = w.c + 2 * LG_D;
  return w;
}

constexpr int LG_CS = 64;               // rows behind the common shift c of a side

// lane's element of the normalised table row, and the clamped norm (F.normalize: e / max(|e|, 1e-12))
__device__ __forceinline__ float lg_unit_row(const float *__restrict__ tab, int64_t row, int lane, float &nrm) {
  const float e = tab[row * LG_D + lane];
  nrm = fmaxf(sqrtf(wave_sum(e * e)), 1e-12f);
  return e / nrm;
}

// blocks 0 .. ceil(B / 4) - 1: a wave per sample.  The ONE block after them forms c, the mean of LG_CS normalised rows of each side
// (samples k B / LG_CS; every sample where B < LG_CS), once: wave w adds its quarter of them in ascending order, the four sums
// are added in wave order.
__global__ __launch_bounds__(256) void lg_rows_kernel(const float *__restrict__ tab_u, const float *__restrict__ tab_i, int64_t U,
                                                      int64_t I, const int64_t *__restrict__ users, const int64_t *__restrict__ items,
                                                      int64_t B, float *__restrict__ ws, LgWs w) {
  __shared__ float cpart[2][4][LG_D];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t Bp = (B + 3) / 4 * 4;
  if ((int64_t)blockIdx.x * 4 >= B) {           // (block-uniform)
    const int cs = B < LG_CS ? (int)B : LG_CS;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      float c = 0.f;
      for (int k = wave * (LG_CS / 4); k < (wave + 1) * (LG_CS / 4) && k < cs; ++k) {
        const int64_t bs = (int64_t)k * B / cs;
        float nrm;
        c += lg_unit_row(side ? tab_i : tab_u, side ? clamp_index(items[bs], I) : clamp_index(users[bs], U), lane, nrm);
      }
      cpart[side][wave][lane] = c;
    }
    __syncthreads();
    if (threadIdx.x < 2 * LG_D) {
      const int side = wave;
      ws[w.c + side * LG_D + lane] = (((cpart[side][0][lane] + cpart[side][1][lane]) + cpart[side][2][lane]) + cpart[side][3][lane]) / (float)cs;
    }
    return;
  }
  const int64_t b = (int64_t)blockIdx.x * 4 + wave;
  if (b >= B) return;
  float zz[2];
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    float nrm;
    const float z = lg_unit_row(side ? tab_i : tab_u, side ? clamp_index(items[b], I) : clamp_index(users[b], U), lane, nrm);
    zz[side] = z;
    ws[w.z + ((int64_t)side * B + b) * LG_D + lane] = z;
    if (lane == 0) ws[w.nrm + side * Bp + b] = nrm;
  }
  const float d = zz[0] - zz[1];
  const float a = wave_sum(d * d);
  if (lane == 0) ws[w.al + b] = a;
}

// zc_b = z_b - c with c the common shift lg_rows left, and n_b = <zc_b, zc_b>.  Distances do not see the shift, and
// r_i z_i - sum_j e_ij z_j = r_i zc_i - sum_j e_ij zc_j: what cancels in both is then of the size of the batch's spread, not of
// the size 1 of a normalised row -- a batch of one id (zc = rounding noise) leaves a gradient of 0 up to that noise, where the
// uncentred form left 1e-7 of |z| in every row, all of one sign.  n as lg_pairs' MFMA forms <zc_i, zc_j>: ONE fmaf chain, k
// ascending; two samples of one id then sit at n_i + n_j - 2 <zc_i, zc_j> = 0 exactly, e = 1 exactly, as torch's pdist has them.
__global__ __launch_bounds__(256) void lg_center_kernel(int64_t B, float *__restrict__ ws, LgWs w) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t Bp = (B + 3) / 4 * 4;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const float zc = ws[w.z + ((int64_t)side * B + b) * LG_D + lane] - ws[w.c + side * LG_D + lane];
    ws[w.zc + ((int64_t)side * B + b) * LG_D + lane] = zc;
    float n2 = 0.f;
#pragma unroll
    for (int k = 0; k < LG_D; ++k) {
      const float zk = __shfl(zc, k, 64);
      n2 = fmaf(zk, zk, n2);
    }
    if (lane == 0) ws[w.n2 + side * Bp + b] = n2;
  }
}

__global__ __launch_bounds__(256) void lg_pairs_kernel(int64_t B, float *__restrict__ ws, LgWs w) {
  __shared__ float Ts[LG_D][LG_TC + 1];       // [k][column j]
  __shared__ float ns[LG_TC];                 // n_j
  __shared__ float Gs[LG_RB][LG_D + 1];       // [row i][d]: the four waves' sums
  __shared__ float rs[4][LG_RB];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 31, h = lane >> 5;
  const int side = blockIdx.z, split = blockIdx.y;
  const int64_t Bp = (B + 3) / 4 * 4;
  const float *__restrict__ Z = ws + w.zc + (int64_t)side * B * LG_D;
  const float *__restrict__ N2 = ws + w.n2 + side * Bp;
  const int64_t i = (int64_t)blockIdx.x * LG_RB + r;
  const bool live = i < B;
  const int64_t tiles = (B + LG_TC - 1) / LG_TC;
  const int64_t t_beg = (int64_t)split * w.tiles_per_split, t_end = min(tiles, t_beg + w.tiles_per_split);

  float bf[LG_D / 2];
#pragma unroll
  for (int s = 0; s < LG_D / 2; ++s) bf[s] = live ? Z[i * LG_D + 2 * s + h] : 0.f;
  const float ni = live ? N2[i] : 0.f;
  float rsum = 0.f;
  f32x16 dg[2] = {vae_zero(), vae_zero()};

  for (int64_t tile = t_beg; tile < t_end; ++tile) {
    const int64_t j0 = tile * LG_TC;
    __syncthreads();
    vae_stage_transposed<LG_TC>(Ts, Z, j0, B, t);
    if (t < LG_TC) ns[t] = (j0 + t < B) ? N2[j0 + t] : 0.f;
    __syncthreads();
    if (j0 + 32 * wave >= B) continue;        // (wave-uniform: none of this wave's columns exists; the barriers are above)
    f32x16 acc = vae_zero();
#pragma unroll
    for (int s = 0; s < LG_D / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ts[2 * s + h][32 * wave + r], bf[s], acc, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = 32 * wave + vae_row(q, h);
      const int64_t j = j0 + c;
      const float d2 = fmaxf((ni + ns[c]) - 2.0f * acc[q], 0.f);
      const float e = (j < B && j != i) ? expf(-2.0f * d2) : 0.f;
      acc[q] = e;
      rsum += e;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = 32 * wave + vae_row(q, h);
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) dg[jj] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ts[32 * jj + r][c], acc[q], dg[jj], 0, 0, 0);
    }
  }
  // the two half-waves saw different columns of the same row; then the waves, in wave order
  const float r2 = rsum + __shfl_xor(rsum, 32, 64);
  if (h == 0) rs[wave][r] = r2;
  for (int wv = 0; wv < 4; ++wv) {
    __syncthreads();
    if (wave == wv) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          float *dst = &Gs[r][32 * jj + vae_row(q, h)];     // dg: row = d, column = the lane's own row i
          *dst = (wv ? *dst : 0.f) + dg[jj][q];
        }
    }
  }
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * LG_RB;
  float *__restrict__ gp = ws + w.gp + (((int64_t)side * w.splits + split) * B + i0) * LG_D;
  for (int v = t; v < LG_RB * LG_D; v += 256) {
    const int row = v >> 6, d = v & 63;
    if (i0 + row < B) gp[(int64_t)row * LG_D + d] = Gs[row][d];
  }
  if (t < LG_RB && i0 + t < B)
    ws[w.rp + ((int64_t)side * w.splits + split) * Bp + i0 + t] = ((rs[0][t] + rs[1][t]) + rs[2][t]) + rs[3][t];
}

// out = (loss, align, unif_u, unif_i); loss0 the 0-dim loss; row_grad [2, B, 64] or NULL
__global__ __launch_bounds__(256) void lg_finish_kernel(int64_t B, float gamma, const float *__restrict__ ws, LgWs w,
                                                        float *__restrict__ out, float *__restrict__ loss0,
                                                        float *__restrict__ row_grad) {
  __shared__ double red[256];
  __shared__ double tot[3];
  const int t = threadIdx.x, lane = t & 63;
  const int64_t Bp = (B + 3) / 4 * 4;
  const int splits = (int)w.splits;
  for (int what = 0; what < 3; ++what) {        // 0, 1: sum_i r_i of the side; 2: sum_b |x_b - y_b|^2
    double v = 0.0;
    for (int64_t b = t; b < B; b += 256) {
      if (what == 2) {
        v += (double)ws[w.al + b];
      } else {
        float ri = 0.f;
        for (int sp = 0; sp < splits; ++sp) ri += ws[w.rp + ((int64_t)what * splits + sp) * Bp + b];
        v += (double)ri;
      }
    }
    block_sum_f64(v, red);
    if (t == 0) tot[what] = red[0];
    __syncthreads();
  }
  const double P = 0.5 * (double)B * (double)(B - 1);
  const double S[2] = {0.5 * tot[0], 0.5 * tot[1]};
  if (blockIdx.x == 0 && t == 0) {
    const double align = tot[2] / (double)B, uu = log(S[0] / P), ui = log(S[1] / P);
    const float l = (float)(align + (double)gamma * (uu + ui) * 0.5);
    out[0] = l;
    out[1] = (float)align;
    out[2] = (float)uu;
    out[3] = (float)ui;
    loss0[0] = l;
  }
  if (!row_grad) return;
  const int64_t b = (int64_t)blockIdx.x * 4 + (t >> 6);
  if (b >= B) return;
  const float x = ws[w.z + b * LG_D + lane], y = ws[w.z + (B + b) * LG_D + lane];
  const float da = 2.0f * (x - y) / (float)B;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const float z = side ? y : x, zc = ws[w.zc + ((int64_t)side * B + b) * LG_D + lane];
    float ri = 0.f, G = 0.f;
    for (int sp = 0; sp < splits; ++sp) {
      ri += ws[w.rp + ((int64_t)side * splits + sp) * Bp + b];
      G += ws[w.gp + (((int64_t)side * splits + sp) * B + b) * LG_D + lane];
    }
    const float cu = (float)((double)gamma * 0.5 * (-4.0 / S[side]));
    const float g = cu * (ri * zc - G) + (side ? -da : da);
    const float zg = wave_sum(z * g);
    row_grad[((int64_t)side * B + b) * LG_D + lane] = (g - z * zg) / ws[w.nrm + side * Bp + b];
  }
}

// g[ids[b]] += go row_grad[side][b]: the first sample of an id owns the table row and adds every sample of that id in batch order
__global__ __launch_bounds__(64 * LG_SCATTER_WAVES) void lg_scatter_kernel(const float *__restrict__ row_grad,
                                                                           const int64_t *__restrict__ users,
                                                                           const int64_t *__restrict__ items, int B, int64_t U, int64_t I,
                                                                           const float *__restrict__ grad_out, float *__restrict__ g_u,
                                                                           float *__restrict__ g_i) {
  __shared__ int32_t keys[LG_MAX_B];
  const int side = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t *__restrict__ ids = side ? items : users;
  const int64_t rows = side ? I : U;
  for (int j = threadIdx.x; j < B; j += blockDim.x) keys[j] = (int32_t)clamp_index(ids[j], rows);
  __syncthreads();
  const int me = (int)blockIdx.x * LG_SCATTER_WAVES + (threadIdx.x >> 6);
  if (me >= B) return;
  const int32_t key = keys[me];
  for (int base = 0; base < me; base += 64) {
    const int j = base + lane;
    if (__any(j < me && keys[j] == key)) return;
  }
  const float go = grad_out ? grad_out[0] : 1.0f;
  float *dst = (side ? g_i : g_u) + (int64_t)key * LG_D + lane;
  const float *__restrict__ src = row_grad + (int64_t)side * B * LG_D + lane;
  float acc = *dst;
  for (int base = me & ~63; base < B; base += 64) {
    const int j = base + lane;
    unsigned long long m = __ballot(j >= me && j < B && keys[j] == key);
    while (m) {                                 // wave-uniform, ascending sample number
      const int jj = base + (int)__builtin_ctzll(m);
      m &= m - 1;
      acc += mul_rn(go, src[(int64_t)jj * LG_D]);
    }
  }
  *dst = acc;
}

static int lg_check_shape(const char *who, int64_t B, int32_t D) {
  if (D != LG_D) return fail(CHAOREC_E_INVALID, "%s: D=%d, the kernels tile D=%d", who, (int)D, LG_D);
  if (B < 2) return fail(CHAOREC_E_INVALID, "%s: B=%lld, the uniformity term is a mean over B (B - 1) / 2 pairs", who, (long long)B);
  if (B > LG_MAX_B) return fail(CHAOREC_E_INVALID, "%s: B=%lld, at most %d samples", who, (long long)B, LG_MAX_B);
  return CHAOREC_OK;
}

}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_lightgode_check_shape(int64_t B, int32_t D) { return lg_check_shape("lightgode_check_shape", B, D); }

extern "C" int chaorec_lightgode_workspace(int64_t B, int32_t D, int64_t *n_floats) {
  if (!n_floats) return fail(CHAOREC_E_INVALID, "lightgode_workspace: NULL argument");
  if (int rc = lg_check_shape("lightgode_workspace", B, D)) return rc;
  *n_floats = lg_plan(B).total;
  return CHAOREC_OK;
}

extern "C" int chaorec_lightgode_loss_f32(const float *tab_u, const float *tab_i, int64_t U, int64_t I, const int64_t *users,
                                          const int64_t *items, int64_t B, int32_t D, float gamma, float *workspace,
                                          int64_t ws_floats, float *out, float *loss, float *row_grad, void *stream) {
  if (!tab_u || !tab_i || !users || !items || !workspace || !out || !loss) return fail(CHAOREC_E_INVALID, "lightgode_loss: NULL argument");
  if (int rc = lg_check_shape("lightgode_loss", B, D)) return rc;
  if (U <= 0 || I <= 0 || U >= ((int64_t)1 << 31) || I >= ((int64_t)1 << 31))
    return fail(CHAOREC_E_INVALID, "lightgode_loss: U=%lld I=%lld", (long long)U, (long long)I);
  const LgWs w = lg_plan(B);
  if (ws_floats < w.total)
    return fail(CHAOREC_E_WORKSPACE, "lightgode_loss: workspace of %lld floats, chaorec_lightgode_workspace says %lld",
                (long long)ws_floats, (long long)w.total);
  if (!aligned16(workspace)) return fail(CHAOREC_E_INVALID, "lightgode_loss: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const unsigned sample_blocks = (unsigned)((B + 3) / 4);
  hipLaunchKernelGGL(lg_rows_kernel, dim3(sample_blocks + 1), dim3(256), 0, st, tab_u, tab_i, U, I, users, items, B, workspace, w);
  hipLaunchKernelGGL(lg_center_kernel, dim3(sample_blocks), dim3(256), 0, st, B, workspace, w);
  hipLaunchKernelGGL(lg_pairs_kernel, dim3((unsigned)((B + LG_RB - 1) / LG_RB), (unsigned)w.splits, 2), dim3(256), 0, st, B, workspace, w);
  hipLaunchKernelGGL(lg_finish_kernel, dim3(sample_blocks), dim3(256), 0, st, B, gamma, (const float *)workspace, w, out, loss, row_grad);
  return check_launch("lightgode_loss");
}

extern "C" int chaorec_lightgode_bwd_f32(const float *row_grad, const int64_t *users, const int64_t *items, int64_t B, int32_t D,
                                         int64_t U, int64_t I, const float *grad_out, float *g_u, float *g_i, void *stream) {
  if (!row_grad || !users || !items || !g_u || !g_i) return fail(CHAOREC_E_INVALID, "lightgode_bwd: NULL argument");
  if (int rc = lg_check_shape("lightgode_bwd", B, D)) return rc;
  if (U <= 0 || I <= 0 || U >= ((int64_t)1 << 31) || I >= ((int64_t)1 << 31))
    return fail(CHAOREC_E_INVALID, "lightgode_bwd: U=%lld I=%lld", (long long)U, (long long)I);
  const dim3 grid((unsigned)((B + LG_SCATTER_WAVES - 1) / LG_SCATTER_WAVES), 2);
  hipLaunchKernelGGL(lg_scatter_kernel, grid, dim3(64 * LG_SCATTER_WAVES), 0, (hipStream_t)stream, row_grad, users, items, (int)B, U, I,
                     grad_out, g_u, g_i);
  return check_launch("lightgode_bwd");
}
