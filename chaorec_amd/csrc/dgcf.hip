// DGCF (Model/DGCF.py): intent-weighted propagation, the routing update of the intent scores, and the distance
// correlation of consecutive intent slices (utils.py:83-108).
//
// Graph: the LightGCN-normalised CSR (rows = destinations, entries in the reference's edge order) plus eid[entry] = the
// undirected edge the entry belongs to.  Intent state P / S is ENTRY-MAJOR [E, K]: one entry reads its K weights from one
// 4K-byte run.  Lane layout of the row kernels: a row is D/4 lanes (one float4 each), so slice k of the row is the lanes
// [k * D/(4K), (k+1) * D/(4K)) -- `D % (4K) == 0` keeps a slice on whole lanes.  No float atomics anywhere: every output row
// has one writer, every S[e] / P[e] has one writer (the user-row entry of edge e), and the dCor sums are combined in a fixed
// order.
#include <algorithm>
#include <math.h>

#include "common.h"

using namespace chaorec;

namespace {

// sum over the LPS lanes of one slice (aligned groups of LPS lanes: xor offsets below LPS never leave the group).
// NOT common.h's group_sum: this butterfly ASCENDS (off = 1 first), another summation order and therefore other bits.
template <int LPS>
__device__ __forceinline__ float slice_sum(float v) {
#pragma unroll
  for (int off = 1; off < LPS; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// F.normalize(x, dim=1) of one slice (eps 1e-12): x / max(|x|, eps)
template <int LPS>
__device__ __forceinline__ float4 slice_normalize(float4 v) {
  const float n = fmaxf(sqrtf(slice_sum<LPS>(dot4(v, v))), 1e-12f);
  return make_float4(v.x / n, v.y / n, v.z / n, v.w / n);
}

// One launch of a (layer, iteration) pair, rows [row_begin, row_end):
//   acc[r] = sum_e (norm_e * P[eid_e, k(lane)]) * x[col_e]           (DGCFConv.message + scatter add, Model/DGCF.py:27-46)
//   y[r] = acc (if y);  zout[r] = z[r] + acc (if zout: the layer sum of the forward, the + G of the backward)
// ROUTE, rows r < route_end (user rows): the routing update of every entry of the row (Model/DGCF.py:124-140)
//   score_k = < normalize(acc_k), tanh(normalize(x_k[col_e])) >,   S[eid_e, k] = P[eid_e, k] + score_k,
//   P_next[eid_e, :] = softmax_k(S[eid_e, :])          (the next iteration's `self.S = softmax(self.S)`, kept beside S)
// P and P_next are different buffers: rows that only propagate read P while user rows write P_next in the same launch.
template <int LPR, int K, bool ROUTE>
__global__ __launch_bounds__(256) void dgcf_rows_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                        const float *__restrict__ norm, const int32_t *__restrict__ eid,
                                                        const float *__restrict__ P, const float4 *__restrict__ x,
                                                        float4 *__restrict__ y, const float4 *z, float4 *zout,
                                                        int64_t row_begin, int64_t row_end, int64_t route_end,
                                                        float *__restrict__ S, float *__restrict__ P_next) {
  constexpr int LPS = LPR / K;          // lanes per intent slice
  constexpr int RPW = 64 / LPR;         // rows per wave
  const int lane = threadIdx.x & 63, sub = lane % LPR, k = sub / LPS;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r0 = row_begin + wave * RPW; r0 < row_end; r0 += n_waves * RPW) {
    const int64_t r = r0 + lane / LPR;
    const bool live = r < row_end;
    const int64_t e0 = live ? rowptr[r] : 0, e1 = live ? rowptr[r + 1] : 0;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t e = e0; e < e1; ++e) {
      const float w = mul_rn(norm[e], P[(int64_t)eid[e] * K + k]);
      acc = add_rn4(acc, mul_rn4(w, x[(int64_t)col[e] * LPR + sub]));
    }
    if (live) {
      if (y) y[r * LPR + sub] = acc;
      if (zout) zout[r * LPR + sub] = add_rn4(z[r * LPR + sub], acc);
    }
    if constexpr (ROUTE) {
      // route_end is a multiple of nothing in particular: rows of one wave may straddle it, so the test is per row, and
      // the shuffles below run on every lane of the wave (a group that does not route contributes nothing)
      const bool route = live && r < route_end;
      const int64_t n_e = route ? e1 - e0 : 0;
      int64_t n_max = n_e;
#pragma unroll
      for (int off = LPR; off < 64; off <<= 1) {
        const int64_t o = __shfl_xor(n_max, off, 64);
        n_max = o > n_max ? o : n_max;
      }
      const float4 un = slice_normalize<LPS>(acc);
      for (int64_t q = 0; q < n_max; ++q) {
        const bool has = q < n_e;
        const int64_t e = e0 + (has ? q : 0);
        const int32_t ed = has ? eid[e] : 0;
        const float4 xi = has ? x[(int64_t)col[e] * LPR + sub] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 in = slice_normalize<LPS>(xi);
        const float4 t = make_float4(tanhf(in.x), tanhf(in.y), tanhf(in.z), tanhf(in.w));
        const float score = slice_sum<LPS>(dot4(un, t));
        const float s_new = (has ? P[(int64_t)ed * K + k] : 0.f) + score;
        // the K new scores of this entry, from the first lane of every slice of the row's lane group
        const int base = lane - sub;
        float s[K];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          s[j] = __shfl(s_new, base + j * LPS, 64);
          m = fmaxf(m, s[j]);
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) sum += expf(s[j] - m);
        if (has && sub < K) {
          float mine = s[0];
#pragma unroll
          for (int j = 1; j < K; ++j) mine = (sub == j) ? s[j] : mine;
          S[(int64_t)ed * K + sub] = mine;
          P_next[(int64_t)ed * K + sub] = expf(mine - m) / sum;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void dgcf_softmax_kernel(const float *__restrict__ S, float *__restrict__ P, int64_t E,
                                                           int K) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    float m = -INFINITY, sum = 0.f;
    for (int j = 0; j < K; ++j) m = fmaxf(m, S[e * K + j]);
    for (int j = 0; j < K; ++j) sum += expf(S[e * K + j] - m);
    for (int j = 0; j < K; ++j) P[e * K + j] = expf(S[e * K + j] - m) / sum;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Distance correlation.  Per slice k of the gathered rows X [n, D]: a_k(i,j) = sqrt(max(r_i - 2 <x_i,x_j> + r_j, 0) + 1e-8)
// (utils.py:87-90), r = row sums of squares.  Double centering is linear and self-adjoint, so with R_k[i] = sum_j a_k(i,j):
//   sum A_k o A_l = sum a_k a_l - (2/n) sum_i R_k[i] R_l[i] + (sum R_k)(sum R_l) / n^2
// and d(sum A o B)/d a = B (centred).  Nothing n x n is stored: pass 1 walks the pairs once for every slice's row sums and
// pair sums, pass 2 walks them again for the row gradients.
constexpr int DC_T = 16;              // 16 x 16 pairs per tile; a workgroup owns 16 rows and walks every column tile

__global__ __launch_bounds__(256) void dcor_gather_kernel(const float *__restrict__ table, const int64_t *__restrict__ idx,
                                                          int64_t n, int D, int K, float *__restrict__ X,
                                                          float *__restrict__ r) {
  const int w = D / K;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * K; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / K;
    const int k = (int)(t % K);
    const float *src = table + idx[i] * D + k * w;
    float *dst = X + i * D + k * w;
    float s = 0.f;
    for (int d = 0; d < w; ++d) {
      const float v = src[d];
      dst[d] = v;
      s = fmaf(v, v, s);
    }
    r[i * K + k] = s;
  }
}

template <int K, int D>
__device__ __forceinline__ void dcor_tile_distances(const float (*xi)[D + 1], const float (*xj)[D + 1], const float *ri,
                                                    const float *rj, int ti, int tj, float *a, bool *pos) {
  constexpr int W = D / K;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float dot = 0.f;
#pragma unroll 8
    for (int d = 0; d < W; ++d) dot = fmaf(xi[ti][k * W + d], xj[tj][k * W + d], dot);
    const float q = ri[ti * K + k] - 2.f * dot + rj[tj * K + k];
    pos[k] = q > 0.f;
    a[k] = sqrtf(fmaxf(q, 0.f) + 1e-8f);
  }
}

template <int K, int D>
__device__ __forceinline__ void dcor_load_tile(const float *X, const float *r, int64_t n, int64_t j0, float (*xs)[D + 1],
                                               float *rs) {
  for (int t = threadIdx.x; t < DC_T * D; t += 256) {
    const int jj = t / D, d = t % D;
    xs[jj][d] = (j0 + jj < n) ? X[(j0 + jj) * D + d] : 0.f;
  }
  for (int t = threadIdx.x; t < DC_T * K; t += 256) rs[t] = (j0 + t / K < n) ? r[j0 * K + t] : 0.f;
}

// pass 1: R[k][i] (double), and per workgroup the partial sums  sum a_k a_{k+1}  (k < K-1) and  sum a_k^2
template <int K, int D>
__global__ __launch_bounds__(256) void dcor_pass1_kernel(const float *__restrict__ X, const float *__restrict__ r, int64_t n,
                                                         double *__restrict__ R, double *__restrict__ part) {
  __shared__ float xi[DC_T][D + 1], xj[DC_T][D + 1];
  __shared__ float ri[DC_T * K], rj[DC_T * K];
  __shared__ double red[256];
  const int ti = threadIdx.x / DC_T, tj = threadIdx.x % DC_T;
  const int64_t i0 = (int64_t)blockIdx.x * DC_T, i = i0 + ti;
  dcor_load_tile<K, D>(X, r, n, i0, xi, ri);
  double rs[K], ps[K], qs[K];
#pragma unroll
  for (int k = 0; k < K; ++k) rs[k] = ps[k] = qs[k] = 0.0;
  for (int64_t j0 = 0; j0 < n; j0 += DC_T) {
    __syncthreads();
    dcor_load_tile<K, D>(X, r, n, j0, xj, rj);
    __syncthreads();
    if (i < n && j0 + tj < n) {
      float a[K];
      bool pos[K];
      dcor_tile_distances<K, D>(xi, xj, ri, rj, ti, tj, a, pos);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        rs[k] += a[k];
        qs[k] += (double)a[k] * a[k];
        if (k + 1 < K) ps[k] += (double)a[k] * a[k + 1];
      }
    }
  }
  // row sums: the 16 column lanes of a row, in order
  for (int k = 0; k < K; ++k) {
    __syncthreads();
    red[threadIdx.x] = rs[k];
    __syncthreads();
    if (tj == 0 && i < n) {
      double s = 0.0;
      for (int c = 0; c < DC_T; ++c) s += red[ti * DC_T + c];
      R[k * n + i] = s;
    }
  }
  // workgroup partials: a fixed tree over the 256 threads
  for (int q = 0; q < 2 * K; ++q) {
    __syncthreads();
    block_sum_f64(q < K ? ps[q] : qs[q - K], red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * 2 * K + q] = red[0];
  }
}

// combine (one workgroup, fixed order): the loss and the coefficients of pass 2.
// stats: [0] cor (already / ((K+1) K / 2)); [1 .. K] abar_k = sum R_k / n^2 ; [1+K .. 3K] per slice (cprev, cnext, cself)
// of  G_k = cprev A_{k-1} + cnext A_{k+1} + cself A_k  (d cor / d a_k);  mean [K, n] = R / n.
__global__ __launch_bounds__(256) void dcor_combine_kernel(const double *__restrict__ R, const double *__restrict__ part,
                                                           int n_parts, int64_t n, int K, float *__restrict__ loss,
                                                           float *__restrict__ stats, float *__restrict__ mean) {
  __shared__ double red[256];
  __shared__ double sums[3 * 8 + 2 * 8];          // sumR[k], RR[k] (k,k+1), R2[k], pair sums, square sums
  const double nd = (double)n;
  auto reduce = [&](double v) -> double {
    __syncthreads();      // (the previous total is still being read)
    block_sum_f64(v, red);
    return red[0];
  };
  for (int k = 0; k < K; ++k) {
    double s = 0.0, rr = 0.0, r2 = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
      const double a = R[k * n + i];
      s += a;
      r2 += a * a;
      if (k + 1 < K) rr += a * R[(k + 1) * n + i];
      mean[k * n + i] = (float)(a / nd);
    }
    const double ts = reduce(s), trr = reduce(rr), tr2 = reduce(r2);
    double pp = 0.0, qq = 0.0;
    for (int b = threadIdx.x; b < n_parts; b += 256) {
      pp += part[(int64_t)b * 2 * K + k];
      qq += part[(int64_t)b * 2 * K + K + k];
    }
    const double tpp = reduce(pp), tqq = reduce(qq);
    if (threadIdx.x == 0) {
      sums[k] = ts;
      sums[8 + k] = trr;
      sums[16 + k] = tr2;
      sums[24 + k] = tpp;
      sums[32 + k] = tqq;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n2 = nd * nd;
  const double Z = (double)(K + 1) * K / 2.0;
  double s_self[8], g_self[8] = {0}, g_next[8] = {0};
  for (int k = 0; k < K; ++k) s_self[k] = sums[32 + k] - 2.0 / nd * sums[16 + k] + sums[k] * sums[k] / n2;
  double cor = 0.0;
  for (int k = 0; k + 1 < K; ++k) {
    const double s12 = sums[24 + k] - 2.0 / nd * sums[8 + k] + sums[k] * sums[k + 1] / n2;
    const double s11 = s_self[k], s22 = s_self[k + 1];
    const double c12 = sqrt(fmax(s12 / n2, 0.0) + 1e-8), c11 = sqrt(fmax(s11 / n2, 0.0) + 1e-8),
                 c22 = sqrt(fmax(s22 / n2, 0.0) + 1e-8);
    const double prod = fmax(c11 * c22, 0.0), sp = sqrt(prod), den = sp + 1e-10;
    cor += c12 / den;
    // d dcor / d S_xy = d dcor / d dcov_xy * [S_xy > 0] / (2 dcov_xy n^2)
    const double d12 = 1.0 / den, dsp = -c12 / (den * den);
    const double d11 = prod > 0.0 ? dsp * c22 / (2.0 * sp) : 0.0, d22 = prod > 0.0 ? dsp * c11 / (2.0 * sp) : 0.0;
    const double g12 = s12 > 0.0 ? d12 / (2.0 * c12 * n2) : 0.0;
    const double g11 = s11 > 0.0 ? d11 / (2.0 * c11 * n2) : 0.0;
    const double g22 = s22 > 0.0 ? d22 / (2.0 * c22 * n2) : 0.0;
    g_next[k] = g12 / Z;                     // d S_{k,k+1} / d a_k = A_{k+1};  d / d a_{k+1} = A_k
    g_self[k] += 2.0 * g11 / Z;              // d S_kk / d a_k = 2 A_k
    g_self[k + 1] += 2.0 * g22 / Z;
  }
  loss[0] = (float)(cor / Z);
  for (int k = 0; k < K; ++k) {
    stats[1 + k] = (float)(sums[k] / n2);
    stats[1 + K + 3 * k + 0] = k > 0 ? (float)g_next[k - 1] : 0.f;
    stats[1 + K + 3 * k + 1] = k + 1 < K ? (float)g_next[k] : 0.f;
    stats[1 + K + 3 * k + 2] = (float)g_self[k];
  }
  stats[0] = loss[0];
}

// pass 2: grad_rows[i] = g * sum_j  w_k(i,j) (x_i - x_j) on slice k,  w_k = 2 G_k(i,j) / a_k(i,j) where q_k > 0 (else 0):
// a(i,j) and a(j,i) are the same distance, each contributes G / (2a) * 2 (x_i - x_j).
template <int K, int D>
__global__ __launch_bounds__(256) void dcor_pass2_kernel(const float *__restrict__ X, const float *__restrict__ r, int64_t n,
                                                         const float *__restrict__ stats, const float *__restrict__ mean,
                                                         const float *__restrict__ grad_out, float *__restrict__ grad_rows) {
  constexpr int W = D / K, DPT = D / DC_T;
  __shared__ float xi[DC_T][D + 1], xj[DC_T][D + 1];
  __shared__ float ri[DC_T * K], rj[DC_T * K];
  __shared__ float wt[DC_T][DC_T][K];
  const int ti = threadIdx.x / DC_T, tj = threadIdx.x % DC_T;
  const int64_t i0 = (int64_t)blockIdx.x * DC_T, i = i0 + ti;
  dcor_load_tile<K, D>(X, r, n, i0, xi, ri);
  float abar[K], cp[K], cn[K], cs[K], mi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    abar[k] = stats[1 + k];
    cp[k] = stats[1 + K + 3 * k];
    cn[k] = stats[1 + K + 3 * k + 1];
    cs[k] = stats[1 + K + 3 * k + 2];
    mi[k] = i < n ? mean[k * n + i] : 0.f;
  }
  float acc[DPT];
#pragma unroll
  for (int m = 0; m < DPT; ++m) acc[m] = 0.f;
  for (int64_t j0 = 0; j0 < n; j0 += DC_T) {
    __syncthreads();
    dcor_load_tile<K, D>(X, r, n, j0, xj, rj);
    __syncthreads();
    const int64_t j = j0 + tj;
    float wk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) wk[k] = 0.f;
    if (i < n && j < n) {
      float a[K], A[K];
      bool pos[K];
      dcor_tile_distances<K, D>(xi, xj, ri, rj, ti, tj, a, pos);
#pragma unroll
      for (int k = 0; k < K; ++k) A[k] = a[k] - mi[k] - mean[k * n + j] + abar[k];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float G = cs[k] * A[k];
        if (k > 0) G += cp[k] * A[k - 1];
        if (k + 1 < K) G += cn[k] * A[k + 1];
        wk[k] = pos[k] ? 2.f * G / a[k] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) wt[ti][tj][k] = wk[k];
    __syncthreads();
    // rows ti, dimensions tj, tj + 16, ...: the 16 column partners of this tile in order
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
      const int d = tj + m * DC_T, k = d / W;
      const float xv = xi[ti][d];
      float s = acc[m];
      for (int c = 0; c < DC_T; ++c) s = fmaf(wt[ti][c][k], xv - xj[c][d], s);
      acc[m] = s;
    }
  }
  if (i < n) {
    const float g = grad_out[0];
#pragma unroll
    for (int m = 0; m < DPT; ++m) grad_rows[i * D + tj + m * DC_T] = g * acc[m];
  }
}

// grad_table = 0, by a kernel: a memset node of a captured graph acts on its first replay only, and rows no
// sample of a later batch touches would keep an earlier batch's gradient
__global__ __launch_bounds__(256) void dcor_zero_kernel(float4 *__restrict__ out, int64_t n4) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n4; t += (int64_t)gridDim.x * blockDim.x)
    out[t] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// grad_table[idx[p]] = sum of grad_rows over the gathered rows with that index, in gathered order.  sorted / perm: a
// stable sort of idx.  Each written row has one writer (the first of its run).
__global__ __launch_bounds__(256) void dcor_scatter_kernel(const int64_t *__restrict__ sorted, const int64_t *__restrict__ perm,
                                                           const float *__restrict__ grad_rows, int64_t n, int D,
                                                           float *__restrict__ grad_table) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n * D; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = t / D;
    const int d = (int)(t % D);
    if (p > 0 && sorted[p - 1] == sorted[p]) continue;
    float s = 0.f;
    for (int64_t q = p; q < n && sorted[q] == sorted[p]; ++q) s += grad_rows[perm[q] * D + d];
    grad_table[sorted[p] * D + d] = s;
  }
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

int check_shape(const char *what, int D, int K) {
  if (!pow2(K) || K > 8 || !pow2(D) || D > 256 || D % (4 * K))
    return fail(CHAOREC_E_INVALID, "%s: D=%d K=%d (needs K in {1,2,4,8}, D a power of two <= 256, D %% (4K) == 0)", what, D, K);
  return CHAOREC_OK;
}

template <int LPR, int K>
void launch_rows(bool route, unsigned blocks, hipStream_t st, const int64_t *rowptr, const int32_t *col, const float *norm,
                 const int32_t *eid, const float *P, const float *x, float *y, const float *z, float *zout, int64_t rb,
                 int64_t re, int64_t route_end, float *S, float *P_next) {
  if (route)
    dgcf_rows_kernel<LPR, K, true><<<blocks, 256, 0, st>>>(rowptr, col, norm, eid, P, (const float4 *)x, (float4 *)y,
                                                          (const float4 *)z, (float4 *)zout, rb, re, route_end, S, P_next);
  else
    dgcf_rows_kernel<LPR, K, false><<<blocks, 256, 0, st>>>(rowptr, col, norm, eid, P, (const float4 *)x, (float4 *)y,
                                                           (const float4 *)z, (float4 *)zout, rb, re, route_end, S, P_next);
}

template <int LPR>
int dispatch_k(int K, bool route, unsigned blocks, hipStream_t st, const int64_t *rowptr, const int32_t *col,
               const float *norm, const int32_t *eid, const float *P, const float *x, float *y, const float *z, float *zout,
               int64_t rb, int64_t re, int64_t route_end, float *S, float *P_next) {
  switch (K) {
#define CHAOREC_DGCF_K(KK)                                                                                          \
  case KK:                                                                                                          \
    if constexpr (LPR % KK == 0) {                                                                                  \
      launch_rows<LPR, KK>(route, blocks, st, rowptr, col, norm, eid, P, x, y, z, zout, rb, re, route_end, S, P_next); \
      return CHAOREC_OK;                                                                                            \
    }                                                                                                               \
    break;
    CHAOREC_DGCF_K(1)
    CHAOREC_DGCF_K(2)
    CHAOREC_DGCF_K(4)
    CHAOREC_DGCF_K(8)
#undef CHAOREC_DGCF_K
  }
  return fail(CHAOREC_E_INVALID, "dgcf_propagate: unsupported K=%d for D=%d", K, 4 * LPR);
}

template <int K, int D>
void launch_dcor(int pass, unsigned blocks, hipStream_t st, const float *X, const float *r, int64_t n, double *R,
                 double *part, const float *stats, const float *mean, const float *grad_out, float *grad_rows) {
  if (pass == 1)
    dcor_pass1_kernel<K, D><<<blocks, 256, 0, st>>>(X, r, n, R, part);
  else
    dcor_pass2_kernel<K, D><<<blocks, 256, 0, st>>>(X, r, n, stats, mean, grad_out, grad_rows);
}

template <int K>
int dcor_dispatch_d(int D, int pass, unsigned blocks, hipStream_t st, const float *X, const float *r, int64_t n, double *R,
                    double *part, const float *stats, const float *mean, const float *grad_out, float *grad_rows) {
  switch (D) {
#define CHAOREC_DCOR_D(DD)                                                                                 \
  case DD:                                                                                                 \
    if constexpr (DD % (4 * K) == 0) {                                                                     \
      launch_dcor<K, DD>(pass, blocks, st, X, r, n, R, part, stats, mean, grad_out, grad_rows);            \
      return CHAOREC_OK;                                                                                   \
    }                                                                                                      \
    break;
    CHAOREC_DCOR_D(16)
    CHAOREC_DCOR_D(32)
    CHAOREC_DCOR_D(64)
    CHAOREC_DCOR_D(128)
    CHAOREC_DCOR_D(256)
#undef CHAOREC_DCOR_D
  }
  return fail(CHAOREC_E_INVALID, "dgcf_dcor: unsupported D=%d for K=%d", D, K);
}

int dcor_dispatch(int K, int D, int pass, unsigned blocks, hipStream_t st, const float *X, const float *r, int64_t n,
                  double *R, double *part, const float *stats, const float *mean, const float *grad_out, float *grad_rows) {
  switch (K) {
    case 2: return dcor_dispatch_d<2>(D, pass, blocks, st, X, r, n, R, part, stats, mean, grad_out, grad_rows);
    case 4: return dcor_dispatch_d<4>(D, pass, blocks, st, X, r, n, R, part, stats, mean, grad_out, grad_rows);
    case 8: return dcor_dispatch_d<8>(D, pass, blocks, st, X, r, n, R, part, stats, mean, grad_out, grad_rows);
  }
  return fail(CHAOREC_E_INVALID, "dgcf_dcor: K=%d (2, 4 or 8: one slice has no consecutive pair)", K);
}

// workspace layout (bytes, 256-aligned pieces): X [n, D] f32 | r [n, K] f32 | R [K, n] f64 | part [blocks, 2K] f64 |
// mean [K, n] f32 | stats [1 + 4K] f32
struct DcorWs {
  float *X, *r, *mean, *stats;
  double *R, *part;
};
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
size_t dcor_ws_layout(int64_t n, int D, int K, char *base, DcorWs *ws) {
  const int64_t blocks = (n + DC_T - 1) / DC_T;
  size_t off = 0;
  auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += align256(bytes); return p; };
  char *X = take((size_t)n * D * 4), *r = take((size_t)n * K * 4), *R = take((size_t)K * n * 8),
       *part = take((size_t)blocks * 2 * K * 8), *mean = take((size_t)K * n * 4), *stats = take((size_t)(1 + 4 * K) * 4);
  if (ws) *ws = DcorWs{(float *)X, (float *)r, (float *)mean, (float *)stats, (double *)R, (double *)part};
  return off;
}

}  // namespace

extern "C" int chaorec_dgcf_check_shape(int32_t D, int32_t K) { return check_shape("dgcf", D, K); }

extern "C" int chaorec_dgcf_softmax_f32(const float *S, float *P, int64_t E, int32_t K, void *stream) {
  if (!S || !P || E < 0 || K < 1 || K > 8) return fail(CHAOREC_E_INVALID, "dgcf_softmax: E=%lld K=%d", (long long)E, K);
  if (E == 0) return CHAOREC_OK;
  const unsigned blocks = (unsigned)std::min<int64_t>((E + 255) / 256, 16384);
  dgcf_softmax_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(S, P, E, K);
  return check_launch("dgcf_softmax");
}

extern "C" int chaorec_dgcf_propagate_f32(const int64_t *rowptr, const int32_t *col, const float *norm, const int32_t *eid,
                                          const float *P, const float *x, float *y, const float *z, float *zout,
                                          int64_t row_begin, int64_t row_end, int64_t route_end, int32_t D, int32_t K,
                                          float *S, float *P_next, void *stream) {
  if (int rc = check_shape("dgcf_propagate", D, K)) return rc;
  if (!rowptr || !col || !norm || !eid || !P || !x || (!y && !zout) || (zout && !z))
    return fail(CHAOREC_E_INVALID, "dgcf_propagate: null pointer");
  if (row_begin < 0 || row_end < row_begin || route_end < 0)
    return fail(CHAOREC_E_INVALID, "dgcf_propagate: rows [%lld, %lld) route_end %lld", (long long)row_begin,
                (long long)row_end, (long long)route_end);
  const bool route = route_end > row_begin;
  if (route && (!S || !P_next)) return fail(CHAOREC_E_INVALID, "dgcf_propagate: routing needs S and P_next");
  if (route && (P_next == P)) return fail(CHAOREC_E_INVALID, "dgcf_propagate: P_next must not alias P");
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(z) |
        reinterpret_cast<uintptr_t>(zout)) & 15))
    return fail(CHAOREC_E_INVALID, "dgcf_propagate: x / y / z / zout must be 16-byte aligned");
  if (row_end == row_begin) return CHAOREC_OK;
  const int lpr = D / 4;
  const int64_t waves = (row_end - row_begin + (64 / lpr) - 1) / (64 / lpr);
  const unsigned blocks = (unsigned)std::min<int64_t>((waves + 3) / 4, 65535);
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (lpr) {
    case 4: rc = dispatch_k<4>(K, route, blocks, st, rowptr, col, norm, eid, P, x, y, z, zout, row_begin, row_end, route_end, S, P_next); break;
    case 8: rc = dispatch_k<8>(K, route, blocks, st, rowptr, col, norm, eid, P, x, y, z, zout, row_begin, row_end, route_end, S, P_next); break;
    case 16: rc = dispatch_k<16>(K, route, blocks, st, rowptr, col, norm, eid, P, x, y, z, zout, row_begin, row_end, route_end, S, P_next); break;
    case 32: rc = dispatch_k<32>(K, route, blocks, st, rowptr, col, norm, eid, P, x, y, z, zout, row_begin, row_end, route_end, S, P_next); break;
    case 64: rc = dispatch_k<64>(K, route, blocks, st, rowptr, col, norm, eid, P, x, y, z, zout, row_begin, row_end, route_end, S, P_next); break;
    default: return fail(CHAOREC_E_INVALID, "dgcf_propagate: D=%d", D);
  }
  if (rc) return rc;
  return check_launch("dgcf_propagate");
}

extern "C" size_t chaorec_dgcf_dcor_workspace_bytes(int64_t n, int32_t D, int32_t K) {
  return dcor_ws_layout(n, D, K, nullptr, nullptr);
}

extern "C" int chaorec_dgcf_dcor_fwd_f32(const float *table, const int64_t *idx, int64_t n, int32_t D, int32_t K, float *loss,
                                         void *ws, size_t ws_bytes, void *stream) {
  if (int rc = check_shape("dgcf_dcor_fwd", D, K)) return rc;
  if (K < 2) return fail(CHAOREC_E_INVALID, "dgcf_dcor_fwd: K=%d (at least 2 slices)", K);
  // refused here, before the gather below is launched: pass 2 gives every thread D / 16 columns of its row
  if (D < DC_T) return fail(CHAOREC_E_INVALID, "dgcf_dcor_fwd: unsupported D=%d for K=%d", D, K);
  if (!table || !idx || !loss || !ws || n < 1) return fail(CHAOREC_E_INVALID, "dgcf_dcor_fwd: null pointer or n=%lld", (long long)n);
  if (ws_bytes < dcor_ws_layout(n, D, K, nullptr, nullptr)) return fail(CHAOREC_E_INVALID, "dgcf_dcor_fwd: workspace too small");
  DcorWs w;
  dcor_ws_layout(n, D, K, (char *)ws, &w);
  hipStream_t st = (hipStream_t)stream;
  const unsigned gb = (unsigned)std::min<int64_t>((n * K + 255) / 256, 4096);
  dcor_gather_kernel<<<gb, 256, 0, st>>>(table, idx, n, D, K, w.X, w.r);
  const unsigned blocks = (unsigned)((n + DC_T - 1) / DC_T);
  if (int rc = dcor_dispatch(K, D, 1, blocks, st, w.X, w.r, n, w.R, w.part, nullptr, nullptr, nullptr, nullptr)) return rc;
  dcor_combine_kernel<<<1, 256, 0, st>>>(w.R, w.part, (int)blocks, n, K, loss, w.stats, w.mean);
  return check_launch("dgcf_dcor_fwd");
}

extern "C" int chaorec_dgcf_dcor_bwd_f32(const int64_t *sorted_idx, const int64_t *perm, int64_t n, int32_t D, int32_t K,
                                         const float *grad_out, const void *ws, float *grad_rows, float *grad_table,
                                         int64_t n_table_rows, void *stream) {
  if (int rc = check_shape("dgcf_dcor_bwd", D, K)) return rc;
  if (K < 2) return fail(CHAOREC_E_INVALID, "dgcf_dcor_bwd: K=%d (at least 2 slices)", K);
  if (!sorted_idx || !perm || !grad_out || !ws || !grad_rows || !grad_table || n < 1 || n_table_rows < 1)
    return fail(CHAOREC_E_INVALID, "dgcf_dcor_bwd: null pointer or n=%lld rows=%lld", (long long)n, (long long)n_table_rows);
  if (reinterpret_cast<uintptr_t>(grad_table) & 15) return fail(CHAOREC_E_INVALID, "dgcf_dcor_bwd: grad_table must be 16-byte aligned");
  DcorWs w;
  dcor_ws_layout(n, D, K, (char *)ws, &w);
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((n + DC_T - 1) / DC_T);
  if (int rc = dcor_dispatch(K, D, 2, blocks, st, w.X, w.r, n, nullptr, nullptr, w.stats, w.mean, grad_out, grad_rows))
    return rc;
  const int64_t n4 = n_table_rows * D / 4;
  dcor_zero_kernel<<<(unsigned)std::min<int64_t>((n4 + 255) / 256, 16384), 256, 0, st>>>((float4 *)grad_table, n4);
  const unsigned sb = (unsigned)std::min<int64_t>((n * D + 255) / 256, 16384);
  dcor_scatter_kernel<<<sb, 256, 0, st>>>(sorted_idx, perm, grad_rows, n, D, grad_table);
  return check_launch("dgcf_dcor_bwd");
}
