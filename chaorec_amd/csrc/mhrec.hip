// MHRec (Model/MHRec.py:53-89): the hypergraph attention layer with the epilogue the model applies after it (:724-726),
// forward and backward.  gfx950, fp32 tables, D = 64.
//
// The rebuilt hypergraph has exactly k distinct nodes per hyperedge, every value 1 (train_and_evaluate.py:394-497), so H^T is
// an ELL table nodes int32 [E, k] and H the CSR of the same pairs (rowptr int64 [N + 1], edge int32 [E k]: a node's
// hyperedges ascending).  With a = [a1; a2], E_j = sum_{n in j} X_n, s_n = <X_n, a1>, r_j = <E_j, a2>:
//     w_nj = exp(s_n + r_j)     Z_n = sum_{j of n} w_nj     alpha_nj = w_nj / (Z_n + 1e-16)     out_n = sum_{j of n} alpha_nj E_j
//     y_n = keep ? 2 (out_n + X_n) : 0                                   (dropout 0.5 over the residual sum)
// evaluated with the exponent shifted by the row's maximum M_n = s_n + max_{j of n} r_j, numerator and denominator alike:
//     alpha_nj = exp(r_j - rmax_n) / (Z'_n + eps'_n)     Z'_n = sum_j exp(r_j - rmax_n)     eps'_n = 1e-16 exp(-M_n)
// which is the formula above term for term.  Kept per node for the backward: stat[n] = (-rmax_n, 1 / (Z'_n + eps'_n),
// eps'_n / (Z'_n + eps'_n), s_n); alpha is re-formed from it, never stored per entry.  A node in no hyperedge: out_n = +0,
// stat = (0, 0, 0, s_n).
//
// Backward for g = dL/dy: gm_n = keep ? 2 g_n : 0 (the mask and the residual folded in), t_n = <gm_n, out_n>,
//     de_nj = alpha_nj (<gm_n, E_j> - t_n)
//     dE_j  = sum_{n in j} alpha_nj gm_n + a2 sum_{n in j} de_nj          da2 = sum_j E_j sum_{n in j} de_nj
//     dX_n  = gm_n + sum_{j of n} dE_j + a1 sde_n                         da1 = sum_n X_n sde_n
// where sde_n = sum_{j of n} de_nj = <gm_n, sum_j alpha_nj E_j> - t_n sum_j alpha_nj = t_n (1 - sum_j alpha_nj)
//             = t_n eps'_n / (Z'_n + eps'_n) = t_n stat[n].z: what is left of s_n's cancellation in the softmax, taken from its
// closed form (summed entry by entry in fp32 it is rounding noise of the size of alpha_nj t_n around a value 1e-16 / Z_n of that).
//
// Sums over a row's entries (up to the number of hyperedges) and the dot products run in double and are rounded to fp32 once:
// a node's output is a mean of hundreds of nearly equal rows in which the fp32 running sum's error, not the terms', would set
// the result's last digits (the modal weights' gradient, a difference of two table-wide products, showed it: 1.3e-6 against
// 2e-7 of the float64 value).  The launches stay bound by their gathers.
//
// Layout.  A row is 256 B: 16 lanes x float4, so a wave holds four rows and issues full 16-byte loads; a workgroup of 256
// threads holds MH_GB = 16 lane groups.  Hyperedge launches: a group per hyperedge, its k rows in table order.  Node launches: a
// group per node, its CSR row in order.  A node row longer than MH_LONG entries is cut into chunks of MH_CHUNK entries, each
// taken by a workgroup (its 16 groups' sums added in group order); a second launch adds a row's chunk partials in chunk
// order (the forward's carry their own maxima and are rescaled to the row's).  da1 / da2 leave the launches as one partial row per
// workgroup, for chaorec_colsum_f32.  Every output has one owner and every sum a fixed order: no float atomics, the same bits on
// every run.
// The dropout draw: keep (n, d) when draw_uniform<24>(draw_key(seed, state[1], MH_SALT + salt), n, d) >= 0.5; keep != NULL:
// given uint8 flags [N, 64]; keep == NULL and training == 0: no dropout, y = out + X.
#include <float.h>
#include <math.h>
#include "draws.h"

namespace chaorec {

constexpr int MH_D = 64;
constexpr int MH_GB = 16;             // lane groups (rows) per workgroup
constexpr int MH_LONG = 256;          // a longer node row goes through the chunk launches
constexpr int MH_CHUNK = 256;         // entries per chunk workgroup
constexpr uint64_t MH_SALT = 0x6d68726563687970ull;
constexpr float MH_LOG_EPS = -36.841361487904734f;      // log(1e-16)

struct MhDrop {
  const uint8_t *keep;
  uint64_t key;
  int training;
};

// the epilogue's multiplier of element (n, d): 2 kept, 0 dropped, 1 without dropout
__device__ __forceinline__ float mh_mult(const MhDrop &dr, int64_t n, int d) {
  if (dr.keep) return dr.keep[n * MH_D + d] ? 2.f : 0.f;
  if (!dr.training) return 1.f;
  return draw_uniform<24>(dr.key, (uint64_t)n, (uint64_t)d) >= 0.5f ? 2.f : 0.f;
}
// a dropped element is +0 whatever it held
__device__ __forceinline__ float mh_masked(const MhDrop &dr, int64_t n, int d, float v) {
  const float m = mh_mult(dr, n, d);
  return m == 0.f ? 0.f : m * v;
}
__device__ __forceinline__ float4 mh_masked4(const MhDrop &dr, int64_t n, int d0, float4 v) {
  return make_float4(mh_masked(dr, n, d0, v.x), mh_masked(dr, n, d0 + 1, v.y), mh_masked(dr, n, d0 + 2, v.z), mh_masked(dr, n, d0 + 3, v.w));
}
__device__ __forceinline__ MhDrop mh_drop(const uint8_t *keep, uint64_t seed, const int64_t *state, uint64_t salt, int training) {
  MhDrop dr;
  dr.keep = keep;
  dr.training = training;
  dr.key = (!keep && training) ? draw_key(seed, (uint64_t)state[1], MH_SALT + salt) : 0;
  return dr;
}

// four columns of a row's running sum, in double
struct d4 {
  double x, y, z, w;
};
__device__ __forceinline__ d4 d4_zero() { return d4{0.0, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ d4 d4_of(float4 v) { return d4{(double)v.x, (double)v.y, (double)v.z, (double)v.w}; }
__device__ __forceinline__ d4 add(d4 a, float4 v) { return d4{a.x + (double)v.x, a.y + (double)v.y, a.z + (double)v.z, a.w + (double)v.w}; }
__device__ __forceinline__ d4 add(d4 a, d4 b) { return d4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }
__device__ __forceinline__ d4 fma(double s, float4 v, d4 a) {
  return d4{::fma(s, (double)v.x, a.x), ::fma(s, (double)v.y, a.y), ::fma(s, (double)v.z, a.z), ::fma(s, (double)v.w, a.w)};
}
__device__ __forceinline__ d4 scale(d4 a, double s) { return d4{a.x * s, a.y * s, a.z * s, a.w * s}; }
__device__ __forceinline__ float4 rounded(d4 a) { return make_float4((float)a.x, (float)a.y, (float)a.z, (float)a.w); }
__device__ __forceinline__ double dot(float4 a, float4 b) {
  return ::fma((double)a.w, (double)b.w, ::fma((double)a.z, (double)b.z, ::fma((double)a.y, (double)b.y, (double)a.x * (double)b.x)));
}

__device__ __forceinline__ float4 ld4(const float *p, int64_t row, int sub) { return reinterpret_cast<const float4 *>(p + row * MH_D)[sub]; }
__device__ __forceinline__ void st4(float *p, int64_t row, int sub, float4 v) { reinterpret_cast<float4 *>(p + row * MH_D)[sub] = v; }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float group_max16(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// the node's statistics from its shifted sums; out = acc * (1 / den)
__device__ __forceinline__ float4 mh_stat(float s, float rmax, double Z, double &inv) {
  const double eps = exp((double)MH_LOG_EPS - ((double)s + (double)rmax));       // 1e-16 exp(-M_n)
  const double den = Z + eps;
  inv = 1.0 / den;
  const float inv_f = (float)inv;
  if (isinf(eps) || inv_f == 0.f) {      // the whole row underflows against the 1e-16: alpha = 0
    inv = 0.0;
    return make_float4(-rmax, 0.f, 1.f, s);
  }
  return make_float4(-rmax, inv_f, (float)(eps * inv), s);
}

// the sums of the 16 groups' rows in group order: part[g][d] -> the value of column threadIdx.x, for the first 64 threads
__device__ __forceinline__ double mh_block_rows_sum(double (&part)[MH_GB][MH_D]) {
  __syncthreads();
  double v = 0.0;
  if (threadIdx.x < MH_D) {
#pragma unroll
    for (int g = 0; g < MH_GB; ++g) v += part[g][threadIdx.x];
  }
  return v;
}
__device__ __forceinline__ void mh_part_store(double (&part)[MH_GB][MH_D], int grp, int sub, d4 v) {
  part[grp][4 * sub + 0] = v.x;
  part[grp][4 * sub + 1] = v.y;
  part[grp][4 * sub + 2] = v.z;
  part[grp][4 * sub + 3] = v.w;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mh_edge_fwd_kernel(const int32_t *__restrict__ nodes, int64_t E, int k, int64_t N,
                                                          const float *__restrict__ X, const float *__restrict__ a,
                                                          float *__restrict__ Eo, float *__restrict__ r) {
  const int sub = threadIdx.x & 15;
  const int64_t j = (int64_t)blockIdx.x * MH_GB + (threadIdx.x >> 4);
  if (j >= E) return;                     // (a lane group leaves together; nothing below crosses groups)
  const int32_t *row = nodes + j * k;
  d4 acc = d4_zero();
  int i = 0;
  for (; i + 4 <= k; i += 4) {            // four rows in flight, added in table order
    const float4 x0 = ld4(X, clamp_index(row[i], N), sub), x1 = ld4(X, clamp_index(row[i + 1], N), sub);
    const float4 x2 = ld4(X, clamp_index(row[i + 2], N), sub), x3 = ld4(X, clamp_index(row[i + 3], N), sub);
    acc = add(add(add(add(acc, x0), x1), x2), x3);
  }
  for (; i < k; ++i) acc = add(acc, ld4(X, clamp_index(row[i], N), sub));
  const float4 Ej = rounded(acc);
  st4(Eo, j, sub, Ej);
  const double rr = group_sum<16>(dot(Ej, ld4(a, 1, sub)));       // of the STORED row: what every later launch reads
  if (sub == 0) r[j] = (float)rr;
}

__global__ __launch_bounds__(256) void mh_node_fwd_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ edge, int64_t N,
                                                          int64_t E, int64_t nnz, const float *__restrict__ X, const float *__restrict__ a,
                                                          const float *__restrict__ Eo, const float *__restrict__ r, const uint8_t *keep,
                                                          uint64_t seed, const int64_t *__restrict__ state, uint64_t salt, int training,
                                                          float4 *__restrict__ stat, float *__restrict__ out, float *__restrict__ y) {
  const int sub = threadIdx.x & 15;
  const int64_t n = (int64_t)blockIdx.x * MH_GB + (threadIdx.x >> 4);
  if (n >= N) return;
  const int64_t beg = max((int64_t)0, rowptr[n]), end = min(rowptr[n + 1], nnz);
  if (end - beg > MH_LONG) return;        // the chunk launches own this row
  const float4 x = ld4(X, n, sub);
  const float s = (float)group_sum<16>(dot(x, ld4(a, 0, sub)));
  float rmax = -INFINITY;
  for (int64_t e = beg + sub; e < end; e += 16) rmax = fmaxf(rmax, r[clamp_index((int64_t)edge[e], E)]);
  rmax = group_max16(rmax);
  double Z = 0.0;
  d4 acc = d4_zero();
  int64_t e = beg;
  for (; e + 2 <= end; e += 2) {          // two rows in flight, added in entry order
    const int64_t j0 = clamp_index((int64_t)edge[e], E), j1 = clamp_index((int64_t)edge[e + 1], E);
    const float4 E0 = ld4(Eo, j0, sub), E1 = ld4(Eo, j1, sub);
    const double w0 = (double)expf(r[j0] - rmax), w1 = (double)expf(r[j1] - rmax);
    Z = (Z + w0) + w1;
    acc = fma(w1, E1, fma(w0, E0, acc));
  }
  if (e < end) {
    const int64_t j0 = clamp_index((int64_t)edge[e], E);
    const double w0 = (double)expf(r[j0] - rmax);
    Z += w0;
    acc = fma(w0, ld4(Eo, j0, sub), acc);
  }
  float4 st = make_float4(0.f, 0.f, 0.f, s), o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (end > beg) {
    double inv;
    st = mh_stat(s, rmax, Z, inv);
    o = rounded(scale(acc, inv));
  }
  if (sub == 0) stat[n] = st;
  st4(out, n, sub, o);
  const MhDrop dr = mh_drop(keep, seed, state, salt, training);
  st4(y, n, sub, mh_masked4(dr, n, 4 * sub, add4(o, x)));
}

// one chunk of a long row.  FWD: the chunk's own maximum m, Z = sum exp(r - m), acc = sum exp(r - m) E_j over Eo's rows;
// otherwise the plain sum of the rows of `rows` (the backward's dE).  pacc double [C, 64], pz double [C, 2] = (m, Z).
template <bool FWD>
__global__ __launch_bounds__(256) void mh_chunk_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ edge, int64_t N,
                                                       int64_t E, int64_t nnz, const int32_t *__restrict__ chunk_node,
                                                       const int64_t *__restrict__ chunk_beg, const float *__restrict__ rows,
                                                       const float *__restrict__ r, double *__restrict__ pacc, double *__restrict__ pz) {
  __shared__ double part[MH_GB][MH_D];
  __shared__ float red[256];
  __shared__ double zs[MH_GB];
  const int t = threadIdx.x, sub = t & 15, grp = t >> 4;
  const int64_t c = blockIdx.x;
  const int64_t n = clamp_index((int64_t)chunk_node[c], N);
  const int64_t beg = clamp_index(chunk_beg[c], nnz), end = min(min(beg + MH_CHUNK, rowptr[n + 1]), nnz);
  float m = 0.f;
  if (FWD) {
    float v = -INFINITY;
    for (int64_t e = beg + t; e < end; e += 256) v = fmaxf(v, r[clamp_index((int64_t)edge[e], E)]);
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) red[t] = fmaxf(red[t], red[t + s]);
      __syncthreads();
    }
    m = red[0];
  }
  double Z = 0.0;
  d4 acc = d4_zero();
  for (int64_t e = beg + grp; e < end; e += MH_GB) {
    const int64_t j = clamp_index((int64_t)edge[e], E);
    if (FWD) {
      const double w = (double)expf(r[j] - m);
      Z += w;
      acc = fma(w, ld4(rows, j, sub), acc);
    } else {
      acc = add(acc, ld4(rows, j, sub));
    }
  }
  mh_part_store(part, grp, sub, acc);
  if (FWD && sub == 0) zs[grp] = Z;
  const double col = mh_block_rows_sum(part);
  if (t < MH_D) pacc[c * MH_D + t] = col;
  if (FWD && t == 0) {
    double z = 0.0;
#pragma unroll
    for (int g = 0; g < MH_GB; ++g) z += zs[g];
    pz[2 * c] = (double)m;
    pz[2 * c + 1] = z;
  }
}

// a long row's chunk partials added in chunk order, then the node launch's tail.  One wave per row, lane = column.
__global__ __launch_bounds__(64) void mh_long_fwd_kernel(const int32_t *__restrict__ long_node, const int64_t *__restrict__ long_cptr,
                                                         int64_t N, int64_t C, const float *__restrict__ X, const float *__restrict__ a,
                                                         const double *__restrict__ pacc, const double *__restrict__ pz, const uint8_t *keep,
                                                         uint64_t seed, const int64_t *__restrict__ state, uint64_t salt, int training,
                                                         float4 *__restrict__ stat, float *__restrict__ out, float *__restrict__ y) {
  const int lane = threadIdx.x;
  const int64_t n = clamp_index((int64_t)long_node[blockIdx.x], N);
  const int64_t c0 = clamp_index(long_cptr[blockIdx.x], C), c1 = min(long_cptr[blockIdx.x + 1], C);
  const float x = X[n * MH_D + lane];
  const float s = (float)group_sum<64>((double)x * (double)a[lane]);
  float rmax = -INFINITY;
  for (int64_t c = c0; c < c1; ++c) rmax = fmaxf(rmax, (float)pz[2 * c]);
  double Z = 0.0, acc = 0.0;
  for (int64_t c = c0; c < c1; ++c) {
    const double f = (double)expf((float)pz[2 * c] - rmax);
    Z = ::fma(f, pz[2 * c + 1], Z);
    acc = ::fma(f, pacc[c * MH_D + lane], acc);
  }
  double inv;
  const float4 st = mh_stat(s, rmax, Z, inv);
  const float o = (float)(acc * inv);
  if (lane == 0) stat[n] = st;
  out[n * MH_D + lane] = o;
  const MhDrop dr = mh_drop(keep, seed, state, salt, training);
  y[n * MH_D + lane] = mh_masked(dr, n, lane, o + x);
}

// ---- backward --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mh_prologue_kernel(const float *__restrict__ g, const float *__restrict__ out, int64_t N,
                                                          const uint8_t *keep, uint64_t seed, const int64_t *__restrict__ state, uint64_t salt,
                                                          int training, float *__restrict__ gm, float *__restrict__ tn) {
  const int sub = threadIdx.x & 15;
  const int64_t n = (int64_t)blockIdx.x * MH_GB + (threadIdx.x >> 4);
  if (n >= N) return;
  const MhDrop dr = mh_drop(keep, seed, state, salt, training);
  const float4 v = mh_masked4(dr, n, 4 * sub, ld4(g, n, sub));
  st4(gm, n, sub, v);
  const double t = group_sum<16>(dot(v, ld4(out, n, sub)));
  if (sub == 0) tn[n] = (float)t;
}

__global__ __launch_bounds__(256) void mh_edge_bwd_kernel(const int32_t *__restrict__ nodes, int64_t E, int k, int64_t N,
                                                          const float *__restrict__ a, const float *__restrict__ Eo, const float *__restrict__ r,
                                                          const float4 *__restrict__ stat, const float *__restrict__ gm,
                                                          const float *__restrict__ tn, float *__restrict__ dE, float *__restrict__ pa2) {
  __shared__ double part[MH_GB][MH_D];
  const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int64_t j = (int64_t)blockIdx.x * MH_GB + grp;
  d4 p = d4_zero();
  if (j < E) {
    const float4 Ej = ld4(Eo, j, sub);
    const float rj = r[j];
    const int32_t *row = nodes + j * k;
    d4 acc = d4_zero();
    double sde = 0.0;
    for (int i = 0; i < k; ++i) {
      const int64_t n = clamp_index((int64_t)row[i], N);
      const float4 st = stat[n], gn = ld4(gm, n, sub);
      const double alpha = (double)expf(rj + st.x) * (double)st.y;
      sde += alpha * (group_sum<16>(dot(gn, Ej)) - (double)tn[n]);
      acc = fma(alpha, gn, acc);
    }
    st4(dE, j, sub, rounded(fma(sde, ld4(a, 1, sub), acc)));
    p = scale(d4_of(Ej), sde);
  }
  mh_part_store(part, grp, sub, p);
  const double col = mh_block_rows_sum(part);
  if (threadIdx.x < MH_D) pa2[(int64_t)blockIdx.x * MH_D + threadIdx.x] = (float)col;
}

__global__ __launch_bounds__(256) void mh_node_bwd_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ edge, int64_t N,
                                                          int64_t E, int64_t nnz, const float *__restrict__ X, const float *__restrict__ a,
                                                          const float4 *__restrict__ stat, const float *__restrict__ gm,
                                                          const float *__restrict__ tn, const float *__restrict__ dE, float *__restrict__ dX,
                                                          float *__restrict__ pa1) {
  __shared__ double part[MH_GB][MH_D];
  const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int64_t n = (int64_t)blockIdx.x * MH_GB + grp;
  d4 p = d4_zero();
  if (n < N) {
    const double sde = (double)tn[n] * (double)stat[n].z;
    p = scale(d4_of(ld4(X, n, sub)), sde);
    const int64_t beg = max((int64_t)0, rowptr[n]), end = min(rowptr[n + 1], nnz);
    if (end - beg <= MH_LONG) {           // (a longer row: mh_long_bwd_kernel writes dX)
      d4 acc = d4_of(ld4(gm, n, sub));
      int64_t e = beg;
      for (; e + 2 <= end; e += 2) {
        const float4 d0 = ld4(dE, clamp_index((int64_t)edge[e], E), sub), d1 = ld4(dE, clamp_index((int64_t)edge[e + 1], E), sub);
        acc = add(add(acc, d0), d1);
      }
      if (e < end) acc = add(acc, ld4(dE, clamp_index((int64_t)edge[e], E), sub));
      st4(dX, n, sub, rounded(fma(sde, ld4(a, 0, sub), acc)));
    }
  }
  mh_part_store(part, grp, sub, p);
  const double col = mh_block_rows_sum(part);
  if (threadIdx.x < MH_D) pa1[(int64_t)blockIdx.x * MH_D + threadIdx.x] = (float)col;
}

__global__ __launch_bounds__(64) void mh_long_bwd_kernel(const int32_t *__restrict__ long_node, const int64_t *__restrict__ long_cptr,
                                                         int64_t N, int64_t C, const float *__restrict__ a, const float4 *__restrict__ stat,
                                                         const float *__restrict__ gm, const float *__restrict__ tn,
                                                         const double *__restrict__ pacc, float *__restrict__ dX) {
  const int lane = threadIdx.x;
  const int64_t n = clamp_index((int64_t)long_node[blockIdx.x], N);
  const int64_t c0 = clamp_index(long_cptr[blockIdx.x], C), c1 = min(long_cptr[blockIdx.x + 1], C);
  double acc = (double)gm[n * MH_D + lane];
  for (int64_t c = c0; c < c1; ++c) acc += pacc[c * MH_D + lane];
  dX[n * MH_D + lane] = (float)::fma((double)tn[n] * (double)stat[n].z, (double)a[lane], acc);
}

static inline unsigned mh_blocks(int64_t rows) { return (unsigned)((rows + MH_GB - 1) / MH_GB); }

static int mh_check(const char *what, int64_t E, int32_t k, int64_t N, int64_t L, int64_t C, const void *long_node, const void *long_cptr,
                    const void *chunk_node, const void *chunk_beg, const void *pacc) {
  if (E <= 0 || k <= 0 || N <= 0 || L < 0 || C < L || E >= ((int64_t)1 << 31) - MH_GB || N >= ((int64_t)1 << 31) - MH_GB ||
      E * (int64_t)k >= ((int64_t)1 << 31))
    return fail(CHAOREC_E_INVALID, "%s: E=%lld k=%d N=%lld long=%lld chunks=%lld", what, (long long)E, (int)k, (long long)N, (long long)L,
                (long long)C);
  if (L > 0 && (!long_node || !long_cptr || !chunk_node || !chunk_beg || !pacc))
    return fail(CHAOREC_E_INVALID, "%s: long rows without their chunk lists", what);
  return CHAOREC_OK;
}

static bool mh_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_mhrec_check_shape(int32_t D) {
  if (D != MH_D) return fail(CHAOREC_E_INVALID, "mhrec_check_shape: D=%d, the kernels tile D=%d", (int)D, MH_D);
  return CHAOREC_OK;
}

extern "C" int64_t chaorec_mhrec_long_row(void) { return MH_LONG; }
extern "C" int64_t chaorec_mhrec_chunk(void) { return MH_CHUNK; }
extern "C" int64_t chaorec_mhrec_rows_per_block(void) { return MH_GB; }

extern "C" int chaorec_mhrec_layer_fwd_f32(const int32_t *nodes, int64_t E, int32_t k, const int64_t *rowptr, const int32_t *edge, int64_t N,
                                           const int32_t *long_node, const int64_t *long_cptr, int64_t L, const int32_t *chunk_node,
                                           const int64_t *chunk_beg, int64_t C, const float *X, const float *a, const uint8_t *keep,
                                           uint64_t seed, const int64_t *state, int32_t salt, int32_t training, float *Eo, float *r,
                                           float *stat, float *out, float *y, double *pacc, double *pz, void *stream) {
  if (!nodes || !rowptr || !edge || !X || !a || !Eo || !r || !stat || !out || !y) return fail(CHAOREC_E_INVALID, "mhrec_layer_fwd: NULL argument");
  if (int rc = mh_check("mhrec_layer_fwd", E, k, N, L, C, long_node, long_cptr, chunk_node, chunk_beg, pacc)) return rc;
  if (L > 0 && !pz) return fail(CHAOREC_E_INVALID, "mhrec_layer_fwd: long rows without pz");
  if (!keep && training && !state) return fail(CHAOREC_E_INVALID, "mhrec_layer_fwd: neither a mask nor a step counter");
  if (salt < 0) return fail(CHAOREC_E_INVALID, "mhrec_layer_fwd: salt=%d", (int)salt);
  if (mh_misaligned(X) || mh_misaligned(a) || mh_misaligned(Eo) || mh_misaligned(stat) || mh_misaligned(out) || mh_misaligned(y))
    return fail(CHAOREC_E_INVALID, "mhrec_layer_fwd: X, a, Eo, stat, out and y must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nnz = E * (int64_t)k;
  hipLaunchKernelGGL(mh_edge_fwd_kernel, dim3(mh_blocks(E)), dim3(256), 0, st, nodes, E, (int)k, N, X, a, Eo, r);
  hipLaunchKernelGGL(mh_node_fwd_kernel, dim3(mh_blocks(N)), dim3(256), 0, st, rowptr, edge, N, E, nnz, X, a, (const float *)Eo,
                     (const float *)r, keep, seed, state, (uint64_t)salt, (int)training, reinterpret_cast<float4 *>(stat), out, y);
  if (L > 0) {
    hipLaunchKernelGGL((mh_chunk_kernel<true>), dim3((unsigned)C), dim3(256), 0, st, rowptr, edge, N, E, nnz, chunk_node, chunk_beg,
                       (const float *)Eo, (const float *)r, pacc, pz);
    hipLaunchKernelGGL(mh_long_fwd_kernel, dim3((unsigned)L), dim3(64), 0, st, long_node, long_cptr, N, C, X, a, (const double *)pacc,
                       (const double *)pz, keep, seed, state, (uint64_t)salt, (int)training, reinterpret_cast<float4 *>(stat), out, y);
  }
  return check_launch("mhrec_layer_fwd");
}

extern "C" int chaorec_mhrec_layer_bwd_f32(const int32_t *nodes, int64_t E, int32_t k, const int64_t *rowptr, const int32_t *edge, int64_t N,
                                           const int32_t *long_node, const int64_t *long_cptr, int64_t L, const int32_t *chunk_node,
                                           const int64_t *chunk_beg, int64_t C, const float *g, const float *X, const float *a,
                                           const float *Eo, const float *r, const float *stat, const float *out, const uint8_t *keep,
                                           uint64_t seed, const int64_t *state, int32_t salt, int32_t training, float *gm, float *tn,
                                           float *dE, float *dX, float *pa1, float *pa2, double *pacc, void *stream) {
  if (!nodes || !rowptr || !edge || !g || !X || !a || !Eo || !r || !stat || !out || !gm || !tn || !dE || !dX || !pa1 || !pa2)
    return fail(CHAOREC_E_INVALID, "mhrec_layer_bwd: NULL argument");
  if (int rc = mh_check("mhrec_layer_bwd", E, k, N, L, C, long_node, long_cptr, chunk_node, chunk_beg, pacc)) return rc;
  if (!keep && training && !state) return fail(CHAOREC_E_INVALID, "mhrec_layer_bwd: neither a mask nor a step counter");
  if (salt < 0) return fail(CHAOREC_E_INVALID, "mhrec_layer_bwd: salt=%d", (int)salt);
  if (mh_misaligned(g) || mh_misaligned(X) || mh_misaligned(a) || mh_misaligned(Eo) || mh_misaligned(stat) || mh_misaligned(out) ||
      mh_misaligned(gm) || mh_misaligned(dE) || mh_misaligned(dX))
    return fail(CHAOREC_E_INVALID, "mhrec_layer_bwd: the row tables must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nnz = E * (int64_t)k;
  const float4 *stat4 = reinterpret_cast<const float4 *>(stat);
  hipLaunchKernelGGL(mh_prologue_kernel, dim3(mh_blocks(N)), dim3(256), 0, st, g, out, N, keep, seed, state, (uint64_t)salt, (int)training, gm, tn);
  hipLaunchKernelGGL(mh_edge_bwd_kernel, dim3(mh_blocks(E)), dim3(256), 0, st, nodes, E, (int)k, N, a, Eo, r, stat4, (const float *)gm,
                     (const float *)tn, dE, pa2);
  hipLaunchKernelGGL(mh_node_bwd_kernel, dim3(mh_blocks(N)), dim3(256), 0, st, rowptr, edge, N, E, nnz, X, a, stat4, (const float *)gm,
                     (const float *)tn, (const float *)dE, dX, pa1);
  if (L > 0) {
    hipLaunchKernelGGL((mh_chunk_kernel<false>), dim3((unsigned)C), dim3(256), 0, st, rowptr, edge, N, E, nnz, chunk_node, chunk_beg,
                       (const float *)dE, (const float *)nullptr, pacc, (double *)nullptr);
    hipLaunchKernelGGL(mh_long_bwd_kernel, dim3((unsigned)L), dim3(64), 0, st, long_node, long_cptr, N, C, a, stat4, (const float *)gm,
                       (const float *)tn, (const double *)pacc, dX);
  }
  return check_launch("mhrec_layer_bwd");
}
