// The user-user co-occurrence graph of DRAGON (and of DualGNN, COHESION, MHRec, which read the same file): built on the
// device from the interactions, sampled per epoch on the device, aggregated without a [U, k, 2D] gather.
//
//  (a) ug_build_kernel     row u of R R^T (R = the user-item matrix) cut to its N largest entries, no [U, U] buffer: one
//                          workgroup per user, the counters of a TILE of user ids in LDS.  Replaces the reference's
//                          dualgnn-gen-u-u-matrix.py (a dense [U, U] float matrix filled by a Python double loop, :20-50,
//                          then torch.topk per row, :90-103).
//  (b) ug_sample_kernel    Model/DRAGON.py:231-270 (topk_sample): the first k neighbours, padded by the reference's urn
//                          when a user has fewer, and the softmax of their counts.
//  (c) ug_agg_fwd / _bwd   Model/DRAGON.py:289-302 (weight_u * [v_rep | t_rep], User_Graph_sample.forward, the residual)
//                          and its gradient, one lane group per row, ordered and atomic-free.
//  (d) dg_fuse_fwd / _bwd  Model/DualGNN.py:189-239: the same aggregation over the weighted SUM a v + b t, with the item rows
//                          v + t in the same launch -- the whole result table [U + I, D] and its gradient.
//  (e) cf_fuse_fwd / cf_chunk / cf_rows   Model/COHESION.py:340-359: the aggregation over rows of three tables side by side
//                          (id | v | t, 192 floats), the item rows plus their item-graph term -- and a backward whose long
//                          reverse lists are cut into chunks summed by separate lane groups, the partials added in chunk order.
//
// Key convention (the project's): (count << 32) | (0xFFFFFFFF - id), larger key first = count descending, id ascending.
// A key of 0 is "no entry" (a count of 0 is never stored).
#include "draws.h"

namespace chaorec {

constexpr int UG_THREADS = 256;
constexpr int UG_MAX_N = 256;          // neighbours kept per user (the reference keeps 200)
constexpr int UG_MAX_TILE = 32768;     // 32-bit counters of one tile: 128 KiB of the CU's 160 KiB LDS

// sum / max of one int per thread over the workgroup, the same value returned to every thread (red: 4 ints of LDS)
__device__ __forceinline__ int ug_block_sum(int v, int *red) {
  v = group_sum<64>(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ int ug_block_max(int v, int *red) {
  v = wave_max_i32(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const int a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
  return a > b ? a : b;
}

__device__ __forceinline__ uint64_t ug_key(int count, int64_t id) {
  return ((uint64_t)(uint32_t)count << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)id);
}

// keys[0 .. n) into descending order (n a power of two, every workgroup thread calls; sorted on return)
__device__ __forceinline__ void ug_bitonic_desc(uint64_t *keys, int n) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += UG_THREADS) {
        const int p = i ^ j;
        if (p > i) {
          const uint64_t a = keys[i], b = keys[p];
          if (((i & k) == 0) ? a < b : a > b) {
            keys[i] = b;
            keys[p] = a;
          }
        }
      }
      __syncthreads();
    }
}

// One workgroup per user u.  Per tile [lo, lo + tile) of user ids:
//   1. walk items(u) x holders(i) (a wave per item, a lane per holder) and bump the LDS counter of every holder in the tile:
//      integer atomics, so the counters do not depend on the order in which they land;
//   2. find the cut: the largest count T that at least N users reach, by bisection over [1, max count] (a counting scan of
//      the tile per probe -- counts are small integers, a handful of probes);
//   3. take every user above T (fewer than N, in any order: they are sorted afterwards and their keys are distinct) and the
//      lowest ids AT T, which an exclusive prefix over the threads' contiguous id ranges hands out in id order; the same
//      pass clears the counters for the next tile;
//   4. sort the at most N new keys together with the N carried from the tiles before (top-N of a union = top-N of the
//      parts' top-Ns) and keep the first N.
__global__ __launch_bounds__(UG_THREADS) void ug_build_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                              const int64_t *__restrict__ item_ptr, const int32_t *__restrict__ item_users,
                                                              int64_t U, int64_t I, int N, int tile, int32_t *__restrict__ nbr_idx,
                                                              int32_t *__restrict__ nbr_cnt, int32_t *__restrict__ nbr_len) {
  extern __shared__ int ug_cnt[];                 // [tile]
  __shared__ uint64_t keys[2 * UG_MAX_N];         // [0, 256): carried from earlier tiles; [256, 512): this tile's
  __shared__ int scan[UG_THREADS];
  __shared__ int red[4];
  __shared__ int n_above;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t u = blockIdx.x;
  for (int j = t; j < tile; j += UG_THREADS) ug_cnt[j] = 0;
  keys[t] = 0;
  keys[t + UG_THREADS] = 0;
  __syncthreads();
  const int64_t ubeg = rowptr[u], uend = rowptr[u + 1];
  const bool single = (int64_t)tile >= U;         // one tile: nothing is carried, the new half alone is sorted
  for (int64_t lo = 0; lo < U; lo += tile) {
    const int64_t hi = lo + tile < U ? lo + tile : U;
    const int span = (int)(hi - lo);
    for (int64_t e = ubeg + wave; e < uend; e += UG_THREADS / 64) {
      const int64_t i = col[e];
      if (i < 0 || i >= I) continue;
      const int64_t hend = item_ptr[i + 1];
      for (int64_t h = item_ptr[i] + lane; h < hend; h += 64) {
        const int64_t v = item_users[h];
        if (v != u && v >= lo && v < hi) atomicAdd(&ug_cnt[v - lo], 1);
      }
    }
    __syncthreads();
    int nz = 0, mx = 0;
    for (int j = t; j < span; j += UG_THREADS) {
      const int c = ug_cnt[j];
      nz += c > 0;
      mx = c > mx ? c : mx;
    }
    const int c1 = ug_block_sum(nz, red);
    if (c1 == 0) continue;                        // (uniform) nobody in this tile shares an item; the counters are zero
    const int maxc = ug_block_max(mx, red);
    int T = 0, A = c1;                            // take every count above T: A of them; T = 0 takes all c1 <= N
    if (c1 > N) {
      int64_t lo_t = 1, hi_t = (int64_t)maxc + 1; // count(>= lo_t) >= N > count(>= hi_t) = c_hi
      int c_hi = 0;
      while (hi_t - lo_t > 1) {
        const int mid = (int)(lo_t + (hi_t - lo_t) / 2);
        int n = 0;
        for (int j = t; j < span; j += UG_THREADS) n += ug_cnt[j] >= mid;
        n = ug_block_sum(n, red);
        if (n >= N) lo_t = mid;
        else hi_t = mid, c_hi = n;
      }
      T = (int)lo_t;
      A = c_hi;
    }
    const int need = N - A;                       // of the users AT T, the `need` lowest ids (T > 0 only)
    const int chunk = ((span + UG_THREADS - 1) / UG_THREADS) | 1;   // odd: the threads' ranges start in different banks
    const int j0 = t * chunk < span ? t * chunk : span, j1 = j0 + chunk < span ? j0 + chunk : span;
    int at = 0;
    if (T > 0)
      for (int j = j0; j < j1; ++j) at += ug_cnt[j] == T;
    if (t == 0) n_above = 0;
    scan[t] = at;
    __syncthreads();
    for (int off = 1; off < UG_THREADS; off <<= 1) {   // inclusive prefix over the threads
      const int add = t >= off ? scan[t - off] : 0;
      __syncthreads();
      scan[t] += add;
      __syncthreads();
    }
    int p = scan[t] - at;
    uint64_t *fresh = keys + UG_MAX_N;
    for (int j = j0; j < j1; ++j) {
      const int c = ug_cnt[j];
      ug_cnt[j] = 0;
      if (c > T) {
        const int s = atomicAdd(&n_above, 1);
        if (s < UG_MAX_N) fresh[s] = ug_key(c, lo + j);
      } else if (T > 0 && c == T) {
        if (p < need) fresh[A + p] = ug_key(c, lo + j);
        ++p;
      }
    }
    __syncthreads();
    if (single) {
      ug_bitonic_desc(fresh, UG_MAX_N);
    } else {
      ug_bitonic_desc(keys, 2 * UG_MAX_N);
      if (t >= N) keys[t] = 0;
      keys[t + UG_THREADS] = 0;
      __syncthreads();
    }
  }
  const uint64_t *top = single ? keys + UG_MAX_N : keys;
  int have = 0;
  if (t < N) {
    const uint64_t key = top[t];
    have = key != 0;
    nbr_idx[u * N + t] = have ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : 0;
    nbr_cnt[u * N + t] = (int32_t)(key >> 32);
  }
  have = ug_block_sum(have, red);
  if (t == 0) nbr_len[u] = have;
}

// r uniform in [0, n): the negative sampler's generator (bpr.hip sampler_draw) over (seed, epoch, user, slot)
__device__ __forceinline__ uint32_t ug_draw(uint64_t seed, uint64_t epoch, uint32_t u, uint32_t slot, uint32_t n) {
  const uint64_t h = draw_hash(seed, epoch, ((uint64_t)u << 32) | slot);
  return (uint32_t)(((h >> 32) * (uint64_t)n) >> 32);
}

// A wave per user.  Slot j < len is neighbour j; slot j >= len copies slot r_j < j of the GROWN list (the reference's urn,
// Model/DRAGON.py:249-252), so a lane follows its own chain of draws down to an original neighbour: no lane waits for
// another.  The softmax is taken in double and rounded once.
__global__ __launch_bounds__(UG_THREADS) void ug_sample_kernel(const int32_t *__restrict__ nbr_idx, const int32_t *__restrict__ nbr_cnt,
                                                               const int32_t *__restrict__ nbr_len, int64_t U, int N, int k, uint64_t seed,
                                                               uint64_t epoch, int32_t *__restrict__ epoch_idx, float *__restrict__ epoch_w) {
  const int lane = threadIdx.x & 63;
  const int64_t u = (int64_t)blockIdx.x * (UG_THREADS / 64) + (threadIdx.x >> 6);
  if (u >= U) return;
  int len = nbr_len[u];
  len = len < 0 ? 0 : (len > N ? N : len);
  int id[UG_MAX_N / 64], c[UG_MAX_N / 64];
  int mx = 0;
#pragma unroll
  for (int q = 0; q < UG_MAX_N / 64; ++q) {
    const int j = lane + 64 * q;
    id[q] = c[q] = 0;
    if (j < k && len > 0) {
      uint32_t s = (uint32_t)j;
      while (s >= (uint32_t)len) s = ug_draw(seed, epoch, (uint32_t)u, s, s);
      id[q] = nbr_idx[u * N + s];
      c[q] = nbr_cnt[u * N + s];
      mx = c[q] > mx ? c[q] : mx;
    }
  }
  mx = wave_max_i32(mx);
  double e[UG_MAX_N / 64], sum = 0.0;
#pragma unroll
  for (int q = 0; q < UG_MAX_N / 64; ++q) {
    e[q] = (lane + 64 * q < k && len > 0) ? exp((double)(c[q] - mx)) : 0.0;
    sum += e[q];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
#pragma unroll
  for (int q = 0; q < UG_MAX_N / 64; ++q) {
    const int j = lane + 64 * q;
    if (j < k) {
      epoch_idx[u * k + j] = id[q];
      epoch_w[u * k + j] = len > 0 ? (float)(e[q] / sum) : 0.f;   // no neighbour: the reference's all-zero weight row
    }
  }
}

// x[r, :] = (a_r v[r, :], b_r t[r, :]): a lane's four columns of it.  A lane group of D / 2 lanes owns a row of 2 D floats.
template <int D>
struct UgLane {
  const float *src;      // v or t, whichever half this lane is in
  int c, which;
  __device__ __forceinline__ UgLane(const float *v, const float *t, int l) {
    which = l >= D / 4;
    src = which ? t : v;
    c = (which ? l - D / 4 : l) * 4;
  }
  __device__ __forceinline__ float4 raw(int64_t r) const { return *reinterpret_cast<const float4 *>(src + r * D + c); }
};

template <int D>
__global__ __launch_bounds__(UG_THREADS) void ug_agg_fwd_kernel(const float *__restrict__ v, const float *__restrict__ t,
                                                                const float *__restrict__ wu, const int32_t *__restrict__ idx,
                                                                const float *__restrict__ w, int64_t U, int k, float *__restrict__ out) {
  constexpr int LPR = D / 2;
  const int l = threadIdx.x % LPR;
  const int64_t u = (int64_t)blockIdx.x * (UG_THREADS / LPR) + threadIdx.x / LPR;
  if (u >= U) return;
  const UgLane<D> ln(v, t, l);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int32_t *iu = idx + u * k;
  const float *wr = w + u * k;
#pragma unroll 4
  for (int j = 0; j < k; ++j) {
    const int64_t r = iu[j];
    if (r < 0 || r >= U) continue;
    acc = add_rn4(acc, mul_rn4(wr[j], mul_rn4(wu[r * 2 + ln.which], ln.raw(r))));
  }
  const float4 self = mul_rn4(wu[u * 2 + ln.which], ln.raw(u));
  *reinterpret_cast<float4 *>(out + u * (2 * D) + l * 4) = add_rn4(self, acc);
}

// The owner of gradient row r walks the slots that name r, in ascending (u, j): rev_u / rev_w [rev_ptr[r], rev_ptr[r + 1]).
template <int D>
__global__ __launch_bounds__(UG_THREADS) void ug_agg_bwd_kernel(const float *__restrict__ g, const float *__restrict__ v,
                                                                const float *__restrict__ t, const float *__restrict__ wu,
                                                                const int64_t *__restrict__ rev_ptr, const int32_t *__restrict__ rev_u,
                                                                const float *__restrict__ rev_w, int64_t U, float *__restrict__ dv,
                                                                float *__restrict__ dt, float *__restrict__ dw) {
  constexpr int LPR = D / 2;
  const int l = threadIdx.x % LPR;
  const int64_t r = (int64_t)blockIdx.x * (UG_THREADS / LPR) + threadIdx.x / LPR;
  if (r >= U) return;                                // (whole lane groups leave: the shuffles below stay inside a group)
  const UgLane<D> ln(v, t, l);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t end = rev_ptr[r + 1];
#pragma unroll 4
  for (int64_t e = rev_ptr[r]; e < end; ++e) {
    const int64_t u = rev_u[e];
    if (u < 0 || u >= U) continue;
    acc = add_rn4(acc, mul_rn4(rev_w[e], *reinterpret_cast<const float4 *>(g + u * (2 * D) + l * 4)));
  }
  const float4 gx = add_rn4(*reinterpret_cast<const float4 *>(g + r * (2 * D) + l * 4), acc);
  const float4 x = ln.raw(r);
  *reinterpret_cast<float4 *>((ln.which ? dt : dv) + r * D + ln.c) = mul_rn4(wu[r * 2 + ln.which], gx);
  float dot = add_rn(add_rn(mul_rn(gx.x, x.x), mul_rn(gx.y, x.y)), add_rn(mul_rn(gx.z, x.z), mul_rn(gx.w, x.w)));
  dot = group_sum<D / 4>(dot);   // within the half's D / 4 lanes
  if (ln.c == 0) dw[r * 2 + ln.which] = dot;
}

// ---- DualGNN (Model/DualGNN.py:189-239): the modality mix is a weighted SUM, x[r, :] = a_r v[r, :] + b_r t[r, :], a row of D floats
// (DRAGON's is the concatenation above), and the item rows v + t are written by the same launch: one [U + I, D] table out.
// A lane group of D / 4 lanes owns a row, one dwordx4 of v and one of t per lane.
template <int D>
struct DgLane {
  const float *v, *t, *wu;
  int c;
  __device__ __forceinline__ DgLane(const float *v_, const float *t_, const float *wu_, int l) : v(v_), t(t_), wu(wu_), c(l * 4) {}
  __device__ __forceinline__ float4 row(const float *p, int64_t r) const { return *reinterpret_cast<const float4 *>(p + r * D + c); }
  __device__ __forceinline__ float4 x(int64_t r) const {
    return add_rn4(mul_rn4(wu[r * 2], row(v, r)), mul_rn4(wu[r * 2 + 1], row(t, r)));
  }
};

template <int D>
__global__ __launch_bounds__(UG_THREADS) void dg_fuse_fwd_kernel(const float *__restrict__ v, const float *__restrict__ t,
                                                                 const float *__restrict__ wu, const int32_t *__restrict__ idx,
                                                                 const float *__restrict__ w, int64_t U, int64_t N, int k,
                                                                 float *__restrict__ out) {
  constexpr int LPR = D / 4;
  const int64_t r = (int64_t)blockIdx.x * (UG_THREADS / LPR) + threadIdx.x / LPR;
  if (r >= N) return;
  const DgLane<D> ln(v, t, wu, threadIdx.x % LPR);
  float4 *dst = reinterpret_cast<float4 *>(out + r * D + ln.c);
  if (r >= U) {                                      // an item row: representation[U:] = v_rep + t_rep (:189, :231)
    *dst = add_rn4(ln.row(v, r), ln.row(t, r));
    return;
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int32_t *iu = idx + r * k;
  const float *wr = w + r * k;
#pragma unroll 4
  for (int j = 0; j < k; ++j) {
    const int64_t s = iu[j];
    if (s < 0 || s >= U) continue;
    acc = add_rn4(acc, mul_rn4(wr[j], ln.x(s)));
  }
  *dst = add_rn4(ln.x(r), acc);
}

// The owner of gradient row r < U walks the slots that name r as ug_agg_bwd_kernel does; an item row hands g on to both tables.
template <int D>
__global__ __launch_bounds__(UG_THREADS) void dg_fuse_bwd_kernel(const float *__restrict__ g, const float *__restrict__ v,
                                                                 const float *__restrict__ t, const float *__restrict__ wu,
                                                                 const int64_t *__restrict__ rev_ptr, const int32_t *__restrict__ rev_u,
                                                                 const float *__restrict__ rev_w, int64_t U, int64_t N,
                                                                 float *__restrict__ dv, float *__restrict__ dt, float *__restrict__ dw) {
  constexpr int LPR = D / 4;
  const int64_t r = (int64_t)blockIdx.x * (UG_THREADS / LPR) + threadIdx.x / LPR;
  if (r >= N) return;                                // (whole lane groups leave: the shuffles below stay inside a group)
  const DgLane<D> ln(v, t, wu, threadIdx.x % LPR);
  const float4 gr = ln.row(g, r);
  float4 *pv = reinterpret_cast<float4 *>(dv + r * D + ln.c), *pt = reinterpret_cast<float4 *>(dt + r * D + ln.c);
  if (r >= U) {
    *pv = gr;
    *pt = gr;
    return;
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t end = rev_ptr[r + 1];
#pragma unroll 4
  for (int64_t e = rev_ptr[r]; e < end; ++e) {
    const int64_t u = rev_u[e];
    if (u < 0 || u >= U) continue;
    acc = add_rn4(acc, mul_rn4(rev_w[e], ln.row(g, u)));
  }
  const float4 gx = add_rn4(gr, acc);
  *pv = mul_rn4(wu[r * 2], gx);
  *pt = mul_rn4(wu[r * 2 + 1], gx);
  const float4 xv = ln.row(v, r), xt = ln.row(t, r);
  float da = add_rn(add_rn(mul_rn(gx.x, xv.x), mul_rn(gx.y, xv.y)), add_rn(mul_rn(gx.z, xv.z), mul_rn(gx.w, xv.w)));
  float db = add_rn(add_rn(mul_rn(gx.x, xt.x), mul_rn(gx.y, xt.y)), add_rn(mul_rn(gx.z, xt.z), mul_rn(gx.w, xt.w)));
#pragma unroll
  for (int off = LPR / 2; off > 0; off >>= 1) {      // within the row's D / 4 lanes, fixed order
    da += __shfl_xor(da, off, 64);
    db += __shfl_xor(db, off, 64);
  }
  if (ln.c == 0) {
    dw[r * 2] = da;
    dw[r * 2 + 1] = db;
  }
}

// ---- COHESION (Model/COHESION.py:340-359): x[r, :] = (idr[r, :] | v[r, :] | t[r, :]), a row of 3 x 64 floats that is never
// concatenated in memory; the item rows take their item-graph term h = mm_adj^L x[U:] from three [I, 64] tables (or none).
// A lane group of 16 lanes owns a row: the same four columns of each of the three tables, three dwordx4 per lane.
constexpr int CF_D = 64;               // COHESION hard-codes dim_latent = 64
constexpr int CF_W = 3 * CF_D;         // a row of result / g
constexpr int CF_LIVE = 2 * CF_D;      // the columns of g that carry a gradient: the id third is detached (:321)

__device__ __forceinline__ float4 cf_row(const float *p, int64_t r, int c) { return *reinterpret_cast<const float4 *>(p + r * CF_D + c); }

__global__ __launch_bounds__(UG_THREADS) void cf_fuse_fwd_kernel(const float *__restrict__ idr, const float *__restrict__ v,
                                                                 const float *__restrict__ t, const float *__restrict__ h_id,
                                                                 const float *__restrict__ h_v, const float *__restrict__ h_t,
                                                                 const int32_t *__restrict__ idx, const float *__restrict__ w, int64_t U,
                                                                 int64_t N, int k, float *__restrict__ out) {
  constexpr int LPR = CF_D / 4;
  const int64_t r = (int64_t)blockIdx.x * (UG_THREADS / LPR) + threadIdx.x / LPR;
  if (r >= N) return;
  const int c = (threadIdx.x % LPR) * 4;
  float4 *dst = reinterpret_cast<float4 *>(out + r * CF_W + c);
  const float4 x0 = cf_row(idr, r, c), x1 = cf_row(v, r, c), x2 = cf_row(t, r, c);
  if (r >= U) {                                      // an item row: item_rep + h_i (:348-355); no item graph: item_rep
    const int64_t i = r - U;
    const bool has = h_id != nullptr;
    dst[0] = has ? add_rn4(x0, cf_row(h_id, i, c)) : x0;
    dst[CF_D / 4] = has ? add_rn4(x1, cf_row(h_v, i, c)) : x1;
    dst[2 * CF_D / 4] = has ? add_rn4(x2, cf_row(h_t, i, c)) : x2;
    return;
  }
  float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0;
  const int32_t *iu = idx + r * k;
  const float *wr = w + r * k;
#pragma unroll 4
  for (int j = 0; j < k; ++j) {
    const int64_t s = iu[j];
    if (s < 0 || s >= U) continue;
    const float ws = wr[j];
    a0 = add_rn4(a0, mul_rn4(ws, cf_row(idr, s, c)));
    a1 = add_rn4(a1, mul_rn4(ws, cf_row(v, s, c)));
    a2 = add_rn4(a2, mul_rn4(ws, cf_row(t, s, c)));
  }
  dst[0] = add_rn4(x0, a0);
  dst[CF_D / 4] = add_rn4(x1, a1);
  dst[2 * CF_D / 4] = add_rn4(x2, a2);
}

// Backward, first launch.  A lane group of 32 lanes owns one CHUNK of a reverse list -- entries [first, first + chunk) of
// rev_u / rev_w, cut at the end of the row's list -- over the 128 live columns of g, one dwordx4 per lane:
// part[c, :] = ((0 + w_1 g_1) + w_2 g_2) + ... in list order.  No list is longer than `chunk` for any lane group, so the
// launch's time follows the bytes it moves, not the longest list (dg_fuse_bwd_kernel above walks that one alone).
__global__ __launch_bounds__(UG_THREADS) void cf_chunk_kernel(const float *__restrict__ g, const int64_t *__restrict__ rev_ptr,
                                                              const int32_t *__restrict__ rev_u, const float *__restrict__ rev_w,
                                                              const int32_t *__restrict__ chunk_row, const int64_t *__restrict__ chunk_first,
                                                              int64_t n_chunks, int64_t chunk, int64_t U, float *__restrict__ part) {
  constexpr int LPC = CF_LIVE / 4;
  const int64_t q = (int64_t)blockIdx.x * (UG_THREADS / LPC) + threadIdx.x / LPC;
  if (q >= n_chunks) return;
  const int c = (threadIdx.x % LPC) * 4;
  const int64_t r = chunk_row[q];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (r >= 0 && r < U) {
    const int64_t first = chunk_first[q], row_end = rev_ptr[r + 1];
    const int64_t end = (chunk > 0 && first + chunk < row_end) ? first + chunk : row_end;
#pragma unroll 4
    for (int64_t e = first < rev_ptr[r] ? rev_ptr[r] : first; e < end; ++e) {
      const int64_t u = rev_u[e];
      if (u < 0 || u >= U) continue;
      acc = add_rn4(acc, mul_rn4(rev_w[e], *reinterpret_cast<const float4 *>(g + u * CF_W + CF_D + c)));
    }
  }
  *reinterpret_cast<float4 *>(part + q * CF_LIVE + c) = acc;
}

// Backward, second launch.  A lane group of 32 lanes owns gradient row r: a user row adds its chunks' partials in chunk order,
// S = ((p_0 + p_1) + p_2) + ..., then gx = g[r, 64:] + S; an item row hands g[r, 64:] on to the table and to its h term.
// Columns 0 .. 63 of g are never read and nothing is written for them.
__global__ __launch_bounds__(UG_THREADS) void cf_rows_kernel(const float *__restrict__ g, const float *__restrict__ part,
                                                             const int64_t *__restrict__ row_chunk, int64_t n_chunks, int64_t U, int64_t N,
                                                             float *__restrict__ dv, float *__restrict__ dt, float *__restrict__ dh_v,
                                                             float *__restrict__ dh_t) {
  constexpr int LPR = CF_LIVE / 4;
  const int64_t r = (int64_t)blockIdx.x * (UG_THREADS / LPR) + threadIdx.x / LPR;
  if (r >= N) return;
  const int c = (threadIdx.x % LPR) * 4;                      // a column of the live 128: [0, 64) is v's, [64, 128) t's
  const float4 gr = *reinterpret_cast<const float4 *>(g + r * CF_W + CF_D + c);
  const bool is_t = c >= CF_D;
  const int cc = is_t ? c - CF_D : c;
  float4 *dst = reinterpret_cast<float4 *>((is_t ? dt : dv) + r * CF_D + cc);
  if (r >= U) {
    *dst = gr;
    float *dh = is_t ? dh_t : dh_v;
    if (dh) *reinterpret_cast<float4 *>(dh + (r - U) * CF_D + cc) = gr;
    return;
  }
  int64_t q = row_chunk[r], q_end = row_chunk[r + 1];
  q = q < 0 ? 0 : q;
  q_end = q_end > n_chunks ? n_chunks : q_end;
  float4 S = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q < q_end) {
    S = *reinterpret_cast<const float4 *>(part + q * CF_LIVE + c);
    for (++q; q < q_end; ++q) S = add_rn4(S, *reinterpret_cast<const float4 *>(part + q * CF_LIVE + c));
  }
  *dst = add_rn4(gr, S);
}

static int ug_tile(int64_t U, int32_t tile_users) {
  int64_t tile = U < UG_MAX_TILE ? U : UG_MAX_TILE;
  if (tile_users > 0 && tile_users < tile) tile = tile_users;
  return (int)(tile < 1 ? 1 : tile);
}

}  // namespace chaorec

using namespace chaorec;

extern "C" int64_t chaorec_usergraph_max_users(void) { return (int64_t)INT32_MAX; }

extern "C" int64_t chaorec_usergraph_tile_users(int64_t U, int32_t tile_users) { return U > 0 ? ug_tile(U, tile_users) : 0; }

extern "C" int chaorec_usergraph_build(const int64_t *hist_rowptr, const int32_t *hist_col, const int64_t *item_ptr,
                                       const int32_t *item_users, int64_t U, int64_t I, int32_t N, int32_t tile_users, int32_t *nbr_idx,
                                       int32_t *nbr_cnt, int32_t *nbr_len, void *stream) {
  if (!hist_rowptr || !hist_col || !item_ptr || !item_users || !nbr_idx || !nbr_cnt || !nbr_len)
    return fail(CHAOREC_E_INVALID, "usergraph_build: NULL argument");
  if (U <= 0 || U > chaorec_usergraph_max_users() || I <= 0 || I > (int64_t)INT32_MAX)
    return fail(CHAOREC_E_INVALID, "usergraph_build: U=%lld I=%lld (ids are 32-bit: at most %lld users)", (long long)U, (long long)I,
                (long long)chaorec_usergraph_max_users());
  if (N < 1 || N > UG_MAX_N || tile_users < 0)
    return fail(CHAOREC_E_INVALID, "usergraph_build: N=%d (1 .. %d) tile_users=%d", (int)N, UG_MAX_N, (int)tile_users);
  const int tile = ug_tile(U, tile_users);
  const size_t lds = (size_t)tile * sizeof(int);
  if (lds > 48 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ug_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(ug_build_kernel, dim3((unsigned)U), dim3(UG_THREADS), lds, (hipStream_t)stream, hist_rowptr, hist_col, item_ptr,
                     item_users, U, I, (int)N, tile, nbr_idx, nbr_cnt, nbr_len);
  return check_launch("ug_build_kernel");
}

extern "C" int chaorec_usergraph_sample(const int32_t *nbr_idx, const int32_t *nbr_cnt, const int32_t *nbr_len, int64_t U, int32_t N,
                                        int32_t k, uint64_t seed, uint64_t epoch, int32_t *epoch_idx, float *epoch_w, void *stream) {
  if (!nbr_idx || !nbr_cnt || !nbr_len || !epoch_idx || !epoch_w) return fail(CHAOREC_E_INVALID, "usergraph_sample: NULL argument");
  if (U <= 0 || U > chaorec_usergraph_max_users() || N < 1 || N > UG_MAX_N || k < 1 || k > N)
    return fail(CHAOREC_E_INVALID, "usergraph_sample: U=%lld N=%d k=%d (1 <= k <= N <= %d)", (long long)U, (int)N, (int)k, UG_MAX_N);
  hipLaunchKernelGGL(ug_sample_kernel, dim3((unsigned)((U + 3) / 4)), dim3(UG_THREADS), 0, (hipStream_t)stream, nbr_idx, nbr_cnt, nbr_len,
                     U, (int)N, (int)k, seed, epoch, epoch_idx, epoch_w);
  return check_launch("ug_sample_kernel");
}

extern "C" int chaorec_usergraph_aggregate_fwd_f32(const float *v, const float *t, const float *weight_u, const int32_t *epoch_idx,
                                                   const float *epoch_w, int64_t U, int32_t k, int32_t D, float *out, void *stream) {
  if (!v || !t || !weight_u || !epoch_idx || !epoch_w || !out) return fail(CHAOREC_E_INVALID, "usergraph_aggregate_fwd: NULL argument");
  if (U <= 0 || U > chaorec_usergraph_max_users() || k < 1 || (D != 64 && D != 128))
    return fail(CHAOREC_E_INVALID, "usergraph_aggregate_fwd: U=%lld k=%d D=%d (D is 64 or 128)", (long long)U, (int)k, (int)D);
  if (D == 64)
    hipLaunchKernelGGL(ug_agg_fwd_kernel<64>, dim3((unsigned)((U + 7) / 8)), dim3(UG_THREADS), 0, (hipStream_t)stream, v, t, weight_u,
                       epoch_idx, epoch_w, U, (int)k, out);
  else
    hipLaunchKernelGGL(ug_agg_fwd_kernel<128>, dim3((unsigned)((U + 3) / 4)), dim3(UG_THREADS), 0, (hipStream_t)stream, v, t, weight_u,
                       epoch_idx, epoch_w, U, (int)k, out);
  return check_launch("ug_agg_fwd_kernel");
}

extern "C" int chaorec_usergraph_aggregate_bwd_f32(const float *g, const float *v, const float *t, const float *weight_u,
                                                   const int64_t *rev_ptr, const int32_t *rev_u, const float *rev_w, int64_t U, int32_t D,
                                                   float *dv, float *dt, float *dw, void *stream) {
  if (!g || !v || !t || !weight_u || !rev_ptr || !rev_u || !rev_w || !dv || !dt || !dw)
    return fail(CHAOREC_E_INVALID, "usergraph_aggregate_bwd: NULL argument");
  if (U <= 0 || U > chaorec_usergraph_max_users() || (D != 64 && D != 128))
    return fail(CHAOREC_E_INVALID, "usergraph_aggregate_bwd: U=%lld D=%d (D is 64 or 128)", (long long)U, (int)D);
  if (D == 64)
    hipLaunchKernelGGL(ug_agg_bwd_kernel<64>, dim3((unsigned)((U + 7) / 8)), dim3(UG_THREADS), 0, (hipStream_t)stream, g, v, t, weight_u,
                       rev_ptr, rev_u, rev_w, U, dv, dt, dw);
  else
    hipLaunchKernelGGL(ug_agg_bwd_kernel<128>, dim3((unsigned)((U + 3) / 4)), dim3(UG_THREADS), 0, (hipStream_t)stream, g, v, t, weight_u,
                       rev_ptr, rev_u, rev_w, U, dv, dt, dw);
  return check_launch("ug_agg_bwd_kernel");
}

static int dg_check(const char *what, int64_t U, int64_t N, int32_t k, int32_t D) {
  if (U <= 0 || U > chaorec_usergraph_max_users() || N < U || N > 2 * chaorec_usergraph_max_users() || k < 1 || (D != 64 && D != 128))
    return fail(CHAOREC_E_INVALID, "%s: U=%lld N=%lld k=%d D=%d (1 <= U <= N, k >= 1, D is 64 or 128)", what, (long long)U,
                (long long)N, (int)k, (int)D);
  return CHAOREC_OK;
}

extern "C" int chaorec_dualgnn_fuse_fwd_f32(const float *v, const float *t, const float *weight_u, const int32_t *epoch_idx,
                                            const float *epoch_w, int64_t U, int64_t N, int32_t k, int32_t D, float *result,
                                            void *stream) {
  if (!v || !t || !weight_u || !epoch_idx || !epoch_w || !result) return fail(CHAOREC_E_INVALID, "dualgnn_fuse_fwd: NULL argument");
  if (const int rc = dg_check("dualgnn_fuse_fwd", U, N, k, D)) return rc;
  if (D == 64)
    hipLaunchKernelGGL(dg_fuse_fwd_kernel<64>, dim3((unsigned)((N + 15) / 16)), dim3(UG_THREADS), 0, (hipStream_t)stream, v, t, weight_u,
                       epoch_idx, epoch_w, U, N, (int)k, result);
  else
    hipLaunchKernelGGL(dg_fuse_fwd_kernel<128>, dim3((unsigned)((N + 7) / 8)), dim3(UG_THREADS), 0, (hipStream_t)stream, v, t, weight_u,
                       epoch_idx, epoch_w, U, N, (int)k, result);
  return check_launch("dg_fuse_fwd_kernel");
}

extern "C" int chaorec_dualgnn_fuse_bwd_f32(const float *g, const float *v, const float *t, const float *weight_u, const int64_t *rev_ptr,
                                            const int32_t *rev_u, const float *rev_w, int64_t U, int64_t N, int32_t D, float *dv,
                                            float *dt, float *dw, void *stream) {
  if (!g || !v || !t || !weight_u || !rev_ptr || !rev_u || !rev_w || !dv || !dt || !dw)
    return fail(CHAOREC_E_INVALID, "dualgnn_fuse_bwd: NULL argument");
  if (const int rc = dg_check("dualgnn_fuse_bwd", U, N, 1, D)) return rc;
  if (D == 64)
    hipLaunchKernelGGL(dg_fuse_bwd_kernel<64>, dim3((unsigned)((N + 15) / 16)), dim3(UG_THREADS), 0, (hipStream_t)stream, g, v, t, weight_u,
                       rev_ptr, rev_u, rev_w, U, N, dv, dt, dw);
  else
    hipLaunchKernelGGL(dg_fuse_bwd_kernel<128>, dim3((unsigned)((N + 7) / 8)), dim3(UG_THREADS), 0, (hipStream_t)stream, g, v, t, weight_u,
                       rev_ptr, rev_u, rev_w, U, N, dv, dt, dw);
  return check_launch("dg_fuse_bwd_kernel");
}

static int cf_check(const char *what, int64_t U, int64_t N, int32_t k, int32_t D) {
  if (U <= 0 || U > chaorec_usergraph_max_users() || N < U || N > 2 * chaorec_usergraph_max_users() || k < 1 || D != CF_D)
    return fail(CHAOREC_E_INVALID, "%s: U=%lld N=%lld k=%d D=%d (1 <= U <= N, k >= 1, D is 64)", what, (long long)U, (long long)N,
                (int)k, (int)D);
  return CHAOREC_OK;
}

extern "C" int chaorec_cohesion_fuse_fwd_f32(const float *idr, const float *v, const float *t, const float *h_id, const float *h_v,
                                             const float *h_t, const int32_t *epoch_idx, const float *epoch_w, int64_t U, int64_t N,
                                             int32_t k, int32_t D, float *result, void *stream) {
  if (!idr || !v || !t || !epoch_idx || !epoch_w || !result) return fail(CHAOREC_E_INVALID, "cohesion_fuse_fwd: NULL argument");
  if ((h_id != nullptr) != (h_v != nullptr) || (h_id != nullptr) != (h_t != nullptr))
    return fail(CHAOREC_E_INVALID, "cohesion_fuse_fwd: h_id, h_v, h_t are given together or not at all");
  if (const int rc = cf_check("cohesion_fuse_fwd", U, N, k, D)) return rc;
  hipLaunchKernelGGL(cf_fuse_fwd_kernel, dim3((unsigned)((N + 15) / 16)), dim3(UG_THREADS), 0, (hipStream_t)stream, idr, v, t, h_id, h_v,
                     h_t, epoch_idx, epoch_w, U, N, (int)k, result);
  return check_launch("cf_fuse_fwd_kernel");
}

extern "C" int chaorec_cohesion_fuse_bwd_f32(const float *g, const int64_t *rev_ptr, const int32_t *rev_u, const float *rev_w,
                                             const int32_t *chunk_row, const int64_t *chunk_first, const int64_t *row_chunk,
                                             int64_t n_chunks, int32_t chunk, int64_t U, int64_t N, int32_t D, float *part, float *dv,
                                             float *dt, float *dh_v, float *dh_t, void *stream) {
  if (!g || !rev_ptr || !rev_u || !rev_w || !row_chunk || !dv || !dt) return fail(CHAOREC_E_INVALID, "cohesion_fuse_bwd: NULL argument");
  if (n_chunks < 0 || chunk < 0 || (n_chunks > 0 && (!chunk_row || !chunk_first || !part)))
    return fail(CHAOREC_E_INVALID, "cohesion_fuse_bwd: n_chunks=%lld chunk=%d (chunk_row, chunk_first and part hold n_chunks entries)",
                (long long)n_chunks, (int)chunk);
  if ((dh_v != nullptr) != (dh_t != nullptr)) return fail(CHAOREC_E_INVALID, "cohesion_fuse_bwd: dh_v and dh_t are given together or not at all");
  if (const int rc = cf_check("cohesion_fuse_bwd", U, N, 1, D)) return rc;
  if (n_chunks > 0) {
    hipLaunchKernelGGL(cf_chunk_kernel, dim3((unsigned)((n_chunks + 7) / 8)), dim3(UG_THREADS), 0, (hipStream_t)stream, g, rev_ptr, rev_u,
                       rev_w, chunk_row, chunk_first, n_chunks, (int64_t)chunk, U, part);
    if (const int rc = check_launch("cf_chunk_kernel")) return rc;
  }
  hipLaunchKernelGGL(cf_rows_kernel, dim3((unsigned)((N + 7) / 8)), dim3(UG_THREADS), 0, (hipStream_t)stream, g, part, row_chunk, n_chunks,
                     U, N, dv, dt, dh_v, dh_t);
  return check_launch("cf_rows_kernel");
}
