// Rank lists past 64 columns: the exact scores of a user range staged in HBM, then the exact top-k of every staged row.
//
// Replaces gene_ranklist's torch.matmul + python mask loop + torch.topk (Model/LightGCN.py:147-155, Model/FREEDOM.py:230-238,
// Model/MMGCN.py:220-230) for 64 < topk <= 1024, where score_topk.hip's candidate lists (64 keys per lane, 128-key register
// sorts) end.
//
//  (a) score_rows_kernel   the geometry of score_topk_f32_kernel -- one wave64 = 32 users x a stream of 32-item tiles on
//                          v_mfma_f32_32x32x2_f32, items the A rows, users the B columns, so a lane holds ONE user's 16
//                          scores of the tile -- with the accumulator stored instead of selected from.  Same operands in the
//                          same k order, so a score has the bits the narrow routes rank (oracle_score_dot).  Registers 4g ..
//                          4g + 3 of a lane are four consecutive items of its user's row: one 16-byte store where the row
//                          allows it.  The launch is bound by the f32 MFMA chain (2 U I D flops at the vector rate), the
//                          stores are a few GB/s beside it: they are not staged through LDS.
//  (b) rows_topk_wide_kernel  one workgroup per row.  mc_topk_kernel's 4-bit radix search for the k-th largest key (8 counting
//                          passes over the L2-resident row), an ordered compaction of the k winners by block-wide prefix sums
//                          (every key above the k-th, then keys equal to it in ascending index order), a bitonic sort in LDS
//                          of up to 1024 64-bit (key << 32 | ~index) entries, padded with 0 -- below every entry -- up to a
//                          power of two.  No atomics, no scratch: the same bits on every run.
#include "common.h"

namespace chaorec {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWideK = 1024;

__device__ __forceinline__ uint32_t wide_order_key(float x) {      // ascending with the float order (mc_order_key, f32_to_ord)
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float wide_key_value(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

struct RowsArgs {
  const float *user_emb;       // [n_users, D]
  const float *item_emb;       // [n_items, D]
  int64_t n_items;
  int Dk;                      // run-time K-dim of the streamed variant
  int64_t user_begin, n;       // the range
  const int64_t *hist_rowptr;
  const int32_t *hist_col;
  float mask_value;
  float *scores;               // [n, ld]
  int64_t ld;
  int tiles_per_split;
  int vec4;                    // rows 16-byte aligned: ld % 4 == 0 and the base is
};

// D > 0: the users' fragment lives in registers for the whole stream; D == 0: K-dim = Dk at run time (a multiple of 64), both
// operands re-read per 64-wide chunk -- the two variants of score_topk_f32_kernel, chain for chain.
template <int D>
__global__ __launch_bounds__(64) void score_rows_kernel(const RowsArgs A) {
  const int lane = threadIdx.x;
  const int ur = lane & 31;
  const int h = lane >> 5;
  const int64_t r = (int64_t)blockIdx.x * 32 + ur;      // row of the staging block
  const bool u_ok = r < A.n;
  const int64_t u = A.user_begin + (u_ok ? r : 0);      // row of the tables
  const uint32_t n_items = (uint32_t)A.n_items;
  const int n_tiles = (int)((A.n_items + 31) / 32);
  const int t_begin = (int)blockIdx.y * A.tiles_per_split;
  const int t_end = min(n_tiles, t_begin + A.tiles_per_split);

  constexpr int DR = D > 0 ? D : 64;
  float bu[DR / 2];      // users' B fragment: lane (ur, h) holds k = h*D/2 + s
  if (D > 0) {
    if (u_ok) {
      const float4 *src = reinterpret_cast<const float4 *>(A.user_emb + (size_t)u * DR + h * (DR / 2));
#pragma unroll
      for (int q = 0; q < DR / 8; ++q) {
        const float4 v = src[q];
        bu[4 * q + 0] = v.x;
        bu[4 * q + 1] = v.y;
        bu[4 * q + 2] = v.z;
        bu[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int s = 0; s < DR / 2; ++s) bu[s] = 0.f;
    }
  }

  // history cursor: first interacted item >= first item of the range
  int64_t hp = 0, hend = 0;
  uint32_t hnext = 0xFFFFFFFFu;
  if (A.hist_rowptr && u_ok) {
    int64_t lo = A.hist_rowptr[u];
    hend = A.hist_rowptr[u + 1];
    int64_t hi = hend;
    const uint32_t first = (uint32_t)t_begin * 32u;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((uint32_t)A.hist_col[mid] < first) lo = mid + 1; else hi = mid;
    }
    hp = lo;
    if (hp < hend) hnext = (uint32_t)A.hist_col[hp];
  }
  float *out = A.scores + (size_t)(u_ok ? r : 0) * A.ld;

  auto store = [&](f32x16 &acc, int t) {
    const uint32_t j0 = (uint32_t)t * 32u;
    uint32_t mbits = 0;
    while (hnext < j0 + 32u) {
      if (hnext >= j0) mbits |= 1u << (hnext - j0);
      ++hp;
      hnext = hp < hend ? (uint32_t)A.hist_col[hp] : 0xFFFFFFFFu;
    }
    if (__any(mbits != 0)) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int off = (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if ((mbits >> off) & 1u) acc[reg] = A.mask_value;
      }
    }
    if (!u_ok) return;
    if (A.vec4 && j0 + 32u <= n_items) {
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4 *>(out + j0 + 8 * g + 4 * h) = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
    } else {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const uint32_t j = j0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (j < n_items) out[j] = acc[reg];
      }
    }
  };

  auto load_items = [&](float (&a)[DR / 2], int t) {      // lane (r, h): D/2 consecutive floats of item row 32t + r; zero past the table
    const int64_t j = (int64_t)t * 32 + ur;
    if (j < A.n_items) {
      const float4 *src = reinterpret_cast<const float4 *>(A.item_emb + (size_t)j * DR + h * (DR / 2));
#pragma unroll
      for (int q = 0; q < DR / 8; ++q) {
        const float4 v = src[q];
        a[4 * q + 0] = v.x;
        a[4 * q + 1] = v.y;
        a[4 * q + 2] = v.z;
        a[4 * q + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int s = 0; s < DR / 2; ++s) a[s] = 0.f;
    }
  };

  if (D > 0) {
    float a0[DR / 2], a1[DR / 2];      // the next tile's fragment is loaded ahead of the 32*D MFMA cycles of this one
    int t = t_begin;
    if (t < t_end) load_items(a0, t);
    while (t < t_end) {
      {
        load_items(a1, t + 1 < t_end ? t + 1 : t);
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int s = 0; s < DR / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], bu[s], acc, 0, 0, 0);
        store(acc, t);
        ++t;
      }
      if (t >= t_end) break;
      {
        load_items(a0, t + 1 < t_end ? t + 1 : t);
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int s = 0; s < DR / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], bu[s], acc, 0, 0, 0);
        store(acc, t);
        ++t;
      }
    }
  } else {
    for (int t = t_begin; t < t_end; ++t) {
      const int64_t j = (int64_t)t * 32 + ur;
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      for (int kc = 0; kc < A.Dk; kc += 64) {
        float4 av[8], bv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          av[q] = make_float4(0.f, 0.f, 0.f, 0.f);
          bv[q] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (j < A.n_items) av[q] = reinterpret_cast<const float4 *>(A.item_emb + (size_t)j * A.Dk + kc + h * 32)[q];
          if (u_ok) bv[q] = reinterpret_cast<const float4 *>(A.user_emb + (size_t)u * A.Dk + kc + h * 32)[q];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].x, bv[q].x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].y, bv[q].y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].z, bv[q].z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q].w, bv[q].w, acc, 0, 0, 0);
        }
      }
      store(acc, t);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// exact top-K of a row, 64 < K <= min(1024, I).  The row is read 10 times (8 counting passes, the count above the K-th key,
// the compaction), each counting pass with 15 compare-adds per element, as in mc_topk_kernel; its 64 x 64 rank-by-counting
// sort does not scale to 1024 entries, the bitonic network below is log2(P) (log2(P) + 1) / 2 <= 55 steps of P / 2 compare-
// exchanges over the workgroup.
// ---------------------------------------------------------------------------------------------------------------
// f(key) for every element of the row this thread owns (t, t + 256, ...), eight independent loads in flight: the counting
// passes are chains of L2 round trips otherwise (the order of the calls does not matter to a count)
template <class F>
__device__ __forceinline__ void for_each_key(const float *__restrict__ x, int64_t I, int t, F f) {
  int64_t e = t;
  for (; e + 7 * 256 < I; e += 8 * 256) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = x[e + i * 256];
#pragma unroll
    for (int i = 0; i < 8; ++i) f(wide_order_key(v[i]));
  }
  for (; e < I; e += 256) f(wide_order_key(x[e]));
}

__global__ __launch_bounds__(256) void rows_topk_wide_kernel(const float *__restrict__ scores, int64_t I, int64_t ld, int K, int64_t id_offset,
                                                             int64_t *__restrict__ idx_out, float *__restrict__ val_out) {
  __shared__ uint64_t sel[kWideK];
  __shared__ int cnt[4][16];
  __shared__ int wtot[4][2];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t row = blockIdx.x;
  const float *x = scores + row * ld;
  uint32_t prefix = 0;      // invariant: at least K keys are >= prefix
  for (int shift = 28; shift >= 0; shift -= 4) {
    int c[15];
#pragma unroll
    for (int j = 0; j < 15; ++j) c[j] = 0;
    for_each_key(x, I, t, [&](uint32_t key) {
      const uint32_t dg = key >= prefix ? min((key - prefix) >> shift, 15u) : 0u;
#pragma unroll
      for (int j = 0; j < 15; ++j) c[j] += dg >= (uint32_t)(j + 1) ? 1 : 0;
    });
#pragma unroll
    for (int j = 0; j < 15; ++j) {
      int v = c[j];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) cnt[wave][j] = v;
    }
    __syncthreads();
    uint32_t best = 0;
#pragma unroll
    for (int j = 0; j < 15; ++j)
      if (cnt[0][j] + cnt[1][j] + cnt[2][j] + cnt[3][j] >= K) best = j + 1;      // (the counts fall with j)
    prefix += best << shift;
    __syncthreads();
  }
  const uint32_t T = prefix;      // the K-th largest key
  int n_gt = 0;
  for_each_key(x, I, t, [&](uint32_t key) { n_gt += key > T ? 1 : 0; });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n_gt += __shfl_xor(n_gt, off, 64);
  if (lane == 0) cnt[wave][0] = n_gt;
  __syncthreads();
  n_gt = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0];      // < K: T is itself one of the K largest
  const int need_eq = K - n_gt;
  int P = 128;      // entries the sort runs over
  while (P < K) P <<= 1;
  for (int i = K + t; i < P; i += 256) sel[i] = 0ull;      // (an entry is never 0: its index is below 2^31)
  int run_gt = 0, run_eq = 0;
  float ahead = t < I ? x[t] : 0.f;      // the next chunk's element is loaded while this one's barriers pass
  for (int64_t base = 0; base < I && (run_gt < n_gt || run_eq < need_eq); base += 256) {
    const int64_t e = base + t;
    const uint32_t key = e < I ? wide_order_key(ahead) : 0u;
    if (e + 256 < I) ahead = x[e + 256];
    const bool gt = e < I && key > T, eq = e < I && key == T;
    const unsigned long long bg = __ballot(gt), be = __ballot(eq);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    __syncthreads();                                   // the previous chunk's readers of wtot are done
    if (lane == 0) {
      wtot[wave][0] = __popcll(bg);
      wtot[wave][1] = __popcll(be);
    }
    __syncthreads();
    int pg = run_gt + __popcll(bg & below), pe = run_eq + __popcll(be & below);
    for (int w = 0; w < 4; ++w) {
      if (w < wave) {
        pg += wtot[w][0];
        pe += wtot[w][1];
      }
      run_gt += wtot[w][0];
      run_eq += wtot[w][1];
    }
    const uint64_t entry = ((uint64_t)key << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)e);
    if (gt && pg < n_gt) sel[pg] = entry;
    else if (eq && pe < need_eq) sel[n_gt + pe] = entry;
  }
  __syncthreads();
  // descending bitonic sort of sel[0 .. P): pair (i, i | j) of block i & k
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = t; p < P / 2; p += 256) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));      // p with a 0 inserted at bit log2(j)
        const int q = i | j;
        const uint64_t a = sel[i], b = sel[q];
        const bool desc = (i & k) == 0;
        if ((a < b) == desc) {
          sel[i] = b;
          sel[q] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int r = t; r < K; r += 256) {
    const uint64_t e = sel[r];
    idx_out[row * K + r] = (int64_t)(0xFFFFFFFFu - (uint32_t)(e & 0xFFFFFFFFull)) + id_offset;
    val_out[row * K + r] = wide_key_value((uint32_t)(e >> 32));
  }
}

template <int D>
static void launch_rows(const RowsArgs &a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(score_rows_kernel<D>, grid, dim3(64), 0, st, a);
}

}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_score_rows_f32(const float *user_emb, const float *item_emb, int64_t n_users, int64_t n_items, int32_t D,
                                      int64_t user_begin, int64_t n, const int64_t *hist_rowptr, const int32_t *hist_col,
                                      float mask_value, float *scores, int64_t ld, size_t scores_bytes, void *stream) {
  if (!user_emb || !item_emb || !scores) return fail(CHAOREC_E_INVALID, "score_rows: NULL argument");
  if (n_users <= 0 || n_items <= 0 || n_items > 0x7FFFFFE0ll) return fail(CHAOREC_E_INVALID, "score_rows: bad sizes");
  if (user_begin < 0 || n <= 0 || n > n_users - user_begin)
    return fail(CHAOREC_E_INVALID, "score_rows: users %lld .. +%lld outside [0, %lld)", (long long)user_begin, (long long)n, (long long)n_users);
  if (ld < n_items) return fail(CHAOREC_E_INVALID, "score_rows: ld=%lld < n_items=%lld", (long long)ld, (long long)n_items);
  if ((size_t)n * (size_t)ld * sizeof(float) > scores_bytes)
    return fail(CHAOREC_E_WORKSPACE, "score_rows: staging block %zu < %zu (rank in user ranges)", scores_bytes, (size_t)n * (size_t)ld * sizeof(float));
  if (hist_rowptr && !hist_col) return fail(CHAOREC_E_INVALID, "score_rows: hist_rowptr without hist_col");
  if (!((D == 8 || D == 16 || D == 32 || D == 64 || D == 128) || (D > 128 && D % 64 == 0)))
    return fail(CHAOREC_E_INVALID, "score_rows: D=%d not in {8,16,32,64,128} and not a multiple of 64 above 128", D);
  RowsArgs a;
  a.user_emb = user_emb;
  a.item_emb = item_emb;
  a.n_items = n_items;
  a.Dk = D;
  a.user_begin = user_begin;
  a.n = n;
  a.hist_rowptr = hist_rowptr;
  a.hist_col = hist_col;
  a.mask_value = mask_value;
  a.scores = scores;
  a.ld = ld;
  a.vec4 = (ld % 4 == 0 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0) ? 1 : 0;
  // item splits: the waves of a range should fill the chip several times over (256 CUs x 4 SIMDs); a split is at least 8
  // tiles, so the user fragment's load and the history search are amortised
  const int64_t groups = (n + 31) / 32, n_tiles = (n_items + 31) / 32;
  int64_t splits = (8192 + groups - 1) / groups;
  if (splits > (n_tiles + 7) / 8) splits = (n_tiles + 7) / 8;
  if (splits < 1) splits = 1;
  if (splits > 65535) splits = 65535;
  a.tiles_per_split = (int)((n_tiles + splits - 1) / splits);
  splits = (n_tiles + a.tiles_per_split - 1) / a.tiles_per_split;
  if (groups > 0x7FFFFFFFll) return fail(CHAOREC_E_INVALID, "score_rows: n=%lld too large for one launch", (long long)n);
  const dim3 grid((unsigned)groups, (unsigned)splits);
  hipStream_t st = (hipStream_t)stream;
  switch (D) {
    case 8: launch_rows<8>(a, grid, st); break;
    case 16: launch_rows<16>(a, grid, st); break;
    case 32: launch_rows<32>(a, grid, st); break;
    case 64: launch_rows<64>(a, grid, st); break;
    case 128: launch_rows<128>(a, grid, st); break;
    default: launch_rows<0>(a, grid, st); break;
  }
  return check_launch("score_rows_kernel");
}

extern "C" int chaorec_rows_topk_wide_f32(const float *scores, int64_t n_rows, int64_t I, int64_t ld, int32_t topk, int64_t id_offset,
                                          int64_t *idx, float *val, void *stream) {
  if (!scores || !idx || !val) return fail(CHAOREC_E_INVALID, "rows_topk_wide: NULL argument");
  if (n_rows <= 0 || n_rows > 0x7FFFFFFFll || topk <= 64 || topk > kWideK || I < topk || I > 0x7FFFFFFF || ld < I)
    return fail(CHAOREC_E_INVALID, "rows_topk_wide: n_rows=%lld I=%lld ld=%lld topk=%d (64 < topk <= min(%d, I), I <= ld)", (long long)n_rows,
                (long long)I, (long long)ld, (int)topk, kWideK);
  hipLaunchKernelGGL(rows_topk_wide_kernel, dim3((unsigned)n_rows), dim3(256), 0, (hipStream_t)stream, scores, I, ld, (int)topk, id_offset, idx,
                     val);
  return check_launch("rows_topk_wide_kernel");
}
