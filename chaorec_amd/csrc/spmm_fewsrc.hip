// y = alpha * (A x) + beta * z for a source with FEW non-zero rows, every row of y written -- the first backward propagate of a
// LightGCN step over a small graph (train_and_evaluate.py:46 loss.backward() through Model/LightGCN.py:81-83):
// g_{L-1} = w (A G) + w G with G the batch gradient, at most 3 B non-zero rows out of N.  On the sports graph (N = 44 147,
// 317 108 entries, B = 1024) 86 % of the dense launch's gathers fetch rows of exact zeros.
//
// What differs from the gated instantiation of csrc/spmm.hip (chaorec_spmm_csr_rowsparse_f32), which probes the bitmap in
// memory once per entry and stays at ~80 % of the dense launch:
//   * every workgroup first copies the WHOLE source bitmap into LDS ((N + 31) / 32 words; 5.5 KB at sports) -- every bit test
//     after that is an LDS read, not an L2 request;
//   * the 16 lanes of a row's group test DIFFERENT entries at once: lanes 4 .. 9 the six columns that came with the row's
//     descriptor (they hold those dwords already), then every lane one column of each 16-entry block of the remainder, two
//     blocks requested together.  A ballot gives the flagged set; only flagged entries load their value and gather, lowest
//     entry first, four source rows in flight per group;
//   * a row above the long threshold is scanned by the whole workgroup, 256 entries a turn, its flagged entries compacted
//     in entry order into LDS; the 16 groups then share the gathers and the row's owner adds the products in list order.
//
// The result is the dense launch's bit for bit.  A row's sum starts at +0 and takes the flagged entries in ascending entry
// order with separately rounded product and sum (mul_rn4 / add_rn4); a skipped term is val * (+0) = +-0, and adding that to a
// sum that started at +0 changes no bit (finite values).  The epilogue is spmm.hip's, s = alpha * sum, then s + beta * z,
// with +0 standing for an unflagged row of z -- which is what that row holds.
#include "common.h"
#include <algorithm>

namespace chaorec {
namespace {

// The row-descriptor layout of csrc/spmm.hip (kInline, kDescDwords; chaorec_amd/graph.py restates it as K_INLINE,
// DESC_DWORDS): 16 dwords per schedule slot = row (-1: empty), degree | long-workgroup flag (bit 31), first entry lo / hi,
// the first six columns, the first six values.  tests/test_gpu_fewsrc.py compares this kernel with the dense one on rows
// of 6 / 7 entries and on long rows: it fails if the two drift.
constexpr int kInline = 6;
constexpr int kDescDwords = 16;

// Registers (gfx950, -Rpass-analysis=kernel-resource-usage): six waves per SIMD asked for = 80 VGPRs, no scratch, 10.4 KB of
// static LDS; eight = 64 VGPRs with 15 of them spilled (4 spilled with two gathers in flight), seven = 72 with 6 spilled.
// Six it is: a spill store sits on every row's path.
#ifndef CHAOREC_FEWSRC_UNR
#define CHAOREC_FEWSRC_UNR 4
#endif
#ifndef CHAOREC_FEWSRC_MINW
#define CHAOREC_FEWSRC_MINW 6
#endif

constexpr int kLanes = 16;        // lanes per row: D = 64, one float4 each
constexpr int kGroups = 4;        // rows per wave
constexpr int kUnr = CHAOREC_FEWSRC_UNR;          // gathered source rows in flight per group
constexpr int kTurn = 256;        // entries of a long row scanned per turn (one per thread)
constexpr int kTile = 32;         // products of a long row parked in LDS per step (two per group)
constexpr int64_t kMaxBitmapBytes = 48 * 1024;   // the LDS copy of the bitmap (+ ~11 KB of static LDS: under 64 KB)
static_assert(4 + 2 * kInline == kDescDwords && kDescDwords == kLanes, "one descriptor dword per lane of a group");

__device__ __forceinline__ bool bit_of(const uint32_t *bits, int r) { return (bits[r >> 5] >> (r & 31)) & 1u; }

__global__ __launch_bounds__(256, CHAOREC_FEWSRC_MINW) void spmm_fewsrc_kernel(const int32_t *__restrict__ col, const float *__restrict__ val,
                                                             const float *x, float *__restrict__ y, float alpha,
                                                             const float *z, float beta, const uint32_t *__restrict__ src_bits,
                                                             const uint32_t *z_bits, int n_words,
                                                             const int32_t *__restrict__ sched, int64_t n_sched_blocks,
                                                             int long_t) {
  extern __shared__ uint32_t bits_s[];                  // the source bitmap
  __shared__ float4 tile[kTile * kLanes];               // a long row's products, list order
  __shared__ int lc[kTurn];                             // a long row's flagged entries of this turn: columns ..
  __shared__ float lv[kTurn];                           // .. and values
  __shared__ long long long_e0[4 * kGroups];
  __shared__ int long_n[4 * kGroups];
  __shared__ int wcnt[4];
  __shared__ int n_long_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, sub = lane / kLanes, li = lane % kLanes;
  const int g0 = sub * kLanes;                          // first lane of this row's group
  const int grp = tid / kLanes;                         // group within the workgroup (long rows)
  const float4 *x4 = reinterpret_cast<const float4 *>(x);
  const float4 *z4 = reinterpret_cast<const float4 *>(z);
  float4 *y4 = reinterpret_cast<float4 *>(y);
  const bool z_lds = z_bits == src_bits;                // (kernel-uniform: the step's launch, one bitmap for both)

  // one descriptor dword per lane; the first block's travel with the bitmap copy
  auto desc = [&](int64_t sb) { return sched[((size_t)(sb * 4 + wv) * kGroups + sub) * kDescDwords + li]; };
  int64_t sb = blockIdx.x;
  int dws = desc(sb);
  for (int i = tid; i < n_words; i += 256) bits_s[i] = src_bits[i];
  __syncthreads();

  for (; sb < n_sched_blocks; sb += gridDim.x) {        // (block-uniform trip count: barriers inside)
    const int64_t sb_next = sb + gridDim.x;
    const int dws_next = sb_next < n_sched_blocks ? desc(sb_next) : 0;
    const int r = __shfl(dws, g0, 64);
    const int d1 = __shfl(dws, g0 + 1, 64);
    const int64_t e0 = ((int64_t)__shfl(dws, g0 + 3, 64) << 32) | (int64_t)(unsigned int)__shfl(dws, g0 + 2, 64);
    const int deg = d1 & 0x7fffffff;
    const bool blk_long = d1 < 0;                       // block-uniform: the host sets it on all descriptors of a workgroup
    const bool row_ok = r >= 0;
    const bool is_long = deg > long_t;
    const int deg1 = is_long ? 0 : deg;
    const int rest = max(deg1 - kInline, 0);            // entries to be fetched from the CSR arrays
    const int64_t e0r = e0 + kInline;
    int dmax = __builtin_amdgcn_readlane(rest, 0);      // wave-uniform trip counts keep every shuffle fully active
#pragma unroll
    for (int g = 1; g < kGroups; ++g) dmax = max(dmax, __builtin_amdgcn_readlane(rest, g * kLanes));

    // two column blocks of the remainder, requested before anything is tested
    int c0 = 0, c1 = 0;
    auto load_cols = [&](int base) {
      c0 = c1 = 0;
      if (base + li < rest) c0 = col[e0r + base + li];
      if (base + kLanes + li < rest) c1 = col[e0r + base + kLanes + li];
    };
    load_cols(0);

    bool zflag = false;
    if (z && row_ok) zflag = z_lds ? bit_of(bits_s, r) : bit_of(z_bits, r);
    float4 zrow = make_float4(0.f, 0.f, 0.f, 0.f);
    if (zflag) zrow = z4[(size_t)r * kLanes + li];

    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
    // The flagged entries of one block (a lane each: column c, value v in lane + voff), lowest first, kUnr gathers in flight.
    auto walk = [&](int c, float v, int voff, unsigned long long bal) {
      uint32_t gm = (uint32_t)(bal >> g0) & 0xffffu;
      int jmax = 0;
#pragma unroll
      for (int g = 0; g < kGroups; ++g) jmax = max(jmax, (int)__popc((uint32_t)(bal >> (g * kLanes)) & 0xffffu));
      for (int j = 0; j < jmax; j += kUnr) {
        int src[kUnr];
        bool p[kUnr];
        float4 xv[kUnr];
#pragma unroll
        for (int u = 0; u < kUnr; ++u) {
          p[u] = gm != 0;
          src[u] = g0 + (p[u] ? (int)__builtin_ctz(gm) : 0);
          gm &= gm - 1;                                 // (0 stays 0)
          const int cj = __shfl(c, src[u], 64);
          xv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (p[u]) xv[u] = x4[(size_t)cj * kLanes + li];
        }
#pragma unroll
        for (int u = 0; u < kUnr; ++u) {
          const float vj = __shfl(v, src[u] + voff, 64);
          if (p[u]) sum = add_rn4(sum, mul_rn4(vj, xv[u]));
        }
      }
    };

    // the entries that came with the descriptor: lane 4 + j holds column j, lane 10 + j its value
    {
      const int j = li - 4;
      const bool f = row_ok && j >= 0 && j < kInline && j < deg1 && bit_of(bits_s, dws);
      const unsigned long long bal = __ballot(f);
      if (bal) walk(dws, __int_as_float(dws), kInline, bal);
    }
    // the rest of a short row
    for (int base = 0; base < dmax; base += 2 * kLanes) {
      if (base) load_cols(base);
      const bool f0 = base + li < rest && bit_of(bits_s, c0);
      const bool f1 = base + kLanes + li < rest && bit_of(bits_s, c1);
      float v0 = 0.f, v1 = 0.f;
      if (f0) v0 = val[e0r + base + li];
      if (f1) v1 = val[e0r + base + kLanes + li];
      const unsigned long long b0 = __ballot(f0), b1 = __ballot(f1);
      if (b0) walk(c0, v0, 0, b0);
      if (b1) walk(c1, v1, 0, b1);
    }

    // long rows, one at a time, by the whole workgroup
    if (blk_long) {
      if (tid == 0) n_long_s = 0;
      __syncthreads();
      int my_slot = -1;
      if (row_ok && is_long && li == 0) {
        my_slot = atomicAdd(&n_long_s, 1);
        long_e0[my_slot] = e0;
        long_n[my_slot] = deg;
      }
      my_slot = __shfl(my_slot, g0, 64);
      __syncthreads();
      const int nl = n_long_s;
      for (int t = 0; t < nl; ++t) {
        const int n = long_n[t];
        const int64_t le0 = long_e0[t];
        for (int t0 = 0; t0 < n; t0 += kTurn) {
          // one coalesced pass over this turn's (col, val), the flagged ones compacted in entry order
          const int e = t0 + tid;
          int ce = 0;
          float ve = 0.f;
          if (e < n) {
            ce = col[le0 + e];
            ve = val[le0 + e];
          }
          const bool fe = e < n && bit_of(bits_s, ce);
          const unsigned long long bm = __ballot(fe);
          if (lane == 0) wcnt[wv] = (int)__popcll(bm);
          __syncthreads();
          int total = 0, mybase = 0;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            if (w == wv) mybase = total;
            total += wcnt[w];
          }
          if (fe) {
            const int pos = mybase + (int)__popcll(bm & ((1ull << lane) - 1ull));
            lc[pos] = ce;
            lv[pos] = ve;
          }
          __syncthreads();
          // every group gathers two entries of the list per step; the owner adds the products in list order
          for (int k0 = 0; k0 < total; k0 += kTile) {
#pragma unroll
            for (int u = 0; u < kTile / 16; ++u) {
              const int slot = u * 16 + grp;
              if (k0 + slot < total)
                tile[slot * kLanes + li] = mul_rn4(lv[k0 + slot], x4[(size_t)lc[k0 + slot] * kLanes + li]);
            }
            __syncthreads();
            if (my_slot == t) {
              const int cnt = min(kTile, total - k0);
              for (int q = 0; q < cnt; ++q) sum = add_rn4(sum, tile[q * kLanes + li]);
            }
            __syncthreads();
          }
        }
      }
    }

    if (row_ok) {
      float4 s = mul_rn4(alpha, sum);
      if (z) s = add_rn4(s, mul_rn4(beta, zrow));
      y4[(size_t)r * kLanes + li] = s;
    }
    dws = dws_next;
  }
}

}  // namespace
}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_spmm_csr_fewsrc_f32(const int32_t *col, const float *val, const float *x, float *y, int64_t n_rows,
                                           int64_t n_cols, int32_t D, float alpha, const float *z, float beta,
                                           const int32_t *schedule, const uint32_t *src_bits, const uint32_t *z_bits,
                                           void *stream) {
  if (!col || !val || !x || !y || !schedule || !src_bits) return fail(CHAOREC_E_INVALID, "spmm (few sources): NULL argument");
  if ((z != nullptr) != (z_bits != nullptr)) return fail(CHAOREC_E_INVALID, "spmm (few sources): z and z_bits come together");
  if (D != 4 * kLanes) return fail(CHAOREC_E_INVALID, "spmm (few sources): built for D = 64 (D=%d)", D);
  if (n_rows < 0 || n_rows != n_cols) return fail(CHAOREC_E_INVALID, "spmm (few sources): a square graph, one bitmap over its rows");
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)z) & 15u) return fail(CHAOREC_E_INVALID, "spmm (few sources): x / y / z must be 16-byte aligned");
  if (x == y) return fail(CHAOREC_E_INVALID, "spmm (few sources): y is gathered from while it is written");
  const int64_t n_words = (n_cols + 31) / 32;
  if (n_words * 4 > kMaxBitmapBytes)
    return fail(CHAOREC_E_INVALID, "spmm (few sources): the bitmap of %lld rows exceeds the LDS budget of %lld bytes",
                (long long)n_rows, (long long)kMaxBitmapBytes);
  if (n_rows == 0) return CHAOREC_OK;
  const int64_t waves = (n_rows + kGroups - 1) / kGroups;
  const int64_t sched_blocks = (waves + 3) / 4;         // the schedule has exactly 4 * sched_blocks wave slots
  // as many workgroups as are resident at once (one wave per SIMD each: CHAOREC_FEWSRC_MINW per CU by registers, fewer by LDS), each taking an equal share of the schedule's
  // blocks: the bitmap is copied once per workgroup, not once per 16 rows
  static int cus = 0;
  if (cus <= 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      return fail(CHAOREC_E_LAUNCH, "spmm (few sources): no device");
    cus = n;
  }
  const int64_t lds = n_words * 4 + 12 * 1024;
  const int64_t per_cu = std::min<int64_t>(CHAOREC_FEWSRC_MINW, std::max<int64_t>(1, (160 * 1024) / lds));
  const int64_t cap = (int64_t)cus * per_cu;
  const int64_t iters = (sched_blocks + cap - 1) / cap;
  const int64_t grid = (sched_blocks + iters - 1) / iters;
  hipLaunchKernelGGL(spmm_fewsrc_kernel, dim3((unsigned)grid), dim3(256), (size_t)(n_words * 4), (hipStream_t)stream, col, val, x,
                     y, alpha, z, beta, src_bits, z_bits, (int)n_words, schedule, sched_blocks, chaorec_spmm_long_threshold());
  return check_launch("spmm_fewsrc_kernel");
}
