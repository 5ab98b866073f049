// The last forward propagate AND the BPR forward + backward of an INNER step of a k-step replay of the fused LightGCN step, in
// one launch (chaorec_amd/optim.py: FusedLightGCNStep, _inner_frontier_mode).  Nothing reads such a step's propagated table
// outside the batch's 3 B rows, so x_L = A x_{L-1} is computed for those rows only, by the launch that reads them: on the
// sports graph (N = 44 147, 317 108 entries, B = 1024) the batch's rows hold 58 k entries of the graph's 317 k, and the dense
// propagate stored 11.3 MB of which the BPR launch read 0.8.
//
// Geometry: ONE workgroup of 256 threads per triple.  Its sixteen 16-lane groups (D = 64: a float4 per lane) share the
// gathers of the triple's three rows, which are walked as ONE run of entries -- user row, positive row, negative row -- in
// rounds of kCH = 16 kK entries: group g gathers entries g kK .. g kK + kK - 1 of the round, all in flight at once, with
// clamped indices and no branch (a slot past the run's end repeats its last entry; nobody adds it), and parks the rounded
// products in an LDS tile.  Then wave w (w < 3; a lane per column) adds row w's slots of the tile in entry order to its
// running sum: the sequential CSR-order sum from +0 with separately rounded product and sum, i.e. spmm_csr_ordered_kernel's
// row, bit for bit.  A round's gathers are requested before the round before it is summed and its (col, val) a round earlier
// still (kPipe; with the gathers after the sum the launch took 17.5 us instead of 15.7 on sports, with kK = 4 15.9:
// profiles/inner_frontier_sports_step.json).
// A triple's three rows hold 57 entries on average: one round.  The longest sports row (624) takes five; a wave per triple
// walking 32 entries a turn would take twenty dependent round trips.
// The rows of x_0 .. x_{L-1} at the batch's rows depend on the ids only and are requested before the first round.  The
// mean rows w x_0 + ... + w x_L (mean_of: the last propagate's epilogue, rounding for rounding) stay in registers, go through
// 768 bytes of LDS to wave 0 for the dot products and the gradient adds, and are parked in `rows` for the ordered launch.
#include "bpr_rows.h"
#include "draws.h"

namespace chaorec {
namespace {

#ifndef CHAOREC_FRONTIER_K
#define CHAOREC_FRONTIER_K 8
#endif
#ifndef CHAOREC_FRONTIER_PIPE
#define CHAOREC_FRONTIER_PIPE 1
#endif
constexpr int kLanes = 16;                  // lanes per group: D = 64, one float4 each
constexpr int kGroups = 16;                 // groups per workgroup
constexpr int kK = CHAOREC_FRONTIER_K;      // entries per group and round
constexpr bool kPipe = CHAOREC_FRONTIER_PIPE != 0;   // a round's gathers are requested before the round before it is summed
constexpr int kCH = kGroups * kK;           // entries per round; the tile is kCH * 256 bytes (kK = 8: 32 KiB, four workgroups per CU)
constexpr int kD = 4 * kLanes;
static_assert(kK >= 1 && kK <= kLanes, "a lane of the group holds one (col, val) of its group's kK");
static_assert(kCH * kD * 4 + 3 * kD * 4 <= 40 * 1024, "four workgroups per CU: 1 024 triples resident on 256 CUs");

struct Batch {                              // the draw's operands (bpr_fwd_bwd_drawn_kernel's)
  const int64_t *edges;
  int64_t n_edges;
  const int64_t *hist_rowptr;
  const int32_t *hist_col;
  int64_t num_user;
  uint32_t num_item;
  uint64_t seed, step;
  const int64_t *step_dev;
  const int64_t *in_users, *in_pos, *in_neg;
  int64_t *out_users, *out_pos, *out_neg;
  const int64_t *perm, *perm_pos;
  int64_t pos_offset;
};

__device__ __forceinline__ int64_t uniform_i64(int64_t v, int src_lane) {
  const int lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffll), src_lane);
  const int hi = __builtin_amdgcn_readlane((int)(v >> 32), src_lane);
  return ((int64_t)hi << 32) | (int64_t)(unsigned int)lo;
}

template <int NT>      // the tables in memory, x_0 .. x_{NT-1}: the mean has NT + 1 terms
__global__ __launch_bounds__(256, 4) void bpr_fwd_bwd_frontier_kernel(
    const MeanSrc M, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const Batch Q, int B, int variant, float reg_weight, float *__restrict__ coef, float *__restrict__ ws, float *g_u,
    float *g_i, int32_t *__restrict__ adam_step, float beta1, float beta2, float *__restrict__ adam_bc, uint32_t *row_bits,
    int64_t bits_item_offset) {
  __shared__ float4 tile[kCH * kLanes];     // the round's products, slot-major: slot s, columns 4 li .. 4 li + 3
  __shared__ float mrow[3][kD];             // the triple's rows of the mean
  const int tid = threadIdx.x, lane = tid & 63, li = tid & (kLanes - 1), grp = tid / kLanes, g0 = lane & ~(kLanes - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;

  // the triple: every wave's lane 0 draws it (the same counters, the same triple; no hand-over), wave 0 writes it out
  int64_t u = 0, p = 0, n = 0;
  if (Q.edges) {
    uint64_t step = Q.step;
    if (Q.step_dev) step += (uint64_t)Q.step_dev[0];
    if (lane == 0) {
      draw_triple(Q.edges, Q.n_edges, Q.hist_rowptr, Q.hist_col, Q.num_user, Q.num_item, Q.seed, step, (uint32_t)b, u, p, n,
                  Q.perm, Q.perm ? Q.perm_pos[0] + Q.pos_offset : 0);
      if (wv == 0) {
        Q.out_users[b] = u;
        Q.out_pos[b] = p;
        Q.out_neg[b] = n;
      }
    }
    u = uniform_i64(u, 0);
    p = uniform_i64(p, 0);
    n = uniform_i64(n, 0);
  } else {
    u = Q.in_users[b];
    p = Q.in_pos[b];
    n = Q.in_neg[b];
  }
  const int64_t r0 = u, r1 = M.item_offset + p, r2 = M.item_offset + n;

  // the rows' extents (lanes 0 .. 5) and, under them, this wave's row of the tables in memory (a lane per column)
  int64_t rp = 0;
  if (lane < 6) rp = rowptr[(lane < 2 ? r0 : lane < 4 ? r1 : r2) + (lane & 1)];
  float t[NT + 1];
  {
    const size_t o = (size_t)(wv == 0 ? r0 : wv == 1 ? r1 : r2) * kD + lane;
#pragma unroll
    for (int i = 0; i < NT; ++i) t[i] = wv < 3 ? M.t[i][o] : 0.f;
  }
  const int64_t e0 = uniform_i64(rp, 0), e1 = uniform_i64(rp, 2), e2 = uniform_i64(rp, 4);
  const int d0 = (int)(uniform_i64(rp, 1) - e0), d1 = (int)(uniform_i64(rp, 3) - e1), d2 = (int)(uniform_i64(rp, 5) - e2);
  const int p1 = d0, p2 = d0 + d1, T = p2 + d2;       // the three rows as one run of T entries
  const int rounds = (T + kCH - 1) / kCH;             // (workgroup-uniform: barriers inside)
  const int my_lo = wv == 0 ? 0 : wv == 1 ? p1 : p2;  // wave w's row in the run
  const int my_hi = wv == 0 ? p1 : wv == 1 ? p2 : T;

  // entry q of the run -> its index in col / val; past the end: the run's last entry (rounds > 0 -> T > 0)
  auto entry = [&](int q) {
    q = min(q, T - 1);
    return q < p1 ? e0 + q : q < p2 ? e1 + (q - p1) : e2 + (q - p2);
  };
  const float4 *__restrict__ x4 = reinterpret_cast<const float4 *>(M.t[NT - 1]);
  const float *tilef = reinterpret_cast<const float *>(tile);
  int c = 0;
  float v = 0.f;
  if (rounds > 0 && li < kK) {
    const int64_t e = entry(grp * kK + li);
    c = col[e];
    v = val[e];
  }
  float acc = 0.f;
  float4 xv[kK];
  auto next_cv = [&](int r, int &cn, float &vn) {     // round r's (col, val), one per lane li < kK of a group
    cn = 0, vn = 0.f;
    if (r < rounds && li < kK) {
      const int64_t e = entry(r * kCH + grp * kK + li);
      cn = col[e];
      vn = val[e];
    }
  };
  auto gather = [&](int cc) {
#pragma unroll
    for (int k = 0; k < kK; ++k) xv[k] = x4[(size_t)__shfl(cc, g0 + k, 64) * kLanes + li];
  };
  int c_next = 0;
  float v_next = 0.f;
  if constexpr (kPipe) {
    if (rounds > 0) gather(c);
    next_cv(1, c_next, v_next);
  }
  for (int r = 0; r < rounds; ++r) {
    if constexpr (!kPipe) {
      next_cv(r + 1, c_next, v_next);
      gather(c);
    }
#pragma unroll
    for (int k = 0; k < kK; ++k) tile[(grp * kK + k) * kLanes + li] = mul_rn4(__shfl(v, g0 + k, 64), xv[k]);
    c = c_next;
    v = v_next;
    if constexpr (kPipe) {                 // the next round's gathers fly under this round's sum, the one after's (col, val) behind them
      if (r + 1 < rounds) gather(c);
      next_cv(r + 2, c_next, v_next);
    }
    __syncthreads();
    if (wv < 3) {
      const int s0 = max(my_lo - r * kCH, 0), s1 = min(my_hi - r * kCH, kCH);
#pragma unroll 8
      for (int s = s0; s < s1; ++s) acc = add_rn(acc, tilef[s * kD + lane]);
    }
    if (r + 1 < rounds) __syncthreads();   // (the next round rewrites the tile)
  }

  if (wv < 3) {
    t[NT] = acc;
    const float m = mean_of<NT + 1>(M.w, t);
    mrow[wv][lane] = m;
    M.rows[((size_t)3 * b + wv) * kD + lane] = m;
  }
  __syncthreads();
  // the optimizer's step count and this step's bias corrections: two double pow()s, on a wave that has nothing left to do
  if (wv == 3 && b == 0 && lane == 0 && adam_step) adam_step_on(adam_step, beta1, beta2, adam_bc);
  if (wv != 0) return;
  const float mu = mrow[0][lane], mp = mrow[1][lane], mn = mrow[2][lane];
  const float cf = bpr_terms_wave_of([&](int, float &uu, float &pp, float &nn) { uu = mu, pp = mp, nn = mn; }, b, B, kD, variant,
                                     coef, ws) * 1.0f;
  const float reg2 = 1.0f * 2.0f * reg_weight / ((float)B * (float)kD);
  if (g_u)                                 // (NULL: the ordered launch that follows adds the rows -- CHAOREC_BPR_ORDERED=2)
    bpr_grad_adds(g_u, g_i, (size_t)u * kD + lane, (size_t)p * kD + lane, (size_t)n * kD + lane, cf, reg2, mu, mp, mn);
  flag_triple_rows(row_bits, bits_item_offset, lane, u, p, n);
}

}  // namespace
}  // namespace chaorec

using namespace chaorec;

extern "C" int64_t chaorec_bpr_frontier_round_entries(void) { return kCH; }

extern "C" int chaorec_bpr_fwd_bwd_frontier_f32(const float *const *tabs, int32_t n_tabs, float w, int64_t item_offset, float *rows,
                                                const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                                                int32_t mode, const int64_t *edges, int64_t n_edges,
                                                const int64_t *hist_rowptr, const int32_t *hist_col, int64_t num_user,
                                                int32_t num_item, uint64_t seed, uint64_t step, const int64_t *step_dev,
                                                const int64_t *in_users, const int64_t *in_pos, const int64_t *in_neg, int32_t B,
                                                int32_t D, int32_t variant, float reg_weight, int64_t *out_users,
                                                int64_t *out_pos, int64_t *out_neg, float *coef, float *workspace,
                                                const int64_t *perm, const int64_t *perm_pos, int64_t pos_offset, float *g_u,
                                                float *g_i, int32_t *adam_step, float beta1, float beta2, float *adam_bc,
                                                uint32_t *row_bits, int64_t bits_item_offset, void *stream) {
  const char *who = "bpr_fwd_bwd_frontier";
  if (D != kD) return fail(CHAOREC_E_INVALID, "%s: built for D = %d (D=%d)", who, kD, D);
  if (!tabs || n_tabs < 1 || n_tabs > kMeanMaxTabs - 1)
    return fail(CHAOREC_E_INVALID, "%s: %d layer tables in memory (1 .. %d)", who, n_tabs, kMeanMaxTabs - 1);
  if (!rows || item_offset < 0) return fail(CHAOREC_E_INVALID, "%s: NULL rows buffer or a negative item offset", who);
  if (!rowptr || !col || !val || n_rows <= 0) return fail(CHAOREC_E_INVALID, "%s: NULL graph arrays or no rows", who);
  if (mode != 0) return fail(CHAOREC_E_INVALID, "%s: a graph with dynamic values (mode %d) is not built", who, mode);
  MeanSrc M;
  for (int k = 0; k < kMeanMaxTabs; ++k) {
    M.t[k] = k < n_tabs ? tabs[k] : nullptr;
    if (k < n_tabs && !tabs[k]) return fail(CHAOREC_E_INVALID, "%s: NULL table %d", who, k);
  }
  if ((uintptr_t)tabs[n_tabs - 1] & 15u) return fail(CHAOREC_E_INVALID, "%s: the gathered table must be 16-byte aligned", who);
  M.n = n_tabs + 1, M.w = w, M.item_offset = item_offset, M.rows = rows;
  if (int rc = bpr_fwd_bwd_check(who, coef, workspace, g_u, g_i, edges, n_edges, hist_rowptr, num_item, in_users, in_pos, in_neg,
                                 out_users, out_pos, out_neg, perm, perm_pos, pos_offset, adam_step, adam_bc, B, D, variant))
    return rc;
  const bool ordered = bpr_ordered_after_fused(B, D);
  const Batch Q{edges,    n_edges, hist_rowptr, hist_col, num_user, (uint32_t)num_item, seed, step,     step_dev,
                in_users, in_pos,  in_neg,      out_users, out_pos, out_neg,            perm, perm_pos, pos_offset};
#define CHAOREC_FRONTIER_LAUNCH(NT)                                                                                          \
  hipLaunchKernelGGL(bpr_fwd_bwd_frontier_kernel<NT>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, M, rowptr, col, val, \
                     Q, B, variant, reg_weight, coef, workspace, ordered ? (float *)nullptr : g_u, g_i, adam_step, beta1, beta2, \
                     adam_bc, row_bits, bits_item_offset)
  static_assert(kMeanMaxTabs == 4, "one instantiation per table count below");
  if (n_tabs == 1) CHAOREC_FRONTIER_LAUNCH(1);
  else if (n_tabs == 2) CHAOREC_FRONTIER_LAUNCH(2);
  else CHAOREC_FRONTIER_LAUNCH(3);
#undef CHAOREC_FRONTIER_LAUNCH
  int rc = check_launch("bpr_fwd_bwd_frontier_kernel");
  if (rc || !ordered) return rc;
  return bpr_bwd_ordered(nullptr, nullptr, rows, edges ? out_users : in_users, edges ? out_pos : in_pos,
                         edges ? out_neg : in_neg, B, D, coef, reg_weight, nullptr, g_u, g_i, stream);
}
