// What the BPR launches over table rows share (csrc/bpr.hip, csrc/bpr_frontier.hip): the wave that reduces one triple, the
// layer-mean row source, R0's bits, the argument checks of the fused forward + backward launches and the ordered gradient
// launch that may follow them.  One definition of every rounding: the launches are compared bit for bit.
#pragma once
#include "common.h"

namespace chaorec {

// the wave of triple b: five wave butterflies over the three rows' elements -- rows(k, u, p, n) yields element k of the user /
// positive / negative row --, lane 0 writes the term / coefficient / L2 parts
template <class Rows>
__device__ __forceinline__ float bpr_terms_wave_of(Rows &&rows, int b, int B, int D, int variant, float *__restrict__ coef,
                                                   float *__restrict__ ws) {
  const int lane = threadIdx.x & 63;
  float sp = 0.f, sn = 0.f, ru = 0.f, rp = 0.f, rn = 0.f;
  for (int k = lane; k < D; k += 64) {
    float u, p, n;
    rows(k, u, p, n);
    sp += u * p;
    sn += u * n;
    ru += u * u;
    rp += p * p;
    rn += n * n;
  }
  sp = wave_sum(sp);
  sn = wave_sum(sn);
  ru = wave_sum(ru);
  rp = wave_sum(rp);
  rn = wave_sum(rn);
  float c = 0.f;
  if (lane == 0) {
    const float d = sp - sn;
    const float invB = 1.0f / (float)B;
    float term;
    if (variant == CHAOREC_BPR_LOG_SIGMOID_EPS) {
      const float s = sigmoidf_acc(d);
      term = logf(s + 1e-5f);
      c = -invB * (s * (1.0f - s)) / (s + 1e-5f);
    } else if (variant == CHAOREC_BPR_LOGSIGMOID) {
      // logsigmoid(d) = min(d,0) - log1p(exp(-|d|))
      term = fminf(d, 0.f) - log1pf(expf(-fabsf(d)));
      c = -invB * sigmoidf_acc(-d);
    } else {
      const float s = sigmoidf_acc(d);
      term = logf(s);
      c = -invB * (1.0f - s);
    }
    coef[b] = c;
    ws[b] = term;
    ws[B + b] = ru;
    ws[2 * B + b] = rp;
    ws[3 * B + b] = rn;
  }
  return __shfl(c, 0, 64);
}

// Layer-table row source: see bpr_fwd_bwd_drawn_kernel<NT> (csrc/bpr.hip).
constexpr int kMeanMaxTabs = 4;
constexpr int kMeanMaxQ = 4;
struct MeanSrc {
  const float *t[kMeanMaxTabs];             // x_0 .. x_L, [N, D] each, users first
  int n;
  float w;
  int64_t item_offset;                      // row of item 0
  float *rows;
};
// one element of the mean of NT layer values: w t_0 + w t_1 + ..., left to right, every product and sum rounded
template <int NT>
__device__ __forceinline__ float mean_of(float w, const float (&t)[NT]) {
  float m = mul_rn(w, t[0]);
#pragma unroll
  for (int i = 1; i < NT; ++i) m = add_rn(m, mul_rn(w, t[i]));
  return m;
}
// (NT, the table count, is a template parameter of the launch: with a run-time count every table's load sat in a branch of
//  its own and waited for the one before -- twelve round trips in a row instead of one, 7.4 -> 10.7 us)
template <int NT>
__device__ __forceinline__ void mean_elems(const MeanSrc &M, size_t ou, size_t op, size_t on, float &mu, float &mp, float &mn) {
  float tu[NT], tp[NT], tn[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) tu[i] = M.t[i][ou], tp[i] = M.t[i][op], tn[i] = M.t[i][on];
  mu = mean_of<NT>(M.w, tu), mp = mean_of<NT>(M.w, tp), mn = mean_of<NT>(M.w, tn);
}

// one element of a sample's three gradient rows (d(loss) = 1; c its coefficient, r2 = 2 reg / (B D)), added atomically: the
// values of bpr_bwd_kernel with grad_out = 1
__device__ __forceinline__ void bpr_grad_adds(float *g_u, float *g_i, size_t eu, size_t ep, size_t en, float c, float r2,
                                              float uu, float pp, float nn) {
  atomicAdd(g_u + eu, c * (pp - nn) + r2 * uu);
  atomicAdd(g_i + ep, c * uu + r2 * pp);
  atomicAdd(g_i + en, -c * uu + r2 * nn);
}

// the rows of the gradient buffer a sample touched, for the row-sparse backward propagates (chaorec_spmm_csr_rowsparse_f32):
// bit r of a bitmap over the joined table's rows, items from bits_item_offset on; lanes 0 .. 2 of the calling wave
__device__ __forceinline__ void flag_triple_rows(uint32_t *row_bits, int64_t bits_item_offset, int lane, int64_t u, int64_t p,
                                                 int64_t n) {
  if (row_bits && lane < 3) {
    const int64_t r = lane == 0 ? u : bits_item_offset + (lane == 1 ? p : n);
    atomicOr(row_bits + (r >> 5), 1u << (r & 31));
  }
}

// the optimizer's step count and this step's bias corrections, by ONE thread of the launch
__device__ __forceinline__ void adam_step_on(int32_t *__restrict__ adam_step, float beta1, float beta2, float *__restrict__ adam_bc) {
  const int st = adam_step[0] + 1;
  adam_step[0] = st;
  adam_bias_corrections(st, beta1, beta2, adam_bc[0], adam_bc[1]);
}

// the arguments every fused forward + backward launch takes (who: the export's short name)
inline int bpr_fwd_bwd_check(const char *who, const float *coef, const float *workspace, const float *g_u, const float *g_i,
                             const int64_t *edges, int64_t n_edges, const int64_t *hist_rowptr, int32_t num_item,
                             const int64_t *in_users, const int64_t *in_pos, const int64_t *in_neg, const int64_t *out_users,
                             const int64_t *out_pos, const int64_t *out_neg, const int64_t *perm, const int64_t *perm_pos,
                             int64_t pos_offset, const int32_t *adam_step, const float *adam_bc, int32_t B, int32_t D,
                             int32_t variant) {
  if (!coef || !workspace || !g_u || !g_i) return fail(CHAOREC_E_INVALID, "%s: NULL argument", who);
  if (pos_offset < 0) return fail(CHAOREC_E_INVALID, "%s: pos_offset %lld", who, (long long)pos_offset);
  if (adam_step && !adam_bc) return fail(CHAOREC_E_INVALID, "%s: adam_step without adam_bc", who);
  if (edges) {
    if (!hist_rowptr || !out_users || !out_pos || !out_neg) return fail(CHAOREC_E_INVALID, "%s: NULL draw argument", who);
    if (n_edges <= 0 || num_item <= 0) return fail(CHAOREC_E_INVALID, "%s: bad sizes", who);
    if (perm && !perm_pos) return fail(CHAOREC_E_INVALID, "%s: perm without perm_pos", who);
  } else if (!in_users || !in_pos || !in_neg) {
    return fail(CHAOREC_E_INVALID, "%s: neither an edge list to draw from nor a batch", who);
  }
  if (B <= 0 || D <= 0) return fail(CHAOREC_E_INVALID, "%s: B=%d D=%d", who, B, D);
  if (variant < 0 || variant > 2) return fail(CHAOREC_E_INVALID, "%s: variant %d", who, variant);
  return CHAOREC_OK;
}

// CHAOREC_BPR_ORDERED=2: the fused steps' gradient rows too are added by the ordered, atomic-free launch (one more launch per
// step -- ~7 us of a 121 us sports step, nothing of a configs[4] step --: a LightGCN run is then the same bits every time,
// and the fused step equals the autograd step bit for bit also on batches with repeated rows).  Read per call.
bool bpr_ordered_after_fused(int32_t B, int32_t D);

// the ordered gradient launch (csrc/bpr.hip).  rows: NULL = the table rows users[b] / pos[b] / neg[b] of tab_u / tab_i; else
// MeanSrc::rows, the tables unused
int bpr_bwd_ordered(const float *tab_u, const float *tab_i, const float *rows, const int64_t *users, const int64_t *pos,
                    const int64_t *neg, int32_t B, int32_t D, const float *coef, float reg_weight, const float *grad_out,
                    float *g_u, float *g_i, void *stream);

}  // namespace chaorec
