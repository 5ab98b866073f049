// AdaGCL (Model/AdaGCL.py): the E-sized work of its two view generators.  gfx950, D = 64.
//
// The structure is the model's one symmetric-pattern CSR over N = U + I nodes (rowptr int64 [N + 1], col int32 [E],
// entry_row int32 [E], tentry int32 [E]: entry tentry[e] is the stored entry (col e, row e)).
//
// Row ownership, everywhere a row is summed, and the MLP tile of (c) are edge_mlp.h's (shared with grade.hip): 8 lanes per
// row, a row with more than AG_LONG = 64 entries taken by its whole wave; a sum's order depends on the row's length alone:
// two runs give the same bits.  No atomics on floats; the one atomic is the integer count of kept entries in (c).
//
// (a) edge gate, DenoisingNet.generate (evaluation form) / DenoisingNet.call (training form), per layer:
//   logit[e] = (s_nb[row e] + s_self[col e]) + b_att          (the last Linear has one output: two per-NODE scalars)
//   gate     = sigmoid(logit)                                          evaluation, fp32
//            = sigmoid(((log u - log(1 - u)) + logit) / beta)          training -- in DOUBLE, rounded once into m: the reference's
//              numpy draw is float64 and promotes this one expression (Model/AdaGCL.py:583-596 ends in .float())
//   m[e]     = clamp(gate * 1.5 - 0.45, 0, 1);  S[n] = sum_{e in row n} m[e] + eps;  d[n] = clamp(S^-1/2, 0, 10)  (S = 0: 10)
//   val[e]   = (m[e] d[row e]) d[col e];  l0 = 1 / E sum_e sigmoid(logit[e] - beta log(0.45 / 1.05))
//   u: given fp32 [E], or u NULL: lo + (hi - lo) draw_uniform<24>(draw_key(seed, state[1], salt), 0, e) clamped into
//   [lo, hi] = [1e-7f, fl32(1 - 1e-7)]; written to u_out if not NULL (the backward reads it: no redraw).
//   Launch 1 (ag_gate_rows_kernel) owns rows: m, S, d, u_out, one l0 partial per workgroup.  Launch 2 (ag_gate_vals_kernel)
//   owns entries: val; its workgroup 0 adds the partials in double, thread t the entries t, t + 256, ..., then a tree.
// (b) edge gate backward, three launches, each row owned once per launch:
//   1 g_d[n] = sum_{e in row n} (g_val[e] m[e] + g_val[t] m[t]) d[col e], t = tentry[e] (the entries whose COLUMN is n);
//     g_S[n] = -1/2 S^-3/2 g_d where 0 <= S^-1/2 <= 10 (torch's clamp hands the gradient through at equality), else 0
//   2 g_m = g_val[e] d[row] d[col] + g_S[row]; g_logit[e] = g_m [0 <= stretched <= 1] 1.5 gate (1 - gate) (/ beta in training)
//     + g_l0 / E s (1 - s), s the l0 sigmoid; g_s_nb[n] = the row's sum; one g_b partial per workgroup
//   3 g_s_self[n] = sum_{e in row n} g_logit[tentry[e]]; workgroup 0 adds the g_b partials as above
// (c) edge MLP keep, vgae.generate (Model/AdaGCL.py:483-501), forward only:
//   logit[e] = w2 . relu(W1 relu(z[row e] * z[col e]) + b1) + b2;  keep[e] = floor(sigmoid(logit) + 0.5) != 0
//   out[e] = keep ? vals[e] : +0;  kept = the count (int64 on the device);  a second launch: out[e] /= fl32(kept / E), kept = 0
//   leaves the zeros.  One wave = 64 entries x 64 x 64 on v_mfma_f32_32x32x2_f32 (exact fp32 products, k-ascending chain):
//   C[feature][entry] = sum_k W1[feature][k] P[entry][k] -- A = W1 from LDS (16 KB, Ws[k][f ^ 32 (k & 1)]: the two k of
//   one instruction sit in different halves of the 64 banks), B = the gathered rows' product, formed in registers.  The
//   features are the accumulator's rows, so the w2 dot is a per-lane sum over 32 registers and one xor-32 exchange.
//   Workgroups stride over the tiles of 256 entries; the tail is masked.
#include "edge_mlp.h"

namespace chaorec {

constexpr float AG_GAMMA = -0.45f, AG_STRETCH = 1.5f;      // zeta - gamma = 1.05 + 0.45
constexpr float AG_U_LO = 1e-7f, AG_U_HI = 0.99999988f;    // fl32(1 - 1e-7)

// part[blockIdx.x] = the sum of the group leaders' v over the workgroup: butterfly per wave, then waves 0..3 in order
__device__ __forceinline__ void ag_block_partial(float v, int lane, int wave, float *__restrict__ part) {
  __shared__ float ws[4];
  v = wave_sum((lane & 7) == 0 ? v : 0.f);
  if (lane == 0) ws[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// out[0] = scale * sum(part[0 .. n)) by ONE workgroup of 256 threads, in double, fixed order
__device__ __forceinline__ void ag_block_total(const float *__restrict__ part, int64_t n, double scale, float *__restrict__ out) {
  __shared__ double red[256];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) v += (double)part[i];
  block_sum_f64(v, red);
  if (threadIdx.x == 0) out[0] = (float)(red[0] * scale);
}

__device__ __forceinline__ float ag_l0_shift(float beta) { return beta * logf(0.45f / 1.05f); }

struct AgGate {
  float m;        // the mask
  float slope;    // d m / d logit (0 where the stretched value left [0, 1])
};
__device__ __forceinline__ AgGate ag_gate(float logit, float u, float beta, int training) {
  if (training) {
    const double ud = (double)u;
    const double g = 1.0 / (1.0 + exp(-(((log(ud) - log(1.0 - ud)) + (double)logit) / (double)beta)));
    const double s = g * 1.5 + (-0.45);
    const bool in = s >= 0.0 && s <= 1.0;
    return {(float)(s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s)), in ? (float)(1.5 * g * (1.0 - g) / (double)beta) : 0.f};
  }
  const float g = sigmoidf_acc(logit);
  const float s = g * AG_STRETCH + AG_GAMMA;
  const bool in = s >= 0.f && s <= 1.f;
  return {fminf(fmaxf(s, 0.f), 1.f), in ? AG_STRETCH * (g * (1.f - g)) : 0.f};
}

__global__ __launch_bounds__(256) void ag_gate_rows_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t N,
                                                           const float *__restrict__ s_nb, const float *__restrict__ s_self,
                                                           const float *__restrict__ b_att, float beta, float eps, int training,
                                                           const float *__restrict__ u, uint64_t seed, const int64_t *__restrict__ state,
                                                           uint64_t salt, float *__restrict__ m, float *__restrict__ S, float *__restrict__ d,
                                                           float *__restrict__ u_out, float *__restrict__ l0_part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const LaneRow row = lane_group_row(rowptr, N);
  const float b = b_att[0], shift = ag_l0_shift(beta);
  const uint64_t key = (training && !u) ? draw_key(seed, (uint64_t)state[1], salt) : 0;
  const ag2 acc = ag_row_reduce(row.n, row.beg, row.end, lane, [&](int64_t e, int64_t r) -> ag2 {
    const float logit = (s_nb[r] + s_self[clamp_index(col[e], N)]) + b;
    float ue = 0.5f;
    if (training) {
      ue = u ? u[e] : fminf(fmaxf(AG_U_LO + (AG_U_HI - AG_U_LO) * draw_uniform<24>(key, 0, (uint64_t)e), AG_U_LO), AG_U_HI);
      if (u_out) u_out[e] = ue;
    }
    const float me = ag_gate(logit, ue, beta, training).m;
    m[e] = me;
    return {me, sigmoidf_acc(logit - shift)};
  });
  if (row.valid && (lane & 7) == 0) {
    const float s = acc.a + eps;
    S[row.n] = s;
    d[row.n] = fminf(fmaxf(1.0f / sqrtf(s), 0.f), 10.f);
  }
  ag_block_partial(acc.b, lane, wave, l0_part);
}

__global__ __launch_bounds__(256) void ag_gate_vals_kernel(const int32_t *__restrict__ entry_row, const int32_t *__restrict__ col, int64_t N,
                                                           int64_t E, const float *__restrict__ m, const float *__restrict__ d,
                                                           float *__restrict__ val, const float *__restrict__ l0_part, int64_t n_part,
                                                           float *__restrict__ l0) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < E) val[e] = mul_rn(mul_rn(m[e], d[clamp_index(entry_row[e], N)]), d[clamp_index(col[e], N)]);
  if (blockIdx.x == 0) ag_block_total(l0_part, n_part, 1.0 / (double)E, l0);
}

__global__ __launch_bounds__(256) void ag_bwd_gd_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                        const int32_t *__restrict__ tentry, int64_t N, int64_t E, const float *__restrict__ m,
                                                        const float *__restrict__ S, const float *__restrict__ d,
                                                        const float *__restrict__ g_val, float *__restrict__ g_S) {
  const int lane = threadIdx.x & 63;
  const LaneRow row = lane_group_row(rowptr, N);
  const ag2 acc = ag_row_reduce(row.n, row.beg, row.end, lane, [&](int64_t e, int64_t) -> ag2 {
    const int64_t t = clamp_index((int64_t)tentry[e], E);
    return {(g_val[e] * m[e] + g_val[t] * m[t]) * d[clamp_index(col[e], N)], 0.f};
  });
  if (row.valid && (lane & 7) == 0) {
    const float s = S[row.n], r = 1.0f / sqrtf(s);
    g_S[row.n] = (r >= 0.f && r <= 10.f) ? -0.5f * (r / s) * acc.a : 0.f;
  }
}

__global__ __launch_bounds__(256) void ag_bwd_logit_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t N,
                                                           int64_t E, const float *__restrict__ s_nb, const float *__restrict__ s_self,
                                                           const float *__restrict__ b_att, float beta, int training,
                                                           const float *__restrict__ u, const float *__restrict__ d,
                                                           const float *__restrict__ g_val, const float *__restrict__ g_S,
                                                           const float *__restrict__ g_l0, float *__restrict__ g_logit,
                                                           float *__restrict__ g_s_nb, float *__restrict__ gb_part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const LaneRow row = lane_group_row(rowptr, N);
  const float b = b_att[0], shift = ag_l0_shift(beta);
  const float gl = g_l0 ? g_l0[0] / (float)E : 0.f;
  const ag2 acc = ag_row_reduce(row.n, row.beg, row.end, lane, [&](int64_t e, int64_t r) -> ag2 {
    const int c = clamp_index(col[e], N);
    const float logit = (s_nb[r] + s_self[c]) + b;
    const float gm = (g_val[e] * d[r]) * d[c] + g_S[r];
    const float s0 = sigmoidf_acc(logit - shift);
    const float gz = gm * ag_gate(logit, training ? u[e] : 0.5f, beta, training).slope + gl * (s0 * (1.f - s0));
    g_logit[e] = gz;
    return {gz, 0.f};
  });
  if (row.valid && (lane & 7) == 0) g_s_nb[row.n] = acc.a;
  ag_block_partial(acc.a, lane, wave, gb_part);
}

__global__ __launch_bounds__(256) void ag_bwd_self_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ tentry, int64_t N,
                                                          int64_t E, const float *__restrict__ g_logit, float *__restrict__ g_s_self,
                                                          const float *__restrict__ gb_part, int64_t n_part, float *__restrict__ g_b) {
  const int lane = threadIdx.x & 63;
  const LaneRow row = lane_group_row(rowptr, N);
  const ag2 acc = ag_row_reduce(row.n, row.beg, row.end, lane, [&](int64_t e, int64_t) -> ag2 {
    const int64_t t = clamp_index((int64_t)tentry[e], E);
    return {g_logit[t], 0.f};
  });
  if (row.valid && (lane & 7) == 0) g_s_self[row.n] = acc.a;
  if (blockIdx.x == 0) ag_block_total(gb_part, n_part, 1.0, g_b);
}

__global__ __launch_bounds__(256) void ag_keep_kernel(const float *__restrict__ z, int64_t N, const int32_t *__restrict__ entry_row,
                                                      const int32_t *__restrict__ col, int64_t E, const float *__restrict__ W1,
                                                      const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2,
                                                      const float *__restrict__ vals, uint8_t *__restrict__ keep, float *__restrict__ out,
                                                      unsigned long long *__restrict__ kept, float *__restrict__ logit_out) {
  __shared__ EdgeMlpLds lds;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  edge_mlp_stage(lds, W1, b1, w2, t);
  const float bias2 = b2[0];
  const int64_t n_tiles = (E + 255) / 256;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t e0 = tile * 256 + wave * 64;
    if (e0 >= E) continue;
    const float mine = edge_mlp_tile(lds, z, bias2, lane, [&](int slot) -> EdgeNodes {
      const int64_t e = e0 + slot, ee = e < E ? e : E - 1;
      return {clamp_index(entry_row[ee], N), clamp_index(col[ee], N)};
    });
    const int64_t e = e0 + lane;
    const bool valid = e < E;
    const bool kp = valid && floorf(sigmoidf_acc(mine) + 0.5f) != 0.f;
    if (valid) {
      keep[e] = kp ? 1 : 0;
      out[e] = kp ? vals[e] : 0.f;
      if (logit_out) logit_out[e] = mine;
    }
    const unsigned long long votes = __ballot(kp);
    if (lane == 0 && votes) atomicAdd(kept, (unsigned long long)__popcll(votes));
  }
}

__global__ __launch_bounds__(256) void ag_keep_scale_kernel(float *__restrict__ out, int64_t E, const unsigned long long *__restrict__ kept) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const unsigned long long k = kept[0];
  if (e >= E || k == 0) return;
  out[e] = out[e] / (float)((double)k / (double)E);
}

static inline unsigned ag_row_blocks(int64_t N) { return (unsigned)((N + AG_RB - 1) / AG_RB); }
static inline unsigned ag_entry_blocks(int64_t E) { return (unsigned)((E + 255) / 256); }

}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_adagcl_check_shape(int32_t D) {
  if (D != AG_D) return fail(CHAOREC_E_INVALID, "adagcl_check_shape: D=%d, the kernels tile D=%d", (int)D, AG_D);
  return CHAOREC_OK;
}

extern "C" int64_t chaorec_adagcl_rows_per_block(void) { return AG_RB; }
extern "C" int64_t chaorec_adagcl_long_row(void) { return AG_LONG; }

extern "C" int chaorec_adagcl_tick(int64_t *state, void *stream) {
  return launch_step_tick("adagcl_tick", state, stream);
}

static int ag_check_graph(const char *what, int64_t N, int64_t E) {
  if (N <= 0 || E <= 0 || N >= ((int64_t)1 << 31) - AG_RB || E >= ((int64_t)1 << 31) - 256)
    return fail(CHAOREC_E_INVALID, "%s: N=%lld E=%lld", what, (long long)N, (long long)E);
  return CHAOREC_OK;
}

extern "C" int chaorec_adagcl_gate_fwd_f32(const int64_t *rowptr, const int32_t *col, const int32_t *entry_row, int64_t N, int64_t E,
                                           const float *s_nb, const float *s_self, const float *b_att, float beta, float eps,
                                           int32_t training, const float *u, uint64_t seed, const int64_t *state, int32_t salt,
                                           float *m, float *S, float *d, float *val, float *l0, float *u_out, float *part,
                                           int64_t n_part, void *stream) {
  if (!rowptr || !col || !entry_row || !s_nb || !s_self || !b_att || !m || !S || !d || !val || !l0 || !part)
    return fail(CHAOREC_E_INVALID, "adagcl_gate_fwd: NULL argument");
  if (ag_check_graph("adagcl_gate_fwd", N, E)) return CHAOREC_E_INVALID;
  if (training && !u && !state) return fail(CHAOREC_E_INVALID, "adagcl_gate_fwd: neither u nor a step counter");
  if (training && !(beta > 0.f)) return fail(CHAOREC_E_INVALID, "adagcl_gate_fwd: beta=%g", (double)beta);
  if (salt < 0) return fail(CHAOREC_E_INVALID, "adagcl_gate_fwd: salt=%d", (int)salt);
  if (n_part < (int64_t)ag_row_blocks(N))
    return fail(CHAOREC_E_WORKSPACE, "adagcl_gate_fwd: %lld partials, %lld needed", (long long)n_part, (long long)ag_row_blocks(N));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ag_gate_rows_kernel, dim3(ag_row_blocks(N)), dim3(256), 0, st, rowptr, col, N, s_nb, s_self, b_att, beta, eps,
                     (int)training, u, seed, state, (uint64_t)salt, m, S, d, training ? u_out : nullptr, part);
  hipLaunchKernelGGL(ag_gate_vals_kernel, dim3(ag_entry_blocks(E)), dim3(256), 0, st, entry_row, col, N, E, m, d, val, part,
                     (int64_t)ag_row_blocks(N), l0);
  return check_launch("adagcl_gate_fwd");
}

extern "C" int chaorec_adagcl_gate_bwd_f32(const int64_t *rowptr, const int32_t *col, const int32_t *tentry, int64_t N, int64_t E,
                                           const float *s_nb, const float *s_self, const float *b_att, float beta, int32_t training,
                                           const float *u, const float *m, const float *S, const float *d, const float *g_val,
                                           const float *g_l0, float *g_logit, float *g_S, float *g_s_nb, float *g_s_self, float *g_b,
                                           float *part, int64_t n_part, void *stream) {
  if (!rowptr || !col || !tentry || !s_nb || !s_self || !b_att || !m || !S || !d || !g_val || !g_logit || !g_S || !g_s_nb ||
      !g_s_self || !g_b || !part)
    return fail(CHAOREC_E_INVALID, "adagcl_gate_bwd: NULL argument");
  if (ag_check_graph("adagcl_gate_bwd", N, E)) return CHAOREC_E_INVALID;
  if (training && (!u || !(beta > 0.f))) return fail(CHAOREC_E_INVALID, "adagcl_gate_bwd: the training form needs u and beta > 0");
  if (n_part < (int64_t)ag_row_blocks(N))
    return fail(CHAOREC_E_WORKSPACE, "adagcl_gate_bwd: %lld partials, %lld needed", (long long)n_part, (long long)ag_row_blocks(N));
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(ag_row_blocks(N)), block(256);
  hipLaunchKernelGGL(ag_bwd_gd_kernel, grid, block, 0, st, rowptr, col, tentry, N, E, m, S, d, g_val, g_S);
  hipLaunchKernelGGL(ag_bwd_logit_kernel, grid, block, 0, st, rowptr, col, N, E, s_nb, s_self, b_att, beta, (int)training, u, d, g_val,
                     g_S, g_l0, g_logit, g_s_nb, part);
  hipLaunchKernelGGL(ag_bwd_self_kernel, grid, block, 0, st, rowptr, tentry, N, E, g_logit, g_s_self, part, (int64_t)ag_row_blocks(N),
                     g_b);
  return check_launch("adagcl_gate_bwd");
}

extern "C" int chaorec_adagcl_keep_f32(const float *z, int64_t N, const int32_t *entry_row, const int32_t *col, int64_t E,
                                       const float *W1, const float *b1, const float *w2, const float *b2, const float *vals,
                                       uint8_t *keep, float *out, int64_t *kept, float *logit_out, void *stream) {
  if (!z || !entry_row || !col || !W1 || !b1 || !w2 || !b2 || !vals || !keep || !out || !kept)
    return fail(CHAOREC_E_INVALID, "adagcl_keep: NULL argument");
  if (ag_check_graph("adagcl_keep", N, E)) return CHAOREC_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(z) & 15) || (reinterpret_cast<uintptr_t>(kept) & 7))
    return fail(CHAOREC_E_INVALID, "adagcl_keep: z must be 16-byte aligned, kept 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(kept, 0, sizeof(int64_t), st) != hipSuccess) return fail(CHAOREC_E_LAUNCH, "adagcl_keep: hipMemsetAsync failed");
  const int64_t tiles = (E + 255) / 256;
  hipLaunchKernelGGL(ag_keep_kernel, dim3((unsigned)(tiles < 2048 ? tiles : 2048)), dim3(256), 0, st, z, N, entry_row, col, E, W1, b1, w2,
                     b2, vals, keep, out, reinterpret_cast<unsigned long long *>(kept), logit_out);
  hipLaunchKernelGGL(ag_keep_scale_kernel, dim3(ag_entry_blocks(E)), dim3(256), 0, st, out, E,
                     reinterpret_cast<const unsigned long long *>(kept));
  return check_launch("adagcl_keep");
}
