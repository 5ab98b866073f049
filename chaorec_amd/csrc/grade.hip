// Grade (Model/Grade.py): the views of its G generators (ID, visual, textual; vgae.generate + normalize_adjacency_matrix) over
// one symmetric-pattern CSR of N = U + I nodes.  gfx950, D = 64, fp32.  The generators are independent (all run without
// gradient on fixed weights), so every launch runs over them in gridDim.y: z [G, N, 64], W1 [G, 64, 64], b1 [G, 64],
// w2 [G, 64], b2 [G].
//
// The structure is AdaGCL's (rowptr int64 [N + 1], col int32 [E], entry_row int32 [E], tentry int32 [E]: entry tentry[e] is
// the stored entry (col e, row e)) and owner int32 [P]: the entries with entry_row[e] <= col[e], each undirected pair once.
//
// 1 gr_pair_kernel, over the owner list: edge_mlp.h's tile, 64 owners per wave
//     logit = w2 . relu(W1 relu(z[row] * z[col]) + b1) + b2;  p = sigmoid(logit);  keep = floor(p + 0.5) != 0
//     val[g][e] = val[g][tentry[e]] = keep ? p : +0 (the same bits: a view is symmetric bit for bit); keep and, if asked,
//     logit at both places; kept[g] += the stored entries kept (2 for an off-diagonal pair): one integer atomic per wave.
// 2 gr_rows_kernel, row ownership of edge_mlp.h: S = (the row's sum of val) + 1e-7f, d[g][n] = S^-1/2.  An empty or
//     all-dropped row: d = (1e-7f)^-1/2, which multiplies only zeros.
// 3 gr_vals_kernel, over the owner list: val[g][e] = val[g][tentry[e]] = (d[row e] val[g][e]) d[col e], D.dot(A).dot(D)'s order
//     at the owner's entry, in place, no contraction.  The product is formed once per pair because (d_r p) d_c and (d_c p) d_r
//     can differ in the last bit: the reversed entry gets the owner's bits.
// No float atomics; two runs give the same bits.
#include "edge_mlp.h"

namespace chaorec {

constexpr float GR_EPS = 1e-7f;
constexpr int GR_MAX_G = 64;

__global__ __launch_bounds__(256) void gr_pair_kernel(const float *__restrict__ z, int64_t N, const int32_t *__restrict__ entry_row,
                                                      const int32_t *__restrict__ col, const int32_t *__restrict__ tentry, int64_t E,
                                                      const int32_t *__restrict__ owner, int64_t P, const float *__restrict__ W1,
                                                      const float *__restrict__ b1, const float *__restrict__ w2,
                                                      const float *__restrict__ b2, float *__restrict__ val, uint8_t *__restrict__ keep,
                                                      unsigned long long *__restrict__ kept, float *__restrict__ logit_out) {
  __shared__ EdgeMlpLds lds;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t g = blockIdx.y;
  edge_mlp_stage(lds, W1 + g * AG_D * AG_D, b1 + g * AG_D, w2 + g * AG_D, t);
  const float bias2 = b2[g];
  const float *zg = z + g * N * AG_D;
  float *valg = val + g * E;
  uint8_t *keepg = keep + g * E;
  float *logitg = logit_out ? logit_out + g * E : nullptr;
  const int64_t n_tiles = (P + 255) / 256;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t p0 = tile * 256 + wave * 64;
    if (p0 >= P) continue;
    const float mine = edge_mlp_tile(lds, zg, bias2, lane, [&](int slot) -> EdgeNodes {
      const int64_t p = p0 + slot;
      const int64_t e = clamp_index((int64_t)owner[p < P ? p : P - 1], E);
      return {clamp_index(entry_row[e], N), clamp_index(col[e], N)};
    });
    const int64_t p = p0 + lane;
    const bool valid = p < P;
    const int64_t e = clamp_index((int64_t)owner[valid ? p : P - 1], E);
    const int64_t te = clamp_index((int64_t)tentry[e], E);
    const float prob = sigmoidf_acc(mine);
    const bool kp = valid && floorf(prob + 0.5f) != 0.f;
    if (valid) {
      const float v = kp ? prob : 0.f;
      const uint8_t k = kp ? 1 : 0;
      valg[e] = v;
      keepg[e] = k;
      if (logitg) logitg[e] = mine;
      if (te != e) {
        valg[te] = v;
        keepg[te] = k;
        if (logitg) logitg[te] = mine;
      }
    }
    const unsigned long long votes = __ballot(kp), pairs = __ballot(kp && te != e);
    if (lane == 0 && votes) atomicAdd(kept + g, (unsigned long long)(__popcll(votes) + __popcll(pairs)));
  }
}

__global__ __launch_bounds__(256) void gr_rows_kernel(const int64_t *__restrict__ rowptr, int64_t N, int64_t E,
                                                      const float *__restrict__ val, float *__restrict__ d) {
  const int lane = threadIdx.x & 63;
  const int64_t g = blockIdx.y;
  const float *valg = val + g * E;
  const LaneRow row = lane_group_row(rowptr, N);
  const ag2 acc = ag_row_reduce(row.n, row.beg, row.end, lane, [&](int64_t e, int64_t) -> ag2 {
    return {valg[clamp_index(e, E)], 0.f};
  });
  if (row.valid && (lane & 7) == 0) d[g * N + row.n] = 1.0f / sqrtf(acc.a + GR_EPS);
}

__global__ __launch_bounds__(256) void gr_vals_kernel(const int32_t *__restrict__ entry_row, const int32_t *__restrict__ col,
                                                      const int32_t *__restrict__ tentry, int64_t N, int64_t E,
                                                      const int32_t *__restrict__ owner, int64_t P, const float *__restrict__ d,
                                                      float *__restrict__ val) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x, g = blockIdx.y;
  if (p >= P) return;
  const int64_t e = clamp_index((int64_t)owner[p], E), te = clamp_index((int64_t)tentry[e], E);
  const float *dg = d + g * N;
  float *valg = val + g * E;
  const float v = mul_rn(mul_rn(dg[clamp_index(entry_row[e], N)], valg[e]), dg[clamp_index(col[e], N)]);
  valg[e] = v;
  if (te != e) valg[te] = v;
}

}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_grade_check_shape(int32_t D) {
  if (D != AG_D) return fail(CHAOREC_E_INVALID, "grade_check_shape: D=%d, the kernels tile D=%d", (int)D, AG_D);
  return CHAOREC_OK;
}

extern "C" int chaorec_grade_views_f32(const float *z, const float *W1, const float *b1, const float *w2, const float *b2, int32_t G,
                                       int64_t N, const int64_t *rowptr, const int32_t *col, const int32_t *entry_row,
                                       const int32_t *tentry, int64_t E, const int32_t *owner, int64_t P, float *val, uint8_t *keep,
                                       int64_t *kept, float *logit_out, float *d, void *stream) {
  if (!z || !W1 || !b1 || !w2 || !b2 || !rowptr || !col || !entry_row || !tentry || !owner || !val || !keep || !kept || !d)
    return fail(CHAOREC_E_INVALID, "grade_views: NULL argument");
  if (G < 1 || G > GR_MAX_G) return fail(CHAOREC_E_INVALID, "grade_views: G=%d, 1 .. %d generators", (int)G, GR_MAX_G);
  if (N <= 0 || E <= 0 || P <= 0 || P > E || N >= ((int64_t)1 << 31) - AG_RB || E >= ((int64_t)1 << 31) - 256)
    return fail(CHAOREC_E_INVALID, "grade_views: N=%lld E=%lld P=%lld", (long long)N, (long long)E, (long long)P);
  if ((reinterpret_cast<uintptr_t>(z) & 15) || (reinterpret_cast<uintptr_t>(kept) & 7))
    return fail(CHAOREC_E_INVALID, "grade_views: z must be 16-byte aligned, kept 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(kept, 0, sizeof(int64_t) * (size_t)G, st) != hipSuccess)
    return fail(CHAOREC_E_LAUNCH, "grade_views: hipMemsetAsync failed");
  const int64_t tiles = (P + 255) / 256;
  const unsigned g = (unsigned)G;
  hipLaunchKernelGGL(gr_pair_kernel, dim3((unsigned)(tiles < 2048 ? tiles : 2048), g), dim3(256), 0, st, z, N, entry_row, col, tentry, E,
                     owner, P, W1, b1, w2, b2, val, keep, reinterpret_cast<unsigned long long *>(kept), logit_out);
  hipLaunchKernelGGL(gr_rows_kernel, dim3((unsigned)((N + AG_RB - 1) / AG_RB), g), dim3(256), 0, st, rowptr, N, E, val, d);
  hipLaunchKernelGGL(gr_vals_kernel, dim3((unsigned)tiles, g), dim3(256), 0, st, entry_row, col, tentry, N, E, owner, P, d, val);
  return check_launch("grade_views");
}
