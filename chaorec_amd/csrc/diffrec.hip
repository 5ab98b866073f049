// DiffRec's two hot paths (Model/DiffRec.py:263-303, 425-463): the denoiser's output layer with the importance-weighted x0
// loss and the complete gradient by the layer's output in one pass, and one step of the sampling chain collapsed to the
// hidden width.  Additive to ABI 16.  fp32, no atomics on floats, no scratch, the same bits every run.
//
// (a) dr_tile_kernel<DR_LOSS>   d_out = c_b (h W_out^T + b_out - x0), per-row partials of err^2 per item tile
// (b) dr_reduce_kernel          the row partials in item-tile order -> reloss_rows (double), loss = mean_b reloss_b / pt_b
// (c) dr_tile_kernel<DR_CHAIN>  p_next = c1 (z G^T + g0) + c2 p,  z_next = tanh(p_next + e_next)
//
// One tile serves both: out_tile.h's placement of the workgroups and its K loop, the chain of an element cut into segments
// of 64 k; (a)'s epilogue and padded store are out_tile.h's as well, shared with diffmm.hip's output layer.
#include "out_tile.h"

namespace chaorec {

constexpr int DR_LOSS = 0, DR_CHAIN = 1;

// What the two epilogues read and write beside the product.  LOSS: bias = b_out [N], bits, c_row [M], out0 = d_out [M, ldo]
// (columns N .. ldo written 0), part [M, NT].  CHAIN: bias = g0 [N], e = e_next [N], prev = p [M, ldp], out0 = p_next and
// out1 = z_next [M, ldo], c1, c2.
struct DrEpilogue {
  const float *bias;
  const uint32_t *bits;
  int64_t nwords;
  const float *c_row;
  float *part;
  const float *e;
  const float *prev;
  int64_t ldp;
  float c1, c2;
  float *out0, *out1;
  int64_t ldo;
};

template <int EPI>
static __global__ __launch_bounds__(256) void dr_tile_kernel(const float *__restrict__ A, int64_t lda, const float *__restrict__ Bm,
                                                             int64_t ldb, int64_t M, int64_t N, int64_t K, int64_t MT, int64_t NT,
                                                             DrEpilogue ep) {
  __shared__ OtStage As, Bs;
  const OutTile tp = out_tile_place(MT, NT);
  if (!tp.live) return;           // the whole workgroup: no barrier has been reached

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = vae_zero();
  out_tile_run<true>(acc, tp, As, Bs, A, lda, Bm, ldb, M, N, K);

  if constexpr (EPI == DR_LOSS) {
    __shared__ float Ps[2][OT_BM];      // the row partials: the chain kernel does not carry them
    out_tile_x0_err(acc, tp, Ps, ep.bias, ep.bits, ep.nwords, ep.c_row, M, N, NT, ep.part);
    out_tile_store_padded(acc, tp, M, N, ep.out0, ep.ldo);
  } else {
    // p_next = fl(fl(c1 fl(acc + g0)) + fl(c2 p)), z_next = fl(tanh(fl(p_next + e_next))), the tanh itself evaluated in double:
    // B N evaluations against the tile's 2 B N K flops.  Every element has one owner.
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t gn = tp.n0 + tp.wcol + 32 * j + tp.rr;
        if (gn >= N) continue;
        const float g0 = ep.bias[gn], en = ep.e[gn];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int64_t gm = tp.m0 + tp.wrow + 32 * i + vae_row(reg, tp.hh);
          if (gm >= M) continue;
          const float pn = ep.c1 * (acc[i][j][reg] + g0) + ep.c2 * ep.prev[gm * ep.ldp + gn];
          ep.out0[gm * ep.ldo + gn] = pn;
          ep.out1[gm * ep.ldo + gn] = (float)tanh((double)(pn + en));     // one rounding: the chain feeds on z for steps - 1 launches
        }
      }
  }
}

// (b) reloss_rows[b] = w_b / I sum_tiles part[b, .] (tiles ascending, in double), loss = mean_b reloss_rows[b] / pt_b: one
// workgroup, rows strided per thread, then a tree -- the same order every run.
template <class = void>
static __global__ __launch_bounds__(256) void dr_reduce_kernel(const float *__restrict__ part, int64_t NT, const double *__restrict__ w,
                                                               const double *__restrict__ pt, int64_t B, int64_t I,
                                                               double *__restrict__ reloss_rows, float *__restrict__ loss) {
  __shared__ double red[256];
  double sd = 0.0;
  for (int64_t b = threadIdx.x; b < B; b += 256) {
    double sq = 0.0;
    for (int64_t n = 0; n < NT; ++n) sq += (double)part[b * NT + n];
    const double re = w[b] * (sq / (double)I);
    reloss_rows[b] = re;
    sd += re / pt[b];
  }
  red[threadIdx.x] = sd;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)B);
}

}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_diffrec_check_shape(int64_t B, int64_t I, int64_t H) {
  if (B <= 0 || I <= 0 || H <= 0) return fail(CHAOREC_E_INVALID, "diffrec: B=%lld I=%lld H=%lld", (long long)B, (long long)I, (long long)H);
  if (H % 4) return fail(CHAOREC_E_INVALID, "diffrec: H=%lld is no multiple of 4 (rows are read as float4)", (long long)H);
  if (I > ((int64_t)1 << 31) - 256 || B > ((int64_t)1 << 31) - 256) return fail(CHAOREC_E_INVALID, "diffrec: B=%lld I=%lld", (long long)B, (long long)I);
  return CHAOREC_OK;
}

extern "C" int chaorec_diffrec_tiles(int32_t *bm, int32_t *bn, int32_t *bk) {
  if (!bm || !bn || !bk) return fail(CHAOREC_E_INVALID, "diffrec_tiles: NULL argument");
  *bm = OT_BM;
  *bn = OT_BN;
  *bk = OT_BK;
  return CHAOREC_OK;
}

extern "C" int chaorec_diffrec_out_loss_f32(const float *h, int64_t ldh, const float *W_out, int64_t ldw, const float *b_out,
                                            const uint32_t *bits, const double *w, const double *pt, const float *c_row,
                                            int64_t B, int64_t I, int64_t H, float *d_out, int64_t ldd, float *part,
                                            double *reloss_rows, float *loss, void *stream) {
  if (!h || !W_out || !b_out || !bits || !w || !pt || !c_row || !d_out || !part || !reloss_rows || !loss)
    return fail(CHAOREC_E_INVALID, "diffrec_out_loss: NULL argument");
  if (int rc = chaorec_diffrec_check_shape(B, I, H)) return rc;
  if (ldh < H || ldw < H || (ldh & 3) || (ldw & 3) || ldd < I || !aligned16(h) || !aligned16(W_out))
    return fail(CHAOREC_E_INVALID, "diffrec_out_loss: h, W_out must be 16-byte aligned with row strides that are multiples of 4, ldd >= I");
  const OutGrid g = out_tile_grid(B, I);
  if (!g.blocks) return fail(CHAOREC_E_INVALID, "diffrec_out_loss: too many workgroups at B=%lld I=%lld", (long long)B, (long long)I);
  if (ldd > g.NT * OT_BN) return fail(CHAOREC_E_INVALID, "diffrec_out_loss: ldd=%lld past the last item tile", (long long)ldd);
  DrEpilogue ep = {};
  ep.bias = b_out;
  ep.bits = bits;
  ep.nwords = (I + 31) / 32;
  ep.c_row = c_row;
  ep.part = part;
  ep.out0 = d_out;
  ep.ldo = ldd;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dr_tile_kernel<DR_LOSS>, dim3((unsigned)g.blocks), dim3(256), 0, st, h, ldh, W_out, ldw, B, I, H, g.MT, g.NT, ep);
  if (int rc = check_launch("dr_tile_kernel<loss>")) return rc;
  hipLaunchKernelGGL(dr_reduce_kernel<>, dim3(1), dim3(256), 0, st, part, g.NT, w, pt, B, I, reloss_rows, loss);
  return check_launch("dr_reduce_kernel");
}

extern "C" int chaorec_diffrec_chain_f32(const float *z, int64_t ldz, const float *G, int64_t ldg, const float *g0, const float *p,
                                         int64_t ldp, const float *e_next, float c1, float c2, int64_t B, int64_t N, int64_t K,
                                         float *p_next, float *z_next, int64_t ldo, void *stream) {
  if (!z || !G || !g0 || !p || !e_next || !p_next || !z_next) return fail(CHAOREC_E_INVALID, "diffrec_chain: NULL argument");
  if (int rc = chaorec_diffrec_check_shape(B, N, K)) return rc;
  if (ldz < K || ldg < K || (ldz & 3) || (ldg & 3) || ldp < N || ldo < N || !aligned16(z) || !aligned16(G))
    return fail(CHAOREC_E_INVALID, "diffrec_chain: z, G must be 16-byte aligned with row strides that are multiples of 4, ldp, ldo >= N");
  if (p_next == z_next || p_next == z || z_next == z || z_next == p)
    return fail(CHAOREC_E_INVALID, "diffrec_chain: the outputs must not alias each other or an operand another workgroup reads");
  const OutGrid g = out_tile_grid(B, N);
  if (!g.blocks) return fail(CHAOREC_E_INVALID, "diffrec_chain: too many workgroups at B=%lld N=%lld", (long long)B, (long long)N);
  DrEpilogue ep = {};
  ep.bias = g0;
  ep.e = e_next;
  ep.prev = p;
  ep.ldp = ldp;
  ep.c1 = c1;
  ep.c2 = c2;
  ep.out0 = p_next;
  ep.out1 = z_next;
  ep.ldo = ldo;
  hipLaunchKernelGGL(dr_tile_kernel<DR_CHAIN>, dim3((unsigned)g.blocks), dim3(256), 0, (hipStream_t)stream, z, ldz, G, ldg, B, N, K, g.MT, g.NT, ep);
  return check_launch("dr_tile_kernel<chain>");
}
