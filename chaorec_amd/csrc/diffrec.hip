// DiffRec's two hot paths (Model/DiffRec.py:263-303, 425-463): the denoiser's output layer with the importance-weighted x0
// loss and the complete gradient by the layer's output in one pass, and one step of the sampling chain collapsed to the
// hidden width.  Additive to ABI 16.  fp32, no atomics on floats, no scratch, the same bits every run.
//
// (a) dr_tile_kernel<DR_LOSS>   d_out = c_b (h W_out^T + b_out - x0), per-row partials of err^2 per item tile
// (b) dr_reduce_kernel          the row partials in item-tile order -> reloss_rows (double), loss = mean_b reloss_b / pt_b
// (c) dr_tile_kernel<DR_CHAIN>  p_next = c1 (z G^T + g0) + c2 p,  z_next = tanh(p_next + e_next)
//
// One tile loop serves both: acc = A[m0 .., 0 .. K) . Bm[n0 .., 0 .. K)^T on v_mfma_f32_32x32x2_f32, both operands
// [rows][k], staged k-major in LDS and double-buffered, 128 x 128 x 16 per workgroup (waves 2 x 2 of 64 x 64).  The k chain
// of an element is cut into segments of DR_SEG = 64 whose values are added in ascending order, as csrc/diffmm.hip's output
// layer does and for its measured reason (one chain over K = 1000 deviated 4 to 5 times as much as a blocked sum).
#include "vae_common.h"

namespace chaorec {

constexpr int DR_BM = 128, DR_BN = 128, DR_BK = 16, DR_PAD = 4;
constexpr int DR_SEG = 64;        // k per segment of a chain (a multiple of DR_BK)
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

// Workgroups are dealt to the 8 XCDs round-robin: block id -> (id % 8, id / 8), and the workgroups of one XCD walk the row
// tiles of one column tile before the next, so a slice of Bm is read into one L2 and A stays in all of them.
template <int EPI>
static __global__ __launch_bounds__(256) void dr_tile_kernel(const float *__restrict__ A, int64_t lda, const float *__restrict__ Bm,
                                                             int64_t ldb, int64_t M, int64_t N, int64_t K, int64_t MT, int64_t NT,
                                                             DrEpilogue ep) {
  __shared__ float As[2][DR_BK][DR_BM + DR_PAD];
  __shared__ float Bs[2][DR_BK][DR_BN + DR_PAD];
  __shared__ float Ps[2][DR_BM];
  const int64_t slot = (int64_t)blockIdx.x >> 3;
  const int64_t nt = (slot / MT) * 8 + ((int64_t)blockIdx.x & 7), mt = slot % MT;
  if (nt >= NT) return;           // the whole workgroup: no barrier has been reached
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int rr = lane & 31, hh = lane >> 5;
  const int wrow = (wave >> 1) * 64, wcol = (wave & 1) * 64;
  const int64_t m0 = mt * DR_BM, n0 = nt * DR_BN;

  f32x16 acc[2][2], sum[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = sum[i][j] = vae_zero();

  float4 ra[2], rb[2];
  auto fetch = [&](int64_t k0) {      // K is a multiple of 4 and rows are 16-byte aligned: a float4 is inside or outside
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int v = t + p * 256, row = v >> 2, k4 = (v & 3) * 4;
      const int64_t gk = k0 + k4;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
      if (m0 + row < M && gk < K) x = *reinterpret_cast<const float4 *>(A + (m0 + row) * lda + gk);
      if (n0 + row < N && gk < K) y = *reinterpret_cast<const float4 *>(Bm + (n0 + row) * ldb + gk);
      ra[p] = x;
      rb[p] = y;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int v = t + p * 256, row = v >> 2, k4 = (v & 3) * 4;
      As[buf][k4 + 0][row] = ra[p].x;
      As[buf][k4 + 1][row] = ra[p].y;
      As[buf][k4 + 2][row] = ra[p].z;
      As[buf][k4 + 3][row] = ra[p].w;
      Bs[buf][k4 + 0][row] = rb[p].x;
      Bs[buf][k4 + 1][row] = rb[p].y;
      Bs[buf][k4 + 2][row] = rb[p].z;
      Bs[buf][k4 + 3][row] = rb[p].w;
    }
  };
  int buf = 0;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int64_t k0 = 0; k0 < K; k0 += DR_BK) {
    const bool more = k0 + DR_BK < K;
    if (more) fetch(k0 + DR_BK);
    float af[DR_BK / 2][2], bf[DR_BK / 2][2];
#pragma unroll
    for (int s = 0; s < DR_BK / 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[s][i] = As[buf][2 * s + hh][wrow + 32 * i + rr];
        bf[s][i] = Bs[buf][2 * s + hh][wcol + 32 * i + rr];
      }
#pragma unroll
    for (int s = 0; s < DR_BK / 2; ++s)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s][i], bf[s][j], acc[i][j], 0, 0, 0);
    if (((k0 + DR_BK) % DR_SEG) == 0) {     // a segment is complete: into the running sum, the chain restarts from zero
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          sum[i][j] = sum[i][j] + acc[i][j];
          acc[i][j] = vae_zero();
        }
    }
    if (more) stash(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = sum[i][j] + acc[i][j];      // the last, partial segment (zero when K % 64 == 0)

  if constexpr (EPI == DR_LOSS) {
    // err = (acc + b_out[i]) - x0[b, i] (x0 from the bit table: the 32 columns of a lane group are one word), the tile's share
    // of sum_i err^2 per row: columns in a fixed butterfly order, then the two column halves in order; acc = c_b err
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = wrow + 32 * i + vae_row(reg, hh);
        const int64_t gm = m0 + row;
        const float cb = gm < M ? ep.c_row[gm] : 0.f;
        float sq = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int64_t g0 = n0 + wcol + 32 * j, gn = g0 + rr;
          float err = 0.f;
          if (gm < M && gn < N) {
            const uint32_t word = ep.bits[gm * ep.nwords + (g0 >> 5)];
            const float x0 = ((word >> rr) & 1u) ? 1.f : 0.f;
            err = (acc[i][j][reg] + ep.bias[gn]) - x0;
          }
          sq = sq + err * err;
          acc[i][j][reg] = cb * err;
        }
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) sq = sq + __shfl_xor(sq, off, 64);   // within the 32 lanes that hold the row
        if (rr == 0) Ps[wave & 1][row] = sq;
      }
    }
    __syncthreads();
    if (t < DR_BM && m0 + t < M) ep.part[(m0 + t) * NT + nt] = Ps[0][t] + Ps[1][t];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t gn = n0 + wcol + 32 * j + rr;
        if (gn >= ep.ldo) continue;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int64_t gm = m0 + wrow + 32 * i + vae_row(reg, hh);
          if (gm < M) ep.out0[gm * ep.ldo + gn] = gn < N ? acc[i][j][reg] : 0.f;
        }
      }
  } else {
    // p_next = fl(fl(c1 fl(acc + g0)) + fl(c2 p)), z_next = fl(tanh(fl(p_next + e_next))), the tanh itself evaluated in double:
    // B N evaluations against the tile's 2 B N K flops.  Every element has one owner.
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int64_t gn = n0 + wcol + 32 * j + rr;
        if (gn >= N) continue;
        const float g0 = ep.bias[gn], en = ep.e[gn];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int64_t gm = m0 + wrow + 32 * i + vae_row(reg, hh);
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

static bool dr_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the launch grid of a tile kernel over [M, N]; 0: too many workgroups
static int64_t dr_blocks(int64_t M, int64_t N, int64_t *MT, int64_t *NT) {
  *MT = (M + DR_BM - 1) / DR_BM;
  *NT = (N + DR_BN - 1) / DR_BN;
  const int64_t blocks = (*NT + 7) / 8 * *MT * 8;
  return blocks > 0x7fffffff ? 0 : blocks;
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
  *bm = DR_BM;
  *bn = DR_BN;
  *bk = DR_BK;
  return CHAOREC_OK;
}

extern "C" int chaorec_diffrec_out_loss_f32(const float *h, int64_t ldh, const float *W_out, int64_t ldw, const float *b_out,
                                            const uint32_t *bits, const double *w, const double *pt, const float *c_row,
                                            int64_t B, int64_t I, int64_t H, float *d_out, int64_t ldd, float *part,
                                            double *reloss_rows, float *loss, void *stream) {
  if (!h || !W_out || !b_out || !bits || !w || !pt || !c_row || !d_out || !part || !reloss_rows || !loss)
    return fail(CHAOREC_E_INVALID, "diffrec_out_loss: NULL argument");
  if (int rc = chaorec_diffrec_check_shape(B, I, H)) return rc;
  if (ldh < H || ldw < H || (ldh & 3) || (ldw & 3) || ldd < I || !dr_aligned16(h) || !dr_aligned16(W_out))
    return fail(CHAOREC_E_INVALID, "diffrec_out_loss: h, W_out must be 16-byte aligned with row strides that are multiples of 4, ldd >= I");
  int64_t MT, NT;
  const int64_t blocks = dr_blocks(B, I, &MT, &NT);
  if (!blocks) return fail(CHAOREC_E_INVALID, "diffrec_out_loss: too many workgroups at B=%lld I=%lld", (long long)B, (long long)I);
  if (ldd > NT * DR_BN) return fail(CHAOREC_E_INVALID, "diffrec_out_loss: ldd=%lld past the last item tile", (long long)ldd);
  DrEpilogue ep = {};
  ep.bias = b_out;
  ep.bits = bits;
  ep.nwords = (I + 31) / 32;
  ep.c_row = c_row;
  ep.part = part;
  ep.out0 = d_out;
  ep.ldo = ldd;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dr_tile_kernel<DR_LOSS>, dim3((unsigned)blocks), dim3(256), 0, st, h, ldh, W_out, ldw, B, I, H, MT, NT, ep);
  if (int rc = check_launch("dr_tile_kernel<loss>")) return rc;
  hipLaunchKernelGGL(dr_reduce_kernel<>, dim3(1), dim3(256), 0, st, part, NT, w, pt, B, I, reloss_rows, loss);
  return check_launch("dr_reduce_kernel");
}

extern "C" int chaorec_diffrec_chain_f32(const float *z, int64_t ldz, const float *G, int64_t ldg, const float *g0, const float *p,
                                         int64_t ldp, const float *e_next, float c1, float c2, int64_t B, int64_t N, int64_t K,
                                         float *p_next, float *z_next, int64_t ldo, void *stream) {
  if (!z || !G || !g0 || !p || !e_next || !p_next || !z_next) return fail(CHAOREC_E_INVALID, "diffrec_chain: NULL argument");
  if (int rc = chaorec_diffrec_check_shape(B, N, K)) return rc;
  if (ldz < K || ldg < K || (ldz & 3) || (ldg & 3) || ldp < N || ldo < N || !dr_aligned16(z) || !dr_aligned16(G))
    return fail(CHAOREC_E_INVALID, "diffrec_chain: z, G must be 16-byte aligned with row strides that are multiples of 4, ldp, ldo >= N");
  if (p_next == z_next || p_next == z || z_next == z || z_next == p)
    return fail(CHAOREC_E_INVALID, "diffrec_chain: the outputs must not alias each other or an operand another workgroup reads");
  int64_t MT, NT;
  const int64_t blocks = dr_blocks(B, N, &MT, &NT);
  if (!blocks) return fail(CHAOREC_E_INVALID, "diffrec_chain: too many workgroups at B=%lld N=%lld", (long long)B, (long long)N);
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
  hipLaunchKernelGGL(dr_tile_kernel<DR_CHAIN>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, ldz, G, ldg, B, N, K, MT, NT, ep);
  return check_launch("dr_tile_kernel<chain>");
}
