// MVGAE (Model/MVGAE.py): the conv epilogue and the product-of-experts / KL / BPR tail.  gfx950, fp32, D = 64.
//
// Geometry, everywhere: a row of 64 floats is held by 16 lanes, one float4 each (16-byte accesses); a wave holds
// MG_RW = 4 rows, a workgroup of 256 threads MG_RB = 16 rows; grids are ceil(rows / 16).  A row's sums are a 16-lane
// butterfly (xor 8, 4, 2, 1), the same on every run.  No atomics.  LDS: 128 bytes of KL partials in mg_tail_rows_kernel, 2 112
// bytes (256 + 8 doubles) in the single workgroup of mg_tail_final_kernel.
//
// The draws: key = draw_key(seed, state[1], salt); state[1] is the step counter chaorec_mvgae_tick advanced (state[0] += 1,
// state[1] = state[0]).  A draw is a function of (seed, step, salt, counters) alone, so a backward redraws its forward's.
//   dropout of conv `salt` in 0..14: element (r, d) is KEPT when draw_uniform<24>(key, 0, r * 64 + d) >= 0.1
//   noise of view x in (P, V, T, C) = 0..3: salt 16 + x (apart from the convs'), eps_x[r][d] = draw_normal<24>(key, r, d) --
//   keyed by the table ROW: two batch slots that name one row see one noise row, as the reference's whole-table draw gives.
//
// (a) conv epilogue (BaseModel.update + the leaky_relu around it), per row r:
//   a = s[r] + bias, n = sqrt(sum_d a^2), q = a / max(n, 1e-12), y = leaky_relu(q * m, 0.01); m = 1 / 0.9 for a kept element,
//   0 for a dropped one, 1 in evaluation.  keep != NULL: uint8 [N, 64] given flags (training only).
//   backward: gq = gy * (q m > 0 ? 1 : 0.01) * m;  gs = (gq - q sum_d(gq q)) / n for n >= 1e-12, gq / 1e-12 below.  q, n and m are
//   recomputed from s and bias: nothing but s is kept.  The bias gradient is the caller's column sum of gs.
//
// (b) tail.  PoE(ma, la, mb, lb): ta = 1 / (exp(la) + 1e-8), tb likewise; mean (ma ta + mb tb) / (ta + tb), log-variance
//   log(1 / (ta + tb)).  (M1, L1) = PoE(V, T), (Pm, Pl) = PoE((M1, L1), C).  Per view x: lc = min(l_x, 10),
//   KL_x = -0.5 / N sum (1 + lc - m^2 - exp(lc)), z_x[r] = m_x[r] + (eps_x[r] * 0.1) * exp(0.5 lc) (training; m_x[r] otherwise),
//   BPR_x = -1 / B sum_b log(sigmoid(<z_u, z_p> - <z_u, z_n>) + 1e-5), total = sum BPR_x + kl_weight sum KL_x.
//   chaorec_mvgae_tail_fwd_f32, three launches:
//     1 mg_tail_rows_kernel   all rows: writes Pm [N, 64] and per workgroup four KL partials (double, summed lane -> row ->
//                             wave -> workgroup in that fixed order) into workspace[blk * 4 + x]
//     2 mg_tail_batch_kernel  16 lanes per sample: the z rows of its three slots in four views -> zrows [4, 3, B, 64] (slot
//                             kind 0 = user, 1 = positive, 2 = negative), eps_out likewise if not NULL, bpr[x * B + b] = the
//                             sample's term, coef[x * B + b] = dBPR_x / d(score difference) (1 / B included).  The PoE, the
//                             z rows, the two scores, the term and the coefficient of these 3B rows are evaluated in
//                             double and rounded once when stored
//     3 mg_tail_final_kernel  one workgroup, in double, the fixed order of vae_sum_kernel: thread t adds the entries t, t + 256,
//                             ... ascending, then a shared-memory tree over the 256 threads; out[0] = total,
//                             out[1..4] = BPR_P, V, T, C, out[5..8] = KL_P, V, T, C
//   Every output is written whole; nothing needs zeroing.  workspace: chaorec_mvgae_tail_workspace_bytes(N), 8-byte aligned.
//   eps != NULL: given noise [4, N, 64] in the order P, V, T, C.  Row ids must lie in [0, N); they are clamped into it for
//   memory safety only.
//   chaorec_mvgae_tail_bwd_f32, ONE launch, row r of all six gradient tables owned by one lane group: the KL terms of r in
//   the four views; plus, over the slots perm[slot_ptr[r] .. slot_ptr[r + 1]) -- perm = a stable sort of the 3B ids
//   [users; pos; neg], so r's slots come as user, positive, negative, each in ascending sample order (the order of
//   chaorec_bpr_bwd_ordered_f32) -- dz_x += coef (z_p - z_n) | coef z_u | -coef z_u, one running fp32 sum per element; then
//   the reparametrisation (the clamp passes gradient where l <= 10, equality included), the two PoE stages, all times
//   gtotal[0].  A row without slots draws no noise.  All six tables are written whole.
#include "draws.h"

namespace chaorec {

constexpr int MG_D = 64;          // the row width
constexpr int MG_RW = 4;          // rows per wave
constexpr int MG_RB = 16;         // rows per workgroup
constexpr int MG_VIEWS = 4;       // P, V, T, C
constexpr uint64_t MG_VIEW_SALT = 16;
constexpr float MG_E = 1e-8f, MG_MAX_LOGVAR = 10.f, MG_DROP = 0.1f, MG_KEEP_SCALE = 1.0f / 0.9f, MG_SLOPE = 0.01f;

struct f4 {
  float v[4];
};
__device__ __forceinline__ f4 mg_ld(const float *__restrict__ p) {
  const float4 x = *reinterpret_cast<const float4 *>(p);
  return {{x.x, x.y, x.z, x.w}};
}
__device__ __forceinline__ void mg_st(float *__restrict__ p, const f4 &a) {
  *reinterpret_cast<float4 *>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
}

// the dropout multiplier of the four elements (r, d0 .. d0 + 3)
__device__ __forceinline__ f4 mg_mult(const uint8_t *__restrict__ keep, uint64_t key, int training, int64_t r, int d0) {
  f4 m;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bool k = true;
    if (training) k = keep ? keep[r * MG_D + d0 + j] != 0 : draw_uniform<24>(key, 0, (uint64_t)(r * MG_D + d0 + j)) >= MG_DROP;
    m.v[j] = training ? (k ? MG_KEEP_SCALE : 0.f) : 1.f;
  }
  return m;
}

template <bool BWD>
__global__ __launch_bounds__(256) void mg_conv_kernel(const float *__restrict__ gy, const float *__restrict__ s, const float *__restrict__ bias,
                                                      int64_t N, const uint8_t *__restrict__ keep, uint64_t seed,
                                                      const int64_t *__restrict__ state, uint64_t salt, int training, float *__restrict__ out) {
  const int64_t r0 = (int64_t)blockIdx.x * MG_RB + (threadIdx.x >> 4);
  const bool valid = r0 < N;
  const int64_t r = valid ? r0 : N - 1;
  const int d0 = (threadIdx.x & 15) * 4;
  const f4 x = mg_ld(s + r * MG_D + d0), b = mg_ld(bias + d0);
  f4 a, q, y;
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a.v[j] = x.v[j] + b.v[j];
    ss += a.v[j] * a.v[j];
  }
  const float n = sqrtf(group_sum<16>(ss)), dn = fmaxf(n, 1e-12f);
  const f4 m = mg_mult(keep, training ? draw_key(seed, (uint64_t)state[1], salt) : 0, training, r, d0);
#pragma unroll
  for (int j = 0; j < 4; ++j) q.v[j] = a.v[j] / dn;
  if constexpr (!BWD) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = q.v[j] * m.v[j];
      y.v[j] = t > 0.f ? t : t * MG_SLOPE;
    }
  } else {
    const f4 g = mg_ld(gy + r * MG_D + d0);
    f4 gq;
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = q.v[j] * m.v[j];
      gq.v[j] = g.v[j] * (t > 0.f ? 1.f : MG_SLOPE) * m.v[j];
      dot += gq.v[j] * q.v[j];
    }
    dot = group_sum<16>(dot);
#pragma unroll
    for (int j = 0; j < 4; ++j) y.v[j] = n >= 1e-12f ? (gq.v[j] - q.v[j] * dot) / n : gq.v[j] / 1e-12f;
  }
  if (valid) mg_st(out + r * MG_D + d0, y);
}

// one element of a product of experts
struct MgPoe {
  float ea, eb, ta, tb, S, m, l;
};
__device__ __forceinline__ MgPoe mg_poe(float ma, float la, float mb, float lb) {
  MgPoe p;
  p.ea = expf(la);
  p.eb = expf(lb);
  p.ta = 1.f / (p.ea + MG_E);
  p.tb = 1.f / (p.eb + MG_E);
  p.S = p.ta + p.tb;
  p.m = (ma * p.ta + mb * p.tb) / p.S;
  p.l = logf(1.f / p.S);
  return p;
}
// (gm, gl) of its outputs -> the gradients of its four inputs
__device__ __forceinline__ void mg_poe_bwd(const MgPoe &p, float ma, float mb, float gm, float gl, float &gma, float &gla, float &gmb,
                                           float &glb) {
  const float invS = 1.f / p.S;
  gma = gm * p.ta * invS;
  gmb = gm * p.tb * invS;
  const float gta = (gm * (ma - p.m) - gl) * invS, gtb = (gm * (mb - p.m) - gl) * invS;
  gla = gta * -(p.ta * p.ta * p.ea);
  glb = gtb * -(p.tb * p.tb * p.eb);
}

struct MgTables {
  const float *Vm, *Vl, *Tm, *Tl, *Cm, *Cl;
};
// means and log-variances of the four views (P, V, T, C) at the elements (r, d0 .. d0 + 3)
struct MgViews {
  f4 m[MG_VIEWS], l[MG_VIEWS];
};
__device__ __forceinline__ MgViews mg_views(const MgTables &t, int64_t r, int d0) {
  MgViews w;
  const int64_t o = r * MG_D + d0;
  w.m[1] = mg_ld(t.Vm + o);
  w.l[1] = mg_ld(t.Vl + o);
  w.m[2] = mg_ld(t.Tm + o);
  w.l[2] = mg_ld(t.Tl + o);
  w.m[3] = mg_ld(t.Cm + o);
  w.l[3] = mg_ld(t.Cl + o);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const MgPoe p1 = mg_poe(w.m[1].v[j], w.l[1].v[j], w.m[2].v[j], w.l[2].v[j]);
    const MgPoe p2 = mg_poe(p1.m, p1.l, w.m[3].v[j], w.l[3].v[j]);
    w.m[0].v[j] = p2.m;
    w.l[0].v[j] = p2.l;
  }
  return w;
}

__device__ __forceinline__ float mg_eps(const float *__restrict__ eps, uint64_t seed, uint64_t step, int x, int64_t N, int64_t r, int d) {
  if (eps) return eps[((int64_t)x * N + r) * MG_D + d];
  return draw_normal<24>(draw_key(seed, step, MG_VIEW_SALT + (uint64_t)x), (uint64_t)r, (uint64_t)d);
}

__global__ __launch_bounds__(256) void mg_tail_rows_kernel(MgTables t, int64_t N, float *__restrict__ Pm, double *__restrict__ partial) {
  __shared__ double red[4][MG_VIEWS];
  const int64_t r0 = (int64_t)blockIdx.x * MG_RB + (threadIdx.x >> 4);
  const bool valid = r0 < N;
  const int64_t r = valid ? r0 : N - 1;
  const int d0 = (threadIdx.x & 15) * 4;
  const MgViews w = mg_views(t, r, d0);
  if (valid) mg_st(Pm + r * MG_D + d0, w.m[0]);
#pragma unroll
  for (int x = 0; x < MG_VIEWS; ++x) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float lc = fminf(w.l[x].v[j], MG_MAX_LOGVAR), m = w.m[x].v[j];
      acc += (double)(1.f + lc - m * m - expf(lc));
    }
    if (!valid) acc = 0.0;
    acc = group_sum<64>(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][x] = acc;
  }
  __syncthreads();
  if (threadIdx.x < MG_VIEWS)
    partial[(int64_t)blockIdx.x * MG_VIEWS + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void mg_tail_batch_kernel(MgTables t, int64_t N, const int64_t *__restrict__ users, const int64_t *__restrict__ pos,
                                                            const int64_t *__restrict__ neg, int64_t B, const float *__restrict__ eps, uint64_t seed,
                                                            const int64_t *__restrict__ state, int training, float *__restrict__ zrows,
                                                            float *__restrict__ eps_out, float *__restrict__ bpr, float *__restrict__ coef) {
  const int64_t b0 = (int64_t)blockIdx.x * MG_RB + (threadIdx.x >> 4);
  const bool valid = b0 < B;
  const int64_t b = valid ? b0 : B - 1;
  const int d0 = (threadIdx.x & 15) * 4;
  const uint64_t step = (uint64_t)state[1];
  const int64_t rows[3] = {clamp_index(users[b], N), clamp_index(pos[b], N), clamp_index(neg[b], N)};
  // The z rows and the scores in DOUBLE (3B rows only): a sample's coefficient is as sensitive to its score difference as
  // 1 : 1, and fp32 z rows of magnitude 30 leave that difference with an error of 1e-5 and more.  The rows kept for the
  // backward are these values rounded once.
  double zu[MG_VIEWS][4], dp[MG_VIEWS], dq[MG_VIEWS];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t o = rows[k] * MG_D + d0;
    const f4 Vm = mg_ld(t.Vm + o), Vl = mg_ld(t.Vl + o), Tm = mg_ld(t.Tm + o), Tl = mg_ld(t.Tl + o), Cm = mg_ld(t.Cm + o), Cl = mg_ld(t.Cl + o);
    double acc[MG_VIEWS] = {0.0, 0.0, 0.0, 0.0};
    f4 zf[MG_VIEWS], ef[MG_VIEWS];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double tv = 1.0 / (exp((double)Vl.v[j]) + 1e-8), tt = 1.0 / (exp((double)Tl.v[j]) + 1e-8), tc = 1.0 / (exp((double)Cl.v[j]) + 1e-8);
      const double S1 = tv + tt, m1 = ((double)Vm.v[j] * tv + (double)Tm.v[j] * tt) / S1, l1 = log(1.0 / S1);
      const double t1 = 1.0 / (exp(l1) + 1e-8), S2 = t1 + tc;
      const double m[MG_VIEWS] = {(m1 * t1 + (double)Cm.v[j] * tc) / S2, (double)Vm.v[j], (double)Tm.v[j], (double)Cm.v[j]};
      const double l[MG_VIEWS] = {log(1.0 / S2), (double)Vl.v[j], (double)Tl.v[j], (double)Cl.v[j]};
#pragma unroll
      for (int x = 0; x < MG_VIEWS; ++x) {
        double zz = m[x];
        float e = 0.f;
        if (training) {
          e = mg_eps(eps, seed, step, x, N, rows[k], d0 + j);
          zz = zz + ((double)e * 0.1) * exp(fmin(l[x], 10.0) * 0.5);
        }
        zf[x].v[j] = (float)zz;
        ef[x].v[j] = e;
        if (k == 0) zu[x][j] = zz;
        else acc[x] += zu[x][j] * zz;
      }
    }
#pragma unroll
    for (int x = 0; x < MG_VIEWS; ++x) {
      const int64_t oz = (((int64_t)x * 3 + k) * B + b) * MG_D + d0;
      if (valid) {
        mg_st(zrows + oz, zf[x]);
        if (eps_out) mg_st(eps_out + oz, ef[x]);
      }
      if (k == 1) dp[x] = acc[x];
      if (k == 2) dq[x] = acc[x];
    }
  }
#pragma unroll
  for (int x = 0; x < MG_VIEWS; ++x) {
    const double p = group_sum<16>(dp[x]), q = group_sum<16>(dq[x]);
    const double diff = p - q, e = exp(-diff), sg = 1.0 / (1.0 + e);
    const double om = e < 1.0 ? e / (1.0 + e) : 1.0 - sg;      // 1 - sigmoid without the cancellation near 1
    if (valid && (threadIdx.x & 15) == 0) {
      bpr[(int64_t)x * B + b] = (float)-log(sg + 1e-5);
      coef[(int64_t)x * B + b] = (float)(-(sg * om) / (sg + 1e-5) / (double)B);
    }
  }
}

__global__ __launch_bounds__(256) void mg_tail_final_kernel(const double *__restrict__ partial, int64_t nblk, int64_t N, const float *__restrict__ bpr,
                                                            int64_t B, float kl_weight, float *__restrict__ out) {
  __shared__ double red[256];
  __shared__ double parts[2 * MG_VIEWS];
  for (int p = 0; p < 2 * MG_VIEWS; ++p) {
    double v = 0.0;
    if (p < MG_VIEWS) {
      for (int64_t i = threadIdx.x; i < B; i += 256) v += (double)bpr[(int64_t)p * B + i];
    } else {
      for (int64_t i = threadIdx.x; i < nblk; i += 256) v += partial[i * MG_VIEWS + (p - MG_VIEWS)];
    }
    block_sum_f64(v, red);
    if (threadIdx.x == 0) parts[p] = p < MG_VIEWS ? red[0] / (double)B : red[0] * (-0.5 / (double)N);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double bsum = 0.0, ksum = 0.0;
    for (int x = 0; x < MG_VIEWS; ++x) {
      bsum += parts[x];
      ksum += parts[MG_VIEWS + x];
      out[1 + x] = (float)parts[x];
      out[1 + MG_VIEWS + x] = (float)parts[MG_VIEWS + x];
    }
    out[0] = (float)(bsum + (double)kl_weight * ksum);
  }
}

struct MgGrads {
  float *Vm, *Vl, *Tm, *Tl, *Cm, *Cl;
};

__global__ __launch_bounds__(256) void mg_tail_bwd_kernel(MgTables t, int64_t N, const int64_t *__restrict__ slot_ptr, const int64_t *__restrict__ perm,
                                                          int64_t B, const float *__restrict__ zrows, const float *__restrict__ coef,
                                                          const float *__restrict__ eps, uint64_t seed, const int64_t *__restrict__ state, int training,
                                                          float kl_weight, const float *__restrict__ gtotal, MgGrads g) {
  const int64_t r0 = (int64_t)blockIdx.x * MG_RB + (threadIdx.x >> 4);
  const bool valid = r0 < N;
  const int64_t r = valid ? r0 : N - 1;
  const int d0 = (threadIdx.x & 15) * 4;
  const int64_t o = r * MG_D + d0;
  const f4 Vm = mg_ld(t.Vm + o), Vl = mg_ld(t.Vl + o), Tm = mg_ld(t.Tm + o), Tl = mg_ld(t.Tl + o), Cm = mg_ld(t.Cm + o), Cl = mg_ld(t.Cl + o);
  const int64_t lo = slot_ptr[r], hi = valid ? slot_ptr[r + 1] : lo;
  f4 dz[MG_VIEWS];
#pragma unroll
  for (int x = 0; x < MG_VIEWS; ++x) dz[x] = {{0.f, 0.f, 0.f, 0.f}};
  for (int64_t q = lo; q < hi; ++q) {
    const int64_t slot = perm[q], kind = slot / B, b = slot - kind * B;
#pragma unroll
    for (int x = 0; x < MG_VIEWS; ++x) {
      const float c = coef[(int64_t)x * B + b];
      const float *zx = zrows + ((int64_t)x * 3 * B + b) * MG_D + d0;     // kind k at zx + k B 64
      if (kind == 0) {
        const f4 zp = mg_ld(zx + B * MG_D), zn = mg_ld(zx + 2 * B * MG_D);
#pragma unroll
        for (int j = 0; j < 4; ++j) dz[x].v[j] += c * (zp.v[j] - zn.v[j]);
      } else {
        const f4 zu = mg_ld(zx);
        const float cs = kind == 1 ? c : -c;
#pragma unroll
        for (int j = 0; j < 4; ++j) dz[x].v[j] += cs * zu.v[j];
      }
    }
  }
  const bool noisy = training && hi > lo;
  const uint64_t step = (uint64_t)state[1];
  const float gt = gtotal[0], invN = 1.0f / (float)N;
  f4 oVm, oVl, oTm, oTl, oCm, oCl;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const MgPoe p1 = mg_poe(Vm.v[j], Vl.v[j], Tm.v[j], Tl.v[j]);
    const MgPoe p2 = mg_poe(p1.m, p1.l, Cm.v[j], Cl.v[j]);
    const float m[MG_VIEWS] = {p2.m, Vm.v[j], Tm.v[j], Cm.v[j]}, l[MG_VIEWS] = {p2.l, Vl.v[j], Tl.v[j], Cl.v[j]};
    float gm[MG_VIEWS], gl[MG_VIEWS];
#pragma unroll
    for (int x = 0; x < MG_VIEWS; ++x) {
      const float lc = fminf(l[x], MG_MAX_LOGVAR);
      gm[x] = dz[x].v[j] + kl_weight * (m[x] * invN);
      float v = kl_weight * ((-0.5f * invN) * (1.f - expf(lc)));
      if (noisy) v += dz[x].v[j] * ((mg_eps(eps, seed, step, x, N, r, d0 + j) * 0.1f) * (0.5f * expf(lc * 0.5f)));
      gl[x] = l[x] <= MG_MAX_LOGVAR ? v : 0.f;
    }
    float gM1, gL1, gc_m, gc_l, gv_m, gv_l, gt_m, gt_l;
    mg_poe_bwd(p2, p1.m, Cm.v[j], gm[0], gl[0], gM1, gL1, gc_m, gc_l);
    mg_poe_bwd(p1, Vm.v[j], Tm.v[j], gM1, gL1, gv_m, gv_l, gt_m, gt_l);
    oVm.v[j] = gt * (gm[1] + gv_m);
    oVl.v[j] = gt * (gl[1] + gv_l);
    oTm.v[j] = gt * (gm[2] + gt_m);
    oTl.v[j] = gt * (gl[2] + gt_l);
    oCm.v[j] = gt * (gm[3] + gc_m);
    oCl.v[j] = gt * (gl[3] + gc_l);
  }
  if (valid) {
    mg_st(g.Vm + o, oVm);
    mg_st(g.Vl + o, oVl);
    mg_st(g.Tm + o, oTm);
    mg_st(g.Tl + o, oTl);
    mg_st(g.Cm + o, oCm);
    mg_st(g.Cl + o, oCl);
  }
}

static int64_t mg_blocks(int64_t rows) { return (rows + MG_RB - 1) / MG_RB; }

}  // namespace chaorec

using namespace chaorec;

extern "C" int chaorec_mvgae_check_shape(int32_t D) {
  if (D != MG_D) return fail(CHAOREC_E_INVALID, "mvgae_check_shape: D=%d, the kernels tile D=%d", (int)D, MG_D);
  return CHAOREC_OK;
}

extern "C" int64_t chaorec_mvgae_rows_per_wave(void) { return MG_RW; }
extern "C" int64_t chaorec_mvgae_rows_per_block(void) { return MG_RB; }

extern "C" int chaorec_mvgae_tick(int64_t *state, void *stream) {
  return launch_step_tick("mvgae_tick", state, stream);
}

extern "C" int chaorec_mvgae_conv_fwd_f32(const float *s, const float *bias, int64_t N, const uint8_t *keep, uint64_t seed, const int64_t *state,
                                          int32_t salt, int32_t training, float *y, void *stream) {
  if (!s || !bias || !state || !y) return fail(CHAOREC_E_INVALID, "mvgae_conv_fwd: NULL argument");
  if (N <= 0 || salt < 0 || salt >= (int32_t)MG_VIEW_SALT) return fail(CHAOREC_E_INVALID, "mvgae_conv_fwd: N=%lld salt=%d", (long long)N, (int)salt);
  hipLaunchKernelGGL((mg_conv_kernel<false>), dim3((unsigned)mg_blocks(N)), dim3(256), 0, (hipStream_t)stream, (const float *)nullptr, s, bias, N, keep,
                     seed, state, (uint64_t)salt, (int)training, y);
  return check_launch("mg_conv_kernel<fwd>");
}

extern "C" int chaorec_mvgae_conv_bwd_f32(const float *gy, const float *s, const float *bias, int64_t N, const uint8_t *keep, uint64_t seed,
                                          const int64_t *state, int32_t salt, int32_t training, float *gs, void *stream) {
  if (!gy || !s || !bias || !state || !gs) return fail(CHAOREC_E_INVALID, "mvgae_conv_bwd: NULL argument");
  if (N <= 0 || salt < 0 || salt >= (int32_t)MG_VIEW_SALT) return fail(CHAOREC_E_INVALID, "mvgae_conv_bwd: N=%lld salt=%d", (long long)N, (int)salt);
  hipLaunchKernelGGL((mg_conv_kernel<true>), dim3((unsigned)mg_blocks(N)), dim3(256), 0, (hipStream_t)stream, gy, s, bias, N, keep, seed, state,
                     (uint64_t)salt, (int)training, gs);
  return check_launch("mg_conv_kernel<bwd>");
}

extern "C" size_t chaorec_mvgae_tail_workspace_bytes(int64_t N) { return (size_t)mg_blocks(N > 0 ? N : 1) * MG_VIEWS * sizeof(double); }

extern "C" int chaorec_mvgae_tail_fwd_f32(const float *Vm, const float *Vl, const float *Tm, const float *Tl, const float *Cm, const float *Cl,
                                          int64_t N, const int64_t *users, const int64_t *pos, const int64_t *neg, int64_t B, const float *eps,
                                          uint64_t seed, const int64_t *state, int32_t training, float kl_weight, float *Pm, float *zrows,
                                          float *eps_out, float *bpr, float *coef, void *workspace, size_t workspace_bytes, float *out,
                                          void *stream) {
  if (!Vm || !Vl || !Tm || !Tl || !Cm || !Cl || !users || !pos || !neg || !state || !Pm || !zrows || !bpr || !coef || !workspace || !out)
    return fail(CHAOREC_E_INVALID, "mvgae_tail_fwd: NULL argument");
  if (N <= 0 || B <= 0) return fail(CHAOREC_E_INVALID, "mvgae_tail_fwd: N=%lld B=%lld", (long long)N, (long long)B);
  if (workspace_bytes < chaorec_mvgae_tail_workspace_bytes(N) || (reinterpret_cast<uintptr_t>(workspace) & 7))
    return fail(CHAOREC_E_WORKSPACE, "mvgae_tail_fwd: workspace of %zu bytes, %zu needed, 8-byte aligned", workspace_bytes,
                chaorec_mvgae_tail_workspace_bytes(N));
  hipStream_t st = (hipStream_t)stream;
  const MgTables t{Vm, Vl, Tm, Tl, Cm, Cl};
  const int64_t nblk = mg_blocks(N);
  hipLaunchKernelGGL(mg_tail_rows_kernel, dim3((unsigned)nblk), dim3(256), 0, st, t, N, Pm, (double *)workspace);
  int rc = check_launch("mg_tail_rows_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(mg_tail_batch_kernel, dim3((unsigned)mg_blocks(B)), dim3(256), 0, st, t, N, users, pos, neg, B, eps, seed, state, (int)training,
                     zrows, eps_out, bpr, coef);
  rc = check_launch("mg_tail_batch_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(mg_tail_final_kernel, dim3(1), dim3(256), 0, st, (const double *)workspace, nblk, N, (const float *)bpr, B, kl_weight, out);
  return check_launch("mg_tail_final_kernel");
}

extern "C" int chaorec_mvgae_tail_bwd_f32(const float *Vm, const float *Vl, const float *Tm, const float *Tl, const float *Cm, const float *Cl,
                                          int64_t N, const int64_t *slot_ptr, const int64_t *perm, int64_t B, const float *zrows, const float *coef,
                                          const float *eps, uint64_t seed, const int64_t *state, int32_t training, float kl_weight,
                                          const float *gtotal, float *dVm, float *dVl, float *dTm, float *dTl, float *dCm, float *dCl,
                                          void *stream) {
  if (!Vm || !Vl || !Tm || !Tl || !Cm || !Cl || !slot_ptr || !perm || !zrows || !coef || !state || !gtotal || !dVm || !dVl || !dTm || !dTl ||
      !dCm || !dCl)
    return fail(CHAOREC_E_INVALID, "mvgae_tail_bwd: NULL argument");
  if (N <= 0 || B <= 0) return fail(CHAOREC_E_INVALID, "mvgae_tail_bwd: N=%lld B=%lld", (long long)N, (long long)B);
  const MgTables t{Vm, Vl, Tm, Tl, Cm, Cl};
  const MgGrads g{dVm, dVl, dTm, dTl, dCm, dCl};
  hipLaunchKernelGGL(mg_tail_bwd_kernel, dim3((unsigned)mg_blocks(N)), dim3(256), 0, (hipStream_t)stream, t, N, slot_ptr, perm, B, zrows, coef, eps,
                     seed, state, (int)training, kl_weight, gtotal, g);
  return check_launch("mg_tail_bwd_kernel");
}
