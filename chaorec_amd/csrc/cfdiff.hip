// CF_Diff's attention core (Model/CF_Diff.py:108-111: nn.MultiheadAttention(16, 4, dropout=0.5) with the second-hop tokens
// as queries and the first-hop tokens as keys and values) without an [L, L] array.  Additive to ABI 16.  fp32 VALU, no
// atomics on floats, no scratch; every output row has one owner and every sum a fixed order: the same bits every run.
//
// q, k, v, out and their gradients are [B, L, 16], head h in columns 4h .. 4h + 3; scores are <q, k> / 2.  A workgroup
// owns one (b, head): its 4 waves stage what the lanes read at a uniform address in LDS, once, and then walk tiles of
// CF_TILE = 128 owners, two per lane (owner t0 + lane and t0 + 64 + lane), so one broadcast ds_read_b128 serves two
// (owner, other) pairs.
//
// (a) cf_fwd_kernel    lane = query.  LDS: k, v (32 B per token).  Pass 1 the row maximum, pass 2 p = 2^(s2 - m2), their
//                      sum over ALL keys, and the kept p v; out = (2 or 1) acc / l, lse = (m2 + log2 l) ln 2.
// (b) cf_bwd_q_kernel  lane = query.  LDS as (a).  p = 2^(s2 - lse2); dq = (1/2) (1 / sum p) sum_j dS_ij k_j and
//                      rnorm[b, h, i] = 1 / sum p: the fp32 lse is half an ulp of ~7 off, which scales every p of the row
//                      by one factor -- the row's own sum takes it out again, for (c) too.
// (c) cf_bwd_kv_kernel lane = key.  LDS: per query (q C, dout, lse2, rnorm, D) (48 B per token).  dk, dv.
// (d) cf_keep_kernel   the flags of the device draws as bytes (tests, the plain composition).
//
// Every sum over the other side runs in ascending index order in segments of CF_SEG = 32: a segment's value is formed from
// zero and added to the running total, segments ascending (a single chain over 1034 terms rounds at the magnitude of its
// growing partial sum 1034 times).  s2 = <q C, k> with C = log2(e) / 2 folded into q once: v_exp_f32 is the only
// transcendental of a pair.
//
// The device-drawn keep flags: flag (b, head, query i, key j) is bit (j & 63) of
//   draw_bits64(draw_key(seed, state[1], salt), (b0 + b) * 4 + head, (i << 20) | (j >> 6))
// -- one 64-bit draw serves the 64 keys of an aligned key word, set bit = kept (rate 1/2).  b0 is the slot of the launch's
// first row: a row's flags do not depend on the launch it is part of.  (a), (b) hold the draw of (query, word) in the
// query's lane, once per word; (c) draws the tile's two key words of 32 queries in the 64 lanes (word u in lanes 32 u ..)
// and reads them back lane by lane.
#include "draws.h"

namespace chaorec {

constexpr int CF_THREADS = 256, CF_WAVES = 4;
constexpr int CF_TILE = 128;                       // owners per wave and tile: two per lane
constexpr int CF_SEG = 32;                         // terms per segment of a sum
constexpr int CF_KV_BYTES = 32, CF_Q_BYTES = 48;   // LDS per token: (a), (b) / (c)
constexpr int CF_LDS_BYTES = 64 * 1024;            // per workgroup: two of them are resident on a CU (160 KiB) at ANY accepted L
constexpr int CF_MAX_LEN = CF_LDS_BYTES / CF_Q_BYTES;   // 1365
constexpr float CF_C = 0.72134752044448170368f;    // log2(e) / 2
constexpr float CF_LOG2E = 1.44269504088896340736f, CF_LN2 = 0.69314718055994530942f;

__device__ __forceinline__ float cf_dot(const float4 a, const float4 b) { return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x))); }
__device__ __forceinline__ void cf_axpy(float4 &y, float a, const float4 x) {
  y.x = fmaf(a, x.x, y.x);
  y.y = fmaf(a, x.y, y.y);
  y.z = fmaf(a, x.z, y.z);
  y.w = fmaf(a, x.w, y.w);
}
__device__ __forceinline__ void cf_add(float4 &y, const float4 x) {
  y.x += x.x;
  y.y += x.y;
  y.z += x.z;
  y.w += x.w;
}
__device__ __forceinline__ float4 cf_scale(const float4 x, float a) { return make_float4(x.x * a, x.y * a, x.z * a, x.w * a); }
__device__ __forceinline__ float4 cf_row(const float *__restrict__ p, int64_t token, int h) {
  return *reinterpret_cast<const float4 *>(p + token * 16 + 4 * h);
}
__device__ __forceinline__ uint64_t cf_draw(uint64_t key, uint64_t a, int query, int word) {
  return draw_bits64(key, a, ((uint64_t)query << 20) | (uint64_t)word);
}

// MODE 0: no dropout (training == 0); 1: device-drawn flags; 2: given flags keep uint8 [B, 4, L, L]
template <int MODE>
static __global__ __launch_bounds__(CF_THREADS) void cf_fwd_kernel(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, int n, const uint8_t *__restrict__ keep,
    uint64_t seed, const int64_t *__restrict__ state, uint64_t salt, int64_t b0, float *__restrict__ out, float *__restrict__ lse) {
  extern __shared__ float4 cf_sm[];
  float4 *ks = cf_sm, *vs = cf_sm + n;
  const int64_t bh = blockIdx.x, b = bh >> 2, tok0 = b * n;
  const int h = (int)(bh & 3), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < n; j += CF_THREADS) {
    ks[j] = cf_row(k, tok0 + j, h);
    vs[j] = cf_row(v, tok0 + j, h);
  }
  __syncthreads();
  uint64_t key = 0, a = 0;
  if constexpr (MODE == 1) {
    key = draw_key(seed, (uint64_t)state[1], salt);
    a = ((uint64_t)(b0 + b) << 2) | (uint64_t)h;
  }
  for (int t0 = wave * CF_TILE; t0 < n; t0 += CF_WAVES * CF_TILE) {
    int iq[2], ic[2];
    float4 qs[2], acc[2];
    float m[2], l[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      iq[u] = t0 + 64 * u + lane;
      ic[u] = iq[u] < n ? iq[u] : n - 1;             // a lane past the end computes the last query and stores nothing
      qs[u] = cf_scale(cf_row(q, tok0 + ic[u], h), CF_C);
      m[u] = -INFINITY;
      l[u] = 0.f;
      acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int j = 0; j < n; ++j) {
      const float4 kj = ks[j];
#pragma unroll
      for (int u = 0; u < 2; ++u) m[u] = fmaxf(m[u], cf_dot(qs[u], kj));
    }
    uint64_t word[2] = {0, 0};
    for (int j0 = 0; j0 < n; j0 += CF_SEG) {
      const int cnt = n - j0 < CF_SEG ? n - j0 : CF_SEG;
      uint32_t bits[2] = {~0u, ~0u};
      if constexpr (MODE == 1) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if ((j0 & 32) == 0) word[u] = cf_draw(key, a, ic[u], j0 >> 6);      // one draw serves the word's two segments
          bits[u] = (uint32_t)(word[u] >> (j0 & 32));
        }
      }
      float cl[2] = {0.f, 0.f};
      float4 ca[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
      for (int jj = 0; jj < cnt; ++jj) {
        const int j = j0 + jj;
        const float4 kj = ks[j], vj = vs[j];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float p = __builtin_amdgcn_exp2f(cf_dot(qs[u], kj) - m[u]);
          cl[u] += p;
          bool kept = true;
          if constexpr (MODE == 1) kept = (bits[u] >> jj) & 1u;
          if constexpr (MODE == 2) kept = keep[(bh * n + ic[u]) * n + j] != 0;
          cf_axpy(ca[u], kept ? p : 0.f, vj);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        l[u] += cl[u];
        cf_add(acc[u], ca[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (iq[u] >= n) continue;
      const float sc = (MODE ? 2.f : 1.f) / l[u];    // l >= 1: the maximum's own term
      *reinterpret_cast<float4 *>(out + (tok0 + iq[u]) * 16 + 4 * h) = cf_scale(acc[u], sc);
      lse[bh * n + iq[u]] = (m[u] + __builtin_amdgcn_logf(l[u])) * CF_LN2;      // v_log_f32 is log2
    }
  }
}

template <int MODE>
static __global__ __launch_bounds__(CF_THREADS) void cf_bwd_q_kernel(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, const float *__restrict__ out,
    const float *__restrict__ lse, const float *__restrict__ dout, int n, const uint8_t *__restrict__ keep, uint64_t seed,
    const int64_t *__restrict__ state, uint64_t salt, int64_t b0, float *__restrict__ dq, float *__restrict__ rnorm) {
  extern __shared__ float4 cf_sm[];
  float4 *ks = cf_sm, *vs = cf_sm + n;
  const int64_t bh = blockIdx.x, b = bh >> 2, tok0 = b * n;
  const int h = (int)(bh & 3), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = threadIdx.x; j < n; j += CF_THREADS) {
    ks[j] = cf_row(k, tok0 + j, h);
    vs[j] = cf_row(v, tok0 + j, h);
  }
  __syncthreads();
  uint64_t key = 0, a = 0;
  if constexpr (MODE == 1) {
    key = draw_key(seed, (uint64_t)state[1], salt);
    a = ((uint64_t)(b0 + b) << 2) | (uint64_t)h;
  }
  constexpr float F = MODE ? 2.f : 1.f;
  for (int t0 = wave * CF_TILE; t0 < n; t0 += CF_WAVES * CF_TILE) {
    int iq[2], ic[2];
    float4 qs[2], go[2], acc[2];
    float D[2], ls2[2], l[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      iq[u] = t0 + 64 * u + lane;
      ic[u] = iq[u] < n ? iq[u] : n - 1;
      qs[u] = cf_scale(cf_row(q, tok0 + ic[u], h), CF_C);
      go[u] = cf_row(dout, tok0 + ic[u], h);
      D[u] = cf_dot(go[u], cf_row(out, tok0 + ic[u], h));
      ls2[u] = lse[bh * n + ic[u]] * CF_LOG2E;
      l[u] = 0.f;
      acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    uint64_t word[2] = {0, 0};
    for (int j0 = 0; j0 < n; j0 += CF_SEG) {
      const int cnt = n - j0 < CF_SEG ? n - j0 : CF_SEG;
      uint32_t bits[2] = {~0u, ~0u};
      if constexpr (MODE == 1) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if ((j0 & 32) == 0) word[u] = cf_draw(key, a, ic[u], j0 >> 6);      // one draw serves the word's two segments
          bits[u] = (uint32_t)(word[u] >> (j0 & 32));
        }
      }
      float cl[2] = {0.f, 0.f};
      float4 ca[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
      for (int jj = 0; jj < cnt; ++jj) {
        const int j = j0 + jj;
        const float4 kj = ks[j], vj = vs[j];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float p = __builtin_amdgcn_exp2f(cf_dot(qs[u], kj) - ls2[u]);
          cl[u] += p;
          bool kept = true;
          if constexpr (MODE == 1) kept = (bits[u] >> jj) & 1u;
          if constexpr (MODE == 2) kept = keep[(bh * n + ic[u]) * n + j] != 0;
          const float t = kept ? F * cf_dot(go[u], vj) : 0.f;
          cf_axpy(ca[u], p * (t - D[u]), kj);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        l[u] += cl[u];
        cf_add(acc[u], ca[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (iq[u] >= n) continue;
      const float r = 1.f / l[u];
      *reinterpret_cast<float4 *>(dq + (tok0 + iq[u]) * 16 + 4 * h) = cf_scale(acc[u], 0.5f * r);
      rnorm[bh * n + iq[u]] = r;
    }
  }
}

template <int MODE>
static __global__ __launch_bounds__(CF_THREADS) void cf_bwd_kv_kernel(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v, const float *__restrict__ out,
    const float *__restrict__ lse, const float *__restrict__ dout, const float *__restrict__ rnorm, int n,
    const uint8_t *__restrict__ keep, uint64_t seed, const int64_t *__restrict__ state, uint64_t salt, int64_t b0,
    float *__restrict__ dk, float *__restrict__ dv) {
  extern __shared__ float4 cf_sm[];           // per query: q C | dout | (lse2, rnorm, D, 0)
  const int64_t bh = blockIdx.x, b = bh >> 2, tok0 = b * n;
  const int h = (int)(bh & 3), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < n; i += CF_THREADS) {
    const float4 go = cf_row(dout, tok0 + i, h);
    cf_sm[3 * i] = cf_scale(cf_row(q, tok0 + i, h), CF_C);
    cf_sm[3 * i + 1] = go;
    cf_sm[3 * i + 2] = make_float4(lse[bh * n + i] * CF_LOG2E, rnorm[bh * n + i], cf_dot(go, cf_row(out, tok0 + i, h)), 0.f);
  }
  __syncthreads();
  uint64_t key = 0, a = 0;
  if constexpr (MODE == 1) {
    key = draw_key(seed, (uint64_t)state[1], salt);
    a = ((uint64_t)(b0 + b) << 2) | (uint64_t)h;
  }
  constexpr float F = MODE ? 2.f : 1.f;
  for (int t0 = wave * CF_TILE; t0 < n; t0 += CF_WAVES * CF_TILE) {
    int jk[2], jc[2];
    float4 kj[2], vj[2], ak[2], av[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      jk[u] = t0 + 64 * u + lane;                 // bit `lane` of key word (t0 >> 6) + u
      jc[u] = jk[u] < n ? jk[u] : n - 1;
      kj[u] = cf_row(k, tok0 + jc[u], h);
      vj[u] = cf_row(v, tok0 + jc[u], h);
      ak[u] = av[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int i0 = 0; i0 < n; i0 += CF_SEG) {
      const int cnt = n - i0 < CF_SEG ? n - i0 : CF_SEG;
      int lo = 0, hi = 0;
      if constexpr (MODE == 1) {                  // lane l < 32 draws the tile's first key word of query i0 + l, lane l + 32 its second
        const int il = i0 + (lane & 31) < n ? i0 + (lane & 31) : n - 1;
        const uint64_t r = cf_draw(key, a, il, (t0 >> 6) + (lane >> 5));
        lo = (int)(uint32_t)r;
        hi = (int)(uint32_t)(r >> 32);
      }
      float4 ck[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
      float4 cv[2] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
      for (int ii = 0; ii < cnt; ++ii) {
        const int i = i0 + ii;
        const float4 qi = cf_sm[3 * i], gi = cf_sm[3 * i + 1], si = cf_sm[3 * i + 2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float p = __builtin_amdgcn_exp2f(cf_dot(qi, kj[u]) - si.x) * si.y;
          bool kept = true;
          if constexpr (MODE == 1) {
            const uint64_t r = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, ii + 32 * u) << 32) |
                               (uint64_t)(uint32_t)__builtin_amdgcn_readlane(lo, ii + 32 * u);
            kept = (r >> lane) & 1ull;
          }
          if constexpr (MODE == 2) kept = keep[(bh * n + i) * n + jc[u]] != 0;
          const float t = kept ? F * cf_dot(gi, vj[u]) : 0.f;
          cf_axpy(ck[u], p * (t - si.z), qi);           // the query pass's expression: one key gives t == D and an exact zero
          cf_axpy(cv[u], kept ? F * p : 0.f, gi);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        cf_add(ak[u], ck[u]);
        cf_add(av[u], cv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (jk[u] >= n) continue;
      *reinterpret_cast<float4 *>(dk + (tok0 + jk[u]) * 16 + 4 * h) = cf_scale(ak[u], CF_LN2);     // (1/2) / C
      *reinterpret_cast<float4 *>(dv + (tok0 + jk[u]) * 16 + 4 * h) = av[u];
    }
  }
}

template <class = void>
static __global__ __launch_bounds__(256) void cf_keep_kernel(int64_t total, int n, int nw, uint64_t seed, const int64_t *__restrict__ state,
                                                             uint64_t salt, int64_t b0, uint8_t *__restrict__ keep) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int w = (int)(t % nw), i = (int)((t / nw) % n);
  const int64_t bh = t / ((int64_t)nw * n);
  const uint64_t r = cf_draw(draw_key(seed, (uint64_t)state[1], salt), ((uint64_t)(b0 + (bh >> 2)) << 2) | (uint64_t)(bh & 3), i, w);
  for (int jj = 0; jj < 64 && 64 * w + jj < n; ++jj) keep[(bh * n + i) * n + 64 * w + jj] = (uint8_t)((r >> jj) & 1ull);
}

}  // namespace chaorec

using namespace chaorec;

extern "C" int64_t chaorec_cfdiff_max_len(void) { return CF_MAX_LEN; }

extern "C" int chaorec_cfdiff_check_shape(int64_t B, int64_t L) {
  if (L < 1 || L > CF_MAX_LEN)
    return fail(CHAOREC_E_INVALID, "cfdiff: L=%lld; a workgroup stages %d bytes per token in at most %d of LDS: 1 .. %d", (long long)L,
                CF_Q_BYTES, CF_LDS_BYTES, CF_MAX_LEN);
  if (B < 1 || B > ((int64_t)1 << 28)) return fail(CHAOREC_E_INVALID, "cfdiff: B=%lld", (long long)B);
  return CHAOREC_OK;
}

static int cf_check_draws(const char *what, int64_t B, int32_t training, const uint8_t *keep, const int64_t *state, int64_t b0) {
  if (training && !keep && !state) return fail(CHAOREC_E_INVALID, "%s: device draws without a state", what);
  if (b0 < 0 || b0 + B > ((int64_t)1 << 30)) return fail(CHAOREC_E_INVALID, "%s: b0=%lld", what, (long long)b0);
  return CHAOREC_OK;
}

extern "C" int chaorec_cfdiff_attn_fwd_f32(const float *q, const float *k, const float *v, int64_t B, int64_t L, int32_t training,
                                           const uint8_t *keep, uint64_t seed, const int64_t *state, uint32_t salt, int64_t b0,
                                           float *out, float *lse, void *stream) {
  if (int rc = chaorec_cfdiff_check_shape(B, L)) return rc;
  if (!q || !k || !v || !out || !lse) return fail(CHAOREC_E_INVALID, "cfdiff_attn_fwd: NULL argument");
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out))
    return fail(CHAOREC_E_INVALID, "cfdiff_attn_fwd: q, k, v, out must be 16-byte aligned");
  if (int rc = cf_check_draws("cfdiff_attn_fwd", B, training, keep, state, b0)) return rc;
  const dim3 grid((unsigned)(4 * B)), block(CF_THREADS);
  const size_t lds = (size_t)L * CF_KV_BYTES;
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)L;
  if (!training) hipLaunchKernelGGL(cf_fwd_kernel<0>, grid, block, lds, st, q, k, v, n, keep, seed, state, (uint64_t)salt, b0, out, lse);
  else if (!keep) hipLaunchKernelGGL(cf_fwd_kernel<1>, grid, block, lds, st, q, k, v, n, keep, seed, state, (uint64_t)salt, b0, out, lse);
  else hipLaunchKernelGGL(cf_fwd_kernel<2>, grid, block, lds, st, q, k, v, n, keep, seed, state, (uint64_t)salt, b0, out, lse);
  return check_launch("cf_fwd_kernel");
}

extern "C" int chaorec_cfdiff_attn_bwd_f32(const float *q, const float *k, const float *v, const float *out, const float *lse,
                                           const float *dout, int64_t B, int64_t L, int32_t training, const uint8_t *keep,
                                           uint64_t seed, const int64_t *state, uint32_t salt, int64_t b0, float *dq, float *dk,
                                           float *dv, float *rnorm, void *stream) {
  if (int rc = chaorec_cfdiff_check_shape(B, L)) return rc;
  if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || !rnorm) return fail(CHAOREC_E_INVALID, "cfdiff_attn_bwd: NULL argument");
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || !aligned16(dout) || !aligned16(dq) ||
      !aligned16(dk) || !aligned16(dv))
    return fail(CHAOREC_E_INVALID, "cfdiff_attn_bwd: the [B, L, 16] operands must be 16-byte aligned");
  if (int rc = cf_check_draws("cfdiff_attn_bwd", B, training, keep, state, b0)) return rc;
  const dim3 grid((unsigned)(4 * B)), block(CF_THREADS);
  const size_t lds_q = (size_t)L * CF_KV_BYTES, lds_kv = (size_t)L * CF_Q_BYTES;
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)L;
  const uint64_t s = salt;
  if (!training) hipLaunchKernelGGL(cf_bwd_q_kernel<0>, grid, block, lds_q, st, q, k, v, out, lse, dout, n, keep, seed, state, s, b0, dq, rnorm);
  else if (!keep) hipLaunchKernelGGL(cf_bwd_q_kernel<1>, grid, block, lds_q, st, q, k, v, out, lse, dout, n, keep, seed, state, s, b0, dq, rnorm);
  else hipLaunchKernelGGL(cf_bwd_q_kernel<2>, grid, block, lds_q, st, q, k, v, out, lse, dout, n, keep, seed, state, s, b0, dq, rnorm);
  if (int rc = check_launch("cf_bwd_q_kernel")) return rc;
  if (!training) hipLaunchKernelGGL(cf_bwd_kv_kernel<0>, grid, block, lds_kv, st, q, k, v, out, lse, dout, rnorm, n, keep, seed, state, s, b0, dk, dv);
  else if (!keep) hipLaunchKernelGGL(cf_bwd_kv_kernel<1>, grid, block, lds_kv, st, q, k, v, out, lse, dout, rnorm, n, keep, seed, state, s, b0, dk, dv);
  else hipLaunchKernelGGL(cf_bwd_kv_kernel<2>, grid, block, lds_kv, st, q, k, v, out, lse, dout, rnorm, n, keep, seed, state, s, b0, dk, dv);
  return check_launch("cf_bwd_kv_kernel");
}

extern "C" int chaorec_cfdiff_attn_keep_u8(int64_t B, int64_t L, uint64_t seed, const int64_t *state, uint32_t salt, int64_t b0,
                                           uint8_t *keep, void *stream) {
  if (int rc = chaorec_cfdiff_check_shape(B, L)) return rc;
  if (!state || !keep) return fail(CHAOREC_E_INVALID, "cfdiff_attn_keep: NULL argument");
  if (int rc = cf_check_draws("cfdiff_attn_keep", B, 1, nullptr, state, b0)) return rc;
  const int nw = (int)((L + 63) / 64);
  const int64_t total = 4 * B * L * nw, blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return fail(CHAOREC_E_INVALID, "cfdiff_attn_keep: %lld workgroups", (long long)blocks);
  hipLaunchKernelGGL(cf_keep_kernel<>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total, (int)L, nw, seed, state,
                     (uint64_t)salt, b0, keep);
  return check_launch("cf_keep_kernel");
}
