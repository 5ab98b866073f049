// The device-drawn layer: the counter RNG over common.h's mix64 and the step counter its draws are keyed by.  One
// definition of the bits of a draw; every file that draws on the device includes this (the autoencoders through
// vae_common.h).  A draw depends on its counters only, never on launch geometry: a replayed graph whose step counter moved
// draws fresh values and a backward redraws its forward's.
// The kernels here are static templates: a file that launches one has its own copy (the link sees no duplicate), a file
// that does not has none -- `template <class = void>` is there for that alone.
#pragma once
#include "common.h"

namespace chaorec {

// (seed, step, salt) -> key; (key, a, b) -> uniform STRICTLY inside (0, 1), BITS random bits + 0.5 (exact in fp32 for
// BITS <= 24; log(-log(u)) is finite)
__device__ __forceinline__ uint64_t draw_key(uint64_t seed, uint64_t step, uint64_t salt) { return mix64(mix64(seed ^ salt) + step); }
template <int BITS>
__device__ __forceinline__ float draw_uniform(uint64_t key, uint64_t a, uint64_t b) {
  const uint64_t r = mix64(key ^ mix64((a << 32) ^ b));
  return ((float)(r >> (64 - BITS)) + 0.5f) * (1.0f / (float)(1 << BITS));
}
// the 64 bits draw_uniform cuts its value from: 64 fair coins of (key, a, b) (cfdiff.hip's rate-1/2 keep flags)
__device__ __forceinline__ uint64_t draw_bits64(uint64_t key, uint64_t a, uint64_t b) { return mix64(key ^ mix64((a << 32) ^ b)); }
template <int BITS>
__device__ __forceinline__ float draw_normal(uint64_t key, uint64_t a, uint64_t c) {   // Box-Muller
  const float u1 = draw_uniform<BITS>(key, a, 2 * c), u2 = draw_uniform<BITS>(key, a, 2 * c + 1);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

// the older keying (the negative sampler, the edge dropouts, the user graph's neighbour pick): 64 bits of (seed, step, x);
// each caller packs its own x (salts and shifts stay with it) and cuts its own bits from the result
__device__ __forceinline__ uint64_t draw_hash(uint64_t seed, uint64_t step, uint64_t x) { return mix64(seed ^ mix64(step ^ mix64(x))); }

// ---- the BPR sampler's draws (csrc/bpr.hip, csrc/bpr_frontier.hip) ----------------------------------------------------
// Counter-based: the draw_hash keying over (seed, step, b, attempt).  Stateless, so a draw does not depend on launch
// geometry or on how many draws other samples needed.
__device__ __forceinline__ uint32_t sampler_draw(uint64_t seed, uint64_t step, uint32_t b,
                                                 uint32_t attempt, uint32_t num_item) {
  uint64_t h = draw_hash(seed, step, ((uint64_t)b << 32) | attempt);
  // Lemire multiply-shift onto [0, num_item): bias <= num_item / 2^32, far below test resolution
  return (uint32_t)(((h >> 32) * (uint64_t)num_item) >> 32);
}

// sample b of batch `step`: a training edge picked uniformly (user, positive as LOCAL item id) and one negative the
// user has not interacted with (rejection against the ascending history row, bounded)
__device__ __forceinline__ void draw_triple(const int64_t *__restrict__ edges, int64_t n_edges,
                                            const int64_t *__restrict__ hist_rowptr,
                                            const int32_t *__restrict__ hist_col, int64_t num_user, uint32_t num_item,
                                            uint64_t seed, uint64_t step, uint32_t b, int64_t &u, int64_t &p,
                                            int64_t &n, const int64_t *__restrict__ perm,
                                            int64_t perm_pos) {
  uint64_t idx;
  if (perm) {
    // epoch permutation (DataLoader(shuffle=True)): every edge once.  A read position past the end (a caller that
    // draws more batches than the epoch holds) is clamped, never dereferenced.
    const int64_t q = perm_pos + (int64_t)b;
    idx = (uint64_t)perm[q < n_edges ? (q < 0 ? 0 : q) : n_edges - 1];
  } else {
    const uint64_t hsel = draw_hash(seed, step, 0xED6E5ull ^ ((uint64_t)b << 32));
    // 64x64 -> high 64 multiply-shift onto [0, n_edges)
    idx = (uint64_t)(((unsigned __int128)hsel * (unsigned __int128)(uint64_t)n_edges) >> 64);
  }
  u = edges[2 * idx];
  p = edges[2 * idx + 1] - num_user;
  const int64_t h0 = hist_rowptr[u], h1 = hist_rowptr[u + 1];
  uint32_t cand = 0;
  for (uint32_t attempt = 0;; ++attempt) {
    cand = sampler_draw(seed, step, b, attempt, num_item);
    int64_t lo = h0, hi = h1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((uint32_t)hist_col[mid] < cand) lo = mid + 1; else hi = mid;
    }
    const bool seen = (lo < h1) && ((uint32_t)hist_col[lo] == cand);
    if (!seen || attempt >= 4096u) break;
  }
  n = (int64_t)cand;
}

// out[e] = std * N(0, 1) keyed (seed, state[1], SALT, e) (the autoencoders' epsilon: it keeps their prefix, and its name)
template <int BITS, uint64_t SALT>
static __global__ __launch_bounds__(256) void vae_normal_kernel(float *__restrict__ out, int64_t n, uint64_t seed,
                                                                const int64_t *__restrict__ state, float std) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  out[e] = std * draw_normal<BITS>(draw_key(seed, (uint64_t)state[1], SALT), (uint64_t)e, 0);
}

// the step tick: state[0] += 1, state[1] = state[0] -- state[1] is the step the launches after it key their draws by
template <class = void>
static __global__ void step_tick_kernel(int64_t *state) {
  if (threadIdx.x || blockIdx.x) return;
  const int64_t c = state[0] + 1;
  state[0] = c;
  state[1] = c;
}
template <class = void>
static int launch_step_tick(const char *what, int64_t *state, void *stream) {
  if (!state) return fail(CHAOREC_E_INVALID, "%s: NULL argument", what);
  hipLaunchKernelGGL(step_tick_kernel<>, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
  return check_launch(what);
}

}  // namespace chaorec
