/*
 * chaorec_hip.h -- C-ABI of libchaorec_hip.so: the MI355X (gfx950) kernels under
 * ChaoRec's GCN-propagation + BPR-training + full-rank-evaluation hot path.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); kernels are
 *     only ENQUEUED, nothing here synchronises or allocates;
 *   - the caller owns every buffer, including workspaces (sizes from the *_workspace_bytes
 *     queries, which are host-only and launch nothing);
 *   - return value: 0 = ok, <0 = error (CHAOREC_E_*); chaorec_last_error() returns a
 *     host string describing the last failure on the calling thread;
 *   - row-major dense tables, fp32, leading dimension == D unless an ld* argument exists.
 *
 * The reference (Ricardo-Ping/ChaoRec) is pure Python with no FFI layer: each entry point
 * below names the reference library call it replaces (file:line relative to the reference
 * root).  The Python binding a maintainer adds is shown in INTEGRATION.md.
 */
#ifndef CHAOREC_HIP_H
#define CHAOREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CHAOREC_ABI_VERSION 16  /* 2: gemm workspace, score stats, rank metrics; 3: edge dropout, weighted sampling,
                                  row cosine, two-pass reductions, BPR forward with the batch drawn in the launch,
                                  SpMM dynamic-values mode, gemm act 2, 256-B aligned score workspace;
                                  4: SpMM with the Adam update in its epilogue, BPR forward + backward in one launch,
                                  stand-alone BPR finalize with loss / optimizer bookkeeping, layer mean in the last
                                  forward SpMM, scoring with carried thresholds, split-bf16 NT GEMM;
                                  5: weighted_sample_keys (sharded edge pruning);
                                  6: BPR batch at an offset + one finalize for k captured steps, NGCF elementwise backward;
                                  7: Adam over a feature table with a low-rank, row-sparse gradient (dense / lazy / flush), split-bf16 TN GEMM
                                     (weight gradients), multi-tensor Adam;
                                  8: rows_mean (layer mean of exchanged rows: fused sharded LightGCN step);
                                  9: split-bf16 NN GEMM (input gradients, accumulate epilogue), MMGCN's layer tail
                                     (leaky_cat_add / leaky_split_bwd), normalize_rows, multi-term BPR, draw_batch item_offset, shift_cat,
                                     peer-to-peer exchange kernels;
                                  10: multi-term BPR backward scatters the gradient of gathered row blocks itself;
                                  11: row-sparse backward propagates (row bitmaps written by the BPR launch, read by
                                      chaorec_spmm_csr_rowsparse_f32, cleared by chaorec_spmm_csr_adam_f32);
                                  12: the frontier-restricted step: chaorec_batch_rows (the batch before the forward), list
                                      launches with a layer-mean epilogue and workgroup-per-row launches for long rows,
                                      chaorec_expand_row_bits over rectangular blocks, rows_list_from_bits, rows_mean_by_bits,
                                      zero_rows_by_bits, rows_copy_by_bits, or_words, peer-to-peer exchange of flagged rows, frontier pack / unpack;
                                  13: scoring: CHAOREC_SCORE_FRONT / _BACK (one call as two phases), a raised-threshold pass for
                                      users whose candidate lists overflow (long item ranges), chaorec_score_topk_stats out10;
                                  14: chaorec_edge_dot_f32 (edge scores over a CSR's entries);
                                  15: ordered (atomic-free, run-to-run reproducible) BPR backward launches;
                                  16: chaorec_spmm_csr_rowlist_f32's long_cnt is int32[4] (column-striped very long rows) */

#define CHAOREC_OK 0
#define CHAOREC_E_INVALID (-1)     /* bad argument (NULL, negative size, unsupported D/K) */
#define CHAOREC_E_LAUNCH (-2)      /* hipLaunch / hipMemsetAsync reported an error */
#define CHAOREC_E_WORKSPACE (-3)   /* workspace too small */

int chaorec_abi_version(void);
const char *chaorec_last_error(void);

/* ---------------------------------------------------------------------------------------
 * P1/P7/P12: normalised-adjacency propagate  y = alpha * (A x) [+ beta * z],  A in CSR.
 *
 * Replaces: PyG MessagePassing.propagate = index_select + message (norm * x_j) + scatter_add
 *           (Model/LightGCN.py:40-43, BasicGCN.py:48-53,78-82) and torch.sparse.mm(adj, x)
 *           (Model/FREEDOM.py:168,174).
 *
 * Row r of the CSR is the DESTINATION node; its entries are the incoming edges in the
 * reference's edge order (stable sort by destination), so mode 0 reproduces the reference
 * CPU accumulation order:  s = 0; for e in row: s = s + (val[e] * x[col[e]])  -- product and
 * sum rounded separately (no FMA), exactly what message() then scatter_add_ do.
 * Epilogue, in this order, every step rounded to fp32:
 *     s = alpha * s                       (alpha == 1 is exact)
 *     if z:   s = s + (beta * z[r])
 *     y[r] = s                            (y may be NULL when only acc is wanted)
 *     if acc: a0 = acc_init ? (acc_w * acc_init[r]) : acc[r];   acc[r] = a0 + (acc_w * s)
 * The acc epilogue is LightGCN.forward's layer mean (Model/LightGCN.py:86-93):
 * final += (1/(L+1)) * x_l, with acc_init = x_0 on the first layer.
 * Backward (A symmetric for LightGCN/FREEDOM-ui/BasicGCN) is the same call with the
 * transposed CSR:  g_l = A^T g_{l+1} + beta * G.
 *
 * D must be a multiple of 4, 4 <= D <= 1024.  rowptr is int64 (nnz of config 5 > 2^31).
 * schedule (optional, may be NULL): the array built by chaorec_spmm_build_schedule() for this graph and D,
 *   copied to the device.  It fixes which workgroup walks which rows (longest rows first, one heavy group per
 *   workgroup) and carries a 64-B descriptor per row {row, degree, first entry, first 6 (col,val) pairs} so the
 *   kernel's dependent-load chain is descriptor -> x instead of order -> rowptr -> (col,val) -> x.  It changes
 *   scheduling and latency only, never results.
 * mode: 0 = ordered (bit-reproducible, reference order).  CHAOREC_SPMM_DYNAMIC_VALUES (1): same, but the schedule
 *   was built for this structure under OTHER values (the value array is rewritten every step, e.g. edge dropout):
 *   the kernel then ignores the values stored in the schedule and reads all of them from val[].
 * ------------------------------------------------------------------------------------- */
#define CHAOREC_SPMM_DYNAMIC_VALUES 1
int chaorec_spmm_csr_f32(const int64_t *rowptr, const int32_t *col, const float *val,
                         const float *x, float *y, int64_t n_rows, int64_t n_cols, int32_t D,
                         float alpha, const float *z, float beta,
                         float *acc, const float *acc_init, float acc_w,
                         const int32_t *schedule, int32_t mode, void *stream);

/* The LAST forward propagate of LightGCN.forward with the WHOLE layer mean in its epilogue (Model/LightGCN.py:86-93):
 *     s = (A x)[r];  a = w * terms[0][r];  a = a + w * terms[k][r] (k = 1 .. n_terms-1, in order);  mean_out[r] = a + w * s
 * -- the reference's accumulation order (final = 0 + w x_0 + w x_1 + ... + w x_L), every step rounded, so the result is
 * bit-identical to chaorec_spmm_csr_f32's per-layer acc epilogue; what it saves is that epilogue's read-modify-write of
 * the [N, D] mean in every earlier layer (terms = the earlier layers' outputs x_0 .. x_{L-1}, host array of DEVICE
 * pointers, n_terms <= 3, and <= 2 for D > 64: register budget).  y may be NULL (x_L itself is not needed). */
int chaorec_spmm_csr_mean_f32(const int64_t *rowptr, const int32_t *col, const float *val, const float *x,
                              float *y, int64_t n_rows, int64_t n_cols, int32_t D, float *mean_out,
                              const float *const *terms, int32_t n_terms, float w, const int32_t *schedule,
                              int32_t mode, void *stream);

/* The LAST backward propagate of a training step with the optimizer update in its epilogue
 * (train_and_evaluate.py:46-47: loss.backward(); optimizer.step(), for a model whose parameter table IS the
 * propagate's input: LightGCN, Model/LightGCN.py:76-95):
 *     g[r]   = alpha * (A x)[r] + beta * z[r]         -- chaorec_spmm_csr_f32's arithmetic, e.g. g_0 = A^T g_1 + w G
 *     Adam(param[r], g[r], exp_avg[r], exp_avg_sq[r]) -- chaorec_adam_step_f32's arithmetic, bit for bit
 * in one launch: no separate optimizer launch and no second pass over the gradient (grad_out may be NULL).
 * bias_corr: device float[2] = {1 - beta1^t, sqrt(1 - beta2^t)} of this step (chaorec_bpr_finalize_f32 writes it).
 * clear_z != 0: every row of z that was non-zero is zeroed after it was read -- z is then the batch gradient buffer
 * that chaorec_bpr_fwd_bwd_f32 adds into, kept all-zero between steps instead of being zero-filled every step
 * (refused when x == z: another wave could still gather the row).  D <= 256. */
/* clear_bits_a / _b (optional, n_words_* uint32 words each): row bitmaps of the row-sparse propagates below that this
 * launch zeroes as a side job -- it is the step's last launch, every reader of the step's bitmaps is done. */
int chaorec_spmm_csr_adam_f32(const int64_t *rowptr, const int32_t *col, const float *val, const float *x,
                              float *grad_out, int64_t n_rows, int64_t n_cols, int32_t D, float alpha,
                              float *z, float beta, const int32_t *schedule, int32_t mode, float *param,
                              float *exp_avg, float *exp_avg_sq, const float *bias_corr, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int32_t clear_z,
                              uint32_t *clear_bits_a, int64_t n_words_a, uint32_t *clear_bits_b, int64_t n_words_b,
                              void *stream);

/* The same launch with z read THROUGH A BITMAP (z = the batch gradient G: 3 B non-zero rows out of N): a row of z whose bit
 * in z_bits (n_words_z uint32 words, bit r & 31 of word r >> 5; a superset of z's non-zero rows) is clear is not loaded and
 * counts as +0, so param / moments / grad_out are chaorec_spmm_csr_adam_f32's bit for bit; clear_z zeroes exactly the flagged
 * rows that were non-zero, an unflagged row of z is neither read nor written.  z_bits may lie inside clear_bits_a / _b: a
 * gated launch clears them as its LAST act instead of at entry -- every workgroup takes a ticket from `ticket`
 * (CHAOREC_SPMM_TICKET_WORDS device uint32, zero on entry and zero again when the launch is done) after its rows are stored,
 * the workgroup that draws the last one clears.  z, z_bits (at least n_rows bits) and ticket are all required:
 * CHAOREC_E_INVALID otherwise. */
#define CHAOREC_SPMM_TICKET_WORDS 2080
int chaorec_spmm_csr_adam_gated_f32(const int64_t *rowptr, const int32_t *col, const float *val, const float *x,
                                    float *grad_out, int64_t n_rows, int64_t n_cols, int32_t D, float alpha,
                                    float *z, float beta, const int32_t *schedule, int32_t mode, float *param,
                                    float *exp_avg, float *exp_avg_sq, const float *bias_corr, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, int32_t clear_z,
                                    uint32_t *clear_bits_a, int64_t n_words_a, uint32_t *clear_bits_b, int64_t n_words_b,
                                    const uint32_t *z_bits, int64_t n_words_z, uint32_t *ticket, int64_t n_words_ticket,
                                    void *stream);

/* A backward propagate whose operands are ROW-SPARSE (train_and_evaluate.py:46 loss.backward() through
 * Model/LightGCN.py:81-83 for a BPR batch): the batch gradient G has 3 B non-zero rows out of N, the first backward
 * propagate's result is non-zero in their neighbours only.  Same arithmetic, entry order and result as
 * chaorec_spmm_csr_f32's  y = alpha (A x) + beta z  (bit for bit, up to the sign of an exact zero); the bitmaps only gate
 * LOADS: a source row whose bit in src_bits is clear is not gathered (its term is val * (+0)), a row of z whose bit in
 * z_bits is clear is not read.  A set bit means "may be non-zero": supersets are fine.  out_bits (optional, all-zero on
 * entry) receives such a superset for y.  Bitmaps: uint32 words, bit r & 31 of word r >> 5; any of the three may be NULL.
 * 64 <= D <= 256. */
/* row_bits (optional): a superset of the rows of y that can be non-zero -- normally chaorec_expand_row_bits of src_bits.
 * A row whose bit is clear (and whose z row is not flagged) walks no entries at all; it stores zeros when write_zeros != 0
 * (the next launch reads y densely) and nothing otherwise (the next launch gathers flagged rows only).  Per-entry bitmap
 * tests alone leave such a launch at ~80 % of the dense one (a 4-byte L2 request per entry instead of a row gather); with
 * the row mask its cost follows the frontier, not the graph. */
int chaorec_spmm_csr_rowsparse_f32(const int64_t *rowptr, const int32_t *col, const float *val, const float *x,
                                   float *y, int64_t n_rows, int64_t n_cols, int32_t D, float alpha, const float *z,
                                   float beta, const int32_t *schedule, int32_t mode, const uint32_t *src_bits,
                                   const uint32_t *z_bits, uint32_t *out_bits, const uint32_t *row_bits,
                                   int32_t write_zeros, void *stream);

/* The same propagate for a source with FEW non-zero rows over a graph small enough that the bitmap fits in LDS (the first
 * backward propagate of a BPR step, train_and_evaluate.py:46 loss.backward() through Model/LightGCN.py:81-83, on a graph like
 * sports: 3 B batch rows out of 44 147) -- csrc/spmm_fewsrc.hip.  y = alpha (A x) + beta z with EVERY row of y written and
 * only the flagged rows of x gathered / of z read: rows of x whose bit in src_bits is clear, and rows of z whose bit in z_bits
 * is clear, must hold +0 and are never loaded.  Bit for bit chaorec_spmm_csr_f32's result on the same operands (finite
 * values).  Every workgroup copies src_bits into LDS and tests every entry there; a row's lanes test different entries at
 * once.  A square graph (n_rows == n_cols, bitmaps over its rows: uint32 words, bit r & 31 of word r >> 5), its static
 * schedule (chaorec_spmm_build_schedule; no DYNAMIC_VALUES mode), D = 64, (n_rows + 31) / 32 words <= 48 KiB of LDS, x / y /
 * z 16-byte aligned; z and z_bits come together or not at all (z_bits == src_bits: tested in LDS too).  Anything else:
 * CHAOREC_E_INVALID. */
int chaorec_spmm_csr_fewsrc_f32(const int32_t *col, const float *val, const float *x, float *y, int64_t n_rows,
                                int64_t n_cols, int32_t D, float alpha, const float *z, float beta,
                                const int32_t *schedule, const uint32_t *src_bits, const uint32_t *z_bits, void *stream);

/* bits_out |= bits_self | {columns of the rows flagged in bits_in}: the rows a propagate can make non-zero when its source
 * is non-zero in the flagged rows only.  bits_in: a bitmap over the CSR's n_rows rows; bits_self (optional) and bits_out:
 * bitmaps over its n_out_rows COLUMNS (symmetric graph: bits_self = bits_in, n_out_rows = n_rows; a user shard's
 * rectangular blocks B_g / B_g^T: the batch rows of the other side).  Work ~ the flagged rows' entries.  list / list_n
 * (optional; *list_n zero on entry, list_cap entries): every row whose bit this launch sets first is also appended. */
int chaorec_expand_row_bits(const int64_t *rowptr, const int32_t *col, int64_t n_rows, const uint32_t *bits_in,
                            const uint32_t *bits_self, int64_t n_out_rows, uint32_t *bits_out, int32_t *list,
                            int32_t *list_n, int64_t list_cap, void *stream);

/* y[r, :] = 0 for every row flagged in `bits` (a buffer that is non-zero in a frontier's rows only goes back to all-zero
 * without a pass over the whole of it).  D a multiple of 4. */
int chaorec_zero_rows_by_bits_f32(float *y, int64_t n_rows, int32_t D, const uint32_t *bits, void *stream);

/* list[0 .. *list_n) = the rows flagged in `bits` (arbitrary order; *list_n zero on entry, list_cap entries): the work list
 * of a chaorec_spmm_csr_rowlist_f32 launch over a frontier that exists as a bitmap only. */
int chaorec_rows_list_from_bits(const uint32_t *bits, int64_t n_rows, int32_t *list, int32_t *list_n, int64_t list_cap,
                                void *stream);

/* out[r] = ((w t0[r] + w t1[r]) + ..) for the rows flagged in `bits` (chaorec_rows_mean_f32's association; n_terms <= 8): the
 * layer mean of Model/LightGCN.py:85-95 for a light step's item rows of a user shard. */
int chaorec_rows_mean_by_bits_f32(const float *const *terms, int32_t n_terms, float w, float *out, int64_t n_rows, int32_t D,
                                  const uint32_t *bits, void *stream);

/* dst[w] = src[0][w] | .. | src[n_src - 1][w] (src: n_src bitmaps of n_words words, back to back): the union of the ranks'
 * row bitmaps after an all-gather -- RCCL has no bitwise-or reduction.  dst may be one of the sources. */
int chaorec_or_words_u32(uint32_t *dst, const uint32_t *src, int32_t n_src, int64_t n_words, void *stream);

/* chaorec_spmm_csr_rowsparse_f32's arithmetic for the rows of a device-side LIST only (y[r] for r in list[0 .. *list_n); other
 * rows of y are not touched): the first backward propagate of a BPR step, whose output is non-zero in the 1-hop image of the
 * 3 B batch rows -- 1-2 % of the graph at BASELINE configs[4], where even a launch that only LOOKS at every row's descriptor
 * costs a third of the dense one.  One lane group per listed row, entries in CSR order, unflagged sources skipped (their
 * term is +0): bit-identical rows.  64 <= D <= 256. */
/* mean_out (optional; y may then be NULL): the layer mean of Model/LightGCN.py:85-95 for the listed rows,
 * mean_out[r] = ((w t0[r] + w t1[r]) + ..) + w y[r] over n_mean_terms <= 4 earlier-layer tables (chaorec_spmm_csr_mean_f32's
 * association): the LAST forward propagate of a training step, which needs the propagated table in its batch's rows only. */
int chaorec_spmm_csr_rowlist_f32(const int64_t *rowptr, const int32_t *col, const float *val, const float *x, float *y,
                                 int64_t n_rows, int32_t D, float alpha, const float *z, float beta, const uint32_t *src_bits,
                                 const uint32_t *z_bits, const int32_t *list, const int32_t *list_n, int64_t list_cap,
                                 float *mean_out, const float *const *mean_terms, int32_t n_mean_terms, float mean_w,
                                 int32_t *long_list, int32_t *long_cnt, int64_t long_cap, int32_t long_threshold,
                                 void *stream);
/* long_list / long_cnt (optional): listed rows with more than long_threshold entries are deferred to long_list (long_cap
 * entries; long_cnt: int32[4] since ABI 16, zero on entry and zero again afterwards) and computed by a second launch with one
 * WORKGROUP per row instead of being the tail of a 16..64-lane group (a popular item's row has 1e4-1e5 entries): without
 * src_bits (a forward propagate of a light step: every entry gathered) the gathers are shared by 256 threads and the products
 * summed in entry order through an LDS tile -- and a row above 8192 entries (CHAOREC_ROWLIST_STRIPE_T) by D / 32 workgroups,
 * one per 128-byte column stripe (a list of more than 65 536 rows: above four times that): the same chain of adds per output
 * element, D / 32 times the bytes in flight; with src_bits (the backward's first propagate) the workgroup scans 1024 entries per
 * round and queues the few flagged ones in entry order for one lane group to gather and add -- the sequential CSR-order sum
 * either way. */

/* destination rows handled by one wave64 for feature width D (host helper, launches nothing) */
int chaorec_spmm_rows_per_wave(int32_t D);
/* rows with more entries than this are walked cooperatively by their workgroup; a schedule built outside the library
 * (chaorec_amd/graph.py: schedule_tensors, the same words from tensor operations on the device) groups rows by it */
int chaorec_spmm_long_threshold(void);

/* Host-side schedule builder for chaorec_spmm_csr_f32 (HOST pointers, no GPU work): int32 elements needed,
 * and the build itself.  Graph-static: build once per (graph, D), keep the copy in HBM next to the CSR. */
int64_t chaorec_spmm_schedule_len(int64_t n_rows, int32_t D);
int chaorec_spmm_build_schedule(const int64_t *rowptr, const int32_t *col, const float *val,
                                int64_t n_rows, int32_t D, int32_t *out, int64_t out_len);

/* ---------------------------------------------------------------------------------------
 * P4/P5/P9/P13: fused BPR step on a batch of (user, pos, neg) triples.
 *
 * Replaces: three row gathers + mul + sum + log(sigmoid) + mean (+ L2 means)
 *           Model/LightGCN.py:97-121 (variant 0), Model/FREEDOM.py:185-192 (variant 1),
 *           Model/MMGCN.py:188-202 (variant 2) and their autograd backward (index_add).
 *
 * users[b] indexes rows of tab_u, pos[b]/neg[b] index rows of tab_i (LOCAL row ids).
 *   d_b  = sum_k u*p - sum_k u*n
 *   variant 0: t_b = log(sigmoid(d_b) + 1e-5)     variant 1: t_b = logsigmoid(d_b)
 *   variant 2: t_b = log(sigmoid(d_b))
 *   bpr  = -(1/B) sum_b t_b
 *   reg  = reg_weight * (mean(u^2) + mean(p^2) + mean(n^2)),  means over B*D  (0 if reg_weight==0)
 *   out_loss[0] = bpr + reg, out_loss[1] = bpr, out_loss[2] = reg;  out_total (optional, may be NULL) also
 *   receives bpr + reg as a stand-alone scalar (a separate allocation keeps the host-side autograd simple)
 *   coef[b] = d(bpr)/d(d_b)   (kept for the backward)
 * workspace: 4*B floats.  Reductions run in a fixed order: results are run-to-run identical.
 *
 * bwd: g_u[users[b]] += go*(coef_b*(p-n) + (2*reg_weight/(B*D))*u), g_i[pos[b]] += go*(coef_b*u + ..*p),
 *      g_i[neg[b]] += go*(-coef_b*u + ..*n);  go = *grad_out (device scalar) or 1 if NULL.
 *      Accumulated with fp32 atomics (duplicates inside a batch); g_u/g_i must be zeroed or
 *      hold the gradient being accumulated.
 * ------------------------------------------------------------------------------------- */
#define CHAOREC_BPR_LOG_SIGMOID_EPS 0
#define CHAOREC_BPR_LOGSIGMOID 1
#define CHAOREC_BPR_LOG_SIGMOID 2

int chaorec_bpr_fwd_f32(const float *tab_u, const float *tab_i,
                        const int64_t *users, const int64_t *pos, const int64_t *neg,
                        int32_t B, int32_t D, int32_t variant, float reg_weight,
                        float *out_loss, float *out_total, float *coef, float *workspace, void *stream);

int chaorec_bpr_bwd_f32(const float *tab_u, const float *tab_i,
                        const int64_t *users, const int64_t *pos, const int64_t *neg,
                        int32_t B, int32_t D, const float *coef, float reg_weight,
                        const float *grad_out, float *g_u, float *g_i, void *stream);
/* The same row sums WITHOUT atomics, reproducible run to run: every destination row has one owner wave that adds the row's
 * contributions in ascending (role, sample) order into ONE running float sum -- first the batch's contributions to
 * `emb[users]`, then to `emb[pos]`, then to `emb[neg]` (Model/LightGCN.py:113-121, Model/MMGCN.py:193-197), each in batch order: a
 * DEFINED order (oracle_bpr_bwd_ordered_f32 restates it), not torch's -- autograd sums the three index_select gradients as three
 * separately accumulated tensors, another association of the same addends.  fp32 atomic adds are applied in an order that
 * moves with the load on the chip; three addends in one element then differ in the last bit between runs, and Adam's first
 * steps turn that into a visible parameter difference.  Same arguments; g_u / g_i may alias (one joined table).  Falls back
 * to the atomic launch beyond 16384 slots (3 B) or D > 256.  chaorec_bpr_fwd_bwd_f32 / _at_f32 (the fused LightGCN steps) add
 * their gradient rows through this launch as well when the environment says CHAOREC_BPR_ORDERED=2 (read per call). */
int chaorec_bpr_bwd_ordered_f32(const float *tab_u, const float *tab_i,
                                const int64_t *users, const int64_t *pos, const int64_t *neg,
                                int32_t B, int32_t D, const float *coef, float reg_weight,
                                const float *grad_out, float *g_u, float *g_i, void *stream);

/* ---------------------------------------------------------------------------------------
 * S: uniform negative sampler with history rejection.
 *
 * Replaces: TrainingDataset.__getitem__'s `random.sample(all_set,1)` rejection loop
 *           (dataload.py:74-79).  Parity is distributional (uniform over items the user has
 *           not interacted with), not bit-wise: the reference uses Python's Mersenne Twister.
 * hist_* is the user -> interacted LOCAL item ids CSR, ids ascending inside a row.
 * Draws are a pure function of (seed, step, b, attempt): reproducible and order-free.
 * step_dev (optional device int64 scalar) is added to `step`, so a captured hipGraph can advance the stream
 * of draws from a device-resident batch counter.
 * out_neg[b] = local item id + id_offset (the reference hands out GLOBAL ids = item + num_user).
 * The reference draws a SECOND item per sample by the same rule (dataload.py:81-84: `int_items`, handed out only to MCLN,
 * :103-104): that is this function again under  seed ^ CHAOREC_SECOND_DRAW_SALT  -- an independent stream of the same
 * counter generator, never in the user's history either.
 * ------------------------------------------------------------------------------------- */
#define CHAOREC_SECOND_DRAW_SALT 0x9E3779B97F4A7C15ull
int chaorec_sample_negatives(const int64_t *hist_rowptr, const int32_t *hist_col,
                             const int64_t *users, int32_t B, int32_t num_item,
                             uint64_t seed, uint64_t step, const int64_t *step_dev, int64_t id_offset,
                             int64_t *out_neg, void *stream);

/* One launch per training batch for a streaming trainer: B edges picked uniformly from `edges` ([n_edges, 2]
 * int64, GLOBAL item ids, device), their (user, positive) gathered and one negative drawn for each by the rule
 * above (same draw stream as chaorec_sample_negatives).  Replaces DataLoader(shuffle=True) +
 * TrainingDataset.__getitem__ (main.py:194-195, dataload.py:74-106).  Outputs LOCAL item ids + item_offset (ABI 9:
 * item_offset = num_user gives the GLOBAL ids the reference's dataset hands to Model.loss()). */
/* The batch BEFORE the forward: chaorec_draw_batch's triples (edges != NULL; the same triples chaorec_bpr_fwd_bwd_at_f32
 * draws for the same seed / step / permutation position, LOCAL item ids) or a given batch (edges == NULL: users / pos / neg
 * are inputs), and the three table rows of every sample flagged in row_bits (bit u, bit bits_item_offset + pos,
 * bit bits_item_offset + neg); list / list_n (optional, *list_n zero on entry): every row this launch flags first is
 * appended.  For a training step whose forward propagates are restricted to the rows its loss reads
 * (train_and_evaluate.py:43-48 never looks at the other rows of Model/LightGCN.py:95's mean). */
int chaorec_batch_rows(const int64_t *edges, int64_t n_edges, const int64_t *hist_rowptr, const int32_t *hist_col,
                       int32_t B, int64_t num_user, int32_t num_item, uint64_t seed, uint64_t step,
                       const int64_t *step_dev, const int64_t *perm, const int64_t *perm_pos, int64_t pos_offset,
                       int64_t *users, int64_t *pos, int64_t *neg, uint32_t *row_bits, int64_t bits_item_offset,
                       int32_t *list, int32_t *list_n, int64_t list_cap, void *stream);

int chaorec_draw_batch(const int64_t *edges, int64_t n_edges, const int64_t *hist_rowptr,
                       const int32_t *hist_col, int32_t B, int64_t num_user, int32_t num_item,
                       uint64_t seed, uint64_t step, const int64_t *step_dev, int64_t *out_users,
                       int64_t *out_pos, int64_t *out_neg, int64_t item_offset, void *stream);

/* out[0:B] = pos - offset, out[B:2B] = neg - offset: Model.loss()'s id shift (Model/FREEDOM.py:195-196) and the row list of
 * the batch's 2 B items in one launch (ABI 9). */
int chaorec_shift_cat_i64(const int64_t *pos, const int64_t *neg, int64_t offset, int32_t B, int64_t *out, void *stream);

/* The fused form the training loop uses (north_star: "fused BPR negative-sample + gather + pairwise-logsigmoid +
 * L2-reg kernel using wavefront shuffles"): chaorec_draw_batch + chaorec_bpr_fwd_f32 in ONE forward launch -- lane 0 of
 * sample b's wave draws (user, positive, negative) exactly as chaorec_draw_batch does for (seed, step + *step_dev, b),
 * the wave shares the ids by shuffle, gathers the three rows and reduces.  out_users / out_pos / out_neg receive the
 * ids (LOCAL item ids; the backward launch chaorec_bpr_bwd_f32 takes them).  Everything else as chaorec_bpr_fwd_f32;
 * results are bit-identical to the two-call form.  advance (optional, may be step_dev itself): a device counter that
 * the single-block finalize launch increments by one after the draw, so a captured step needs no separate
 * counter kernel.  perm / perm_pos (optional): draw the training edges from an epoch permutation instead -- sample b
 * takes edge perm[*perm_pos + b] (DataLoader(shuffle=True): every edge once per epoch; negatives as above); with
 * `advance` set, *perm_pos moves on by B in the finalize launch. */
int chaorec_bpr_fwd_drawn_f32(const float *tab_u, const float *tab_i, const int64_t *edges, int64_t n_edges,
                              const int64_t *hist_rowptr, const int32_t *hist_col, int64_t num_user,
                              int32_t num_item, uint64_t seed, uint64_t step, const int64_t *step_dev,
                              int32_t B, int32_t D, int32_t variant, float reg_weight, int64_t *out_users,
                              int64_t *out_pos, int64_t *out_neg, float *out_loss, float *out_total,
                              float *coef, float *workspace, int64_t *advance, const int64_t *perm,
                              int64_t *perm_pos, void *stream);

/* Forward terms AND backward row updates of the BPR(+L2) loss in ONE launch, for a loss differentiated with
 * d(loss) = 1 (a plain loss.backward(), train_and_evaluate.py:46): sample b's coefficient depends on its own score
 * difference only, so the wave that reduced the triple adds its three gradient rows at once (the arithmetic of
 * chaorec_bpr_bwd_f32 with grad_out = 1).  The batch is drawn in the launch when `edges` != NULL (exactly as
 * chaorec_bpr_fwd_drawn_f32; out_* receive the ids) or given by in_users / in_pos / in_neg (LOCAL item ids).
 * g_u / g_i must be zero wherever no sample lands.  The loss itself comes from chaorec_bpr_finalize_f32 on the
 * same workspace.  adam_step / adam_bc (optional): torch.optim.Adam's step count is incremented and the new step's
 * bias corrections {1 - beta1^t, sqrt(1 - beta2^t)} are written here, by one otherwise idle thread (consumed later in
 * the step by chaorec_spmm_csr_adam_f32). */
int chaorec_bpr_fwd_bwd_f32(const float *tab_u, const float *tab_i, const int64_t *edges, int64_t n_edges,
                            const int64_t *hist_rowptr, const int32_t *hist_col, int64_t num_user,
                            int32_t num_item, uint64_t seed, uint64_t step, const int64_t *step_dev,
                            const int64_t *in_users, const int64_t *in_pos, const int64_t *in_neg,
                            int32_t B, int32_t D, int32_t variant, float reg_weight, int64_t *out_users,
                            int64_t *out_pos, int64_t *out_neg, float *coef, float *workspace,
                            const int64_t *perm, const int64_t *perm_pos, float *g_u, float *g_i,
                            int32_t *adam_step, float beta1, float beta2, float *adam_bc, void *stream);

/* The single-block, fixed-order reduction of a BPR forward's workspace ([4, B]: terms, sum u^2, sum p^2, sum n^2)
 * into out_loss[3] = {total, bpr, reg} (+ out_total[0] = total), and the step's scalar bookkeeping, all optional:
 * loss_accum[0] += total (the per-epoch loss sum of train_and_evaluate.py:48 without its per-batch host sync);
 * advance[0] += 1 and perm_pos[0] += B (batch counter / epoch-permutation position of the in-launch draw);
 * adam_step[0] += 1 and adam_bc[2] = {1 - beta1^t, sqrt(1 - beta2^t)} for the new t (torch.optim.Adam's step count
 * and bias corrections, consumed by chaorec_spmm_csr_adam_f32). */
int chaorec_bpr_finalize_f32(const float *workspace, int32_t B, int32_t D, float reg_weight, float *out_loss,
                             float *out_total, float *loss_accum, int64_t *advance, int64_t *perm_pos,
                             int32_t *adam_step, float beta1, float beta2, float *adam_bc, void *stream);

/* The two above for a replay of k captured steps that runs its loss bookkeeping ONCE (chaorec_amd/optim.py:
 * FusedLightGCNStep, steps_per_replay > 1): step j of the replay draws its batch with step = j and
 * pos_offset = j * B (read position *perm_pos + pos_offset of the epoch permutation) into its own workspace
 * workspace + j * ws_stride, and ONE chaorec_bpr_finalize_steps_f32 after the last step reduces the k workspaces in
 * order -- the same sums and the same sequence of additions into loss_accum as k single launches -- writes the LAST
 * step's out_loss / out_total and moves *advance on by k and *perm_pos by k * B.  scratch: 2 k + 1 floats, the last one an
 * int ticket that is zero on entry and zero again afterwards (one workgroup per step; the last to arrive does the
 * bookkeeping in step order). */
int chaorec_bpr_fwd_bwd_at_f32(const float *tab_u, const float *tab_i, const int64_t *edges, int64_t n_edges,
                               const int64_t *hist_rowptr, const int32_t *hist_col, int64_t num_user,
                               int32_t num_item, uint64_t seed, uint64_t step, const int64_t *step_dev,
                               const int64_t *in_users, const int64_t *in_pos, const int64_t *in_neg,
                               int32_t B, int32_t D, int32_t variant, float reg_weight, int64_t *out_users,
                               int64_t *out_pos, int64_t *out_neg, float *coef, float *workspace,
                               const int64_t *perm, const int64_t *perm_pos, int64_t pos_offset, float *g_u,
                               float *g_i, int32_t *adam_step, float beta1, float beta2, float *adam_bc,
                               uint32_t *row_bits, int64_t bits_item_offset, void *stream);
/* (row_bits, optional: bit u, bit bits_item_offset + pos, bit bits_item_offset + neg of every sample are set -- the
 *  rows of the gradient buffer the launch touched, for chaorec_spmm_csr_rowsparse_f32) */

/* chaorec_bpr_fwd_bwd_at_f32 over a table that is never formed (an INNER step of a k-step replay: Model/LightGCN.py:95's
 * layer mean is read in the batch's rows only, and the next step overwrites it before anything else could look):
 *     tab[r] = w * tabs[0][r] + w * tabs[1][r] + ... + w * tabs[n_tabs - 1][r]
 * for the 3 B rows of the batch, accumulated left to right with separately rounded multiplies and adds -- bit for bit the
 * table chaorec_spmm_csr_mean_f32 writes when tabs[n_tabs - 1] is its propagate's result.  tabs: a HOST array of 1 .. 4 device
 * tables, [N, D] each with the users first and item i at row item_offset + i; rows: device float [3 B, D], receives triple b's
 * user / positive / negative row of the mean at 3 b, 3 b + 1, 3 b + 2 (the ordered gradient launch of
 * CHAOREC_BPR_ORDERED=2 reads them there).  Everything else -- draw, terms, coefficient, gradient rows into g_u / g_i,
 * counters, row_bits -- is the _at_ launch's. */
int chaorec_bpr_fwd_bwd_layers_f32(const float *const *tabs, int32_t n_tabs, float w, int64_t item_offset, float *rows,
                                   const int64_t *edges, int64_t n_edges, const int64_t *hist_rowptr,
                                   const int32_t *hist_col, int64_t num_user, int32_t num_item, uint64_t seed,
                                   uint64_t step, const int64_t *step_dev, const int64_t *in_users,
                                   const int64_t *in_pos, const int64_t *in_neg, int32_t B, int32_t D, int32_t variant,
                                   float reg_weight, int64_t *out_users, int64_t *out_pos, int64_t *out_neg,
                                   float *coef, float *workspace, const int64_t *perm, const int64_t *perm_pos,
                                   int64_t pos_offset, float *g_u, float *g_i, int32_t *adam_step, float beta1,
                                   float beta2, float *adam_bc, uint32_t *row_bits, int64_t bits_item_offset,
                                   void *stream);
int chaorec_bpr_finalize_steps_f32(const float *workspace, int64_t ws_stride, int32_t n_steps, int32_t B,
                                   int32_t D, float reg_weight, float *out_loss, float *out_total,
                                   float *loss_accum, int64_t *advance, int64_t *perm_pos, float *scratch, void *stream);

/* chaorec_bpr_fwd_bwd_layers_f32 with the LAST layer table never formed either (csrc/bpr_frontier.hip; an inner step of a
 * k-step replay): tabs holds x_0 .. x_{n_tabs - 1} (1 .. 3 tables) and the launch computes the batch's 3 B rows of
 *     x_{n_tabs} = A x_{n_tabs - 1}
 * itself from the CSR arrays (rowptr int64 [n_rows + 1], col, val; tabs[n_tabs - 1] 16-byte aligned) -- every row the
 * sequential CSR-order sum from +0 with separately rounded product and sum, the row chaorec_spmm_csr_f32 writes with
 * alpha = 1 and no z, bit for bit -- and the mean over the n_tabs + 1 tables from them.  So it stands for the last forward
 * propagate AND the BPR launch: same ids, coef, workspace, `rows`, gradient rows, row_bits and Adam counters.
 * One workgroup per triple; a round of chaorec_bpr_frontier_round_entries() entries of the triple's three rows is gathered
 * at once.  D = 64 only; mode: the propagate's (CHAOREC_SPMM_DYNAMIC_VALUES is refused).  Checked before any launch. */
int chaorec_bpr_fwd_bwd_frontier_f32(const float *const *tabs, int32_t n_tabs, float w, int64_t item_offset, float *rows,
                                     const int64_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                                     int32_t mode, const int64_t *edges, int64_t n_edges, const int64_t *hist_rowptr,
                                     const int32_t *hist_col, int64_t num_user, int32_t num_item, uint64_t seed,
                                     uint64_t step, const int64_t *step_dev, const int64_t *in_users,
                                     const int64_t *in_pos, const int64_t *in_neg, int32_t B, int32_t D, int32_t variant,
                                     float reg_weight, int64_t *out_users, int64_t *out_pos, int64_t *out_neg,
                                     float *coef, float *workspace, const int64_t *perm, const int64_t *perm_pos,
                                     int64_t pos_offset, float *g_u, float *g_i, int32_t *adam_step, float beta1,
                                     float beta2, float *adam_bc, uint32_t *row_bits, int64_t bits_item_offset,
                                     void *stream);
int64_t chaorec_bpr_frontier_round_entries(void);

/* ---------------------------------------------------------------------------------------
 * R: all-items scoring + history mask + top-K, never materialising the [U, I] matrix.
 *
 * Replaces: torch.matmul(user, item.T) + per-user python mask loop + torch.topk
 *           (Model/LightGCN.py:147-155, Model/FREEDOM.py:230-238, Model/MMGCN.py:220-230)
 *           and the kNN build torch.mm + topk (Model/FREEDOM.py:114-118) with hist == NULL.
 *
 *   score[u][i] = sum_k user_emb[u][k] * item_emb[i][k]          (precision below)
 *   score[u][i] = mask_value   for every i in hist row u          (1e-6 / 1e-5 in the reference)
 *   out = the K largest per user, descending; ties -> LOWEST item index first.
 *   out_idx = item index + id_offset (int64), out_val = the (masked) score.
 *
 * The RESULT is the same for every `precision` value: the exact top-K of the fp32 scores defined by the
 * k-ordered fmaf chain below (what v_mfma_f32_32x32x2_f32 computes), bit-identical to
 * oracle/chaorec_oracle.c:oracle_score_dot().  With the K-dim cut into chunks of C floats (C = D for
 * D <= 128, C = 64 above), per chunk base b:
 *     for s in [0, C/2): acc = fmaf(u[b+s], i[b+s], acc); acc = fmaf(u[b+C/2+s], i[b+C/2+s], acc)
 * `precision` selects the route to it:
 *   0  fastest exact route.  D in {64, 128} and >= 4096 items: the [U, I] sweep runs on the bf16 MFMA pipe
 *      (v_mfma_f32_32x32x16_bf16, 16x the f32 MFMA rate) as a PREFILTER with a proven per-item error bound
 *      |s~ - s| <= e_uj = 1.05 * 2^-8 * ||u|| * ||i_j||: every item whose upper bound s~ + e exceeds a per-user
 *      threshold T_u becomes a candidate, every candidate is re-scored with the exact fp32 chain and the top-K is
 *      ranked on those values; the answer is certified when the K-th best exact score is > T_u (anything outside
 *      the candidates is then strictly beaten by K items).  T_u is estimated from a sample of the items; a user that
 *      cannot be certified (list overflow, too few / too many candidates) gets all its scores computed exactly.
 *      From 524 288 items and 2 U I D >= 3e13 flops per call on (environment CHAOREC_PF_CLS_MIN_ITEMS: an item count as the
 *      only condition, 0 = never) the prefilter works on a
 *      NORM-SORTED copy of the item table: items in descending order of their norm class (exponent + 3 mantissa bits), the
 *      bound taken per run of classes instead of per item -- e_u = c ||u|| N_run folded into the users' operand scale, so
 *      the bound costs no MFMA (one in nine at D = 128) --, thresholds sampled from every 32nd / 16th / 8th item of that
 *      order.  Same candidates-superset guarantee, same exact re-score, same result bit for bit; the workspace holds the
 *      permutation (chaorec_score_topk_workspace_bytes accounts for it under the same environment).
 *      Otherwise: route 2.
 *   1  one unthresholded fp32 MFMA pass (A/B runs and tests).
 *   2  fp32 MFMA sweep with a sampled per-user threshold: tau0 = 32nd best score over every s-th 32-item tile,
 *      the full pass keeps only scores above it, a certification step counts them and any user with fewer
 *      than K is re-ranked without a threshold.
 * D in {8, 16, 32, 64, 128} (users' fragment register-resident) or a multiple of 64 above 128
 * (streamed; the kNN build over modality features);  1 <= K <= 64;  n_items >= K.
 * hist_rowptr may be NULL (no mask).  hist_col ascending inside a row.
 * workspace: chaorec_score_topk_workspace_bytes() bytes, 256-byte aligned; nothing in it survives the call.  The
 * call issues kernels only (no memset / memcpy nodes), so it may be captured in a hipGraph.
 * ------------------------------------------------------------------------------------- */
size_t chaorec_score_topk_workspace_bytes(int64_t n_users, int64_t n_items, int32_t K, int32_t D);

int chaorec_score_topk_f32(const float *user_emb, const float *item_emb,
                           int64_t n_users, int64_t n_items, int32_t D,
                           const int64_t *hist_rowptr, const int32_t *hist_col,
                           float mask_value, int32_t K, int64_t id_offset,
                           int64_t *out_idx, float *out_val,
                           void *workspace, size_t workspace_bytes,
                           int32_t precision, void *stream);

/* chaorec_score_topk_f32 (route 0) with the per-user thresholds CARRIED from one call to the next: an evaluation
 * loop ranks the same users once per epoch (train_and_evaluate.py:655-659) and one epoch moves the scores little.
 *   hint_out (optional, [n_users] float, device): receives, per user, one float below the exact score of rank
 *            hint_rank (K < hint_rank <= 128; 80 is a good value for K = 50) -- the next call's threshold.
 *   hint_in  (optional): such an array from the previous call (may alias hint_out).  Pass A sweeps with T_u = hint_in
 *            (no sampling pass, about half the candidates of a sampled threshold); users it cannot certify -- scores
 *            moved too much since -- are queued on the device and retried with a sampled threshold (pass B), then, if
 *            need be, ranked exactly.  hint_in == NULL: pass B for everybody (= chaorec_score_topk_f32).
 *            A queue of at most 16 users skips pass B and is ranked exactly, per user, at once.
 *   flags    CHAOREC_SCORE_LIGHT: launch no pass B at all (three launches and their one-wave critical path less) -- for
 *            a caller that saw a short queue last time; whatever pass A leaves is ranked exactly per user, which is slow
 *            only if that expectation was wrong.
 *   counters_out (optional, device int32[4]): {users pass A queued, users ranked by the exact route, users of the wide
 *            selection, queued users taken by the exact route} of THIS call -- what a caller bases the next call's flags on.
 * A threshold never changes the result, only the work: the output is bit-identical to chaorec_score_topk_f32's
 * whatever the hints hold (NaN / inf / stale values included).  Needs the prefilter route (D in {64,128}, >= 4096
 * items, K <= 64); otherwise the hints are ignored and hint_out / counters_out are left untouched.
 *   flags    CHAOREC_SCORE_FRONT / CHAOREC_SCORE_BACK: run only the first / only the second PHASE of the call.  The front
 *            is everything up to and including the call's first sweep over all users (pack, sampling when there are no
 *            hints, sweep); the back is the rest (selection, retry passes, exact routes).  Two calls with the same
 *            arguments and the same workspace, FRONT then BACK (in stream order, or on two streams with an event between
 *            them), are one whole call.  For a caller that ranks several user ranges: range k's back phase -- gather- and
 *            VALU-bound -- beside range k + 1's front phase -- MFMA-bound -- on another stream, one workspace per range in
 *            flight.  Neither flag (or both): the whole call.  On the routes without a prefilter the BACK call does
 *            everything and the FRONT call nothing.
 * Long item ranges (>= 131072 items), where the exact per-user route streams the whole item table per user: a user whose
 * candidate lists overflowed (threshold too low) first gets a RAISED threshold -- the exact score of a rank >= K among
 * the candidates its lists kept -- and one more compact sweep + selection (pass C); only what that cannot certify
 * either is ranked by the exact routes. */
#define CHAOREC_SCORE_LIGHT 1
#define CHAOREC_SCORE_FRONT 2
#define CHAOREC_SCORE_BACK 4
int chaorec_score_topk_hinted_f32(const float *user_emb, const float *item_emb,
                                  int64_t n_users, int64_t n_items, int32_t D,
                                  const int64_t *hist_rowptr, const int32_t *hist_col,
                                  float mask_value, int32_t K, int64_t id_offset,
                                  int64_t *out_idx, float *out_val,
                                  void *workspace, size_t workspace_bytes,
                                  const float *hint_in, float *hint_out, int32_t hint_rank, int32_t flags,
                                  int32_t *counters_out, void *stream);

/* Monitoring: what the prefilter route of the LAST scoring call on this workspace did (same sizes).
 * out10 (device, 10 x uint64): [0] users handed to the exact routes, [1] candidates re-scored in total, [2] longest
 * per-lane sweep list (entries), [3] users, [4..8] users the last selection pass could not certify, by reason (list
 * overflow, fewer than K candidates, more candidates than the selection holds, K-th best not above the sweep
 * threshold, unused), [9] users that were given a raised threshold and one more pass (pass C).  All zeros if that call
 * did not take the prefilter route. */
int chaorec_score_topk_stats(const void *workspace, int64_t n_users, int64_t n_items, int32_t K, int32_t D,
                             uint64_t *out10, void *stream);

/* ---------------------------------------------------------------------------------------
 * Rank lists past 64 columns (csrc/topk_wide.hip).  Additive to ABI 16: new names only.
 *
 * Replaces: the same gene_ranklist lines as chaorec_score_topk_f32 (Model/LightGCN.py:147-155, Model/FREEDOM.py:230-238,
 *           Model/MMGCN.py:220-230) for 64 < topk <= 1024, in two launches per user range: the exact scores of the range
 *           into a staging block, then the exact top-k of every staged row.
 *
 * chaorec_score_rows_f32: scores[u - user_begin, i] for the users user_begin .. user_begin + n of user_emb [n_users, D]
 * against all n_items rows of item_emb -- the same fp32 value as chaorec_score_topk_f32 ranks (the two interleaved fmaf
 * chains stated there, 64-wide chunks above D = 128), history entries (hist_rowptr int64 [n_users + 1], hist_col int32
 * LOCAL item ids ascending inside a row; hist_rowptr may be NULL) = mask_value.  scores is [n, ld] fp32 with ld >= n_items
 * (columns n_items .. ld are left alone); n * ld * 4 must not exceed scores_bytes: the [U, I] matrix never exists whole, the
 * caller walks the users in ranges.  D as chaorec_score_topk_f32.  One launch, no workspace. */
int chaorec_score_rows_f32(const float *user_emb, const float *item_emb, int64_t n_users, int64_t n_items, int32_t D,
                           int64_t user_begin, int64_t n, const int64_t *hist_rowptr, const int32_t *hist_col,
                           float mask_value, float *scores, int64_t ld, size_t scores_bytes, void *stream);
/* Exact top-k of every row of scores [n_rows, ld] (row r = scores + r * ld, its first I columns; any 4-byte alignment) for
 * 64 < topk <= min(1024, I): descending by chaorec_macrid_topk_f32's bit-pattern order (-0 < +0, a NaN by sign and
 * payload), ties to the lowest index (torch.topk's values, Model/LightGCN.py:155): idx [n_rows, topk] = column + id_offset,
 * val [n_rows, topk].  One workgroup per row: radix search for the k-th key, ordered compaction, bitonic sort of the k
 * winners in LDS.  No atomics: the same bits on every run. */
int chaorec_rows_topk_wide_f32(const float *scores, int64_t n_rows, int64_t I, int64_t ld, int32_t topk, int64_t id_offset,
                               int64_t *idx, float *val, void *stream);

/* ---------------------------------------------------------------------------------------
 * M: ranking metrics of every evaluation row in one launch.
 *
 * Replaces: utils.gene_metrics' python loop over users x K x {precision, recall, ndcg, hit_rate, map}
 *           (utils.py:112-139) with the per-user formulas of metrics.py:13-57 and their corner cases: set()
 *           semantics for precision / recall / hit_rate, `item in test_list` per position for ndcg / map,
 *           len(test_list) (duplicates included) as denominator, 0 for an empty list, natural-log discounts.
 *
 *   rank_idx   [n_users, rank_stride] int64 global item ids, best first (chaorec_score_topk_f32's out_idx)
 *   row_user   [n_rows] user of each evaluation row; pos_rowptr/pos_items: the rows' positives as a CSR
 *              (val.npy / test.npy rows [user, pos...]), global item ids, duplicates allowed
 *   k_list     HOST array of n_k <= 8 cut-offs, each <= min(1024, rank_stride).  With every cut-off <= 64 a thread owns
 *              an evaluation row (one 64-bit hit mask); a call with a larger one gives every row to a wave (16 mask words)
 *              and needs chaorec_rank_metrics_wide_workspace_bytes(n_rows, n_k, max k) of workspace, which also holds
 *              the discount table (it travels in kernel arguments, 480 doubles per launch: still kernels only)
 *   discount   HOST array, discount[p] = 1 / log(p + 2) for p < max(k) as the caller's libm gives it (the
 *              per-user terms are then bit-identical to a host evaluation with the same table)
 *   out        DEVICE [n_k][5] fp64: precision, recall, ndcg, hit_rate, map, each averaged over n_rows
 * fp64 throughout; the sums over rows are reduced in a fixed order (run-to-run identical).
 * ------------------------------------------------------------------------------------- */
size_t chaorec_rank_metrics_workspace_bytes(int64_t n_rows, int32_t n_k);
/* (kmax <= 64: the value above) */
size_t chaorec_rank_metrics_wide_workspace_bytes(int64_t n_rows, int32_t n_k, int32_t kmax);
int chaorec_rank_metrics_f64(const int64_t *rank_idx, int64_t n_users, int64_t rank_stride,
                             const int64_t *row_user, const int64_t *pos_rowptr, const int64_t *pos_items,
                             int64_t n_rows, const int32_t *k_list, int32_t n_k, const double *discount,
                             double *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Dense fp32 GEMM on the f32 MFMA pipe (exact fp32 products, fp32 accumulate):
 *   C[M,N] = op(A) * op(B) (+ bias[N]) (+ C if accumulate)
 * transA/transB: 0 = as stored [M,K]/[K,N], 1 = stored transposed [K,M]/[N,K].
 *
 * Replaces: nn.Linear forward/backward on modality features and MMGCN's per-layer Linears
 *           (Model/FREEDOM.py:59-60,209,212; Model/MMGCN.py:40,97,102-131; BasicGCN.py:40).
 *   forward  y = x W^T + b      : transA=0, transB=1 (W stored [N,K])
 *   grad x   = gy W             : transA=0, transB=0
 *   grad W   = gy^T x           : transA=1, transB=0
 * act: 0 none, 1 leaky_relu(0.01) applied to the result (F.leaky_relu default slope), 2 leaky_relu(0.2)
 *      (nn.LeakyReLU(0.2), Model/NGCF.py:32).
 * Few output tiles with a long reduction (weight gradients: K = number of graph nodes) are split along K into
 * slabs in `workspace` (size from chaorec_gemm_workspace_bytes) and summed in a fixed order by a second launch:
 * deterministic, equal to the unsplit chain to rounding. */
size_t chaorec_gemm_workspace_bytes(int64_t M, int64_t N, int64_t K);
int chaorec_gemm_f32(const float *A, const float *B, float *C, const float *bias,
                     int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                     int32_t transA, int32_t transB, int32_t accumulate, int32_t act,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * y = x W^T (+ bias, + leaky-relu) on the bf16 MFMA pipe at fp32-grade accuracy: the FORWARD of the modality
 * projections image_trs / text_trs over the [I, 4096] / [I, 384] feature tables (Model/FREEDOM.py:59-60,209,212) and
 * of MMGCN's Linears (Model/MMGCN.py:40,97,102-131; BasicGCN.py:40).
 *   C[M,N] = A[M,K] . B[N,K]^T, both operands k-contiguous (torch's nn.Linear layout), fp32 in / fp32 out.
 * Every operand is split exactly into three bf16 planes (8+8+8 significand bits) and six of the nine plane products
 * are accumulated in fp32 by v_mfma_f32_32x32x16_bf16: |C - exact| <= ~4e-7 * sum_k |a||b| (an fp32 GEMM's accuracy
 * class; NOT bit-identical to chaorec_gemm_f32 / oracle_gemm_f32, whose k-ascending fmaf chain stays available), at
 * 2.7x the f32 MFMA rate -- the skinny N = 64 projections become HBM-bound (A is read once).
 * act: 0 none, 1 leaky_relu(0.01), 2 leaky_relu(0.2).  workspace: chaorec_gemm_nt_bf16x3_workspace_bytes(M,N,K)
 * (K-slabs of outputs with few tiles, summed in a fixed order).
 * ------------------------------------------------------------------------------------- */
size_t chaorec_gemm_nt_bf16x3_workspace_bytes(int64_t M, int64_t N, int64_t K);
int chaorec_gemm_nt_bf16x3(const float *A, const float *B, float *C, const float *bias, int64_t M, int64_t N,
                           int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t act, void *workspace,
                           size_t workspace_bytes, void *stream);

/* The weight gradient of those Linears on the same pipe:  C[M, N] = A[K, M]^T B[K, N]  (A = the gradient of the layer's
 * output, B = its input, K = the rows both run over -- every graph node for Model/MMGCN.py:97-131's layers), same
 * three-plane split, same accuracy class, slabs along K summed in a fixed order (deterministic).  Replaces
 * autograd's  grad_output.t() @ input  (an fp32 GEMM).  lda >= M, ldb >= N, ldc >= N. */
size_t chaorec_gemm_tn_bf16x3_workspace_bytes(int64_t M, int64_t N, int64_t K);
int chaorec_gemm_tn_bf16x3(const float *A, const float *B, float *C, int64_t M, int64_t N, int64_t K, int64_t lda,
                           int64_t ldb, int64_t ldc, void *workspace, size_t workspace_bytes, void *stream);

/* The INPUT gradient of those Linears,  C[M, N] = A[M, K] . B[K, N]  with B = the layer's weight [out = K, in = N] as it
 * lies in memory (autograd's  grad_output @ weight, Model/MMGCN.py:97-131's layers backwards): same pipe, same split,
 * same accuracy class.  lda >= K, ldb >= N, ldc >= N.  accumulate != 0: C += A B (a node's second gradient flow added in
 * the epilogue instead of by a separate launch; a + b is commutative, so the bits are those of the separate add). */
size_t chaorec_gemm_nn_bf16x3_workspace_bytes(int64_t M, int64_t N, int64_t K);
int chaorec_gemm_nn_bf16x3(const float *A, const float *B, float *C, int64_t M, int64_t N, int64_t K, int64_t lda,
                           int64_t ldb, int64_t ldc, int32_t accumulate, void *workspace, size_t workspace_bytes,
                           void *stream);

/* The two Linears MMGCN applies to the same x -- conv.lin (BasicGCN.py:40) and linear_layer (Model/MMGCN.py:104-131) -- as ONE
 * product each way, their operands concatenated virtually (second pointers, no copies), same pipe and accuracy class (ABI 9):
 *   nt_dual  [C1 | C2] = act1/act2( A [B1; B2]^T + [bias1 | bias2] )      B1 [N1, K], B2 [N2, K]; C1 [M, N1], C2 [M, N2]
 *   nn_dual  C = [A1 | A2] [B1; B2]                                      A1 [M, K1], A2 [M, K2]; B1 [K1, N], B2 [K2, N]
 *   tn_dual  [C1; C2] = [A1 | A2]^T B                                    A1 [K, M1], A2 [K, M2]; B [K, N]; C1 [M1, N], C2 [M2, N]
 * The split sizes (N1 / K1 / M1) and the second operands' leading dimensions are multiples of 4, the second pointers 16-byte
 * aligned.  nt_dual serves shapes without split-K only (error otherwise: call the products separately). */
int chaorec_gemm_nt_bf16x3_dual(const float *A, const float *B1, const float *B2, float *C1, float *C2, const float *bias1,
                                const float *bias2, int64_t M, int64_t N1, int64_t N2, int64_t K, int64_t lda, int64_t ldb1,
                                int64_t ldb2, int64_t ldc1, int64_t ldc2, int32_t act1, int32_t act2, void *stream);
size_t chaorec_gemm_nn_bf16x3_dual_workspace_bytes(int64_t M, int64_t N, int64_t K);
int chaorec_gemm_nn_bf16x3_dual(const float *A1, const float *A2, const float *B1, const float *B2, float *C, int64_t M,
                                int64_t N, int64_t K1, int64_t K2, int64_t lda1, int64_t lda2, int64_t ldb1, int64_t ldb2,
                                int64_t ldc, void *workspace, size_t workspace_bytes, void *stream);
size_t chaorec_gemm_tn_bf16x3_dual_workspace_bytes(int64_t M, int64_t N, int64_t K);
int chaorec_gemm_tn_bf16x3_dual(const float *A1, const float *A2, const float *B, float *C1, float *C2, int64_t M1, int64_t M2,
                                int64_t N, int64_t K, int64_t lda1, int64_t lda2, int64_t ldb, int64_t ldc1, int64_t ldc2,
                                void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------
 * Fused Adam step over one flat fp32 parameter (torch.optim.Adam defaults, main.py:397):
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 *   p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * t = *step_dev when step_dev != NULL (a device counter, so the launch can sit in a captured hipGraph),
 * else `step`.
 * ------------------------------------------------------------------------------------- */
int chaorec_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                          int64_t n, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int32_t step, const int32_t *step_dev, void *stream);

/* The same update for up to chaorec_adam_multi_max() parameter tensors in ONE launch (host arrays of `count` device
 * pointers and element counts; the pointers travel in the kernel argument): a model with ~50 small tensors
 * (Model/MMGCN.py) otherwise pays one launch latency per tensor and step.  Same arithmetic, bit for bit. */
int32_t chaorec_adam_multi_max(void);
int chaorec_adam_multi_f32(int32_t count, float *const *param, const float *const *grad, float *const *exp_avg,
                           float *const *exp_avg_sq, const int64_t *numel, float lr, float beta1, float beta2,
                           float eps, float weight_decay, int32_t step, const int32_t *step_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * Adam over a trainable feature table whose gradient is  G = gy W  (rank R <= 64, non-zero in the few rows of the batch).
 *
 * Replaces: the dense [n_rows, K] gradient of nn.Embedding.from_pretrained(feat, freeze=False).weight behind
 *           trs(feat.weight)[pos | neg] (Model/FREEDOM.py:59-60, 209-213: autograd materialises gy W, 186 MB at
 *           clothing size) + torch.optim.Adam streaming it (main.py:397).
 *
 * param, exp_avg, exp_avg_sq [n_rows, K] (K % 4 == 0, 16-byte aligned); gy [n_rows, R] = gradient with respect to the
 * projection's output (zero rows for items outside the batch); W [R, K] = the projection's weight (nn.Linear layout).
 *   g[n, c] = fmaf chain over r ascending of gy[n, r] * W[r, c], starting from +0; a row whose gy row is all zero takes
 *   g = +0; then chaorec_adam_step_f32's arithmetic with t = *step_dev (or `step`).
 * mode 0 (dense): every row is updated: the tables always equal what chaorec_adam_step_f32 on the dense gradient gives.
 * mode 1 (lazy):  only rows with a non-zero gy row are read or written; such a row first replays the zero-gradient
 *                 steps it sat out (last[strip, row] + 1 .. t - 1: same operations, order and bias corrections), then
 *                 takes step t.  `last`: int32 [chaorec_adam_lowrank_strips(K), n_rows], initialised to the step count at
 *                 which lazy updating starts.
 * mode 2 (flush): every row catches up to step t inclusive with zero gradients and no new step (gy, W unused): after
 *                 it the three tables are bit-identical to mode 0's.  Readers of `param` must flush first, or
 * mode 3 (catch up): the same for the rows with a non-zero row in `gy` only (gy is then a flag array [n_rows, R], W
 *                 unused): the rows of a batch, before its forward gathers them.
 * bc_table (optional, float[2 * bc_len] from chaorec_adam_bias_table): (1 - beta1^s, sqrt(1 - beta2^s)) per step s,
 * spares the replay two double-precision pow() per missed step; steps >= bc_len are computed in the launch.
 * rowlist / rowcount / rowcap (modes 1 and 3): these modes walk a list of distinct rows (int32 ids in device memory,
 * *rowcount <= rowcap of them).  rows_given != 0: the caller filled it (chaorec_unique_rows over the batch's item ids)
 * and the launch visits exactly these rows -- a listed row whose gy row is zero takes the step with g = +0 (mode 1),
 * which is what mode 0 does to it; mode 3 then needs no flag array (gy may be NULL).  rows_given == 0: the launch
 * fills the list itself with the rows whose gy (or flag) row is non-zero (rowcap >= n_rows).
 *
 * mode 0 with step_dev: the step used is *step_dev + step (ABI 9) -- a launch issued before the optimizer advanced its device
 * counter (on a side stream, beside the rest of the backward pass) passes step = 1, every other caller 0.
 *
 * chaorec_unique_rows: list[0 .. *count) = the distinct values of rows[0 .. n) (item ids of a batch, duplicates
 * allowed; ids outside [0, n_rows) are dropped), order unspecified.  claim: int32 [n_rows] scratch and stamp_dev: int32 [1], both zero-initialised once and
 * then left to the launches: each one takes the stamp *stamp_dev + 1, marks the rows it lists with it and stores it
 * back, so nothing is cleared between launches (also not between replays of a captured hipGraph).  One workgroup:
 * meant for batches of a few thousand ids.
 * ------------------------------------------------------------------------------------- */
int32_t chaorec_adam_lowrank_strips(int32_t K);
int chaorec_adam_bias_table(float *table, int32_t n_steps, float beta1, float beta2, void *stream);
int chaorec_unique_rows(const int64_t *rows, int64_t n, int64_t n_rows, int32_t *claim, int32_t *stamp_dev,
                        int32_t *list, int32_t *count, void *stream);
int chaorec_adam_lowrank_f32(float *param, const float *gy, const float *W, float *exp_avg, float *exp_avg_sq,
                             int64_t n_rows, int32_t K, int32_t R, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int32_t step, const int32_t *step_dev, int32_t mode, int32_t *last,
                             const float *bc_table, int32_t bc_len, int32_t *rowlist, int32_t *rowcount,
                             int32_t rowcap, int32_t rows_given, void *stream);

/* ---------------------------------------------------------------------------------------
 * Per-step edge dropout + symmetric renormalisation of a structure-static CSR (NGCF).
 *
 * Replaces: dropout_adj + add_self_loops + degree + deg^-1/2[row]*deg^-1/2[col] inside every NGCFConv.forward
 *           (Model/NGCF.py:38-58), which rebuilds the edge list of the graph on every call.
 *
 * The graph is the destination-major CSR of the bidirectional train edges WITH one self loop per node (the
 * structure of chaorec_spmm_csr_f32's operand, built once).  entry_row[k] = destination of entry k, col[k] = its
 * source, transpose_entry[k] = the entry holding the reversed edge (a bijection; a self loop maps to itself).
 *   keep_k = 1 for self loops (they are appended after the dropout), else u_k >= p with
 *            u_k = 2^-24 * (mix64(seed ^ mix64(step' ^ mix64((salt << 48) ^ k))) >> 40), step' = step + *step_dev
 *            (or keep_in[k] != 0 when keep_in is given: an externally drawn mask, used by the parity tests)
 *   deg[n]  = number of kept entries whose SOURCE is n          (degree(row) on the kept list, int32 in deg_ws)
 *   val[k]   = keep_k                  ? (1/sqrt(deg[col[k]])) * (1/sqrt(deg[entry_row[k]])) : 0
 *   val_t[k] = keep_transpose_entry[k] ? the same product : 0      (the values of A^T in the same structure)
 * p == 0 keeps everything.  deg_ws: n_nodes int32.  salt < 65536 separates the conv layers of one step.
 * Not bit-comparable with the reference's mask (torch's generator); the keep law (independent, rate 1-p) is.
 * ------------------------------------------------------------------------------------- */
int chaorec_edge_dropout_norm(const int32_t *entry_row, const int32_t *col, const int32_t *transpose_entry,
                              int64_t nnz, int64_t n_nodes, float p, uint64_t seed, uint64_t step,
                              const int64_t *step_dev, uint32_t salt, const uint8_t *keep_in,
                              int32_t *deg_ws, float *val, float *val_t, void *stream);

/* ---------------------------------------------------------------------------------------
 * Weighted sampling WITHOUT replacement as a keep mask (FREEDOM's degree-sensitive pruning).
 *
 * Replaces: torch.multinomial(edge_values, k) (Model/FREEDOM.py:151), which is limited to 2^24 categories; the
 *           reference only uses the drawn SET (the pruned graph is coalesced right after, :152-162).
 *
 * Exponential race: key_e = |log(u_e)| / w_e with u_e uniform in (0,1) from the counter generator
 * (mix64(seed ^ mix64(step' ^ mix64((0x5A3B << 48) ^ e)))); the k smallest keys are kept -- the same law as k
 * sequential draws without replacement with probabilities proportional to w.  The k-th smallest 64-bit key
 * ((fp32 key bits << 32) | 32 fresh hash bits) is found by an exact radix select (6 passes, integer histograms),
 * so the mask is a deterministic function of (weights, seed, step').  keep[e] = key_e <= that key: exactly k
 * ones unless two entries share all 64 key bits.  w_e <= 0 is never kept (while k <= #positive weights).
 * keys_out (optional, may be NULL): the n 64-bit keys, for the tests.
 * ------------------------------------------------------------------------------------- */
size_t chaorec_weighted_sample_workspace_bytes(void);
int chaorec_weighted_sample_keep(const float *weights, int64_t n, int64_t k, uint64_t seed, uint64_t step,
                                 const int64_t *step_dev, void *workspace, size_t workspace_bytes,
                                 uint8_t *keep, uint64_t *keys_out, void *stream);

/* The keys of that race alone, entry j numbered ids[j] (NULL: j): what a RANK of a user-sharded job computes for its
 * own share of the edge list (chaorec_amd/dist.py:ShardedFREEDOM.pre_epoch_processing) -- with the edges' numbers in
 * the whole list the keys, hence the kept set { key <= the k-th smallest key of ALL ranks }, do not depend on the
 * sharding; the k-th smallest key over the ranks is found by a radix select over all-reduced histograms. */
int chaorec_weighted_sample_keys(const float *weights, const int64_t *ids, int64_t n, uint64_t seed, uint64_t step,
                                 const int64_t *step_dev, uint64_t *keys_out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Row-wise cosine re-weighting of a propagated layer (LayerGCN).
 *
 * Replaces: _weights = F.cosine_similarity(all_embeddings, ego_embeddings, dim=-1)
 *           all_embeddings = torch.einsum('a,ab->ab', _weights, all_embeddings)       (Model/LayerGCN.py:125-127)
 *           and their autograd backward -- ~12 + ~25 elementwise / reduction launches per layer in the reference.
 *
 * fwd:  w_r = <y_r, e_r> / (max(|y_r|, 1e-8) * max(|e_r|, 1e-8));  out_r = w_r * y_r;  w_out[r] = w_r (optional).
 * bwd:  with a = max(|y|, eps), b = max(|e|, eps), s = <grad_out, y>:
 *         grad_y = w grad_out + s (e/(a b) - [|y| > eps] w y / a^2),  grad_e = s (y/(a b) - [|e| > eps] w e / b^2)
 * y, e, out, grads: fp32 [n_rows, D] row-major, D a multiple of 4 in [4, 1024].  One launch each, one pass over HBM.
 * ------------------------------------------------------------------------------------- */
int chaorec_row_cosine_scale_fwd_f32(const float *y, const float *e, float *out, float *w_out,
                                     int64_t n_rows, int32_t D, void *stream);
int chaorec_row_cosine_scale_bwd_f32(const float *grad_out, const float *y, const float *e, float *grad_y,
                                     float *grad_e, int64_t n_rows, int32_t D, void *stream);

/* NGCF's elementwise backward, one launch each (n a multiple of 4; 16-B aligned pointers).
 * Replaces: torch.where(y > 0, g, 0.2 g) (three launches: the backward of nn.LeakyReLU(0.2), Model/NGCF.py:32,80-84) and
 *           the backward of x_j * x_i (Model/NGCF.py:78: two multiplies and the add into the aggregate's other gradient).
 *   chaorec_leaky_bwd_f32:     grad_in = y > 0 ? grad_out : slope * grad_out
 *   chaorec_mul_pair_bwd_f32:  grad_s += grad_t * x (separately rounded product and sum);  grad_x = grad_t * s */
int chaorec_leaky_bwd_f32(const float *y, const float *grad_out, float slope, float *grad_in, int64_t n, void *stream);
int chaorec_mul_pair_bwd_f32(const float *grad_t, const float *s, const float *x, float *grad_s, float *grad_x,
                             int64_t n, void *stream);

/* out = w * terms[0] + w * terms[1] + ... + w * terms[n_terms-1] over n floats, accumulated in that order (products and
 * sums rounded separately): LightGCN's layer mean (Model/LightGCN.py:86-93) for rows whose propagated values arrive
 * AFTER the propagate launches -- the replicated item rows of a user-row shard, summed over the ranks by the per-layer
 * exchange (chaorec_amd/dist.py).  Same association as chaorec_spmm_csr_mean_f32's epilogue.  terms: HOST array of
 * n_terms (<= 8) device pointers; n a multiple of 4. */
int chaorec_rows_mean_f32(const float *const *terms, int32_t n_terms, float w, float *out, int64_t n, void *stream);

/* ---------------------------------------------------------------------------------------
 * Deterministic two-pass reductions (fixed order, no atomics, no semaphores, no memset nodes).
 *
 * Replaces: the bias gradient of every nn.Linear (grad_out.sum(0), autograd of Model/MMGCN.py:97-131,
 *           Model/FREEDOM.py:209,212, Model/MGCN.py gates) and the scalar means of the regularisers
 *           (Model/MMGCN.py:198-199, Model/LayerGCN.py:147-155, Model/MGCN.py:301) INSIDE captured training steps:
 *           torch's multi-block reductions zero a semaphore buffer with a memset, and a memset node of a captured
 *           hipGraph does not replay on this stack (stale / garbage sums from the second replay on).
 *
 * colsum: out[c] = sum_r x[r*ldx + c]  (x fp32 [M, N] row-major).   sum: out[0] = scale * sum_i x[i].
 * workspace: chaorec_reduce_workspace_bytes(M, N) bytes (use M = n, N = 1 for the scalar sum).
 * ------------------------------------------------------------------------------------- */
size_t chaorec_reduce_workspace_bytes(int64_t M, int64_t N);
int chaorec_colsum_f32(const float *x, int64_t M, int64_t N, int64_t ldx, float *out, void *workspace,
                       size_t workspace_bytes, void *stream);
int chaorec_sum_f32(const float *x, int64_t n, float scale, float *out, void *workspace, size_t workspace_bytes,
                    void *stream);

/* ---------------------------------------------------------------------------------------
 * Peer-to-peer exchange of a sharded layer's item partial (the "direct" reduce-scatter + all-gather in which
 * every row block crosses one xGMI link once), as two plain kernels over IPC-mapped peer buffers ("mailboxes"):
 *   pull_sum:    out[0:n] = sum over r = 0..world-1, in that order, of peers[r][offset : offset + n]
 *   pull_gather: out[r * block : (r + 1) * block] = peers[r][0 : block]   for every r
 * peers: HOST array of `world` (<= 16) device pointers -- this rank's own mailbox at its own index, the others mapped from
 * the peers' processes (hipIpcOpenMemHandle): the partial mailboxes (whole buffer) for pull_sum, the result mailboxes (one
 * block) for pull_gather.  The caller orders the phases across the ranks (a barrier between mailbox write, pull_sum and
 * pull_gather; chaorec_amd/dist.py: a one-element all-reduce on the stream).  offset, n, block in floats, multiples of 4.
 * Plain launches: capturable in a hipGraph (ABI 9).
 * ------------------------------------------------------------------------------------- */
int chaorec_exchange_pull_sum_f32(const void *const *peers, int32_t world, int64_t offset, int64_t n, float *out,
                                  void *stream);
int chaorec_exchange_pull_gather_f32(const void *const *peers, int32_t world, int64_t block, float *out, void *stream);

/* The same exchange for a buffer that is non-zero in a FRONTIER's rows only (ABI 12; the gradient seed and the frontier
 * partials of dist.FusedShardedLightGCNStep's row-sparse backward).  bits: a bitmap over the buffer's n_rows rows, identical
 * on every rank, a superset of the rows that are non-zero on any rank.  Only flagged rows move:
 *   chaorec_rows_copy_by_bits_f32:        dst[r] = src[r]                      (the partial into the mailbox)
 *   chaorec_exchange_pull_sum_rows_f32:   out[r - row0] = sum over ranks, rank order, of peers[q][r]   for the flagged rows r of
 *                                         this rank's block [row0, row0 + n_block)
 *   chaorec_exchange_pull_gather_rows_f32: out[r] = peers[r / n_block][r - (r / n_block) n_block]      for every flagged row
 * The other rows of the caller's buffer are not touched (zeros on every rank, and zeros is their sum).  Row pointers in
 * units of rows of D floats (D a multiple of 4). */
int chaorec_rows_copy_by_bits_f32(float *dst, const float *src, int64_t n_rows, int32_t D, const uint32_t *bits, void *stream);
int chaorec_exchange_pull_sum_rows_f32(const void *const *peers, int32_t world, int64_t row0, int64_t n_block, int64_t n_rows,
                                       int32_t D, const uint32_t *bits, float *out, void *stream);
int chaorec_exchange_pull_gather_rows_f32(const void *const *peers, int32_t world, int64_t n_block, int64_t n_rows, int32_t D,
                                          const uint32_t *bits, float *out, void *stream);

/* The COMPACT form of a frontier exchange, for collectives that cannot skip rows (RCCL): the bitmap being the same on every
 * rank, "flagged row number k in bitmap order" names the same row everywhere.  pack: prefix[w] = flagged rows before word w
 * (prefix: int32 [n_words + 1] scratch, prefix[n_words] = their total), compact[k] = src[row k] for k < cap, the rest of
 * compact zeroed; the caller all-reduces compact ([cap, D]); unpack: dst[row k] = compact[k].  Rows beyond cap are dropped:
 * only for frontiers with a static bound (the batch items of all ranks: <= 2 B world). */
int chaorec_frontier_pack_f32(const float *src, int64_t n_rows, int32_t D, const uint32_t *bits, int32_t *prefix, float *compact,
                              int64_t cap, void *stream);
int chaorec_frontier_unpack_f32(float *dst, int64_t n_rows, int32_t D, const uint32_t *bits, const int32_t *prefix,
                                const float *compact, int64_t cap, void *stream);

/* ---------------------------------------------------------------------------------------
 * Several BPR terms over ONE user table and one batch of users (Model/FREEDOM.py:203-215:
 *   mf_loss + reg_weight * (mf_t_loss + mf_v_loss), each -mean(logsigmoid(s+ - s-)) over its own item table):
 *   losses[k] = BPR(tab_u[users], tabs[k][pos[k]], tabs[k][neg[k]]),  out_total = sum_k wvec[k] * losses[k]
 * T <= 4 terms; tabs / pos / neg / g_i: HOST arrays of T device pointers (copied into the kernel argument).
 * coef [T, B] and workspace [T, 4 B] floats are kept for the backward, which adds
 *   grad_out * wvec[k] * d losses[k]  into g_u (shared) and g_i[k] (atomic row adds; the buffers must be zero where no
 * sample lands).  wvec, grad_out: device pointers (grad_out may be NULL = 1).  Two launches forward, one backward.
 * ------------------------------------------------------------------------------------- */
int chaorec_bpr_multi_fwd_f32(const float *tab_u, const int64_t *users, int32_t T, const float *const *tabs,
                              const int64_t *const *pos, const int64_t *const *neg, int32_t B, int32_t D,
                              int32_t variant, const float *wvec, float *losses, float *out_total, float *coef,
                              float *workspace, void *stream);
/* scatter_rows / scatter_out (both NULL, or HOST arrays of T device pointers, entries NULL per term): term k's item table
 * is a block of rows gathered from a longer table (Model/FREEDOM.py:208-213 reads the batch rows of the projected feature
 * table: here only those rows are projected) -- row r of it is row scatter_rows[k][r] of that table, and the backward adds
 * its gradient ALSO into scatter_out[k][scatter_rows[k][r], :] (zero where no sample lands): the [I, D] row gradient the
 * feature table's optimizer takes, without a separate zero fill + index_add launch per table. */
int chaorec_bpr_multi_bwd_f32(const float *tab_u, const int64_t *users, int32_t T, const float *const *tabs,
                              const int64_t *const *pos, const int64_t *const *neg, int32_t B, int32_t D,
                              const float *coef, const float *wvec, const float *grad_out, float *g_u,
                              float *const *g_i, const int64_t *const *scatter_rows, float *const *scatter_out,
                              void *stream);
/* ... and its ordered, atomic-free form (see chaorec_bpr_bwd_ordered_f32): g_u, every g_i[k] and every scatter_out[k] must be
 * DISTINCT buffers (each is one group of rows with one owner wave per row).  The DEFINED order, restated by
 * oracle_bpr_multi_bwd_ordered_f32 and compared bit for bit (tests/test_gpu_bpr_multi.py): with
 * c = coef[k][b] * (grad_out * wvec[k]), a row of g_u takes the addends c * (p - n) of all terms, term by term and in batch
 * order inside a term; a row of g_i[k] first the batch's positive slots in batch order (c * u), then its negative slots
 * ((-c) * u); a row of scatter_out[k] the same two passes, keyed by scatter_rows[k][pos] / scatter_rows[k][neg].  Every
 * addend is rounded to float and added to the row's ONE running float sum, which starts from what the buffer holds.  Falls
 * back to the atomic launch (no defined order) beyond 16384 slots in a group (T B for the users, 2 B per table) or D > 256. */
int chaorec_bpr_multi_bwd_ordered_f32(const float *tab_u, const int64_t *users, int32_t T, const float *const *tabs,
                                      const int64_t *const *pos, const int64_t *const *neg, int32_t B, int32_t D,
                                      const float *coef, const float *wvec, const float *grad_out, float *g_u,
                                      float *const *g_i, const int64_t *const *scatter_rows, float *const *scatter_out,
                                      void *stream);

/* ---------------------------------------------------------------------------------------
 * Edge scores over the stored entries of a CSR: out[k] = <a[entry_row[k]], b[col[k]]>, k in [0, nnz).
 * Replaces the family's per-edge gather + product + row sum -- `torch.sum(x[row] * x[col], dim=1)` over an edge list
 * (Model/DCCF.py:109-111 cosine edge weights, Model/DDRec.py:197-204 the threshold filter, Model/GRCN.py:31 / Model/MGAT.py:43
 * attention logits) and the gradient torch.sparse.mm gives a sparse operand's values (d val[k] = <gy[row_k], x[col_k]>) --
 * which writes two [nnz, D] gathers and their product to HBM, by one pass that reads the two rows of every entry.
 * a [n_rows, D], b [n_cols, D] contiguous fp32, D a multiple of 4; entry_row / col int32 [nnz] (the CSR's entry -> row map and
 * column array).  Backward (through the caller's autograd): the two SpMMs  ga = G b,  gb = G^T a  over the same structure with
 * the incoming gradient as values (chaorec_spmm_csr_f32, CHAOREC_SPMM_DYNAMIC_VALUES).
 * ------------------------------------------------------------------------------------- */
int chaorec_edge_dot_f32(const int32_t *entry_row, const int32_t *col, const float *a, const float *b, float *out,
                         int64_t nnz, int32_t D, void *stream);

/* ---------------------------------------------------------------------------------------
 * MMGCN's layer tail in one pass each way (Model/MMGCN.py:102-131, per layer:
 *   h = F.leaky_relu(conv(x));  x_hat = F.leaky_relu(linear(x)) + id_embedding;  cat((h, x_hat), dim=1) ):
 *   out[r] = [ leaky_relu(s[r]) | u[r] + id[r] ]       s [n, d1], u / id [n, d2] (id may be NULL), out [n, d1 + d2]
 * and backwards from the concatenation's gradient:
 *   grad_s = g[:, :d1] * leaky'(cat[:, :d1]),  grad_u = g[:, d1:] * leaky'(uy),  grad_id (optional) = g[:, d1:]
 * (uy = the activated Linear output u; cat = the forward's output).  d1, d2 multiples of 4, everything contiguous.
 * ------------------------------------------------------------------------------------- */
int chaorec_leaky_cat_add_f32(const float *s, const float *u, const float *id, float *out, int64_t n_rows, int32_t d1,
                              int32_t d2, float slope, void *stream);
int chaorec_leaky_split_bwd_f32(const float *grad_cat, const float *cat, const float *uy, float *grad_s, float *grad_u,
                                float *grad_id, int64_t n_rows, int32_t d1, int32_t d2, float slope, void *stream);

/* F.normalize(torch.cat((a, b), dim=0), p=2, dim=1, eps) (Model/MMGCN.py:99-100) without the concatenation: rows
 * [0, rows_a) are read from a, rows [rows_a, n_rows) from b (b may be NULL when rows_a == n_rows); y [n_rows, D],
 * norm [n_rows] = |x_r| for the backward:  grad_x = (grad_y - y <grad_y, y>) / |x|  where |x| >= eps, grad_y / eps below;
 * rows < skip_rows of grad_x are left unwritten (the caller does not need them).  D a multiple of 4. */
int chaorec_normalize_rows_fwd_f32(const float *a, const float *b, int64_t rows_a, int64_t n_rows, int32_t D, float eps,
                                   float *y, float *norm, void *stream);
int chaorec_normalize_rows_bwd_f32(const float *grad_y, const float *y, const float *norm, int64_t skip_rows,
                                   int64_t n_rows, int32_t D, float eps, float *grad_x, void *stream);

/* ---------------------------------------------------------------------------------------
 * DGCF (Model/DGCF.py) -- csrc/dgcf.hip.  Intent state is ENTRY-MAJOR [E, K] (the reference keeps S as [K, E]); the graph is
 * the LightGCN-normalised CSR (norm = deg^-1/2[row] deg^-1/2[col], Model/DGCF.py:31-37) with eid [nnz] int32 = the undirected
 * edge (train_data row) of every entry.  Shapes: K in {1, 2, 4, 8}, D a power of two <= 256, D % (4K) == 0
 * (chaorec_dgcf_check_shape: 0 or CHAOREC_E_INVALID with the limit in chaorec_last_error()).
 * ------------------------------------------------------------------------------------- */
int chaorec_dgcf_check_shape(int32_t D, int32_t K);

/* P = softmax(S, over the K intents of every edge): `self.S = torch.softmax(self.S, dim=0)` (Model/DGCF.py:110). */
int chaorec_dgcf_softmax_f32(const float *S, float *P, int64_t E, int32_t K, void *stream);

/* One (layer, iteration) of DGCF.forward (Model/DGCF.py:112-140) over rows [row_begin, row_end): the K per-factor
 * conv_embed propagates of width D/K as one launch,  acc[r] = sum_e (norm_e * P[eid_e, k]) x[col_e]  with k = the slice of
 * the column;  y[r] = acc (y may be NULL),  zout[r] = z[r] + acc (zout may be NULL: the layer sum of :145, or the + G of the
 * backward).  Rows r < route_end are also ROUTED (:124-140, the user rows): per entry e of the row and intent k,
 *   S[eid_e, k] = P[eid_e, k] + < normalize(acc_k[r]), tanh(normalize(x_k[col_e])) >  and  P_next[eid_e, :] = softmax(S[eid_e, :])
 * (P_next != P: rows that are only propagated keep reading P).  route_end <= row_begin: no routing (S, P_next unused).
 * A_P is symmetric, so the backward is the same launch with the layer's P.  x, y, z, zout [n_rows, D] fp32, 16-byte aligned. */
int chaorec_dgcf_propagate_f32(const int64_t *rowptr, const int32_t *col, const float *norm, const int32_t *eid,
                               const float *P, const float *x, float *y, const float *z, float *zout, int64_t row_begin,
                               int64_t row_end, int64_t route_end, int32_t D, int32_t K, float *S, float *P_next,
                               void *stream);

/* DGCF.cor_loss (Model/DGCF.py:179-195 with utils.distance_correlation, utils.py:83-108): the n rows table[idx[i]] cut
 * into K slices, sum over k < K-1 of dCor(slice_k, slice_{k+1}), / ((K+1) K / 2) -> loss[0].  No n x n matrix: one pass
 * over the pairs gives every slice's distance row sums and the pair sums (ordered: per-workgroup partials, one fixed-order
 * combine, fp64 sums), so two runs give the same bits.  K >= 2.  The workspace (chaorec_dgcf_dcor_workspace_bytes) keeps
 * what the backward needs: pass it unchanged to chaorec_dgcf_dcor_bwd_f32. */
size_t chaorec_dgcf_dcor_workspace_bytes(int64_t n, int32_t D, int32_t K);
int chaorec_dgcf_dcor_fwd_f32(const float *table, const int64_t *idx, int64_t n, int32_t D, int32_t K, float *loss, void *ws,
                              size_t ws_bytes, void *stream);
/* The gradient of that loss times grad_out[0]: grad_rows [n, D] per gathered row, then grad_table [n_table_rows, D] =
 * zero except rows idx, which receive the sum over their repeats in gathered order (sorted_idx / perm: a stable sort of idx). */
int chaorec_dgcf_dcor_bwd_f32(const int64_t *sorted_idx, const int64_t *perm, int64_t n, int32_t D, int32_t K,
                              const float *grad_out, const void *ws, float *grad_rows, float *grad_table,
                              int64_t n_table_rows, void *stream);

/* ---------------------------------------------------------------------------------------
 * MultVAE (Model/MultVAE.py) -- csrc/multvae.hip.  Additive to ABI 16: new names only, no existing prototype changed.
 * Layouts: Wq_t [I, 128] row-major (layers_q.0.weight [128, I] transposed), bq [128], Wp [I, 64], bp [I], z [B, 64],
 * h = [mu | logvar] [B, 128].  The latent width is 64 (p_dims = [64], :38).  hist = (rowptr int64 [U + 1], col int32 LOCAL
 * item ids) is the user-history CSR; (item_ptr int64 [I + 1], item_users int32, item_pos int32 = the entry's place in its
 * user's history row) its item-major transpose; (slot_ptr int64 [U + 1], perm int64 [B]) a stable sort of the batch's users:
 * user u sits in samples perm[slot_ptr[u] .. slot_ptr[u + 1]).  state int64 [2] = {update_count, the count this step reads}.
 * Every gradient scale (gnll, gkl, gsq) is a device scalar.  No atomics: two runs give the same bits.
 * ------------------------------------------------------------------------------------- */
/* state[1] = state[0]; state[0] += 1; anneal[0] = min(cap, state[1] / total) (:145-148, :162; total <= 0: cap). */
int chaorec_multvae_tick(int64_t *state, float *anneal, float anneal_cap, int64_t total_anneal_steps, void *stream);

/* out[0] (+)= sum x^2 (torch.norm(p, 2) ** 2 of :127-136), two passes in a fixed order; partial [n_partial <= 4096]. */
int chaorec_multvae_sumsq_f32(const float *x, int64_t n, float *partial, int64_t n_partial, float *out, int32_t accumulate,
                              void *stream);

/* q_graph + the reparametrisation (:75-93, :113-114) for the B samples users[b], no [B, I] input:
 *   h_b = bq + s_b sum_{j : keep_bj} Wq_t[hist(u_b)_j, :],  s_b = 1 / max(sqrt(n_b), 1e-12) (/ keep_prob when training),
 *   z = mu + eps exp(logvar / 2),  klrow[b] = 0.5 sum(-logvar + exp(logvar) + mu^2 - 1),  kl[0] = mean_b klrow.
 * keep (uint8, sample 0's row, then sample 1's, ... with keep_off [B] the rows' starts) and eps_in [B, 64] are GIVEN draws;
 * NULL: the counter RNG (seed, state[1], sample, entry / column).  eps_out [B, 64] = the eps used. */
int chaorec_multvae_encode_fwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                   const float *Wq_t, const float *bq, const uint8_t *keep, const int64_t *keep_off,
                                   const float *eps_in, const int64_t *state, uint64_t seed, int32_t training,
                                   float keep_prob, float *h, float *z, float *eps_out, float *klrow, float *kl,
                                   void *stream);
/* Its backward from gz [B, 64], gkl [1] and gsq [1] (the gradient of the loss w.r.t. sum ||p||^2):
 *   dWq_t[i, :] = sum_{b, keep_bi} s_b dh_b + 2 gsq Wq_t[i, :]  (every row of Wq_t is written),  dbq = sum_b dh_b + 2 gsq bq.
 * sdh [B, 128] and partial [n_partial >= ceil(B / 64), 128] are scratch. */
int chaorec_multvae_encode_bwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, int64_t I,
                                   const int64_t *item_ptr, const int32_t *item_users, const int32_t *item_pos,
                                   const int64_t *slot_ptr, const int64_t *perm, const float *Wq_t, const float *bq,
                                   const uint8_t *keep, const int64_t *keep_off, const int64_t *state, uint64_t seed,
                                   int32_t training, float keep_prob, const float *h, const float *eps, const float *gz,
                                   const float *gkl, const float *gsq, float *sdh, float *partial, int64_t n_partial,
                                   float *dWq_t, float *dbq, void *stream);

/* The item splits of the sample-owned decoder passes (the first dimension of pm / ps / dzp). */
int64_t chaorec_multvae_decode_splits(int64_t B, int64_t I);
/* p_graph + log_softmax + the multinomial likelihood (:98-105, :155-156) with no [B, I] buffer:
 *   lse_b = logsumexp_i (z_b . Wp[i] + bp[i]),  nll_b = n_b lse_b - sum_{i in hist(u_b)} logit_bi,  neg_ll[0] = mean_b nll_b;
 * cnt [B] = n_b;  lse2 [2, B] = (the row maximum M, log of the sum rescaled by it): the backward forms exp((logit - M) - L),
 * near values subtracted first as log_softmax does.  pm, ps [splits, B]: scratch. */
int chaorec_multvae_decode_fwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                   const float *z, const float *Wp, const float *bp, int64_t I, float *pm, float *ps,
                                   int64_t splits, float *lse, float *lse2, float *cnt, float *nll, float *neg_ll,
                                   void *stream);
/* Its backward with P_bi = gnll n_b exp(logit_bi - lse_b) / B and X the multi-hot batch:
 *   dz = P Wp - gnll X Wp / B,  dWp = P^T z - gnll X^T z / B + 2 gsq Wp,  dbp = sum_b P - gnll sum_b x / B + 2 gsq bp.
 * dzp [splits, B, 64]: scratch. */
int chaorec_multvae_decode_bwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                   const int64_t *item_ptr, const int32_t *item_users, const int64_t *slot_ptr,
                                   const int64_t *perm, const float *z, const float *Wp, const float *bp, int64_t I,
                                   const float *lse2, const float *cnt, const float *gnll, const float *gsq, float *dzp,
                                   int64_t splits, float *dz, float *dWp, float *dbp, void *stream);

/* ---------------------------------------------------------------------------------------
 * MacridVAE (Model/MacridVAE.py) -- csrc/macridvae.hip.  Additive to ABI 16: new names only.
 * D = dim_E = 64, K = kfac = 10, H = 600 are what the kernels tile (any other value: CHAOREC_E_INVALID).  Layouts:
 * item_emb [I, D], k_emb [K, D], items [I, D] (normalised rows), cates [I, K], W1_t [I, H] row-major (encoder.0.weight
 * [H, I] transposed), a [B, K, H], zh [B, K, D] (the normalised z of every (sample, concept)).  hist, the item-major
 * transpose, (slot_ptr, perm) and the keep / keep_off flags: as for MultVAE above.  state int64 [2] = {update, the count
 * the step's draws are keyed by}.  No [B, I] or [B, K, I] buffer, no atomics: two runs give the same bits.
 * ------------------------------------------------------------------------------------- */
/* The largest [users, I] fp32 staging one chaorec_macrid_scores_f32 call may fill: the caller ranks users in ranges. */
#define CHAOREC_MACRID_STAGING_BYTES 536870912
/* CHAOREC_OK if the kernels tile (D, K, H). */
int chaorec_macrid_check_shape(int32_t D, int32_t K, int32_t H);
/* state[0] += 1; state[1] = state[0]; anneal[0] = min(cap, state[0] / total): incremented BEFORE it is read (:135-137). */
int chaorec_macrid_tick(int64_t *state, float *anneal, float anneal_cap, int64_t total_anneal_steps, void *stream);
/* out[e] = std * N(0, 1), e < n, from the counter RNG (seed, state[1], e): reparameterize's epsilon (:69). */
int chaorec_macrid_normal_f32(float *out, int64_t n, const int64_t *state, uint64_t seed, float std, void *stream);

/* Concept weights (:76-77, :86-94) in one pass over the item rows: items = normalize(item_emb),
 * cates = softmax(items . normalize(k_emb)^T / tau + g), g = the GIVEN Gumbel noise [I, K] or, NULL, -log(Exp(1)) from the
 * counter RNG (seed, state[1], item, k); training == 0: no noise. */
int chaorec_macrid_concept_fwd_f32(const float *item_emb, const float *k_emb, int64_t I, int32_t D, int32_t K, float tau,
                                   const float *gumbel, const int64_t *state, uint64_t seed, int32_t training, float *items,
                                   float *cates, void *stream);
/* Its backward from d_items [I, D] and d_cates [I, K]: d_item_emb [I, D], d_k_emb [K, D] (a fixed-order sum over items
 * through partial [n_partial >= ceil(I / 64), K, D]). */
int chaorec_macrid_concept_bwd_f32(const float *item_emb, const float *k_emb, int64_t I, int32_t D, int32_t K, float tau,
                                   const float *cates, const float *d_items, const float *d_cates, float *partial,
                                   int64_t n_partial, float *d_item_emb, float *d_k_emb, void *stream);

/* The encoder's first layer for all K concepts (:82-83, :101-105), no [B, I] input:
 *   a[b, k, :] = b1 + s_b sum_{j : keep_bj} cates[hist(u_b)_j, k] W1_t[hist(u_b)_j, :],  s_b = 1 / max(sqrt(n_b), 1e-12)
 * (/ keep_prob when training); a row of W1_t is read once per (sample, entry).  srow [B] = s_b.  keep / keep_off: GIVEN
 * flags; NULL: the counter RNG (seed, state[1], sample, entry).  Evaluation: training = 0, users = a range. */
int chaorec_macrid_encode_fwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                  const float *W1_t, const float *b1, const float *cates, int32_t K, int32_t H,
                                  const uint8_t *keep, const int64_t *keep_off, const int64_t *state, uint64_t seed,
                                  int32_t training, float keep_prob, float *a, float *srow, void *stream);
/* Its backward from da [B, K, H]:  dW1_t[i, :] = sum_{b, keep_bi} s_b sum_k cates[i, k] da_bk (every row is written),
 * d_cates[i, k] = sum_{b, keep_bi} s_b W1_t[i, :] . da_bk,  db1 = sum_{b, k} da_bk through partial
 * [n_partial >= ceil(B K / 64), H]. */
int chaorec_macrid_encode_bwd_f32(int64_t B, int64_t I, const int64_t *item_ptr, const int32_t *item_users,
                                  const int32_t *item_pos, const int64_t *slot_ptr, const int64_t *perm, const float *W1_t,
                                  const float *cates, int32_t K, int32_t H, const uint8_t *keep, const int64_t *keep_off,
                                  const int64_t *state, uint64_t seed, int32_t training, float keep_prob, const float *srow,
                                  const float *da, float *partial, int64_t n_partial, float *dW1_t, float *db1, float *d_cates,
                                  void *stream);

/* The item splits of the sample-owned likelihood passes (the first dimension of ps / dzp). */
int64_t chaorec_macrid_mix_splits(int64_t B, int64_t I);
/* The mixture likelihood (:119-126, :150) with p_bi = sum_k cates[i, k] exp(zh_bk . items_i / tau):
 *   lse_b = log sum_i p_bi,  nll_b = n_b lse_b - sum_{i in hist(u_b)} log p_bi,  ce[0] = mean_b nll_b;
 * coef [B] = n_b / (B sum_i p_bi) is what the backward reads.  |logit| <= 1 / tau, so no running maximum is kept.
 * ps [splits, K, B]: scratch. */
int chaorec_macrid_mix_fwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                               const float *zh, const float *items, const float *cates, int64_t I, int32_t D, int32_t K,
                               float tau, float *ps, int64_t splits, float *lse, float *coef, float *nll, float *ce,
                               void *stream);
/* Its backward, gce [1] = d loss / d ce, w_bi = gce (n_b p_bi / sum_i p_bi - x_bi) / B, r_bik = exp(l_bik) / p_bi:
 *   d_zh_bk = sum_i w_bi cates_ik r_bik items_i / tau,  d_items_i = sum_{b,k} w_bi cates_ik r_bik zh_bk / tau,
 *   d_cates_ik = sum_b w_bi r_bik.   dzp [splits, B, K, D]: scratch. */
int chaorec_macrid_mix_bwd_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                               const int64_t *item_ptr, const int32_t *item_users, const int64_t *slot_ptr,
                               const int64_t *perm, const float *zh, const float *items, const float *cates, int64_t I,
                               int32_t D, int32_t K, float tau, const float *coef, const float *gce, float *dzp,
                               int64_t splits, float *d_zh, float *d_items, float *d_cates, void *stream);

/* gene_ranklist's scores (:176-182) for the users user_begin .. user_begin + n_users: scores[u - user_begin, i] =
 * log p_ui, history entries (hist_rowptr int64 [U + 1], hist_col int64 LOCAL item ids) = mask_value.  n_users I 4 bytes
 * must not exceed CHAOREC_MACRID_STAGING_BYTES: the [U, I] matrix never exists whole. */
int chaorec_macrid_scores_f32(const float *zh, int64_t n_users, const float *items, const float *cates, int64_t I, int32_t D,
                              int32_t K, float tau, int64_t user_begin, const int64_t *hist_rowptr, const int64_t *hist_col,
                              float mask_value, float *scores, size_t scores_bytes, void *stream);
/* Exact top-k of every row of scores [n_rows, I] (1 <= topk <= 64, topk <= I), ties to the lowest index (torch.topk's
 * values, :185): idx [n_rows, topk] = column + id_offset, val [n_rows, topk]. */
int chaorec_macrid_topk_f32(const float *scores, int64_t n_rows, int64_t I, int32_t topk, int64_t id_offset, int64_t *idx,
                            float *val, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * DualVAE (Model/DualVAE.py) -- csrc/dualvae.hip.  Additive to ABI 16: new names only.
 * k = 25, a = 5, hidden = 20 are what the kernels tile.  One family serves both sides: a SAMPLE is a batch row (ids [B],
 * each in [0, S)), the TABLE is the other side's table [N, 5, 25] (theta or beta).  (rowptr int64 [S + 1], col int32) is
 * the samples' CSR over table rows, (tptr int64 [N + 1], tcol int32) its transpose, (slot_ptr [S + 1], perm [B]) the
 * batch's stable sort as for MultVAE above.  Layouts: z [B, 5, 25], zh = tanh(decoder(z)) [B, 5, 20],
 * th = tanh(decoder(table)) [N, 5, 20], w [N, 5] the aspect weights, We_t [N, 20] the encoder's first weight row-major
 * per table row.  s_bna = sigmoid(z_ba . T_na + tanh(zh_ba . th_na)), p_bn = sum_a w_na s_bna.
 * ------------------------------------------------------------------------------------------------------------------ */
/* The largest [users, I] fp32 staging one chaorec_dualvae_scores_f32 call may fill: the caller ranks users in ranges. */
#define CHAOREC_DUALVAE_STAGING_BYTES 536870912
/* CHAOREC_OK if the kernels tile (k, a, hidden). */
int chaorec_dualvae_check_shape(int32_t k, int32_t a, int32_t hidden);
/* state[0] += 1; state[1] = state[0]: the step counter the device-drawn epsilon is keyed by. */
int chaorec_dualvae_tick(int64_t *state, void *stream);
/* pre[b, a, :] = bias + sum_{n in row(ids[b])} w[n, a] We_t[n, :]  -> [B, 5, 20] (:195, :236 up to the first Linear). */
int chaorec_dualvae_encode_fwd_f32(const int64_t *ids, int64_t B, int64_t S, const int64_t *rowptr, const int32_t *col, int64_t N,
                                   const float *We_t, const float *bias, const float *w, float *pre, void *stream);
/* Its backward from dpre [B, 5, 20]: dWe_t [N, 20] and the sparse part of dw [N, 5], one owner per table row (every row
 * is written). */
int chaorec_dualvae_encode_bwd_f32(int64_t B, int64_t N, const int64_t *tptr, const int32_t *tcol, const int64_t *slot_ptr,
                                   const int64_t *perm, const float *We_t, const float *w, const float *dpre, float *dWe_t,
                                   float *dw, void *stream);
/* How many table splits the dense passes use for (B, N): psum is [splits, 5, B], pnei / dzp [splits, B, 5, 25], dzhp
 * [splits, B, 5, 20]. */
int64_t chaorec_dualvae_splits(int64_t B, int64_t N);
/* sum_p[b] = sum_n p_bn, xlog[b] = sum_{n in row(b)} log(p_bn + 1e-10), nei[b, a, :] = sum_n w_na s_bna T_na; no [B, N]
 * buffer: the tiles are recomputed on the f32 MFMA pipe, the splits added in ascending order. */
int chaorec_dualvae_dense_fwd_f32(const int64_t *ids, int64_t B, int64_t S, const int64_t *rowptr, const int32_t *col,
                                  const float *z, const float *zh, const float *table, const float *th, const float *w, int64_t N,
                                  float *psum, float *pnei, int64_t splits, float *sum_p, float *xlog, float *nei, void *stream);
/* Its backward from g1 [B] = d / d sum_p, g2 [B] = d / d xlog, gN [B, 5, 25] = d / d nei: dz [B, 5, 25], dzh [B, 5, 20],
 * dth [N, 5, 20], dw [N, 5] (the table itself carries no gradient). */
int chaorec_dualvae_dense_bwd_f32(const int64_t *ids, int64_t B, int64_t S, const int64_t *rowptr, const int32_t *col,
                                  const int64_t *tptr, const int32_t *tcol, const int64_t *slot_ptr, const int64_t *perm,
                                  const float *z, const float *zh, const float *table, const float *th, const float *w, int64_t N,
                                  const float *g1, const float *g2, const float *gN, float *dzp, float *dzhp, int64_t splits,
                                  float *dz, float *dzh, float *dth, float *dw, void *stream);
/* The small Linears' backward over R rows (gy [R, M], x [R, N], M <= 32, N <= 31): gw [M, N] = gy^T x, gb [M] = column sums
 * of gy, accumulated in double (the products are exact) and rounded once.  workspace: 8-byte aligned,
 * chaorec_dualvae_linear_bwd_workspace_bytes(R, M). */
size_t chaorec_dualvae_linear_bwd_workspace_bytes(int64_t R, int32_t M);
int chaorec_dualvae_linear_bwd_f32(const float *gy, const float *x, int64_t R, int32_t M, int32_t N, float *gw, float *gb,
                                   void *workspace, size_t workspace_bytes, void *stream);
/* One side's scalars from double sums, each rounded once: out[0] = kl_weight kl - ll + ssl_reg cl[0] (:274),
 * out[1] = kl = sum over the n_kl = B 5 25 elements of -0.5 (1 + 2 log std - mu^2 - std^2) / (5 B) with std = sigmoid(std_pre)
 * evaluated in double (:197-198, :216), out[2] = ll = (sum xlog - sum sum_p) / B.  workspace: 8-byte aligned, >= 512 bytes. */
int chaorec_dualvae_loss_f32(const float *mu, const float *std_pre, int64_t n_kl, const float *xlog, const float *sum_p, int64_t B,
                             const float *cl, float kl_weight, float ssl_reg, float *out, void *workspace, size_t workspace_bytes,
                             void *stream);
/* table[ids[b]] = z[b], mu_table[ids[b]] = mu[b] (:289-290, :300-301); where an id repeats, the highest batch position
 * wins. */
int chaorec_dualvae_writeback_f32(const int64_t *ids, int64_t B, int64_t S, const int64_t *slot_ptr, const int64_t *perm,
                                  const float *z, const float *mu, float *table, float *mu_table, void *stream);
/* gene_ranklist's scores (:314-327) for the users user_begin .. user_begin + n_users (z [n_users, 5, 25] their mu_theta
 * rows, zh their decoded rows): scores[u - user_begin, i] = sum_a w[i, a] s_uia with w AS GIVEN, history entries
 * (hist_rowptr int64 [U + 1], hist_col int64 LOCAL item ids) = mask_value.  n_users I 4 bytes must not exceed
 * CHAOREC_DUALVAE_STAGING_BYTES. */
int chaorec_dualvae_scores_f32(const float *z, const float *zh, int64_t n_users, const float *table, const float *th,
                               const float *w, int64_t I, int64_t user_begin, const int64_t *hist_rowptr, const int64_t *hist_col,
                               float mask_value, float *scores, size_t scores_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The user-user co-occurrence graph (Model/DRAGON.py; DualGNN, COHESION and MHRec read the same user_graph_dict.npy) --
 * csrc/usergraph.hip.  Additive to ABI 16: new names only.
 * ------------------------------------------------------------------------------------------------------------------ */
/* The largest U the entries below accept (user ids are 32-bit in every array): beyond it they return CHAOREC_E_INVALID. */
int64_t chaorec_usergraph_max_users(void);
/* How many user ids one LDS tile of chaorec_usergraph_build covers for (U, tile_users): min(U, 32768), capped by a
 * positive tile_users. */
int64_t chaorec_usergraph_tile_users(int64_t U, int32_t tile_users);
/* dualgnn-gen-u-u-matrix.py:20-50 and :90-103 (the dense [U, U] co-occurrence matrix and its per-row torch.topk) without
 * the matrix.  (hist_rowptr int64 [U + 1], hist_col int32 local item ids, no repeats) is the user-history CSR, (item_ptr
 * int64 [I + 1], item_users int32) its item-major transpose.  Row u of nbr_idx / nbr_cnt [U, N]: the users v != u with
 * c(u, v) = |items(u) & items(v)| > 0, by c descending then v ascending, cut at N <= 256; nbr_len[u] = how many; slots
 * past it hold 0 / 0.  tile_users: 0 = the kernel's own tile, else a cap on it (the result does not depend on it). */
int chaorec_usergraph_build(const int64_t *hist_rowptr, const int32_t *hist_col, const int64_t *item_ptr, const int32_t *item_users,
                            int64_t U, int64_t I, int32_t N, int32_t tile_users, int32_t *nbr_idx, int32_t *nbr_cnt,
                            int32_t *nbr_len, void *stream);
/* Model/DRAGON.py:231-270 (topk_sample), k <= N: epoch_idx int32 [U, k], epoch_w fp32 [U, k] = softmax over the k slots'
 * counts.  nbr_len >= k: the first k neighbours.  0 < nbr_len < k: slot j >= nbr_len copies slot r_j of the same row,
 * r_j = ((mix64(seed ^ mix64(epoch ^ mix64(u << 32 | j))) >> 32) * j) >> 32 (:249-252, the urn over the grown list).
 * nbr_len = 0: indices 0, weights 0 (:244-246). */
int chaorec_usergraph_sample(const int32_t *nbr_idx, const int32_t *nbr_cnt, const int32_t *nbr_len, int64_t U, int32_t N, int32_t k,
                             uint64_t seed, uint64_t epoch, int32_t *epoch_idx, float *epoch_w, void *stream);
/* Model/DRAGON.py:289-302 in one pass: with x[r, :] = (weight_u[r, 0] v[r, :], weight_u[r, 1] t[r, :]) (v, t fp32 [U, D],
 * weight_u [U, 2]), out[u, :] = x[u, :] + sum_j epoch_w[u, j] x[epoch_idx[u, j], :]  -> [U, 2 D]; the sum in ascending j,
 * product and add rounded separately, the residual last.  D is 64 or 128. */
int chaorec_usergraph_aggregate_fwd_f32(const float *v, const float *t, const float *weight_u, const int32_t *epoch_idx,
                                        const float *epoch_w, int64_t U, int32_t k, int32_t D, float *out, void *stream);
/* Its backward from g [U, 2 D].  (rev_ptr int64 [U + 1], rev_u int32, rev_w fp32): for every user r the slots (u, j) with
 * epoch_idx[u, j] = r in ascending (u, j), as their u and their epoch_w.  gx[r] = g[r] + sum rev_w g[rev_u] in that order;
 * dv[r] = weight_u[r, 0] gx[r, :D], dt[r] = weight_u[r, 1] gx[r, D:], dw[r] = (<gx[r, :D], v[r]>, <gx[r, D:], t[r]>).
 * One owner per row, no atomics: the same bits every run. */
int chaorec_usergraph_aggregate_bwd_f32(const float *g, const float *v, const float *t, const float *weight_u,
                                        const int64_t *rev_ptr, const int32_t *rev_u, const float *rev_w, int64_t U, int32_t D,
                                        float *dv, float *dt, float *dw, void *stream);

/* Model/DualGNN.py:189-239 in one pass over the whole result table of N = U + I rows (v, t fp32 [N, D], the two modality GCN
 * outputs; weight_u [U, 2]).  With x[r, :] = weight_u[r, 0] v[r, :] + weight_u[r, 1] t[r, :] for r < U:
 * result[u, :] = x[u, :] + sum_j epoch_w[u, j] x[epoch_idx[u, j], :] for u < U (ascending j, product and add rounded
 * separately, the residual last; a slot whose index lies outside [0, U) is skipped), result[r, :] = v[r, :] + t[r, :] for
 * r >= U.  N == U is legal.  D is 64 or 128. */
int chaorec_dualgnn_fuse_fwd_f32(const float *v, const float *t, const float *weight_u, const int32_t *epoch_idx,
                                 const float *epoch_w, int64_t U, int64_t N, int32_t k, int32_t D, float *result, void *stream);
/* Its backward from g [N, D] over the reverse structure of chaorec_usergraph_aggregate_bwd_f32: for r < U
 * gx[r] = g[r] + sum rev_w g[rev_u] in the list's order, dv[r] = weight_u[r, 0] gx[r], dt[r] = weight_u[r, 1] gx[r],
 * dw[r] = (<gx[r], v[r]>, <gx[r], t[r]>); for r >= U dv[r] = dt[r] = g[r].  dv, dt [N, D] and dw [U, 2] are written in
 * every element.  One owner per row, no atomics: the same bits every run. */
int chaorec_dualgnn_fuse_bwd_f32(const float *g, const float *v, const float *t, const float *weight_u, const int64_t *rev_ptr,
                                 const int32_t *rev_u, const float *rev_w, int64_t U, int64_t N, int32_t D, float *dv, float *dt,
                                 float *dw, void *stream);

/* Model/COHESION.py:340-359 in one pass over the whole result table of N = U + I rows.  idr, v, t fp32 [N, 64]: the three
 * modality tables (id, visual, textual), x[r, :] = (idr[r, :] | v[r, :] | t[r, :]), 192 floats that are never concatenated.
 * h_id, h_v, h_t fp32 [I, 64]: the item-graph terms mm_adj^L table[U:], all three given or all three NULL (mm_layers = 0).
 * result [N, 192]: result[u] = x[u] + sum_j epoch_w[u, j] x[epoch_idx[u, j]] for u < U (ascending j, product and add
 * rounded separately, the residual last; a slot whose index lies outside [0, U) is skipped); result[r] = x[r] + (h_id |
 * h_v | h_t)[r - U] for r >= U, x[r] itself without h tables.  N == U is legal.  D is 64. */
int chaorec_cohesion_fuse_fwd_f32(const float *idr, const float *v, const float *t, const float *h_id, const float *h_v,
                                  const float *h_t, const int32_t *epoch_idx, const float *epoch_w, int64_t U, int64_t N, int32_t k,
                                  int32_t D, float *result, void *stream);
/* Its backward from g [N, 192] to dv, dt [N, 64] and dh_v, dh_t [I, 64] (both or neither NULL).  The id third is detached
 * (Model/COHESION.py:321): columns 0 .. 63 of g are never read and nothing is written for them.  Item row r >= U:
 * dv[r] = dh_v[r - U] = g[r, 64:128], dt[r] = dh_t[r - U] = g[r, 128:192].  User row r: gx[r] = g[r, 64:192] + S_r,
 * dv[r] = gx[r, :64], dt[r] = gx[r, 64:].  THE ORDER OF S_r: row r's reverse list, entries [rev_ptr[r], rev_ptr[r + 1]) of
 * rev_u / rev_w (the structure of chaorec_usergraph_aggregate_bwd_f32), is cut into consecutive chunks of `chunk` entries
 * (the last may be shorter; chunk = 0: the whole list is one chunk); a chunk's partial is p_c = ((0 + w_1 g_1) + w_2 g_2)
 * + ... in list order, the row's sum S_r = ((p_0 + p_1) + p_2) + ... in chunk order, every product and add rounded
 * separately; an empty list gives S_r = 0.  The chunks are listed by the caller: chunk_row int32 [n_chunks] (the row a
 * chunk belongs to), chunk_first int64 [n_chunks] (its first entry), row_chunk int64 [U + 1] (row r's chunks are
 * [row_chunk[r], row_chunk[r + 1]), ascending); part fp32 [n_chunks, 128] is the workspace of the partials.  Two launches,
 * a lane group per chunk and then a lane group per row; no atomics: the same bits every run, whatever the grid.  Every
 * element of dv, dt, dh_v, dh_t is written.  D is 64. */
int chaorec_cohesion_fuse_bwd_f32(const float *g, const int64_t *rev_ptr, const int32_t *rev_u, const float *rev_w,
                                  const int32_t *chunk_row, const int64_t *chunk_first, const int64_t *row_chunk, int64_t n_chunks,
                                  int32_t chunk, int64_t U, int64_t N, int32_t D, float *part, float *dv, float *dt, float *dh_v,
                                  float *dh_t, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * MVGAE (Model/MVGAE.py) -- csrc/mvgae.hip.  Additive to ABI 16: new names only.
 * D = 64 is what the kernels tile (chaorec_mvgae_check_shape: CHAOREC_E_INVALID otherwise).  16 lanes hold a row (one
 * float4 each), a wave chaorec_mvgae_rows_per_wave() = 4 rows, a workgroup chaorec_mvgae_rows_per_block() = 16.  fp32, no
 * atomics: every sum has one owner and a fixed order.  state int64 [2]: chaorec_mvgae_tick does state[0] += 1,
 * state[1] = state[0]; every draw is keyed (seed, state[1], salt, counters) and a backward redraws its forward's values.
 * --------------------------------------------------------------------------------------------------------------- */
int chaorec_mvgae_check_shape(int32_t D);
int64_t chaorec_mvgae_rows_per_wave(void);
int64_t chaorec_mvgae_rows_per_block(void);
int chaorec_mvgae_tick(int64_t *state, void *stream);
/* The conv epilogue, per row r of s [N, 64]: a = s[r] + bias, n = |a|, q = a / max(n, 1e-12), y = leaky_relu(q m, 0.01);
 * m = 1 in evaluation; in training 1 / 0.9 for a kept element and 0 for a dropped one, kept = keep[r, d] != 0 (uint8 [N, 64])
 * or, keep NULL, uniform(seed, state[1], salt, r * 64 + d) >= 0.1.  salt in 0 .. 15: the conv's number. */
int chaorec_mvgae_conv_fwd_f32(const float *s, const float *bias, int64_t N, const uint8_t *keep, uint64_t seed,
                               const int64_t *state, int32_t salt, int32_t training, float *y, void *stream);
/* gs [N, 64] from gy: gq = gy (q m > 0 ? 1 : 0.01) m, gs = (gq - q <gq, q>) / n for n >= 1e-12, gq / 1e-12 below; q, n, m
 * recomputed from s, bias and the same draw.  The bias gradient is the column sum of gs. */
int chaorec_mvgae_conv_bwd_f32(const float *gy, const float *s, const float *bias, int64_t N, const uint8_t *keep,
                               uint64_t seed, const int64_t *state, int32_t salt, int32_t training, float *gs, void *stream);
/* The tail over six [N, 64] tables (mean, log-variance of the visual, textual, collaborative view) and a batch of B
 * samples of global row ids in [0, N).  PoE(a, b): t = 1 / (exp(l) + 1e-8), mean (ma ta + mb tb) / (ta + tb), log-variance
 * log(1 / (ta + tb)); P = PoE(PoE(V, T), C).  Views x = P, V, T, C: lc = min(l, 10), KL_x = -0.5 / N sum(1 + lc - m^2 -
 * exp(lc)), z = m + (eps 0.1) exp(0.5 lc) in training (m otherwise), BPR_x = -1 / B sum log(sigmoid(<zu, zp> - <zu, zn>) +
 * 1e-5).  eps: given [4, N, 64], or NULL: normal(seed, state[1], 16 + x, row, d).  Written whole: Pm [N, 64]; zrows
 * [4, 3, B, 64] (the z rows of user, positive, negative); eps_out likewise unless NULL; bpr, coef [4, B] (a sample's term and
 * its derivative by the score difference, 1 / B included; both from z rows and scores evaluated in double); out [9] = total,
 * BPR_P V T C, KL_P V T C (summed in double: strided per thread, then a tree, the same order every run).  workspace:
 * chaorec_mvgae_tail_workspace_bytes(N) bytes, 8-byte aligned.  Three launches. */
size_t chaorec_mvgae_tail_workspace_bytes(int64_t N);
int chaorec_mvgae_tail_fwd_f32(const float *Vm, const float *Vl, const float *Tm, const float *Tl, const float *Cm,
                               const float *Cl, int64_t N, const int64_t *users, const int64_t *pos, const int64_t *neg, int64_t B,
                               const float *eps, uint64_t seed, const int64_t *state, int32_t training, float kl_weight, float *Pm,
                               float *zrows, float *eps_out, float *bpr, float *coef, void *workspace, size_t workspace_bytes,
                               float *out, void *stream);
/* Its backward, one launch, every row of the six gradient tables written by its one owner: the KL terms, plus the dz of the
 * slots perm[slot_ptr[r] .. slot_ptr[r + 1]) -- perm int64 [3B] = a stable sort of [users; pos; neg], slot_ptr int64 [N + 1]
 * -- added in that order (as user, as positive, as negative, ascending sample number), then the reparametrisation (the
 * clamp passes gradient where l <= 10) and both PoE stages, times gtotal[0]. */
int chaorec_mvgae_tail_bwd_f32(const float *Vm, const float *Vl, const float *Tm, const float *Tl, const float *Cm,
                               const float *Cl, int64_t N, const int64_t *slot_ptr, const int64_t *perm, int64_t B,
                               const float *zrows, const float *coef, const float *eps, uint64_t seed, const int64_t *state,
                               int32_t training, float kl_weight, const float *gtotal, float *dVm, float *dVl, float *dTm,
                               float *dTl, float *dCm, float *dCl, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * DiffMM (Model/DiffMM.py) -- csrc/diffmm.hip.  Additive to ABI 16: new names only.  fp32, no float atomics, no scratch.
 * The embedding width of r and F is 64; H (the denoiser's hidden width) is a multiple of 4
 * (chaorec_diffmm_check_shape: CHAOREC_E_INVALID otherwise).  The output layer runs on the f32 MFMA pipe
 * (v_mfma_f32_32x32x2_f32): exact fp32 products in a k-ascending chain per element, as chaorec_gemm_f32, cut into segments
 * of 64 k whose values are added in ascending order -- not the three-plane bf16 split; chaorec_diffmm_tiles gives its tile (128 x 128 x 16), chaorec_diffmm_rows_per_block the rows of
 * a workgroup of the rows launch (4, a wave each).
 * --------------------------------------------------------------------------------------------------------------- */
int chaorec_diffmm_check_shape(int64_t B, int64_t I, int64_t H, int32_t D);
int chaorec_diffmm_tiles(int32_t *bm, int32_t *bn, int32_t *bk);
int64_t chaorec_diffmm_rows_per_block(void);
/* The denoiser's input rows without the dense [U, I] matrix and without a [B, I] batch, noise or x_t tensor
 * (dataload.DiffusionData, GaussianDiffusion.q_sample :580-592 called at :627-632, nn.Dropout(0.5) in Denoise.forward
 * :458-459).  Row b is user users[b]'s history row of the CSR (rowptr int64 [U + 1], col int32 local item ids; an id outside
 * [0, U) or a column outside [0, I) counts as absent): x0[b, i] in {0, 1}, x_t = fl(fl(a_row[b] x0) + fl(s_row[b] n)) -- two
 * roundings, no fused multiply-add --, x_in = kept ? fl(2 x_t) : 0.  n = noise[b, i] (fp32 [B, I]) or, noise NULL, a
 * Box-Muller normal keyed (seed, step, 2 salt, user id, item id); kept = keep[b, i] != 0 (uint8 [B, I]) or, keep NULL, a
 * uniform keyed (seed, step, 2 salt + 1, user id, item id) < 1/2: a draw does not depend on the row's place in the batch.
 * plain != 0: x_in = x0 (a_row, s_row, noise, keep unused): the multi-hot rows p_sample starts from at steps = 0 (:549-550).
 * x_in fp32 [B, ld], ld = I rounded up to a multiple of 4, columns I .. ld written 0; bits uint32 [B, ceil(I / 32)]: bit
 * i % 32 of word i / 32 is x0[b, i].  One launch, one wave per row. */
int chaorec_diffmm_rows_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col, int64_t I,
                            int64_t ld, const float *a_row, const float *s_row, const float *noise, const uint8_t *keep,
                            uint64_t seed, uint64_t step, uint32_t salt, int32_t plain, float *x_in, uint32_t *bits,
                            void *stream);
/* The same launch with x_in = x_t: the noised rows themselves, no input dropout and no keep draw (CF_Diff, Model/CF_Diff.py:
 * 84-96, encodes x_t and drops out after the encoder).  Arguments, keying of the noise and outputs as above. */
int chaorec_diffmm_rows_noised_f32(const int64_t *users, int64_t B, int64_t U, const int64_t *rowptr, const int32_t *col,
                                   int64_t I, int64_t ld, const float *a_row, const float *s_row, const float *noise,
                                   uint64_t seed, uint64_t step, uint32_t salt, float *x_t, uint32_t *bits, void *stream);
/* The output layer of Denoise.forward (:468-471) with GaussianDiffusion.training_losses' mse, weight, diff_loss and gc_loss
 * (:640-658) and the mean over the batch of both, in one pass; model_output, the squared error and usr_model_embeds do
 * not exist.  out = h W_out^T + b_out (h [B, H] row stride ldh, W_out [I, H] row stride ldw), err = out - x0 (x0 from bits
 * as above), r fp32 [B, 64] = out F - x0 E supplied by the caller as h (W_out^T F) + b_out F - x0 E, F fp32 [I, 64]:
 *   d_out[b, i] = c_row[b] err[b, i] + kf <r_b, F_i>        (fp32 [B, ldd], columns I .. ldd written 0)
 *   diff_rows[b] = w[b] / I sum_i err^2   (double; w double [B])      gc_rows[b] = mean_d r[b, d]^2
 *   loss[0] = mean_b diff_rows + e_loss mean_b gc_rows
 * With c_row[b] = 2 w[b] / (B I) and kf = 2 e_loss / (B 64), d_out is d loss / d out.  part fp32 [B, ceil(I / 128)] holds
 * every row's sum of err^2 per item tile; a second launch adds them in tile order, in double: no atomics, the same bits
 * every run. */
int chaorec_diffmm_out_loss_f32(const float *h, int64_t ldh, const float *W_out, int64_t ldw, const float *b_out,
                                const uint32_t *bits, const float *r, const float *F, const double *w, const float *c_row,
                                float kf, float e_loss, int64_t B, int64_t I, int64_t H, float *d_out, int64_t ldd,
                                float *part, double *diff_rows, float *gc_rows, float *loss, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * DiffRec (Model/DiffRec.py) -- csrc/diffrec.hip.  Additive to ABI 16: new names only.  fp32, no float atomics, no scratch,
 * the same bits every run.  One 128 x 128 x 16 tile loop on the f32 MFMA pipe (v_mfma_f32_32x32x2_f32) with two epilogues:
 * both operands [rows][k], k a multiple of 4 (chaorec_diffrec_check_shape: CHAOREC_E_INVALID otherwise, nothing launched),
 * rows 16-byte aligned, the k chain of an element cut into segments of 64 added in ascending order as DiffMM's.
 * chaorec_diffrec_tiles gives the tile.
 * --------------------------------------------------------------------------------------------------------------- */
int chaorec_diffrec_check_shape(int64_t B, int64_t I, int64_t H);
int chaorec_diffrec_tiles(int32_t *bm, int32_t *bn, int32_t *bk);
/* The output layer of DNN.forward (:86-89) with training_losses' mse, reweight_loss, the division by pt and the batch mean
 * (:445-461) in one pass; model_output does not exist.  out = h W_out^T + b_out (h [B, H] row stride ldh, W_out [I, H] row
 * stride ldw), err = out - x0 with x0 from bits (uint32 [B, ceil(I / 32)], bit i % 32 of word i / 32, as
 * chaorec_diffmm_rows_f32 writes it):
 *   d_out[b, i] = c_row[b] err[b, i]                   (fp32 [B, ldd], I <= ldd <= the end of the last item tile, columns I .. ldd written 0)
 *   reloss_rows[b] = w[b] / I sum_i err^2              (double; w double [B]: what update_Lt_history receives)
 *   loss[0] = mean_b reloss_rows[b] / pt[b]            (pt double [B])
 * With c_row[b] = 2 w[b] / (pt[b] B I), d_out is d loss / d out.  part fp32 [B, ceil(I / 128)] holds every row's sum of err^2
 * per item tile (columns in a fixed butterfly order); a second launch adds them in tile order, in double. */
int chaorec_diffrec_out_loss_f32(const float *h, int64_t ldh, const float *W_out, int64_t ldw, const float *b_out,
                                 const uint32_t *bits, const double *w, const double *pt, const float *c_row, int64_t B,
                                 int64_t I, int64_t H, float *d_out, int64_t ldd, float *part, double *reloss_rows,
                                 float *loss, void *stream);
/* One step of p_sample (:263-303 at sampling_steps = 0, no sampling noise) in the denoiser's hidden space:
 *   p_next[b, n] = c1 (sum_k z[b, k] G[n, k] + g0[n]) + c2 p[b, n],   z_next[b, n] = tanh(p_next[b, n] + e_next[n])
 * z fp32 [B, K] row stride ldz, G fp32 [N, K] row stride ldg, p fp32 [B, N] row stride ldp, g0 and e_next fp32 [N], p_next and
 * z_next fp32 [B, N] row stride ldo; c1, c2 the posterior-mean coefficients of the step (one t for the whole batch).  p_next
 * may be p itself; no other aliasing.  In DiffRec N = K = H, G = W1x W_out and g0 = W1x b_out. */
int chaorec_diffrec_chain_f32(const float *z, int64_t ldz, const float *G, int64_t ldg, const float *g0, const float *p,
                              int64_t ldp, const float *e_next, float c1, float c2, int64_t B, int64_t N, int64_t K,
                              float *p_next, float *z_next, int64_t ldo, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * LightGODE (Model/LightGODE.py:97-146) -- csrc/lightgode.hip.  Additive to ABI 16: new names only.  fp32, D = 64, no float
 * atomics, no scratch, the same bits every run.  The alignment + uniformity loss of a batch of B (user, item) pairs with the
 * pair terms on the f32 MFMA pipe (v_mfma_f32_32x32x2_f32); no [B, B] and no [B (B - 1) / 2] buffer.
 * chaorec_lightgode_check_shape: CHAOREC_E_INVALID for D != 64, B < 2 (the reference's mean over zero pairs) or B > 8192 (the
 * backward keeps the batch's ids in LDS); nothing launched.  chaorec_lightgode_workspace: the floats of `workspace` for B.
 * --------------------------------------------------------------------------------------------------------------- */
int chaorec_lightgode_check_shape(int64_t B, int32_t D);
int chaorec_lightgode_workspace(int64_t B, int32_t D, int64_t *n_floats);
/* x_b = normalize(tab_u[users[b]]), y_b = normalize(tab_i[items[b]]) (F.normalize: / max(|e|, 1e-12)); tab_u [U, 64], tab_i
 * [I, 64] (one joined table: tab_i = tab_u + item_offset * 64), ids int64 [B], LOCAL item ids.  Per side, with
 * e_ij = exp(-2 max(n_i + n_j - 2 <z_i, z_j>, 0)), r_i = sum_{j != i} e_ij and S = 1/2 sum_i r_i:
 *   out[4] = (loss, align, unif_u, unif_i): align = mean_b |x_b - y_b|^2, unif = log(S / (B (B - 1) / 2)),
 *            loss = align + gamma (unif_u + unif_i) / 2; loss[0] = out[0]
 *   row_grad fp32 [2, B, 64] (may be NULL): d loss / d the UN-normalised gathered rows, users' then items',
 *            (g - z <z, g>) / max(|e|, 1e-12) with g = (gamma / 2) (-4 / S) (r_i z_i - sum_{j != i} e_ij z_j) +- 2 (x_b - y_b) / B
 * Four launches (rows, centre, pairs, finish): the pair terms are evaluated on rows shifted by a common vector (a mean of 64 of
 * them), which distances do not see; the partial sums of the pair launch are added in split order, S in double. */
int chaorec_lightgode_loss_f32(const float *tab_u, const float *tab_i, int64_t U, int64_t I, const int64_t *users,
                               const int64_t *items, int64_t B, int32_t D, float gamma, float *workspace, int64_t ws_floats,
                               float *out, float *loss, float *row_grad, void *stream);
/* g_u[users[b]] += go row_grad[0, b], g_i[items[b]] += go row_grad[1, b]; go = *grad_out (device scalar) or 1 if NULL.  One
 * owner wave per table row, repeated ids added in batch order into the row's ONE running float sum, which starts from what the
 * buffer holds (zero-filled by the caller).  g_u and g_i may be the two parts of one joined buffer. */
int chaorec_lightgode_bwd_f32(const float *row_grad, const int64_t *users, const int64_t *items, int64_t B, int32_t D,
                              int64_t U, int64_t I, const float *grad_out, float *g_u, float *g_i, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * AdaGCL (Model/AdaGCL.py) -- csrc/adagcl.hip.  Additive to ABI 16: new names only.
 * The E-sized work of the two view generators over ONE symmetric-pattern CSR of N = U + I nodes: rowptr int64 [N + 1],
 * col int32 [E], entry_row int32 [E], tentry int32 [E] (the stored entry of the reversed pair).  D = 64 is what the keep
 * kernel tiles (chaorec_adagcl_check_shape: CHAOREC_E_INVALID otherwise).  A row is owned by 8 lanes, a row longer than
 * chaorec_adagcl_long_row() = 64 entries by its wave; chaorec_adagcl_rows_per_block() = 32 rows per workgroup, which is also
 * the number of rows behind one float of `part` (n_part >= ceil(N / 32)).  No float atomics: every sum has one owner and a
 * fixed order.  state int64 [2]: chaorec_adagcl_tick does state[0] += 1, state[1] = state[0] (the shared step tick of
 * csrc/draws.h, as chaorec_dualvae_tick and chaorec_mvgae_tick launch it); device draws are keyed (seed, state[1], salt, entry).
 * --------------------------------------------------------------------------------------------------------------- */
int chaorec_adagcl_check_shape(int32_t D);
int64_t chaorec_adagcl_rows_per_block(void);
int64_t chaorec_adagcl_long_row(void);
int chaorec_adagcl_tick(int64_t *state, void *stream);
/* DenoisingNet's hard-concrete edge gate (Model/AdaGCL.py:572-624, :647-689) from two per-node scores:
 *   logit[e] = s_nb[row e] + s_self[col e] + b_att[0]
 *   gate = sigmoid(logit) (training = 0) | sigmoid((log u - log(1 - u) + logit) / beta) (training != 0; evaluated in double
 *   and rounded once, as the reference's float64 draw makes it)
 *   m[e] = clamp(1.5 gate - 0.45, 0, 1), S[n] = sum_row m + eps, d[n] = clamp(S^-1/2, 0, 10), val[e] = m[e] d[row e] d[col e]
 *   l0[0] = mean_e sigmoid(logit[e] - beta log(0.45 / 1.05))
 * u fp32 [E] in [1e-7, 1 - 1e-7] given, or NULL: drawn in the launch; u_out (may be NULL) receives the values used.
 * Two launches; every output is written whole. */
int chaorec_adagcl_gate_fwd_f32(const int64_t *rowptr, const int32_t *col, const int32_t *entry_row, int64_t N, int64_t E,
                                const float *s_nb, const float *s_self, const float *b_att, float beta, float eps,
                                int32_t training, const float *u, uint64_t seed, const int64_t *state, int32_t salt, float *m,
                                float *S, float *d, float *val, float *l0, float *u_out, float *part, int64_t n_part,
                                void *stream);
/* Its backward: g_val fp32 [E] and g_l0 fp32 [1] (NULL = 0) -> g_s_nb [N], g_s_self [N], g_b [1]; g_logit [E] and g_S [N] are
 * scratch the three launches hand to each other; m, S, d as the forward wrote them, u the values it used. */
int chaorec_adagcl_gate_bwd_f32(const int64_t *rowptr, const int32_t *col, const int32_t *tentry, int64_t N, int64_t E,
                                const float *s_nb, const float *s_self, const float *b_att, float beta, int32_t training,
                                const float *u, const float *m, const float *S, const float *d, const float *g_val,
                                const float *g_l0, float *g_logit, float *g_S, float *g_s_nb, float *g_s_self, float *g_b,
                                float *part, int64_t n_part, void *stream);
/* vgae.generate's keep decision (Model/AdaGCL.py:483-501) per stored entry, on v_mfma_f32_32x32x2_f32 (exact fp32 products):
 *   logit[e] = w2 . relu(W1 relu(z[row e] * z[col e]) + b1) + b2[0], keep[e] = floor(sigmoid(logit) + 0.5) != 0
 *   out[e] = keep ? vals[e] / fl32(kept / E) : +0, kept[0] = the number of kept entries (0: out is all zero)
 * z fp32 [N, 64] (16-byte aligned), W1 [64, 64] row-major (out, in), b1 [64], w2 [64], b2 [1]; logit_out may be NULL.
 * Two launches and one 8-byte memset, no host synchronisation. */
int chaorec_adagcl_keep_f32(const float *z, int64_t N, const int32_t *entry_row, const int32_t *col, int64_t E, const float *W1,
                            const float *b1, const float *w2, const float *b2, const float *vals, uint8_t *keep, float *out,
                            int64_t *kept, float *logit_out, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Grade (Model/Grade.py) -- csrc/grade.hip.  Additive to ABI 16: new names only.  D = 64 is what the kernels tile
 * (chaorec_grade_check_shape: CHAOREC_E_INVALID otherwise).
 * The views of G independent generators (vgae.generate + normalize_adjacency_matrix) over AdaGCL's structure, three launches
 * with the generators in gridDim.y: z [G, N, 64], W1 [G, 64, 64], b1 [G, 64], w2 [G, 64], b2 [G]; owner int32 [P]: the
 * entries with entry_row[e] <= col[e] (each undirected pair once; every entry is e or tentry[e] of exactly one of them).
 *   logit = w2 . relu(W1 relu(z[row] * z[col]) + b1) + b2, p = sigmoid(logit), keep = floor(p + 0.5) != 0, computed once per
 *   pair and written to both of its entries; S[n] = sum_row (keep ? p : 0) + 1e-7f, d[n] = S^-1/2;
 *   val[e] = val[tentry[e]] = (d[row e] p[e]) d[col e] at the owner e, +0 where dropped.
 * -> val fp32 [G, E], keep uint8 [G, E], kept int64 [G] (stored entries kept; zeroed here), d fp32 [G, N], logit_out fp32
 * [G, E] or NULL.  No float atomics: two runs give the same bits, and val[tentry[e]] has the bits of val[e].
 * --------------------------------------------------------------------------------------------------------------- */
int chaorec_grade_check_shape(int32_t D);
int chaorec_grade_views_f32(const float *z, const float *W1, const float *b1, const float *w2, const float *b2, int32_t G,
                            int64_t N, const int64_t *rowptr, const int32_t *col, const int32_t *entry_row,
                            const int32_t *tentry, int64_t E, const int32_t *owner, int64_t P, float *val, uint8_t *keep,
                            int64_t *kept, float *logit_out, float *d, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * GraphAug (Model/GraphAug.py) -- csrc/graphaug.hip.  Additive to ABI 16: new names only.  D = 64 is what the kernels
 * tile (chaorec_graphaug_check_shape: CHAOREC_E_INVALID otherwise).  No float atomics: every output has one owner and
 * every sum a fixed order, so two runs on the same inputs give the same bits.
 * --------------------------------------------------------------------------------------------------------------- */
int chaorec_graphaug_check_shape(int32_t D);
int64_t chaorec_graphaug_rows_per_block(void);
int64_t chaorec_graphaug_long_row(void);
/* The view learner's edge sampler (Model/GraphAug.py:268-309) per stored entry e = (row, col) of a symmetric-pattern CSR
 * (rowptr int64 [N + 1], col int32 [E], tentry int32 [E]: the stored entry of the reversed pair), forward only, fp32:
 *   logit = b2[0] + sum_j w2[j] relu((P[row][j] + b1[j]) + Q[col][j])     P = z W1[:, :64]^T, Q = z W1[:, 64:]^T, fp32 [N, 64]
 *   eps = -0.9998 u1 + 0.9999;  att = clamp(sigmoid(log eps - log(1 - eps) + logit), 0.01, 0.99)
 *   u2' = clamp(u2, 2^-23, 1 - 2^-23);  s = clamp(sigmoid((log u2' - log1p(-u2') + log att - log1p(-att)) / 0.9), FLT_MIN, 1 - 2^-23)
 *   val[e] = s > 0.2 ? s : +0
 * A row is owned by 8 lanes (chaorec_graphaug_rows_per_block() = 32 rows per workgroup), a row longer than
 * chaorec_graphaug_long_row() = 64 entries by its wave.  u1, u2 fp32 [E] given, or NULL: drawn in the launch, keyed
 * (seed, state[1], salt, entry) -- state int64 [2] as the shared step tick keeps it (any of the three *_tick exports); u_out fp32 [2, E] (may be NULL) receives
 * the draws used.  val_t (may be NULL): val_t[tentry[e]] = val[e]; logit_out may be NULL.  One launch. */
int chaorec_graphaug_sample_f32(const int64_t *rowptr, const int32_t *col, const int32_t *tentry, int64_t N, int64_t E,
                                const float *P, const float *Q, const float *b1, const float *w2, const float *b2,
                                const float *u1, const float *u2, uint64_t seed, const int64_t *state, int32_t salt, float *val,
                                float *val_t, float *logit_out, float *u_out, void *stream);
/* lse[b] = log sum_m exp(<A_b, T_m> inv_temp) for A fp32 [B, 64], T fp32 [M, 64] (16-byte aligned): a plain sum, no running
 * max -- for normalised rows, as contrastLoss (Model/GraphAug.py:534-541) has them.  v_mfma_f32_32x32x2_f32; per-split
 * partials part fp32 [splits, B], splits = chaorec_graphaug_lse_splits(B, M), added in split order (in double) by a second
 * launch.  lse fp32 [2, B]: row 0 the result, row 1 what its rounding to fp32 lost (the backward subtracts both in turn). */
int64_t chaorec_graphaug_lse_splits(int64_t B, int64_t M);
int chaorec_graphaug_lse_fwd_f32(const float *A, const float *T, int64_t B, int64_t M, float inv_temp, float *part, int64_t splits,
                                 float *lse, void *stream);
/* Its backward for g fp32 [B] and lse [2, B] as the forward wrote it: w_bm = g_b inv_temp exp(<A_b, T_m> inv_temp - lse_b), dA_b = sum_m w_bm T_m (per-split partials
 * part fp32 [splits, B, 64], added in split order), dT_m = sum_b w_bm A_b (one owner per 64 table rows, looping over B).
 * Three launches; dA and dT are written whole. */
int chaorec_graphaug_lse_bwd_f32(const float *A, const float *T, int64_t B, int64_t M, float inv_temp, const float *lse,
                                 const float *g, float *part, int64_t splits, float *dA, float *dT, void *stream);
/* y[n] = act(z[n] + alpha sum_{e in row n} x[col e]) over the CSR of a step's random entries (rowptr int64 [n_rows + 1], col
 * int32), x fp32 [n_cols, 64], z (may be NULL) and y fp32 [n_rows, 64]; act = LeakyReLU(slope), slope = 1: none.  A wave per
 * row, the entries in order. */
int chaorec_graphaug_rand_spmm_f32(const int64_t *rowptr, const int32_t *col, int64_t n_rows, int64_t n_cols, const float *x,
                                   const float *z, float alpha, float slope, float *y, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * MHRec (Model/MHRec.py) -- csrc/mhrec.hip.  Additive to ABI 16: new names only.  The hypergraph attention layer
 * (HypergraphAttentionLayer.forward, :53-89) with the epilogue the model applies after it (:724-726), fp32, D = 64
 * (chaorec_mhrec_check_shape: CHAOREC_E_INVALID otherwise).  No float atomics: every output has one owner and every sum
 * a fixed order, so two runs on the same inputs give the same bits.
 *
 * The hypergraph: E hyperedges of exactly k distinct nodes, all values 1.  nodes int32 [E, k] (H^T as an ELL table) and the
 * node-major CSR of the same pairs: rowptr int64 [N + 1], edge int32 [E k], a node's hyperedges ascending.  A node row of
 * more than chaorec_mhrec_long_row() entries is cut into chunks of chaorec_mhrec_chunk() entries: long_node int32 [L],
 * long_cptr int64 [L + 1] (a long row's chunks), chunk_node int32 [C], chunk_beg int64 [C] (a chunk's first CSR entry);
 * L = 0: the four may be NULL.  A lane group of 16 lanes x float4 holds a row, chaorec_mhrec_rows_per_block() = 16 groups
 * per workgroup.
 * --------------------------------------------------------------------------------------------------------------- */
int chaorec_mhrec_check_shape(int32_t D);
int64_t chaorec_mhrec_long_row(void);
int64_t chaorec_mhrec_chunk(void);
int64_t chaorec_mhrec_rows_per_block(void);
/* Forward, X fp32 [N, 64], a fp32 [128] = [a1; a2]:
 *   Eo[j] = sum_{n in j} X_n (table order), r[j] = <Eo_j, a2>                                       hyperedge launch
 *   s_n = <X_n, a1>, alpha_nj = exp(s_n + r_j) / (sum_{j of n} exp(s_n + r_j) + 1e-16), out_n = sum_{j of n} alpha_nj Eo_j
 *   y_n = keep ? 2 (out_n + X_n) : 0                                                               node launch
 * evaluated with the exponent shifted by the row's maximum, the 1e-16 scaled alike.  stat fp32 [N, 4] =
 * (-max_j r_j, 1 / denominator, scaled 1e-16 / denominator, s_n) is what the backward re-forms alpha from; a node in no
 * hyperedge: out_n = 0, stat = (0, 0, 0, s_n).  keep: uint8 [N, 64] given flags, or NULL: with training != 0 element (n, d) is
 * kept when draw_uniform<24>(key(seed, state[1], salt), n, d) >= 0.5 (state int64 [2] as the step tick keeps it), with
 * training == 0 there is no dropout and y = out + X.  Sums over a row's entries and the dot products run in double and are
 * rounded once.  Long rows: pacc double [C, 64], pz double [C, 2] receive the chunks' partials, a further launch adds them in
 * chunk order.  Two launches, four with long rows; Eo [E, 64], r [E], out and y
 * [N, 64] are written whole. */
int chaorec_mhrec_layer_fwd_f32(const int32_t *nodes, int64_t E, int32_t k, const int64_t *rowptr, const int32_t *edge, int64_t N,
                                const int32_t *long_node, const int64_t *long_cptr, int64_t L, const int32_t *chunk_node,
                                const int64_t *chunk_beg, int64_t C, const float *X, const float *a, const uint8_t *keep,
                                uint64_t seed, const int64_t *state, int32_t salt, int32_t training, float *Eo, float *r,
                                float *stat, float *out, float *y, double *pacc, double *pz, void *stream);
/* Backward for g = dL/dy fp32 [N, 64] with the forward's Eo, r, stat, out and the same mask / draw arguments:
 *   gm_n = keep ? 2 g_n : 0, t_n = <gm_n, out_n>                                                    node prologue
 *   de_nj = alpha_nj (<gm_n, Eo_j> - t_n), dE_j = sum_{n in j} alpha_nj gm_n + a2 sum_{n in j} de_nj  hyperedge launch
 *   dX_n = gm_n + sum_{j of n} dE_j + a1 sde_n, sde_n = sum_{j of n} de_nj = t_n stat[n][2]                node launch
 * pa2 fp32 [ceil(E / 16), 64] and pa1 fp32 [ceil(N / 16), 64] receive one partial row per workgroup of
 * da2 = sum_j Eo_j sum_{n in j} de_nj and da1 = sum_n X_n sde_n: chaorec_colsum_f32 over each gives the gradient of a.
 * gm [N, 64], tn [N], dE [E, 64] are workspaces written whole, pacc double [C, 64] as in the forward.  Three launches,
 * five with long rows. */
int chaorec_mhrec_layer_bwd_f32(const int32_t *nodes, int64_t E, int32_t k, const int64_t *rowptr, const int32_t *edge, int64_t N,
                                const int32_t *long_node, const int64_t *long_cptr, int64_t L, const int32_t *chunk_node,
                                const int64_t *chunk_beg, int64_t C, const float *g, const float *X, const float *a,
                                const float *Eo, const float *r, const float *stat, const float *out, const uint8_t *keep,
                                uint64_t seed, const int64_t *state, int32_t salt, int32_t training, float *gm, float *tn,
                                float *dE, float *dX, float *pa1, float *pa2, double *pacc, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * BSPM (Model/BSPM.py:133-181) -- csrc/bspm.hip.  Additive to ABI 16: new names only.  The training-free blur / sharpen
 * filter for a tile of B users (B a multiple of 4 in [4, 1024]: the SpMM's rule for its feature width), in item space:
 * P = Rn^T Rn as a CSR (p_ptr int64 [I + 1], p_col int32, p_val fp32, nnz entries) and the ODE state transposed,
 * Yt fp32 [I, B].  Xt, the tile's rows of Rn transposed, is a tile-local CSR over items: xt_ptr int64 [I + 1], xt_slot
 * int32 (the slot within the tile, ascending inside an item), xt_val fp32, nxt entries.  No float atomics: every output
 * has one owner and every sum a fixed order, so two runs on the same inputs give the same bits.
 * chaorec_bspm_check_shape: CHAOREC_E_INVALID unless B is as above and m a multiple of 4 in [4, 128].
 * chaorec_bspm_long_row(): a row of P with more entries is shared by the four waves of a last_step workgroup.
 * --------------------------------------------------------------------------------------------------------------- */
int chaorec_bspm_check_shape(int64_t I, int64_t B, int64_t m);
int64_t chaorec_bspm_long_row(void);
/* Z[b, :] = sum_e x_val[e] F[x_item[e], :] over slot b's entries x_ptr[b] .. x_ptr[b + 1] in order (x_ptr int64 [B + 1],
 * nx entries); F fp32 [I, m], Z fp32 [B, m] written whole. */
int chaorec_bspm_project_f32(const int64_t *x_ptr, const int32_t *x_item, const float *x_val, int64_t nx, const float *F,
                             int64_t I, int64_t B, int64_t m, float *Z, void *stream);
/* Y0t[j, :] = beta idlT[j, :] + sum_{i in P_j} P_ji Xt[i, :], the entries of P_j in CSR order; only the stored entries of
 * Xt are walked.  idlT fp32 [I, B] may be NULL when beta is 0.  Y0t fp32 [I, B] written whole. */
int chaorec_bspm_seed_f32(const int64_t *p_ptr, const int32_t *p_col, const float *p_val, int64_t nnz, int64_t I,
                          const int64_t *xt_ptr, const int32_t *xt_slot, const float *xt_val, int64_t nxt, int64_t B,
                          float beta, const float *idlT, float *Y0t, void *stream);
/* scores[b, j] = Yt[j, b] - h (P Yt)[j, b] with the SpMM epilogue's roundings for alpha = -h, beta = 1, then mask_value at
 * the (j, slot) pairs of xt_ptr / xt_slot (xt_ptr NULL: no mask); scores fp32 [B, I] row-major, written whole, not Yt's
 * memory.  h = 0: the masked transpose of Yt, bit for bit. */
int chaorec_bspm_last_step_f32(const int64_t *p_ptr, const int32_t *p_col, const float *p_val, int64_t nnz, int64_t I,
                               const float *Yt, int64_t B, float h, const int64_t *xt_ptr, const int32_t *xt_slot, int64_t nxt,
                               float mask_value, float *scores, void *stream);

/* ---------------------------------------------------------------------------------------------------------------
 * CF_Diff (Model/CF_Diff.py:108-111) -- csrc/cfdiff.hip.  Additive to ABI 16: new names only.  The core of
 * nn.MultiheadAttention(16, 4, dropout = 0.5): 4 heads of width 4 over L tokens, never forming an [L, L] array.  q, k, v, out
 * and their gradients fp32 [B, L, 16] contiguous, 16-byte aligned, head h in columns 4h .. 4h + 3, one L for queries and
 * keys; scores <q, k> / 2.  fp32, no float atomics, no scratch; every output row has one owner and every sum runs in
 * ascending index order (in segments of 32 terms): the same bits every run.
 * A workgroup owns one (b, head) and stages 32 bytes (forward, query pass) or 48 bytes (key pass) per token in LDS, at most
 * 64 KiB: chaorec_cfdiff_max_len() = 1365, and two workgroups are resident on a CU at any accepted L.
 * chaorec_cfdiff_check_shape: CHAOREC_E_INVALID unless 1 <= L <= max_len and 1 <= B <= 2^28.
 *
 * The keep flags of the rate-1/2 dropout on the probabilities: training == 0: none.  Otherwise keep uint8 [B, 4, L, L]
 * (given; non-zero = kept) or, keep NULL, device draws: flag (b, head, query i, key j) is bit (j & 63) of the 64-bit draw
 *   mix64(key ^ mix64((((b0 + b) * 4 + head) << 32) ^ ((i << 20) | (j >> 6)))),  key = mix64(mix64(seed ^ salt) + state[1])
 * (csrc/draws.h: draw_bits64 over draw_key; state int64 [2] as the step tick keeps it) -- one draw serves the 64 keys of an
 * aligned key word, a set bit is a kept entry.  b0 is the slot of the launch's first row (0 <= b0, b0 + B <= 2^30): a row's
 * flags depend on its slot, not on the launch geometry or on the launch it is part of.
 * --------------------------------------------------------------------------------------------------------------- */
int64_t chaorec_cfdiff_max_len(void);
int chaorec_cfdiff_check_shape(int64_t B, int64_t L);
/* out = (keep ? 2 P : 0) V (training == 0: P V), P = softmax over ALL keys of the scores (F.dropout after the softmax); a
 * query whose keys are all dropped gives exact zeros.  lse fp32 [B, 4, L] = log sum_j exp(score). */
int chaorec_cfdiff_attn_fwd_f32(const float *q, const float *k, const float *v, int64_t B, int64_t L, int32_t training,
                                const uint8_t *keep, uint64_t seed, const int64_t *state, uint32_t salt, int64_t b0, float *out,
                                float *lse, void *stream);
/* dq, dk, dv from the forward's operands, out, lse and dout, with the same draw arguments: the flags are redrawn, no mask is
 * stored.  D_i = <dout_i, out_i>, dS_ij = P_ij (2 keep_ij <dout_i, v_j> - D_i), dq_i = 1/2 sum_j dS_ij k_j,
 * dk_j = 1/2 sum_i dS_ij q_i, dv_j = sum_i 2 keep_ij P_ij dout_i.  Two launches: the query pass writes dq and rnorm fp32
 * [B, 4, L] (1 / sum_j exp(score - lse): the rounding of the stored lse, taken out of P again), the key pass reads it. */
int chaorec_cfdiff_attn_bwd_f32(const float *q, const float *k, const float *v, const float *out, const float *lse,
                                const float *dout, int64_t B, int64_t L, int32_t training, const uint8_t *keep, uint64_t seed,
                                const int64_t *state, uint32_t salt, int64_t b0, float *dq, float *dk, float *dv, float *rnorm,
                                void *stream);
/* The device-drawn flags of (seed, state[1], salt, b0) as bytes, keep uint8 [B, 4, L, L]: for the plain composition and
 * the tests, which reproduce a device-drawn step with them. */
int chaorec_cfdiff_attn_keep_u8(int64_t B, int64_t L, uint64_t seed, const int64_t *state, uint32_t salt, int64_t b0,
                                uint8_t *keep, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CHAOREC_HIP_H */
