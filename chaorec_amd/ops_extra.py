"""Optimizer and model-specific wrappers: Adam launches (single tensor, multi-tensor, the low-rank feature-table update),
ops.linear_rows (a Linear over gathered rows), and the kernels of the sparse.mm model family (edge dropout, dynamic-value
SpMM, NGCF's layer, weighted sampling without replacement, LayerGCN's row re-weighting).  Moved out of ops.py in round 5
 with no behaviour change; `chaorec_amd.ops` re-exports every name here."""
import ctypes
import os  # noqa: F401

import torch

from . import _lib
from . import ops as _ops
from .ops import RowScatterToken, _f32c, _need_cuda, _ptr, _stream, col_sum, spmm_raw  # noqa: F401
from .ops_dense import gemm_nn_bf16x3, gemm_nt_bf16x3, gemm_raw, gemm_tn_bf16x3  # noqa: F401


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
              step_dev=None, numel=None):
    """One fused Adam launch over a flat fp32 tensor.  `step_dev` (int32 device scalar) overrides `step` so the
    launch can be captured in a hipGraph.  `numel` > param.numel(): the four arrays continue contiguously past this
    tensor (adjacent parameters updated by one launch, see optim.FusedAdam)."""
    _need_cuda(param, grad, exp_avg, exp_avg_sq, step_dev)
    _lib.load().chaorec_adam_step_f32(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                                      param.numel() if numel is None else int(numel),
                                      lr, betas[0], betas[1], eps, weight_decay, int(step), _ptr(step_dev), _stream())


def adam_bias_table(n_steps, betas, device):
    """float [n_steps, 2]: (1 - beta1^s, sqrt(1 - beta2^s)) per step s (entry 0 unused), computed by the device with the
    same double-precision expression every Adam launch uses for its own step."""
    t = torch.empty((int(n_steps), 2), dtype=torch.float32, device=device)
    _lib.load().chaorec_adam_bias_table(_ptr(t), int(n_steps), betas[0], betas[1], _stream())
    return t


def unique_rows(rows, claim, stamp_dev, out_list, out_count):
    """out_list[0 .. out_count[0]) = the distinct ids in `rows` (int64, duplicates allowed), any order; `claim` int32
    [n_rows] and `stamp_dev` int32 [1]: scratch the launches keep between them (zero-initialised once)."""
    _need_cuda(rows, claim, stamp_dev, out_list, out_count)
    rows = rows.to(torch.int64).contiguous()
    if out_list.numel() < rows.numel():
        raise ValueError("unique_rows: the list must hold as many ids as `rows`")
    _lib.load().chaorec_unique_rows(_ptr(rows), rows.numel(), claim.numel(), _ptr(claim), _ptr(stamp_dev),
                                    _ptr(out_list), _ptr(out_count), _stream())


def adam_lowrank_strips(K):
    return int(_lib.load().chaorec_adam_lowrank_strips(int(K)))


def adam_lowrank(param, gy, weight, exp_avg, exp_avg_sq, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 step_dev=None, mode=0, last=None, bc_table=None, rowlist=None, rows_given=True):
    """Adam on a feature table [n, K] whose gradient is gy [n, R] @ weight [R, K], never materialised
    (chaorec_adam_lowrank_f32).  mode 0: every row, every step; 1: only the rows with a non-zero gy row, after they
    caught up on the zero-gradient steps they sat out (`last` int32 [strips, n]); 2: flush -- every row catches up;
    3: the rows flagged by a non-zero row of `gy` catch up (before a forward reads them).
    rowlist (modes 1, 3): (list int32 [cap], count int32 [1]); rows_given: filled by unique_rows -- visit exactly these
    rows; else scratch (cap >= n) the launch fills with the rows whose gy (flag) row is non-zero."""
    _need_cuda(param, exp_avg, exp_avg_sq, step_dev, last, bc_table)
    if rowlist is None and mode in (1, 3):               # scratch for the launch's own row scan
        rowlist = (torch.empty(param.shape[0], dtype=torch.int32, device=param.device),
                   torch.empty(1, dtype=torch.int32, device=param.device))
        rows_given = False
    rl, rc_, cap = (rowlist[0], rowlist[1], rowlist[0].numel()) if rowlist is not None else (None, None, 0)
    _need_cuda(rl, rc_)
    n, K = param.shape
    R = 1
    if mode <= 1:
        _need_cuda(gy, weight)
        gy, weight = _f32c(gy), _f32c(weight)
        if tuple(gy.shape) != (n, weight.shape[0]) or weight.shape[1] != K:
            raise ValueError(f"adam_lowrank: param {tuple(param.shape)} gy {tuple(gy.shape)} weight {tuple(weight.shape)}")
        R = weight.shape[0]
    elif mode == 3 and gy is not None:
        _need_cuda(gy)
        gy = _f32c(gy)                                   # row flags [n, R]
        if gy.dim() != 2 or gy.shape[0] != n:
            raise ValueError(f"adam_lowrank: flags {tuple(gy.shape)} for a table of {n} rows")
        R = gy.shape[1]
    if not (param.is_contiguous() and exp_avg.is_contiguous() and exp_avg_sq.is_contiguous()):
        raise ValueError("adam_lowrank: contiguous tables")
    _lib.load().chaorec_adam_lowrank_f32(_ptr(param), _ptr(gy if mode != 2 else None),
                                         _ptr(weight if mode <= 1 else None), _ptr(exp_avg), _ptr(exp_avg_sq),
                                         n, K, R, lr, betas[0], betas[1], eps, weight_decay, int(step),
                                         _ptr(step_dev), int(mode), _ptr(last), _ptr(bc_table),
                                         0 if bc_table is None else bc_table.shape[0], _ptr(rl), _ptr(rc_), cap,
                                         int(bool(rows_given)), _stream())


class _LinearRows(torch.autograd.Function):
    """y = (x W^T + b)[rows], computed on the gathered rows only (a row of a Linear depends on that row alone).
    Model/FREEDOM.py:209-213 projects the whole trainable feature table every step and then reads the 2 B rows of the
    batch: 2 B x K instead of I x K of reads, and a gradient  gy W  that is non-zero in those rows only.  When the
    optimizer has claimed x (optim.FusedAdam, chaorec_adam_lowrank_f32) the [I, K] gradient is never formed: the
    optimizer receives gy (scattered to [I, R]) and W instead; otherwise x.grad is the usual dense tensor."""

    @staticmethod
    def forward(ctx, x, rows, weight, bias, scatter_token=None):
        sink = getattr(x, "_chaorec_lowrank_sink", None)
        ctx.scatter_token = scatter_token
        ctx.row_token = None
        if sink is not None and sink.lazy_rows and sink.accepts(x):
            ctx.row_token = sink.catch_up(x, rows)       # lazily updated table: these rows must be current first
        xg = x.index_select(0, rows)
        if _ops.LINEAR_FORWARD == "bf16x3" and xg.shape[1] >= 64 and xg.shape[0] >= 256:
            y = gemm_nt_bf16x3(xg, weight, bias=bias)
        else:
            y = gemm_raw(xg, weight, transB=True, bias=bias)
        ctx.save_for_backward(xg, rows, weight)
        ctx.x_param, ctx.has_bias = x, bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        xg, rows, weight = ctx.saved_tensors
        x = ctx.x_param
        gy = gy.contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            gy_full = ctx.scatter_token.take(x.shape[0], gy.shape[1], rows) if ctx.scatter_token is not None else None
            if gy_full is None:                          # (else: already scattered by the multi-term BPR backward's launch)
                gy_full = torch.zeros((x.shape[0], gy.shape[1]), dtype=gy.dtype, device=gy.device)
                gy_full.index_add_(0, rows, gy)          # an item can sit in the batch more than once
            sink = getattr(x, "_chaorec_lowrank_sink", None)
            if sink is not None and sink.accepts(x):
                sink.submit(x, gy_full, weight, ctx.row_token)
            elif _ops.LINEAR_FORWARD == "bf16x3" and weight.shape[0] >= 64 and gy_full.shape[0] >= 256:
                gx = gemm_nn_bf16x3(gy_full, weight)
            else:
                gx = gemm_raw(gy_full, weight)
        gw = gemm_raw(gy, xg, transA=True) if ctx.needs_input_grad[2] else None
        gb = col_sum(gy) if ctx.has_bias and ctx.needs_input_grad[3] else None
        return gx, None, gw, gb, None


def linear_rows(x, rows, weight, bias=None):
    """== linear(x, weight, bias)[rows].  The result carries a RowScatterToken (`_chaorec_row_scatter`): a bpr_loss_multi
    that takes it as a gathered term hands this node the already scattered row gradient through it."""
    token = RowScatterToken()
    y = _LinearRows.apply(x, rows, weight, bias, token)
    y._chaorec_row_scatter = token
    return y


def adam_multi(tensors, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step_dev=None):
    """One Adam launch over several small tensors: `tensors` = [(param, grad, exp_avg, exp_avg_sq, numel)], at most
    adam_multi_max() of them (chaorec_adam_multi_f32; same arithmetic as adam_step)."""
    n = len(tensors)
    if n == 0:
        return
    arr = lambda vals: (ctypes.c_void_p * n)(*vals)
    for t in tensors:
        _need_cuda(t[0], t[1], t[2], t[3])
    numel = (ctypes.c_int64 * n)(*[int(t[4]) for t in tensors])
    _lib.load().chaorec_adam_multi_f32(n, arr([t[0].data_ptr() for t in tensors]),
                                       arr([t[1].data_ptr() for t in tensors]),
                                       arr([t[2].data_ptr() for t in tensors]),
                                       arr([t[3].data_ptr() for t in tensors]), numel, lr, betas[0], betas[1], eps,
                                       weight_decay, int(step), _ptr(step_dev), _stream())


def adam_multi_max():
    return int(_lib.load().chaorec_adam_multi_max())


class _SpMMAdd(torch.autograd.Function):
    """y = A x + z in one launch (FREEDOM's `i_g_embeddings + h`, Model/FREEDOM.py:168,181)."""

    @staticmethod
    def forward(ctx, x, z, csr):
        ctx.csr = csr
        return _ops.spmm_raw(csr, x, z=_f32c(z), beta=1.0)

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        return _ops.spmm_raw(ctx.csr.t(), gy), gy, None


def spmm_add(csr, x, z):
    return _SpMMAdd.apply(x, z, csr)


# --------------------------------------------------------------------------------------------
# per-step edge dropout (NGCF) and weighted edge sampling (FREEDOM)
# --------------------------------------------------------------------------------------------
def edge_dropout_norm(structure, p, seed, step=0, step_dev=None, salt=0, keep=None):
    """Values of the dropped-and-renormalised graph and of its transpose over graph.DropoutStructure (one call per
    NGCFConv.forward, Model/NGCF.py:38-58).  Returns (val, val_t), both fp32 [nnz] in the structure's entry order.
    `keep` (uint8 [nnz], optional) replaces the generator with an externally drawn mask."""
    _need_cuda(structure.col, step_dev, keep)
    nnz = structure.nnz
    dev = structure.col.device
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    val_t = torch.empty(nnz, dtype=torch.float32, device=dev)
    if keep is not None:
        keep = keep.to(torch.uint8).contiguous()
    _lib.load().chaorec_edge_dropout_norm(_ptr(structure.entry_row), _ptr(structure.col),
                                          _ptr(structure.transpose_entry), nnz, structure.n_rows, float(p),
                                          int(seed) & (2**64 - 1), int(step), _ptr(step_dev), int(salt),
                                          _ptr(keep), _ptr(structure.deg_ws), _ptr(val), _ptr(val_t), _stream())
    return val, val_t


def edge_dot_raw(entry_row, col, a, b, n_entries=None):
    """out[k] = <a[entry_row[k]], b[col[k]]> for the first n_entries stored entries (all of them by default): one pass that
    reads two rows per entry (chaorec_edge_dot_f32) instead of two [nnz, D] gathers, their product and its row sum."""
    _need_cuda(a, b, entry_row, col)
    for name, t in (("entry_row", entry_row), ("col", col)):      # (the kernel reads 4-byte indices: an int64 tensor would be
        if t.dtype != torch.int32 or not t.is_contiguous():       #  read as pairs of int32 -- garbage rows, out-of-bounds gathers)
            raise TypeError(f"edge_dot: {name} must be a contiguous int32 tensor, got {t.dtype}, contiguous={t.is_contiguous()}")
    a, b = _f32c(a), _f32c(b)
    if a.dim() != 2 or b.dim() != 2 or a.shape[1] != b.shape[1]:
        raise ValueError(f"edge_dot: a {tuple(a.shape)} and b {tuple(b.shape)} must be 2-D with the same width")
    n = int(col.numel()) if n_entries is None else int(n_entries)
    if n < 0 or n > int(col.numel()) or n > int(entry_row.numel()):
        raise ValueError(f"edge_dot: n_entries={n} beyond the {int(col.numel())} stored entries / {int(entry_row.numel())} entry rows")
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    _lib.load().chaorec_edge_dot_f32(_ptr(entry_row), _ptr(col), _ptr(a), _ptr(b), _ptr(out), n, a.shape[1], _stream())
    return out


class _EdgeDot(torch.autograd.Function):
    """Edge scores over (the first n entries of) a symmetric-pattern structure, differentiable in both tables: with G the sparse
    matrix that holds the incoming gradient at those entries,  d a = G b,  d b = G^T a  -- two dynamic-values SpMMs."""

    @staticmethod
    def forward(ctx, a, b, structure, n):
        ctx.structure, ctx.n = structure, n
        ctx.save_for_backward(a, b)
        return edge_dot_raw(structure.entry_row, structure.col, a, b, n)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        st, n = ctx.structure, ctx.n
        g = g.contiguous()
        if n != st.nnz:
            g = torch.cat([g, g.new_zeros(st.nnz - n)])
        ga = _ops.spmm_raw(st.with_values(g), _f32c(b)) if ctx.needs_input_grad[0] else None
        gb = _ops.spmm_raw(st.with_values(g[st.transpose_entry.long()]), _f32c(a)) if ctx.needs_input_grad[1] else None
        return ga, gb, None, None


def edge_dot(structure, a, b, n_entries=None):
    """<a[row_k], b[col_k]> per stored entry k of `structure` (a graph.DropoutStructure: symmetric pattern, entry -> row and
    entry -> reversed-entry maps), or of its first n_entries entries -- the (user, item) half of the bipartite structures
    the models build --, with autograd into both tables.  Needs a.shape[0] = b.shape[0] = the structure's node count."""
    return _EdgeDot.apply(a, b, structure, structure.nnz if n_entries is None else int(n_entries))


class _SpMMValues(torch.autograd.Function):
    """y = A x where A's values change every call (edge dropout, learned edge weights) while its structure is fixed:
    forward with `val`, backward with `val_t` (A^T in the same structure).  Values that require a gradient get one
    (what torch.sparse.mm gives a sparse operand's values): d val[k] = <gy[row_k], x[col_k]> per stored entry -- `val_t`
    is only the transposed COPY the backward SpMM reads, no gradient flows through it."""

    @staticmethod
    def forward(ctx, x, structure, val, val_t):
        ctx.structure = structure
        ctx.val_grad = ctx.needs_input_grad[2]
        ctx.save_for_backward(val_t, x if ctx.val_grad else None)
        return _ops.spmm_raw(structure.with_values(val.detach()), x)

    @staticmethod
    def backward(ctx, gy):
        val_t, x = ctx.saved_tensors
        st, gy = ctx.structure, gy.contiguous()
        gx = _ops.spmm_raw(st.with_values(val_t.detach()), gy) if ctx.needs_input_grad[0] else None
        gval = edge_dot_raw(st.entry_row, st.col, gy, x) if ctx.val_grad else None
        return gx, None, gval, None


def spmm_values(structure, val, val_t, x):
    return _SpMMValues.apply(x, structure, val, val_t)


class _NGCFLayer(torch.autograd.Function):
    """leaky_relu_0.2(s W1^T + (s * x) W2^T): the dense half of NGCFConv (Model/NGCF.py:68-84) as two MFMA GEMM launches
    (the second accumulating into the first's output with the activation in its epilogue) after one product launch;
    backward: the activation's mask in one launch (chaorec_leaky_bwd_f32), four GEMMs, and the product's backward plus
    the sum into s's other gradient in one launch (chaorec_mul_pair_bwd_f32)."""

    @staticmethod
    def forward(ctx, s, x, w1, w2):
        t = s * x
        y = gemm_raw(s, w1, transB=True)
        gemm_raw(t, w2, transB=True, out=y, accumulate=True, act=2)
        ctx.save_for_backward(s, x, w1, t, w2, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        s, x, w1, t, w2, y = ctx.saved_tensors
        lib = _lib.load()
        gy = gy.contiguous()
        g = torch.empty_like(gy)
        lib.chaorec_leaky_bwd_f32(_ptr(y), _ptr(gy), 0.2, _ptr(g), g.numel(), _stream())
        gs = gemm_raw(g, w1)
        gt = gemm_raw(g, w2)
        gx = torch.empty_like(x)
        lib.chaorec_mul_pair_bwd_f32(_ptr(gt), _ptr(s), _ptr(x), _ptr(gs), _ptr(gx), gs.numel(), _stream())
        gw1 = gemm_raw(g, s, transA=True) if ctx.needs_input_grad[2] else None
        gw2 = gemm_raw(g, t, transA=True) if ctx.needs_input_grad[3] else None
        return gs, gx, gw1, gw2


def ngcf_layer(s, x, w1, w2):
    """leaky_relu_0.2(s W1^T + (s * x) W2^T) for [N, D] tables with D a multiple of 4."""
    _need_cuda(s, x, w1, w2)
    return _NGCFLayer.apply(_f32c(s), _f32c(x), w1, w2)


def weighted_sample_keep(weights, k, seed, step=0, step_dev=None, return_keys=False):
    """uint8 [n] keep mask of a weighted sample without replacement of k of the n entries (FREEDOM's
    torch.multinomial(edge_values, k), Model/FREEDOM.py:151, as a set; any n)."""
    _need_cuda(weights, step_dev)
    weights = _f32c(weights)
    n = weights.numel()
    lib = _lib.load()
    nbytes = lib.chaorec_weighted_sample_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=weights.device)
    keep = torch.empty(n, dtype=torch.uint8, device=weights.device)
    keys = torch.empty(n, dtype=torch.int64, device=weights.device) if return_keys else None
    lib.chaorec_weighted_sample_keep(_ptr(weights), n, int(k), int(seed) & (2**64 - 1), int(step), _ptr(step_dev),
                                     _ptr(ws), nbytes, _ptr(keep), _ptr(keys), _stream())
    return (keep, keys) if return_keys else keep


def weighted_sample_keys(weights, ids=None, seed=0, step=0, step_dev=None):
    """int64 [n] race keys of chaorec_weighted_sample_keep alone, entry j numbered ids[j] (its number in the whole
    edge list; None: j): one rank's share of a sharded pruning (dist.ShardedFREEDOM).  Non-negative as int64 for
    positive weights; entries with weight <= 0 get -1 (all 64 bits set: never among the k smallest of the unsigned order)."""
    _need_cuda(weights, ids, step_dev)
    weights = _f32c(weights)
    n = weights.numel()
    if ids is not None:
        ids = ids.to(torch.int64).contiguous()
        if ids.numel() != n:
            raise ValueError("weighted_sample_keys: ids and weights differ in length")
    keys = torch.empty(n, dtype=torch.int64, device=weights.device)
    _lib.load().chaorec_weighted_sample_keys(_ptr(weights), _ptr(ids), n, int(seed) & (2**64 - 1), int(step),
                                             _ptr(step_dev), _ptr(keys), _stream())
    return keys


# --------------------------------------------------------------------------------------------
# row-wise cosine re-weighting (LayerGCN)
# --------------------------------------------------------------------------------------------
class _RowCosineScale(torch.autograd.Function):
    """out = cosine_similarity(y, e, dim=-1)[:, None] * y (Model/LayerGCN.py:125-127): one launch forward, one backward."""

    @staticmethod
    def forward(ctx, y, e):
        _need_cuda(y, e)
        y, e = _f32c(y), _f32c(e)
        out = torch.empty_like(y)
        _lib.load().chaorec_row_cosine_scale_fwd_f32(_ptr(y), _ptr(e), _ptr(out), None, y.shape[0], y.shape[1], _stream())
        ctx.save_for_backward(y, e)
        return out

    @staticmethod
    def backward(ctx, g):
        y, e = ctx.saved_tensors
        g = g.contiguous()
        gy, ge = torch.empty_like(y), torch.empty_like(e)
        _lib.load().chaorec_row_cosine_scale_bwd_f32(_ptr(g), _ptr(y), _ptr(e), _ptr(gy), _ptr(ge), y.shape[0],
                                                     y.shape[1], _stream())
        return gy, ge


def row_cosine_scale(y, e):
    return _RowCosineScale.apply(y, e)


# --------------------------------------------------------------------------------------------
# DGCF (csrc/dgcf.hip): intent-weighted propagation with routing, distance correlation
# --------------------------------------------------------------------------------------------
def dgcf_check_shape(D, K, n_layers=1, n_iterations=1):
    """The shapes csrc/dgcf.hip supports; anything else raises ValueError naming the limit."""
    if int(n_layers) < 1 or int(n_iterations) < 1:
        raise ValueError(f"DGCF: n_layers={n_layers}, n_iterations={n_iterations} (both must be >= 1)")
    lib = _lib.load()
    if lib.chaorec_dgcf_check_shape(int(D), int(K)) != 0:
        raise ValueError(lib.chaorec_last_error().decode())


def dgcf_softmax(S, P):
    """P = softmax(S) over the K intents of every edge (entry-major [E, K])."""
    _need_cuda(S, P)
    _lib.load().chaorec_dgcf_softmax_f32(_ptr(S), _ptr(P), S.shape[0], S.shape[1], _stream())


def dgcf_propagate_raw(g, P, x, y=None, z=None, zout=None, rows=None, route_end=0, S=None, P_next=None):
    """One chaorec_dgcf_propagate_f32 launch over graph g (graph.DGCFStructure) with intent weights P [E, K]: rows
    [rows[0], rows[1]) (default all), y = A_P x, zout = z + A_P x; rows below route_end are routed (S, P_next written)."""
    _need_cuda(g.rowptr, P, x, y, z, zout, S, P_next)
    x = _f32c(x)
    D, K = x.shape[1], P.shape[1]
    r0, r1 = rows if rows is not None else (0, g.n_rows)
    _lib.load().chaorec_dgcf_propagate_f32(_ptr(g.rowptr), _ptr(g.col), _ptr(g.val), _ptr(g.eid), _ptr(P), _ptr(x),
                                           _ptr(y), _ptr(z), _ptr(zout), int(r0), int(r1), int(route_end), D, K,
                                           _ptr(S), _ptr(P_next), _stream())
    return y if y is not None else zout


def dgcf_p_schedule(n_layers, n_iterations):
    """Which buffer every (layer, iteration) reads its intent weights from and writes the next ones to, as names:
    'state' (the persistent P = softmax(S)), ('saved', l) (kept for layer l's backward: the P its LAST iteration reads),
    ('scratch', 0 / 1).  The last launch writes 'state' again; no launch writes the buffer it reads."""
    L, T = int(n_layers), int(n_iterations)
    LT = L * T
    src, dst = [None] * LT, [None] * LT
    src[0] = "state" if T > 1 else ("saved", 0)          # (T == 1: layer 0's P must outlive the last launch's write)
    for j in range(LT):
        if j > 0:
            src[j] = dst[j - 1]
        if j == LT - 1:
            dst[j] = "state"
        elif (j + 1) % T == T - 1:
            dst[j] = ("saved", (j + 1) // T)
        else:
            dst[j] = ("scratch", 1) if src[j] == ("scratch", 0) else ("scratch", 0)
    return src, dst


def dgcf_forward_raw(x0, g, S, P, n_layers, n_iterations, result=None):
    """DGCF.forward (Model/DGCF.py:84-152) from ego_0 = x0: result = ego_0 + ... + ego_L; S / P (entry-major [E, K],
    P = softmax(S)) are updated in place, L * T times.  -> (result, the per-layer P's the backward reads)."""
    L, T = int(n_layers), int(n_iterations)
    N, U = x0.shape[0], g.num_user
    saved = [torch.empty_like(P) for _ in range(L)]
    scratch = [torch.empty_like(P) for _ in range(min(2, max(T - 1, 0)))]
    buf = {"state": P}
    buf.update({("saved", l): t for l, t in enumerate(saved)})
    buf.update({("scratch", i): t for i, t in enumerate(scratch)})
    src, dst = dgcf_p_schedule(L, T)
    if T == 1:
        dgcf_softmax(S, saved[0])
    result = torch.empty_like(x0) if result is None else result
    egos = [torch.empty_like(x0), torch.empty_like(x0)] if L > 1 else [torch.empty_like(x0)]
    ego = x0
    for l in range(L):
        nxt = egos[l % len(egos)]
        for t in range(T):
            j = l * T + t
            if t < T - 1:           # an iteration whose X only feeds the routing: the user rows alone
                dgcf_propagate_raw(g, buf[src[j]], ego, y=nxt, rows=(0, U), route_end=U, S=S, P_next=buf[dst[j]])
            else:                   # the layer's output: every row, user rows routed, the layer sum in the epilogue
                dgcf_propagate_raw(g, buf[src[j]], ego, y=nxt, z=x0 if l == 0 else result, zout=result, route_end=U,
                                   S=S, P_next=buf[dst[j]])
        ego = nxt
    return result, saved


class _DGCFForward(torch.autograd.Function):
    """result = sum_l ego_l with ego_{l+1} = A_{P_l} ego_l, P_l held constant (the scores reach S through
    nn.Embedding.from_pretrained, which detaches them: Model/DGCF.py:127-130).  Backward: g_L = G, g_l = G + A_{P_l} g_{l+1}
    (A_P is symmetric), one launch per layer."""

    @staticmethod
    def forward(ctx, x0, g, S, P, n_layers, n_iterations):
        _need_cuda(x0, S, P)
        x0 = _f32c(x0)
        result, saved = dgcf_forward_raw(x0, g, S, P, n_layers, n_iterations)
        ctx.g, ctx.saved_p = g, saved
        return result

    @staticmethod
    def backward(ctx, G):
        G = _f32c(G)
        cur = G
        for P_l in reversed(ctx.saved_p):
            cur = dgcf_propagate_raw(ctx.g, P_l, cur, z=G, zout=torch.empty_like(G))
        return cur, None, None, None, None, None


def dgcf_forward(x0, g, S, P, n_layers, n_iterations):
    return _DGCFForward.apply(x0, g, S, P, int(n_layers), int(n_iterations))


class _DGCFCor(torch.autograd.Function):
    """DGCF.cor_loss over table rows idx (chaorec_dgcf_dcor_fwd_f32 / _bwd_f32) -> [1]."""

    @staticmethod
    def forward(ctx, table, idx, K):
        _need_cuda(table, idx)
        table = _f32c(table)
        idx = idx.to(torch.int64).contiguous()
        n, D = idx.numel(), table.shape[1]
        lib = _lib.load()
        ws = torch.empty(lib.chaorec_dgcf_dcor_workspace_bytes(n, D, K), dtype=torch.uint8, device=table.device)
        loss = torch.empty(1, dtype=torch.float32, device=table.device)
        lib.chaorec_dgcf_dcor_fwd_f32(_ptr(table), _ptr(idx), n, D, K, _ptr(loss), _ptr(ws), ws.numel(), _stream())
        ctx.save_for_backward(idx)
        ctx.ws, ctx.K, ctx.shape = ws, K, tuple(table.shape)
        return loss

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        n, (N, D) = idx.numel(), ctx.shape
        sorted_idx, perm = torch.sort(idx, stable=True)
        grad_rows = torch.empty((n, D), dtype=torch.float32, device=idx.device)
        grad_table = torch.empty((N, D), dtype=torch.float32, device=idx.device)      # (zeroed by the launch itself)
        _lib.load().chaorec_dgcf_dcor_bwd_f32(_ptr(sorted_idx), _ptr(perm), n, D, ctx.K, _ptr(g.contiguous()), _ptr(ctx.ws),
                                              _ptr(grad_rows), _ptr(grad_table), N, _stream())
        return grad_table, None, None


def dgcf_cor_loss(table, idx, K):
    """sum_{k < K-1} dCor(slice_k, slice_{k+1}) / ((K+1) K / 2) of the rows table[idx] ([1]; exactly 0 for K == 1)."""
    if int(K) < 2:
        return torch.zeros(1, dtype=torch.float32, device=table.device)
    return _DGCFCor.apply(table, idx, int(K))


# --------------------------------------------------------------------------------------------
# The autoencoders (csrc/multvae.hip, macridvae.hip, dualvae.hip over csrc/vae_common.h): what the three share
# --------------------------------------------------------------------------------------------
# MultVAEStructure has three users: MultVAE and MacridVAE walk the user-history CSR with it, DualVAE builds one per side
# (rows = that side's samples, columns = the other side's table rows).  It keeps the name of its first user.
class MultVAEStructure:
    """What the autoencoder kernels walk: the user-history CSR (rowptr int64 [U + 1], col int32 local item ids, ascending)
    and its item-major transpose with every entry's place in its user's row (graph.item_major_hist)."""

    def __init__(self, rowptr, col, num_item):
        from .graph import item_major_hist
        self.num_user, self.num_item = int(rowptr.numel() - 1), int(num_item)
        self.rowptr, self.col = rowptr.to(torch.int64).contiguous(), col.to(torch.int32).contiguous()
        self.item_ptr, self.item_users, self.item_pos = item_major_hist(self.rowptr.cpu(), self.col.cpu(), self.num_item)
        self.user_ids = torch.arange(self.num_user + 1, dtype=torch.int64)

    def to(self, device):
        for k in ("rowptr", "col", "item_ptr", "item_users", "item_pos", "user_ids"):
            setattr(self, k, getattr(self, k).to(device))
        return self

    def batch(self, users):
        """users int64 [B] -> (users, slot_ptr [U + 1], perm [B]): user u sits in samples perm[slot_ptr[u] : slot_ptr[u + 1]],
        ascending (a stable sort; capturable: no host decision)."""
        users = users.to(torch.int64).contiguous()
        sorted_u, perm = torch.sort(users, stable=True)
        return users, torch.searchsorted(sorted_u, self.user_ids).contiguous(), perm.contiguous()

    def keep_offsets(self, users):
        """Where each sample's keep flags start when they are GIVEN (sample 0's history row, then sample 1's, ...)."""
        n = self.rowptr[users + 1] - self.rowptr[users]
        return (torch.cumsum(n, 0) - n).contiguous()


def _vae_f32(model, t, what, shape=None):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{model}: {what} must be a contiguous float32 tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{model}: {what} is {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _range_users(staging_bytes, num_item):
    return max(1, staging_bytes // (int(num_item) * 4))


# --------------------------------------------------------------------------------------------
# MultVAE (csrc/multvae.hip): history-row encoder, all-items multinomial likelihood without [B, I]
# --------------------------------------------------------------------------------------------
MULTVAE_LATENT = 64      # p_dims = [64] (Model/MultVAE.py:38): the width the kernels tile


def multvae_tick(state, anneal, cap, total_steps):
    """state[1] = state[0] (the update_count this step reads), state[0] += 1, anneal[0] = min(cap, state[1] / total)."""
    _need_cuda(state, anneal)
    _lib.load().chaorec_multvae_tick(_ptr(state), _ptr(anneal), float(cap), int(total_steps), _stream())


def _multvae_sumsq(tensors, out):
    lib = _lib.load()
    for k, t in enumerate(tensors):
        n_partial = max(1, min(1024, t.numel() // 4096))
        partial = torch.empty(n_partial, dtype=torch.float32, device=t.device)
        lib.chaorec_multvae_sumsq_f32(_ptr(t), t.numel(), _ptr(partial), n_partial, _ptr(out), 1 if k else 0, _stream())


class _MultVAEEncode(torch.autograd.Function):
    """(Wq_t [I, 128], bq [128]) -> z [B, 64], kl [1], sum ||Wq||^2 + ||bq||^2 [1] (Model/MultVAE.py:75-93, :113-114)."""

    @staticmethod
    def forward(ctx, Wq_t, bq, s, batch, state, seed, training, keep_prob, keep, keep_off, eps):
        users, slot_ptr, perm = batch
        _need_cuda(Wq_t, bq, users, s.rowptr, state, keep, keep_off, eps)
        Wq_t, bq = _vae_f32("multvae", Wq_t, "Wq_t"), _vae_f32("multvae", bq, "bq")
        B, dev = users.numel(), Wq_t.device
        if Wq_t.shape != (s.num_item, 2 * MULTVAE_LATENT):
            raise ValueError(f"multvae: Wq_t is {tuple(Wq_t.shape)}, the kernels tile [{s.num_item}, {2 * MULTVAE_LATENT}]")
        if eps is not None:
            eps = _vae_f32("multvae", eps, "eps")
            if eps.shape != (B, MULTVAE_LATENT):
                raise ValueError("multvae: eps must be [B, 64]")
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        h, z, eps_out, klrow, kl, sq = f(B, 2 * MULTVAE_LATENT), f(B, MULTVAE_LATENT), f(B, MULTVAE_LATENT), f(B), f(1), f(1)
        _lib.load().chaorec_multvae_encode_fwd_f32(_ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(Wq_t), _ptr(bq),
                                                   _ptr(keep), _ptr(keep_off), _ptr(eps), _ptr(state), int(seed), int(training),
                                                   float(keep_prob), _ptr(h), _ptr(z), _ptr(eps_out), _ptr(klrow), _ptr(kl),
                                                   _stream())
        _multvae_sumsq((Wq_t, bq), sq)
        ctx.save_for_backward(Wq_t, bq, h, eps_out)
        ctx.s, ctx.batch, ctx.state, ctx.draw = s, batch, state, (int(seed), int(training), float(keep_prob), keep, keep_off)
        ctx.mark_non_differentiable(h, eps_out)
        return z, kl, sq, h, eps_out

    @staticmethod
    def backward(ctx, gz, gkl, gsq, _gh, _ge):
        Wq_t, bq, h, eps = ctx.saved_tensors
        s, (users, slot_ptr, perm) = ctx.s, ctx.batch
        seed, training, keep_prob, keep, keep_off = ctx.draw
        B, dev = users.numel(), Wq_t.device
        n_partial = (B + 63) // 64
        sdh = torch.empty_like(h)
        partial = torch.empty((n_partial, 2 * MULTVAE_LATENT), dtype=torch.float32, device=dev)
        dW, db = torch.empty_like(Wq_t), torch.empty_like(bq)
        _lib.load().chaorec_multvae_encode_bwd_f32(
            _ptr(users), B, s.num_user, _ptr(s.rowptr), s.num_item, _ptr(s.item_ptr), _ptr(s.item_users), _ptr(s.item_pos),
            _ptr(slot_ptr), _ptr(perm), _ptr(Wq_t), _ptr(bq), _ptr(keep), _ptr(keep_off), _ptr(ctx.state), seed, training,
            keep_prob, _ptr(h), _ptr(eps), _ptr(_f32c(gz)), _ptr(_f32c(gkl)), _ptr(_f32c(gsq)), _ptr(sdh), _ptr(partial),
            n_partial, _ptr(dW), _ptr(db), _stream())
        return dW, db, None, None, None, None, None, None, None, None, None


def multvae_encode(Wq_t, bq, s, batch, state, seed, training, keep_prob=0.5, keep=None, keep_off=None, eps=None):
    """-> z [B, 64], kl [1], sum of squares of (Wq_t, bq) [1], h = [mu | logvar] [B, 128], the eps used [B, 64]."""
    return _MultVAEEncode.apply(Wq_t, bq, s, batch, state, seed, bool(training), keep_prob, keep, keep_off, eps)


class _MultVAEDecode(torch.autograd.Function):
    """(z [B, 64], Wp [I, 64], bp [I]) -> neg_ll [1], sum ||Wp||^2 + ||bp||^2 [1], lse [B] (Model/MultVAE.py:98-105,
    :155-156), the logits recomputed tile by tile in the forward and in both backward passes."""

    @staticmethod
    def forward(ctx, z, Wp, bp, s, batch):
        users, slot_ptr, perm = batch
        _need_cuda(z, Wp, bp, users)
        z, Wp, bp = _vae_f32("multvae", z, "z"), _vae_f32("multvae", Wp, "Wp"), _vae_f32("multvae", bp, "bp")
        B, I, dev = users.numel(), s.num_item, z.device
        if Wp.shape != (I, MULTVAE_LATENT) or z.shape != (B, MULTVAE_LATENT) or bp.shape != (I,):
            raise ValueError(f"multvae: decoder shapes z {tuple(z.shape)}, Wp {tuple(Wp.shape)}, bp {tuple(bp.shape)}; "
                             f"the kernels tile a latent width of {MULTVAE_LATENT}")
        lib = _lib.load()
        splits = int(lib.chaorec_multvae_decode_splits(B, I))
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        pm, ps, lse, lse2, cnt, nll, neg_ll, sq = f(splits, B), f(splits, B), f(B), f(2, B), f(B), f(B), f(1), f(1)
        lib.chaorec_multvae_decode_fwd_f32(_ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(z), _ptr(Wp), _ptr(bp),
                                           I, _ptr(pm), _ptr(ps), splits, _ptr(lse), _ptr(lse2), _ptr(cnt), _ptr(nll), _ptr(neg_ll),
                                           _stream())
        _multvae_sumsq((Wp, bp), sq)
        ctx.save_for_backward(z, Wp, bp, lse2, cnt)
        ctx.s, ctx.batch, ctx.splits = s, batch, splits
        ctx.mark_non_differentiable(lse)
        return neg_ll, sq, lse

    @staticmethod
    def backward(ctx, gnll, gsq, _glse):
        z, Wp, bp, lse2, cnt = ctx.saved_tensors
        s, (users, slot_ptr, perm) = ctx.s, ctx.batch
        B, I, dev = users.numel(), s.num_item, z.device
        dzp = torch.empty((ctx.splits, B, MULTVAE_LATENT), dtype=torch.float32, device=dev)
        dz, dW, db = torch.empty_like(z), torch.empty_like(Wp), torch.empty_like(bp)
        _lib.load().chaorec_multvae_decode_bwd_f32(
            _ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(s.item_ptr), _ptr(s.item_users), _ptr(slot_ptr),
            _ptr(perm), _ptr(z), _ptr(Wp), _ptr(bp), I, _ptr(lse2), _ptr(cnt), _ptr(_f32c(gnll)), _ptr(_f32c(gsq)), _ptr(dzp),
            ctx.splits, _ptr(dz), _ptr(dW), _ptr(db), _stream())
        return dz, dW, db, None, None


def multvae_decode(z, Wp, bp, s, batch):
    """-> neg_ll [1], sum of squares of (Wp, bp) [1], lse [B]."""
    return _MultVAEDecode.apply(z, Wp, bp, s, batch)


# --------------------------------------------------------------------------------------------
# MacridVAE (csrc/macridvae.hip): per-concept history-row encoder, mixture likelihood without [B, I] / [B, K, I]
# --------------------------------------------------------------------------------------------
MACRID_D, MACRID_K, MACRID_H = 64, 10, 600      # dim_E, kfac, hidden width the kernels tile (Model/MacridVAE.py:27-28)
MACRID_STAGING_BYTES = 512 << 20                # CHAOREC_MACRID_STAGING_BYTES: one ranking range's [users, I] fp32 scores


def macrid_check_shape(D, K=MACRID_K, H=MACRID_H):
    if (int(D), int(K), int(H)) != (MACRID_D, MACRID_K, MACRID_H):
        raise ValueError(f"MacridVAE: dim_E={D}, kfac={K}, hidden={H}; the kernels tile dim_E={MACRID_D}, kfac={MACRID_K}, "
                         f"hidden={MACRID_H}")


def macrid_tick(state, anneal, cap, total_steps):
    """state[0] += 1, state[1] = state[0], anneal[0] = min(cap, state[0] / total): incremented BEFORE it is read."""
    _need_cuda(state, anneal)
    _lib.load().chaorec_macrid_tick(_ptr(state), _ptr(anneal), float(cap), int(total_steps), _stream())


def macrid_normal(shape, state, seed, std, device):
    """std * N(0, 1) of `shape` from the counter RNG (seed, state[1], element)."""
    _need_cuda(state)
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _lib.load().chaorec_macrid_normal_f32(_ptr(out), out.numel(), _ptr(state), int(seed), float(std), _stream())
    return out


class _MacridConcept(torch.autograd.Function):
    """(item_embedding [I, D], k_embedding [K, D]) -> items [I, D], cates [I, K] (Model/MacridVAE.py:76-77, :86-94)."""

    @staticmethod
    def forward(ctx, E, Kemb, tau, gumbel, state, seed, training):
        _need_cuda(E, Kemb, gumbel, state)
        E, Kemb = _vae_f32("macrid", E, "item_embedding"), _vae_f32("macrid", Kemb, "k_embedding")
        I, D = E.shape
        K = Kemb.shape[0]
        macrid_check_shape(D, K)
        if gumbel is not None:
            gumbel = _vae_f32("macrid", gumbel, "gumbel")
            if gumbel.shape != (I, K):
                raise ValueError("macrid: gumbel must be [I, K]")
        items, cates = torch.empty_like(E), torch.empty((I, K), dtype=torch.float32, device=E.device)
        _lib.load().chaorec_macrid_concept_fwd_f32(_ptr(E), _ptr(Kemb), I, D, K, float(tau), _ptr(gumbel), _ptr(state), int(seed),
                                                   int(training), _ptr(items), _ptr(cates), _stream())
        ctx.save_for_backward(E, Kemb, cates)
        ctx.tau = float(tau)
        return items, cates

    @staticmethod
    def backward(ctx, d_items, d_cates):
        E, Kemb, cates = ctx.saved_tensors
        I, D = E.shape
        K = Kemb.shape[0]
        n_partial = (I + 63) // 64
        partial = torch.empty((n_partial, K, D), dtype=torch.float32, device=E.device)
        dE, dK = torch.empty_like(E), torch.empty_like(Kemb)
        _lib.load().chaorec_macrid_concept_bwd_f32(_ptr(E), _ptr(Kemb), I, D, K, ctx.tau, _ptr(cates), _ptr(_f32c(d_items)),
                                                   _ptr(_f32c(d_cates)), _ptr(partial), n_partial, _ptr(dE), _ptr(dK), _stream())
        return dE, dK, None, None, None, None, None


def macrid_concept(E, Kemb, tau, state, seed, training, gumbel=None):
    """-> items = normalize(E) [I, D], cates = softmax(items . normalize(Kemb)^T / tau (+ Gumbel noise in training)) [I, K]."""
    return _MacridConcept.apply(E, Kemb, tau, gumbel, state, seed, bool(training))


class _MacridEncode(torch.autograd.Function):
    """(W1_t [I, 600], b1 [600], cates [I, K]) -> a [B, K, 600] (Model/MacridVAE.py:82-83, :101-105 up to the first Linear)."""

    @staticmethod
    def forward(ctx, W1_t, b1, cates, s, batch, state, seed, training, keep_prob, keep, keep_off):
        users, slot_ptr, perm = batch
        _need_cuda(W1_t, b1, cates, users, s.rowptr, state, keep, keep_off)
        W1_t, b1, cates = _vae_f32("macrid", W1_t, "W1_t"), _vae_f32("macrid", b1, "b1"), _vae_f32("macrid", cates, "cates")
        B, dev, K, H = users.numel(), W1_t.device, cates.shape[1], W1_t.shape[1]
        macrid_check_shape(MACRID_D, K, H)
        if W1_t.shape[0] != s.num_item or cates.shape[0] != s.num_item:
            raise ValueError(f"macrid: W1_t {tuple(W1_t.shape)}, cates {tuple(cates.shape)} for {s.num_item} items")
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
        a = torch.empty((B, K, H), dtype=torch.float32, device=dev)
        srow = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.load().chaorec_macrid_encode_fwd_f32(_ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(W1_t), _ptr(b1),
                                                  _ptr(cates), K, H, _ptr(keep), _ptr(keep_off), _ptr(state), int(seed), int(training),
                                                  float(keep_prob), _ptr(a), _ptr(srow), _stream())
        ctx.save_for_backward(W1_t, cates, srow)
        ctx.s, ctx.batch, ctx.state, ctx.draw = s, batch, state, (int(seed), int(training), float(keep_prob), keep, keep_off)
        return a

    @staticmethod
    def backward(ctx, da):
        W1_t, cates, srow = ctx.saved_tensors
        s, (users, slot_ptr, perm) = ctx.s, ctx.batch
        seed, training, keep_prob, keep, keep_off = ctx.draw
        B, dev, K, H = users.numel(), W1_t.device, cates.shape[1], W1_t.shape[1]
        n_partial = (B * K + 63) // 64
        partial = torch.empty((n_partial, H), dtype=torch.float32, device=dev)
        dW, db, dc = torch.empty_like(W1_t), torch.empty(H, dtype=torch.float32, device=dev), torch.empty_like(cates)
        _lib.load().chaorec_macrid_encode_bwd_f32(
            B, s.num_item, _ptr(s.item_ptr), _ptr(s.item_users), _ptr(s.item_pos), _ptr(slot_ptr), _ptr(perm), _ptr(W1_t), _ptr(cates),
            K, H, _ptr(keep), _ptr(keep_off), _ptr(ctx.state), seed, training, keep_prob, _ptr(srow), _ptr(_f32c(da)), _ptr(partial),
            n_partial, _ptr(dW), _ptr(db), _ptr(dc), _stream())
        return dW, db, dc, None, None, None, None, None, None, None, None


def macrid_encode(W1_t, b1, cates, s, batch, state, seed, training, keep_prob=0.5, keep=None, keep_off=None):
    """-> a [B, K, 600]: b1 + s_b sum over the kept history entries of cates[i, k] W1_t[i, :]."""
    return _MacridEncode.apply(W1_t, b1, cates, s, batch, state, seed, bool(training), keep_prob, keep, keep_off)


class _MacridSplit(torch.autograd.Function):
    """h [n, 2 D] -> (h[:, :D], h[:, D:]) as contiguous tensors; the backward is one concatenation."""

    @staticmethod
    def forward(ctx, h):
        D = h.shape[1] // 2
        return h[:, :D].contiguous(), h[:, D:].contiguous()

    @staticmethod
    def backward(ctx, g1, g2):
        return torch.cat((g1, g2), 1)


def macrid_split(h):
    return _MacridSplit.apply(h)


class _MacridMix(torch.autograd.Function):
    """(zh [B, K, D], items [I, D], cates [I, K]) -> ce [1], lse [B] (Model/MacridVAE.py:119-126, :150): the logits
    recomputed tile by tile in the forward and in both backward passes."""

    @staticmethod
    def forward(ctx, zh, items, cates, s, batch, tau):
        users, slot_ptr, perm = batch
        _need_cuda(zh, items, cates, users)
        zh, items, cates = _vae_f32("macrid", zh, "zh"), _vae_f32("macrid", items, "items"), _vae_f32("macrid", cates, "cates")
        B, I, dev = users.numel(), s.num_item, zh.device
        K, D = cates.shape[1], items.shape[1]
        macrid_check_shape(D, K)
        if zh.shape != (B, K, D) or items.shape[0] != I or cates.shape[0] != I:
            raise ValueError(f"macrid: zh {tuple(zh.shape)}, items {tuple(items.shape)}, cates {tuple(cates.shape)}")
        lib = _lib.load()
        splits = int(lib.chaorec_macrid_mix_splits(B, I))
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        ps, lse, coef, nll, ce = f(splits, K, B), f(B), f(B), f(B), f(1)
        lib.chaorec_macrid_mix_fwd_f32(_ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(zh), _ptr(items), _ptr(cates),
                                       I, D, K, float(tau), _ptr(ps), splits, _ptr(lse), _ptr(coef), _ptr(nll), _ptr(ce), _stream())
        ctx.save_for_backward(zh, items, cates, coef)
        ctx.s, ctx.batch, ctx.splits, ctx.tau = s, batch, splits, float(tau)
        ctx.mark_non_differentiable(lse)
        return ce, lse

    @staticmethod
    def backward(ctx, gce, _glse):
        zh, items, cates, coef = ctx.saved_tensors
        s, (users, slot_ptr, perm) = ctx.s, ctx.batch
        B, I, dev = users.numel(), s.num_item, zh.device
        K, D = cates.shape[1], items.shape[1]
        dzp = torch.empty((ctx.splits, B, K, D), dtype=torch.float32, device=dev)
        dz, di, dc = torch.empty_like(zh), torch.empty_like(items), torch.empty_like(cates)
        _lib.load().chaorec_macrid_mix_bwd_f32(
            _ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(s.item_ptr), _ptr(s.item_users), _ptr(slot_ptr), _ptr(perm),
            _ptr(zh), _ptr(items), _ptr(cates), I, D, K, ctx.tau, _ptr(coef), _ptr(_f32c(gce)), _ptr(dzp), ctx.splits, _ptr(dz),
            _ptr(di), _ptr(dc), _stream())
        return dz, di, dc, None, None, None


def macrid_mix(zh, items, cates, s, batch, tau):
    """-> ce [1] = mean_b (n_b log sum_i p_bi - sum_{i in hist} log p_bi), lse [B]."""
    return _MacridMix.apply(zh, items, cates, s, batch, tau)


def macrid_range_users(num_item):
    """How many users one ranking range may stage under the cap."""
    return _range_users(MACRID_STAGING_BYTES, num_item)


def macrid_scores(zh, items, cates, tau, user_begin, hist, mask_value, out=None):
    """log p_ui of the users user_begin .. user_begin + n (zh [n, K, D]) -> [n, I] fp32, their history entries = mask_value."""
    _need_cuda(zh, items, cates, hist[0], hist[1])
    zh, items, cates = _vae_f32("macrid", zh, "zh"), _vae_f32("macrid", items, "items"), _vae_f32("macrid", cates, "cates")
    n, K, D = zh.shape
    I = items.shape[0]
    macrid_check_shape(D, K)
    if n > macrid_range_users(I):
        raise ValueError(f"macrid: {n} users x {I} items exceed the staging cap of {MACRID_STAGING_BYTES} bytes; rank in ranges")
    if hist[0].dtype != torch.int64 or hist[1].dtype != torch.int64:
        raise ValueError("macrid: the history CSR must be int64")
    if out is None:
        out = torch.empty((n, I), dtype=torch.float32, device=zh.device)
    _lib.load().chaorec_macrid_scores_f32(_ptr(zh), n, _ptr(items), _ptr(cates), I, D, K, float(tau), int(user_begin), _ptr(hist[0]),
                                          _ptr(hist[1]), float(mask_value), _ptr(out), out.numel() * 4, _stream())
    return out


def macrid_topk(scores, topk, id_offset=0):
    """Exact top-k per row of scores [n, I], ties to the lowest index -> (int64 [n, topk] ids + id_offset, fp32 [n, topk])."""
    _need_cuda(scores)
    scores = _vae_f32("macrid", scores, "scores")
    n, I = scores.shape
    if not 1 <= int(topk) <= min(64, I):
        raise ValueError(f"macrid: topk={topk} (1 .. min(64, I={I}))")
    idx = torch.empty((n, int(topk)), dtype=torch.int64, device=scores.device)
    val = torch.empty((n, int(topk)), dtype=torch.float32, device=scores.device)
    _lib.load().chaorec_macrid_topk_f32(_ptr(scores), n, I, int(topk), int(id_offset), _ptr(idx), _ptr(val), _stream())
    return idx, val


# --------------------------------------------------------------------------------------------
# DualVAE (csrc/dualvae.hip): two-sided aspect encoder, Poisson likelihood and neighbourhood term without [B, U] / [B, I]
# --------------------------------------------------------------------------------------------
DUALVAE_K, DUALVAE_A, DUALVAE_H = 25, 5, 20     # latent width, aspects, hidden width the kernels tile (Model/DualVAE.py:37-49)
DUALVAE_STAGING_BYTES = 512 << 20               # CHAOREC_DUALVAE_STAGING_BYTES: one ranking range's [users, I] fp32 scores


def dualvae_check_shape(k, a=DUALVAE_A, hidden=DUALVAE_H):
    if (int(k), int(a), int(hidden)) != (DUALVAE_K, DUALVAE_A, DUALVAE_H):
        raise ValueError(f"DualVAE: k={k}, a={a}, hidden={hidden}; the kernels tile k={DUALVAE_K}, a={DUALVAE_A}, "
                         f"hidden={DUALVAE_H}")


def step_tick(state, export="chaorec_adagcl_tick"):
    """state int64 [2] on the device: [0] += 1, [1] = [0] -- the step the device draws of the launches after it are keyed
    by.  One kernel (csrc/draws.h) behind three exports, one per library file that launches it; a model without an export
    of its own (GraphAug) calls this with the default."""
    _need_cuda(state)
    getattr(_lib.load(), export)(_ptr(state), _stream())


def dualvae_tick(state):
    step_tick(state, "chaorec_dualvae_tick")


class _DualVAEEncode(torch.autograd.Function):
    """(We_t [N, 20], bias [20], w [N, 5]) -> pre [B, 5, 20] = bias + sum over the sample's row of w[n, a] We_t[n, :]."""

    @staticmethod
    def forward(ctx, We_t, bias, w, s, batch):
        ids, slot_ptr, perm = batch
        _need_cuda(We_t, bias, w, ids, s.rowptr)
        N = s.num_item
        We_t, bias = _vae_f32("dualvae", We_t, "We_t", (N, DUALVAE_H)), _vae_f32("dualvae", bias, "bias", (DUALVAE_H,))
        w = _vae_f32("dualvae", w, "w", (N, DUALVAE_A))
        B = ids.numel()
        pre = torch.empty((B, DUALVAE_A, DUALVAE_H), dtype=torch.float32, device=We_t.device)
        _lib.load().chaorec_dualvae_encode_fwd_f32(_ptr(ids), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), N, _ptr(We_t), _ptr(bias),
                                                   _ptr(w), _ptr(pre), _stream())
        ctx.save_for_backward(We_t, w)
        ctx.s, ctx.batch = s, batch
        return pre

    @staticmethod
    def backward(ctx, dpre):
        We_t, w = ctx.saved_tensors
        s, (ids, slot_ptr, perm) = ctx.s, ctx.batch
        B, N = ids.numel(), s.num_item
        dpre = _f32c(dpre)
        dW, dw = torch.empty_like(We_t), torch.empty_like(w)
        _lib.load().chaorec_dualvae_encode_bwd_f32(B, N, _ptr(s.item_ptr), _ptr(s.item_users), _ptr(slot_ptr), _ptr(perm), _ptr(We_t),
                                                   _ptr(w), _ptr(dpre), _ptr(dW), _ptr(dw), _stream())
        db = col_sum(dpre.view(B * DUALVAE_A, DUALVAE_H))      # (a fixed-order sum over the B * 5 rows)
        return dW, db, dw, None, None


def dualvae_encode(We_t, bias, w, s, batch):
    """-> pre [B, 5, 20]; s: the MultVAEStructure of the SAMPLE side (rows = samples, columns = table rows)."""
    return _DualVAEEncode.apply(We_t, bias, w, s, batch)


class _DualVAEDense(torch.autograd.Function):
    """(z [B, 5, 25], zh [B, 5, 20], th [N, 5, 20], w [N, 5]; table [N, 5, 25] without gradient) -> sum_p [B], xlog [B],
    nei [B, 5, 25]: the tiles s_bna recomputed in the forward and in both backward passes."""

    @staticmethod
    def forward(ctx, z, zh, th, w, table, s, batch):
        ids, slot_ptr, perm = batch
        _need_cuda(z, zh, th, w, table, ids)
        B, N, dev = ids.numel(), s.num_item, z.device
        z, zh = _vae_f32("dualvae", z, "z", (B, DUALVAE_A, DUALVAE_K)), _vae_f32("dualvae", zh, "zh", (B, DUALVAE_A, DUALVAE_H))
        th, w = _vae_f32("dualvae", th, "th", (N, DUALVAE_A, DUALVAE_H)), _vae_f32("dualvae", w, "w", (N, DUALVAE_A))
        table = _vae_f32("dualvae", table, "table", (N, DUALVAE_A, DUALVAE_K))
        lib = _lib.load()
        splits = int(lib.chaorec_dualvae_splits(B, N))
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        psum, pnei = f(splits, DUALVAE_A, B), f(splits, B, DUALVAE_A, DUALVAE_K)
        sum_p, xlog, nei = f(B), f(B), f(B, DUALVAE_A, DUALVAE_K)
        lib.chaorec_dualvae_dense_fwd_f32(_ptr(ids), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(z), _ptr(zh), _ptr(table), _ptr(th),
                                          _ptr(w), N, _ptr(psum), _ptr(pnei), splits, _ptr(sum_p), _ptr(xlog), _ptr(nei), _stream())
        ctx.save_for_backward(z, zh, th, w, table)
        ctx.s, ctx.batch, ctx.splits = s, batch, splits
        return sum_p, xlog, nei

    @staticmethod
    def backward(ctx, g1, g2, gN):
        z, zh, th, w, table = ctx.saved_tensors
        s, (ids, slot_ptr, perm) = ctx.s, ctx.batch
        B, N, dev = ids.numel(), s.num_item, z.device
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        dzp, dzhp = f(ctx.splits, B, DUALVAE_A, DUALVAE_K), f(ctx.splits, B, DUALVAE_A, DUALVAE_H)
        dz, dzh, dth, dw = torch.empty_like(z), torch.empty_like(zh), torch.empty_like(th), torch.empty_like(w)
        _lib.load().chaorec_dualvae_dense_bwd_f32(
            _ptr(ids), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(s.item_ptr), _ptr(s.item_users), _ptr(slot_ptr), _ptr(perm),
            _ptr(z), _ptr(zh), _ptr(table), _ptr(th), _ptr(w), N, _ptr(_f32c(g1)), _ptr(_f32c(g2)), _ptr(_f32c(gN)), _ptr(dzp),
            _ptr(dzhp), ctx.splits, _ptr(dz), _ptr(dzh), _ptr(dth), _ptr(dw), _stream())
        return dz, dzh, dth, dw, None, None, None


def dualvae_dense(z, zh, th, w, table, s, batch):
    """-> sum_p [B] = sum_n p_bn, xlog [B] = sum_{n in row(b)} log(p_bn + 1e-10), nei [B, 5, 25].  `table` must stay as it
    is until the backward has run (the caller passes a snapshot where the table is written in between)."""
    return _DualVAEDense.apply(z, zh, th, w, table, s, batch)


def dualvae_writeback(batch, num_rows, z, mu, table, mu_table):
    """table[ids] = z, mu_table[ids] = mu in place; where an id repeats in the batch the highest position wins."""
    ids, slot_ptr, perm = batch
    _need_cuda(ids, z, mu, table, mu_table)
    B = ids.numel()
    z, mu = _vae_f32("dualvae", z, "z", (B, DUALVAE_A, DUALVAE_K)), _vae_f32("dualvae", mu, "mu", (B, DUALVAE_A, DUALVAE_K))
    _vae_f32("dualvae", table, "table", (num_rows, DUALVAE_A, DUALVAE_K))
    _vae_f32("dualvae", mu_table, "mu_table", (num_rows, DUALVAE_A, DUALVAE_K))
    _lib.load().chaorec_dualvae_writeback_f32(_ptr(ids), B, int(num_rows), _ptr(slot_ptr), _ptr(perm), _ptr(z), _ptr(mu), _ptr(table),
                                              _ptr(mu_table), _stream())


def dualvae_range_users(num_item):
    """How many users one ranking range may stage under the cap."""
    return _range_users(DUALVAE_STAGING_BYTES, num_item)


def dualvae_scores(z, zh, table, th, w, user_begin, hist, mask_value, out=None):
    """sum_a w[i, a] sigmoid(z_ua . table_ia + tanh(zh_ua . th_ia)) of the users user_begin .. user_begin + n -> [n, I] fp32,
    their history entries = mask_value."""
    _need_cuda(z, zh, table, th, w, hist[0], hist[1])
    n, I = z.shape[0], table.shape[0]
    z, zh = _vae_f32("dualvae", z, "z", (n, DUALVAE_A, DUALVAE_K)), _vae_f32("dualvae", zh, "zh", (n, DUALVAE_A, DUALVAE_H))
    table, th = _vae_f32("dualvae", table, "table", (I, DUALVAE_A, DUALVAE_K)), _vae_f32("dualvae", th, "th", (I, DUALVAE_A, DUALVAE_H))
    w = _vae_f32("dualvae", w, "w", (I, DUALVAE_A))
    if n > dualvae_range_users(I):
        raise ValueError(f"dualvae: {n} users x {I} items exceed the staging cap of {DUALVAE_STAGING_BYTES} bytes; rank in ranges")
    if hist[0].dtype != torch.int64 or hist[1].dtype != torch.int64:
        raise ValueError("dualvae: the history CSR must be int64")
    if out is None:
        out = torch.empty((n, I), dtype=torch.float32, device=z.device)
    _lib.load().chaorec_dualvae_scores_f32(_ptr(z), _ptr(zh), n, _ptr(table), _ptr(th), _ptr(w), I, int(user_begin), _ptr(hist[0]),
                                           _ptr(hist[1]), float(mask_value), _ptr(out), out.numel() * 4, _stream())
    return out


class _DualVAELinear(torch.autograd.Function):
    """y = x W^T + b for the small Linears (W [M, N], M <= 32, N <= 31): the forward and the input gradient are the f32
    GEMM's, the weight and bias gradients are summed in double over the rows and rounded once."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_cuda(x, weight, bias)
        x = _f32c(x)
        y = gemm_raw(x, weight, transB=True, bias=bias)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = _f32c(gy)
        R, (M, N) = x.shape[0], weight.shape
        lib = _lib.load()
        nbytes = lib.chaorec_dualvae_linear_bwd_workspace_bytes(R, M)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        gw, gb = torch.empty_like(weight), torch.empty(M, dtype=torch.float32, device=x.device)
        lib.chaorec_dualvae_linear_bwd_f32(_ptr(gy), _ptr(x), R, M, N, _ptr(gw), _ptr(gb), _ptr(ws), nbytes, _stream())
        gx = gemm_raw(gy, weight) if ctx.needs_input_grad[0] else None
        return gx, gw, gb


def dualvae_linear(x, weight, bias):
    """nn.Linear for x [R, N] and a small weight [M, N] (see _DualVAELinear)."""
    return _DualVAELinear.apply(x, weight.contiguous(), bias)


class _DualVAELoss(torch.autograd.Function):
    """(mu, std_pre [B * 5, 25], xlog [B], sum_p [B], cl []) -> [3] = (kl_weight kl - ll + ssl_reg cl, kl, ll) from double sums,
    each rounded once; std = sigmoid(std_pre), the KL's elements are evaluated in double.  The gradient of element 0 only."""

    @staticmethod
    def forward(ctx, mu, std_pre, xlog, sum_p, cl, kl_weight, ssl_reg):
        _need_cuda(mu, std_pre, xlog, sum_p, cl)
        mu, std_pre, xlog, sum_p, cl = _f32c(mu), _f32c(std_pre), _f32c(xlog), _f32c(sum_p), _f32c(cl)
        B = xlog.numel()
        if mu.shape != std_pre.shape or mu.numel() != B * DUALVAE_A * DUALVAE_K or sum_p.numel() != B:
            raise ValueError(f"dualvae: mu {tuple(mu.shape)}, std_pre {tuple(std_pre.shape)} for {B} samples")
        out = torch.empty(3, dtype=torch.float32, device=xlog.device)
        ws = torch.empty(64, dtype=torch.float64, device=xlog.device)
        _lib.load().chaorec_dualvae_loss_f32(_ptr(mu), _ptr(std_pre), mu.numel(), _ptr(xlog), _ptr(sum_p), B, _ptr(cl), float(kl_weight),
                                             float(ssl_reg), _ptr(out), _ptr(ws), ws.numel() * 8, _stream())
        ctx.save_for_backward(mu, std_pre)
        ctx.B, ctx.c = B, (float(kl_weight), float(ssl_reg))
        return out

    @staticmethod
    def backward(ctx, g):
        mu, std_pre = ctx.saved_tensors
        g0 = g[0]
        gB = (g0 / ctx.B).expand(ctx.B)
        gk = g0 * (ctx.c[0] / (DUALVAE_A * ctx.B))
        std = torch.sigmoid(std_pre)
        # d/d mu = mu;  d/d std_pre of -0.5 (2 log std - std^2) = -(1 - std)(1 - std^2)
        return gk * mu, gk * ((std - 1.0) * (1.0 - std * std)), -gB, gB, g0 * ctx.c[1], None, None


def dualvae_loss(mu, std_pre, xlog, sum_p, cl, kl_weight, ssl_reg):
    """-> [3]: one side's loss (Model/DualVAE.py:274), kl and ll."""
    return _DualVAELoss.apply(mu, std_pre, xlog, sum_p, cl, kl_weight, ssl_reg)


# --------------------------------------------------------------------------------------------
# The user-user co-occurrence graph (csrc/usergraph.hip): DRAGON's user_graph_dict built, sampled and aggregated on the device;
# DualGNN's fused node over the same structure; COHESION's over three tables, with a chunked backward
# --------------------------------------------------------------------------------------------
USERGRAPH_TOPN = 200         # dualgnn-gen-u-u-matrix.py:92-103 keeps the 200 largest co-occurrence counts of a user
USERGRAPH_MAX_N = 256        # what the build kernel's sorting network holds
USERGRAPH_DIMS = (64, 128)   # the row widths the aggregation kernels are instantiated for


def usergraph_max_users():
    """The largest user count the usergraph entries accept (ids are 32-bit)."""
    return int(_lib.load().chaorec_usergraph_max_users())


def usergraph_tile_users(num_user, tile_users=0):
    """How many user ids one LDS tile of the build covers."""
    return int(_lib.load().chaorec_usergraph_tile_users(int(num_user), int(tile_users)))


def _ug_i32(t, what, shape=None):
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError(f"usergraph: {what} must be a contiguous int32 tensor")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"usergraph: {what} is {tuple(t.shape)}, expected {tuple(shape)}")
    return t


class UserGraphStructure:
    """nbr_idx / nbr_cnt int32 [U, N], nbr_len int32 [U] (each user's co-occurring users by count descending, id ascending)
    and, once usergraph_sample() has run, the epoch's buffers: epoch_idx int32 [U, k], epoch_w fp32 [U, k] and the reverse
    structure of the aggregation's backward (rev_ptr int64 [U + 1]; rev_slot int64, rev_u int32, rev_w fp32 [U k]: for every
    user r the slots u k + j that name r, ascending).  The epoch buffers are allocated once per k and rewritten in place
    by every later sample, so a captured step that holds their addresses reads the new epoch's graph at its next replay."""

    def __init__(self, nbr_idx, nbr_cnt, nbr_len):
        U, N = nbr_idx.shape
        self.num_user, self.n = int(U), int(N)
        self.nbr_idx, self.nbr_cnt = _ug_i32(nbr_idx, "nbr_idx"), _ug_i32(nbr_cnt, "nbr_cnt", (U, N))
        self.nbr_len = _ug_i32(nbr_len, "nbr_len", (U,))
        self.k = 0
        self.epoch_idx = self.epoch_w = self.rev_ptr = self.rev_slot = self.rev_u = self.rev_w = self._ids = None
        self.rev_chunks = {}      # chunk -> usergraph_rev_chunks() of the current epoch graph (COHESION's backward)

    @classmethod
    def from_dict(cls, user_graph_dict, num_user, n=USERGRAPH_TOPN, device="cpu"):
        """The reference's user_graph_dict.npy ({user: [[ids], [counts]]}, Model/DRAGON.py:170) in the arrays' form."""
        import numpy as np
        idx, cnt = np.zeros((num_user, n), dtype=np.int32), np.zeros((num_user, n), dtype=np.int32)
        length = np.zeros(num_user, dtype=np.int32)
        for u in range(num_user):
            ids, counts = user_graph_dict[u]
            m = min(len(ids), n)
            idx[u, :m], cnt[u, :m], length[u] = ids[:m], np.asarray(counts[:m]).astype(np.int32), m
        return cls(torch.from_numpy(idx).to(device), torch.from_numpy(cnt).to(device), torch.from_numpy(length).to(device))

    def to(self, device):
        for name in ("nbr_idx", "nbr_cnt", "nbr_len", "epoch_idx", "epoch_w", "rev_ptr", "rev_slot", "rev_u", "rev_w", "_ids"):
            if getattr(self, name) is not None:
                setattr(self, name, getattr(self, name).to(device))
        self.rev_chunks = {}
        return self

    def _epoch_buffers(self, k):
        if self.k != k:
            U, dev = self.num_user, self.nbr_idx.device
            self.k = int(k)
            self.epoch_idx = torch.zeros((U, k), dtype=torch.int32, device=dev)
            self.epoch_w = torch.zeros((U, k), dtype=torch.float32, device=dev)
            self.rev_ptr = torch.zeros(U + 1, dtype=torch.int64, device=dev)
            self.rev_slot = torch.zeros(U * k, dtype=torch.int64, device=dev)
            self.rev_u = torch.zeros(U * k, dtype=torch.int32, device=dev)
            self.rev_w = torch.zeros(U * k, dtype=torch.float32, device=dev)
            self._ids = torch.arange(U + 1, dtype=torch.int64, device=dev)

    def set_epoch(self, epoch_idx, epoch_w):
        """Install a GIVEN epoch graph ([U, k] ids and weights, e.g. the reference's own draw) and index it for the backward."""
        U, k = epoch_idx.shape
        if U != self.num_user or tuple(epoch_w.shape) != (U, k):
            raise ValueError(f"usergraph: epoch graph {tuple(epoch_idx.shape)} / {tuple(epoch_w.shape)} for {self.num_user} users")
        self._epoch_buffers(int(k))
        self.epoch_idx.copy_(epoch_idx)
        self.epoch_w.copy_(epoch_w)
        self.index_epoch()
        self.rev_chunks = {}

    def index_epoch(self):
        """The reverse structure of the current epoch_idx: torch's STABLE sort of the flattened slots by the user they name
        (so a user's slots stay in ascending (u, j)), written into the buffers allocated with the epoch graph."""
        flat = self.epoch_idx.view(-1).to(torch.int64)
        named, perm = torch.sort(flat, stable=True)
        self.rev_slot.copy_(perm)
        self.rev_u.copy_(torch.div(perm, self.k, rounding_mode="floor"))
        self.rev_w.copy_(self.epoch_w.view(-1)[perm])
        self.rev_ptr.copy_(torch.searchsorted(named, self._ids))


def usergraph_build(rowptr, col, num_item, n=USERGRAPH_TOPN, tile_users=0, out=None):
    """The co-occurrence graph of the user-history CSR (rowptr int64 [U + 1], col int32 local item ids without repeats, on
    the device) -> UserGraphStructure with N = n neighbours per user.  `out` = (nbr_idx, nbr_cnt, nbr_len) to fill."""
    _need_cuda(rowptr, col)
    if rowptr.dtype != torch.int64 or not rowptr.is_contiguous() or rowptr.dim() != 1:
        raise ValueError("usergraph: rowptr must be a contiguous int64 vector")
    col = _ug_i32(col, "col")
    U, I, dev = int(rowptr.numel() - 1), int(num_item), rowptr.device
    if not 1 <= int(n) <= USERGRAPH_MAX_N:
        raise ValueError(f"usergraph: n = {n}, the build keeps 1 .. {USERGRAPH_MAX_N} neighbours")
    if U < 1 or U > usergraph_max_users() or I < 1:
        raise ValueError(f"usergraph: {U} users, {I} items (at most {usergraph_max_users()} users)")
    # the item-major transpose (item -> ascending holders): a stable sort of the entries by item
    counts = rowptr[1:] - rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(U, dtype=torch.int32, device=dev), counts)
    col64 = col.to(torch.int64)
    item_users = rows[torch.sort(col64, stable=True)[1]].contiguous()
    item_ptr = torch.zeros(I + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(col64, minlength=I)[:I], 0, out=item_ptr[1:])
    if out is None:
        out = (torch.empty((U, n), dtype=torch.int32, device=dev), torch.empty((U, n), dtype=torch.int32, device=dev),
               torch.empty(U, dtype=torch.int32, device=dev))
    nbr_idx, nbr_cnt, nbr_len = _ug_i32(out[0], "nbr_idx", (U, n)), _ug_i32(out[1], "nbr_cnt", (U, n)), _ug_i32(out[2], "nbr_len", (U,))
    _need_cuda(nbr_idx, nbr_cnt, nbr_len)
    _lib.load().chaorec_usergraph_build(_ptr(rowptr), _ptr(col), _ptr(item_ptr), _ptr(item_users), U, I, int(n), int(tile_users),
                                        _ptr(nbr_idx), _ptr(nbr_cnt), _ptr(nbr_len), _stream())
    return UserGraphStructure(nbr_idx, nbr_cnt, nbr_len)


def usergraph_sample(s, k, seed, epoch):
    """Model/DRAGON.py:231-270 on the device: fills s.epoch_idx / s.epoch_w [U, k] for (seed, epoch) and re-indexes them."""
    _need_cuda(s.nbr_idx, s.nbr_cnt, s.nbr_len)
    if not 1 <= int(k) <= s.n:
        raise ValueError(f"usergraph: k = {k}, the structure holds {s.n} neighbours per user")
    s._epoch_buffers(int(k))
    _lib.load().chaorec_usergraph_sample(_ptr(s.nbr_idx), _ptr(s.nbr_cnt), _ptr(s.nbr_len), s.num_user, s.n, int(k),
                                         int(seed) & (2**64 - 1), int(epoch) & (2**64 - 1), _ptr(s.epoch_idx), _ptr(s.epoch_w),
                                         _stream())
    s.index_epoch()
    s.rev_chunks = {}
    return s.epoch_idx, s.epoch_w


class _UserGraphAggregate(torch.autograd.Function):
    """(v [U, D], t [U, D], weight_u [U, 2(, 1)]) -> [U, 2 D] (Model/DRAGON.py:289-302): neither user_rep, nor
    features[user_graph] [U, k, 2 D], nor h_u exists in memory, forward or backward."""

    @staticmethod
    def forward(ctx, v, t, weight_u, s):
        _need_cuda(v, t, weight_u, s.epoch_idx)
        if v.dim() != 2 or v.shape[1] not in USERGRAPH_DIMS:
            raise ValueError(f"usergraph: v is {tuple(v.shape)}, the aggregation is built for D in {USERGRAPH_DIMS}")
        U, D = s.num_user, int(v.shape[1])
        v, t = _vae_f32("usergraph", v, "v", (U, D)), _vae_f32("usergraph", t, "t", (U, D))
        weight_u = _vae_f32("usergraph", weight_u, "weight_u")
        if weight_u.numel() != 2 * U or weight_u.shape[0] != U:
            raise ValueError(f"usergraph: weight_u is {tuple(weight_u.shape)}, expected ({U}, 2)")
        if s.k < 1:
            raise ValueError("usergraph: no epoch graph yet (usergraph_sample / set_epoch)")
        out = torch.empty((U, 2 * D), dtype=torch.float32, device=v.device)
        _lib.load().chaorec_usergraph_aggregate_fwd_f32(_ptr(v), _ptr(t), _ptr(weight_u), _ptr(s.epoch_idx), _ptr(s.epoch_w), U, s.k, D,
                                                        _ptr(out), _stream())
        ctx.save_for_backward(v, t, weight_u)
        ctx.s = s
        return out

    @staticmethod
    def backward(ctx, g):
        v, t, weight_u = ctx.saved_tensors
        s, (U, D) = ctx.s, v.shape
        g = _f32c(g)
        dv, dt, dw = torch.empty_like(v), torch.empty_like(t), torch.empty_like(weight_u)
        _lib.load().chaorec_usergraph_aggregate_bwd_f32(_ptr(g), _ptr(v), _ptr(t), _ptr(weight_u), _ptr(s.rev_ptr), _ptr(s.rev_u),
                                                        _ptr(s.rev_w), U, D, _ptr(dv), _ptr(dt), _ptr(dw), _stream())
        return dv, dt, dw, None


def usergraph_aggregate(v, t, weight_u, s):
    """out[u] = x[u] + sum_j s.epoch_w[u, j] x[s.epoch_idx[u, j]], x[r] = (weight_u[r, 0] v[r], weight_u[r, 1] t[r])."""
    return _UserGraphAggregate.apply(v, t, weight_u, s)


class _DualGNNFuse(torch.autograd.Function):
    """(v [N, D], t [N, D], weight_u [U, 2(, 1)]) -> result [N, D] (Model/DualGNN.py:189-239): none of user_rep,
    features[user_graph] [U, k, D], h_u1 or representation exists in memory, forward or backward."""

    @staticmethod
    def forward(ctx, v, t, weight_u, s, num_user):
        _need_cuda(v, t, weight_u, s.epoch_idx)
        if v.dim() != 2 or v.shape[1] not in USERGRAPH_DIMS:
            raise ValueError(f"dualgnn_fuse: v is {tuple(v.shape)}, the kernels are built for D in {USERGRAPH_DIMS}")
        U, (N, D) = int(num_user), (int(v.shape[0]), int(v.shape[1]))
        if U != s.num_user or N < U:
            raise ValueError(f"dualgnn_fuse: {U} users, a table of {N} rows, a user graph of {s.num_user} users")
        v, t = _vae_f32("dualgnn_fuse", v, "v", (N, D)), _vae_f32("dualgnn_fuse", t, "t", (N, D))
        weight_u = _vae_f32("dualgnn_fuse", weight_u, "weight_u")
        if tuple(weight_u.shape) not in ((U, 2), (U, 2, 1)):
            raise ValueError(f"dualgnn_fuse: weight_u is {tuple(weight_u.shape)}, expected ({U}, 2) or ({U}, 2, 1)")
        if s.k < 1:
            raise ValueError("dualgnn_fuse: no epoch graph yet (usergraph_sample / set_epoch)")
        out = torch.empty((N, D), dtype=torch.float32, device=v.device)
        _lib.load().chaorec_dualgnn_fuse_fwd_f32(_ptr(v), _ptr(t), _ptr(weight_u), _ptr(s.epoch_idx), _ptr(s.epoch_w), U, N, s.k, D,
                                                 _ptr(out), _stream())
        ctx.save_for_backward(v, t, weight_u)
        ctx.s, ctx.U = s, U
        return out

    @staticmethod
    def backward(ctx, g):
        v, t, weight_u = ctx.saved_tensors
        s, U, (N, D) = ctx.s, ctx.U, v.shape
        g = _f32c(g)
        dv, dt, dw = torch.empty_like(v), torch.empty_like(t), torch.empty_like(weight_u)   # every element is written
        _lib.load().chaorec_dualgnn_fuse_bwd_f32(_ptr(g), _ptr(v), _ptr(t), _ptr(weight_u), _ptr(s.rev_ptr), _ptr(s.rev_u),
                                                 _ptr(s.rev_w), U, N, D, _ptr(dv), _ptr(dt), _ptr(dw), _stream())
        return dv, dt, dw, None, None


def dualgnn_fuse(v, t, weight_u, s, num_user):
    """result[u] = x[u] + sum_j s.epoch_w[u, j] x[s.epoch_idx[u, j]] with x[r] = weight_u[r, 0] v[r] + weight_u[r, 1] t[r] for
    u < num_user, result[r] = v[r] + t[r] below: DualGNN's whole table from the two modality tables in one launch."""
    return _DualGNNFuse.apply(v, t, weight_u, s, num_user)


COHESION_DIM = 64            # Model/COHESION.py:92 hard-codes dim_latent; the cf_* kernels are instantiated for it alone
COHESION_CHUNK = 64          # entries of a reverse list one lane group sums in the backward


class RevChunks:
    """The reverse lists of an epoch graph cut into chunks of `chunk` entries (0: one chunk per non-empty list):
    chunk_row int32 [n_chunks] (the row a chunk belongs to), chunk_first int64 [n_chunks] (its first entry in rev_u / rev_w),
    row_chunk int64 [U + 1] (row r's chunks are [row_chunk[r], row_chunk[r + 1]), in list order)."""

    def __init__(self, chunk, chunk_row, chunk_first, row_chunk):
        self.chunk, self.n_chunks = int(chunk), int(chunk_row.numel())
        self.chunk_row, self.chunk_first, self.row_chunk = chunk_row, chunk_first, row_chunk


def usergraph_rev_chunks(s, chunk=COHESION_CHUNK):
    """Index the chunks of s.rev_ptr (once per epoch graph; tensor ops and one read of the chunk count) -> RevChunks, kept
    in s.rev_chunks[chunk] until the next usergraph_sample / set_epoch."""
    chunk = int(chunk)
    if chunk < 0 or chunk > 2**31 - 1:
        raise ValueError(f"usergraph: chunk = {chunk} (0 = one chunk per list, else the entries per chunk)")
    if s.k < 1:
        raise ValueError("usergraph: no epoch graph yet (usergraph_sample / set_epoch)")
    U, dev = s.num_user, s.rev_ptr.device
    length = s.rev_ptr[1:] - s.rev_ptr[:-1]
    per_row = torch.div(length + (chunk - 1), chunk, rounding_mode="floor") if chunk > 0 else (length > 0).to(torch.int64)
    row_chunk = torch.zeros(U + 1, dtype=torch.int64, device=dev)
    torch.cumsum(per_row, 0, out=row_chunk[1:])
    n_chunks = int(row_chunk[-1])
    rows = torch.repeat_interleave(torch.arange(U, dtype=torch.int64, device=dev), per_row, output_size=n_chunks)
    within = torch.arange(n_chunks, dtype=torch.int64, device=dev) - row_chunk[rows]
    chunk_first = (s.rev_ptr[rows] + within * chunk).contiguous()
    out = RevChunks(chunk, rows.to(torch.int32).contiguous(), chunk_first, row_chunk)
    s.rev_chunks[chunk] = out
    return out


class _CohesionFuse(torch.autograd.Function):
    """(idr, v, t [N, 64]; h_id, h_v, h_t [I, 64] or None) -> result [N, 192] (Model/COHESION.py:340-359): none of the
    [N, 192] concatenation, user_rep, features[user_graph] [U, k, 192] or h_u exists in memory, forward or backward."""

    @staticmethod
    def forward(ctx, idr, v, t, h_id, h_v, h_t, s, num_user, chunk):
        _need_cuda(idr, v, t, s.epoch_idx)
        D = COHESION_DIM
        if v.dim() != 2 or v.shape[1] != D:
            raise ValueError(f"cohesion_fuse: v is {tuple(v.shape)}, the kernels are built for D = {D}")
        U, N = int(num_user), int(v.shape[0])
        if U != s.num_user or N < U:
            raise ValueError(f"cohesion_fuse: {U} users, a table of {N} rows, a user graph of {s.num_user} users")
        idr, v, t = (_vae_f32("cohesion_fuse", a, n, (N, D)) for a, n in ((idr, "idr"), (v, "v"), (t, "t")))
        hs = (h_id, h_v, h_t)
        if any(h is None for h in hs) != all(h is None for h in hs):
            raise ValueError("cohesion_fuse: h_id, h_v, h_t are given together or not at all")
        has_h = h_id is not None
        if has_h:
            _need_cuda(*hs)
            h_id, h_v, h_t = (_vae_f32("cohesion_fuse", a, n, (N - U, D)) for a, n in zip(hs, ("h_id", "h_v", "h_t")))
        if s.k < 1:
            raise ValueError("cohesion_fuse: no epoch graph yet (usergraph_sample / set_epoch)")
        ctx.chunks = s.rev_chunks.get(int(chunk)) or usergraph_rev_chunks(s, chunk)
        out = torch.empty((N, 3 * D), dtype=torch.float32, device=v.device)
        _lib.load().chaorec_cohesion_fuse_fwd_f32(_ptr(idr), _ptr(v), _ptr(t), _ptr(h_id), _ptr(h_v), _ptr(h_t), _ptr(s.epoch_idx),
                                                  _ptr(s.epoch_w), U, N, s.k, D, _ptr(out), _stream())
        ctx.s, ctx.U, ctx.N, ctx.has_h = s, U, N, has_h
        return out

    @staticmethod
    def backward(ctx, g):
        s, U, N, c, D = ctx.s, ctx.U, ctx.N, ctx.chunks, COHESION_DIM
        g = _f32c(g)
        dev = g.device
        dv, dt = torch.empty((N, D), dtype=torch.float32, device=dev), torch.empty((N, D), dtype=torch.float32, device=dev)
        dh_v = torch.empty((N - U, D), dtype=torch.float32, device=dev) if ctx.has_h else None
        dh_t = torch.empty((N - U, D), dtype=torch.float32, device=dev) if ctx.has_h else None
        part = torch.empty((c.n_chunks, 2 * D), dtype=torch.float32, device=dev)     # every row is written before it is read
        _lib.load().chaorec_cohesion_fuse_bwd_f32(_ptr(g), _ptr(s.rev_ptr), _ptr(s.rev_u), _ptr(s.rev_w), _ptr(c.chunk_row),
                                                  _ptr(c.chunk_first), _ptr(c.row_chunk), c.n_chunks, c.chunk, U, N, D, _ptr(part),
                                                  _ptr(dv), _ptr(dt), _ptr(dh_v), _ptr(dh_t), _stream())
        return None, dv, dt, None, dh_v, dh_t, None, None, None


def cohesion_fuse(idr, v, t, h_id, h_v, h_t, s, num_user, chunk=COHESION_CHUNK):
    """result[u] = x[u] + sum_j s.epoch_w[u, j] x[s.epoch_idx[u, j]] with x[r] = (idr[r] | v[r] | t[r]) for u < num_user,
    result[r] = x[r] + (h_id | h_v | h_t)[r - num_user] below (x[r] when the h tables are None): COHESION's whole [N, 192]
    table in one launch.  idr and h_id receive no gradient (the reference detaches the id third).  The backward sums every
    reverse list in chunks of `chunk` entries (0: unchunked) and adds the partials in chunk order: see the header."""
    return _CohesionFuse.apply(idr, v, t, h_id, h_v, h_t, s, num_user, chunk)


# --------------------------------------------------------------------------------------------
# MVGAE (csrc/mvgae.hip): the conv epilogue and the product-of-experts / KL / BPR tail, each one autograd node
# --------------------------------------------------------------------------------------------
MVGAE_DIM = 64               # the row width the mg_* kernels tile
MVGAE_VIEWS = 4              # P (the product of experts), V, T, C


def mvgae_check_shape(D):
    if int(D) != MVGAE_DIM:
        raise ValueError(f"MVGAE: dim_E={D}; the kernels tile D={MVGAE_DIM}")


def mvgae_rows():
    """(rows per wave, rows per workgroup) of the mg_* kernels."""
    lib = _lib.load()
    return int(lib.chaorec_mvgae_rows_per_wave()), int(lib.chaorec_mvgae_rows_per_block())


def mvgae_tick(state):
    step_tick(state, "chaorec_mvgae_tick")


class _MVGAEConvTail(torch.autograd.Function):
    """(s [N, 64], bias [64]) -> leaky_relu(dropout_0.1(normalize(s + bias))): one launch each way, nothing kept but s."""

    @staticmethod
    def forward(ctx, s, bias, state, seed, salt, training, keep):
        _need_cuda(s, bias, state, keep)
        s, bias = _vae_f32("mvgae", s.contiguous(), "s"), _vae_f32("mvgae", bias, "bias", (MVGAE_DIM,))
        if s.dim() != 2 or s.shape[1] != MVGAE_DIM:
            raise ValueError(f"mvgae: s is {tuple(s.shape)}, the kernels tile [N, {MVGAE_DIM}]")
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
            if keep.shape != s.shape:
                raise ValueError("mvgae: keep must have s's shape")
        y = torch.empty_like(s)
        _lib.load().chaorec_mvgae_conv_fwd_f32(_ptr(s), _ptr(bias), s.shape[0], _ptr(keep), int(seed), _ptr(state), int(salt),
                                               int(training), _ptr(y), _stream())
        ctx.save_for_backward(s, bias)
        ctx.draw = (state, int(seed), int(salt), int(training), keep)
        return y

    @staticmethod
    def backward(ctx, gy):
        s, bias = ctx.saved_tensors
        state, seed, salt, training, keep = ctx.draw
        gs = torch.empty_like(s)
        _lib.load().chaorec_mvgae_conv_bwd_f32(_ptr(_f32c(gy)), _ptr(s), _ptr(bias), s.shape[0], _ptr(keep), seed, _ptr(state), salt,
                                               training, _ptr(gs), _stream())
        return gs, (col_sum(gs) if ctx.needs_input_grad[1] else None), None, None, None, None, None


def mvgae_conv_tail(s, bias, state, seed, salt, training, keep=None):
    """-> y [N, 64].  keep: given flags [N, 64] (training only); None: the counter RNG keyed (seed, state[1], salt)."""
    return _MVGAEConvTail.apply(s, bias, state, seed, salt, bool(training), keep if training else None)


def mvgae_slot_index(users, pos, neg, n_rows, row_ids=None):
    """-> (slot_ptr int64 [N + 1], perm int64 [3B]): row r is named by the slots perm[slot_ptr[r] : slot_ptr[r + 1]] of
    [users; pos; neg] -- a stable sort, so first as user, then as positive, then as negative, each in ascending sample order
    (capturable: no host decision).  row_ids: a kept arange(N + 1)."""
    ids = torch.cat((users, pos, neg))
    sorted_ids, perm = torch.sort(ids, stable=True)
    if row_ids is None:
        row_ids = torch.arange(n_rows + 1, dtype=torch.int64, device=ids.device)
    return torch.searchsorted(sorted_ids, row_ids).contiguous(), perm.contiguous()


class _MVGAETail(torch.autograd.Function):
    """Six [N, 64] tables -> total [1], parts [8], Pm [N, 64], eps rows [4, 3, B, 64] (csrc/mvgae.hip (b))."""

    @staticmethod
    def forward(ctx, Vm, Vl, Tm, Tl, Cm, Cl, users, pos, neg, kl_weight, state, seed, training, eps, want_eps, row_ids):
        tabs = [Vm, Vl, Tm, Tl, Cm, Cl]
        _need_cuda(*tabs, users, pos, neg, state, eps)
        N = Vm.shape[0]
        tabs = [_vae_f32("mvgae", t.contiguous(), "table", (N, MVGAE_DIM)) for t in tabs]
        users, pos, neg = (t.to(torch.int64).contiguous() for t in (users, pos, neg))
        B, dev = users.numel(), Vm.device
        if pos.numel() != B or neg.numel() != B or B == 0:
            raise ValueError("mvgae: users, pos and neg must be three non-empty id vectors of one length")
        if eps is not None:
            eps = _vae_f32("mvgae", eps, "eps", (MVGAE_VIEWS, N, MVGAE_DIM))
        lib = _lib.load()
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)   # noqa: E731
        Pm, zrows, bpr, coef, out = f(N, MVGAE_DIM), f(MVGAE_VIEWS, 3, B, MVGAE_DIM), f(MVGAE_VIEWS, B), f(MVGAE_VIEWS, B), f(9)
        eps_out = f(MVGAE_VIEWS, 3, B, MVGAE_DIM) if want_eps else None
        nbytes = lib.chaorec_mvgae_tail_workspace_bytes(N)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        lib.chaorec_mvgae_tail_fwd_f32(*(_ptr(t) for t in tabs), N, _ptr(users), _ptr(pos), _ptr(neg), B, _ptr(eps), int(seed),
                                       _ptr(state), int(training), float(kl_weight), _ptr(Pm), _ptr(zrows), _ptr(eps_out), _ptr(bpr),
                                       _ptr(coef), _ptr(ws), nbytes, _ptr(out), _stream())
        slot_ptr, perm = mvgae_slot_index(users, pos, neg, N, row_ids)
        ctx.save_for_backward(*tabs, zrows, coef, slot_ptr, perm)
        ctx.draw = (state, int(seed), int(training), float(kl_weight), eps)
        total, parts = out[:1], out[1:]
        ctx.mark_non_differentiable(parts, Pm)
        if want_eps:
            ctx.mark_non_differentiable(eps_out)
            return total, parts, Pm, eps_out
        return total, parts, Pm

    @staticmethod
    def backward(ctx, gtotal, *_):
        *tabs, zrows, coef, slot_ptr, perm = ctx.saved_tensors
        state, seed, training, kl_weight, eps = ctx.draw
        N, B = tabs[0].shape[0], coef.shape[1]
        grads = [torch.empty_like(t) for t in tabs]
        _lib.load().chaorec_mvgae_tail_bwd_f32(*(_ptr(t) for t in tabs), N, _ptr(slot_ptr), _ptr(perm), B, _ptr(zrows), _ptr(coef),
                                               _ptr(eps), seed, _ptr(state), training, kl_weight, _ptr(_f32c(gtotal).reshape(1)),
                                               *(_ptr(g) for g in grads), _stream())
        return (*grads, None, None, None, None, None, None, None, None, None, None)


def mvgae_tail(Vm, Vl, Tm, Tl, Cm, Cl, users, pos, neg, kl_weight, state, seed, training, eps=None, return_eps=False,
               row_ids=None):
    """-> (total [1], parts [8] = BPR_P, V, T, C, KL_P, V, T, C, Pm [N, 64][, the eps rows [4, 3, B, 64] of the batch's user,
    positive and negative rows]).  users, pos, neg: GLOBAL row ids in [0, N).  eps: given noise [4, N, 64] in the order P, V,
    T, C (training only); None: the counter RNG keyed (seed, state[1], 16 + view, row, d)."""
    return _MVGAETail.apply(Vm, Vl, Tm, Tl, Cm, Cl, users, pos, neg, kl_weight, state, seed, bool(training),
                            eps if training else None, bool(return_eps), row_ids)


# --------------------------------------------------------------------------------------------
# DiffMM (csrc/diffmm.hip): the noised history rows in one launch, the denoiser's output layer with both losses and the
# gradient by its output in one pass
# --------------------------------------------------------------------------------------------
DIFFMM_D = 64                # the embedding width of r and F


def diffmm_check_shape(B, I, H, D=DIFFMM_D):
    _lib.load().chaorec_diffmm_check_shape(int(B), int(I), int(H), int(D))


def diffmm_tiles():
    """(bm, bn, bk) of the one-pass output layer."""
    v = [ctypes.c_int32(0) for _ in range(3)]
    _lib.load().chaorec_diffmm_tiles(*(ctypes.byref(x) for x in v))
    return tuple(int(x.value) for x in v)


def diffmm_rows_per_block():
    return int(_lib.load().chaorec_diffmm_rows_per_block())


def diffmm_ld(num_item):
    """The row stride of x_in and d_out: I rounded up to a multiple of 4 (float4 stores, vector loads in the GEMMs)."""
    return (int(num_item) + 3) // 4 * 4


def diffmm_rows(users, rowptr, col, num_item, a_row=None, s_row=None, noise=None, keep=None, seed=0, step=0, salt=0, plain=False):
    """users int64 [B] -> (x_in fp32 [B, I], a view of a [B, ld] buffer whose pad columns are 0; bits uint32-as-int32
    [B, ceil(I / 32)]).  plain: the multi-hot rows themselves.  Otherwise x_in = dropout_0.5(a x0 + s n) with n and the keep
    flags given ([B, I]) or drawn from the counter RNG keyed (seed, step, salt, user, item)."""
    _need_cuda(users, rowptr, col, a_row, s_row, noise, keep)
    users = users.to(torch.int64).contiguous()
    B, I, U = users.numel(), int(num_item), rowptr.numel() - 1
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32:
        raise TypeError("diffmm_rows: rowptr must be int64 and col int32")
    if not plain:
        a_row, s_row = _vae_f32("diffmm", a_row, "a_row", (B,)), _vae_f32("diffmm", s_row, "s_row", (B,))
        if noise is not None:
            noise = _vae_f32("diffmm", noise, "noise", (B, I))
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
            if tuple(keep.shape) != (B, I):
                raise ValueError("diffmm: keep must be [B, I]")
    ld = diffmm_ld(I)
    x = torch.empty((B, ld), dtype=torch.float32, device=users.device)
    bits = torch.empty((B, (I + 31) // 32), dtype=torch.int32, device=users.device)
    _lib.load().chaorec_diffmm_rows_f32(_ptr(users), B, U, _ptr(rowptr), _ptr(col), I, ld, _ptr(a_row), _ptr(s_row),
                                        _ptr(None if plain else noise), _ptr(None if plain else keep), int(seed), int(step),
                                        int(salt), int(bool(plain)), _ptr(x), _ptr(bits), _stream())
    return x[:, :I], bits


def _diffmm_big(rows):
    """The split-bf16 GEMMs read strided operands in place and pay from a few hundred rows on (ops_dense._linear_fwd_raw)."""
    return _ops.LINEAR_FORWARD == "bf16x3" and rows >= 256


def diffmm_out_loss_raw(h, W_out, b_out, bits, x0E, F, w, e_loss):
    """The forward of diffmm_denoise_loss without a tape -> (loss [1], diff_rows [B] float64, gc_rows [B], d_out [B, ld] with
    d loss / d out in its first I columns and 0 in the rest, r [B, 64])."""
    _need_cuda(h, W_out, b_out, bits, x0E, F, w)
    B, H = h.shape
    I = W_out.shape[0]
    h, W_out = _ops._f32rows(h), _ops._f32rows(W_out)
    b_out, F = _vae_f32("diffmm", b_out, "b_out", (I,)), _vae_f32("diffmm", F, "F", (I, DIFFMM_D))
    x0E = _vae_f32("diffmm", x0E, "x0E", (B, DIFFMM_D))
    if W_out.shape[1] != H or tuple(bits.shape) != (B, (I + 31) // 32) or bits.dtype != torch.int32 or not bits.is_contiguous():
        raise ValueError("diffmm: W_out must be [I, H] and bits int32 [B, ceil(I / 32)]")
    if w.dtype != torch.float64 or tuple(w.shape) != (B,):
        raise ValueError("diffmm: the weight is float64 [B] (GaussianDiffusion.SNR works on float64 tables)")
    diffmm_check_shape(B, I, H)
    lib, dev = _lib.load(), h.device
    M = gemm_raw(W_out, F, transA=True)                                     # [H, 64]
    r = gemm_raw(h, M)                                                      # [B, 64]
    r = (r + gemm_raw(b_out.reshape(1, I), F) - x0E).contiguous()
    w = w.contiguous()
    c_row = (w * (2.0 / (float(B) * float(I)))).to(torch.float32)           # formed in double
    kf = 2.0 * float(e_loss) / (float(B) * DIFFMM_D)
    bn = diffmm_tiles()[1]
    ld, NT = diffmm_ld(I), (I + bn - 1) // bn
    d_out = torch.empty((B, ld), dtype=torch.float32, device=dev)
    part = torch.empty((B, NT), dtype=torch.float32, device=dev)
    diff_rows = torch.empty(B, dtype=torch.float64, device=dev)
    gc_rows, loss = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
    lib.chaorec_diffmm_out_loss_f32(_ptr(h), h.stride(0), _ptr(W_out), W_out.stride(0), _ptr(b_out), _ptr(bits), _ptr(r), _ptr(F),
                                    _ptr(w), _ptr(c_row), kf, float(e_loss), B, I, H, _ptr(d_out), ld, _ptr(part),
                                    _ptr(diff_rows), _ptr(gc_rows), _ptr(loss), _stream())
    return loss, diff_rows, gc_rows, d_out, r


class _DiffMMDenoiseLoss(torch.autograd.Function):
    """(h [B, H], W_out [I, H], b_out [I]) -> loss [1], diff_rows [B] float64, gc_rows [B] (Model/DiffMM.py:468-471,
    :640-658).  Forward: M = W_out^T F, r = h M + b_out F - x0 E (three small GEMMs), then the one-pass launch, which leaves
    d loss / d out.  Backward: dW_out = d_out^T (g h), dh = g (d_out W_out), db_out = g colsum(d_out); g is folded into the
    [B, H] operands, d_out is not passed over again."""

    @staticmethod
    def forward(ctx, h, W_out, b_out, bits, x0E, F, w, e_loss):
        loss, diff_rows, gc_rows, d_out, _ = diffmm_out_loss_raw(h, W_out, b_out, bits, x0E, F, w, e_loss)
        ctx.save_for_backward(h, W_out, d_out)
        ctx.mark_non_differentiable(diff_rows, gc_rows)
        return loss, diff_rows, gc_rows

    @staticmethod
    def backward(ctx, g, _gd, _gg):
        h, W_out, d_full = ctx.saved_tensors
        B, I = h.shape[0], W_out.shape[0]
        g = _f32c(g).reshape(1)
        d_out = d_full[:, :I]
        dW = dh = db = None
        if ctx.needs_input_grad[1]:
            gh = h * g
            dW = gemm_tn_bf16x3(d_out, gh) if _diffmm_big(B) else gemm_raw(d_out.contiguous(), gh.contiguous(), transA=True)
        if ctx.needs_input_grad[0]:
            dh = gemm_nn_bf16x3(d_out, W_out) if _diffmm_big(B) else gemm_raw(d_out.contiguous(), W_out.contiguous())
            dh = dh * g
        if ctx.needs_input_grad[2]:
            db = col_sum(d_full)[:I] * g
        return dh, dW, db, None, None, None, None, None


def diffmm_denoise_loss(h, W_out, b_out, bits, x0E, F, w, e_loss):
    """-> (loss [1] = mean_b w_b mse_b + e_loss mean_b gc_b, diff_rows [B] float64, gc_rows [B]).  bits: the x0 bit table of
    diffmm_rows; x0E [B, 64] = the batch's history-row sums of the item embeddings; F [I, 64] the modality's projected
    features; w float64 [B] the SNR weight.  x0E and F carry no gradient (the reference detaches them)."""
    return _DiffMMDenoiseLoss.apply(h, W_out, b_out, bits, x0E.detach(), F.detach(), w, float(e_loss))


# --------------------------------------------------------------------------------------------
# AdaGCL (csrc/adagcl.hip): the per-entry work of its two view generators over one graph.DropoutStructure
# --------------------------------------------------------------------------------------------
ADAGCL_DIM = 64              # the row width the keep kernel tiles


def adagcl_check_shape(D):
    if int(D) != ADAGCL_DIM:
        raise ValueError(f"AdaGCL: dim_E={D}; the kernels tile D={ADAGCL_DIM}")


def adagcl_tick(state):
    step_tick(state, "chaorec_adagcl_tick")


def _adagcl_parts(structure, device):
    n = int(_lib.load().chaorec_adagcl_rows_per_block())
    n_part = (structure.n_rows + n - 1) // n
    return torch.empty(n_part, dtype=torch.float32, device=device), n_part


class _AdaGCLEdgeGate(torch.autograd.Function):
    """Two per-node scores -> (val [E], l0 [1], m [E], d [N], u [E] or None) (csrc/adagcl.hip (a), (b))."""

    @staticmethod
    def forward(ctx, s_nb, s_self, b_att, st, beta, eps, training, state, seed, salt, u):
        _need_cuda(s_nb, s_self, b_att, st.rowptr, state, u)
        N, E = st.n_rows, st.nnz
        s_nb = _vae_f32("adagcl", s_nb.detach().contiguous(), "s_nb", (N,))
        s_self = _vae_f32("adagcl", s_self.detach().contiguous(), "s_self", (N,))
        b_att = _vae_f32("adagcl", b_att.detach().contiguous().reshape(-1), "b_att", (1,))
        if u is not None:
            u = _vae_f32("adagcl", u, "u", (E,))
        elif training and state is None:
            raise ValueError("adagcl: the training form needs given draws u or a device step counter")
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=s_nb.device)  # noqa: E731
        m, S, d, val, l0 = f(E), f(N), f(N), f(E), f(1)
        u_used = u if (u is not None or not training) else f(E)
        part, n_part = _adagcl_parts(st, s_nb.device)
        _lib.load().chaorec_adagcl_gate_fwd_f32(_ptr(st.rowptr), _ptr(st.col), _ptr(st.entry_row), N, E, _ptr(s_nb), _ptr(s_self),
                                                _ptr(b_att), float(beta), float(eps), int(bool(training)), _ptr(u), int(seed),
                                                _ptr(state), int(salt), _ptr(m), _ptr(S), _ptr(d), _ptr(val), _ptr(l0),
                                                _ptr(u_used if u is None else None), _ptr(part), n_part, _stream())
        ctx.st, ctx.beta, ctx.training = st, float(beta), bool(training)
        ctx.save_for_backward(s_nb, s_self, b_att, m, S, d, u_used if training else None)
        ctx.mark_non_differentiable(m, d)
        if training:
            ctx.mark_non_differentiable(u_used)
        return val, l0, m, d, (u_used if training else None)

    @staticmethod
    def backward(ctx, g_val, g_l0, *_):
        s_nb, s_self, b_att, m, S, d, u = ctx.saved_tensors
        st = ctx.st
        N, E = st.n_rows, st.nnz
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=s_nb.device)  # noqa: E731
        g_val = torch.zeros(E, dtype=torch.float32, device=s_nb.device) if g_val is None else _f32c(g_val)
        g_l0 = None if g_l0 is None else _f32c(g_l0).reshape(-1)
        g_logit, g_S, g_nb, g_self, g_b = f(E), f(N), f(N), f(N), f(1)
        part, n_part = _adagcl_parts(st, s_nb.device)
        _lib.load().chaorec_adagcl_gate_bwd_f32(_ptr(st.rowptr), _ptr(st.col), _ptr(st.transpose_entry), N, E, _ptr(s_nb), _ptr(s_self),
                                                _ptr(b_att), ctx.beta, int(ctx.training), _ptr(u), _ptr(m), _ptr(S), _ptr(d),
                                                _ptr(g_val), _ptr(g_l0), _ptr(g_logit), _ptr(g_S), _ptr(g_nb), _ptr(g_self), _ptr(g_b),
                                                _ptr(part), n_part, _stream())
        return g_nb, g_self, g_b, None, None, None, None, None, None, None, None


def adagcl_edge_gate(structure, s_nb, s_self, b_att, beta, eps, training, state, seed, salt, u=None, return_parts=False):
    """DenoisingNet's hard-concrete gate over the stored entries of `structure` (a graph.DropoutStructure) from the two
    per-node scores: -> (val [E], l0 [1]); return_parts adds (m [E], d [N], u [E] -- the draws used, None in evaluation).
    training: the noised form at temperature beta with eps on the row sums; u: given draws in [1e-7, 1 - 1e-7], else drawn in
    the launch keyed (seed, state[1], salt).  b_att: the one-element bias tensor.  One autograd node."""
    out = _AdaGCLEdgeGate.apply(s_nb, s_self, b_att.reshape(-1), structure, beta, eps, bool(training), state, seed, salt, u)
    return out if return_parts else out[:2]


def adagcl_edge_keep(structure, z, W1, b1, w2, b2, vals, return_logits=False):
    """vgae.generate's keep decision per stored entry (csrc/adagcl.hip (c)); no gradient.  z [N, 64], W1 [64, 64], b1 [64],
    w2 [64] or [1, 64], b2 [1], vals [E] -> (out [E] = kept ? vals / fl32(kept / E) : +0, keep bool [E], kept int64 [1] on the
    device[, logits [E]])."""
    _need_cuda(z, W1, b1, w2, b2, vals, structure.rowptr)
    N, E = structure.n_rows, structure.nnz
    with torch.no_grad():
        if z.dim() != 2:
            raise ValueError(f"adagcl: z is {tuple(z.shape)}, expected [N, {ADAGCL_DIM}]")
        adagcl_check_shape(z.shape[1])
        z = _vae_f32("adagcl", z.detach().contiguous(), "z", (N, ADAGCL_DIM))
        W1 = _vae_f32("adagcl", W1.detach().contiguous(), "W1", (ADAGCL_DIM, ADAGCL_DIM))
        b1 = _vae_f32("adagcl", b1.detach().contiguous(), "b1", (ADAGCL_DIM,))
        w2 = _vae_f32("adagcl", w2.detach().contiguous().reshape(-1), "w2", (ADAGCL_DIM,))
        b2 = _vae_f32("adagcl", b2.detach().contiguous().reshape(-1), "b2", (1,))
        vals = _vae_f32("adagcl", vals.detach().contiguous(), "vals", (E,))
        keep = torch.empty(E, dtype=torch.uint8, device=z.device)
        out = torch.empty(E, dtype=torch.float32, device=z.device)
        kept = torch.empty(1, dtype=torch.int64, device=z.device)
        logits = torch.empty(E, dtype=torch.float32, device=z.device) if return_logits else None
        _lib.load().chaorec_adagcl_keep_f32(_ptr(z), N, _ptr(structure.entry_row), _ptr(structure.col), E, _ptr(W1), _ptr(b1), _ptr(w2),
                                            _ptr(b2), _ptr(vals), _ptr(keep), _ptr(out), _ptr(kept), _ptr(logits), _stream())
    res = (out, keep.to(torch.bool), kept)
    return res + (logits,) if return_logits else res


# --------------------------------------------------------------------------------------------
# Grade (csrc/grade.hip): the views of its G generators over one graph.DropoutStructure, three launches
# --------------------------------------------------------------------------------------------
GRADE_DIM = 64               # the row width the kernels tile


def grade_check_shape(D):
    if int(D) != GRADE_DIM:
        raise ValueError(f"Grade: dim_E={D}; the kernels tile D={GRADE_DIM}")


def grade_pair_owner(structure):
    """The entries with entry_row[e] <= col[e], ascending, int32 [P]: every stored entry is e or transpose_entry[e] of exactly
    one of them.  Built once per structure (one host round trip for P) and cached on the structure object."""
    owner = getattr(structure, "pair_owner", None)
    if owner is None:
        owner = torch.nonzero(structure.entry_row <= structure.col).reshape(-1).to(torch.int32).contiguous()
        structure.pair_owner = owner
    return owner


def grade_views(structure, z, W1, b1, w2, b2, return_parts=False):
    """The normalised views of G generators (vgae.generate, Model/Grade.py:119-151) per stored entry of `structure` (a
    graph.DropoutStructure); no gradient, no host synchronisation (the owner list is cached by grade_pair_owner).
    z [G, N, 64] or [N, 64] (G = 1), W1 [G, 64, 64], b1 [G, 64], w2 [G, 64] or [G, 1, 64], b2 [G] or [G, 1] -> val [G, E];
    return_parts adds (keep bool [G, E], kept int64 [G] on the device, logits [G, E], d [G, N])."""
    _need_cuda(z, W1, b1, w2, b2, structure.rowptr)
    N, E = structure.n_rows, structure.nnz
    with torch.no_grad():
        if z.dim() == 2:
            z = z.unsqueeze(0)
        if z.dim() != 3:
            raise ValueError(f"grade: z is {tuple(z.shape)}, expected [G, N, {GRADE_DIM}]")
        grade_check_shape(z.shape[2])
        G = int(z.shape[0])
        z = _vae_f32("grade", z.detach().contiguous(), "z", (G, N, GRADE_DIM))
        W1 = _vae_f32("grade", W1.detach().contiguous().reshape(-1, GRADE_DIM, GRADE_DIM), "W1", (G, GRADE_DIM, GRADE_DIM))
        b1 = _vae_f32("grade", b1.detach().contiguous().reshape(-1, GRADE_DIM), "b1", (G, GRADE_DIM))
        w2 = _vae_f32("grade", w2.detach().contiguous().reshape(-1, GRADE_DIM), "w2", (G, GRADE_DIM))
        b2 = _vae_f32("grade", b2.detach().contiguous().reshape(-1), "b2", (G,))
        owner = grade_pair_owner(structure)
        val = torch.empty(G, E, dtype=torch.float32, device=z.device)
        keep = torch.empty(G, E, dtype=torch.uint8, device=z.device)
        kept = torch.empty(G, dtype=torch.int64, device=z.device)
        d = torch.empty(G, N, dtype=torch.float32, device=z.device)
        logits = torch.empty(G, E, dtype=torch.float32, device=z.device) if return_parts else None
        _lib.load().chaorec_grade_views_f32(_ptr(z), _ptr(W1), _ptr(b1), _ptr(w2), _ptr(b2), G, N, _ptr(structure.rowptr),
                                            _ptr(structure.col), _ptr(structure.entry_row), _ptr(structure.transpose_entry), E,
                                            _ptr(owner), int(owner.numel()), _ptr(val), _ptr(keep), _ptr(kept), _ptr(logits), _ptr(d),
                                            _stream())
    return (val, keep.to(torch.bool), kept, logits, d) if return_parts else val


# --------------------------------------------------------------------------------------------
# GraphAug (csrc/graphaug.hip): the view learner's edge sampler, the contrastive loss's whole-table log-sum-exp, the
# propagate's random-entry term
# --------------------------------------------------------------------------------------------
GRAPHAUG_DIM = 64            # the row width the kernels tile


def graphaug_check_shape(D):
    if int(D) != GRAPHAUG_DIM:
        raise ValueError(f"GraphAug: dim_E={D}; the kernels tile D={GRAPHAUG_DIM}")


def graphaug_edge_sample(structure, P, Q, b1, w2, b2, u1=None, u2=None, state=None, seed=0, salt=0, want_val_t=True,
                         return_logits=False, return_draws=False):
    """The view learner's sampled value per stored entry of `structure` (a graph.DropoutStructure), csrc/graphaug.hip (a); no
    gradient.  P = z W1[:, :64]^T and Q = z W1[:, 64:]^T fp32 [N, 64], b1 [64], w2 [64] or [1, 64], b2 [1]; u1, u2 fp32 [E]
    given draws, or None: drawn in the launch keyed (seed, state[1], salt).  -> (val [E], val_t [E] or None, logits [E] or
    None, u [2, E] -- the draws used -- or None)."""
    _need_cuda(P, Q, b1, w2, b2, u1, u2, state, structure.rowptr)
    N, E = structure.n_rows, structure.nnz
    with torch.no_grad():
        if P.dim() != 2:
            raise ValueError(f"graphaug: P is {tuple(P.shape)}, expected [N, {GRAPHAUG_DIM}]")
        graphaug_check_shape(P.shape[1])
        P = _vae_f32("graphaug", P.detach().contiguous(), "P", (N, GRAPHAUG_DIM))
        Q = _vae_f32("graphaug", Q.detach().contiguous(), "Q", (N, GRAPHAUG_DIM))
        b1 = _vae_f32("graphaug", b1.detach().contiguous(), "b1", (GRAPHAUG_DIM,))
        w2 = _vae_f32("graphaug", w2.detach().contiguous().reshape(-1), "w2", (GRAPHAUG_DIM,))
        b2 = _vae_f32("graphaug", b2.detach().contiguous().reshape(-1), "b2", (1,))
        if (u1 is None) != (u2 is None):
            raise ValueError("graphaug: give both u1 and u2, or neither")
        if u1 is not None:
            u1, u2 = _vae_f32("graphaug", u1, "u1", (E,)), _vae_f32("graphaug", u2, "u2", (E,))
        elif state is None:
            raise ValueError("graphaug: the sampler needs given draws or a device step counter")
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=P.device)  # noqa: E731
        val = f(E)
        val_t = f(E) if want_val_t else None
        logits = f(E) if return_logits else None
        u_out = f(2, E) if return_draws else None
        _lib.load().chaorec_graphaug_sample_f32(_ptr(structure.rowptr), _ptr(structure.col), _ptr(structure.transpose_entry), N, E,
                                                _ptr(P), _ptr(Q), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(u1), _ptr(u2), int(seed),
                                                _ptr(state), int(salt), _ptr(val), _ptr(val_t), _ptr(logits), _ptr(u_out), _stream())
    return val, val_t, logits, u_out


class _GraphAugLSE(torch.autograd.Function):
    """lse[b] = log sum_m exp(<A_b, T_m> inv_temp) without a [B, M] buffer (csrc/graphaug.hip (b))."""

    @staticmethod
    def forward(ctx, A, T, inv_temp):
        _need_cuda(A, T)
        if A.dim() != 2 or T.dim() != 2 or A.shape[1] != T.shape[1]:
            raise ValueError(f"graphaug_lse: A is {tuple(A.shape)}, T is {tuple(T.shape)}")
        graphaug_check_shape(A.shape[1])
        A = _vae_f32("graphaug_lse", A.detach().contiguous(), "A")
        T = _vae_f32("graphaug_lse", T.detach().contiguous(), "T")
        B, M = A.shape[0], T.shape[0]
        lib = _lib.load()
        splits = int(lib.chaorec_graphaug_lse_splits(B, M))
        part = torch.empty(splits * B, dtype=torch.float32, device=A.device)
        lse = torch.empty((2, B), dtype=torch.float32, device=A.device)      # [1]: what rounding [0] to fp32 lost
        lib.chaorec_graphaug_lse_fwd_f32(_ptr(A), _ptr(T), B, M, float(inv_temp), _ptr(part), splits, _ptr(lse), _stream())
        ctx.inv_temp, ctx.splits = float(inv_temp), splits
        ctx.save_for_backward(A, T, lse)
        return lse[0]

    @staticmethod
    def backward(ctx, g):
        A, T, lse = ctx.saved_tensors
        B, M = A.shape[0], T.shape[0]
        g = _f32c(g)
        part = torch.empty(ctx.splits * B * GRAPHAUG_DIM, dtype=torch.float32, device=A.device)
        dA, dT = torch.empty_like(A), torch.empty_like(T)
        _lib.load().chaorec_graphaug_lse_bwd_f32(_ptr(A), _ptr(T), B, M, ctx.inv_temp, _ptr(lse), _ptr(g), _ptr(part), ctx.splits,
                                                 _ptr(dA), _ptr(dT), _stream())
        return dA, dT, None


def graphaug_lse(A, T, inv_temp):
    """-> lse [B] = log sum_m exp(<A_b, T_m> inv_temp), A [B, 64], T [M, 64]: a plain sum without a running max (rows are
    expected normalised: |<a, t>| inv_temp stays far from fp32's exp range), no [B, M] buffer, one autograd node."""
    return _GraphAugLSE.apply(A, T, inv_temp)


class RandEntries:
    """A step's random entries (rows[k], cols[k]), all of one value, as a CSR and its transpose (duplicates kept: they add)."""

    def __init__(self, rows, cols, n):
        rows, cols = rows.long(), cols.long()
        self.n = int(n)
        self.rowptr, self.col = self._csr(rows, cols, self.n)
        self.rowptr_t, self.col_t = self._csr(cols, rows, self.n)

    @staticmethod
    def _csr(rows, cols, n):
        """sorted by (row, col) on the device; no host synchronisation"""
        key, _ = torch.sort(rows * n + cols)
        r = torch.div(key, n, rounding_mode="floor")
        rowptr = torch.searchsorted(r, torch.arange(n + 1, dtype=torch.int64, device=rows.device))
        return rowptr.contiguous(), (key - r * n).to(torch.int32).contiguous()


def _graphaug_rand_spmm(rowptr, col, n, x, z, alpha, slope):
    y = torch.empty((n, GRAPHAUG_DIM), dtype=torch.float32, device=x.device)
    _lib.load().chaorec_graphaug_rand_spmm_f32(_ptr(rowptr), _ptr(col), n, x.shape[0], _ptr(x), _ptr(z), float(alpha), float(slope),
                                               _ptr(y), _stream())
    return y


class _GraphAugRandLayer(torch.autograd.Function):
    """y = LeakyReLU_slope(z + alpha R x), R a RandEntries (csrc/graphaug.hip (c)); backward: g = gy (y > 0 ? 1 : slope),
    gz = g, gx = alpha R^T g."""

    @staticmethod
    def forward(ctx, z, x, R, alpha, slope):
        _need_cuda(z, x, R.rowptr)
        graphaug_check_shape(x.shape[1])
        z = _vae_f32("graphaug", z.detach().contiguous(), "z", (R.n, GRAPHAUG_DIM))
        x = _vae_f32("graphaug", x.detach().contiguous(), "x", (R.n, GRAPHAUG_DIM))
        y = _graphaug_rand_spmm(R.rowptr, R.col, R.n, x, z, alpha, slope)
        ctx.R, ctx.alpha, ctx.slope = R, float(alpha), float(slope)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, = ctx.saved_tensors
        g = torch.where(y > 0, gy, gy * ctx.slope).contiguous()
        gx = _graphaug_rand_spmm(ctx.R.rowptr_t, ctx.R.col_t, ctx.R.n, g, None, ctx.alpha, 1.0) if ctx.needs_input_grad[1] else None
        return g, gx, None, None, None


def graphaug_rand_layer(z, x, R, alpha=0.05, slope=0.5):
    """GCNLayer over a GraphAug view (Model/GraphAug.py:47-71): z = the learned entries' product with x, R the step's random
    entries of value alpha -> LeakyReLU_slope(z + alpha R x)."""
    return _GraphAugRandLayer.apply(z, x, R, alpha, slope)


# --------------------------------------------------------------------------------------------
# MHRec (csrc/mhrec.hip): the hypergraph attention layer with its residual / dropout epilogue, one autograd node
# --------------------------------------------------------------------------------------------
MHREC_DIM = 64               # the row width the kernels tile
MHREC_LONG_ROW = 256         # chaorec_mhrec_long_row(): a longer node row is cut into chunks
MHREC_CHUNK = 256            # chaorec_mhrec_chunk(): entries per chunk


def mhrec_check_shape(D):
    if int(D) != MHREC_DIM:
        raise ValueError(f"MHRec: dim_E={D}; the kernels tile D={MHREC_DIM}")


def mhrec_long_row():
    """The node-row length past which the layer's node launches hand a row to the chunk launches (the library's value)."""
    return int(_lib.load().chaorec_mhrec_long_row())


class HyperGraph:
    """A hypergraph of E hyperedges with exactly k distinct nodes each, all values 1 (what train_and_evaluate.py:394-497
    builds from torch.topk): `nodes` int32 [E, k], H^T as an ELL table, and the node-major CSR of the same pairs -- rowptr
    int64 [N + 1], edge int32 [E k], a node's hyperedges ascending (a stable sort of the flattened table by node).  Node rows
    longer than MHREC_LONG_ROW are listed with their chunks of MHREC_CHUNK entries: long_node int32 [L], long_cptr int64
    [L + 1], chunk_node int32 [C], chunk_beg int64 [C].  Built with tensor operations on the table's device; validate: ids in
    [0, N) and a hyperedge's nodes distinct, else ValueError."""

    def __init__(self, nodes, num_nodes, validate=True):
        nodes = torch.as_tensor(nodes)
        if nodes.dim() != 2 or nodes.shape[0] < 1 or nodes.shape[1] < 1 or nodes.dtype.is_floating_point:
            raise ValueError(f"HyperGraph: the node table must be an integer [E, k] tensor, got {tuple(nodes.shape)} {nodes.dtype}")
        E, k = int(nodes.shape[0]), int(nodes.shape[1])
        N, dev = int(num_nodes), nodes.device
        if N < 1 or E * k >= 2 ** 31:
            raise ValueError(f"HyperGraph: {N} nodes, {E} x {k} entries (fewer than 2^31)")
        flat = nodes.reshape(-1).to(torch.int64)
        if validate:
            lo, hi = int(flat.min()), int(flat.max())
            if lo < 0 or hi >= N:
                raise ValueError(f"HyperGraph: node ids span [{lo}, {hi}], expected [0, {N})")
            srt = torch.sort(flat.view(E, k), dim=1)[0]
            if k > 1 and bool((srt[:, 1:] == srt[:, :-1]).any()):
                raise ValueError("HyperGraph: a hyperedge names a node twice")
        self.num_nodes, self.num_edges, self.k = N, E, k
        self.nodes = nodes.to(torch.int32).contiguous()
        named, perm = torch.sort(flat, stable=True)
        self.edge = torch.div(perm, k, rounding_mode="floor").to(torch.int32).contiguous()
        self.rowptr = torch.searchsorted(named, torch.arange(N + 1, dtype=torch.int64, device=dev)).contiguous()
        deg = self.rowptr[1:] - self.rowptr[:-1]
        long_node = torch.nonzero(deg > MHREC_LONG_ROW).reshape(-1)
        n_chunks = torch.div(deg[long_node] + (MHREC_CHUNK - 1), MHREC_CHUNK, rounding_mode="floor")
        self.long_node = long_node.to(torch.int32).contiguous()
        self.long_cptr = torch.zeros(long_node.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(n_chunks, 0, out=self.long_cptr[1:])
        row_of = torch.repeat_interleave(torch.arange(long_node.numel(), dtype=torch.int64, device=dev), n_chunks)
        self.chunk_node = self.long_node[row_of].contiguous()
        self.chunk_beg = (self.rowptr[long_node[row_of]]
                          + (torch.arange(row_of.numel(), dtype=torch.int64, device=dev) - self.long_cptr[row_of]) * MHREC_CHUNK).contiguous()
        self.n_long, self.n_chunks = int(long_node.numel()), int(row_of.numel())

    def degrees(self):
        return self.rowptr[1:] - self.rowptr[:-1]

    def incidence(self):
        """H [N, E] as a coalesced torch sparse tensor of ones (what the reference's layer takes)."""
        rows = self.nodes.reshape(-1).to(torch.int64)
        cols = torch.arange(self.num_edges, dtype=torch.int64, device=rows.device).repeat_interleave(self.k)
        return torch.sparse_coo_tensor(torch.stack([rows, cols]), torch.ones(rows.numel(), dtype=torch.float32, device=rows.device),
                                       (self.num_nodes, self.num_edges)).coalesce()


def _mhrec_args(hg):
    return (_ptr(hg.nodes), hg.num_edges, hg.k, _ptr(hg.rowptr), _ptr(hg.edge), hg.num_nodes,
            _ptr(hg.long_node) if hg.n_long else None, _ptr(hg.long_cptr) if hg.n_long else None, hg.n_long,
            _ptr(hg.chunk_node) if hg.n_long else None, _ptr(hg.chunk_beg) if hg.n_long else None, hg.n_chunks)


class _MHRecHyperLayer(torch.autograd.Function):
    """(X [N, 64], a [128, 1]) -> y = dropout_0.5(attention(X) + X) over a HyperGraph; also returns the attention's own output
    `out` (no gradient flows through it).  Kept for the backward: X, a, the hyperedge sums Eo [E, 64], r [E], stat [N, 4], out."""

    @staticmethod
    def forward(ctx, X, a, hg, keep, state, seed, salt, training):
        _need_cuda(X, a, hg.nodes, keep, state)
        if X.dim() != 2 or X.shape[0] != hg.num_nodes:
            raise ValueError(f"mhrec: X is {tuple(X.shape)}, the hypergraph has {hg.num_nodes} nodes")
        mhrec_check_shape(X.shape[1])
        lib = _lib.load()
        if int(lib.chaorec_mhrec_long_row()) != MHREC_LONG_ROW or int(lib.chaorec_mhrec_chunk()) != MHREC_CHUNK:
            raise RuntimeError("mhrec: the library's long-row threshold / chunk differ from ops_extra's")
        N, E, dev = hg.num_nodes, hg.num_edges, X.device
        X = _vae_f32("mhrec", X.detach().contiguous(), "X")
        ctx.a_shape = tuple(a.shape)
        a = _vae_f32("mhrec", a.detach().contiguous().reshape(-1), "a", (2 * MHREC_DIM,))
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
            if tuple(keep.shape) != (N, MHREC_DIM):
                raise ValueError("mhrec: keep must have X's shape")
        elif training and state is None:
            raise ValueError("mhrec: training without a given mask needs the device step counter")
        Eo = torch.empty((E, MHREC_DIM), dtype=torch.float32, device=dev)
        r = torch.empty(E, dtype=torch.float32, device=dev)
        stat = torch.empty((N, 4), dtype=torch.float32, device=dev)
        out, y = torch.empty_like(X), torch.empty_like(X)
        pacc = torch.empty((hg.n_chunks, MHREC_DIM), dtype=torch.float64, device=dev) if hg.n_long else None
        pz = torch.empty((hg.n_chunks, 2), dtype=torch.float64, device=dev) if hg.n_long else None
        lib.chaorec_mhrec_layer_fwd_f32(*_mhrec_args(hg), _ptr(X), _ptr(a), _ptr(keep), int(seed) & (2**64 - 1), _ptr(state), int(salt),
                                        int(bool(training)), _ptr(Eo), _ptr(r), _ptr(stat), _ptr(out), _ptr(y), _ptr(pacc), _ptr(pz),
                                        _stream())
        ctx.save_for_backward(X, a, Eo, r, stat, out)
        ctx.hg, ctx.draw = hg, (keep, state, int(seed) & (2**64 - 1), int(salt), int(bool(training)))
        ctx.mark_non_differentiable(out)
        return y, out

    @staticmethod
    def backward(ctx, gy, _gout):
        X, a, Eo, r, stat, out = ctx.saved_tensors
        hg = ctx.hg
        keep, state, seed, salt, training = ctx.draw
        N, E, dev = hg.num_nodes, hg.num_edges, X.device
        rb = int(_lib.load().chaorec_mhrec_rows_per_block())
        g = _f32c(gy)
        gm, dX = torch.empty_like(X), torch.empty_like(X)
        tn = torch.empty(N, dtype=torch.float32, device=dev)
        dE = torch.empty_like(Eo)
        pa1 = torch.empty(((N + rb - 1) // rb, MHREC_DIM), dtype=torch.float32, device=dev)
        pa2 = torch.empty(((E + rb - 1) // rb, MHREC_DIM), dtype=torch.float32, device=dev)
        pacc = torch.empty((hg.n_chunks, MHREC_DIM), dtype=torch.float64, device=dev) if hg.n_long else None
        _lib.load().chaorec_mhrec_layer_bwd_f32(*_mhrec_args(hg), _ptr(g), _ptr(X), _ptr(a), _ptr(Eo), _ptr(r), _ptr(stat), _ptr(out),
                                                _ptr(keep), seed, _ptr(state), salt, training, _ptr(gm), _ptr(tn), _ptr(dE), _ptr(dX),
                                                _ptr(pa1), _ptr(pa2), _ptr(pacc), _stream())
        da = torch.cat([col_sum(pa1), col_sum(pa2)]).reshape(ctx.a_shape) if ctx.needs_input_grad[1] else None
        return dX, da, None, None, None, None, None, None


def mhrec_hyper_layer(hg, X, a, keep=None, state=None, seed=0, salt=0, training=True, return_out=False):
    """HypergraphAttentionLayer.forward (Model/MHRec.py:53-89) over hg with the epilogue of Model/MHRec.py:724-726 fused:
    y_n = keep ? 2 (out_n + X_n) : 0.  keep: given flags [N, 64]; None with training: drawn in the launch, keyed (seed,
    state[1], salt, node, column) -- state int64 [2] as ops_extra.step_tick keeps it; None without training: y = out + X.
    Gradients flow to X and a [128, 1].  return_out: also the attention's own output (detached)."""
    y, out = _MHRecHyperLayer.apply(X, a, hg, keep, state, seed, salt, bool(training))
    return (y, out) if return_out else y


def mhrec_hyper_layer_torch(hg, X, a, keep=None, training=True, return_out=False):
    """The same layer in plain torch on hg's arrays (the reference's lines over the ELL table: gathers, a [nnz, 128]
    concatenation, two index_adds), for the model's fused_hyper = False and for measurements.  The two index_adds run in double
    and are rounded once, as the kernels' sums are: in fp32 their atomics add a node's hundreds of terms in another order every
    run, and the modal weights' gradient downstream moved between 0.3 and 0.9 of its bound from run to run."""
    E, k, D = hg.num_edges, hg.k, X.shape[1]
    node = hg.nodes.reshape(-1).to(torch.int64)
    hedge = torch.arange(E, dtype=torch.int64, device=X.device).repeat_interleave(k)
    Ej = X[node].view(E, k, D).sum(1)
    e = torch.matmul(torch.cat([X[node], Ej[hedge]], dim=1), a).squeeze(-1)
    e_exp = torch.exp(e).double()
    sums = torch.zeros(X.size(0), dtype=torch.float64, device=X.device).index_add(0, node, e_exp)
    alpha = e_exp / (sums[node] + 1e-16)
    out = torch.zeros(X.shape, dtype=torch.float64, device=X.device).index_add(0, node, alpha.unsqueeze(-1) * Ej[hedge].double()).to(X.dtype)
    y = out + X
    if keep is not None:
        y = y * (keep.to(y.dtype) * 2.0)
    elif training:
        y = torch.nn.functional.dropout(y, 0.5)
    return (y, out.detach()) if return_out else y
