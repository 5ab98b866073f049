"""The kernels of the sparse.mm model family: csrc/graph_dropout.hip (edge dropout, weighted sampling without replacement),
csrc/rowops.hip (per-entry dots, NGCF's layer, LayerGCN's row re-weighting) and the dynamic-value products over csrc/spmm.hip."""
import torch

from . import _lib
from . import ops as _ops
from .ops import _f32c, _need_cuda, _ptr, _stream
from .ops_dense import gemm_raw

__all__ = [
    "_SpMMAdd", "spmm_add", "edge_dropout_norm", "edge_dot_raw", "_EdgeDot", "edge_dot", "_SpMMValues", "spmm_values",
    "_NGCFLayer", "ngcf_layer", "weighted_sample_keep", "weighted_sample_keys", "_RowCosineScale", "row_cosine_scale",
]


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
