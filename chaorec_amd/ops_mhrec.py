"""MHRec over csrc/mhrec.hip: the hypergraph attention layer with its residual / dropout epilogue, one autograd node."""
import torch

from . import _lib
from .ops import _check_dim, _f32, _f32c, _need_cuda, _ptr, _stream, col_sum

__all__ = [
    "MHREC_DIM", "MHREC_LONG_ROW", "MHREC_CHUNK", "mhrec_check_shape", "mhrec_long_row", "HyperGraph", "_mhrec_args",
    "_MHRecHyperLayer", "mhrec_hyper_layer", "mhrec_hyper_layer_torch",
]


MHREC_DIM = 64               # the row width the kernels tile
MHREC_LONG_ROW = 256         # chaorec_mhrec_long_row(): a longer node row is cut into chunks
MHREC_CHUNK = 256            # chaorec_mhrec_chunk(): entries per chunk


def mhrec_check_shape(D):
    _check_dim("MHRec", D, MHREC_DIM)


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
            raise RuntimeError("mhrec: the library's long-row threshold / chunk differ from ops_mhrec's")
        N, E, dev = hg.num_nodes, hg.num_edges, X.device
        X = _f32("mhrec", X.detach().contiguous(), "X")
        ctx.a_shape = tuple(a.shape)
        a = _f32("mhrec", a.detach().contiguous().reshape(-1), "a", (2 * MHREC_DIM,))
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
    state[1], salt, node, column) -- state int64 [2] as ops.step_tick keeps it; None without training: y = out + X.
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
