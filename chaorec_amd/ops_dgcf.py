"""DGCF over csrc/dgcf.hip: intent-weighted propagation with routing, distance correlation."""
import torch

from . import _lib
from .ops import _f32c, _need_cuda, _ptr, _stream

__all__ = [
    "dgcf_check_shape", "dgcf_softmax", "dgcf_propagate_raw", "dgcf_p_schedule", "dgcf_forward_raw", "_DGCFForward",
    "dgcf_forward", "_DGCFCor", "dgcf_cor_loss",
]


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
