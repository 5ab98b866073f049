"""The per-entry view generators over one graph.DropoutStructure: AdaGCL (csrc/adagcl.hip), Grade (csrc/grade.hip) and
GraphAug (csrc/graphaug.hip), all three over csrc/edge_mlp.h."""
import torch

from . import _lib
from .ops import _check_dim, _empty_f32, _f32, _f32c, _need_cuda, _ptr, _stream, step_tick

__all__ = [
    "ADAGCL_DIM", "adagcl_check_shape", "adagcl_tick", "_adagcl_parts", "_AdaGCLEdgeGate", "adagcl_edge_gate",
    "adagcl_edge_keep", "GRADE_DIM", "grade_check_shape", "grade_pair_owner", "grade_views", "GRAPHAUG_DIM",
    "graphaug_check_shape", "graphaug_edge_sample", "_GraphAugLSE", "graphaug_lse", "RandEntries", "_graphaug_rand_spmm",
    "_GraphAugRandLayer", "graphaug_rand_layer",
]


# --------------------------------------------------------------------------------------------
# AdaGCL (csrc/adagcl.hip): the per-entry work of its two view generators over one graph.DropoutStructure
# --------------------------------------------------------------------------------------------
ADAGCL_DIM = 64              # the row width the keep kernel tiles


def adagcl_check_shape(D):
    _check_dim("AdaGCL", D, ADAGCL_DIM)


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
        s_nb = _f32("adagcl", s_nb.detach().contiguous(), "s_nb", (N,))
        s_self = _f32("adagcl", s_self.detach().contiguous(), "s_self", (N,))
        b_att = _f32("adagcl", b_att.detach().contiguous().reshape(-1), "b_att", (1,))
        if u is not None:
            u = _f32("adagcl", u, "u", (E,))
        elif training and state is None:
            raise ValueError("adagcl: the training form needs given draws u or a device step counter")
        f = _empty_f32(s_nb.device)
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
        f = _empty_f32(s_nb.device)
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
        z = _f32("adagcl", z.detach().contiguous(), "z", (N, ADAGCL_DIM))
        W1 = _f32("adagcl", W1.detach().contiguous(), "W1", (ADAGCL_DIM, ADAGCL_DIM))
        b1 = _f32("adagcl", b1.detach().contiguous(), "b1", (ADAGCL_DIM,))
        w2 = _f32("adagcl", w2.detach().contiguous().reshape(-1), "w2", (ADAGCL_DIM,))
        b2 = _f32("adagcl", b2.detach().contiguous().reshape(-1), "b2", (1,))
        vals = _f32("adagcl", vals.detach().contiguous(), "vals", (E,))
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
    _check_dim("Grade", D, GRADE_DIM)


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
        z = _f32("grade", z.detach().contiguous(), "z", (G, N, GRADE_DIM))
        W1 = _f32("grade", W1.detach().contiguous().reshape(-1, GRADE_DIM, GRADE_DIM), "W1", (G, GRADE_DIM, GRADE_DIM))
        b1 = _f32("grade", b1.detach().contiguous().reshape(-1, GRADE_DIM), "b1", (G, GRADE_DIM))
        w2 = _f32("grade", w2.detach().contiguous().reshape(-1, GRADE_DIM), "w2", (G, GRADE_DIM))
        b2 = _f32("grade", b2.detach().contiguous().reshape(-1), "b2", (G,))
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
    _check_dim("GraphAug", D, GRAPHAUG_DIM)


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
        P = _f32("graphaug", P.detach().contiguous(), "P", (N, GRAPHAUG_DIM))
        Q = _f32("graphaug", Q.detach().contiguous(), "Q", (N, GRAPHAUG_DIM))
        b1 = _f32("graphaug", b1.detach().contiguous(), "b1", (GRAPHAUG_DIM,))
        w2 = _f32("graphaug", w2.detach().contiguous().reshape(-1), "w2", (GRAPHAUG_DIM,))
        b2 = _f32("graphaug", b2.detach().contiguous().reshape(-1), "b2", (1,))
        if (u1 is None) != (u2 is None):
            raise ValueError("graphaug: give both u1 and u2, or neither")
        if u1 is not None:
            u1, u2 = _f32("graphaug", u1, "u1", (E,)), _f32("graphaug", u2, "u2", (E,))
        elif state is None:
            raise ValueError("graphaug: the sampler needs given draws or a device step counter")
        f = _empty_f32(P.device)
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
        A = _f32("graphaug_lse", A.detach().contiguous(), "A")
        T = _f32("graphaug_lse", T.detach().contiguous(), "T")
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
        z = _f32("graphaug", z.detach().contiguous(), "z", (R.n, GRAPHAUG_DIM))
        x = _f32("graphaug", x.detach().contiguous(), "x", (R.n, GRAPHAUG_DIM))
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
