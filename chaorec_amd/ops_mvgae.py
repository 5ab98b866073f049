"""MVGAE over csrc/mvgae.hip: the conv epilogue and the product-of-experts / KL / BPR tail, each one autograd node."""
import torch

from . import _lib
from .ops import _check_dim, _empty_f32, _f32, _f32c, _need_cuda, _ptr, _stream, col_sum, step_tick

__all__ = [
    "MVGAE_DIM", "MVGAE_VIEWS", "mvgae_check_shape", "mvgae_rows", "mvgae_tick", "_MVGAEConvTail", "mvgae_conv_tail",
    "mvgae_slot_index", "_MVGAETail", "mvgae_tail",
]


MVGAE_DIM = 64               # the row width the mg_* kernels tile
MVGAE_VIEWS = 4              # P (the product of experts), V, T, C


def mvgae_check_shape(D):
    _check_dim("MVGAE", D, MVGAE_DIM)


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
        s, bias = _f32("mvgae", s.contiguous(), "s"), _f32("mvgae", bias, "bias", (MVGAE_DIM,))
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
        tabs = [_f32("mvgae", t.contiguous(), "table", (N, MVGAE_DIM)) for t in tabs]
        users, pos, neg = (t.to(torch.int64).contiguous() for t in (users, pos, neg))
        B, dev = users.numel(), Vm.device
        if pos.numel() != B or neg.numel() != B or B == 0:
            raise ValueError("mvgae: users, pos and neg must be three non-empty id vectors of one length")
        if eps is not None:
            eps = _f32("mvgae", eps, "eps", (MVGAE_VIEWS, N, MVGAE_DIM))
        lib = _lib.load()
        f = _empty_f32(dev)
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
