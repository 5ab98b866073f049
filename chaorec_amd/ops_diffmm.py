"""DiffMM over csrc/diffmm.hip: the noised history rows in one launch, the denoiser's output layer with both losses and the
gradient by its output in one pass."""
import ctypes

import torch

from . import _lib
from . import ops as _ops
from .ops import _f32, _f32c, _need_cuda, _ptr, _stream, col_sum
from .ops_dense import gemm_nn_bf16x3, gemm_raw, gemm_tn_bf16x3

__all__ = [
    "DIFFMM_D", "diffmm_check_shape", "diffmm_tiles", "diffmm_rows_per_block", "diffmm_ld", "diffmm_rows", "diffmm_rows_noised", "_diffmm_big",
    "_diffmm_rows", "_out_layer_buffers", "_out_layer_backward", "diffmm_out_loss_raw", "_DiffMMDenoiseLoss", "diffmm_denoise_loss",
]


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


def _diffmm_rows(name, noised, users, rowptr, col, num_item, a_row, s_row, noise, keep, seed, step, salt, plain):
    """The body of diffmm_rows and (noised: no keep flags, no plain rows, the other export) diffmm_rows_noised -> (x [B, ld], bits)."""
    _need_cuda(users, rowptr, col, a_row, s_row, noise, keep)
    users = users.to(torch.int64).contiguous()
    B, I, U = users.numel(), int(num_item), rowptr.numel() - 1
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32:
        raise TypeError(f"{name}: rowptr must be int64 and col int32")
    if plain:
        noise = keep = None
    else:
        a_row, s_row = _f32("diffmm", a_row, "a_row", (B,)), _f32("diffmm", s_row, "s_row", (B,))
        if noise is not None:
            noise = _f32("diffmm", noise, "noise", (B, I))
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
            if tuple(keep.shape) != (B, I):
                raise ValueError("diffmm: keep must be [B, I]")
    ld = diffmm_ld(I)
    x = torch.empty((B, ld), dtype=torch.float32, device=users.device)
    bits = torch.empty((B, (I + 31) // 32), dtype=torch.int32, device=users.device)
    head = (_ptr(users), B, U, _ptr(rowptr), _ptr(col), I, ld, _ptr(a_row), _ptr(s_row), _ptr(noise))
    tail = (_ptr(x), _ptr(bits), _stream())
    if noised:
        _lib.load().chaorec_diffmm_rows_noised_f32(*head, int(seed), int(step), int(salt), *tail)
    else:
        _lib.load().chaorec_diffmm_rows_f32(*head, _ptr(keep), int(seed), int(step), int(salt), int(bool(plain)), *tail)
    return x, bits


def diffmm_rows(users, rowptr, col, num_item, a_row=None, s_row=None, noise=None, keep=None, seed=0, step=0, salt=0, plain=False):
    """users int64 [B] -> (x_in fp32 [B, I], a view of a [B, ld] buffer whose pad columns are 0; bits uint32-as-int32
    [B, ceil(I / 32)]).  plain: the multi-hot rows themselves.  Otherwise x_in = dropout_0.5(a x0 + s n) with n and the keep
    flags given ([B, I]) or drawn from the counter RNG keyed (seed, step, salt, user, item)."""
    x, bits = _diffmm_rows("diffmm_rows", False, users, rowptr, col, num_item, a_row, s_row, noise, keep, seed, step, salt, plain)
    return x[:, :int(num_item)], bits


def diffmm_rows_noised(users, rowptr, col, num_item, a_row, s_row, noise=None, seed=0, step=0, salt=0):
    """users int64 [B] -> x_t fp32 [B, I] = a x0 + s n from the history CSR, no input dropout (csrc/diffmm.hip's rows launch
    through chaorec_diffmm_rows_noised_f32).  n: noise [B, I] or, None, the counter RNG keyed (seed, step, 2 salt, user, item)."""
    x, _ = _diffmm_rows("diffmm_rows_noised", True, users, rowptr, col, num_item, a_row, s_row, noise, None, seed, step, salt, False)
    return x[:, :int(num_item)]


def _diffmm_big(rows):
    """The split-bf16 GEMMs read strided operands in place and pay from a few hundred rows on (ops_dense._linear_fwd_raw)."""
    return _ops.LINEAR_FORWARD == "bf16x3" and rows >= 256


def _out_layer_buffers(name, h, W_out, bits, w, bn):
    """The checks both one-pass output layers make of W_out [I, H], the bit table and the weight, and what both launches
    write -> (w contiguous, ld, d_out [B, ld], part [B, item tiles of bn]).  name: the caller's prefix in the messages."""
    (B, H), I = h.shape, W_out.shape[0]
    if W_out.shape[1] != H or tuple(bits.shape) != (B, (I + 31) // 32) or bits.dtype != torch.int32 or not bits.is_contiguous():
        raise ValueError(f"{name}: W_out must be [I, H] and bits int32 [B, ceil(I / 32)]")
    if w.dtype != torch.float64 or tuple(w.shape) != (B,):
        raise ValueError(f"{name}: the weight is float64 [B] (SNR works on float64 tables)")
    ld = diffmm_ld(I)
    d_out = torch.empty((B, ld), dtype=torch.float32, device=h.device)
    part = torch.empty((B, (I + bn - 1) // bn), dtype=torch.float32, device=h.device)
    return w.contiguous(), ld, d_out, part


def _out_layer_backward(ctx, g):
    """The backward both one-pass nodes share, from saved (h, W_out, d_out [B, ld]) -> (dh, dW_out, db_out): dW_out =
    d_out^T (g h), dh = g (d_out W_out), db_out = g colsum(d_out); g is folded into the [B, H] operands, d_out is not passed
    over again."""
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
    return dh, dW, db


def diffmm_out_loss_raw(h, W_out, b_out, bits, x0E, F, w, e_loss):
    """The forward of diffmm_denoise_loss without a tape -> (loss [1], diff_rows [B] float64, gc_rows [B], d_out [B, ld] with
    d loss / d out in its first I columns and 0 in the rest, r [B, 64])."""
    _need_cuda(h, W_out, b_out, bits, x0E, F, w)
    B, H = h.shape
    I = W_out.shape[0]
    h, W_out = _ops._f32rows(h), _ops._f32rows(W_out)
    b_out, F = _f32("diffmm", b_out, "b_out", (I,)), _f32("diffmm", F, "F", (I, DIFFMM_D))
    x0E = _f32("diffmm", x0E, "x0E", (B, DIFFMM_D))
    w, ld, d_out, part = _out_layer_buffers("diffmm", h, W_out, bits, w, diffmm_tiles()[1])
    diffmm_check_shape(B, I, H)
    lib, dev = _lib.load(), h.device
    M = gemm_raw(W_out, F, transA=True)                                     # [H, 64]
    r = gemm_raw(h, M)                                                      # [B, 64]
    r = (r + gemm_raw(b_out.reshape(1, I), F) - x0E).contiguous()
    c_row = (w * (2.0 / (float(B) * float(I)))).to(torch.float32)           # formed in double
    kf = 2.0 * float(e_loss) / (float(B) * DIFFMM_D)
    diff_rows = torch.empty(B, dtype=torch.float64, device=dev)
    gc_rows, loss = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
    lib.chaorec_diffmm_out_loss_f32(_ptr(h), h.stride(0), _ptr(W_out), W_out.stride(0), _ptr(b_out), _ptr(bits), _ptr(r), _ptr(F),
                                    _ptr(w), _ptr(c_row), kf, float(e_loss), B, I, H, _ptr(d_out), ld, _ptr(part),
                                    _ptr(diff_rows), _ptr(gc_rows), _ptr(loss), _stream())
    return loss, diff_rows, gc_rows, d_out, r


class _DiffMMDenoiseLoss(torch.autograd.Function):
    """(h [B, H], W_out [I, H], b_out [I]) -> loss [1], diff_rows [B] float64, gc_rows [B] (Model/DiffMM.py:468-471,
    :640-658).  Forward: M = W_out^T F, r = h M + b_out F - x0 E (three small GEMMs), then the one-pass launch, which leaves
    d loss / d out.  Backward: _out_layer_backward."""

    @staticmethod
    def forward(ctx, h, W_out, b_out, bits, x0E, F, w, e_loss):
        loss, diff_rows, gc_rows, d_out, _ = diffmm_out_loss_raw(h, W_out, b_out, bits, x0E, F, w, e_loss)
        ctx.save_for_backward(h, W_out, d_out)
        ctx.mark_non_differentiable(diff_rows, gc_rows)
        return loss, diff_rows, gc_rows

    @staticmethod
    def backward(ctx, g, _gd, _gg):
        return _out_layer_backward(ctx, g) + (None,) * 5


def diffmm_denoise_loss(h, W_out, b_out, bits, x0E, F, w, e_loss):
    """-> (loss [1] = mean_b w_b mse_b + e_loss mean_b gc_b, diff_rows [B] float64, gc_rows [B]).  bits: the x0 bit table of
    diffmm_rows; x0E [B, 64] = the batch's history-row sums of the item embeddings; F [I, 64] the modality's projected
    features; w float64 [B] the SNR weight.  x0E and F carry no gradient (the reference detaches them)."""
    return _DiffMMDenoiseLoss.apply(h, W_out, b_out, bits, x0E.detach(), F.detach(), w, float(e_loss))
