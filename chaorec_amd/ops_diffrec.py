"""DiffRec over csrc/diffrec.hip: the denoiser's output layer with the importance-weighted x0 loss and the gradient by its
output in one pass, one step of the sampling chain in hidden space, and the plain-torch twins of both (the measurements'
other side)."""
import ctypes

import torch

from . import _lib
from . import ops as _ops
from .ops import _f32, _need_cuda, _ptr, _stream
from .ops_diffmm import _out_layer_backward, _out_layer_buffers

__all__ = [
    "diffrec_check_shape", "diffrec_tiles", "_diffrec_rows16", "diffrec_out_loss_raw", "_DiffRecX0Loss", "diffrec_x0_loss",
    "diffrec_x0_loss_plain", "diffrec_chain_step", "diffrec_chain_step_plain",
]


def diffrec_check_shape(B, I, H):
    """Raises RuntimeError where the tile does not take [B, I] x K = H (H no multiple of 4, a non-positive size): no launch."""
    _lib.load().chaorec_diffrec_check_shape(int(B), int(I), int(H))


def diffrec_tiles():
    """(bm, bn, bk) of the tile kernel."""
    v = [ctypes.c_int32(0) for _ in range(3)]
    _lib.load().chaorec_diffrec_tiles(*(ctypes.byref(x) for x in v))
    return tuple(int(x.value) for x in v)


def _diffrec_rows16(t):
    """A 2-D fp32 operand the tile reads as float4 rows: unit column stride, a row stride that is a multiple of 4 and a
    16-byte aligned base travel in place; anything else is made contiguous."""
    t = _ops._f32rows(t)
    if t.stride(0) % 4 or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def diffrec_out_loss_raw(h, W_out, b_out, bits, w, pt):
    """The forward of diffrec_x0_loss without a tape -> (loss [1], reloss_rows [B] float64 = w_b mean_i err^2, d_out [B, ld]
    with d loss / d out in its first I columns and 0 in the rest)."""
    _need_cuda(h, W_out, b_out, bits, w, pt)
    B, H = h.shape
    I = W_out.shape[0]
    diffrec_check_shape(B, I, H)
    h, W_out = _diffrec_rows16(h), _diffrec_rows16(W_out)
    b_out = _f32("diffrec", b_out, "b_out", (I,))
    w, ld, d_out, part = _out_layer_buffers("diffrec", h, W_out, bits, w, diffrec_tiles()[1])
    if tuple(pt.shape) != (B,):
        raise ValueError("diffrec: pt must be [B]")
    lib, dev = _lib.load(), h.device
    pt = pt.to(torch.float64).contiguous()
    c_row = (w * (2.0 / (float(B) * float(I))) / pt).to(torch.float32)      # formed in double
    reloss = torch.empty(B, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    lib.chaorec_diffrec_out_loss_f32(_ptr(h), h.stride(0), _ptr(W_out), W_out.stride(0), _ptr(b_out), _ptr(bits), _ptr(w), _ptr(pt),
                                     _ptr(c_row), B, I, H, _ptr(d_out), ld, _ptr(part), _ptr(reloss), _ptr(loss), _stream())
    return loss, reloss, d_out


class _DiffRecX0Loss(torch.autograd.Function):
    """(h [B, H], W_out [I, H], b_out [I]) -> loss [1], reloss_rows [B] float64 (Model/DiffRec.py:86-89, :445-461).  Forward: the
    one-pass launch, which leaves d loss / d out.  Backward: ops_diffmm._out_layer_backward, DiffMM's node's as well."""

    @staticmethod
    def forward(ctx, h, W_out, b_out, bits, w, pt):
        loss, reloss, d_out = diffrec_out_loss_raw(h, W_out, b_out, bits, w, pt)
        ctx.save_for_backward(h, W_out, d_out)
        ctx.mark_non_differentiable(reloss)
        return loss, reloss

    @staticmethod
    def backward(ctx, g, _gr):
        return _out_layer_backward(ctx, g) + (None,) * 3


def diffrec_x0_loss(h, W_out, b_out, bits, w, pt):
    """-> (loss [1] = mean_b w_b mse_b / pt_b, reloss_rows [B] float64 = w_b mse_b).  bits: the x0 bit table of diffmm_rows;
    w float64 [B] the SNR weight; pt [B] the importance of each row's timestep (ones under uniform sampling)."""
    return _DiffRecX0Loss.apply(h, W_out, b_out, bits, w, pt)


def diffrec_x0_loss_plain(h, W_out, b_out, x0, w, pt):
    """The reference's lines in plain torch on dense rows x0 [B, I] -> (loss [], reloss_rows [B] float64)."""
    out = torch.nn.functional.linear(h, W_out, b_out)
    reloss = w * ((x0 - out) ** 2).mean(dim=1)
    return (reloss / pt).mean(), reloss


def diffrec_chain_step(z, G, g0, p, e_next, c1, c2):
    """One sampling step in hidden space, one launch -> (p_next, z_next), both [B, N]:
    p_next = c1 (z G^T + g0) + c2 p, z_next = tanh(p_next + e_next).  z [B, K], G [N, K], g0 and e_next [N], p [B, N]."""
    _need_cuda(z, G, g0, p, e_next)
    B, K = z.shape
    N = G.shape[0]
    diffrec_check_shape(B, N, K)
    z, G = _diffrec_rows16(z), _diffrec_rows16(G)
    if G.shape[1] != K:
        raise ValueError("diffrec: G must be [N, K] for z [B, K]")
    g0, e_next = _f32("diffrec", g0, "g0", (N,)), _f32("diffrec", e_next, "e_next", (N,))
    p = _f32("diffrec", p, "p", (B, N))
    p_next = torch.empty((B, N), dtype=torch.float32, device=z.device)
    z_next = torch.empty((B, N), dtype=torch.float32, device=z.device)
    _lib.load().chaorec_diffrec_chain_f32(_ptr(z), z.stride(0), _ptr(G), G.stride(0), _ptr(g0), _ptr(p), N, _ptr(e_next), float(c1),
                                          float(c2), B, N, K, _ptr(p_next), _ptr(z_next), N, _stream())
    return p_next, z_next


def diffrec_chain_step_plain(z, G, g0, p, e_next, c1, c2):
    """diffrec_chain_step in plain torch (any device, any dtype)."""
    p_next = c1 * (z @ G.t() + g0) + c2 * p
    return p_next, torch.tanh(p_next + e_next)
