"""CF_Diff over csrc/cfdiff.hip: the 4-head, width-4 attention core of the denoiser as one forward and one backward node that
never form an [L, L] array, the plain composition of the same function (the CPU path, the measurements' other side and the
route for an L above the kernels' maximum), and the flags of a device-drawn step as bytes."""
import torch

from . import _lib
from .ops import _f32, _need_cuda, _ptr, _stream

__all__ = [
    "CFDIFF_HEADS", "CFDIFF_WIDTH", "cfdiff_max_len", "cfdiff_check_shape", "_cfdiff_operands", "_cfdiff_draw_args", "_cfdiff_forward", "cfdiff_attention_raw", "_CFDiffAttention",
    "cfdiff_attention", "cfdiff_attention_plain", "cfdiff_keep",
]

CFDIFF_HEADS = 4
CFDIFF_WIDTH = 16            # d_model: 4 heads of 4


def cfdiff_max_len():
    """The longest token sequence of the fused launches: 64 KiB of LDS per workgroup / 48 bytes per token."""
    return int(_lib.load().chaorec_cfdiff_max_len())


def cfdiff_check_shape(B, L):
    """chaorec_cfdiff_check_shape's rules, as ValueErrors (no launch)."""
    B, L, top = int(B), int(L), cfdiff_max_len()
    if L < 1 or L > top:
        raise ValueError(f"cfdiff: L={L}; the fused attention stages its tokens in LDS: 1 .. {top} (cfdiff_attention_plain has no limit)")
    if B < 1 or B > 1 << 28:
        raise ValueError(f"cfdiff: B={B}")
    _lib.load().chaorec_cfdiff_check_shape(B, L)


def _cfdiff_operands(what, q, *rest):
    if q.dim() != 3 or q.shape[2] != CFDIFF_WIDTH:
        raise ValueError(f"cfdiff: {what} must be [B, L, {CFDIFF_WIDTH}], got {tuple(q.shape)}")
    B, L = int(q.shape[0]), int(q.shape[1])
    cfdiff_check_shape(B, L)
    return (B, L) + tuple(_f32("cfdiff", t.contiguous(), what, (B, L, CFDIFF_WIDTH)) for t in (q,) + rest)


def _cfdiff_draw_args(B, L, training, keep, state, dev):
    if not training:
        return None, None
    if keep is not None:
        keep = keep.to(device=dev, dtype=torch.uint8).contiguous()
        if tuple(keep.shape) != (B, CFDIFF_HEADS, L, L):
            raise ValueError(f"cfdiff: keep must be [B, {CFDIFF_HEADS}, L, L], got {tuple(keep.shape)}")
        return keep, None
    if state is None or state.dtype != torch.int64 or state.numel() != 2 or not state.is_cuda:
        raise ValueError("cfdiff: device draws need state int64 [2] on the device (ops.step_tick)")
    return None, state


def _cfdiff_forward(q, k, v, training, seed, state, salt, keep, b0):
    """The forward launch -> (out, lse, the operands and draw arguments as it prepared them: q, k, v, keep, state)."""
    B, L, q, k, v = _cfdiff_operands("q, k, v", q, k, v)
    _need_cuda(q, k, v)
    keep, state = _cfdiff_draw_args(B, L, training, keep, state, q.device)
    out = torch.empty_like(q)
    lse = torch.empty((B, CFDIFF_HEADS, L), dtype=torch.float32, device=q.device)
    _lib.load().chaorec_cfdiff_attn_fwd_f32(_ptr(q), _ptr(k), _ptr(v), B, L, int(bool(training)), _ptr(keep), int(seed), _ptr(state),
                                            int(salt), int(b0), _ptr(out), _ptr(lse), _stream())
    return out, lse, (q, k, v, keep, state)


def cfdiff_attention_raw(q, k, v, training, seed, state, salt, keep=None, b0=0):
    """The forward launch without a tape -> (out [B, L, 16], lse [B, 4, L])."""
    return _cfdiff_forward(q, k, v, training, seed, state, salt, keep, b0)[:2]


class _CFDiffAttention(torch.autograd.Function):
    """(q, k, v) [B, L, 16] -> out [B, L, 16]: per head softmax(<q, k> / 2) with a rate-1/2 dropout on the probabilities, times
    v (F.multi_head_attention_forward between its in- and out-projections).  The backward redraws the forward's flags from
    (seed, state[1], salt, b0): state must not be ticked between the two."""

    @staticmethod
    def forward(ctx, q, k, v, training, seed, state, salt, keep, b0):
        out, lse, (q, k, v, keep, state) = _cfdiff_forward(q, k, v, training, seed, state, salt, keep, b0)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.draws = (int(bool(training)), keep, int(seed), state, int(salt), int(b0))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        training, keep, seed, state, salt, b0 = ctx.draws
        B, L = out.shape[:2]
        dout = _f32("cfdiff", dout.contiguous(), "dout", (B, L, CFDIFF_WIDTH))
        dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
        rnorm = torch.empty_like(lse)
        _lib.load().chaorec_cfdiff_attn_bwd_f32(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), _ptr(dout), B, L, training, _ptr(keep),
                                                seed, _ptr(state), salt, b0, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(rnorm), _stream())
        return dq, dk, dv, None, None, None, None, None, None


def cfdiff_attention(q, k, v, training, seed, state, salt, keep=None, b0=0):
    """out [B, L, 16] = (keep ? 2 P : 0) V per head, P = softmax_j(<q_i, k_j> / 2); training False: P V, no draws.  keep: given
    flags uint8 [B, 4, L, L]; None: drawn in the launch, keyed (seed, state[1], salt, b0 + b, head, query, key) -- state int64
    [2] as ops.step_tick keeps it.  L above cfdiff_max_len() raises: cfdiff_attention_plain is the route for it."""
    return _CFDiffAttention.apply(q, k, v, bool(training), seed, state, salt, keep, b0)


def cfdiff_keep(B, L, seed, state, salt, b0=0):
    """The flags cfdiff_attention(..., keep=None) draws for (seed, state[1], salt, b0): uint8 [B, 4, L, L]."""
    cfdiff_check_shape(B, L)
    _need_cuda(state)
    keep = torch.empty((int(B), CFDIFF_HEADS, int(L), int(L)), dtype=torch.uint8, device=state.device)
    _lib.load().chaorec_cfdiff_attn_keep_u8(int(B), int(L), int(seed), _ptr(state), int(salt), int(b0), _ptr(keep), _stream())
    return keep


def cfdiff_attention_plain(q, k, v, training, seed=0, state=None, salt=0, keep=None, b0=0):
    """The same function as torch operations on any device and dtype, materialising P [B, 4, L, L].  training with keep None:
    on the device the flags of the fused launch (cfdiff_keep; state given and L within its range), else torch's own generator."""
    B, L, E = q.shape
    H, W = CFDIFF_HEADS, E // CFDIFF_HEADS

    def heads(t):
        return t.reshape(B, t.shape[1], H, W).transpose(1, 2)

    P = torch.softmax(torch.matmul(heads(q), heads(k).transpose(2, 3)) * 0.5, dim=-1)
    if training:
        if keep is None:
            drawn = q.is_cuda and state is not None and L <= cfdiff_max_len()
            keep = cfdiff_keep(B, L, seed, state, salt, b0) if drawn else torch.rand(P.shape, device=P.device) < 0.5
        P = P * (keep.to(device=P.device, dtype=P.dtype) * 2.0)
    return torch.matmul(P, heads(v)).transpose(1, 2).reshape(B, L, E)
