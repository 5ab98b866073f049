"""LightGODE over csrc/lightgode.hip: the alignment + uniformity loss of a batch as one autograd node, its plain-torch twin
(the measurements' other side, and what other widths run), and the one explicit Euler step of the evaluation's graph ODE on
the SpMM kernel's epilogue."""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib
from .ops import _f32c, _need_cuda, _ptr, _stream, spmm_raw

__all__ = ["lightgode_check_shape", "lightgode_workspace", "_LightGODELoss", "lightgode_loss", "lightgode_loss_plain", "_LightGODEEuler",
           "lightgode_euler"]


def lightgode_check_shape(B, D):
    """Raises RuntimeError for D != 64, B < 2 (the reference's mean over zero pairs is NaN) or B > 8192: no launch."""
    _lib.load().chaorec_lightgode_check_shape(int(B), int(D))


def lightgode_workspace(B, D=64):
    """The floats of the loss launches' workspace for a batch of B."""
    n = ctypes.c_int64(0)
    _lib.load().chaorec_lightgode_workspace(int(B), int(D), ctypes.byref(n))
    return int(n.value)


class _LightGODELoss(torch.autograd.Function):
    """-> (loss 0-dim, parts [4] = (loss, align, unif_u, unif_i)); tab_i=None means "items live in tab_u from row item_offset
    on" (one joined table, one gradient buffer), as in ops._BPR.  The forward leaves d loss / d the gathered rows; the backward
    is the ordered row add."""

    @staticmethod
    def forward(ctx, tab_u, tab_i, users, items, gamma, item_offset):
        _need_cuda(tab_u, tab_i, users, items)
        tab_u = _f32c(tab_u)
        D = tab_u.shape[1]
        B = users.numel()
        lightgode_check_shape(B, D)
        if tuple(users.shape) != (B,) or tuple(items.shape) != (B,):
            raise ValueError("lightgode: users and items must be [B]")
        if tab_i is None:
            U, I = int(item_offset), tab_u.shape[0] - int(item_offset)
            if U <= 0 or I <= 0:
                raise ValueError(f"lightgode: item_offset {item_offset} leaves no users or no items in a table of {tab_u.shape[0]} rows")
            pi = ctypes.c_void_p(tab_u.data_ptr() + U * D * 4)
        else:
            tab_i = _f32c(tab_i)
            if tab_i.shape[1] != D:
                raise ValueError("lightgode: the two tables differ in width")
            U, I = tab_u.shape[0], tab_i.shape[0]
            pi = _ptr(tab_i)
        users, items = users.to(torch.int64).contiguous(), items.to(torch.int64).contiguous()
        dev = tab_u.device
        want_grad = any(ctx.needs_input_grad[:2])
        ws = torch.empty(lightgode_workspace(B, D), dtype=torch.float32, device=dev)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)   # own allocation: its gradient arrives 0-dim
        row_grad = torch.empty((2, B, D), dtype=torch.float32, device=dev) if want_grad else None
        _lib.load().chaorec_lightgode_loss_f32(_ptr(tab_u), pi, U, I, _ptr(users), _ptr(items), B, D, float(gamma), _ptr(ws),
                                               ws.numel(), _ptr(out), _ptr(loss), _ptr(row_grad), _stream())
        if want_grad:
            ctx.save_for_backward(row_grad, users, items)
        ctx.shapes = (tuple(tab_u.shape), None if tab_i is None else tuple(tab_i.shape), U, I)
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)
        return loss, out

    @staticmethod
    def backward(ctx, g_loss, _g_parts):
        if g_loss is None:                       # (grads are not materialised: nothing upstream of the loss)
            return None, None, None, None, None, None
        if g_loss.dtype != torch.float32:
            raise TypeError(f"lightgode: the loss's gradient is {g_loss.dtype}, expected float32")
        row_grad, users, items = ctx.saved_tensors
        shape_u, shape_i, U, I = ctx.shapes
        B, D = users.numel(), shape_u[1]
        g_u = torch.zeros(shape_u, dtype=torch.float32, device=row_grad.device)
        if shape_i is None:
            g_i = None
            pgi = ctypes.c_void_p(g_u.data_ptr() + U * D * 4)
        else:
            g_i = torch.zeros(shape_i, dtype=torch.float32, device=row_grad.device)
            pgi = _ptr(g_i)
        go = g_loss.contiguous()
        _lib.load().chaorec_lightgode_bwd_f32(_ptr(row_grad), _ptr(users), _ptr(items), B, D, U, I, _ptr(go), _ptr(g_u), pgi, _stream())
        return g_u, g_i, None, None, None, None


def lightgode_loss(tab_u, tab_i, users, items, gamma, item_offset=0):
    """-> (loss, parts): loss = mean_b |x_b - y_b|^2 + gamma (unif(x) + unif(y)) / 2 over x = normalize(tab_u[users]),
    y = normalize(tab_i[items]) (LOCAL item ids), unif(z) = log mean_{i<j} exp(-2 |z_i - z_j|^2); parts = (loss, align,
    unif_u, unif_i), not differentiable.  tab_i=None: items are rows item_offset + items of tab_u.  D = 64, 2 <= B <= 8192."""
    return _LightGODELoss.apply(tab_u, tab_i, users, items, gamma, item_offset)


def lightgode_loss_plain(tab_u, tab_i, users, items, gamma, item_offset=0):
    """The reference's lines (Model/LightGODE.py:97-146) in plain torch on the same arguments (any device, dtype and width)."""
    if tab_i is None:
        tab_u, tab_i = tab_u[:item_offset], tab_u[item_offset:]
    x, y = F.normalize(tab_u[users], dim=-1), F.normalize(tab_i[items], dim=-1)
    align = (x - y).norm(p=2, dim=1).pow(2).mean()
    uu, ui = (torch.pdist(z, p=2).pow(2).mul(-2).exp().mean().log() for z in (x, y))
    loss = align + gamma * (uu + ui) / 2
    return loss, torch.stack((loss, align, uu, ui)).detach()


class _LightGODEEuler(torch.autograd.Function):
    """z = x + t (A x + x) = t (A x) + (1 + t) x: one SpMM launch with its epilogue.  A is symmetric, so the backward is the same
    launch on the gradient."""

    @staticmethod
    def forward(ctx, x, csr, t):
        ctx.csr, ctx.t = csr, t
        x = _f32c(x)
        return spmm_raw(csr, x, alpha=t, z=x, beta=1.0 + t)

    @staticmethod
    def backward(ctx, g):
        g = _f32c(g)
        return spmm_raw(ctx.csr, g, alpha=ctx.t, z=g, beta=1.0 + ctx.t), None, None


def lightgode_euler(csr, x, t):
    """One explicit Euler step of dz/dt = A z + x from z(0) = x over [0, t] (torchdiffeq's fixed-grid 'euler' with the two time
    points as its grid): x + t (A x + x), here t (A x) + (1 + t) x -- the reference's order of operations up to rounding.
    csr: a SYMMETRIC graph.CSR (the normalised adjacency); t a python float.  Differentiable by x."""
    _need_cuda(x)
    return _LightGODEEuler.apply(x, csr, float(t))
