"""BSPM over csrc/bspm.hip: a tile of users scored through the item-item filter -- the IDL projection, the sparse seed, the
Euler steps on the SpMM and the last step fused with the history mask and the transposed store."""
import torch

from . import _lib
from .ops import _f32, _i32, _need_cuda, _ptr, _stream, _typed, spmm_raw

__all__ = [
    "BSPM_MAX_TILE", "BSPM_MAX_FACTORS", "bspm_check_shape", "bspm_long_row", "bspm_step_sizes", "BSPMFilter", "BSPMTile", "_tile_args",
    "bspm_project", "bspm_seed", "bspm_last_step", "bspm_idl", "bspm_scores", "bspm_scores_plain",
]


BSPM_MAX_TILE = 1024         # users per tile: the SpMM's widest feature width (the middle Euler steps run at D = B)
BSPM_MAX_FACTORS = 128       # m = factor_dim / 2


def bspm_check_shape(I, B, m):
    """chaorec_bspm_check_shape's rules, as ValueErrors: B a multiple of 4 in [4, 1024], m a multiple of 4 in [4, 128]."""
    I, B, m = int(I), int(B), int(m)
    if I < 1:
        raise ValueError(f"BSPM: num_item={I}")
    if B < 4 or B > BSPM_MAX_TILE or B % 4:
        raise ValueError(f"BSPM: B={B}; the kernels tile a multiple of 4 in [4, {BSPM_MAX_TILE}]")
    if m < 4 or m > BSPM_MAX_FACTORS or m % 4:
        raise ValueError(f"BSPM: m={m}; the kernels tile a multiple of 4 in [4, {BSPM_MAX_FACTORS}]")
    _lib.load().chaorec_bspm_check_shape(I, B, m)


def bspm_long_row():
    """The row length of P past which a last-step workgroup shares the row between its four waves (the library's value)."""
    return int(_lib.load().chaorec_bspm_long_row())


def bspm_step_sizes(K_s, T_s):
    """The K_s Euler steps over sharpening_times = linspace(0, T_s, K_s + 1).float() (Model/BSPM.py:58): each the fp32
    difference of two fp32 times, as the fixed-grid solver forms it."""
    t = torch.linspace(0, T_s, int(K_s) + 1).float()
    return [float(x) for x in (t[1:] - t[:-1]).tolist()]


class BSPMFilter:
    """What the model builds once: P = Rn^T Rn as a graph.CSR [I, I], F = D_I Vi and Gt = (Vi^T D_I^-1)^T, both fp32 [I, m]."""

    def __init__(self, P, F, Gt):
        I = P.n_rows
        if P.n_cols != I or F.dim() != 2 or F.shape[0] != I or tuple(Gt.shape) != tuple(F.shape):
            raise ValueError(f"BSPM: P is {P.n_rows} x {P.n_cols}, F {tuple(F.shape)}, Gt {tuple(Gt.shape)}")
        self.P, self.num_item, self.m = P, I, int(F.shape[1])
        self.F, self.Gt = _f32("BSPM", F, "F"), _f32("BSPM", Gt, "Gt")


class BSPMTile:
    """The history rows of a list of users (int64 ids, any order, duplicates allowed: slot s is ids[s]) out of the normalised
    history CSR (rowptr int64 [U + 1], col int32 local item ids, val fp32 = Rn's entries), in the two layouts the kernels read:
    slot-major -- x_ptr int64 [B + 1], x_item int32, x_val -- for the projection, and item-major -- xt_ptr int64 [I + 1],
    xt_slot int32 ascending inside an item, xt_val: a stable sort of the (slot, item, val) triples by item -- for the seed and
    the mask.  B = width, default the count rounded up to a multiple of 4; slots past the ids are empty.  Tensor operations on
    the ids' device."""

    def __init__(self, rowptr, col, val, num_item, ids, width=None):
        ids = torch.as_tensor(ids)
        if ids.dim() != 1 or ids.dtype != torch.int64 or ids.numel() < 1:
            raise ValueError("BSPM: the user ids must be a non-empty int64 vector")
        dev, n, I = ids.device, int(ids.numel()), int(num_item)
        B = max(4, (n + 3) // 4 * 4) if width is None else int(width)
        if B < n or B % 4 or B > BSPM_MAX_TILE:
            raise ValueError(f"BSPM: B={B}; the kernels tile a multiple of 4 in [4, {BSPM_MAX_TILE}] (and {n} users were given)")
        beg = rowptr[ids]
        cnt = rowptr[ids + 1] - beg
        x_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        torch.cumsum(cnt, 0, out=x_ptr[1:n + 1])
        x_ptr[n + 1:] = x_ptr[n]
        slot = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), cnt)
        pos = torch.arange(slot.numel(), dtype=torch.int64, device=dev) - x_ptr[slot] + beg[slot]
        item = col[pos].to(torch.int64)
        order = torch.sort(item, stable=True)[1]
        self.n, self.B, self.num_item, self.nnz = n, B, I, int(slot.numel())
        self.x_ptr, self.x_item, self.x_val = x_ptr, item.to(torch.int32).contiguous(), val[pos].contiguous()
        self.xt_item = item[order].contiguous()                    # (the plain composition's index; the kernels read xt_ptr)
        self.xt_ptr = torch.searchsorted(self.xt_item, torch.arange(I + 1, dtype=torch.int64, device=dev)).contiguous()
        self.xt_slot, self.xt_val = slot[order].to(torch.int32).contiguous(), self.x_val[order].contiguous()


def _tile_args(op, tile, I):
    if tile.num_item != I:
        raise ValueError(f"{op}: the tile was built for {tile.num_item} items, the filter has {I}")
    _need_cuda(tile.x_ptr, tile.xt_ptr)
    _typed(op, tile.xt_ptr, "xt_ptr", torch.int64, (I + 1,))
    _i32(op, tile.xt_slot, "xt_slot", (tile.nnz,))
    _f32(op, tile.xt_val, "xt_val", (tile.nnz,))


def bspm_project(tile, F, out=None):
    """Z [B, m] = X F for the tile's rows X of Rn: one owner wave per slot, the history entries in CSR order."""
    _need_cuda(F, tile.x_ptr, out)
    I, m = F.shape
    bspm_check_shape(I, tile.B, m)
    F = _f32("bspm_project", F, "F")
    _typed("bspm_project", tile.x_ptr, "x_ptr", torch.int64, (tile.B + 1,))
    _i32("bspm_project", tile.x_item, "x_item", (tile.nnz,))
    _f32("bspm_project", tile.x_val, "x_val", (tile.nnz,))
    Z = torch.empty((tile.B, m), dtype=torch.float32, device=F.device) if out is None else _f32("bspm_project", out, "out", (tile.B, m))
    _lib.load().chaorec_bspm_project_f32(_ptr(tile.x_ptr), _ptr(tile.x_item), _ptr(tile.x_val), tile.nnz, _ptr(F), I, tile.B, m, _ptr(Z),
                                         _stream())
    return Z


def bspm_seed(P, tile, beta=0.0, idlT=None, out=None):
    """Y0t [I, B] = beta idlT + P Xt with Xt walked through its stored entries only; idlT [I, B] may be None when beta is 0."""
    I = P.n_rows
    _need_cuda(P.rowptr, idlT, out)
    bspm_check_shape(I, tile.B, 4)
    _tile_args("bspm_seed", tile, I)
    if idlT is None and float(beta) != 0.0:
        raise ValueError(f"bspm_seed: idl_beta={beta} without idlT")
    if idlT is not None:
        idlT = _f32("bspm_seed", idlT, "idlT", (I, tile.B))
    Y = torch.empty((I, tile.B), dtype=torch.float32, device=P.val.device) if out is None else _f32("bspm_seed", out, "out", (I, tile.B))
    _lib.load().chaorec_bspm_seed_f32(_ptr(P.rowptr), _ptr(P.col), _ptr(P.val), P.nnz, I, _ptr(tile.xt_ptr), _ptr(tile.xt_slot),
                                      _ptr(tile.xt_val), tile.nnz, tile.B, float(beta), _ptr(idlT), _ptr(Y), _stream())
    return Y


def bspm_last_step(P, Yt, h, tile=None, mask_value=1e-6, out=None):
    """scores [B, I] = (Yt - h P Yt)^T with the SpMM epilogue's roundings, the tile's history entries set to mask_value (tile
    None: unmasked), one launch.  h = 0: the masked transpose of Yt, bit for bit."""
    I = P.n_rows
    _need_cuda(P.rowptr, Yt, out)
    if Yt.dim() != 2:
        raise ValueError(f"bspm_last_step: Yt is {tuple(Yt.shape)}, expected ({I}, B)")
    B = int(Yt.shape[1])
    bspm_check_shape(I, B, 4)
    Yt = _f32("bspm_last_step", Yt, "Yt", (I, B))
    if tile is not None:
        _tile_args("bspm_last_step", tile, I)
        if tile.B != B:
            raise ValueError(f"bspm_last_step: the tile has {tile.B} slots, Yt {B} columns")
    scores = torch.empty((B, I), dtype=torch.float32, device=Yt.device) if out is None else _f32("bspm_last_step", out, "out", (B, I))
    _lib.load().chaorec_bspm_last_step_f32(_ptr(P.rowptr), _ptr(P.col), _ptr(P.val), P.nnz, I, _ptr(Yt), B, float(h),
                                           _ptr(tile.xt_ptr if tile is not None else None),
                                           _ptr(tile.xt_slot if tile is not None else None), tile.nnz if tile is not None else 0,
                                           float(mask_value), _ptr(scores), _stream())
    return scores


def bspm_idl(filt, Z):
    """idlT [I, B] = G^T Z^T, the dense [I, m] x [m, B] product of the IDL term (plumbing)."""
    return torch.mm(filt.Gt, Z.t()).contiguous()


def bspm_scores(filt, tile, K_s, T_s, idl_beta, mask_value=1e-6, out=None):
    """Model/BSPM.py:133-181 for a tile, item columns only -> scores [B, I]: project + seed, K_s - 1 Euler steps on the SpMM
    (alpha = -h, beta = 1: y + h * (-(P y)) rounding for rounding), the last step with the mask and the transposed store.
    mask_value None: unmasked (getUsersRating)."""
    hs = bspm_step_sizes(K_s, T_s)
    idlT = bspm_idl(filt, bspm_project(tile, filt.F)) if float(idl_beta) != 0.0 else None
    Yt = bspm_seed(filt.P, tile, idl_beta, idlT)
    for h in hs[:-1]:
        Yt = spmm_raw(filt.P, Yt, alpha=-h, z=Yt, beta=1.0)
    return bspm_last_step(filt.P, Yt, hs[-1], tile if mask_value is not None else None, 0.0 if mask_value is None else mask_value, out)


def bspm_scores_plain(filt, tile, K_s, T_s, idl_beta, mask_value=1e-6, out=None):
    """The same scores from launches that need nothing of csrc/bspm.hip: a dense Xt through the SpMM for the blur, K_s SpMM
    steps, a transposing copy and an indexed mask write.  The baseline the fused route is measured against and its cross-check
    -- a second route the caller asks for by name, never a fallback."""
    I, B, dev = filt.num_item, tile.B, filt.F.device
    _need_cuda(filt.F, tile.x_ptr)
    bspm_check_shape(I, B, filt.m)
    slot = tile.xt_slot.to(torch.int64)
    Xt = torch.zeros((I, B), dtype=torch.float32, device=dev)
    Xt[tile.xt_item, slot] = tile.xt_val
    Yt = spmm_raw(filt.P, Xt)
    if float(idl_beta) != 0.0:
        Z = torch.mm(Xt.t(), filt.F)
        Yt = bspm_idl(filt, Z).mul_(float(idl_beta)).add_(Yt)
    for h in bspm_step_sizes(K_s, T_s):
        Yt = spmm_raw(filt.P, Yt, alpha=-h, z=Yt, beta=1.0)
    scores = torch.empty((B, I), dtype=torch.float32, device=dev) if out is None else _f32("bspm_scores_plain", out, "out", (B, I))
    scores.copy_(Yt.t())
    if mask_value is not None:
        scores[slot, tile.xt_item] = float(mask_value)
    return scores
