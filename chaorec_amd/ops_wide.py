"""Rank lists past 64 columns (csrc/topk_wide.hip): the exact scores of a user range staged in HBM (score_rows), the exact
top-k of every staged row (rows_topk_wide), and the range loop over both that ops.score_topk runs for 64 < K <= 1024."""
import os

import torch

from . import _lib
from .ops import _f32c, _need_cuda, _ptr, _stream

__all__ = ["NARROW_K", "WIDE_K", "WIDE_STAGING_BYTES", "check_wide_k", "wide_range_users", "_hist_i32", "score_rows",
           "rows_topk_wide", "score_topk_wide"]

NARROW_K = 64        # kMaxK of csrc/score_topk.hip, the limit of chaorec_macrid_topk_f32: up to here nothing changed
WIDE_K = 1024        # kWideK of csrc/topk_wide.hip, kMetWideK of csrc/metrics.hip
# the staged score block of one user range (the [U, I] matrix never exists whole), like DUALVAE_STAGING_BYTES
WIDE_STAGING_BYTES = int(os.environ.get("CHAOREC_WIDE_STAGING_BYTES", str(512 << 20)))


def check_wide_k(what, K):
    """ValueError naming the limit for a rank-list width no route serves."""
    if int(K) > WIDE_K:
        raise ValueError(f"{what}: K={int(K)} exceeds the widest rank list the kernels select, {WIDE_K}")


def wide_range_users(ld, staging_bytes=None):
    """Users per range such that n * ld * 4 stays under the staging cap (at least one)."""
    cap = WIDE_STAGING_BYTES if staging_bytes is None else int(staging_bytes)
    return max(1, cap // (4 * int(ld)))


def _hist_i32(hist):
    if hist is None:
        return None, None
    rowptr, col = hist
    _need_cuda(rowptr, col)
    if rowptr.dtype != torch.int64 or col.dtype != torch.int32 or not rowptr.is_contiguous() or not col.is_contiguous():
        raise TypeError("score_rows: the history CSR is (rowptr int64, col int32), contiguous")
    return rowptr, col


def score_rows(user_emb, item_emb, hist, mask_value, user_begin, n, out=None, ld=None):
    """scores [n, ld] fp32 of the users user_begin .. user_begin + n against all items (chaorec_score_rows_f32): the values
    ops.score_topk ranks, history entries = mask_value.  out: a staging tensor of at least n * ld floats to write into."""
    _need_cuda(user_emb, item_emb)
    user_emb, item_emb = _f32c(user_emb), _f32c(item_emb)
    U, D = user_emb.shape
    I = item_emb.shape[0]
    ld = I if ld is None else int(ld)
    rowptr, col = _hist_i32(hist)
    if out is None:
        out = torch.empty(int(n) * ld, dtype=torch.float32, device=user_emb.device)
    _need_cuda(out)
    if out.dtype != torch.float32 or not out.is_contiguous():
        raise TypeError("score_rows: out must be a contiguous float32 tensor")
    _lib.load().chaorec_score_rows_f32(_ptr(user_emb), _ptr(item_emb), U, I, D, int(user_begin), int(n), _ptr(rowptr), _ptr(col),
                                       float(mask_value), _ptr(out), ld, out.numel() * 4, _stream())
    return out.view(-1)[:int(n) * ld].view(int(n), ld)


def rows_topk_wide(scores, topk, id_offset=0, n_cols=None, idx=None, val=None):
    """Exact top-k per row for 64 < topk <= min(1024, I), ties to the lowest index -> (int64 [n, topk] ids + id_offset, fp32
    [n, topk]).  scores: 2-D fp32 with unit column stride and any row stride (rows may start at any 4-byte alignment);
    n_cols: rank the first n_cols columns only (a staged block with ld > I).  idx: a contiguous int64 [n, topk] device tensor
    to write the ids to; val: likewise, float32."""
    _need_cuda(scores)
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.stride(1) != 1 or scores.stride(0) < scores.shape[1]:
        raise ValueError("rows_topk: scores must be a 2-D float32 tensor with unit column stride")
    n = scores.shape[0]
    I = scores.shape[1] if n_cols is None else int(n_cols)
    topk = int(topk)
    check_wide_k("rows_topk", topk)
    if not NARROW_K < topk <= I <= scores.shape[1]:
        raise ValueError(f"rows_topk: topk={topk} ({NARROW_K + 1} .. min({WIDE_K}, I={I}))")
    if idx is None:
        idx = torch.empty((n, topk), dtype=torch.int64, device=scores.device)
    elif not idx.is_cuda or idx.dtype != torch.int64 or tuple(idx.shape) != (n, topk) or not idx.is_contiguous():
        raise TypeError("rows_topk: idx must be a contiguous int64 [n, topk] device tensor")
    if val is None:
        val = torch.empty((n, topk), dtype=torch.float32, device=scores.device)
    elif not val.is_cuda or val.dtype != torch.float32 or tuple(val.shape) != (n, topk) or not val.is_contiguous():
        raise TypeError("rows_topk: val must be a contiguous float32 [n, topk] device tensor")
    _lib.load().chaorec_rows_topk_wide_f32(_ptr(scores), n, I, scores.stride(0), topk, int(id_offset), _ptr(idx), _ptr(val), _stream())
    return idx, val


def score_topk_wide(user_emb, item_emb, hist, mask_value, K, id_offset=0, stats=None, idx_out=None, staging_bytes=None):
    """ops.score_topk for 64 < K <= 1024: user ranges of wide_range_users(I) users, each scored into one staging block
    (score_rows) and selected from (rows_topk_wide), one range after the other on the caller's stream.  Returns (idx, val) as
    ops.score_topk does; a pinned-host idx_out is filled by a copy once the last range is through."""
    K = int(K)
    check_wide_k("score_topk", K)
    _need_cuda(user_emb, item_emb)
    user_emb, item_emb = _f32c(user_emb), _f32c(item_emb)
    U = user_emb.shape[0]
    I = item_emb.shape[0]
    dev = user_emb.device
    if K > I:
        raise RuntimeError(f"score_topk: n_items={I} < K={K} (torch.topk would raise)")
    if idx_out is not None and (idx_out.dtype != torch.int64 or tuple(idx_out.shape) != (U, K) or not idx_out.is_contiguous()
                                or not (idx_out.is_cuda or idx_out.is_pinned())):
        raise TypeError("score_topk: idx_out must be a contiguous int64 [n_users, K] device or pinned host tensor")
    idx = idx_out if idx_out is not None and idx_out.is_cuda else torch.empty((U, K), dtype=torch.int64, device=dev)
    val = torch.empty((U, K), dtype=torch.float32, device=dev)
    ld = (I + 3) // 4 * 4        # 16-byte rows: the scoring launch stores four scores at a time
    per = min(max(U, 1), wide_range_users(ld, staging_bytes))
    stage = torch.empty(per * ld, dtype=torch.float32, device=dev)
    for u0 in range(0, U, per):
        n = min(per, U - u0)
        sc = score_rows(user_emb, item_emb, hist, mask_value, u0, n, out=stage, ld=ld)
        rows_topk_wide(sc, K, id_offset, n_cols=I, idx=idx[u0:u0 + n], val=val[u0:u0 + n])
    if idx_out is not None and idx is not idx_out:
        idx_out.copy_(idx, non_blocking=True)
        idx = idx_out
    if stats is not None:
        stats["wide_users"] = U
    return idx, val
