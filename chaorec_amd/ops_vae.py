"""The autoencoders' wrappers over csrc/multvae.hip, csrc/macridvae.hip and csrc/dualvae.hip (MultVAE, MacridVAE, DualVAE),
the structure the three walk, and rows_topk, the exact per-row top-k of a staged score block."""
import torch

from . import _lib
from .ops import _empty_f32, _f32, _f32c, _need_cuda, _ptr, _stream, col_sum, step_tick
from .ops_dense import gemm_raw

__all__ = [
    "MultVAEStructure", "_range_users", "MULTVAE_LATENT", "multvae_tick", "_multvae_sumsq", "_MultVAEEncode", "multvae_encode",
    "_MultVAEDecode", "multvae_decode", "MACRID_D", "MACRID_K", "MACRID_H", "MACRID_STAGING_BYTES", "macrid_check_shape",
    "macrid_tick", "macrid_normal", "_MacridConcept", "macrid_concept", "_MacridEncode", "macrid_encode", "_MacridSplit",
    "macrid_split", "_MacridMix", "macrid_mix", "macrid_range_users", "macrid_scores", "rows_topk", "macrid_topk", "DUALVAE_K",
    "DUALVAE_A", "DUALVAE_H", "DUALVAE_STAGING_BYTES", "dualvae_check_shape", "dualvae_tick", "_DualVAEEncode",
    "dualvae_encode", "_DualVAEDense", "dualvae_dense", "dualvae_writeback", "dualvae_range_users", "dualvae_scores",
    "_DualVAELinear", "dualvae_linear", "_DualVAELoss", "dualvae_loss",
]


# --------------------------------------------------------------------------------------------
# The autoencoders (csrc/multvae.hip, macridvae.hip, dualvae.hip over csrc/vae_common.h): what the three share
# --------------------------------------------------------------------------------------------
# MultVAEStructure has three users: MultVAE and MacridVAE walk the user-history CSR with it, DualVAE builds one per side
# (rows = that side's samples, columns = the other side's table rows).  It keeps the name of its first user.
class MultVAEStructure:
    """What the autoencoder kernels walk: the user-history CSR (rowptr int64 [U + 1], col int32 local item ids, ascending)
    and its item-major transpose with every entry's place in its user's row (graph.item_major_hist)."""

    def __init__(self, rowptr, col, num_item):
        from .graph import item_major_hist
        self.num_user, self.num_item = int(rowptr.numel() - 1), int(num_item)
        self.rowptr, self.col = rowptr.to(torch.int64).contiguous(), col.to(torch.int32).contiguous()
        self.item_ptr, self.item_users, self.item_pos = item_major_hist(self.rowptr.cpu(), self.col.cpu(), self.num_item)
        self.user_ids = torch.arange(self.num_user + 1, dtype=torch.int64)

    def to(self, device):
        for k in ("rowptr", "col", "item_ptr", "item_users", "item_pos", "user_ids"):
            setattr(self, k, getattr(self, k).to(device))
        return self

    def batch(self, users):
        """users int64 [B] -> (users, slot_ptr [U + 1], perm [B]): user u sits in samples perm[slot_ptr[u] : slot_ptr[u + 1]],
        ascending (a stable sort; capturable: no host decision)."""
        users = users.to(torch.int64).contiguous()
        sorted_u, perm = torch.sort(users, stable=True)
        return users, torch.searchsorted(sorted_u, self.user_ids).contiguous(), perm.contiguous()

    def keep_offsets(self, users):
        """Where each sample's keep flags start when they are GIVEN (sample 0's history row, then sample 1's, ...)."""
        n = self.rowptr[users + 1] - self.rowptr[users]
        return (torch.cumsum(n, 0) - n).contiguous()


def _range_users(staging_bytes, num_item):
    return max(1, staging_bytes // (int(num_item) * 4))


# --------------------------------------------------------------------------------------------
# MultVAE (csrc/multvae.hip): history-row encoder, all-items multinomial likelihood without [B, I]
# --------------------------------------------------------------------------------------------
MULTVAE_LATENT = 64      # p_dims = [64] (Model/MultVAE.py:38): the width the kernels tile


def multvae_tick(state, anneal, cap, total_steps):
    """state[1] = state[0] (the update_count this step reads), state[0] += 1, anneal[0] = min(cap, state[1] / total)."""
    _need_cuda(state, anneal)
    _lib.load().chaorec_multvae_tick(_ptr(state), _ptr(anneal), float(cap), int(total_steps), _stream())


def _multvae_sumsq(tensors, out):
    lib = _lib.load()
    for k, t in enumerate(tensors):
        n_partial = max(1, min(1024, t.numel() // 4096))
        partial = torch.empty(n_partial, dtype=torch.float32, device=t.device)
        lib.chaorec_multvae_sumsq_f32(_ptr(t), t.numel(), _ptr(partial), n_partial, _ptr(out), 1 if k else 0, _stream())


class _MultVAEEncode(torch.autograd.Function):
    """(Wq_t [I, 128], bq [128]) -> z [B, 64], kl [1], sum ||Wq||^2 + ||bq||^2 [1] (Model/MultVAE.py:75-93, :113-114)."""

    @staticmethod
    def forward(ctx, Wq_t, bq, s, batch, state, seed, training, keep_prob, keep, keep_off, eps):
        users, slot_ptr, perm = batch
        _need_cuda(Wq_t, bq, users, s.rowptr, state, keep, keep_off, eps)
        Wq_t, bq = _f32("multvae", Wq_t, "Wq_t"), _f32("multvae", bq, "bq")
        B, dev = users.numel(), Wq_t.device
        if Wq_t.shape != (s.num_item, 2 * MULTVAE_LATENT):
            raise ValueError(f"multvae: Wq_t is {tuple(Wq_t.shape)}, the kernels tile [{s.num_item}, {2 * MULTVAE_LATENT}]")
        if eps is not None:
            eps = _f32("multvae", eps, "eps")
            if eps.shape != (B, MULTVAE_LATENT):
                raise ValueError("multvae: eps must be [B, 64]")
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
        f = _empty_f32(dev)
        h, z, eps_out, klrow, kl, sq = f(B, 2 * MULTVAE_LATENT), f(B, MULTVAE_LATENT), f(B, MULTVAE_LATENT), f(B), f(1), f(1)
        _lib.load().chaorec_multvae_encode_fwd_f32(_ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(Wq_t), _ptr(bq),
                                                   _ptr(keep), _ptr(keep_off), _ptr(eps), _ptr(state), int(seed), int(training),
                                                   float(keep_prob), _ptr(h), _ptr(z), _ptr(eps_out), _ptr(klrow), _ptr(kl),
                                                   _stream())
        _multvae_sumsq((Wq_t, bq), sq)
        ctx.save_for_backward(Wq_t, bq, h, eps_out)
        ctx.s, ctx.batch, ctx.state, ctx.draw = s, batch, state, (int(seed), int(training), float(keep_prob), keep, keep_off)
        ctx.mark_non_differentiable(h, eps_out)
        return z, kl, sq, h, eps_out

    @staticmethod
    def backward(ctx, gz, gkl, gsq, _gh, _ge):
        Wq_t, bq, h, eps = ctx.saved_tensors
        s, (users, slot_ptr, perm) = ctx.s, ctx.batch
        seed, training, keep_prob, keep, keep_off = ctx.draw
        B, dev = users.numel(), Wq_t.device
        n_partial = (B + 63) // 64
        sdh = torch.empty_like(h)
        partial = torch.empty((n_partial, 2 * MULTVAE_LATENT), dtype=torch.float32, device=dev)
        dW, db = torch.empty_like(Wq_t), torch.empty_like(bq)
        _lib.load().chaorec_multvae_encode_bwd_f32(
            _ptr(users), B, s.num_user, _ptr(s.rowptr), s.num_item, _ptr(s.item_ptr), _ptr(s.item_users), _ptr(s.item_pos),
            _ptr(slot_ptr), _ptr(perm), _ptr(Wq_t), _ptr(bq), _ptr(keep), _ptr(keep_off), _ptr(ctx.state), seed, training,
            keep_prob, _ptr(h), _ptr(eps), _ptr(_f32c(gz)), _ptr(_f32c(gkl)), _ptr(_f32c(gsq)), _ptr(sdh), _ptr(partial),
            n_partial, _ptr(dW), _ptr(db), _stream())
        return dW, db, None, None, None, None, None, None, None, None, None


def multvae_encode(Wq_t, bq, s, batch, state, seed, training, keep_prob=0.5, keep=None, keep_off=None, eps=None):
    """-> z [B, 64], kl [1], sum of squares of (Wq_t, bq) [1], h = [mu | logvar] [B, 128], the eps used [B, 64]."""
    return _MultVAEEncode.apply(Wq_t, bq, s, batch, state, seed, bool(training), keep_prob, keep, keep_off, eps)


class _MultVAEDecode(torch.autograd.Function):
    """(z [B, 64], Wp [I, 64], bp [I]) -> neg_ll [1], sum ||Wp||^2 + ||bp||^2 [1], lse [B] (Model/MultVAE.py:98-105,
    :155-156), the logits recomputed tile by tile in the forward and in both backward passes."""

    @staticmethod
    def forward(ctx, z, Wp, bp, s, batch):
        users, slot_ptr, perm = batch
        _need_cuda(z, Wp, bp, users)
        z, Wp, bp = _f32("multvae", z, "z"), _f32("multvae", Wp, "Wp"), _f32("multvae", bp, "bp")
        B, I, dev = users.numel(), s.num_item, z.device
        if Wp.shape != (I, MULTVAE_LATENT) or z.shape != (B, MULTVAE_LATENT) or bp.shape != (I,):
            raise ValueError(f"multvae: decoder shapes z {tuple(z.shape)}, Wp {tuple(Wp.shape)}, bp {tuple(bp.shape)}; "
                             f"the kernels tile a latent width of {MULTVAE_LATENT}")
        lib = _lib.load()
        splits = int(lib.chaorec_multvae_decode_splits(B, I))
        f = _empty_f32(dev)
        pm, ps, lse, lse2, cnt, nll, neg_ll, sq = f(splits, B), f(splits, B), f(B), f(2, B), f(B), f(B), f(1), f(1)
        lib.chaorec_multvae_decode_fwd_f32(_ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(z), _ptr(Wp), _ptr(bp),
                                           I, _ptr(pm), _ptr(ps), splits, _ptr(lse), _ptr(lse2), _ptr(cnt), _ptr(nll), _ptr(neg_ll),
                                           _stream())
        _multvae_sumsq((Wp, bp), sq)
        ctx.save_for_backward(z, Wp, bp, lse2, cnt)
        ctx.s, ctx.batch, ctx.splits = s, batch, splits
        ctx.mark_non_differentiable(lse)
        return neg_ll, sq, lse

    @staticmethod
    def backward(ctx, gnll, gsq, _glse):
        z, Wp, bp, lse2, cnt = ctx.saved_tensors
        s, (users, slot_ptr, perm) = ctx.s, ctx.batch
        B, I, dev = users.numel(), s.num_item, z.device
        dzp = torch.empty((ctx.splits, B, MULTVAE_LATENT), dtype=torch.float32, device=dev)
        dz, dW, db = torch.empty_like(z), torch.empty_like(Wp), torch.empty_like(bp)
        _lib.load().chaorec_multvae_decode_bwd_f32(
            _ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(s.item_ptr), _ptr(s.item_users), _ptr(slot_ptr),
            _ptr(perm), _ptr(z), _ptr(Wp), _ptr(bp), I, _ptr(lse2), _ptr(cnt), _ptr(_f32c(gnll)), _ptr(_f32c(gsq)), _ptr(dzp),
            ctx.splits, _ptr(dz), _ptr(dW), _ptr(db), _stream())
        return dz, dW, db, None, None


def multvae_decode(z, Wp, bp, s, batch):
    """-> neg_ll [1], sum of squares of (Wp, bp) [1], lse [B]."""
    return _MultVAEDecode.apply(z, Wp, bp, s, batch)


# --------------------------------------------------------------------------------------------
# MacridVAE (csrc/macridvae.hip): per-concept history-row encoder, mixture likelihood without [B, I] / [B, K, I]
# --------------------------------------------------------------------------------------------
MACRID_D, MACRID_K, MACRID_H = 64, 10, 600      # dim_E, kfac, hidden width the kernels tile (Model/MacridVAE.py:27-28)
MACRID_STAGING_BYTES = 512 << 20                # CHAOREC_MACRID_STAGING_BYTES: one ranking range's [users, I] fp32 scores


def macrid_check_shape(D, K=MACRID_K, H=MACRID_H):
    if (int(D), int(K), int(H)) != (MACRID_D, MACRID_K, MACRID_H):
        raise ValueError(f"MacridVAE: dim_E={D}, kfac={K}, hidden={H}; the kernels tile dim_E={MACRID_D}, kfac={MACRID_K}, "
                         f"hidden={MACRID_H}")


def macrid_tick(state, anneal, cap, total_steps):
    """state[0] += 1, state[1] = state[0], anneal[0] = min(cap, state[0] / total): incremented BEFORE it is read."""
    _need_cuda(state, anneal)
    _lib.load().chaorec_macrid_tick(_ptr(state), _ptr(anneal), float(cap), int(total_steps), _stream())


def macrid_normal(shape, state, seed, std, device):
    """std * N(0, 1) of `shape` from the counter RNG (seed, state[1], element)."""
    _need_cuda(state)
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _lib.load().chaorec_macrid_normal_f32(_ptr(out), out.numel(), _ptr(state), int(seed), float(std), _stream())
    return out


class _MacridConcept(torch.autograd.Function):
    """(item_embedding [I, D], k_embedding [K, D]) -> items [I, D], cates [I, K] (Model/MacridVAE.py:76-77, :86-94)."""

    @staticmethod
    def forward(ctx, E, Kemb, tau, gumbel, state, seed, training):
        _need_cuda(E, Kemb, gumbel, state)
        E, Kemb = _f32("macrid", E, "item_embedding"), _f32("macrid", Kemb, "k_embedding")
        I, D = E.shape
        K = Kemb.shape[0]
        macrid_check_shape(D, K)
        if gumbel is not None:
            gumbel = _f32("macrid", gumbel, "gumbel")
            if gumbel.shape != (I, K):
                raise ValueError("macrid: gumbel must be [I, K]")
        items, cates = torch.empty_like(E), torch.empty((I, K), dtype=torch.float32, device=E.device)
        _lib.load().chaorec_macrid_concept_fwd_f32(_ptr(E), _ptr(Kemb), I, D, K, float(tau), _ptr(gumbel), _ptr(state), int(seed),
                                                   int(training), _ptr(items), _ptr(cates), _stream())
        ctx.save_for_backward(E, Kemb, cates)
        ctx.tau = float(tau)
        return items, cates

    @staticmethod
    def backward(ctx, d_items, d_cates):
        E, Kemb, cates = ctx.saved_tensors
        I, D = E.shape
        K = Kemb.shape[0]
        n_partial = (I + 63) // 64
        partial = torch.empty((n_partial, K, D), dtype=torch.float32, device=E.device)
        dE, dK = torch.empty_like(E), torch.empty_like(Kemb)
        _lib.load().chaorec_macrid_concept_bwd_f32(_ptr(E), _ptr(Kemb), I, D, K, ctx.tau, _ptr(cates), _ptr(_f32c(d_items)),
                                                   _ptr(_f32c(d_cates)), _ptr(partial), n_partial, _ptr(dE), _ptr(dK), _stream())
        return dE, dK, None, None, None, None, None


def macrid_concept(E, Kemb, tau, state, seed, training, gumbel=None):
    """-> items = normalize(E) [I, D], cates = softmax(items . normalize(Kemb)^T / tau (+ Gumbel noise in training)) [I, K]."""
    return _MacridConcept.apply(E, Kemb, tau, gumbel, state, seed, bool(training))


class _MacridEncode(torch.autograd.Function):
    """(W1_t [I, 600], b1 [600], cates [I, K]) -> a [B, K, 600] (Model/MacridVAE.py:82-83, :101-105 up to the first Linear)."""

    @staticmethod
    def forward(ctx, W1_t, b1, cates, s, batch, state, seed, training, keep_prob, keep, keep_off):
        users, slot_ptr, perm = batch
        _need_cuda(W1_t, b1, cates, users, s.rowptr, state, keep, keep_off)
        W1_t, b1, cates = _f32("macrid", W1_t, "W1_t"), _f32("macrid", b1, "b1"), _f32("macrid", cates, "cates")
        B, dev, K, H = users.numel(), W1_t.device, cates.shape[1], W1_t.shape[1]
        macrid_check_shape(MACRID_D, K, H)
        if W1_t.shape[0] != s.num_item or cates.shape[0] != s.num_item:
            raise ValueError(f"macrid: W1_t {tuple(W1_t.shape)}, cates {tuple(cates.shape)} for {s.num_item} items")
        if keep is not None:
            keep = keep.to(torch.uint8).contiguous()
        a = torch.empty((B, K, H), dtype=torch.float32, device=dev)
        srow = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.load().chaorec_macrid_encode_fwd_f32(_ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(W1_t), _ptr(b1),
                                                  _ptr(cates), K, H, _ptr(keep), _ptr(keep_off), _ptr(state), int(seed), int(training),
                                                  float(keep_prob), _ptr(a), _ptr(srow), _stream())
        ctx.save_for_backward(W1_t, cates, srow)
        ctx.s, ctx.batch, ctx.state, ctx.draw = s, batch, state, (int(seed), int(training), float(keep_prob), keep, keep_off)
        return a

    @staticmethod
    def backward(ctx, da):
        W1_t, cates, srow = ctx.saved_tensors
        s, (users, slot_ptr, perm) = ctx.s, ctx.batch
        seed, training, keep_prob, keep, keep_off = ctx.draw
        B, dev, K, H = users.numel(), W1_t.device, cates.shape[1], W1_t.shape[1]
        n_partial = (B * K + 63) // 64
        partial = torch.empty((n_partial, H), dtype=torch.float32, device=dev)
        dW, db, dc = torch.empty_like(W1_t), torch.empty(H, dtype=torch.float32, device=dev), torch.empty_like(cates)
        _lib.load().chaorec_macrid_encode_bwd_f32(
            B, s.num_item, _ptr(s.item_ptr), _ptr(s.item_users), _ptr(s.item_pos), _ptr(slot_ptr), _ptr(perm), _ptr(W1_t), _ptr(cates),
            K, H, _ptr(keep), _ptr(keep_off), _ptr(ctx.state), seed, training, keep_prob, _ptr(srow), _ptr(_f32c(da)), _ptr(partial),
            n_partial, _ptr(dW), _ptr(db), _ptr(dc), _stream())
        return dW, db, dc, None, None, None, None, None, None, None, None


def macrid_encode(W1_t, b1, cates, s, batch, state, seed, training, keep_prob=0.5, keep=None, keep_off=None):
    """-> a [B, K, 600]: b1 + s_b sum over the kept history entries of cates[i, k] W1_t[i, :]."""
    return _MacridEncode.apply(W1_t, b1, cates, s, batch, state, seed, bool(training), keep_prob, keep, keep_off)


class _MacridSplit(torch.autograd.Function):
    """h [n, 2 D] -> (h[:, :D], h[:, D:]) as contiguous tensors; the backward is one concatenation."""

    @staticmethod
    def forward(ctx, h):
        D = h.shape[1] // 2
        return h[:, :D].contiguous(), h[:, D:].contiguous()

    @staticmethod
    def backward(ctx, g1, g2):
        return torch.cat((g1, g2), 1)


def macrid_split(h):
    return _MacridSplit.apply(h)


class _MacridMix(torch.autograd.Function):
    """(zh [B, K, D], items [I, D], cates [I, K]) -> ce [1], lse [B] (Model/MacridVAE.py:119-126, :150): the logits
    recomputed tile by tile in the forward and in both backward passes."""

    @staticmethod
    def forward(ctx, zh, items, cates, s, batch, tau):
        users, slot_ptr, perm = batch
        _need_cuda(zh, items, cates, users)
        zh, items, cates = _f32("macrid", zh, "zh"), _f32("macrid", items, "items"), _f32("macrid", cates, "cates")
        B, I, dev = users.numel(), s.num_item, zh.device
        K, D = cates.shape[1], items.shape[1]
        macrid_check_shape(D, K)
        if zh.shape != (B, K, D) or items.shape[0] != I or cates.shape[0] != I:
            raise ValueError(f"macrid: zh {tuple(zh.shape)}, items {tuple(items.shape)}, cates {tuple(cates.shape)}")
        lib = _lib.load()
        splits = int(lib.chaorec_macrid_mix_splits(B, I))
        f = _empty_f32(dev)
        ps, lse, coef, nll, ce = f(splits, K, B), f(B), f(B), f(B), f(1)
        lib.chaorec_macrid_mix_fwd_f32(_ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(zh), _ptr(items), _ptr(cates),
                                       I, D, K, float(tau), _ptr(ps), splits, _ptr(lse), _ptr(coef), _ptr(nll), _ptr(ce), _stream())
        ctx.save_for_backward(zh, items, cates, coef)
        ctx.s, ctx.batch, ctx.splits, ctx.tau = s, batch, splits, float(tau)
        ctx.mark_non_differentiable(lse)
        return ce, lse

    @staticmethod
    def backward(ctx, gce, _glse):
        zh, items, cates, coef = ctx.saved_tensors
        s, (users, slot_ptr, perm) = ctx.s, ctx.batch
        B, I, dev = users.numel(), s.num_item, zh.device
        K, D = cates.shape[1], items.shape[1]
        dzp = torch.empty((ctx.splits, B, K, D), dtype=torch.float32, device=dev)
        dz, di, dc = torch.empty_like(zh), torch.empty_like(items), torch.empty_like(cates)
        _lib.load().chaorec_macrid_mix_bwd_f32(
            _ptr(users), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(s.item_ptr), _ptr(s.item_users), _ptr(slot_ptr), _ptr(perm),
            _ptr(zh), _ptr(items), _ptr(cates), I, D, K, ctx.tau, _ptr(coef), _ptr(_f32c(gce)), _ptr(dzp), ctx.splits, _ptr(dz),
            _ptr(di), _ptr(dc), _stream())
        return dz, di, dc, None, None, None


def macrid_mix(zh, items, cates, s, batch, tau):
    """-> ce [1] = mean_b (n_b log sum_i p_bi - sum_{i in hist} log p_bi), lse [B]."""
    return _MacridMix.apply(zh, items, cates, s, batch, tau)


def macrid_range_users(num_item):
    """How many users one ranking range may stage under the cap."""
    return _range_users(MACRID_STAGING_BYTES, num_item)


def macrid_scores(zh, items, cates, tau, user_begin, hist, mask_value, out=None):
    """log p_ui of the users user_begin .. user_begin + n (zh [n, K, D]) -> [n, I] fp32, their history entries = mask_value."""
    _need_cuda(zh, items, cates, hist[0], hist[1])
    zh, items, cates = _f32("macrid", zh, "zh"), _f32("macrid", items, "items"), _f32("macrid", cates, "cates")
    n, K, D = zh.shape
    I = items.shape[0]
    macrid_check_shape(D, K)
    if n > macrid_range_users(I):
        raise ValueError(f"macrid: {n} users x {I} items exceed the staging cap of {MACRID_STAGING_BYTES} bytes; rank in ranges")
    if hist[0].dtype != torch.int64 or hist[1].dtype != torch.int64:
        raise ValueError("macrid: the history CSR must be int64")
    if out is None:
        out = torch.empty((n, I), dtype=torch.float32, device=zh.device)
    _lib.load().chaorec_macrid_scores_f32(_ptr(zh), n, _ptr(items), _ptr(cates), I, D, K, float(tau), int(user_begin), _ptr(hist[0]),
                                          _ptr(hist[1]), float(mask_value), _ptr(out), out.numel() * 4, _stream())
    return out


def rows_topk(scores, topk, id_offset=0):
    """Exact top-k per row of scores [n, I], ties to the lowest index -> (int64 [n, topk] ids + id_offset, fp32 [n, topk]).
    The export and the messages keep the name of the first user (MacridVAE's ranking); DualVAE's ranking and DiffMM's graph
    rebuild call it too.  64 < topk <= min(1024, I): chaorec_rows_topk_wide_f32 (ops_wide.rows_topk_wide), same order."""
    _need_cuda(scores)
    if int(topk) > 64:
        from .ops_wide import rows_topk_wide
        return rows_topk_wide(scores, topk, id_offset)
    scores = _f32("macrid", scores, "scores")
    n, I = scores.shape
    if not 1 <= int(topk) <= min(64, I):
        raise ValueError(f"macrid: topk={topk} (1 .. min(64, I={I}))")
    idx = torch.empty((n, int(topk)), dtype=torch.int64, device=scores.device)
    val = torch.empty((n, int(topk)), dtype=torch.float32, device=scores.device)
    _lib.load().chaorec_macrid_topk_f32(_ptr(scores), n, I, int(topk), int(id_offset), _ptr(idx), _ptr(val), _stream())
    return idx, val


macrid_topk = rows_topk      # the name existing callers know


# --------------------------------------------------------------------------------------------
# DualVAE (csrc/dualvae.hip): two-sided aspect encoder, Poisson likelihood and neighbourhood term without [B, U] / [B, I]
# --------------------------------------------------------------------------------------------
DUALVAE_K, DUALVAE_A, DUALVAE_H = 25, 5, 20     # latent width, aspects, hidden width the kernels tile (Model/DualVAE.py:37-49)
DUALVAE_STAGING_BYTES = 512 << 20               # CHAOREC_DUALVAE_STAGING_BYTES: one ranking range's [users, I] fp32 scores


def dualvae_check_shape(k, a=DUALVAE_A, hidden=DUALVAE_H):
    if (int(k), int(a), int(hidden)) != (DUALVAE_K, DUALVAE_A, DUALVAE_H):
        raise ValueError(f"DualVAE: k={k}, a={a}, hidden={hidden}; the kernels tile k={DUALVAE_K}, a={DUALVAE_A}, "
                         f"hidden={DUALVAE_H}")


def dualvae_tick(state):
    step_tick(state, "chaorec_dualvae_tick")


class _DualVAEEncode(torch.autograd.Function):
    """(We_t [N, 20], bias [20], w [N, 5]) -> pre [B, 5, 20] = bias + sum over the sample's row of w[n, a] We_t[n, :]."""

    @staticmethod
    def forward(ctx, We_t, bias, w, s, batch):
        ids, slot_ptr, perm = batch
        _need_cuda(We_t, bias, w, ids, s.rowptr)
        N = s.num_item
        We_t, bias = _f32("dualvae", We_t, "We_t", (N, DUALVAE_H)), _f32("dualvae", bias, "bias", (DUALVAE_H,))
        w = _f32("dualvae", w, "w", (N, DUALVAE_A))
        B = ids.numel()
        pre = torch.empty((B, DUALVAE_A, DUALVAE_H), dtype=torch.float32, device=We_t.device)
        _lib.load().chaorec_dualvae_encode_fwd_f32(_ptr(ids), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), N, _ptr(We_t), _ptr(bias),
                                                   _ptr(w), _ptr(pre), _stream())
        ctx.save_for_backward(We_t, w)
        ctx.s, ctx.batch = s, batch
        return pre

    @staticmethod
    def backward(ctx, dpre):
        We_t, w = ctx.saved_tensors
        s, (ids, slot_ptr, perm) = ctx.s, ctx.batch
        B, N = ids.numel(), s.num_item
        dpre = _f32c(dpre)
        dW, dw = torch.empty_like(We_t), torch.empty_like(w)
        _lib.load().chaorec_dualvae_encode_bwd_f32(B, N, _ptr(s.item_ptr), _ptr(s.item_users), _ptr(slot_ptr), _ptr(perm), _ptr(We_t),
                                                   _ptr(w), _ptr(dpre), _ptr(dW), _ptr(dw), _stream())
        db = col_sum(dpre.view(B * DUALVAE_A, DUALVAE_H))      # (a fixed-order sum over the B * 5 rows)
        return dW, db, dw, None, None


def dualvae_encode(We_t, bias, w, s, batch):
    """-> pre [B, 5, 20]; s: the MultVAEStructure of the SAMPLE side (rows = samples, columns = table rows)."""
    return _DualVAEEncode.apply(We_t, bias, w, s, batch)


class _DualVAEDense(torch.autograd.Function):
    """(z [B, 5, 25], zh [B, 5, 20], th [N, 5, 20], w [N, 5]; table [N, 5, 25] without gradient) -> sum_p [B], xlog [B],
    nei [B, 5, 25]: the tiles s_bna recomputed in the forward and in both backward passes."""

    @staticmethod
    def forward(ctx, z, zh, th, w, table, s, batch):
        ids, slot_ptr, perm = batch
        _need_cuda(z, zh, th, w, table, ids)
        B, N, dev = ids.numel(), s.num_item, z.device
        z, zh = _f32("dualvae", z, "z", (B, DUALVAE_A, DUALVAE_K)), _f32("dualvae", zh, "zh", (B, DUALVAE_A, DUALVAE_H))
        th, w = _f32("dualvae", th, "th", (N, DUALVAE_A, DUALVAE_H)), _f32("dualvae", w, "w", (N, DUALVAE_A))
        table = _f32("dualvae", table, "table", (N, DUALVAE_A, DUALVAE_K))
        lib = _lib.load()
        splits = int(lib.chaorec_dualvae_splits(B, N))
        f = _empty_f32(dev)
        psum, pnei = f(splits, DUALVAE_A, B), f(splits, B, DUALVAE_A, DUALVAE_K)
        sum_p, xlog, nei = f(B), f(B), f(B, DUALVAE_A, DUALVAE_K)
        lib.chaorec_dualvae_dense_fwd_f32(_ptr(ids), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(z), _ptr(zh), _ptr(table), _ptr(th),
                                          _ptr(w), N, _ptr(psum), _ptr(pnei), splits, _ptr(sum_p), _ptr(xlog), _ptr(nei), _stream())
        ctx.save_for_backward(z, zh, th, w, table)
        ctx.s, ctx.batch, ctx.splits = s, batch, splits
        return sum_p, xlog, nei

    @staticmethod
    def backward(ctx, g1, g2, gN):
        z, zh, th, w, table = ctx.saved_tensors
        s, (ids, slot_ptr, perm) = ctx.s, ctx.batch
        B, N, dev = ids.numel(), s.num_item, z.device
        f = _empty_f32(dev)
        dzp, dzhp = f(ctx.splits, B, DUALVAE_A, DUALVAE_K), f(ctx.splits, B, DUALVAE_A, DUALVAE_H)
        dz, dzh, dth, dw = torch.empty_like(z), torch.empty_like(zh), torch.empty_like(th), torch.empty_like(w)
        _lib.load().chaorec_dualvae_dense_bwd_f32(
            _ptr(ids), B, s.num_user, _ptr(s.rowptr), _ptr(s.col), _ptr(s.item_ptr), _ptr(s.item_users), _ptr(slot_ptr), _ptr(perm),
            _ptr(z), _ptr(zh), _ptr(table), _ptr(th), _ptr(w), N, _ptr(_f32c(g1)), _ptr(_f32c(g2)), _ptr(_f32c(gN)), _ptr(dzp),
            _ptr(dzhp), ctx.splits, _ptr(dz), _ptr(dzh), _ptr(dth), _ptr(dw), _stream())
        return dz, dzh, dth, dw, None, None, None


def dualvae_dense(z, zh, th, w, table, s, batch):
    """-> sum_p [B] = sum_n p_bn, xlog [B] = sum_{n in row(b)} log(p_bn + 1e-10), nei [B, 5, 25].  `table` must stay as it
    is until the backward has run (the caller passes a snapshot where the table is written in between)."""
    return _DualVAEDense.apply(z, zh, th, w, table, s, batch)


def dualvae_writeback(batch, num_rows, z, mu, table, mu_table):
    """table[ids] = z, mu_table[ids] = mu in place; where an id repeats in the batch the highest position wins."""
    ids, slot_ptr, perm = batch
    _need_cuda(ids, z, mu, table, mu_table)
    B = ids.numel()
    z, mu = _f32("dualvae", z, "z", (B, DUALVAE_A, DUALVAE_K)), _f32("dualvae", mu, "mu", (B, DUALVAE_A, DUALVAE_K))
    _f32("dualvae", table, "table", (num_rows, DUALVAE_A, DUALVAE_K))
    _f32("dualvae", mu_table, "mu_table", (num_rows, DUALVAE_A, DUALVAE_K))
    _lib.load().chaorec_dualvae_writeback_f32(_ptr(ids), B, int(num_rows), _ptr(slot_ptr), _ptr(perm), _ptr(z), _ptr(mu), _ptr(table),
                                              _ptr(mu_table), _stream())


def dualvae_range_users(num_item):
    """How many users one ranking range may stage under the cap."""
    return _range_users(DUALVAE_STAGING_BYTES, num_item)


def dualvae_scores(z, zh, table, th, w, user_begin, hist, mask_value, out=None):
    """sum_a w[i, a] sigmoid(z_ua . table_ia + tanh(zh_ua . th_ia)) of the users user_begin .. user_begin + n -> [n, I] fp32,
    their history entries = mask_value."""
    _need_cuda(z, zh, table, th, w, hist[0], hist[1])
    n, I = z.shape[0], table.shape[0]
    z, zh = _f32("dualvae", z, "z", (n, DUALVAE_A, DUALVAE_K)), _f32("dualvae", zh, "zh", (n, DUALVAE_A, DUALVAE_H))
    table, th = _f32("dualvae", table, "table", (I, DUALVAE_A, DUALVAE_K)), _f32("dualvae", th, "th", (I, DUALVAE_A, DUALVAE_H))
    w = _f32("dualvae", w, "w", (I, DUALVAE_A))
    if n > dualvae_range_users(I):
        raise ValueError(f"dualvae: {n} users x {I} items exceed the staging cap of {DUALVAE_STAGING_BYTES} bytes; rank in ranges")
    if hist[0].dtype != torch.int64 or hist[1].dtype != torch.int64:
        raise ValueError("dualvae: the history CSR must be int64")
    if out is None:
        out = torch.empty((n, I), dtype=torch.float32, device=z.device)
    _lib.load().chaorec_dualvae_scores_f32(_ptr(z), _ptr(zh), n, _ptr(table), _ptr(th), _ptr(w), I, int(user_begin), _ptr(hist[0]),
                                           _ptr(hist[1]), float(mask_value), _ptr(out), out.numel() * 4, _stream())
    return out


class _DualVAELinear(torch.autograd.Function):
    """y = x W^T + b for the small Linears (W [M, N], M <= 32, N <= 31): the forward and the input gradient are the f32
    GEMM's, the weight and bias gradients are summed in double over the rows and rounded once."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _need_cuda(x, weight, bias)
        x = _f32c(x)
        y = gemm_raw(x, weight, transB=True, bias=bias)
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = _f32c(gy)
        R, (M, N) = x.shape[0], weight.shape
        lib = _lib.load()
        nbytes = lib.chaorec_dualvae_linear_bwd_workspace_bytes(R, M)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
        gw, gb = torch.empty_like(weight), torch.empty(M, dtype=torch.float32, device=x.device)
        lib.chaorec_dualvae_linear_bwd_f32(_ptr(gy), _ptr(x), R, M, N, _ptr(gw), _ptr(gb), _ptr(ws), nbytes, _stream())
        gx = gemm_raw(gy, weight) if ctx.needs_input_grad[0] else None
        return gx, gw, gb


def dualvae_linear(x, weight, bias):
    """nn.Linear for x [R, N] and a small weight [M, N] (see _DualVAELinear)."""
    return _DualVAELinear.apply(x, weight.contiguous(), bias)


class _DualVAELoss(torch.autograd.Function):
    """(mu, std_pre [B * 5, 25], xlog [B], sum_p [B], cl []) -> [3] = (kl_weight kl - ll + ssl_reg cl, kl, ll) from double sums,
    each rounded once; std = sigmoid(std_pre), the KL's elements are evaluated in double.  The gradient of element 0 only."""

    @staticmethod
    def forward(ctx, mu, std_pre, xlog, sum_p, cl, kl_weight, ssl_reg):
        _need_cuda(mu, std_pre, xlog, sum_p, cl)
        mu, std_pre, xlog, sum_p, cl = _f32c(mu), _f32c(std_pre), _f32c(xlog), _f32c(sum_p), _f32c(cl)
        B = xlog.numel()
        if mu.shape != std_pre.shape or mu.numel() != B * DUALVAE_A * DUALVAE_K or sum_p.numel() != B:
            raise ValueError(f"dualvae: mu {tuple(mu.shape)}, std_pre {tuple(std_pre.shape)} for {B} samples")
        out = torch.empty(3, dtype=torch.float32, device=xlog.device)
        ws = torch.empty(64, dtype=torch.float64, device=xlog.device)
        _lib.load().chaorec_dualvae_loss_f32(_ptr(mu), _ptr(std_pre), mu.numel(), _ptr(xlog), _ptr(sum_p), B, _ptr(cl), float(kl_weight),
                                             float(ssl_reg), _ptr(out), _ptr(ws), ws.numel() * 8, _stream())
        ctx.save_for_backward(mu, std_pre)
        ctx.B, ctx.c = B, (float(kl_weight), float(ssl_reg))
        return out

    @staticmethod
    def backward(ctx, g):
        mu, std_pre = ctx.saved_tensors
        g0 = g[0]
        gB = (g0 / ctx.B).expand(ctx.B)
        gk = g0 * (ctx.c[0] / (DUALVAE_A * ctx.B))
        std = torch.sigmoid(std_pre)
        # d/d mu = mu;  d/d std_pre of -0.5 (2 log std - std^2) = -(1 - std)(1 - std^2)
        return gk * mu, gk * ((std - 1.0) * (1.0 - std * std)), -gB, gB, g0 * ctx.c[1], None, None


def dualvae_loss(mu, std_pre, xlog, sum_p, cl, kl_weight, ssl_reg):
    """-> [3]: one side's loss (Model/DualVAE.py:274), kl and ll."""
    return _DualVAELoss.apply(mu, std_pre, xlog, sum_p, cl, kl_weight, ssl_reg)
