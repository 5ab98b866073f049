"""The user-user co-occurrence graph over csrc/usergraph.hip: DRAGON's user_graph_dict built, sampled and aggregated on the
device; DualGNN's fused node over the same structure; COHESION's over three tables, with a chunked backward."""
import torch

from . import _lib
from .ops import _f32, _f32c, _i32, _need_cuda, _ptr, _stream

__all__ = [
    "USERGRAPH_TOPN", "USERGRAPH_MAX_N", "USERGRAPH_DIMS", "usergraph_max_users", "usergraph_tile_users", "UserGraphStructure",
    "usergraph_build", "usergraph_sample", "_UserGraphAggregate", "usergraph_aggregate", "_DualGNNFuse", "dualgnn_fuse",
    "COHESION_DIM", "COHESION_CHUNK", "RevChunks", "usergraph_rev_chunks", "_CohesionFuse", "cohesion_fuse",
]


USERGRAPH_TOPN = 200         # dualgnn-gen-u-u-matrix.py:92-103 keeps the 200 largest co-occurrence counts of a user
USERGRAPH_MAX_N = 256        # what the build kernel's sorting network holds
USERGRAPH_DIMS = (64, 128)   # the row widths the aggregation kernels are instantiated for


def usergraph_max_users():
    """The largest user count the usergraph entries accept (ids are 32-bit)."""
    return int(_lib.load().chaorec_usergraph_max_users())


def usergraph_tile_users(num_user, tile_users=0):
    """How many user ids one LDS tile of the build covers."""
    return int(_lib.load().chaorec_usergraph_tile_users(int(num_user), int(tile_users)))


class UserGraphStructure:
    """nbr_idx / nbr_cnt int32 [U, N], nbr_len int32 [U] (each user's co-occurring users by count descending, id ascending)
    and, once usergraph_sample() has run, the epoch's buffers: epoch_idx int32 [U, k], epoch_w fp32 [U, k] and the reverse
    structure of the aggregation's backward (rev_ptr int64 [U + 1]; rev_slot int64, rev_u int32, rev_w fp32 [U k]: for every
    user r the slots u k + j that name r, ascending).  The epoch buffers are allocated once per k and rewritten in place
    by every later sample, so a captured step that holds their addresses reads the new epoch's graph at its next replay."""

    def __init__(self, nbr_idx, nbr_cnt, nbr_len):
        U, N = nbr_idx.shape
        self.num_user, self.n = int(U), int(N)
        self.nbr_idx, self.nbr_cnt = _i32("usergraph", nbr_idx, "nbr_idx"), _i32("usergraph", nbr_cnt, "nbr_cnt", (U, N))
        self.nbr_len = _i32("usergraph", nbr_len, "nbr_len", (U,))
        self.k = 0
        self.epoch_idx = self.epoch_w = self.rev_ptr = self.rev_slot = self.rev_u = self.rev_w = self._ids = None
        self.rev_chunks = {}      # chunk -> usergraph_rev_chunks() of the current epoch graph (COHESION's backward)

    @classmethod
    def from_dict(cls, user_graph_dict, num_user, n=USERGRAPH_TOPN, device="cpu"):
        """The reference's user_graph_dict.npy ({user: [[ids], [counts]]}, Model/DRAGON.py:170) in the arrays' form."""
        import numpy as np
        idx, cnt = np.zeros((num_user, n), dtype=np.int32), np.zeros((num_user, n), dtype=np.int32)
        length = np.zeros(num_user, dtype=np.int32)
        for u in range(num_user):
            ids, counts = user_graph_dict[u]
            m = min(len(ids), n)
            idx[u, :m], cnt[u, :m], length[u] = ids[:m], np.asarray(counts[:m]).astype(np.int32), m
        return cls(torch.from_numpy(idx).to(device), torch.from_numpy(cnt).to(device), torch.from_numpy(length).to(device))

    def to(self, device):
        for name in ("nbr_idx", "nbr_cnt", "nbr_len", "epoch_idx", "epoch_w", "rev_ptr", "rev_slot", "rev_u", "rev_w", "_ids"):
            if getattr(self, name) is not None:
                setattr(self, name, getattr(self, name).to(device))
        self.rev_chunks = {}
        return self

    def _epoch_buffers(self, k):
        if self.k != k:
            U, dev = self.num_user, self.nbr_idx.device
            self.k = int(k)
            self.epoch_idx = torch.zeros((U, k), dtype=torch.int32, device=dev)
            self.epoch_w = torch.zeros((U, k), dtype=torch.float32, device=dev)
            self.rev_ptr = torch.zeros(U + 1, dtype=torch.int64, device=dev)
            self.rev_slot = torch.zeros(U * k, dtype=torch.int64, device=dev)
            self.rev_u = torch.zeros(U * k, dtype=torch.int32, device=dev)
            self.rev_w = torch.zeros(U * k, dtype=torch.float32, device=dev)
            self._ids = torch.arange(U + 1, dtype=torch.int64, device=dev)

    def set_epoch(self, epoch_idx, epoch_w):
        """Install a GIVEN epoch graph ([U, k] ids and weights, e.g. the reference's own draw) and index it for the backward."""
        U, k = epoch_idx.shape
        if U != self.num_user or tuple(epoch_w.shape) != (U, k):
            raise ValueError(f"usergraph: epoch graph {tuple(epoch_idx.shape)} / {tuple(epoch_w.shape)} for {self.num_user} users")
        self._epoch_buffers(int(k))
        self.epoch_idx.copy_(epoch_idx)
        self.epoch_w.copy_(epoch_w)
        self.index_epoch()
        self.rev_chunks = {}

    def index_epoch(self):
        """The reverse structure of the current epoch_idx: torch's STABLE sort of the flattened slots by the user they name
        (so a user's slots stay in ascending (u, j)), written into the buffers allocated with the epoch graph."""
        flat = self.epoch_idx.view(-1).to(torch.int64)
        named, perm = torch.sort(flat, stable=True)
        self.rev_slot.copy_(perm)
        self.rev_u.copy_(torch.div(perm, self.k, rounding_mode="floor"))
        self.rev_w.copy_(self.epoch_w.view(-1)[perm])
        self.rev_ptr.copy_(torch.searchsorted(named, self._ids))


def usergraph_build(rowptr, col, num_item, n=USERGRAPH_TOPN, tile_users=0, out=None):
    """The co-occurrence graph of the user-history CSR (rowptr int64 [U + 1], col int32 local item ids without repeats, on
    the device) -> UserGraphStructure with N = n neighbours per user.  `out` = (nbr_idx, nbr_cnt, nbr_len) to fill."""
    _need_cuda(rowptr, col)
    if rowptr.dtype != torch.int64 or not rowptr.is_contiguous() or rowptr.dim() != 1:
        raise ValueError("usergraph: rowptr must be a contiguous int64 vector")
    col = _i32("usergraph", col, "col")
    U, I, dev = int(rowptr.numel() - 1), int(num_item), rowptr.device
    if not 1 <= int(n) <= USERGRAPH_MAX_N:
        raise ValueError(f"usergraph: n = {n}, the build keeps 1 .. {USERGRAPH_MAX_N} neighbours")
    if U < 1 or U > usergraph_max_users() or I < 1:
        raise ValueError(f"usergraph: {U} users, {I} items (at most {usergraph_max_users()} users)")
    # the item-major transpose (item -> ascending holders): a stable sort of the entries by item
    counts = rowptr[1:] - rowptr[:-1]
    rows = torch.repeat_interleave(torch.arange(U, dtype=torch.int32, device=dev), counts)
    col64 = col.to(torch.int64)
    item_users = rows[torch.sort(col64, stable=True)[1]].contiguous()
    item_ptr = torch.zeros(I + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(col64, minlength=I)[:I], 0, out=item_ptr[1:])
    if out is None:
        out = (torch.empty((U, n), dtype=torch.int32, device=dev), torch.empty((U, n), dtype=torch.int32, device=dev),
               torch.empty(U, dtype=torch.int32, device=dev))
    nbr_idx, nbr_cnt = _i32("usergraph", out[0], "nbr_idx", (U, n)), _i32("usergraph", out[1], "nbr_cnt", (U, n))
    nbr_len = _i32("usergraph", out[2], "nbr_len", (U,))
    _need_cuda(nbr_idx, nbr_cnt, nbr_len)
    _lib.load().chaorec_usergraph_build(_ptr(rowptr), _ptr(col), _ptr(item_ptr), _ptr(item_users), U, I, int(n), int(tile_users),
                                        _ptr(nbr_idx), _ptr(nbr_cnt), _ptr(nbr_len), _stream())
    return UserGraphStructure(nbr_idx, nbr_cnt, nbr_len)


def usergraph_sample(s, k, seed, epoch):
    """Model/DRAGON.py:231-270 on the device: fills s.epoch_idx / s.epoch_w [U, k] for (seed, epoch) and re-indexes them."""
    _need_cuda(s.nbr_idx, s.nbr_cnt, s.nbr_len)
    if not 1 <= int(k) <= s.n:
        raise ValueError(f"usergraph: k = {k}, the structure holds {s.n} neighbours per user")
    s._epoch_buffers(int(k))
    _lib.load().chaorec_usergraph_sample(_ptr(s.nbr_idx), _ptr(s.nbr_cnt), _ptr(s.nbr_len), s.num_user, s.n, int(k),
                                         int(seed) & (2**64 - 1), int(epoch) & (2**64 - 1), _ptr(s.epoch_idx), _ptr(s.epoch_w),
                                         _stream())
    s.index_epoch()
    s.rev_chunks = {}
    return s.epoch_idx, s.epoch_w


class _UserGraphAggregate(torch.autograd.Function):
    """(v [U, D], t [U, D], weight_u [U, 2(, 1)]) -> [U, 2 D] (Model/DRAGON.py:289-302): neither user_rep, nor
    features[user_graph] [U, k, 2 D], nor h_u exists in memory, forward or backward."""

    @staticmethod
    def forward(ctx, v, t, weight_u, s):
        _need_cuda(v, t, weight_u, s.epoch_idx)
        if v.dim() != 2 or v.shape[1] not in USERGRAPH_DIMS:
            raise ValueError(f"usergraph: v is {tuple(v.shape)}, the aggregation is built for D in {USERGRAPH_DIMS}")
        U, D = s.num_user, int(v.shape[1])
        v, t = _f32("usergraph", v, "v", (U, D)), _f32("usergraph", t, "t", (U, D))
        weight_u = _f32("usergraph", weight_u, "weight_u")
        if weight_u.numel() != 2 * U or weight_u.shape[0] != U:
            raise ValueError(f"usergraph: weight_u is {tuple(weight_u.shape)}, expected ({U}, 2)")
        if s.k < 1:
            raise ValueError("usergraph: no epoch graph yet (usergraph_sample / set_epoch)")
        out = torch.empty((U, 2 * D), dtype=torch.float32, device=v.device)
        _lib.load().chaorec_usergraph_aggregate_fwd_f32(_ptr(v), _ptr(t), _ptr(weight_u), _ptr(s.epoch_idx), _ptr(s.epoch_w), U, s.k, D,
                                                        _ptr(out), _stream())
        ctx.save_for_backward(v, t, weight_u)
        ctx.s = s
        return out

    @staticmethod
    def backward(ctx, g):
        v, t, weight_u = ctx.saved_tensors
        s, (U, D) = ctx.s, v.shape
        g = _f32c(g)
        dv, dt, dw = torch.empty_like(v), torch.empty_like(t), torch.empty_like(weight_u)
        _lib.load().chaorec_usergraph_aggregate_bwd_f32(_ptr(g), _ptr(v), _ptr(t), _ptr(weight_u), _ptr(s.rev_ptr), _ptr(s.rev_u),
                                                        _ptr(s.rev_w), U, D, _ptr(dv), _ptr(dt), _ptr(dw), _stream())
        return dv, dt, dw, None


def usergraph_aggregate(v, t, weight_u, s):
    """out[u] = x[u] + sum_j s.epoch_w[u, j] x[s.epoch_idx[u, j]], x[r] = (weight_u[r, 0] v[r], weight_u[r, 1] t[r])."""
    return _UserGraphAggregate.apply(v, t, weight_u, s)


class _DualGNNFuse(torch.autograd.Function):
    """(v [N, D], t [N, D], weight_u [U, 2(, 1)]) -> result [N, D] (Model/DualGNN.py:189-239): none of user_rep,
    features[user_graph] [U, k, D], h_u1 or representation exists in memory, forward or backward."""

    @staticmethod
    def forward(ctx, v, t, weight_u, s, num_user):
        _need_cuda(v, t, weight_u, s.epoch_idx)
        if v.dim() != 2 or v.shape[1] not in USERGRAPH_DIMS:
            raise ValueError(f"dualgnn_fuse: v is {tuple(v.shape)}, the kernels are built for D in {USERGRAPH_DIMS}")
        U, (N, D) = int(num_user), (int(v.shape[0]), int(v.shape[1]))
        if U != s.num_user or N < U:
            raise ValueError(f"dualgnn_fuse: {U} users, a table of {N} rows, a user graph of {s.num_user} users")
        v, t = _f32("dualgnn_fuse", v, "v", (N, D)), _f32("dualgnn_fuse", t, "t", (N, D))
        weight_u = _f32("dualgnn_fuse", weight_u, "weight_u")
        if tuple(weight_u.shape) not in ((U, 2), (U, 2, 1)):
            raise ValueError(f"dualgnn_fuse: weight_u is {tuple(weight_u.shape)}, expected ({U}, 2) or ({U}, 2, 1)")
        if s.k < 1:
            raise ValueError("dualgnn_fuse: no epoch graph yet (usergraph_sample / set_epoch)")
        out = torch.empty((N, D), dtype=torch.float32, device=v.device)
        _lib.load().chaorec_dualgnn_fuse_fwd_f32(_ptr(v), _ptr(t), _ptr(weight_u), _ptr(s.epoch_idx), _ptr(s.epoch_w), U, N, s.k, D,
                                                 _ptr(out), _stream())
        ctx.save_for_backward(v, t, weight_u)
        ctx.s, ctx.U = s, U
        return out

    @staticmethod
    def backward(ctx, g):
        v, t, weight_u = ctx.saved_tensors
        s, U, (N, D) = ctx.s, ctx.U, v.shape
        g = _f32c(g)
        dv, dt, dw = torch.empty_like(v), torch.empty_like(t), torch.empty_like(weight_u)   # every element is written
        _lib.load().chaorec_dualgnn_fuse_bwd_f32(_ptr(g), _ptr(v), _ptr(t), _ptr(weight_u), _ptr(s.rev_ptr), _ptr(s.rev_u),
                                                 _ptr(s.rev_w), U, N, D, _ptr(dv), _ptr(dt), _ptr(dw), _stream())
        return dv, dt, dw, None, None


def dualgnn_fuse(v, t, weight_u, s, num_user):
    """result[u] = x[u] + sum_j s.epoch_w[u, j] x[s.epoch_idx[u, j]] with x[r] = weight_u[r, 0] v[r] + weight_u[r, 1] t[r] for
    u < num_user, result[r] = v[r] + t[r] below: DualGNN's whole table from the two modality tables in one launch."""
    return _DualGNNFuse.apply(v, t, weight_u, s, num_user)


COHESION_DIM = 64            # Model/COHESION.py:92 hard-codes dim_latent; the cf_* kernels are instantiated for it alone
COHESION_CHUNK = 64          # entries of a reverse list one lane group sums in the backward


class RevChunks:
    """The reverse lists of an epoch graph cut into chunks of `chunk` entries (0: one chunk per non-empty list):
    chunk_row int32 [n_chunks] (the row a chunk belongs to), chunk_first int64 [n_chunks] (its first entry in rev_u / rev_w),
    row_chunk int64 [U + 1] (row r's chunks are [row_chunk[r], row_chunk[r + 1]), in list order)."""

    def __init__(self, chunk, chunk_row, chunk_first, row_chunk):
        self.chunk, self.n_chunks = int(chunk), int(chunk_row.numel())
        self.chunk_row, self.chunk_first, self.row_chunk = chunk_row, chunk_first, row_chunk


def usergraph_rev_chunks(s, chunk=COHESION_CHUNK):
    """Index the chunks of s.rev_ptr (once per epoch graph; tensor ops and one read of the chunk count) -> RevChunks, kept
    in s.rev_chunks[chunk] until the next usergraph_sample / set_epoch."""
    chunk = int(chunk)
    if chunk < 0 or chunk > 2**31 - 1:
        raise ValueError(f"usergraph: chunk = {chunk} (0 = one chunk per list, else the entries per chunk)")
    if s.k < 1:
        raise ValueError("usergraph: no epoch graph yet (usergraph_sample / set_epoch)")
    U, dev = s.num_user, s.rev_ptr.device
    length = s.rev_ptr[1:] - s.rev_ptr[:-1]
    per_row = torch.div(length + (chunk - 1), chunk, rounding_mode="floor") if chunk > 0 else (length > 0).to(torch.int64)
    row_chunk = torch.zeros(U + 1, dtype=torch.int64, device=dev)
    torch.cumsum(per_row, 0, out=row_chunk[1:])
    n_chunks = int(row_chunk[-1])
    rows = torch.repeat_interleave(torch.arange(U, dtype=torch.int64, device=dev), per_row, output_size=n_chunks)
    within = torch.arange(n_chunks, dtype=torch.int64, device=dev) - row_chunk[rows]
    chunk_first = (s.rev_ptr[rows] + within * chunk).contiguous()
    out = RevChunks(chunk, rows.to(torch.int32).contiguous(), chunk_first, row_chunk)
    s.rev_chunks[chunk] = out
    return out


class _CohesionFuse(torch.autograd.Function):
    """(idr, v, t [N, 64]; h_id, h_v, h_t [I, 64] or None) -> result [N, 192] (Model/COHESION.py:340-359): none of the
    [N, 192] concatenation, user_rep, features[user_graph] [U, k, 192] or h_u exists in memory, forward or backward."""

    @staticmethod
    def forward(ctx, idr, v, t, h_id, h_v, h_t, s, num_user, chunk):
        _need_cuda(idr, v, t, s.epoch_idx)
        D = COHESION_DIM
        if v.dim() != 2 or v.shape[1] != D:
            raise ValueError(f"cohesion_fuse: v is {tuple(v.shape)}, the kernels are built for D = {D}")
        U, N = int(num_user), int(v.shape[0])
        if U != s.num_user or N < U:
            raise ValueError(f"cohesion_fuse: {U} users, a table of {N} rows, a user graph of {s.num_user} users")
        idr, v, t = (_f32("cohesion_fuse", a, n, (N, D)) for a, n in ((idr, "idr"), (v, "v"), (t, "t")))
        hs = (h_id, h_v, h_t)
        if any(h is None for h in hs) != all(h is None for h in hs):
            raise ValueError("cohesion_fuse: h_id, h_v, h_t are given together or not at all")
        has_h = h_id is not None
        if has_h:
            _need_cuda(*hs)
            h_id, h_v, h_t = (_f32("cohesion_fuse", a, n, (N - U, D)) for a, n in zip(hs, ("h_id", "h_v", "h_t")))
        if s.k < 1:
            raise ValueError("cohesion_fuse: no epoch graph yet (usergraph_sample / set_epoch)")
        ctx.chunks = s.rev_chunks.get(int(chunk)) or usergraph_rev_chunks(s, chunk)
        out = torch.empty((N, 3 * D), dtype=torch.float32, device=v.device)
        _lib.load().chaorec_cohesion_fuse_fwd_f32(_ptr(idr), _ptr(v), _ptr(t), _ptr(h_id), _ptr(h_v), _ptr(h_t), _ptr(s.epoch_idx),
                                                  _ptr(s.epoch_w), U, N, s.k, D, _ptr(out), _stream())
        ctx.s, ctx.U, ctx.N, ctx.has_h = s, U, N, has_h
        return out

    @staticmethod
    def backward(ctx, g):
        s, U, N, c, D = ctx.s, ctx.U, ctx.N, ctx.chunks, COHESION_DIM
        g = _f32c(g)
        dev = g.device
        dv, dt = torch.empty((N, D), dtype=torch.float32, device=dev), torch.empty((N, D), dtype=torch.float32, device=dev)
        dh_v = torch.empty((N - U, D), dtype=torch.float32, device=dev) if ctx.has_h else None
        dh_t = torch.empty((N - U, D), dtype=torch.float32, device=dev) if ctx.has_h else None
        part = torch.empty((c.n_chunks, 2 * D), dtype=torch.float32, device=dev)     # every row is written before it is read
        _lib.load().chaorec_cohesion_fuse_bwd_f32(_ptr(g), _ptr(s.rev_ptr), _ptr(s.rev_u), _ptr(s.rev_w), _ptr(c.chunk_row),
                                                  _ptr(c.chunk_first), _ptr(c.row_chunk), c.n_chunks, c.chunk, U, N, D, _ptr(part),
                                                  _ptr(dv), _ptr(dt), _ptr(dh_v), _ptr(dh_t), _stream())
        return None, dv, dt, None, dh_v, dh_t, None, None, None


def cohesion_fuse(idr, v, t, h_id, h_v, h_t, s, num_user, chunk=COHESION_CHUNK):
    """result[u] = x[u] + sum_j s.epoch_w[u, j] x[s.epoch_idx[u, j]] with x[r] = (idr[r] | v[r] | t[r]) for u < num_user,
    result[r] = x[r] + (h_id | h_v | h_t)[r - num_user] below (x[r] when the h tables are None): COHESION's whole [N, 192]
    table in one launch.  idr and h_id receive no gradient (the reference detaches the id third).  The backward sums every
    reverse list in chunks of `chunk` entries (0: unchunked) and adds the partials in chunk order: see the header."""
    return _CohesionFuse.apply(idr, v, t, h_id, h_v, h_t, s, num_user, chunk)
