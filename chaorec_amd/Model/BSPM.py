"""BSPM with the reference's surface (Model/BSPM.py:19-203), compute on HIP kernels (csrc/bspm.hip).

The one model that trains nothing: it builds an item-item filter once, pushes every user's history row through a blur
(one product with P = L^T L), an ideal low-pass term (the top singular vectors of L) and K_s Euler steps of the sharpening
ODE y' = -y P, and ranks.  Same constructor arguments and attribute names (solver_*, K_idl, T_idl, K_b, T_b, K_s, T_s,
final_sharpening, sharpening_off, t_point_combination, factor_dim, idl_beta, the three time grids); K_b, T_b and
blurring_times are stored and, as in the reference, never read.  Only the reference's flag values are built: any other raises
NotImplementedError naming the flag.

What changed underneath (DESIGN: "BSPM").  The reference forms a dense (U + I) x (U + I) adjacency on the host for every
batch of users and runs a dense ODE state against the whole sparse filter.  P is block-diagonal, the users' rows X are zero on
user columns and gene_ranklist reads item columns only, so everything here lives in item space: Rn = D_U R D_I, P = Rn^T Rn
[I, I] as a CSR, and the 2m vectors of sparsesvd(L, 2m) as the m = factor_dim / 2 top right singular vectors of Rn (each
squared singular value of L appears once per block), which is why an odd factor_dim is refused.  A tile of at most 1024 users is
kept transposed, [I, B], and scored by ops.bspm_scores.

Departures from the reference, all deliberate:
  * getUsersRating returns [len, I] -- item columns only -- where the reference returns [len, U + I]; its user columns hold
    the IDL term's spill and nobody reads them (gene_ranklist slices them away, :188).
  * gene_ranklist takes no score matrix: like the other models' here it scores ranges of users itself, the [U, I] matrix
    never exists whole.  The history mask is the VALUE 1e-6 (:193), not minus infinity: most scores are negative, so history
    items do rank above them, and that stays.
  * the mask is taken from the training edges' history (the rows of X); the reference takes it from user_item_dict, which
    holds the same pairs -- the constructor checks that and refuses a dictionary that differs.
  * the truncated SVD comes from scipy.sparse.linalg.svds with a fixed start vector (the reference's sparsesvd is not
    installable here); only the projector Vi Vi^T is defined by the model, never Vi itself.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import graph, ops, ranking

_DENSE_SVD_CELLS = 1 << 22      # a [U, I] matrix this small is decomposed densely (svds needs k < min(U, I) anyway)


def _degrees(u, i, num_user, num_item):
    """(deg + 1e-7)^-1/2 of both sides in float64 (Model/BSPM.py:87-91) over the distinct pairs."""
    du = np.bincount(u, minlength=num_user).astype(np.float64) + 1e-7
    di = np.bincount(i, minlength=num_item).astype(np.float64) + 1e-7
    return np.power(du, -0.5), np.power(di, -0.5)


def _item_filter(u, i, val64, num_user, num_item):
    """P_II = Rn^T Rn in float64, rounded to fp32 once (:106, :114) -> (rowptr int64, col int32 ascending, val fp32).  scipy
    where present, torch's sparse product on the host otherwise."""
    try:
        import scipy.sparse as sp
    except ImportError:
        sp = None
    if sp is not None:
        Rn = sp.csr_matrix((val64, (u, i)), shape=(num_user, num_item))
        P = (Rn.T @ Rn).tocsr()
        P.sort_indices()
        return (torch.from_numpy(P.indptr.astype(np.int64)), torch.from_numpy(P.indices.astype(np.int32)),
                torch.from_numpy(P.data.astype(np.float32)))
    idx = torch.from_numpy(np.stack([u, i]))
    Rn = torch.sparse_coo_tensor(idx, torch.from_numpy(val64), (num_user, num_item)).coalesce()
    P = torch.sparse.mm(Rn.t().coalesce(), Rn).coalesce()
    row, col = P.indices()
    rowptr = torch.zeros(num_item + 1, dtype=torch.int64)
    torch.cumsum(torch.bincount(row, minlength=num_item), 0, out=rowptr[1:])
    return rowptr, col.to(torch.int32).contiguous(), P.values().to(torch.float32).contiguous()


def _right_singular_vectors(u, i, val64, num_user, num_item, m):
    """The top m right singular vectors of Rn, [I, m] float64."""
    if m >= min(num_user, num_item) - 1 or num_user * num_item <= _DENSE_SVD_CELLS:
        Rn = np.zeros((num_user, num_item))
        Rn[u, i] = val64
        if m > min(num_user, num_item):
            raise ValueError(f"BSPM: factor_dim={2 * m} asks for {m} singular vectors of a {num_user} x {num_item} matrix")
        return np.linalg.svd(Rn, full_matrices=False)[2][:m].T.copy()
    try:
        import scipy.sparse as sp
        from scipy.sparse.linalg import svds
    except ImportError as e:
        raise ImportError("BSPM: the truncated SVD needs scipy.sparse.linalg.svds; without scipy pass the item factors "
                          "yourself, BSPM(..., factors=<[num_item, factor_dim / 2] right singular vectors>)") from e
    Rn = sp.csr_matrix((val64, (u, i)), shape=(num_user, num_item))
    v0 = np.random.RandomState(20241008).standard_normal(min(num_user, num_item))    # fixed: two constructions agree
    return svds(Rn, k=m, v0=v0)[2].T.copy()


class BSPM(nn.Module):
    def __init__(self, num_user, num_item, edge_index, user_item_dict, K_s, T_s, K_b, T_b, idl_beta, device, factor_dim=256,
                 factors=None, fused=True):
        super(BSPM, self).__init__()
        self.ua_embedding = None
        self.ia_embedding = None
        self.num_user = num_user
        self.num_item = num_item
        self.user_item_dict = user_item_dict
        self.device = device

        self.solver_idl = 'euler'
        self.solver_blr = 'euler'
        self.solver_shr = 'euler'
        self.K_idl = 1
        self.T_idl = 1
        self.K_b = K_b
        self.T_b = T_b
        self.K_s = K_s
        self.T_s = T_s
        self.final_sharpening = True
        self.sharpening_off = False
        self.t_point_combination = False
        self.factor_dim = int(factor_dim)
        self.idl_beta = idl_beta
        self.fused = bool(fused)
        if self.factor_dim % 2:
            raise ValueError(f"BSPM: factor_dim={factor_dim} is odd; the singular vectors of the bipartite adjacency come in "
                             "pairs, one per side, and an odd count cuts a pair")
        m = self.factor_dim // 2
        if int(K_s) < 1:
            raise ValueError(f"BSPM: K_s={K_s}")
        ops.bspm_check_shape(num_item, 4, m)

        self.idl_times = torch.linspace(0, self.T_idl, self.K_idl + 1).float().to(device)
        self.blurring_times = torch.linspace(0, self.T_b, self.K_b + 1).float().to(device)
        self.sharpening_times = torch.linspace(0, self.T_s, self.K_s + 1).float().to(device)

        e = torch.as_tensor(edge_index)
        rowptr, col = graph.user_hist_csr_from_edges(e.cpu().numpy(), num_user)         # the distinct pairs, items ascending
        mask_ptr, mask_col = graph.user_hist_csr(user_item_dict, num_user)
        if not (torch.equal(rowptr, mask_ptr) and torch.equal(col, mask_col)):
            raise ValueError("BSPM: user_item_dict and edge_index hold different pairs; the history mask is taken from the edges")
        i = col.numpy().astype(np.int64)
        u = np.repeat(np.arange(num_user, dtype=np.int64), np.diff(rowptr.numpy()))
        du, di = _degrees(u, i, num_user, num_item)
        val64 = (du[u] * 1.0) * di[i]                            # D @ A @ D (:101), entry by entry
        self.diag = torch.from_numpy(np.concatenate([du, di])).to(device)
        p_ptr, p_col, p_val = _item_filter(u, i, val64, num_user, num_item)
        P = graph.CSR(p_ptr, p_col, p_val, num_item, num_item, symmetric=True).to(device)
        if factors is None:
            Vi = _right_singular_vectors(u, i, val64, num_user, num_item, m)
        else:
            Vi = np.asarray(factors, dtype=np.float64)
            if Vi.shape != (num_item, m):
                raise ValueError(f"BSPM: factors is {Vi.shape}, expected ({num_item}, {m}) = (num_item, factor_dim / 2)")
        F = torch.from_numpy((di[:, None] * Vi).astype(np.float32)).contiguous().to(device)            # d_mat_i @ vt.T (:64)
        Gt = torch.from_numpy((Vi * (1.0 / di)[:, None]).astype(np.float32)).contiguous().to(device)   # (vt @ d_mat_i_inv)^T (:65)
        self.filter = ops.BSPMFilter(P, F, Gt)
        self.hist = (rowptr.to(device), col.to(device), torch.from_numpy(val64.astype(np.float32)).to(device))   # Rn, rounded once (:121)

    def _check_flags(self):
        for name, built in (("final_sharpening", True), ("sharpening_off", False), ("t_point_combination", False),
                            ("solver_shr", "euler")):
            if getattr(self, name) != built:
                raise NotImplementedError(f"BSPM: {name}={getattr(self, name)!r}; only {name}={built!r} is built")

    def tile(self, users, width=None):
        return ops.BSPMTile(*self.hist, self.num_item, users, width)

    def _scores(self, tile, mask_value, out=None):
        self._check_flags()
        run = ops.bspm_scores if self.fused else ops.bspm_scores_plain
        return run(self.filter, tile, self.K_s, self.T_s, self.idl_beta, mask_value, out)

    def getUsersRating(self, batch_users):
        """Model/BSPM.py:133-181 -> fp32 [len(batch_users), num_item] on the device, unmasked.  ITEM COLUMNS ONLY: the
        reference returns [len, num_user + num_item]; its user columns hold the IDL term's spill and are never read."""
        self._check_flags()
        users = torch.as_tensor(batch_users, dtype=torch.int64).reshape(-1).to(self.device)
        with torch.no_grad():
            rows = [self._scores(self.tile(users[s:s + ops.BSPM_MAX_TILE]), None)[:min(ops.BSPM_MAX_TILE, users.numel() - s)]
                    for s in range(0, users.numel(), ops.BSPM_MAX_TILE)]
        return rows[0] if len(rows) == 1 else torch.cat(rows)

    def gene_ranklist(self, topk=50, to_cpu=True):
        """Model/BSPM.py:183-203 over ranges of at most 1024 users: each range is scored with its history entries = 1e-6 into
        one reused [B, I] staging buffer and ranked by the exact top-k kernel (ties to the lowest index); the [U, I] matrix
        never exists whole.  Ids are item + num_user."""
        self._check_flags()
        U, I, step = self.num_user, self.num_item, ops.BSPM_MAX_TILE
        with torch.no_grad():
            out = torch.empty((U, topk), dtype=torch.int64, device=self.device)
            staging = torch.empty(min(step, (U + 3) // 4 * 4) * I, dtype=torch.float32, device=self.device)
            for u0 in range(0, U, step):
                u1 = min(U, u0 + step)
                tile = self.tile(torch.arange(u0, u1, dtype=torch.int64, device=self.device))
                sc = self._scores(tile, 1e-6, out=staging[:tile.B * I].view(tile.B, I))
                out[u0:u1], _ = ops.rows_topk(sc[:u1 - u0], topk, id_offset=U)
        return ranking._to_host(out) if to_cpu else out

    full_sort_predict = gene_ranklist
