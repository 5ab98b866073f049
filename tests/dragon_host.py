"""Host restatements of what csrc/usergraph.hip and Model/DRAGON.py compute, in integers and float64: the co-occurrence
top-N (scipy R R^T plus the tie rule), the epoch sample (the counter generator in numpy uint64), the aggregation forward and
backward with the sums of absolute addends their error bounds need, and one whole DRAGON step (forward written out, the
gradients float64 autograd over it, the symmetric normalisation without torch-geometric).  Imported by test_dragon_host.py,
test_gpu_dragon.py and golden/gen_dragon.py."""
import os

import numpy as np
import scipy.sparse as sp
import torch
from accept import ULP24, rel_dev, user_item_dict  # noqa: F401
from vae_ops_host import mix64      # csrc/common.h mix64 on uint64 arrays

TOPN = 200
EPS32 = ULP24               # unit roundoff of fp32, 2^-24 (this module's older name for it; accept.EPS32 is the spacing 2^-23)
# the Parameters of Model/DRAGON.py in registration order, and the ones the loss reaches
NAMES = ("weight_u", "weight_i", "MLP_v.weight", "MLP_t.weight", "MLP_user.weight", "MLP_user.bias",
         "v_gcn.preference", "v_gcn.MLP.weight", "v_gcn.MLP.bias", "v_gcn.MLP_1.weight", "v_gcn.MLP_1.bias",
         "t_gcn.preference", "t_gcn.MLP.weight", "t_gcn.MLP.bias", "t_gcn.MLP_1.weight", "t_gcn.MLP_1.bias",
         "image_embedding.weight", "text_embedding.weight", "image_trs.weight", "image_trs.bias", "text_trs.weight", "text_trs.bias")
WITH_GRAD = ("weight_u",
             "v_gcn.preference", "v_gcn.MLP.weight", "v_gcn.MLP.bias", "v_gcn.MLP_1.weight", "v_gcn.MLP_1.bias",
             "t_gcn.preference", "t_gcn.MLP.weight", "t_gcn.MLP.bias", "t_gcn.MLP_1.weight", "t_gcn.MLP_1.bias")


# the reference's DRAGON on the synthetic graph of small_case(): main.py:284's arguments
DIM, REG_WEIGHT, N_LAYERS, II_TOPK, UU_TOPK, MM_IMAGE_WEIGHT = 64, 0.01, 2, 10, 10, 0.6
GRAD_ROWS = np.arange(0, 256, 4)      # the rows of the two [256, feat] MLP.weight gradients the fixture stores


# ---- (a) the co-occurrence graph ---------------------------------------------------------------------------------------------
def history_csr(edges, U):
    """edges [E, 2] (user, GLOBAL item id) -> (rowptr int64 [U + 1], col int32 local ids, ascending, no repeats)."""
    e = np.asarray(edges, dtype=np.int64)
    key = np.unique(e[:, 0] * (1 << 32) + (e[:, 1] - U))
    u, i = key >> 32, key & 0xFFFFFFFF
    rowptr = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(np.bincount(u, minlength=U), out=rowptr[1:])
    return rowptr, i.astype(np.int32)


def cooccurrence(rowptr, col, U, I):
    """R R^T without its diagonal: csr [U, U] of c(u, v) = |items(u) & items(v)| > 0, columns ascending."""
    R = sp.csr_matrix((np.ones(len(col), dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(rowptr, dtype=np.int64)), shape=(U, I))
    C = (R @ R.T).tocsr()
    C.setdiag(0)
    C.eliminate_zeros()
    C.sort_indices()
    return C


def topn(C, N=TOPN):
    """Row u: its users by count descending, then id ascending, cut at N -> idx, cnt int32 [U, N], len int32 [U]."""
    U = C.shape[0]
    idx, cnt, length = np.zeros((U, N), dtype=np.int32), np.zeros((U, N), dtype=np.int32), np.zeros(U, dtype=np.int32)
    for u in range(U):
        ids, c = C.indices[C.indptr[u]:C.indptr[u + 1]], C.data[C.indptr[u]:C.indptr[u + 1]]
        order = np.lexsort((ids, -c))[:N]
        m = len(order)
        idx[u, :m], cnt[u, :m], length[u] = ids[order], c[order], m
    return idx, cnt, length


def user_graph_dict(C, N=TOPN):
    """The reference's user_graph_dict.npy ({user: [[ids], [counts as floats]]}) under the tie rule."""
    idx, cnt, length = topn(C, N)
    return {u: [idx[u, :length[u]].tolist(), cnt[u, :length[u]].astype(np.float32).tolist()] for u in range(C.shape[0])}


def check_ids(u, ids, counts, C, N=TOPN):
    """The id rule against a list whose order among equal counts is unspecified (torch.topk): `ids` / `counts` of user u are a
    valid top-N of row u of C.  Returns None or what is wrong."""
    row_ids, row_c = C.indices[C.indptr[u]:C.indptr[u + 1]], C.data[C.indptr[u]:C.indptr[u + 1]]
    ids, counts = np.asarray(ids, dtype=np.int64), np.asarray(counts, dtype=np.int64)
    if len(ids) != min(len(row_ids), N):
        return f"user {u}: {len(ids)} neighbours, expected {min(len(row_ids), N)}"
    if len(ids) == 0:
        return None
    if not np.array_equal(counts, np.sort(row_c)[::-1][:N]):
        return f"user {u}: count sequence differs"
    if len(np.unique(ids)) != len(ids):
        return f"user {u}: an id repeats"
    true = dict(zip(row_ids.tolist(), row_c.tolist()))
    if any(true.get(int(i)) != int(c) for i, c in zip(ids, counts)):
        return f"user {u}: an id is listed with a count that is not its own"
    last = counts[-1]
    if set(ids[counts > last].tolist()) != set(row_ids[row_c > last].tolist()):
        return f"user {u}: the ids above the last count differ"
    if len(row_ids) <= N and set(ids.tolist()) != set(row_ids.tolist()):
        return f"user {u}: the id set differs"
    return None


# ---- (b) the epoch sample -------------------------------------------------------------------------------------------------
def draw(seed, epoch, u, slot, n):
    """r uniform in [0, n): ((mix64(seed ^ mix64(epoch ^ mix64(u << 32 | slot))) >> 32) * n) >> 32, elementwise (csrc/draws.h draw_hash)."""
    u, slot, n = (np.atleast_1d(np.asarray(a, dtype=np.uint64)) for a in (u, slot, n))
    h = mix64(np.uint64(seed) ^ mix64(np.uint64(epoch) ^ mix64((u << np.uint64(32)) | slot)))
    return ((h >> np.uint64(32)) * n) >> np.uint64(32)


def sample(idx, cnt, length, k, seed, epoch):
    """-> epoch_idx int32 [U, k], weights float64 [U, k], src int64 [U, k] (the ORIGINAL neighbour slot every slot ends at,
    -1 in an empty row), r int64 [U, k] (the slot that slot j >= len copies, -1 elsewhere)."""
    U = idx.shape[0]
    src = np.tile(np.arange(k, dtype=np.int64), (U, 1))
    r = np.full((U, k), -1, dtype=np.int64)
    for u in np.nonzero((length > 0) & (length < k))[0]:
        n = int(length[u])
        for j in range(n, k):                                   # the urn over the GROWN list: slot j copies slot r_j < j
            r[u, j] = int(draw(seed, epoch, u, j, j)[0])
            src[u, j] = src[u, r[u, j]]
    empty = length == 0
    src[empty] = -1
    rows = np.arange(U)[:, None]
    e_idx = np.where(empty[:, None], 0, idx[rows, np.maximum(src, 0)]).astype(np.int32)
    c = np.where(empty[:, None], 0, cnt[rows, np.maximum(src, 0)]).astype(np.float64)
    ex = np.exp(c - c.max(axis=1, keepdims=True))
    w = ex / ex.sum(axis=1, keepdims=True)
    w[empty] = 0.0
    return e_idx, w, src, r


def reverse(epoch_idx, U):
    """For every user r the flat slots u k + j that name r, ascending: (rev_ptr int64 [U + 1], rev_slot int64 [U k])."""
    flat = np.asarray(epoch_idx, dtype=np.int64).reshape(-1)
    perm = np.argsort(flat, kind="stable")
    return np.searchsorted(flat[perm], np.arange(U + 1)), perm


# ---- (c) the aggregation ----------------------------------------------------------------------------------------------------
def _x(v, t, wu):
    v, t, wu = (np.asarray(a, dtype=np.float64) for a in (v, t, wu))
    wu = wu.reshape(-1, 2)
    return np.concatenate((wu[:, :1] * v, wu[:, 1:] * t), axis=1)


def aggregate_fwd(v, t, wu, idx, w):
    """-> out [U, 2 D] and, per element, (the sum of |addends|, the number of addends n = k + 1)."""
    x, w = _x(v, t, wu), np.asarray(w, dtype=np.float64)
    g = x[np.asarray(idx, dtype=np.int64)]                                  # [U, k, 2 D] -- here it may exist
    out = x + (w[:, :, None] * g).sum(axis=1)
    mag = np.abs(x) + (np.abs(w)[:, :, None] * np.abs(g)).sum(axis=1)
    return out, mag, idx.shape[1] + 1


def aggregate_bwd(g, v, t, wu, idx, w):
    """-> dv, dt [U, D], dw [U, 2] and their error bounds for an ordered fp32 evaluation (gx: n rounded products added in
    order, n = owner-list length + 1: (n + 2) eps sum|addends|; the scale by weight_u stays inside it; a row dot of D
    products adds (D + 2) eps sum|products| to the bound its inputs carry)."""
    g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
    v, t = np.asarray(v, dtype=np.float64), np.asarray(t, dtype=np.float64)
    wu = np.asarray(wu, dtype=np.float64).reshape(-1, 2)
    U, k = idx.shape
    D = v.shape[1]
    gx, mag = g.copy(), np.abs(g)
    flat = np.asarray(idx, dtype=np.int64).reshape(-1)
    contrib = w.reshape(-1, 1) * np.repeat(g, k, axis=0)
    np.add.at(gx, flat, contrib)
    np.add.at(mag, flat, np.abs(contrib))
    n = np.bincount(flat, minlength=U)[:, None] + 1
    b_gx = (n + 2) * EPS32 * mag
    dv, dt = wu[:, :1] * gx[:, :D], wu[:, 1:] * gx[:, D:]
    b_dv, b_dt = np.abs(wu[:, :1]) * b_gx[:, :D], np.abs(wu[:, 1:]) * b_gx[:, D:]
    dw = np.stack(((gx[:, :D] * v).sum(1), (gx[:, D:] * t).sum(1)), axis=1)
    b_dw = np.stack(((b_gx[:, :D] * np.abs(v)).sum(1) + (D + 2) * EPS32 * np.abs(gx[:, :D] * v).sum(1),
                     (b_gx[:, D:] * np.abs(t)).sum(1) + (D + 2) * EPS32 * np.abs(gx[:, D:] * t).sum(1)), axis=1)
    return (dv, dt, dw), (b_dv, b_dt, b_dw), int(n.max())


# ---- one DRAGON step --------------------------------------------------------------------------------------------------------
def knn_indices(feat, topk):
    """Model/DRAGON.py:204-207 in float64: each item's topk most cosine-similar items (itself among them)."""
    x = torch.as_tensor(np.asarray(feat), dtype=torch.float64)
    x = x / torch.norm(x, p=2, dim=-1, keepdim=True)
    return torch.topk(x @ x.T, topk, dim=-1)[1].numpy()


def knn_adj(knn_ind, n):
    """:209-225 -> dense float64 [n, n]: a one per listed neighbour, (1e-7 + row sum)^-1/2 on both ends."""
    rows = np.repeat(np.arange(n), knn_ind.shape[1])
    A = np.zeros((n, n))
    np.add.at(A, (rows, knn_ind.reshape(-1)), 1.0)
    d = np.power(1e-7 + A.sum(1), -0.5)
    return A * d[:, None] * d[None, :]


def step(weights, v_feat, t_feat, edges, U, I, epoch_idx, epoch_w, users, pos_local, neg_local, reg_weight, n_layers, knn_v, knn_t,
         mm_image_weight, grads=True):
    """Model/DRAGON.py:272-356 in float64.  weights: {name: array} of NAMES.  -> dict(result, bpr, reg, loss, grads {name})."""
    f64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)   # noqa: E731
    p = {n: f64(weights[n]).requires_grad_(n in WITH_GRAD) for n in NAMES}
    e = np.asarray(edges, dtype=np.int64)
    row, col = torch.as_tensor(np.concatenate((e[:, 0], e[:, 1]))), torch.as_tensor(np.concatenate((e[:, 1], e[:, 0])))
    N = U + I
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, row, torch.ones(row.numel(), dtype=torch.float64))
    norm = (deg.pow(-0.5)[row] * deg.pow(-0.5)[col]).view(-1, 1)            # BasicGCN.py:74-76

    def conv(x):                                                            # source row -> target col, add-aggregated
        return torch.zeros_like(x).index_add_(0, col, norm * x[row])

    def gcn(pre, feat):
        h = torch.nn.functional.leaky_relu(f64(feat) @ p[pre + ".MLP.weight"].T + p[pre + ".MLP.bias"])
        temp = h @ p[pre + ".MLP_1.weight"].T + p[pre + ".MLP_1.bias"]
        x = torch.nn.functional.normalize(torch.cat((p[pre + ".preference"], temp), dim=0))
        h = conv(x)
        return x + h + conv(h)                                              # the same conv twice (:87-90)

    v_rep, t_rep = gcn("v_gcn", v_feat), gcn("t_gcn", t_feat)
    wu = p["weight_u"].view(U, 2)
    x = torch.cat((wu[:, :1] * v_rep[:U], wu[:, 1:] * t_rep[:U]), dim=1)
    idx, w = torch.as_tensor(np.asarray(epoch_idx, dtype=np.int64)), f64(epoch_w)
    user_rep = x + torch.matmul(w.unsqueeze(1), x[idx]).squeeze(1)
    item_rep = torch.cat((v_rep[U:], t_rep[U:]), dim=1)
    mm = f64(mm_image_weight * knn_adj(knn_v, I) + (1.0 - mm_image_weight) * knn_adj(knn_t, I))
    h_i = item_rep
    for _ in range(n_layers):
        h_i = mm @ h_i
    result = torch.cat((user_rep, item_rep + h_i), dim=0)
    users, pos_local, neg_local = (torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos_local, neg_local))
    ue = result[users]
    s = (ue * result[U + pos_local]).sum(1) - (ue * result[U + neg_local]).sum(1)
    bpr = -torch.mean(torch.log(torch.sigmoid(s) + 1e-5))
    reg = reg_weight * ((p["v_gcn.preference"][users] ** 2).mean() + (p["t_gcn.preference"][users] ** 2).mean())
    reg = reg + reg_weight * (p["weight_u"] ** 2).mean()
    loss = bpr + reg
    out = dict(result=result.detach().numpy(), bpr=float(bpr.detach()), reg=float(reg.detach()), loss=float(loss.detach()))
    if grads:
        gs = torch.autograd.grad(loss, [p[n] for n in WITH_GRAD])
        out["grads"] = {n: g.numpy() for n, g in zip(WITH_GRAD, gs)}
    return out


def small_case():
    """U 300, I 257, feature widths 128 and 96 (values exact in fp16).  User 299 holds item 256 alone (no neighbour: the
    all-zero weight row); users 0 .. 9 hold one of the items 0 .. 4 in pairs (one neighbour each: nine urn draws at k = 10);
    the others hold 2 .. 8 of the items 10 .. 255.  B 128 interactions with random negatives."""
    U, I, B = 300, 257, 128
    rng = np.random.default_rng(20261018)
    pairs = {(U - 1, I - 1)}
    for u in range(10):
        pairs.add((u, u // 2))
    for u in range(10, U - 1):
        for i in rng.choice(np.arange(10, I - 1), size=int(rng.integers(2, 9)), replace=False).tolist():
            pairs.add((u, int(i)))
    e = np.array(sorted(pairs), dtype=np.int64)
    edges = np.stack([e[:, 0], e[:, 1] + U], 1)
    pick = rng.choice(len(edges), size=B, replace=False)
    pick[0], pick[1] = len(edges) - 1, 0                       # the user without neighbours and a user with one
    v_feat = rng.standard_normal((I, 128)).astype(np.float16).astype(np.float32)
    t_feat = rng.standard_normal((I, 96)).astype(np.float16).astype(np.float32)
    return dict(U=U, I=I, edges=edges, users=edges[pick, 0].copy(), pos=edges[pick, 1].copy(), neg=rng.integers(U, U + I, B).astype(np.int64),
                v_feat=v_feat, t_feat=t_feat, seed=11, draw_seed=1234)


def init_weights(c):
    """The draws of the constructor (Model/DRAGON.py:136-179, :68-73) replayed on torch's CPU generator -> {name: array}."""
    nn = torch.nn
    U, I, D = c["U"], c["I"], DIM
    torch.manual_seed(c["seed"])
    w = {}

    def lin(name, i, o, bias=True):
        m = nn.Linear(i, o, bias=bias)
        w[name + ".weight"] = m.weight.detach().numpy().copy()
        if bias:
            w[name + ".bias"] = m.bias.detach().numpy().copy()

    def mix(name, n):
        t = nn.init.xavier_normal_(torch.randn(n, 2, 1))
        w[name] = torch.softmax(t, dim=1).numpy().copy()

    lin("MLP_v", D, D, False)
    lin("MLP_t", D, D, False)
    mix("weight_u", U)
    mix("weight_i", I)
    lin("MLP_user", 2 * D, D)
    for pre, feat in (("v_gcn", c["v_feat"]), ("t_gcn", c["t_feat"])):
        w[pre + ".preference"] = nn.init.xavier_normal_(torch.empty(U, D)).numpy().copy()
        lin(pre + ".MLP", feat.shape[1], 4 * D)
        lin(pre + ".MLP_1", 4 * D, D)
    w["image_embedding.weight"], w["text_embedding.weight"] = c["v_feat"].copy(), c["t_feat"].copy()
    lin("image_trs", c["v_feat"].shape[1], DIM)
    lin("text_trs", c["t_feat"].shape[1], DIM)
    return w


def load_fixture(golden_dir, name):
    g = dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))
    return g
