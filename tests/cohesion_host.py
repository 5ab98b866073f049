"""Host restatements of what Model/COHESION.py and the cf_* kernels of csrc/usergraph.hip compute: the fused node in float32
numpy IN THE CONTRACT'S EXACT ORDER (forward; backward with `chunk`), the same node in float64 with the per-element error
bound of any fixed-order fp32 evaluation, the constructor's draws, and one whole COHESION step in float64 (forward written
out, the gradients float64 autograd over it).  The graph side (co-occurrence top-N, the reverse lists, the kNN graph, the
synthetic case) is tests/dragon_host.py's, imported and unchanged.  Imported by test_cohesion_host.py, test_gpu_cohesion.py
and golden/gen_cohesion.py."""
import numpy as np
import torch

import dragon_host as dh

EPS32 = dh.EPS32
D = 64                                  # Model/COHESION.py:92
_GCN = ("preference", "MLP.weight", "MLP.bias", "MLP_1.weight", "MLP_1.bias")
# the Parameters of Model/COHESION.py in state_dict() order, and the ones the loss reaches
NAMES = (("weight_u", "id_feat", "image_embedding.weight", "text_embedding.weight", "image_trs.weight", "image_trs.bias",
          "text_trs.weight", "text_trs.bias") + tuple(f"{b}.{n}" for b in ("v_gcn", "t_gcn", "id_gcn") for n in _GCN))
WITH_GRAD = ("weight_u", "id_feat") + tuple(f"{b}.{n}" for b in ("v_gcn", "t_gcn") for n in _GCN)

# the reference's COHESION on the synthetic graph of dragon_host.small_case(): main.py:381-383's arguments (model.k set to UU_TOPK)
DIM_E, REG_WEIGHT, DROPOUT, N_LAYERS, MM_LAYERS, II_TOPK, MM_IMAGE_WEIGHT, UU_TOPK = 64, 0.001, 0.0, 2, 1, 10, 0.1, 10
GRAD_ROWS = dh.GRAD_ROWS      # the rows of the two [256, feat] MLP.weight gradients the fixture stores


# ---- the fused node, float32 in the contract's order -----------------------------------------------------------------------
def _f32(*arrays):
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in arrays)


def fuse_fwd32(idr, v, t, h, idx, w, U):
    """result [N, 192] fp32 as chaorec_cohesion_fuse_fwd_f32 defines it: acc = 0; acc = acc + w_j * x[idx_j] for ascending j
    (product and add rounded separately, a slot outside [0, U) skipped); result[u] = x[u] + acc; an item row x[r] + h[r - U]
    (h = (h_id, h_v, h_t) or None: x[r])."""
    x = np.concatenate(_f32(idr, v, t), axis=1)
    (w,) = _f32(w)
    idx = np.asarray(idx, dtype=np.int64)
    acc = np.zeros((U, 3 * D), dtype=np.float32)
    for j in range(idx.shape[1]):
        ok = (idx[:, j] >= 0) & (idx[:, j] < U)
        acc[ok] = acc[ok] + w[ok, j, None] * x[idx[ok, j]]
    items = x[U:] if h is None else x[U:] + np.concatenate(_f32(*h), axis=1)
    return np.concatenate((x[:U] + acc, items), axis=0)


def rev_chunks(idx, U, chunk):
    """The reverse lists of idx [U, k] (dragon_host.reverse) and their chunks: (rev_ptr, perm, row_chunk [U + 1], chunk_row,
    first, end [n_chunks]).  chunk = 0: one chunk per non-empty list."""
    rev_ptr, perm = dh.reverse(idx, U)
    length = np.diff(rev_ptr)
    per_row = (length + chunk - 1) // chunk if chunk > 0 else (length > 0).astype(np.int64)
    row_chunk = np.concatenate(([0], np.cumsum(per_row))).astype(np.int64)
    rows = np.repeat(np.arange(U), per_row)
    within = np.arange(len(rows)) - row_chunk[rows]
    first = rev_ptr[rows] + within * chunk
    end = np.minimum(first + chunk, rev_ptr[rows + 1]) if chunk > 0 else rev_ptr[rows + 1]
    return rev_ptr, perm, row_chunk, rows, first, end


def fuse_bwd32(g, idx, w, U, chunk, has_h=True):
    """(dv, dt [N, 64], dh_v, dh_t [I, 64] or None) fp32 from g [N, 192] as chaorec_cohesion_fuse_bwd_f32 defines them: per
    chunk p_c = ((0 + w_1 g_1) + w_2 g_2) + ... in list order, per row S = ((p_0 + p_1) + p_2) + ... in chunk order (an empty
    list: 0), gx = g[r, 64:] + S.  Columns 0 .. 63 of g are not read."""
    (g, w) = _f32(g, w)
    idx = np.asarray(idx, dtype=np.int64)
    k = idx.shape[1]
    gl = g[:, D:]
    rev_ptr, perm, row_chunk, rows, first, end = rev_chunks(idx, U, chunk)
    rev_u, rev_w = perm // k, w.reshape(-1)[perm]
    part = np.zeros((len(rows), 2 * D), dtype=np.float32)
    for p in range(int((end - first).max()) if len(rows) else 0):
        sel = first + p < end
        e = first[sel] + p
        part[sel] = part[sel] + rev_w[e, None] * gl[rev_u[e]]
    per_row = np.diff(row_chunk)
    S = np.zeros((U, 2 * D), dtype=np.float32)
    has = per_row > 0
    S[has] = part[row_chunk[:-1][has]]
    for c in range(1, int(per_row.max()) if U else 0):
        sel = per_row > c
        S[sel] = S[sel] + part[row_chunk[:-1][sel] + c]
    gx = np.concatenate((gl[:U] + S, gl[U:]), axis=0)
    dv, dt = np.ascontiguousarray(gx[:, :D]), np.ascontiguousarray(gx[:, D:])
    return (dv, dt, dv[U:].copy(), dt[U:].copy()) if has_h else (dv, dt, None, None)


# ---- the fused node, float64 with its bound ---------------------------------------------------------------------------------
def fuse_fwd64(idr, v, t, h, idx, w, U):
    """result [N, 192] in float64 and the bound of ANY fixed-order fp32 evaluation of it: a row is a sum of n addends (k
    products and the residual; an item row's two), each rounded at most once before it is added and then carried through at
    most n - 1 rounded adds, so |error| <= gamma_n sum |addends| <= (n + 2) 2^-24 sum |addends| (n 2^-24 << 1)."""
    x = np.concatenate([np.asarray(a, dtype=np.float64) for a in (idr, v, t)], axis=1)
    w = np.asarray(w, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < U)
    safe, wk = np.where(ok, idx, 0), np.where(ok, w, 0.0)
    out_u = x[:U] + (wk[:, :, None] * x[:U][safe]).sum(axis=1)
    mag_u = np.abs(x[:U]) + (np.abs(wk)[:, :, None] * np.abs(x[:U][safe])).sum(axis=1)
    n = idx.shape[1] + 1
    hh = np.zeros_like(x[U:]) if h is None else np.concatenate([np.asarray(a, dtype=np.float64) for a in h], axis=1)
    out = np.concatenate((out_u, x[U:] + hh), axis=0)
    bound = np.concatenate(((n + 2) * EPS32 * mag_u, (2 + 2) * EPS32 * (np.abs(x[U:]) + np.abs(hh)) * (h is not None)), axis=0)
    return out, bound, n


def fuse_bwd64(g, idx, w, U):
    """(dv, dt) [N, 64] in float64, their bounds and the longest reverse list + 1.  User row r: gx = g[r, 64:] + the m_r
    products of its reverse list, n_r = m_r + 1 addends.  Whatever the chunking, an addend is rounded once as a product and
    then passes at most (its chunk's length) + (the row's chunks - 1) + 1 <= n_r rounded adds, so (n_r + 2) 2^-24
    sum |addends| bounds every fixed order.  Item rows are copies: bound 0."""
    g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    k = idx.shape[1]
    gl = g[:, D:]
    flat = idx.reshape(-1)
    ok = (flat >= 0) & (flat < U)
    gx, mag = gl.copy(), np.abs(gl)
    contrib = (w.reshape(-1, 1) * np.repeat(gl[:U], k, axis=0))[ok]
    np.add.at(gx, flat[ok], contrib)
    np.add.at(mag, flat[ok], np.abs(contrib))
    n = np.ones((g.shape[0], 1), dtype=np.int64)
    n[:U, 0] += np.bincount(flat[ok], minlength=U)
    bound = (n + 2) * EPS32 * mag
    bound[U:] = 0.0
    return (gx[:, :D], gx[:, D:]), (bound[:, :D], bound[:, D:]), int(n.max())


# ---- one COHESION step ------------------------------------------------------------------------------------------------------
def norm_adj(edges, U, I):
    """Model/COHESION.py:165-189 -> dense float64 [N, N]: binary A (repeats count once), (1e-7 + degree)^-1/2 on both ends."""
    e = np.asarray(edges, dtype=np.int64)
    N = U + I
    A = np.zeros((N, N))
    A[e[:, 0], e[:, 1]] = 1.0
    A[e[:, 1], e[:, 0]] = 1.0
    d = np.power(A.sum(1) + 1e-7, -0.5)
    return A * d[:, None] * d[None, :]


def step(weights, v_feat, t_feat, edges, U, I, epoch_idx, epoch_w, users, pos_local, neg_local, reg_weight, n_layers, mm_layers,
         knn_v, knn_t, mm_image_weight, grads=True):
    """Model/COHESION.py:296-385 in float64.  weights: {name: array} of NAMES.
    -> dict(result, bpr, reg, loss, grads {name})."""
    f64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)   # noqa: E731
    p = {n: f64(weights[n]).requires_grad_(n in WITH_GRAD) for n in NAMES}
    adj = f64(norm_adj(edges, U, I))

    def gcn(pre, feat, id_embd):                                            # :28-46
        hid = torch.nn.functional.leaky_relu(feat @ p[pre + ".MLP.weight"].T + p[pre + ".MLP.bias"])
        temp = hid @ p[pre + ".MLP_1.weight"].T + p[pre + ".MLP_1.bias"]
        temp = torch.abs((id_embd * id_embd + temp * temp) / 2 + 1e-8).sqrt()
        ego = torch.nn.functional.normalize(torch.cat((p[pre + ".preference"], temp), dim=0))
        layer, total = ego, ego
        for _ in range(n_layers):
            layer = adj @ layer
            layer = torch.nn.functional.cosine_similarity(layer, ego, dim=-1).unsqueeze(1) * layer
            total = total + layer
        return total

    id_feat = p["id_feat"]
    id_rep = gcn("id_gcn", id_feat, id_feat).detach()                       # :321 (id_rep.data)
    rep = torch.cat((id_rep, gcn("v_gcn", f64(v_feat), id_feat), gcn("t_gcn", f64(t_feat), id_feat)), dim=1)
    idx, w = torch.as_tensor(np.asarray(epoch_idx, dtype=np.int64)), f64(epoch_w)
    user_rep = rep[:U] + torch.matmul(w.unsqueeze(1), rep[:U][idx]).squeeze(1)
    mm = f64(mm_image_weight * dh.knn_adj(knn_v, I) + (1.0 - mm_image_weight) * dh.knn_adj(knn_t, I))
    h_i = rep[U:]
    for _ in range(mm_layers):
        h_i = mm @ h_i
    result = torch.cat((user_rep, rep[U:] + h_i), dim=0)
    users, pos_local, neg_local = (torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos_local, neg_local))
    ue, pe, ne = result[users], result[U + pos_local], result[U + neg_local]
    margin = (ue * pe).view(-1, 3, D).sum(-1) - (ue * ne).view(-1, 3, D).sum(-1)
    aw = (1 - margin.softmax(-1).detach()).view(-1, 3, 1).expand(-1, 3, D).reshape(-1, 3 * D)      # :361-369
    s = (ue * pe * aw).sum(1) - (ue * ne * aw).sum(1)
    bpr = -torch.mean(torch.log2(torch.sigmoid(s)))                         # :379
    reg = reg_weight * ((p["v_gcn.preference"][users] ** 2).mean() + (p["t_gcn.preference"][users] ** 2).mean())
    reg = reg + reg_weight * (p["weight_u"] ** 2).mean()
    loss = bpr + reg
    out = dict(result=result.detach().numpy(), bpr=float(bpr.detach()), reg=float(reg.detach()), loss=float(loss.detach()))
    if grads:
        gs = torch.autograd.grad(loss, [p[n] for n in WITH_GRAD])
        out["grads"] = {n: g.numpy() for n, g in zip(WITH_GRAD, gs)}
    return out


def init_weights(c):
    """The draws of the constructor (Model/COHESION.py:102-163, :22-26) replayed on torch's CPU generator -> {name: array}.
    (The tables the reference fills from numpy first are overwritten by xavier_normal_ from torch's generator.)"""
    nn = torch.nn
    U, I = c["U"], c["I"]
    torch.manual_seed(c["seed"])
    w = {}

    def lin(name, i, o):
        m = nn.Linear(i, o)
        w[name + ".weight"], w[name + ".bias"] = m.weight.detach().numpy().copy(), m.bias.detach().numpy().copy()

    def gcn(pre, width):
        w[pre + ".preference"] = nn.init.xavier_normal_(torch.empty(U, D)).numpy().copy()
        lin(pre + ".MLP", width, 4 * D)
        lin(pre + ".MLP_1", 4 * D, D)

    w["image_embedding.weight"], w["text_embedding.weight"] = c["v_feat"].copy(), c["t_feat"].copy()
    lin("image_trs", c["v_feat"].shape[1], DIM_E)
    lin("text_trs", c["t_feat"].shape[1], DIM_E)
    w["weight_u"] = torch.softmax(nn.init.xavier_normal_(torch.empty(U, 2, 1)), dim=1).numpy().copy()
    gcn("v_gcn", c["v_feat"].shape[1])
    gcn("t_gcn", c["t_feat"].shape[1])
    w["id_feat"] = nn.init.xavier_normal_(torch.empty(I, D)).numpy().copy()
    gcn("id_gcn", D)
    return w
