"""Host restatements of what Model/DualGNN.py and the dg_fuse kernels of csrc/usergraph.hip compute, in float64: the fused node
forward and backward with the per-element error bounds of an ordered fp32 evaluation, the constructor's draws, and one whole
DualGNN step (forward written out, the gradients float64 autograd over it).  The graph side (co-occurrence top-N, the epoch
sample, the synthetic case) is tests/dragon_host.py's, imported and unchanged.  Imported by test_dualgnn_host.py,
test_gpu_dualgnn.py and golden/gen_dualgnn.py."""
import numpy as np
import torch

import dragon_host as dh

EPS32 = dh.EPS32
# the Parameters of Model/DualGNN.py in state_dict() order, and the ones the loss reaches
NAMES = ("weight_u", "weight_i", "MLP_v.weight", "MLP_t.weight", "MLP_user.weight", "MLP_user.bias",
         "v_gcn.preference", "v_gcn.MLP.weight", "v_gcn.MLP.bias", "v_gcn.MLP_1.weight", "v_gcn.MLP_1.bias",
         "t_gcn.preference", "t_gcn.MLP.weight", "t_gcn.MLP.bias", "t_gcn.MLP_1.weight", "t_gcn.MLP_1.bias")
WITH_GRAD = ("weight_u", "weight_i",
             "v_gcn.preference", "v_gcn.MLP.weight", "v_gcn.MLP.bias", "v_gcn.MLP_1.weight", "v_gcn.MLP_1.bias",
             "t_gcn.preference", "t_gcn.MLP.weight", "t_gcn.MLP.bias", "t_gcn.MLP_1.weight", "t_gcn.MLP_1.bias")

# the reference's DualGNN on the synthetic graph of dragon_host.small_case(): main.py:280's arguments
DIM, REG_WEIGHT, UU_TOPK = 64, 0.01, 10
GRAD_ROWS = dh.GRAD_ROWS      # the rows of the two [256, feat] MLP.weight gradients the fixture stores


# ---- the fused node ------------------------------------------------------------------------------------------------------------
def _f64(*arrays):
    return (np.asarray(a, dtype=np.float64) for a in arrays)


def fuse_fwd(v, t, wu, idx, w, U):
    """result [N, D] of (v, t [N, D], wu [U, 2(, 1)], idx / w [U, k]) and its per-element error bound for the kernel's fp32
    evaluation.

    User row u: result = x[u] + sum_j w_j x[idx_j] over the slots with 0 <= idx_j < U, x[r] = a_r v[r] + b_r t[r].  The kernel
    rounds a v, b t, their sum and the product with w_j separately -- at most FOUR roundings on an addend (the residual has
    three) -- and then adds the n = k + 1 addends in order, n - 1 roundings at most on any of them.  With
    mag = sum_j |w_j| (|a| |v| + |b| |t|) (the residual's w = 1), the error is at most gamma_(n + 3) mag; (n + 4) 2^-24 mag
    covers the second-order terms of gamma for every n used here (n 2^-24 << 1).
    Item row r >= U: result = v + t, one rounding: 2^-24 (|v| + |t|)."""
    v, t, w = _f64(v, t, w)
    wu = np.asarray(wu, dtype=np.float64).reshape(-1, 2)
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < U)
    safe = np.where(ok, idx, 0)
    x = wu[:, :1] * v[:U] + wu[:, 1:] * t[:U]
    ax = np.abs(wu[:, :1]) * np.abs(v[:U]) + np.abs(wu[:, 1:]) * np.abs(t[:U])
    wk = np.where(ok, w, 0.0)
    out_u = x + (wk[:, :, None] * x[safe]).sum(axis=1)                      # [U, k, D] -- here it may exist
    mag = ax + (np.abs(wk)[:, :, None] * ax[safe]).sum(axis=1)
    n = idx.shape[1] + 1
    out = np.concatenate((out_u, v[U:] + t[U:]), axis=0)
    bound = np.concatenate(((n + 4) * EPS32 * mag, EPS32 * (np.abs(v[U:]) + np.abs(t[U:]))), axis=0)
    return out, bound, n


def fuse_bwd(g, v, t, wu, idx, w, U):
    """(dv, dt [N, D], dw [U, 2]) from g [N, D], their bounds, and the longest owner list + 1.

    User row r: gx[r] = g[r] + sum over the slots (u, j) that name r of w[u, j] g[u]: n_r rounded products added in order
    (n_r = the list's length + 1, the residual g[r] exact), so (n_r + 2) 2^-24 sum |addends| bounds gx with room for the one
    rounding of the scale a_r gx / b_r gx (dragon_host.aggregate_bwd's construction): the bounds of dv and dt are |a_r| and
    |b_r| times that.  A row dot of D rounded products summed in a fixed tree adds (D + 2) 2^-24 sum |products| to what its
    inputs carry (sum b_gx |v|).  Item row r >= U: dv = dt = g, exact."""
    g, v, t, w = _f64(g, v, t, w)
    wu = np.asarray(wu, dtype=np.float64).reshape(-1, 2)
    idx = np.asarray(idx, dtype=np.int64)
    k, D = idx.shape[1], v.shape[1]
    flat = idx.reshape(-1)
    ok = (flat >= 0) & (flat < U)
    gx, mag = g[:U].copy(), np.abs(g[:U])
    contrib = (w.reshape(-1, 1) * np.repeat(g[:U], k, axis=0))[ok]
    np.add.at(gx, flat[ok], contrib)
    np.add.at(mag, flat[ok], np.abs(contrib))
    n = np.bincount(flat[ok], minlength=U)[:, None] + 1
    b_gx = (n + 2) * EPS32 * mag
    zero = np.zeros_like(g[U:])
    dv = np.concatenate((wu[:, :1] * gx, g[U:]), axis=0)
    dt = np.concatenate((wu[:, 1:] * gx, g[U:]), axis=0)
    b_dv = np.concatenate((np.abs(wu[:, :1]) * b_gx, zero), axis=0)
    b_dt = np.concatenate((np.abs(wu[:, 1:]) * b_gx, zero), axis=0)
    dw = np.stack(((gx * v[:U]).sum(1), (gx * t[:U]).sum(1)), axis=1)
    b_dw = np.stack(((b_gx * np.abs(v[:U])).sum(1) + (D + 2) * EPS32 * np.abs(gx * v[:U]).sum(1),
                     (b_gx * np.abs(t[:U])).sum(1) + (D + 2) * EPS32 * np.abs(gx * t[:U]).sum(1)), axis=1)
    return (dv, dt, dw), (b_dv, b_dt, b_dw), int(n.max())


# ---- one DualGNN step --------------------------------------------------------------------------------------------------------
def step(weights, v_feat, t_feat, edges, U, I, epoch_idx, epoch_w, users, pos_local, neg_local, reg_weight, grads=True):
    """Model/DualGNN.py:179-286 ('weighted_sum') in float64.  weights: {name: array} of NAMES.
    -> dict(result, bpr, reg, loss, grads {name})."""
    f64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)   # noqa: E731
    p = {n: f64(weights[n]).requires_grad_(n in WITH_GRAD) for n in NAMES}
    e = np.asarray(edges, dtype=np.int64)
    row, col = torch.as_tensor(np.concatenate((e[:, 0], e[:, 1]))), torch.as_tensor(np.concatenate((e[:, 1], e[:, 0])))
    N = U + I
    deg = torch.zeros(N, dtype=torch.float64).index_add_(0, row, torch.ones(row.numel(), dtype=torch.float64))
    norm = (deg.pow(-0.5)[row] * deg.pow(-0.5)[col]).view(-1, 1)            # Model/DualGNN.py:41-45

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
    x = wu[:, :1] * v_rep[:U] + wu[:, 1:] * t_rep[:U]                       # :198-203
    idx, w = torch.as_tensor(np.asarray(epoch_idx, dtype=np.int64)), f64(epoch_w)
    user_rep = x + torch.matmul(w.unsqueeze(1), x[idx]).squeeze(1)          # :235-236
    result = torch.cat((user_rep, (v_rep + t_rep)[U:]), dim=0)
    users, pos_local, neg_local = (torch.as_tensor(np.asarray(a, dtype=np.int64)) for a in (users, pos_local, neg_local))
    ue = result[users]
    s = (ue * result[U + pos_local]).sum(1) - (ue * result[U + neg_local]).sum(1)
    bpr = -torch.mean(torch.log(torch.sigmoid(s) + 1e-5))
    reg = reg_weight * ((p["v_gcn.preference"][users] ** 2).mean() + (p["t_gcn.preference"][users] ** 2).mean())
    reg = reg + reg_weight * (p["weight_u"] ** 2).mean() + reg_weight * (p["weight_i"] ** 2).mean()      # :265-267
    loss = bpr + reg
    out = dict(result=result.detach().numpy(), bpr=float(bpr.detach()), reg=float(reg.detach()), loss=float(loss.detach()))
    if grads:
        gs = torch.autograd.grad(loss, [p[n] for n in WITH_GRAD])
        out["grads"] = {n: g.numpy() for n, g in zip(WITH_GRAD, gs)}
    return out


def init_weights(c):
    """The draws of the constructor (Model/DualGNN.py:135-157, :68-73) replayed on torch's CPU generator -> {name: array}."""
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
    return w
