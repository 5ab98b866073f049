"""Host restatement of what Model/GraphAug.py computes, in torch on the CPU at a chosen dtype, following the reference's order
of operations: the main propagate, the MixHop encoder, the view learner's sampler written per EDGE over gathered [E, 128] rows
(so that the kernel's P[row] + Q[col] split is checked against something else), the views' propagates over the coalesced sum
of the sampled values and the random entries, the loss with its four parts and its gradients (autograd over the restated
forward), and the plain Adam loop.  float64 is the yardstick; the same lines at float32 measure what fp32 arithmetic alone
costs (the bounds of the kernel tests).  Also the synthetic case, the draws (GIVEN everywhere) and the constructor's weight
draws.  Imported by test_graphaug_host.py, test_gpu_graphaug.py and golden/gen_graphaug.py."""
import math
import os
from collections import OrderedDict

import numpy as np
import torch
from accept import ULP24, rel_dev, user_item_dict  # noqa: F401

D = 64
DIM_E, REG_WEIGHT, N_LAYERS, SSL_TEMP, SSL_ALPHA, LR = 64, 0.001, 3, 0.2, 0.01, 0.001
IB, H, N_RANDOM, RANDOM_VALUE, LEAKY, DROP = 32, 200, 100000, 0.05, 0.5, 0.5
TOPK = 10
N_STEPS = 3
P_LO, P_HI = 2.0 ** -23, 1.0 - 2.0 ** -23          # clamp_probs / _clipped_sigmoid of the torch the golden was made with (fp32 eps)
TINY = float(np.finfo(np.float32).tiny)

UPPER = tuple(f"backbone_gnn.upper_layers.{k}.{p}" for k in range(3) for p in ("weight_matrix", "bias"))
BOTTOM = tuple(f"backbone_gnn.bottom_layers.{k}.{p}" for k in range(3) for p in ("weight_matrix", "bias"))      # NOT parameters
FC = ("backbone_gnn.fully_connected.weight", "backbone_gnn.fully_connected.bias")
MLP = tuple(f"view_learner.mlp_edge_model.{k}.{p}" for k in (0, 2) for p in ("weight", "bias"))
PARAMS = ("uEmbeds", "iEmbeds") + UPPER + FC + MLP                                    # named_parameters() order: 14
# state_dict() order: the encoder is registered twice (backbone_gnn and view_learner.encoder are one module)
NAMES = ("uEmbeds", "iEmbeds") + UPPER + FC + tuple(n.replace("backbone_gnn.", "view_learner.encoder.") for n in UPPER + FC) + MLP
WITH_GRAD = ("uEmbeds", "iEmbeds") + UPPER + FC                                        # the edge MLP gets no gradient
PARTS = ("bpr", "reg", "cl", "kl")


def small_case():
    """84 users, 29 items (N = 113: no multiple of the sampler's 32 rows per workgroup), about 300 distinct interactions: item 0
    has 72 users (a row longer than a wave), user 83 and items 27, 28 have none (empty rows), B = 64.  Item ids in `edges`,
    `pos`, `neg` are GLOBAL."""
    U, I, B, seed = 84, 29, 64, 2025
    rng = np.random.default_rng(seed)
    pairs = {(u, 0) for u in range(72)}
    for u in range(U - 1):
        for i in rng.choice(np.arange(1, 27), size=int(rng.integers(2, 5)), replace=False):
            pairs.add((u, int(i)))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    edges = np.stack([pairs[:, 0], pairs[:, 1] + U], 1)
    pick = rng.choice(len(edges), size=B, replace=False)
    pick[:3] = [k for k in range(len(edges)) if edges[k, 0] == 5][:1] * 3            # a user in three samples
    users, pos = edges[pick, 0].copy(), edges[pick, 1].copy()
    neg = U + rng.integers(0, I, B)
    neg[0] = pos[1]                                                                  # an item positive in one sample, negative in another
    return dict(U=U, I=I, B=B, seed=seed, edges=edges, users=users, pos=pos, neg=neg)


def graph_arrays(c):
    """The reference's normalised adjacency (Model/GraphAug.py:354-394) in row-major, column-ascending order: row, col int64
    [E], val float32 [E] (fp64 arithmetic, stored as fp32), tentry [E] (the entry of the reversed pair)."""
    U, I = c["U"], c["I"]
    N = U + I
    key = np.unique(c["edges"][:, 0] * I + (c["edges"][:, 1] - U))
    u, i = key // I, key % I
    deg = np.zeros(N)
    np.add.at(deg, u, 1.0)
    np.add.at(deg, U + i, 1.0)
    d = np.power(deg + 1e-7, -0.5)
    row, col = np.concatenate([u, U + i]), np.concatenate([U + i, u])
    order = np.argsort(row * N + col, kind="stable")
    row, col = row[order], col[order]
    val = ((d[row] * 1.0) * d[col]).astype(np.float32)
    pos = {(int(r), int(cc)): k for k, (r, cc) in enumerate(zip(row, col))}
    tentry = np.array([pos[(int(cc), int(r))] for r, cc in zip(row, col)], dtype=np.int64)
    return dict(N=N, E=len(row), row=row, col=col, val=val, tentry=tentry)


def draws(c, n_steps=1, seed_offset=1):
    """The draws of n_steps calls of loss(), in the reference's call order: rdm = (rdmUsrs, rdmItms1) int64 [100000], then per
    view six dropout keep masks bool [N, 200] (upper 0..2, bottom 0..2), u1 and u2 float32 [E] in [0, 1)."""
    g = graph_arrays(c)
    rng = np.random.default_rng(c["seed"] + seed_offset)
    out = []
    for _ in range(n_steps):
        rdm = (rng.integers(0, c["U"], N_RANDOM), rng.integers(0, c["I"], N_RANDOM))
        views = []
        for _ in range(2):
            masks = [rng.random((g["N"], H)) >= DROP for _ in range(6)]
            u1, u2 = (np.minimum(rng.random(g["E"]).astype(np.float32), np.float32(1 - ULP24)) for _ in range(2))
            u1[:2] = [0.0, 1 - ULP24]                     # both ends of torch.rand's range
            u2[:3] = [0.0, 1 - ULP24, 0.5]                # (clamp_probs moves the ends to 2^-23 and 1 - 2^-23)
            views.append(dict(masks=masks, u1=u1, u2=u2))
        out.append(dict(rdm=rdm, views=views))
    return out


def init_weights(c):
    """Replays the constructor's draws (same torch seed -> same weights as the reference class): name -> float32 array, the 14
    parameters and the bottom layers' six untrained tensors."""
    import torch.nn as nn
    torch.manual_seed(c["seed"])
    W = OrderedDict()
    W["uEmbeds"] = nn.init.xavier_uniform_(torch.empty(c["U"], DIM_E))
    W["iEmbeds"] = nn.init.xavier_uniform_(torch.empty(c["I"], DIM_E))
    for names, fan_in in ((UPPER, DIM_E), (BOTTOM, 3 * H)):
        for k in range(3):
            W[names[2 * k]] = nn.init.xavier_uniform_(torch.empty(fan_in, H))
            W[names[2 * k + 1]] = nn.init.xavier_uniform_(torch.empty(1, H))
    lins = [nn.Linear(3 * H, 2 * IB), nn.Linear(2 * DIM_E, DIM_E), nn.Linear(DIM_E, 1)]        # default init first ...
    for (wn, bn), lin in zip((FC, MLP[:2], MLP[2:]), lins):                                    # ... then init_emb over modules()
        W[wn] = nn.init.xavier_uniform_(lin.weight.data)
        W[bn] = lin.bias.data.fill_(0.0)
    return OrderedDict((n, v.detach().numpy().copy()) for n, v in W.items())


def load_fixture(golden_dir, name="graphaug_small.npz"):
    g = dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))
    for k in ("U", "I", "seed", "E"):
        g[k] = int(g[k])
    g["nonzero"] = np.unpackbits(g["nonzero_bits"])[:g["E"]].astype(bool)
    return g


# ---- the restated forward ------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self, c, dtype=torch.float64):
        g = graph_arrays(c)
        self.N, self.E, self.U, self.I = g["N"], g["E"], c["U"], c["I"]
        self.row, self.col = torch.from_numpy(g["row"]), torch.from_numpy(g["col"])
        self.val = torch.from_numpy(g["val"]).to(dtype)
        self.tentry = torch.from_numpy(g["tentry"])


def tensors(weights, dtype=torch.float64, requires_grad=True):
    return OrderedDict((n, torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(requires_grad and n in PARAMS)) for n, v in weights.items())


def spmm(G, val, x):
    return torch.zeros(G.N, x.shape[1], dtype=x.dtype).index_add(0, G.row, val[:, None] * x[G.col])


def leaky(x):
    return torch.where(x > 0, x, LEAKY * x)


def propagate(W, G, val, rdm=None):
    """Model/GraphAug.py:411-448 over the values `val` (+ the random entries: the coalesced sum's product)."""
    xs = [torch.cat([W["uEmbeds"], W["iEmbeds"]], 0)]
    for _ in range(N_LAYERS):
        y = spmm(G, val, xs[-1])
        if rdm is not None:
            r, cc = (torch.as_tensor(t) for t in rdm)
            y = y + torch.zeros_like(y).index_add(0, r, RANDOM_VALUE * xs[-1][cc])
        xs.append(leaky(y))
    return sum(xs)


def mixhop(W, G, x, masks, training=True):
    """Model/GraphAug.py:225-244 -> node_emb [N, 64]."""
    def drop(h, m):
        return h * (torch.as_tensor(m).to(h.dtype) / (1.0 - DROP)) if training else h

    def hops(h, n):
        for _ in range(n):
            h = spmm(G, G.val, h)
        return h
    up = [hops(torch.relu(drop(x @ W[UPPER[2 * k]] + W[UPPER[2 * k + 1]], masks[k])), k) for k in range(3)]
    a1 = torch.cat(up, 1)
    low = [hops(drop(a1 @ W[BOTTOM[2 * k]], masks[3 + k]), k) + W[BOTTOM[2 * k + 1]] for k in range(3)]
    return torch.cat(low, 1) @ W[FC[0]].t() + W[FC[1]]


def edge_logits(W, G, z):
    """Model/GraphAug.py:290-295 per edge -> [E]."""
    emb = torch.cat([z[G.row], z[G.col]], 1)
    return (torch.relu(emb @ W[MLP[0]].t() + W[MLP[1]]) @ W[MLP[2]].t() + W[MLP[3]])[:, 0]


def sample(logit, u1, u2):
    """Model/GraphAug.py:297-308 and :268-283 (RelaxedBernoulli(0.9, probs).rsample() written out) -> dict(att, s, val)."""
    dt = logit.dtype
    u1, u2 = torch.as_tensor(u1).to(dt), torch.as_tensor(u2).to(dt)
    bias = 0.0001
    eps = (bias - (1 - bias)) * u1 + (1 - bias)
    w = torch.sigmoid(torch.log(eps) - torch.log(1 - eps) + logit)
    att = torch.clamp(w, 0.01, 0.99)
    uc = torch.clamp(u2, P_LO, P_HI)
    probs = torch.clamp(att, P_LO, P_HI)
    x = (uc.log() - (-uc).log1p() + probs.log() - (-probs).log1p()) / torch.tensor([0.9], dtype=torch.float32).to(dt)
    s = torch.clamp(torch.sigmoid(x), TINY, P_HI)
    return dict(att=att, s=s, val=torch.where(s > 0.2, s, torch.zeros_like(s)))


def contrast(e1, e2, nodes, temp):
    n1 = e1 / e1.norm(dim=1, keepdim=True).clamp_min(1e-12)
    n2 = e2 / e2.norm(dim=1, keepdim=True).clamp_min(1e-12)
    p1, p2 = n1[nodes], n2[nodes]
    nume = torch.exp((p1 * p2).sum(-1) / temp)
    deno = torch.exp(p1 @ n2.t() / temp).sum(-1)
    return -torch.log(nume / deno).mean()


def step(W, c, dr, G=None, training=True):
    """loss() on the weights W (tensors()) and the draws dr -> dict(loss, bpr, reg, cl, kl, node_emb [2][N, 64], logits, s, val
    (per view))."""
    dt = W["uEmbeds"].dtype
    G = Graph(c, dt) if G is None else G
    U = c["U"]
    users, pos, neg = (torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))
    pos, neg = pos - U, neg - U
    ofea = propagate(W, G, G.val)
    out = dict(node_emb=[], logits=[], s=[], val=[], att=[])
    for v in dr["views"]:
        node_emb = mixhop(W, G, ofea, v["masks"], training)
        lg = edge_logits(W, G, node_emb.detach())
        sm = sample(lg, v["u1"], v["u2"])
        out["node_emb"].append(node_emb)
        out["logits"].append(lg.detach())
        for k in ("s", "val", "att"):
            out[k].append(sm[k].detach())
    ne = torch.stack(out["node_emb"], 0).mean(0)
    mu, std = ne[:, :IB], torch.nn.functional.softplus(ne[:, IB:] - IB, beta=1)
    kl = -0.5 * (1 + 2 * std.log() - mu.pow(2) - std.pow(2)).sum(1).mean() / math.log(2)
    main = propagate(W, G, G.val)
    v1, v2 = (propagate(W, G, val, dr["rdm"]) for val in out["val"])
    ue, ie = main[:U], main[U:]
    bpr = -torch.mean(torch.log(torch.sigmoid((ue[users] * ie[pos]).sum(1) - (ue[users] * ie[neg]).sum(1)) + 1e-5))
    reg = REG_WEIGHT * ((W["uEmbeds"][users] ** 2).mean() + (W["iEmbeds"][pos] ** 2).mean() + (W["iEmbeds"][neg] ** 2).mean())
    cl = (contrast(v1[:U], v2[:U], users, SSL_TEMP) + contrast(v1[U:], v2[U:], pos, SSL_TEMP)) * SSL_ALPHA
    out.update(loss=bpr + reg + cl + 0.00001 * kl, bpr=bpr, reg=reg, cl=cl, kl=kl)
    return out


def step_with_grads(weights, c, dr, dtype=torch.float64):
    """-> (step()'s dict with floats for the loss parts, grads: name -> array over WITH_GRAD)"""
    W = tensors(weights, dtype)
    out = step(W, c, dr)
    out["loss"].backward()
    grads = {n: W[n].grad.numpy().copy() for n in WITH_GRAD}
    assert all(W[n].grad is None for n in MLP)
    for k in ("loss",) + PARTS:
        out[k] = float(out[k].detach())
    return out, grads


def trajectory(weights, c, drs, dtype=torch.float64):
    """train_and_evaluate.py:41-47 with Adam(lr) over the 14 parameters, one batch repeated -> (final weights, losses)."""
    W = tensors(weights, dtype)
    opt = torch.optim.Adam([W[n] for n in PARAMS], lr=LR)
    losses = []
    for dr in drs:
        opt.zero_grad()
        loss = step(W, c, dr)["loss"]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return {n: W[n].detach().numpy().copy() for n in PARAMS}, losses


def ranklist(weights, c, topk=TOPK, dtype=torch.float64):
    W = tensors(weights, dtype, requires_grad=False)
    U = c["U"]
    main = propagate(W, Graph(c, dtype), Graph(c, dtype).val)
    score = main[:U] @ main[U:].t()
    for u, items in user_item_dict(c["edges"]).items():
        score[u, torch.tensor(items) - U] = 1e-6
    return (torch.topk(score, topk).indices + U).numpy()


def lse_host(A, T, inv_temp, g=None, dtype=torch.float64):
    """lse[b] = log sum_m exp(<A_b, T_m> inv_temp) by the reference's lines (no max-subtraction) and, for g [B], both
    gradients of sum_b g_b lse_b -> (lse, gA, gT) as arrays."""
    A = torch.tensor(np.asarray(A), dtype=dtype).requires_grad_(True)
    T = torch.tensor(np.asarray(T), dtype=dtype).requires_grad_(True)
    lse = torch.log(torch.exp(A @ T.t() * inv_temp).sum(-1))
    if g is None:
        return lse.detach().numpy(), None, None
    (lse * torch.tensor(np.asarray(g), dtype=dtype)).sum().backward()
    return lse.detach().numpy(), A.grad.numpy(), T.grad.numpy()


def sampler_case(c, scale=6.0):
    """The sampler alone at weights the golden has no run of: node rows z [N, 64] and the edge MLP with its rows scaled so that
    the logits span about +-10 -- both `att` clamps are then taken by the logit as well as by the noise, and s falls on both
    sides of 0.2.  -> (W dict of float32 arrays under the MLP's names, z float32, u1, u2 float32 [E])."""
    g = graph_arrays(c)
    rng = np.random.default_rng(c["seed"] + 77)
    z = rng.standard_normal((g["N"], D)).astype(np.float32)
    W = {MLP[0]: (scale * rng.standard_normal((D, 2 * D)) / np.sqrt(2 * D)).astype(np.float32),
         MLP[1]: (0.5 * rng.standard_normal(D)).astype(np.float32),
         MLP[2]: (rng.standard_normal((1, D)) / np.sqrt(D)).astype(np.float32),
         MLP[3]: np.array([0.25], dtype=np.float32)}
    v = draws(c, 1, seed_offset=5)[0]["views"][0]
    return W, z, v["u1"], v["u2"]


def sampler_host(W, G, z, u1, u2, dtype=torch.float64):
    """-> dict(logits, att, s, val) as arrays, the restated lines at `dtype`."""
    Wt = {n: torch.tensor(v, dtype=dtype) for n, v in W.items()}
    lg = edge_logits(Wt, G, torch.tensor(z, dtype=dtype))
    out = sample(lg, u1, u2)
    out["logits"] = lg
    return {k: v.numpy() for k, v in out.items()}


def flip_band(s32, s64):
    """delta = 4 x the measured fp32-vs-float64 deviation of s: an entry whose float64 s lies within delta of 0.2 may fall on
    either side.  -> (delta, mask of those entries)"""
    delta = 4 * float(np.abs(np.asarray(s32, dtype=np.float64) - s64).max())
    return delta, np.abs(s64 - 0.2) < delta


def lse_case(B, M, seed=0):
    """Normalised rows A [B, 64], T [M, 64] with A[0] = T[min(3, M - 1)] (cosine 1: the largest term e^inv_temp is present),
    g [B]."""
    rng = np.random.default_rng(1000 + 131 * B + M + seed)
    A, T = rng.standard_normal((B, D)), rng.standard_normal((M, D))
    A, T = A / np.linalg.norm(A, axis=1, keepdims=True), T / np.linalg.norm(T, axis=1, keepdims=True)
    T, A = T.astype(np.float32), A.astype(np.float32)
    A[0] = T[min(3, M - 1)]
    return A, T, rng.standard_normal(B).astype(np.float32)
