"""Host restatement of what Model/AdaGCL.py computes, in float64 torch, following the reference's order of operations: the
two view generators (the per-edge keep MLP; the hard-concrete edge gate in both forms, written per EDGE as the reference
does, so that the kernels' per-node factorisation is checked against something else), the four losses of a training step
with their gradients (float64 autograd over the restated forward), and the training loop with its three Adam optimizers.
Also the synthetic case, the draws (GIVEN everywhere: a float32 table per torch.randn call, a float32 vector per
np.random.uniform call) and the constructor's weight draws.  Imported by test_adagcl_host.py, test_gpu_adagcl.py and
golden/gen_adagcl.py."""
import os
from collections import OrderedDict

import numpy as np
import torch
from accept import rel_dev, user_item_dict  # noqa: F401

D = 64
DIM_E, REG_WEIGHT, N_LAYERS, SSL_TEMP, SSL_ALPHA, LR = 64, 0.001, 2, 0.5, 0.1, 0.001
IB_REG, LAMBDA0, GAMMA, ZETA = 0.01, 0.0001, -0.45, 1.05
TOPK = 10
N_STEPS = 3

NAMES = ("uEmbeds", "iEmbeds") + tuple(
    f"generator_1.encoder.{m}.{k}.{p}" for m in ("encoder_mean", "encoder_std") for k in (0, 2) for p in ("weight", "bias")) + tuple(
    f"generator_1.decoder.decoder.{k}.{p}" for k in (1, 3) for p in ("weight", "bias")) + tuple(
    f"generator_2.{m}.0.{p}" for m in ("nblayers_0", "nblayers_1", "selflayers_0", "selflayers_1", "attentions_0", "attentions_1")
    for p in ("weight", "bias"))                                                                                # state_dict() order: 26
ENCODER = tuple(n for n in NAMES if n.startswith("generator_1.encoder."))
GEN_2 = tuple(n for n in NAMES if n.startswith("generator_2."))
GEN_1 = tuple(n for n in NAMES if n.startswith("generator_1."))
LOSSES = ("loss_1", "loss_2", "bpr_reg_loss", "gen_loss")
# the parameters each loss alone reaches (the generators' views are generated without gradient)
WITH_GRAD = {"loss_1": NAMES[:2], "loss_2": NAMES[:2], "bpr_reg_loss": NAMES[:2], "gen_loss": NAMES}


def small_case():
    """83 users, 29 items, about 300 distinct interactions (E about 600: no multiple of 64 or 128): item 0 has 72 users (a row
    longer than a wave), items 27 and 28 have none (empty rows), B = 64.  Item ids in `edges`, `pos`, `neg` are GLOBAL."""
    U, I, B, seed = 83, 29, 64, 2024
    rng = np.random.default_rng(seed)
    pairs = {(u, 0) for u in range(72)}
    for u in range(U):
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
    """The reference's normalised adjacency (Model/AdaGCL.py:65-105) in row-major, column-ascending order: row, col int64 [E],
    val float32 [E] (fp64 arithmetic, stored as fp32, as scipy's path does), tentry [E] (the entry of the reversed pair)."""
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
    """The draws of n_steps training steps, as float32: per step three normal tables [N, 64] (loss_1's and loss_2's view of
    generator 1, gen_loss's encoder) and N_LAYERS uniform vectors [E] in [1e-7, 1 - 1e-7] (gen_loss's DenoisingNet.call)."""
    g = graph_arrays(c)
    rng = np.random.default_rng(c["seed"] + seed_offset)
    out = []
    for _ in range(n_steps):
        randn = [rng.standard_normal((g["N"], D)).astype(np.float32) for _ in range(3)]
        u = [np.clip(rng.uniform(1e-7, 1.0 - 1e-7, g["E"]).astype(np.float32), np.float32(1e-7), np.float32(1.0 - 1e-7)) for _ in range(N_LAYERS)]
        u[0][:4] = [np.float32(1e-7), np.float32(1.0 - 1e-7), 0.5, 0.25]             # both ends of the range
        out.append(dict(randn=randn, u=u))
    return out


def init_weights(c):
    """Replays the constructor's draws (same torch seed -> same weights as the reference class): name -> float32 array."""
    import torch.nn as nn
    torch.manual_seed(c["seed"])
    W = OrderedDict()
    W["uEmbeds"] = nn.init.xavier_uniform_(torch.empty(c["U"], DIM_E))
    W["iEmbeds"] = nn.init.xavier_uniform_(torch.empty(c["I"], DIM_E))
    shapes = [(DIM_E, DIM_E)] * 5 + [(DIM_E, 1)] + [(DIM_E, DIM_E)] * 4 + [(2 * DIM_E, 1)] * 2
    lin_names = [n[:-len(".weight")] for n in NAMES[2:] if n.endswith(".weight")]
    for name, (fan_in, fan_out) in zip(lin_names, shapes):
        lin = nn.Linear(fan_in, fan_out)
        W[name + ".weight"], W[name + ".bias"] = lin.weight.detach(), lin.bias.detach()
    assert tuple(W) == NAMES
    return OrderedDict((n, v.numpy().copy()) for n, v in W.items())


def load_fixture(golden_dir, name="adagcl_small.npz"):
    g = dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))
    for k in ("U", "I", "seed", "E"):
        g[k] = int(g[k])
    g["keep"] = np.unpackbits(g["keep_bits"])[:g["E"]].astype(bool)
    return g


# ---- the restated forward (torch, any dtype; float64 is the yardstick) ----------------------------------------------------
class Graph:
    def __init__(self, c, dtype=torch.float64, arrays=None):
        """The small case's graph, or arrays = dict(N, E, row, col, val, tentry) of any symmetric pattern."""
        g = graph_arrays(c) if arrays is None else arrays
        self.N, self.E = g["N"], g["E"]
        self.U, self.I = (c["U"], c["I"]) if c is not None else (g["N"], 0)
        self.row, self.col = torch.from_numpy(g["row"]), torch.from_numpy(g["col"])
        self.val = torch.from_numpy(g["val"]).to(dtype)
        self.tentry = torch.from_numpy(g["tentry"])


def tensors(weights, dtype=torch.float64, requires_grad=True):
    return OrderedDict((n, torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(requires_grad)) for n, v in weights.items())


def spmm(G, val, x):
    return torch.zeros(G.N, x.shape[1], dtype=x.dtype).index_add(0, G.row, val[:, None] * x[G.col])


def _lin(W, name, x):
    return x @ W[name + ".weight"].t() + W[name + ".bias"]


def graphcl(W, G, val, n_layers=N_LAYERS):
    xs = [torch.cat([W["uEmbeds"], W["iEmbeds"]], 0)]
    for _ in range(n_layers):
        xs.append(spmm(G, val, xs[-1]))
    return sum(xs)


def encoder(W, G, val, noise):
    x = graphcl(W, G, val)
    p = "generator_1.encoder."
    mean = _lin(W, p + "encoder_mean.2", torch.relu(_lin(W, p + "encoder_mean.0", x)))
    std = torch.nn.functional.softplus(_lin(W, p + "encoder_std.2", torch.relu(_lin(W, p + "encoder_std.0", x))))
    return noise * std + mean, mean, std


def decoder_logit(W, rows):
    p = "generator_1.decoder.decoder."
    return _lin(W, p + "3", torch.relu(_lin(W, p + "1", torch.relu(rows))))


def keep_view(W, G, noise):
    """vgae.generate -> (values [E] over the fixed pattern, keep bool [E], logits [E])."""
    x, _, _ = encoder(W, G, G.val, noise)
    return keep_from_rows(W, G, x)


def keep_from_rows(W, G, x):
    logits = decoder_logit(W, x[G.row] * x[G.col])[:, 0]
    keep = (torch.sigmoid(logits) + 0.5).floor().to(torch.bool)
    kept = int(keep.sum())
    vals = torch.zeros_like(G.val)
    if kept:
        vals[keep] = G.val[keep] / (kept / G.E)
    return vals, keep, logits


def gate(W, G, x, layer, beta, training, u=None, retain_logit_grad=False):
    """DenoisingNet's per-EDGE lines (get_attention, hard_concrete_sample, the normalisation, l0_norm) -> dict."""
    p = "generator_2."
    h1 = torch.relu(_lin(W, f"{p}nblayers_{layer}.0", x[G.row]))
    h2 = torch.relu(_lin(W, f"{p}selflayers_{layer}.0", x[G.col]))
    logit = _lin(W, f"{p}attentions_{layer}.0", torch.cat([h1, h2], 1))[:, 0]
    if retain_logit_grad:
        logit = logit.detach().requires_grad_()      # a leaf: its .grad is the cotangent of every entry's logit
    if training:
        # the reference's draw is a float64 numpy array: the sum, the sigmoid, the stretch and the clamp run in float64 whatever
        # the weights' dtype, and the mask is rounded once (.float())
        un = torch.as_tensor(np.asarray(u, dtype=np.float64))
        g = torch.sigmoid((torch.log(un) - torch.log(1.0 - un) + logit) / beta)
    else:
        g = torch.sigmoid(logit)
    stretched = g * (ZETA - GAMMA) + GAMMA
    m = torch.clamp(stretched, 0.0, 1.0).to(x.dtype)
    S = torch.zeros(G.N, dtype=x.dtype).index_add(0, G.row, m) + (1e-6 if training else 0.0)
    d = torch.clamp(torch.pow(S, -0.5), 0.0, 10.0)
    val = m * d[G.row] * d[G.col]
    l0 = torch.mean(torch.sigmoid(logit - beta * float(np.log(np.float64(-GAMMA) / np.float64(ZETA)))))
    return dict(logit=logit, stretched=stretched, m=m, S=S, d=d, val=val, l0=l0)


def graphcl_generated(W, G, n_layers=N_LAYERS):
    """forward_graphcl_ with generator 2's evaluation-form views (generated without gradient)."""
    xs = [torch.cat([W["uEmbeds"], W["iEmbeds"]], 0)]
    for layer in range(n_layers):
        with torch.no_grad():
            val = gate(W, G, xs[-1], layer, 1.0, False)["val"]
        xs.append(spmm(G, val, xs[-1]))
    return sum(xs)


def loss_graphcl(G, x1, x2, users, items, T=SSL_TEMP):
    F = torch.nn.functional
    u1, i1 = F.normalize(x1[:G.U], dim=1), F.normalize(x1[G.U:], dim=1)
    u2, i2 = F.normalize(x2[:G.U], dim=1), F.normalize(x2[G.U:], dim=1)
    a1, a2 = torch.cat([u1[users], i1[items]], 0), torch.cat([u2[users], i2[items]], 0)
    sim = torch.exp((a1 @ a2.t()) / torch.outer(a1.norm(dim=1), a2.norm(dim=1)) / T)
    pos = torch.diagonal(sim)
    return -torch.log(pos / (sim.sum(1) - pos))


def _bpr(xu, xi, users, pos, neg):
    a, p, n = xu[users], xi[pos], xi[neg]
    return -torch.mean(torch.log(torch.sigmoid((a * p).sum(1) - (a * n).sum(1)) + 1e-5))


def _reg(W, names):
    return sum(W[n].norm(2).square() for n in names)


def _views(W, G, noise):
    with torch.no_grad():
        vals = keep_view(W, G, noise)[0]
    return graphcl(W, G, vals), graphcl_generated(W, G)


def loss_1(W, G, users, pos, noise):
    out1, out2 = _views(W, G, noise)
    return loss_graphcl(G, out1, out2, users, pos).mean() * SSL_ALPHA, out1, out2


def loss_2(W, G, users, pos, noise, out1, out2):
    o1, o2 = _views(W, G, noise)
    return (loss_graphcl(G, o1, out1.detach(), users, pos) + loss_graphcl(G, o2, out2.detach(), users, pos)).mean() * IB_REG


def bpr_reg_loss(W, G, users, pos, neg):
    x = graphcl(W, G, G.val)
    reg = REG_WEIGHT * ((W["uEmbeds"][users] ** 2).mean() + (W["iEmbeds"][pos] ** 2).mean() + (W["iEmbeds"][neg] ** 2).mean())
    return _bpr(x[:G.U], x[G.U:], users, pos, neg) + reg


def gen_loss(W, G, features, users, pos, neg, noise, u):
    x, mean, std = encoder(W, G, G.val, noise)
    xu, xi = x[:G.U], x[G.U:]
    pp = torch.sigmoid(decoder_logit(W, xu[users] * xi[pos]))
    pn = torch.sigmoid(decoder_logit(W, xu[users] * xi[neg]))
    loss_rec = -torch.clamp(torch.log(pp), min=-100.0) - torch.clamp(torch.log(1.0 - pn), min=-100.0)        # [B, 1]
    kl = -0.5 * (1 + 2 * torch.log(std) - mean ** 2 - std ** 2).sum(1)
    l1 = (loss_rec + 0.1 * kl.mean() + _bpr(xu, xi, users, pos, neg) + _reg(W, ENCODER) * REG_WEIGHT).mean()
    xs, l0 = [features], 0.0
    for layer in range(N_LAYERS):
        g = gate(W, G, xs[-1], layer, SSL_TEMP, True, u[layer])
        l0 = l0 + g["l0"]
        xs.append(spmm(G, g["val"], xs[-1]))
    z = sum(xs)
    l2 = _bpr(z[:G.U], z[G.U:], users, pos, neg) + _reg(W, GEN_2) * REG_WEIGHT + l0 * LAMBDA0
    return l1 + l2


def _ids(c):
    U = c["U"]
    return (torch.from_numpy(np.asarray(c["users"])).long(), torch.from_numpy(np.asarray(c["pos"]) - U).long(),
            torch.from_numpy(np.asarray(c["neg"]) - U).long())


def _grads(W, loss, names):
    gs = torch.autograd.grad(loss, [W[n] for n in names], allow_unused=True)
    return OrderedDict((n, (g if g is not None else torch.zeros_like(W[n])).numpy().copy()) for n, g in zip(names, gs))


def step_losses(weights, c, dr, features=None, dtype=torch.float64):
    """The four losses of one step on FIXED weights (no optimizer step between them) and the gradient each alone produces."""
    G, W = Graph(c, dtype), tensors(weights, dtype)
    users, pos, neg = _ids(c)
    feats = torch.tensor(np.concatenate([weights["uEmbeds"], weights["iEmbeds"]], 0) if features is None else features, dtype=dtype)
    noise = [torch.tensor(t, dtype=dtype) for t in dr["randn"]]
    out = {"grads": {}}
    l1, out1, out2 = loss_1(W, G, users, pos, noise[0])
    l2 = loss_2(W, G, users, pos, noise[1], out1, out2)
    l3 = bpr_reg_loss(W, G, users, pos, neg)
    l4 = gen_loss(W, G, feats, users, pos, neg, noise[2], dr["u"])
    for name, l in zip(LOSSES, (l1, l2, l3, l4)):
        out[name] = float(l.detach())
        out["grads"][name] = _grads(W, l, WITH_GRAD[name])
    return out


def trajectory(weights, c, drs, dtype=torch.float64):
    """The reference's loop (train_and_evaluate.py:72-97) over the same batch len(drs) times -> (final weights, the losses)."""
    G, W = Graph(c, dtype), tensors(weights, dtype)
    users, pos, neg = _ids(c)
    feats = torch.tensor(np.concatenate([weights["uEmbeds"], weights["iEmbeds"]], 0), dtype=dtype)
    opt = torch.optim.Adam(list(W.values()), lr=LR, weight_decay=0)
    opt_1 = torch.optim.Adam([W[n] for n in GEN_1], lr=LR, weight_decay=0)
    opt_2 = torch.optim.Adam([W[n] for n in GEN_2], lr=LR, weight_decay=0, eps=0.001)
    losses = []
    for dr in drs:
        noise = [torch.tensor(t, dtype=dtype) for t in dr["randn"]]
        for o in (opt, opt_1, opt_2):
            o.zero_grad()
        l1, out1, out2 = loss_1(W, G, users, pos, noise[0])
        l1.backward()
        opt.step()
        opt.zero_grad()
        l2 = loss_2(W, G, users, pos, noise[1], out1, out2)
        l2.backward()
        opt.step()
        opt.zero_grad()
        l3 = bpr_reg_loss(W, G, users, pos, neg)
        l3.backward()
        l4 = gen_loss(W, G, feats, users, pos, neg, noise[2], dr["u"])
        l4.backward()
        opt.step()
        opt_1.step()
        opt_2.step()
        losses.append([float(x.detach()) for x in (l1, l2, l3, l4)])
    return OrderedDict((n, v.detach().numpy().copy()) for n, v in W.items()), np.array(losses)


def rank_scores(weights, c, dtype=torch.float64):
    """gene_ranklist's score matrix [U, I] (history entries 1e-6)."""
    G, W = Graph(c, dtype), tensors(weights, dtype, False)
    x = graphcl(W, G, G.val)
    s = (x[:G.U] @ x[G.U:].t()).numpy().copy()
    for u, items in user_item_dict(c["edges"]).items():
        s[u, np.asarray(items) - c["U"]] = 1e-6
    return s


def scaled_gate_weights(weights, scale_att=60.0):
    """A weight set whose gate logits span about [-6, 6] on the small case: the attention rows scaled."""
    w = OrderedDict((n, np.array(v, copy=True)) for n, v in weights.items())
    for layer in (0, 1):
        w[f"generator_2.attentions_{layer}.0.weight"] = (w[f"generator_2.attentions_{layer}.0.weight"] * scale_att).astype(np.float32)
    return w


def gate_backward(W, G, x, layer, beta, training, u, g_val, g_l0):
    """The cotangents of the two node scores and the bias under sum(g_val * val) + g_l0 * l0, from autograd over the per-EDGE
    lines: g_logit summed by row (s_nb), by column (s_self) and over all entries (b).  -> (g_s_nb, g_s_self, g_b, stretched)."""
    out = gate(W, G, x, layer, beta, training, u, retain_logit_grad=True)
    dt = out["val"].dtype
    ((torch.as_tensor(g_val, dtype=dt) * out["val"]).sum() + float(g_l0) * out["l0"]).backward()
    gl = out["logit"].grad
    z = torch.zeros(G.N, dtype=gl.dtype)
    return (z.index_add(0, G.row, gl).numpy(), z.index_add(0, G.col, gl).numpy(), float(gl.sum()), out["stretched"].detach().numpy())


def gate_case(c, weights, scaled):
    """(weights, x float32 [N, 64], the row whose masks are all 0 or None) for the gate tests.  scaled: the attention rows times
    60 -- logits span about [-6, 6], both clamps are taken -- and user 7's row of x replaced by the one of 4 000 candidates
    that makes its s_nb smallest in both layers: every mask of that row is 0 in both forms."""
    x = np.concatenate([weights["uEmbeds"], weights["iEmbeds"]], 0).copy()
    if not scaled:
        return weights, x, None
    w = scaled_gate_weights(weights)
    rng = np.random.default_rng(c["seed"] + 7)
    cand = (0.6 * rng.standard_normal((4000, D))).astype(np.float32)
    score = []
    for layer in (0, 1):
        h = np.maximum(cand.astype(np.float64) @ w[f"generator_2.nblayers_{layer}.0.weight"].T.astype(np.float64)
                       + w[f"generator_2.nblayers_{layer}.0.bias"], 0.0)
        score.append(h @ w[f"generator_2.attentions_{layer}.0.weight"][0, :D].astype(np.float64))
    x[7] = cand[int(np.argmin(np.maximum(score[0], score[1])))]
    return w, x, 7
