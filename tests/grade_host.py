"""Host restatement of what Model/Grade.py computes, in float64 torch, following the reference's order of operations: the
three vgae view generators (the per-edge MLP, the keep decision, the weighted renormalisation -- written per stored EDGE, both
directions of a pair on their own, as the reference does, so that the kernels' once-per-pair decision is checked against
something else), the three losses of a training step with their gradients (float64 autograd over the restated forward), and
the training loop with its four Adam optimizers.  Also the synthetic case, the draws (GIVEN everywhere: a float32 table per
torch.randn / torch.rand call) and the constructor's weight draws.  Imported by test_grade_host.py, test_gpu_grade.py and
golden/gen_grade.py."""
import os
from collections import OrderedDict

import numpy as np
import torch
from accept import rel_dev, user_item_dict  # noqa: F401

D = 64
DIM_E, REG_WEIGHT, N_LAYERS, SSL_TEMP, SSL_ALPHA, SSL_TEMP2, NOISE_ALPHA, LR = 64, 0.1, 2, 0.3, 0.2, 0.3, 0.2, 0.001
KNN_K, MM_IMAGE_WEIGHT = 10, 0.5
FV, FT = 128, 96
TOPK = 10
N_STEPS = 3
FIRST_SEED = 1
STORED_ROWS = 8

EMB = ("uEmbeds.weight", "utEmbeds.weight", "uvEmbeds.weight", "iEmbeds.weight")
FROZEN = ("v_feat.weight", "t_feat.weight")
TRS = ("image_trs.weight", "image_trs.bias", "text_trs.weight", "text_trs.bias")


def _gen_names(g):
    return tuple(f"generator_{g}.encoder.{m}.{k}.{p}" for m in ("encoder_mean", "encoder_std") for k in (0, 2) for p in ("weight", "bias")) + tuple(
        f"generator_{g}.decoder.decoder.{k}.{p}" for k in (1, 3) for p in ("weight", "bias"))


GEN = {g: _gen_names(g) for g in (1, 2, 3)}
NAMES = EMB + FROZEN + TRS + GEN[1] + GEN[2] + GEN[3]                                   # state_dict() order: 46
LOSSES = ("loss_1", "bpr_reg_loss", "gen_loss")
# the parameters each loss alone reaches (loss_1's views are generated without gradient; the feature tables are frozen)
WITH_GRAD = {"loss_1": EMB + TRS, "bpr_reg_loss": EMB, "gen_loss": EMB + TRS + GEN[1] + GEN[2] + GEN[3]}


def stored(name, x):
    """What the golden keeps of a gradient or a trained tensor: all of it, but of the fifteen 64 x 64 Linear weights and the two
    projections only the first STORED_ROWS rows (the file stays well under the size limit); every deviation next to it was
    measured over the whole tensor."""
    x = np.asarray(x)
    return x[:STORED_ROWS] if name.endswith(".weight") and x.ndim == 2 and x.shape[0] == DIM_E and name not in EMB else x


def small_case(seed=FIRST_SEED):
    """90 users, 72 items, about 725 distinct interactions (E about 1 450; neither E nor E / 2 a multiple of 64): user 0 has 70
    items (a row longer than a wave), items 70 and 71 have no user (empty rows), feature widths 128 and 96, B = 64.  Item ids
    in `edges`, `pos`, `neg` are GLOBAL.  The graph, the features and the batch are fixed; `seed` is the torch seed of the
    weights and the key of the draws."""
    U, I, B = 90, 72, 64
    rng = np.random.default_rng(2025)
    pairs = {(0, i) for i in range(70)}
    for u in range(1, U):
        for i in rng.choice(np.arange(0, 70), size=int(rng.integers(6, 10)), replace=False):
            pairs.add((u, int(i)))
    while len(pairs) % 64 == 0 or len(pairs) % 32 == 0:
        pairs.add((1, int(min(set(range(70)) - {i for u, i in pairs if u == 1}))))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    edges = np.stack([pairs[:, 0], pairs[:, 1] + U], 1)
    pick = rng.choice(len(edges), size=B, replace=False)
    pick[:3] = [k for k in range(len(edges)) if edges[k, 0] == 5][:1] * 3            # a user in three samples
    users, pos = edges[pick, 0].copy(), edges[pick, 1].copy()
    neg = U + rng.integers(0, I, B)
    neg[0] = pos[1]                                                                  # an item positive in one sample, negative in another
    v_feat = rng.standard_normal((I, FV)).astype(np.float32)
    t_feat = rng.standard_normal((I, FT)).astype(np.float32)
    return dict(U=U, I=I, B=B, seed=int(seed), edges=edges, users=users, pos=pos, neg=neg, v_feat=v_feat, t_feat=t_feat)


def knn_arrays(feat, k=KNN_K):
    """The reference's kNN item graph (Model/Grade.py:295-326) in float32: (row, col int64 [I k], val float32 [I k])."""
    x = torch.from_numpy(np.asarray(feat, dtype=np.float32))
    xn = x.div(torch.norm(x, p=2, dim=-1, keepdim=True))
    ind = torch.topk(xn @ xn.t(), k, dim=-1)[1]
    n = x.shape[0]
    row = torch.arange(n).unsqueeze(1).expand(-1, k).reshape(-1)
    col = ind.reshape(-1)
    r = torch.pow(1e-7 + torch.bincount(row, minlength=n).float(), -0.5)
    return row.numpy(), col.numpy(), (r[row] * r[col]).numpy()


def graph_arrays(c):
    """The reference's normalised adjacency (Model/Grade.py:248-288) in row-major, column-ascending order: row, col int64 [E],
    val float32 [E] (fp64 arithmetic, stored as fp32, as scipy's path does), tentry [E] (the entry of the reversed pair); and
    its item-item graph mm_adj = 0.5 image + 0.5 text, coalesced: mm_row, mm_col, mm_val float32."""
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
    (ir, ic, iv), (tr, tc, tv) = knn_arrays(c["v_feat"]), knn_arrays(c["t_feat"])
    mk = np.concatenate([ir * I + ic, tr * I + tc])
    mv = np.concatenate([np.float32(MM_IMAGE_WEIGHT) * iv, np.float32(1.0 - MM_IMAGE_WEIGHT) * tv]).astype(np.float32)
    uniq, inv = np.unique(mk, return_inverse=True)
    mm_val = np.zeros(len(uniq), np.float32)
    np.add.at(mm_val, inv, mv)
    return dict(N=N, E=len(row), row=row, col=col, val=val, tentry=tentry, mm_row=uniq // I, mm_col=uniq % I, mm_val=mm_val)


def draws(c, n_steps=1, seed_offset=1):
    """The draws of n_steps training steps, as float32 [N, 64] tables: per step `randn1` (the three encoders of loss_1's views),
    `rand` (the two noise forwards' uniform tables) and `randn2` (the three encoders of gen_loss)."""
    N = c["U"] + c["I"]
    rng = np.random.default_rng(1000 * c["seed"] + seed_offset)
    out = []
    for _ in range(n_steps):
        out.append(dict(randn1=[rng.standard_normal((N, D)).astype(np.float32) for _ in range(3)],
                        rand=[rng.random((N, D), dtype=np.float32) for _ in range(2)],
                        randn2=[rng.standard_normal((N, D)).astype(np.float32) for _ in range(3)]))
    return out


def init_weights(c):
    """Replays the constructor's draws (same torch seed -> same weights as the reference class): name -> float32 array."""
    import torch.nn as nn
    torch.manual_seed(c["seed"])
    W = OrderedDict()
    for n, rows in zip(EMB, (c["U"], c["U"], c["U"], c["I"])):
        emb = nn.Embedding(rows, DIM_E)               # draws its normal table first
        W[n] = nn.init.xavier_uniform_(emb.weight).detach()
    W["v_feat.weight"], W["t_feat.weight"] = torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"])
    for name, fan_in in (("image_trs", FV), ("text_trs", FT)):
        lin = nn.Linear(fan_in, DIM_E)
        W[name + ".weight"], W[name + ".bias"] = lin.weight.detach(), lin.bias.detach()
    for g in (1, 2, 3):
        lin_names = [n[:-len(".weight")] for n in GEN[g] if n.endswith(".weight")]
        for name, fan_out in zip(lin_names, [DIM_E] * 5 + [1]):
            lin = nn.Linear(DIM_E, fan_out)
            W[name + ".weight"], W[name + ".bias"] = lin.weight.detach(), lin.bias.detach()
    assert tuple(W) == NAMES
    return OrderedDict((n, v.numpy().copy()) for n, v in W.items())


def load_fixture(golden_dir, name="grade_small.npz"):
    g = dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))
    for k in ("U", "I", "seed", "E"):
        g[k] = int(g[k])
    g["keep"] = np.stack([np.unpackbits(g["keep_bits"][k])[:g["E"]].astype(bool) for k in range(3)])
    return g


# ---- the restated forward (torch, any dtype; float64 is the yardstick) ----------------------------------------------------
class Graph:
    def __init__(self, c, dtype=torch.float64, arrays=None):
        """The small case's graph, or arrays = dict(N, E, row, col, val, tentry[, mm_row, mm_col, mm_val]) of any symmetric pattern."""
        g = graph_arrays(c) if arrays is None else arrays
        self.N, self.E = g["N"], g["E"]
        self.U, self.I = (c["U"], c["I"]) if c is not None else (g["N"], 0)
        self.row, self.col = torch.from_numpy(np.asarray(g["row"])).long(), torch.from_numpy(np.asarray(g["col"])).long()
        self.val = torch.from_numpy(np.asarray(g["val"])).to(dtype)
        self.tentry = torch.from_numpy(np.asarray(g["tentry"])).long()
        if "mm_row" in g:
            self.mm_row, self.mm_col = torch.from_numpy(g["mm_row"]).long(), torch.from_numpy(g["mm_col"]).long()
            self.mm_val = torch.from_numpy(g["mm_val"]).to(dtype)


LOGIT_LOG = []          # every view's logits, in call order (the generator compares the reference's with these)


def tensors(weights, dtype=torch.float64, requires_grad=True):
    return OrderedDict((n, torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(requires_grad and n not in FROZEN))
                       for n, v in weights.items())


def spmm(G, val, x):
    return torch.zeros(G.N, x.shape[1], dtype=x.dtype).index_add(0, G.row, val[:, None] * x[G.col])


def item_graph(G, h):
    return torch.zeros(G.I, h.shape[1], dtype=h.dtype).index_add(0, G.mm_row, G.mm_val[:, None] * h[G.mm_col])


def _lin(W, name, x):
    return x @ W[name + ".weight"].t() + W[name + ".bias"]


def _layers(G, val, x0, delta_noise=None, n_layers=N_LAYERS):
    xs = [x0]
    for _ in range(n_layers):
        x = spmm(G, val, xs[-1])
        if delta_noise is not None:
            x = x + delta_noise / float(np.sqrt(np.float32(x0.shape[1])))
        xs.append(x)
    return sum(xs)


def modal_tables(W, which):
    """(the user table, the item table before the item graph) of generator `which` (1 ID, 2 visual, 3 textual)."""
    if which == 1:
        return W["uEmbeds.weight"], W["iEmbeds.weight"]
    if which == 2:
        return W["uvEmbeds.weight"], _lin(W, "image_trs", W["v_feat.weight"])
    return W["utEmbeds.weight"], _lin(W, "text_trs", W["t_feat.weight"])


def graphcl(W, G, which, val):
    """forward_graphcl / visual_ / textual_: the item table plus its item-graph propagate, then the layer sum."""
    u, i = modal_tables(W, which)
    return _layers(G, val, torch.cat([u, i + item_graph(G, i)], 0))


def noise_graphcl(W, G, which, val, delta_noise):
    u, i = modal_tables(W, which)
    return _layers(G, val, torch.cat([u, i], 0), delta_noise)


def forward_gcn(W, G, val):
    i = W["iEmbeds.weight"]
    x = _layers(G, val, torch.cat([W["uEmbeds.weight"], i], 0))
    return x[:G.U], x[G.U:] + item_graph(G, i)


def encoder(W, G, which, val, noise):
    x = graphcl(W, G, which, val)
    p = f"generator_{which}.encoder."
    mean = _lin(W, p + "encoder_mean.2", torch.relu(_lin(W, p + "encoder_mean.0", x)))
    std = torch.nn.functional.softplus(_lin(W, p + "encoder_std.2", torch.relu(_lin(W, p + "encoder_std.0", x))))
    return noise * std + mean, mean, std


def decoder_logit(W, which, rows):
    p = f"generator_{which}.decoder.decoder."
    return _lin(W, p + "3", torch.relu(_lin(W, p + "1", torch.relu(rows))))


def view_from_rows(lin1_w, lin1_b, lin2_w, lin2_b, G, x):
    """vgae.generate's lines after the encoder, per stored entry -> dict(logit, p, keep, S, d, val) over the fixed pattern."""
    h = torch.relu(torch.relu(x[G.row] * x[G.col]) @ lin1_w.t() + lin1_b)
    logit = (h @ lin2_w.reshape(-1, 1) + lin2_b.reshape(-1))[:, 0]
    p = torch.sigmoid(logit)
    keep = (p + 0.5).floor().to(torch.bool)
    pk = torch.where(keep, p, torch.zeros_like(p))
    S = torch.zeros(G.N, dtype=x.dtype).index_add(0, G.row, pk) + 1e-7
    d = torch.pow(S, -0.5)
    return dict(logit=logit, p=p, keep=keep, S=S, d=d, val=d[G.row] * pk * d[G.col])


def view(W, G, which, noise):
    """generator_generate(generator_which) -> dict(logit, p, keep, S, d, val)."""
    with torch.no_grad():
        x, _, _ = encoder(W, G, which, G.val, noise)
        p = f"generator_{which}.decoder.decoder."
        out = view_from_rows(W[p + "1.weight"], W[p + "1.bias"], W[p + "3.weight"], W[p + "3.bias"], G, x)
    LOGIT_LOG.append(out["logit"].numpy().copy())
    return out


def loss_graphcl(G, x1, x2, users, items, T):
    F = torch.nn.functional
    u1, i1 = F.normalize(x1[:G.U], dim=1), F.normalize(x1[G.U:], dim=1)
    u2, i2 = F.normalize(x2[:G.U], dim=1), F.normalize(x2[G.U:], dim=1)
    a1, a2 = torch.cat([u1[users], i1[items]], 0), torch.cat([u2[users], i2[items]], 0)
    sim = torch.exp((a1 @ a2.t()) / torch.outer(a1.norm(dim=1), a2.norm(dim=1)) / T)
    pos = torch.diagonal(sim)
    return -torch.log(pos / (sim.sum(1) - pos))


def loss_1(W, G, users, pos, randn, rand):
    v = [view(W, G, g, randn[g - 1])["val"] for g in (1, 2, 3)]
    out1, out2, out3 = (graphcl(W, G, g, v[g - 1]) for g in (1, 2, 3))
    loss = (loss_graphcl(G, out1, out2, users, pos, SSL_TEMP).mean() + loss_graphcl(G, out1, out3, users, pos, SSL_TEMP).mean()) * SSL_ALPHA
    loss = loss + loss_graphcl(G, out2, noise_graphcl(W, G, 2, v[0], rand[0]), users, pos, SSL_TEMP2).mean() * NOISE_ALPHA
    return loss + loss_graphcl(G, out3, noise_graphcl(W, G, 3, v[0], rand[1]), users, pos, SSL_TEMP2).mean() * NOISE_ALPHA


def bpr_reg_loss(W, G, users, pos, neg):
    xu, xi = forward_gcn(W, G, G.val)
    a, p, n = xu[users], xi[pos], xi[neg]
    bpr = -torch.mean(torch.log(torch.sigmoid((a * p).sum(1) - (a * n).sum(1)) + 1e-5))
    reg = REG_WEIGHT * ((W["uEmbeds.weight"][users] ** 2).mean() + (W["iEmbeds.weight"][pos] ** 2).mean() + (W["iEmbeds.weight"][neg] ** 2).mean()
                        + (W["utEmbeds.weight"][users] ** 2).mean() + (W["uvEmbeds.weight"][users] ** 2).mean())
    return bpr + reg


def vgae_loss(W, G, which, users, pos, neg, noise):
    x, mean, std = encoder(W, G, which, G.val, noise)
    xu, xi = x[:G.U], x[G.U:]
    pp = torch.sigmoid(decoder_logit(W, which, xu[users] * xi[pos]))
    pn = torch.sigmoid(decoder_logit(W, which, xu[users] * xi[neg]))
    loss_rec = (pp - 1.0) ** 2 + pn ** 2                                              # [B, 1]
    kl = -0.5 * (1 + 2 * torch.log(std) - mean ** 2 - std ** 2).sum(1)
    return (1 * kl.mean() + loss_rec).mean()


def gen_loss(W, G, users, pos, neg, randn):
    l1, l2, l3 = (vgae_loss(W, G, g, users, pos, neg, randn[g - 1]) for g in (1, 2, 3))
    return l1 + l3 + l2


def _ids(c):
    U = c["U"]
    return (torch.from_numpy(np.asarray(c["users"])).long(), torch.from_numpy(np.asarray(c["pos"]) - U).long(),
            torch.from_numpy(np.asarray(c["neg"]) - U).long())


def _grads(W, loss, names):
    gs = torch.autograd.grad(loss, [W[n] for n in names], allow_unused=True)
    return OrderedDict((n, (g if g is not None else torch.zeros_like(W[n])).numpy().copy()) for n, g in zip(names, gs))


def _t(tables, dtype):
    return [torch.tensor(t, dtype=dtype) for t in tables]


def step_losses(weights, c, dr, dtype=torch.float64):
    """The three losses of one step on FIXED weights (no optimizer step between them) and the gradient each alone produces."""
    G, W = Graph(c, dtype), tensors(weights, dtype)
    users, pos, neg = _ids(c)
    ls = (loss_1(W, G, users, pos, _t(dr["randn1"], dtype), _t(dr["rand"], dtype)), bpr_reg_loss(W, G, users, pos, neg),
          gen_loss(W, G, users, pos, neg, _t(dr["randn2"], dtype)))
    out = {"grads": {}}
    for name, l in zip(LOSSES, ls):
        out[name] = float(l.detach())
        out["grads"][name] = _grads(W, l, WITH_GRAD[name])
    return out


def trajectory(weights, c, drs, dtype=torch.float64):
    """The reference's loop (train_and_evaluate.py:259-284) over the same batch len(drs) times -> (final weights, the losses)."""
    G, W = Graph(c, dtype), tensors(weights, dtype)
    users, pos, neg = _ids(c)
    opt = torch.optim.Adam([W[n] for n in NAMES if n not in FROZEN], lr=LR, weight_decay=0)
    opt_g = [torch.optim.Adam([W[n] for n in GEN[g]], lr=LR, weight_decay=0) for g in (1, 2, 3)]
    losses = []
    for dr in drs:
        opt.zero_grad()
        l1 = loss_1(W, G, users, pos, _t(dr["randn1"], dtype), _t(dr["rand"], dtype))
        l1.backward()
        opt.step()
        opt.zero_grad()
        l2 = bpr_reg_loss(W, G, users, pos, neg)
        l2.backward()
        opt.step()
        for o in opt_g:
            o.zero_grad()
        l3 = gen_loss(W, G, users, pos, neg, _t(dr["randn2"], dtype))
        l3.backward()
        for o in opt_g:
            o.step()
        losses.append([float(x.detach()) for x in (l1, l2, l3)])
    return OrderedDict((n, v.detach().numpy().copy()) for n, v in W.items()), np.array(losses)


def rank_scores(weights, c, dtype=torch.float64):
    """gene_ranklist's score matrix [U, I] (history entries 1e-6)."""
    G, W = Graph(c, dtype), tensors(weights, dtype, False)
    xu, xi = forward_gcn(W, G, G.val)
    s = (xu @ xi.t()).numpy().copy()
    for u, items in user_item_dict(c["edges"]).items():
        s[u, np.asarray(items) - c["U"]] = 1e-6
    return s


def owner_list(G):
    """The entries with row <= col, ascending (what ops_extra.grade_pair_owner builds)."""
    return np.nonzero(np.asarray(G["row"]) <= np.asarray(G["col"]))[0]
