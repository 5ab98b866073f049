"""Host restatements of what Model/MVGAE.py and the mg_* kernels of csrc/mvgae.hip compute, in float64: the conv epilogue and
the tail (forward and backward written out in numpy, draws GIVEN), the reference's own lines of both in torch with a dtype
argument (the yardstick the GPU tests measure their tolerance with), the counter RNG, the constructor's draws, and one whole
MVGAE step (forward written out in float64 torch, the gradients float64 autograd over it).  Imported by test_mvgae_host.py,
test_gpu_mvgae.py and golden/gen_mvgae.py."""
import os

import numpy as np
import torch
from accept import rel_dev, user_item_dict  # noqa: F401
from vae_ops_host import vae_key, vae_uniform      # the counter RNG of csrc/draws.h in uint64 numpy

D = 64
E = 1e-8
MAX_LOGVAR = 10.0
VIEWS = ("P", "V", "T", "C")
DIM_E, KL_WEIGHT, N_LAYERS, LATENT = 64, 0.1, 2, 128
_PER_GCN = ("MLP.weight", "MLP.bias") + tuple(f"{m}{k}.{p}" for k in (1, 2, 3, 4, 5)
                                              for m in ("conv_embed_", "linear_layer", "g_layer") for p in ("weight", "bias"))
NAMES = tuple(f"{g}.{n}" for g in ("v_gcn", "t_gcn", "c_gcn") for n in _PER_GCN)          # state_dict() order: 96 names


def with_grad(n_layers):
    """The names the loss reaches: linear_layer1..3 never (concate = False), layer k's conv / g only for k <= n_layers."""
    out = []
    for n in NAMES:
        mod = n.split(".")[1]
        k = int(mod[-1]) if mod[-1].isdigit() else 0
        if mod == "MLP" or k >= 4 or (k <= min(n_layers, 3) and not mod.startswith("linear_layer")):
            out.append(n)
    return tuple(out)


def load_fixture(golden_dir, name="mvgae_small.npz"):
    g = dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))
    g["keep"] = np.unpackbits(g["keep_bits"]).reshape(-1)[:int(g["keep_n"]) * (int(g["U"]) + int(g["I"])) * D].reshape(
        int(g["keep_n"]), int(g["U"]) + int(g["I"]), D).astype(bool)
    for k in ("U", "I", "seed"):
        g[k] = int(g[k])
    return g


def keep_mask(seed, step, salt, N):
    """The device's dropout flags of conv `salt`: uniform(key, 0, r * 64 + d) >= 0.1 (exact: the uniform is exact in fp32)."""
    e = np.arange(N * D, dtype=np.uint64)
    return (vae_uniform(vae_key(seed, step, salt), 0, e, 24) >= np.float32(0.1)).reshape(N, D)


# ---- (a) the conv epilogue -------------------------------------------------------------------------------------------------
def _mult(keep, training, shape):
    if not training:
        return np.ones(shape)
    return np.where(np.asarray(keep, dtype=bool), 1.0 / 0.9, 0.0)


def conv_tail(s, bias, keep=None, training=True):
    """y = leaky_relu(q m, 0.01), q = a / max(|a|, 1e-12), a = s + bias; m = 1 / 0.9 kept, 0 dropped, 1 in evaluation."""
    a = np.asarray(s, dtype=np.float64) + np.asarray(bias, dtype=np.float64)
    n = np.sqrt((a * a).sum(1, keepdims=True))
    t = a / np.maximum(n, 1e-12) * _mult(keep, training, a.shape)
    return np.where(t > 0, t, 0.01 * t)


def conv_tail_bwd(gy, s, bias, keep=None, training=True):
    """-> (gs, gbias)."""
    a = np.asarray(s, dtype=np.float64) + np.asarray(bias, dtype=np.float64)
    n = np.sqrt((a * a).sum(1, keepdims=True))
    q, m = a / np.maximum(n, 1e-12), _mult(keep, training, a.shape)
    gq = np.asarray(gy, dtype=np.float64) * np.where(q * m > 0, 1.0, 0.01) * m
    gs = np.where(n >= 1e-12, (gq - q * (gq * q).sum(1, keepdims=True)) / np.maximum(n, 1e-300), gq / 1e-12)
    return gs, gs.sum(0)


def conv_tail_torch(s, bias, keep, training, dtype):
    """The reference's lines (BaseModel.update and the leaky_relu around it) in torch at `dtype`, the mask given as dropout
    applies it (input * (mask / 0.9)) -> (y, backward: gy -> (gs, gbias))."""
    F = torch.nn.functional
    s = torch.tensor(np.asarray(s), dtype=dtype, requires_grad=True)
    b = torch.tensor(np.asarray(bias), dtype=dtype, requires_grad=True)
    y = F.normalize(s + b, p=2, dim=-1)
    if training:
        y = y * (torch.tensor(np.asarray(keep), dtype=dtype) / 0.9)
    y = F.leaky_relu(y)

    def backward(gy):
        gs, gb = torch.autograd.grad(y, (s, b), torch.tensor(np.asarray(gy), dtype=dtype), retain_graph=True)
        return gs.numpy(), gb.numpy()
    return y.detach().numpy(), backward


# ---- (b) the tail ----------------------------------------------------------------------------------------------------------
def _poe(ma, la, mb, lb):
    ea, eb = np.exp(la), np.exp(lb)
    ta, tb = 1.0 / (ea + E), 1.0 / (eb + E)
    S = ta + tb
    return dict(ea=ea, eb=eb, ta=ta, tb=tb, S=S, m=(ma * ta + mb * tb) / S, l=np.log(1.0 / S))


def _poe_bwd(p, ma, mb, gm, gl):
    gma, gmb = gm * p["ta"] / p["S"], gm * p["tb"] / p["S"]
    gta, gtb = (gm * (ma - p["m"]) - gl) / p["S"], (gm * (mb - p["m"]) - gl) / p["S"]
    return gma, gta * -(p["ta"] ** 2 * p["ea"]), gmb, gtb * -(p["tb"] ** 2 * p["eb"])


def tail(tables, users, pos, neg, kl_weight, eps=None, training=True):
    """tables: (Vm, Vl, Tm, Tl, Cm, Cl) [N, 64]; users, pos, neg: GLOBAL row ids; eps [4, N, 64] in the order P, V, T, C.
    -> dict(total, parts [8] = BPR_P V T C, KL_P V T C, Pm, z [4, N, 64], coef [4, B], cache for tail_bwd)."""
    Vm, Vl, Tm, Tl, Cm, Cl = (np.asarray(t, dtype=np.float64) for t in tables)
    N, B = Vm.shape[0], len(users)
    p1 = _poe(Vm, Vl, Tm, Tl)
    p2 = _poe(p1["m"], p1["l"], Cm, Cl)
    ms, ls = [p2["m"], Vm, Tm, Cm], [p2["l"], Vl, Tl, Cl]
    bpr, kl, zs, coef = [], [], [], []
    for x in range(4):
        lc = np.minimum(ls[x], MAX_LOGVAR)
        kl.append(-0.5 / N * (1 + lc - ms[x] ** 2 - np.exp(lc)).sum())
        z = ms[x] + np.asarray(eps[x], dtype=np.float64) * 0.1 * np.exp(0.5 * lc) if training else ms[x]
        diff = (z[users] * z[pos]).sum(1) - (z[users] * z[neg]).sum(1)
        with np.errstate(over="ignore"):
            sg = 1.0 / (1.0 + np.exp(-diff))
        bpr.append(-np.log(sg + 1e-5).mean())
        coef.append(-(sg * (1 - sg)) / (sg + 1e-5) / B)
        zs.append(z)
    parts = np.array(bpr + kl)
    return dict(total=float(sum(bpr) + kl_weight * sum(kl)), parts=parts, Pm=p2["m"], z=np.stack(zs), coef=np.stack(coef),
                cache=(p1, p2, ms, ls))


def tail_bwd(tables, users, pos, neg, kl_weight, eps=None, training=True, gtotal=1.0):
    """-> the six gradient tables (dVm, dVl, dTm, dTl, dCm, dCl), the chain csrc/mvgae.hip's header states."""
    Vm, Vl, Tm, Tl, Cm, Cl = (np.asarray(t, dtype=np.float64) for t in tables)
    N = Vm.shape[0]
    f = tail(tables, users, pos, neg, kl_weight, eps, training)
    p1, p2, ms, ls = f["cache"]
    gm, gl = [], []
    for x in range(4):
        z, c = f["z"][x], f["coef"][x][:, None]
        dz = np.zeros((N, D))
        np.add.at(dz, users, c * (z[pos] - z[neg]))
        np.add.at(dz, pos, c * z[users])
        np.add.at(dz, neg, -c * z[users])
        lc = np.minimum(ls[x], MAX_LOGVAR)
        v = kl_weight * (-0.5 / N) * (1 - np.exp(lc))
        if training:
            v = v + dz * np.asarray(eps[x], dtype=np.float64) * 0.1 * 0.5 * np.exp(0.5 * lc)
        gm.append(dz + kl_weight * ms[x] / N)
        gl.append(np.where(ls[x] <= MAX_LOGVAR, v, 0.0))
    gM1, gL1, gc_m, gc_l = _poe_bwd(p2, p1["m"], Cm, gm[0], gl[0])
    gv_m, gv_l, gt_m, gt_l = _poe_bwd(p1, Vm, Tm, gM1, gL1)
    return tuple(gtotal * g for g in (gm[1] + gv_m, gl[1] + gv_l, gm[2] + gt_m, gl[2] + gt_l, gm[3] + gc_m, gl[3] + gc_l))


def tail_torch(tables, users, pos, neg, kl_weight, eps, training, dtype):
    """The reference's lines (Model/MVGAE.py:75-100, :270-284, :317-342, :364-416) in torch at `dtype`, draws given ->
    (total, parts [8], Pm, the six gradients)."""
    tabs = [torch.tensor(np.asarray(t), dtype=dtype, requires_grad=True) for t in tables]
    users, pos, neg = (torch.as_tensor(np.asarray(t), dtype=torch.int64) for t in (users, pos, neg))

    def experts(mu, logvar, e=1e-8):
        T = 1. / (torch.exp(logvar) + e)
        return torch.sum(mu * T, dim=0) / torch.sum(T, dim=0), torch.log(1. / torch.sum(T, dim=0))

    def reparametrize(mu, logvar, e):
        logvar = logvar.clamp(max=10)
        return mu + e * 0.1 * torch.exp(logvar.mul(0.5)) if training else mu

    def kl_loss(mu, logvar):
        logvar = logvar.clamp(max=10)
        return -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))

    def bpr_loss(z):
        u, p, n = z[users], z[pos], z[neg]
        return -torch.mean(torch.log(torch.sigmoid(torch.sum(u * p, dim=1) - torch.sum(u * n, dim=1)) + 1e-5))

    v_mu, v_lv, t_mu, t_lv, c_mu, c_lv = tabs
    pd_mu, pd_lv = experts(torch.stack([v_mu, t_mu], dim=0), torch.stack([v_lv, t_lv], dim=0))
    pd_mu, pd_lv = experts(torch.stack([pd_mu, c_mu], dim=0), torch.stack([pd_lv, c_lv], dim=0))
    views = [(pd_mu, pd_lv), (v_mu, v_lv), (t_mu, t_lv), (c_mu, c_lv)]
    e = [torch.tensor(np.asarray(eps[x]), dtype=dtype) if training else None for x in range(4)]
    bpr = [bpr_loss(reparametrize(m, l, e[x])) for x, (m, l) in enumerate(views)]
    kl = [kl_loss(m, l) for m, l in views]
    total = sum(b + kl_weight * k for b, k in zip(bpr, kl))
    grads = torch.autograd.grad(total, tabs)
    return (float(total.detach()), np.array([float(v.detach()) for v in bpr + kl]), pd_mu.detach().numpy(), tuple(g.numpy() for g in grads))


def slot_index(users, pos, neg, N):
    """(slot_ptr [N + 1], perm [3B]): a stable sort of [users; pos; neg]."""
    ids = np.concatenate([users, pos, neg]).astype(np.int64)
    perm = np.argsort(ids, kind="stable")
    return np.searchsorted(ids[perm], np.arange(N + 1)), perm


# ---- the model: the synthetic case, the constructor's draws, one step in float64 --------------------------------------------
def small_case():
    """U 37, I 23, 150 interactions, B 16 (one user three times, one item positive in one sample and negative in another),
    feature widths 24 and 12 (values exact in fp16)."""
    U, I, B = 37, 23, 16
    rng = np.random.default_rng(20261019)
    pairs = set()
    while len(pairs) < 150:
        pairs.add((int(rng.integers(0, U)), int(rng.integers(0, I))))
    e = np.array(sorted(pairs), dtype=np.int64)
    edges = np.stack([e[:, 0], e[:, 1] + U], 1)
    pick = rng.choice(len(edges), size=B, replace=False)
    users, pos = edges[pick, 0].copy(), edges[pick, 1].copy()
    same = np.nonzero(edges[:, 0] == users[0])[0]
    for k, j in enumerate(same[:2]):                       # the first sample's user again, with other items of theirs
        users[1 + k], pos[1 + k] = edges[j, 0], edges[j, 1]
    neg = rng.integers(U, U + I, B).astype(np.int64)
    neg[5] = pos[4]
    v_feat = rng.standard_normal((I, 24)).astype(np.float16).astype(np.float32)
    t_feat = rng.standard_normal((I, 12)).astype(np.float16).astype(np.float32)
    return dict(U=U, I=I, edges=edges, users=users, pos=pos, neg=neg, v_feat=v_feat, t_feat=t_feat, seed=7)


def init_weights(c, dim_E=DIM_E):
    """The draws of the constructor (Model/MVGAE.py:246-268, :123-177, :38-40) replayed on torch's CPU generator ->
    ({name: array} for the 96 Parameters, {name: array} for collaborative / preference / result_embed)."""
    nn = torch.nn
    U, I = c["U"], c["I"]
    torch.manual_seed(c["seed"])
    w, plain = {}, {}
    xn = nn.init.xavier_normal_
    plain["collaborative"] = xn(torch.rand((I, dim_E)))
    for g, dim_feat in (("v_gcn", c["v_feat"].shape[1]), ("t_gcn", c["t_feat"].shape[1]), ("c_gcn", dim_E)):
        plain[f"{g}.preference"] = xn(torch.rand((U, LATENT)))

        def linear(name, a, b, xavier=True):
            lin = nn.Linear(a, b)
            if xavier:
                xn(lin.weight)
            w[f"{g}.{name}.weight"], w[f"{g}.{name}.bias"] = lin.weight, lin.bias

        linear("MLP", dim_feat, LATENT)
        for k in (1, 2, 3, 4, 5):
            first = LATENT if k == 1 else dim_E
            weight, bias = torch.empty(first, dim_E), torch.empty(dim_E)
            bound = 1.0 / (first ** 0.5)
            weight.uniform_(-bound, bound)
            bias.uniform_(-bound, bound)
            xn(weight)
            w[f"{g}.conv_embed_{k}.weight"], w[f"{g}.conv_embed_{k}.bias"] = weight, bias
            linear(f"linear_layer{k}", first, dim_E)
            linear(f"g_layer{k}", dim_E, dim_E, xavier=k not in (2, 3))
    plain["result_embed"] = xn(torch.rand((U + I, dim_E)))
    return ({n: w[n].detach().numpy().copy() for n in NAMES}, {n: v.detach().numpy().copy() for n, v in plain.items()})


def dense_adj(edges, N):
    """D^-1/2 (A + I) D^-1/2 of the bidirectional graph, float64 (a repeated edge counts as often as it is listed)."""
    A = np.zeros((N, N))
    e = np.asarray(edges, dtype=np.int64)
    np.add.at(A, (e[:, 0], e[:, 1]), 1.0)
    A = A + A.T + np.eye(N)
    dis = A.sum(1) ** -0.5
    return A * dis[:, None] * dis[None, :]


def step(weights, plain, c, users, pos, neg, kl_weight=KL_WEIGHT, n_layers=N_LAYERS, keep=None, eps=None, training=True):
    """One MVGAE loss() in float64 with GIVEN draws -> dict(loss, parts [8], result [N, 64], tables (six), grads {name: array}
    for with_grad(n_layers))."""
    F = torch.nn.functional
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)      # noqa: E731
    U, I = c["U"], c["I"]
    N = U + I
    A = t64(dense_adj(c["edges"], N))
    w = {n: t64(weights[n]).requires_grad_(True) for n in NAMES}
    keep = [t64(k) for k in keep] if keep is not None else None
    feats = {"v_gcn": t64(c["v_feat"]), "t_gcn": t64(c["t_feat"]), "c_gcn": t64(plain["collaborative"])}
    tables, call = [], 0
    for g in ("v_gcn", "t_gcn", "c_gcn"):
        def conv(k, x):
            nonlocal call
            y = F.normalize(A @ (x @ w[f"{g}.conv_embed_{k}.weight"]) + w[f"{g}.conv_embed_{k}.bias"], p=2, dim=-1)
            if training:
                y = y * keep[call] / 0.9
            call += 1
            return F.leaky_relu(y)

        lin = lambda name, x: x @ w[f"{g}.{name}.weight"].T + w[f"{g}.{name}.bias"]      # noqa: E731
        x = F.normalize(torch.cat((t64(plain[f"{g}.preference"]), lin("MLP", feats[g])), dim=0))
        for k in range(1, min(n_layers, 3) + 1):
            x = F.leaky_relu(lin(f"g_layer{k}", conv(k, x)))
        tables.append(lin("g_layer4", conv(4, x)) + F.leaky_relu(lin("linear_layer4", x)))
        tables.append(lin("g_layer5", conv(5, x)) + F.leaky_relu(lin("linear_layer5", x)))
    tabs_np = [t.detach().numpy() for t in tables]
    f = tail(tabs_np, users, pos, neg, kl_weight, eps, training)
    gt = tail_bwd(tabs_np, users, pos, neg, kl_weight, eps, training)
    names = with_grad(n_layers)
    grads = torch.autograd.grad(tables, [w[n] for n in names], [t64(g) for g in gt])
    return dict(loss=f["total"], parts=f["parts"], result=f["Pm"], tables=tabs_np, grads={n: g.numpy() for n, g in zip(names, grads)})
