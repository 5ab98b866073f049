"""float64 restatement of DualVAE on the CPU from explicit weights, tables, batch and draws: one training step (loss, both
sides' kl / ll / cl, z, nei, the tables it leaves behind, the 18 gradients), an Adam trajectory and gene_ranklist's
scores.  Shared by tests/test_dualvae_host.py (against the reference goldens of tests/golden/gen_dualvae.py) and
tests/test_gpu_dualvae.py (the kernels against it).  [B, U] / [B, I] matrices exist here on purpose: this is the formula.
The forward is written out; the gradients are float64 autograd over it."""
import os

import numpy as np
import torch

from multvae_host import rel_dev, user_item_dict  # noqa: F401

NAMES = ("user_preferences", "item_topics",
         "user_encoder.fc0.weight", "user_encoder.fc0.bias", "user_mu.weight", "user_mu.bias", "user_std.weight", "user_std.bias",
         "item_encoder.fc0.weight", "item_encoder.fc0.bias", "item_mu.weight", "item_mu.bias", "item_std.weight", "item_std.bias",
         "user_decoder.fc_out0.weight", "user_decoder.fc_out0.bias", "item_decoder.fc_out0.weight", "item_decoder.fc_out0.bias")
A, K, H = 5, 25, 20
EPS = 1e-10
KL_WEIGHT, SSL_REG = 0.5, 0.01      # Model_YAML/DualVAE.yaml


def dense_matrix(edges, U, I):
    x = np.zeros((U, I), dtype=np.float64)
    e = np.asarray(edges, dtype=np.int64)
    x[e[:, 0], e[:, 1] - U] = 1.0
    return x


def replay_draws(seed, B):
    """The reference's draws of one loss() call: torch.manual_seed(seed), then randn_like per aspect, item side first
    -> (eps_item, eps_user), each float32 [5, B, 25]."""
    torch.manual_seed(int(seed))
    e = [torch.randn(B, K) for _ in range(2 * A)]
    return torch.stack(e[:A]).numpy(), torch.stack(e[A:]).numpy()


def draw_sums(draws):
    return np.array([float(np.asarray(d, dtype=np.float64).sum()) for d in draws])


def contrast_loss(x, x_):
    x = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    x_ = x_ / x_.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    pos = torch.exp((x_ * x).sum(-1) / 0.2)
    acl = torch.exp(torch.einsum("bak,bck->bac", x_, x) / 0.2).sum(-1)
    ncl = torch.exp(torch.einsum("bak,cak->bac", x_, x) / 0.2).sum(-1)
    return -torch.log(pos / (acl + ncl)).sum(-1).mean()


def side(p, user, x, table, eps):
    """One side of loss() in torch float64: x [B, N] multi-hot rows, table [N, 5, 25], eps [5, B, 25]."""
    s, t = ("user", "item") if user else ("item", "user")
    pref = p["item_topics"] if user else p["user_preferences"]
    w = torch.softmax((table * pref).sum(-1), dim=1)                                   # [N, 5]
    zs, mus, neis, kl, probs = [], [], [], 0.0, 0.0
    for a in range(A):
        h = torch.tanh((x * w[:, a]) @ p[f"{s}_encoder.fc0.weight"].t() + p[f"{s}_encoder.fc0.bias"])
        mu = h @ p[f"{s}_mu.weight"].t() + p[f"{s}_mu.bias"]
        std = torch.sigmoid(h @ p[f"{s}_std.weight"].t() + p[f"{s}_std.bias"])
        kl = kl + (-0.5 * (1 + 2.0 * torch.log(std) - mu ** 2 - std ** 2)).sum(-1).mean()
        z = mu + eps[a] * std
        zh = torch.tanh(z @ p[f"{s}_decoder.fc_out0.weight"].t() + p[f"{s}_decoder.fc_out0.bias"])
        th = torch.tanh(table[:, a] @ p[f"{t}_decoder.fc_out0.weight"].t() + p[f"{t}_decoder.fc_out0.bias"])
        pa = torch.sigmoid(z @ table[:, a].t() + torch.tanh(zh @ th.t())) * w[:, a]
        probs = probs + pa
        zs.append(z)
        mus.append(mu)
        neis.append(pa @ table[:, a])
    z, mu, nei = torch.stack(zs, 1), torch.stack(mus, 1), torch.stack(neis, 1)
    kl = kl / A
    cl = contrast_loss(z, nei)
    ll = (x * torch.log(probs + EPS) - probs).sum(-1).mean()
    return dict(z=z, mu=mu, nei=nei, kl=kl, cl=cl, ll=ll)


def write_back(table, ids, rows):
    """table[ids] = rows with the HIGHEST batch position winning where an id repeats."""
    for b in range(len(ids)):
        table[int(ids[b])] = rows[b]


def step(weights, tables, X, users, pos_local, eps_item, eps_user, kl_weight=KL_WEIGHT, ssl_reg=SSL_REG, grads=True,
         user_writes_first=True):
    """weights: the 18 arrays in NAMES order; tables: (theta, beta, mu_theta, mu_beta); X: the dense [U, I] matrix.
    -> dict(loss, item / user: dict(kl, ll, cl, loss, z, mu, nei), grads (18 float64 arrays), tables (the four, after))."""
    p = {n: torch.tensor(np.asarray(w, dtype=np.float64), requires_grad=grads) for n, w in zip(NAMES, weights)}
    theta, beta, mu_theta, mu_beta = (np.array(t, dtype=np.float64) for t in tables)
    X = torch.as_tensor(X, dtype=torch.float64)
    users, pos_local = np.asarray(users, dtype=np.int64), np.asarray(pos_local, dtype=np.int64)
    it = side(p, False, X.t()[pos_local], torch.tensor(theta), torch.tensor(np.asarray(eps_item, dtype=np.float64)))
    write_back(beta, pos_local, it["z"].detach().numpy())
    write_back(mu_beta, pos_local, it["mu"].detach().numpy())
    us = side(p, True, X[users], torch.tensor(beta), torch.tensor(np.asarray(eps_user, dtype=np.float64)))
    write_back(theta, users, us["z"].detach().numpy())
    write_back(mu_theta, users, us["mu"].detach().numpy())
    out = {}
    for name, s in (("item", it), ("user", us)):
        s["loss"] = kl_weight * s["kl"] - s["ll"] + ssl_reg * s["cl"]
        out[name] = {k: v.detach().numpy() for k, v in s.items()}
    loss = it["loss"] + us["loss"]
    out["loss"] = float(loss.detach())
    if grads:
        g = torch.autograd.grad(loss, [p[n] for n in NAMES])
        out["grads"] = [x.numpy() for x in g]
    out["tables"] = (theta, beta, mu_theta, mu_beta)
    return out


def adam_trajectory(weights, tables, X, batches, seed0, lr, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's defaults over len(batches) steps, draws replayed from seed0 + t -> (losses, weights, tables)."""
    w = [np.asarray(x, dtype=np.float64).copy() for x in weights]
    m, v = [np.zeros_like(x) for x in w], [np.zeros_like(x) for x in w]
    losses = []
    for t, (users, pos_local) in enumerate(batches, start=1):
        ei, eu = replay_draws(seed0 + t - 1, len(users))
        out = step(w, tables, X, users, pos_local, ei, eu)
        losses.append(out["loss"])
        tables = out["tables"]
        for k, g in enumerate(out["grads"]):
            m[k] = betas[0] * m[k] + (1 - betas[0]) * g
            v[k] = betas[1] * v[k] + (1 - betas[1]) * g * g
            w[k] = w[k] - (lr / (1 - betas[0] ** t)) * m[k] / (np.sqrt(v[k]) / np.sqrt(1 - betas[1] ** t) + eps)
    return np.array(losses), w, tables


def scores(weights, mu_theta, mu_beta, users=None):
    """gene_ranklist's scores before the mask, float64 [len(users), I]: the RAW aspect weight sum_k mu_beta item_topics."""
    p = {n: np.asarray(w, dtype=np.float64) for n, w in zip(NAMES, weights)}
    mt = np.asarray(mu_theta, dtype=np.float64)
    mb = np.asarray(mu_beta, dtype=np.float64)
    if users is not None:
        mt = mt[np.asarray(users)]
    aw = (mb * p["item_topics"]).sum(-1)
    out = 0.0
    for a in range(A):
        th = np.tanh(mt[:, a] @ p["user_decoder.fc_out0.weight"].T + p["user_decoder.fc_out0.bias"])
        bh = np.tanh(mb[:, a] @ p["item_decoder.fc_out0.weight"].T + p["item_decoder.fc_out0.bias"])
        out = out + aw[:, a] / (1.0 + np.exp(-(mt[:, a] @ mb[:, a].T + np.tanh(th @ bh.T))))
    return out


def ranklist_check(ranks, sc, hist, users, topk, U, gap_rel=4e-6):
    """ranks [n, topk] (global item ids) against float64 scores sc [n, I] of `users` (history entries set to 1e-6 here)
    -> (share of positions that differ from the float64 list, number of differing positions OUTSIDE the rounding gap).
    A position is inside the gap if the listed item's float64 score is within gap_rel x the row's largest |score| of the
    float64 list's score at that position (fp32 scores of both lists' items round across each other)."""
    sc = np.array(sc, dtype=np.float64)
    for r, u in enumerate(np.asarray(users).tolist()):
        items = np.asarray(sorted(set(hist.get(int(u), []))), dtype=np.int64) - U
        if items.size:
            sc[r, items] = 1e-6
    want = np.argsort(-sc, axis=1, kind="stable")[:, :topk]
    got = np.asarray(ranks, dtype=np.int64) - U
    diff = want != got
    rows = np.arange(sc.shape[0])[:, None]
    gap = np.abs(sc[rows, got] - sc[rows, want]) > gap_rel * np.abs(sc).max(axis=1, keepdims=True)
    return float(diff.mean()), int((diff & gap).sum())


def load_fixture(golden_dir, name):
    g = dict(np.load(os.path.join(golden_dir, f"dualvae_{name}.npz"), allow_pickle=False))
    for k in ("U", "I", "seed", "draw_seed", "topk"):
        if k in g:
            g[k] = int(g[k])
    if "edges" not in g:                     # sports: the committed interactions, not a second copy of them
        g["edges"] = np.load(os.path.join(golden_dir, f"{name}_interactions.npz"))["train"].astype(np.int32)
    return g
