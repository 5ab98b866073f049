"""float64 torch restatement of MacridVAE on the CPU from explicit weights, batch and draws: one training step (loss
parts, lse, the normalised latents, the concept weights, all six gradients), an Adam trajectory, and the eval-mode
scores behind gene_ranklist().  Written from the formulas of the model's description, not from its text.  Imported by
tests/test_macridvae_host.py (against the reference goldens of tests/golden/gen_macridvae.py) and
tests/test_gpu_macridvae.py (the kernels against it).  [B, I] matrices exist here on purpose: this is the formula."""
import os

import numpy as np
import torch

from accept import ULP24
from multvae_host import dense_rows, flags_from_mask, hist_csr, mask_from_flags, rel_dev, user_item_dict  # noqa: F401

K = 10
HIDDEN = 600
TAU = 0.1
STD = 0.01
DROP = 0.5
ANNEAL_CAP = 0.2
TOTAL_ANNEAL_STEPS = 200000
NAMES = ("encoder.0.weight", "encoder.0.bias", "encoder.2.weight", "encoder.2.bias", "item_embedding.weight", "k_embedding.weight")


def anneal_of(update_after_increment):
    return min(ANNEAL_CAP, 1.0 * update_after_increment / TOTAL_ANNEAL_STEPS)


def unit_rows(x):
    return x / torch.clamp(x.norm(dim=1, keepdim=True), min=1e-12)


def concept_weights(E, Kemb, gumbel=None):
    """-> (items [I, D], cates [I, K]); gumbel: the noise added to the logits (training), None: eval."""
    items, cores = unit_rows(E), unit_rows(Kemb)
    cl = items @ cores.t() / TAU
    if gumbel is not None:
        cl = cl + gumbel
    return items, torch.softmax(cl, dim=1)


def latents(W1, b1, W2, b2, cates, xs, eps):
    """xs [B, I]: the scaled (and dropped) rows; eps [K, B, D] or None -> zh [B, K, D], logvar [B, K, D]."""
    D = W2.shape[0] // 2
    zs, lvs = [], []
    for k in range(K):
        a = xs @ (cates[:, k:k + 1] * W1.t()) + b1
        h = torch.tanh(a) @ W2.t() + b2
        mu, lv = unit_rows(h[:, :D]), h[:, D:]
        z = mu if eps is None else mu + eps[k] * torch.exp(0.5 * lv)
        zs.append(unit_rows(z))
        lvs.append(lv)
    return torch.stack(zs, 1), torch.stack(lvs, 1)


def mixture(zh, items, cates):
    """p [B, I] = sum_k cates[i, k] exp(zh_bk . items_i / tau)."""
    p = None
    for k in range(K):
        pk = torch.exp(zh[:, k] @ items.t() / TAU) * cates[:, k][None, :]
        p = pk if p is None else p + pk
    return p


def step(weights, rowptr, col, users, keep, gumbel, eps, update_before, training=True, dtype=torch.float64):
    """weights in NAMES order; keep: per-entry flags; gumbel [I, K]; eps [K, B, D] (std included); update_before: the
    counter BEFORE this step (the step increments it first and reads the anneal from the incremented value).
    -> dict(loss, ce, kl, anneal, lse [B], z [B, K, D], cates [I, K], grads (six))."""
    W1, b1, W2, b2, E, Kemb = (torch.as_tensor(np.asarray(w)).to(dtype).clone().requires_grad_(True) for w in weights)
    I = E.shape[0]
    B = len(users)
    x = dense_rows(rowptr, col, users, I, dtype)
    n = x.sum(1)
    xs = x / torch.clamp(n.sqrt(), min=1e-12)[:, None]
    if training and keep is not None:
        xs = xs * torch.from_numpy(mask_from_flags(keep, rowptr, col, users, I)).to(dtype) / (1.0 - DROP)
    g = torch.as_tensor(np.asarray(gumbel)).to(dtype) if training else None
    items, cates = concept_weights(E, Kemb, g)
    e = torch.as_tensor(np.asarray(eps)).to(dtype) if training else None
    zh, lv = latents(W1, b1, W2, b2, cates, xs, e)
    p = mixture(zh, items, cates)
    lse = torch.log(p.sum(1))
    ce = (n * lse - (torch.log(p) * x).sum(1)).mean()
    kl = (-0.5 * (1 + lv - lv.exp()).sum(2).mean(0)).sum()
    anneal = anneal_of(update_before + 1)
    loss = ce + anneal * kl
    loss.backward()
    return {"loss": loss.item(), "ce": ce.item(), "kl": kl.item(), "anneal": anneal, "lse": lse.detach().numpy(),
            "z": zh.detach().numpy(), "cates": cates.detach().numpy(),
            "grads": tuple(t.grad.numpy() for t in (W1, b1, W2, b2, E, Kemb))}


def adam_trajectory(weights, rowptr, col, batches, keeps, gumbels, epss, update_before, lr, dtype=torch.float64):
    params = [torch.as_tensor(np.asarray(w)).to(dtype).clone().requires_grad_(True) for w in weights]
    opt = torch.optim.Adam(params, lr=lr)
    losses = []
    for t, users in enumerate(batches):
        out = step([p.detach().numpy() for p in params], rowptr, col, users, keeps[t], gumbels[t], epss[t], update_before + t, dtype=dtype)
        opt.zero_grad()
        for p, g in zip(params, out["grads"]):
            p.grad = torch.from_numpy(np.asarray(g)).to(dtype)
        opt.step()
        losses.append(out["loss"])
    return np.asarray(losses), tuple(p.detach().numpy() for p in params)


def eval_scores(weights, rowptr, col, users, dtype=torch.float64):
    """log p_ui in eval mode (no dropout, no Gumbel noise, z = mu) for `users` -> [n, I]."""
    W1, b1, W2, b2, E, Kemb = (torch.as_tensor(np.asarray(w)).to(dtype) for w in weights)
    x = dense_rows(rowptr, col, users, E.shape[0], dtype)
    xs = x / torch.clamp(x.sum(1).sqrt(), min=1e-12)[:, None]
    items, cates = concept_weights(E, Kemb)
    zh, _ = latents(W1, b1, W2, b2, cates, xs, None)
    return torch.log(mixture(zh, items, cates))


# The rounding gap of one fp32 score log p_ui: p's relative error is at most the largest error of a logit l = zh . it / tau.
# With |zh| = |it| = 1 the 64-term dot rounds by at most 64 * 2^-24; zh itself comes out of an fp32 encoder whose longest
# sums have 600 (hidden layer) + 64 (normalisations) terms, one rounding each: (64 + 600 + 64) * 2^-24 / tau = 4.3e-4.
SCORE_GAP = (64 + 600 + 64) * ULP24 / TAU


def ranklist_check(ranks, weights, rowptr, col, hist_rowptr, hist_col, users, topk=50, chunk=512):
    """`ranks` [n, topk] LOCAL item ids of `users` against the fp64 eval scores (history -> the VALUE 1e-6) -> (share of
    positions that differ from the fp64 list, the number of differing positions that are not a swap inside the rounding
    gap: SCORE_GAP per unmasked score of the pair, 0 for a masked one)."""
    ranks = torch.as_tensor(np.asarray(ranks)).long()
    users = np.asarray(users)
    differ = bad = 0
    for o in range(0, len(users), chunk):
        us = users[o:o + chunk]
        sc = eval_scores(weights, rowptr, col, us)
        tol = torch.full_like(sc, SCORE_GAP)
        for r, u in enumerate(us):
            c = torch.as_tensor(np.asarray(hist_col[hist_rowptr[u]:hist_rowptr[u + 1]])).long()
            sc[r, c] = 1e-6
            tol[r, c] = 0.0
        want = torch.topk(sc, topk, dim=1)[1]
        got = ranks[o:o + chunk]
        diff = got != want
        differ += int(diff.sum())
        gap = (torch.gather(sc, 1, got) - torch.gather(sc, 1, want)).abs()
        allowed = torch.gather(tol, 1, got) + torch.gather(tol, 1, want)
        bad += int((diff & (gap > allowed)).sum())
    return differ / float(ranks.numel()), bad


def replay_draws(seed, B, I, D):
    """(keep mask [B, I], gumbel [I, K], eps [K, B, D]) as one training forward of the model draws them after
    torch.manual_seed(seed): the dropout Bernoulli over [B, I], exponential_ over [I, K], normal_(0, std) over [B, D] once
    per concept."""
    torch.manual_seed(int(seed))
    mask = torch.nn.functional.dropout(torch.ones(B, I), DROP) != 0
    gumbel = -torch.empty(I, K).exponential_().log()
    eps = torch.stack([torch.zeros(B, D).normal_(mean=0, std=STD) for _ in range(K)])
    return mask.numpy(), gumbel.numpy(), eps.numpy()


def case_draws(g, seed, users):
    mask, gumbel, eps = replay_draws(seed, len(users), g["I"], g["D"])
    return flags_from_mask(mask, g["rowptr"], g["col"], users), gumbel, eps


def draw_sums(keep, gumbel, eps):
    return np.asarray([float(np.asarray(keep, dtype=np.float64).sum()), float(gumbel.astype(np.float64).sum()),
                       float(eps.astype(np.float64).sum())])


def draws_match(draws, stored):
    """Are these the generator's draws?  Keep flags and eps by exact checksum; the Gumbel noise is -log of the exponential
    draw and the vectorised log differs by an ulp between CPUs, so its checksum is held to 1e-7 per element (another
    stream would differ by about sqrt(n))."""
    d = np.abs(draw_sums(*draws) - np.asarray(stored))
    return bool(d[0] == 0 and d[1] <= 1e-7 * draws[1].size and d[2] < 1e-9)


def load_fixture(golden_dir, name):
    g = dict(np.load(os.path.join(golden_dir, f"macridvae_{name}.npz"), allow_pickle=False))
    if "edges" not in g:
        g["edges"] = np.load(os.path.join(golden_dir, f"{name}_interactions.npz"))["train"]
    g["U"], g["I"], g["D"] = int(g["U"]), int(g["I"]), int(g["D"])
    g["edges"] = np.asarray(g["edges"], dtype=np.int64)
    g["rowptr"], g["col"] = hist_csr(g["edges"], g["U"])
    return g
