"""float64 torch restatement of MultVAE (Model/MultVAE.py) on the CPU from explicit weights, batch and draws: one training
step (loss parts, lse, z, all four gradients), an Adam trajectory, and the scores behind gene_ranklist().  Imported by
tests/test_multvae_host.py (against the reference goldens of tests/golden/gen_multvae.py) and tests/test_gpu_multvae.py
(the kernels against it).  The dense [B, I] rows exist here on purpose: this is the formula, not the product."""
import numpy as np
import torch
import torch.nn.functional as F
from accept import ULP24, rel_dev, user_item_dict  # noqa: F401

LATENT = 64
KEEP_PROB = 0.5
ANNEAL_CAP = 0.2
TOTAL_ANNEAL_STEPS = 200000


def hist_csr(edges, U):
    """train_csr_mat's pattern (Model/MultVAE.py:32-35): rowptr [U + 1], col ascending local item ids, distinct."""
    e = np.asarray(edges, dtype=np.int64)
    key = np.unique(e[:, 0] * (1 << 32) + (e[:, 1] - U))
    u, i = key >> 32, key & 0xFFFFFFFF
    rowptr = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(np.bincount(u, minlength=U), out=rowptr[1:])
    return rowptr, i.astype(np.int64)


def dense_rows(rowptr, col, users, I, dtype=torch.float64):
    users = np.asarray(users, dtype=np.int64)
    x = torch.zeros((len(users), I), dtype=dtype)
    for b, u in enumerate(users):
        x[b, col[rowptr[u]:rowptr[u + 1]]] = 1.0
    return x


def flags_from_mask(mask, rowptr, col, users):
    """A dense [B, I] keep mask -> one flag per entry of the samples' history rows (sample 0's row first, CSR order)."""
    mask = np.asarray(mask)
    return np.concatenate([mask[b, col[rowptr[u]:rowptr[u + 1]]] for b, u in enumerate(np.asarray(users))] or
                          [np.zeros(0)]).astype(np.uint8)


def mask_from_flags(flags, rowptr, col, users, I):
    m = np.zeros((len(users), I), dtype=bool)
    o = 0
    for b, u in enumerate(np.asarray(users)):
        c = col[rowptr[u]:rowptr[u + 1]]
        m[b, c] = np.asarray(flags[o:o + len(c)]) != 0
        o += len(c)
    assert o == len(flags)
    return m


def anneal_of(update_count):
    return min(ANNEAL_CAP, 1.0 * update_count / TOTAL_ANNEAL_STEPS)


def step(weights, rowptr, col, users, keep, eps, update_count, reg_weight, training=True, dtype=torch.float64):
    """weights = (Wq [128, I], bq [128], Wp [I, 64], bp [I]); keep: per-entry flags (None: no dropout); eps [B, 64].
    -> dict(loss, neg_ll, kl, anneal, sumsq, lse [B], z [B, 64], grads = (dWq, dbq, dWp, dbp))."""
    Wq, bq, Wp, bp = (torch.as_tensor(np.asarray(w)).to(dtype).clone().requires_grad_(True) for w in weights)
    I = Wp.shape[0]
    x = dense_rows(rowptr, col, users, I, dtype)
    h = F.normalize(x, p=2, dim=1)
    if training and keep is not None:
        h = h * torch.from_numpy(mask_from_flags(keep, rowptr, col, users, I)).to(dtype) / KEEP_PROB
    h = h @ Wq.t() + bq
    mu, logvar = h[:, :LATENT], h[:, LATENT:]
    std = torch.exp(0.5 * logvar)
    kl = torch.sum(0.5 * (-logvar + logvar.exp() + mu.pow(2) - 1), dim=1).mean()
    z = mu + torch.as_tensor(np.asarray(eps)).to(dtype) * std
    logits = z @ Wp.t() + bp
    lse = torch.logsumexp(logits, dim=-1)
    neg_ll = -(F.log_softmax(logits, dim=-1) * x).sum(dim=-1).mean()
    sumsq = sum((p ** 2).sum() for p in (Wq, bq, Wp, bp))
    anneal = anneal_of(update_count)
    loss = neg_ll + anneal * kl + 2 * (reg_weight * (reg_weight * 0.5 * sumsq))
    loss.backward()
    return {"loss": loss.item(), "neg_ll": neg_ll.item(), "kl": kl.item(), "anneal": anneal, "sumsq": sumsq.item(),
            "lse": lse.detach().numpy(), "z": z.detach().numpy(),
            "grads": tuple(p.grad.numpy() for p in (Wq, bq, Wp, bp))}


def adam_trajectory(weights, rowptr, col, batches, keeps, epss, update_count, reg_weight, lr, dtype=torch.float64):
    """len(batches) steps of torch.optim.Adam(lr) (main.py:397 defaults) -> (losses, final weights)."""
    params = [torch.as_tensor(np.asarray(w)).to(dtype).clone().requires_grad_(True) for w in weights]
    opt = torch.optim.Adam(params, lr=lr)
    losses = []
    for t, users in enumerate(batches):
        out = step([p.detach().numpy() for p in params], rowptr, col, users, keeps[t], epss[t], update_count + t, reg_weight,
                   dtype=dtype)
        opt.zero_grad()
        for p, g in zip(params, out["grads"]):
            p.grad = torch.from_numpy(np.asarray(g)).to(dtype)
        opt.step()
        losses.append(out["loss"])
    return np.asarray(losses), tuple(p.detach().numpy() for p in params)


def latent_all(weights, rowptr, col, U, eps, dtype=torch.float64):
    """z of every user in eval mode (no dropout, eps still drawn: Model/MultVAE.py:113)."""
    Wq, bq = (torch.as_tensor(np.asarray(w)).to(dtype) for w in weights[:2])
    n = torch.from_numpy(np.diff(rowptr)).to(dtype)
    rows = torch.from_numpy(np.repeat(np.arange(U), np.diff(rowptr)))
    h = torch.zeros((U, 2 * LATENT), dtype=dtype).index_add_(0, rows, Wq.t()[torch.from_numpy(np.asarray(col))])
    h = h / torch.clamp(n.sqrt(), min=1e-12)[:, None] + bq
    return h[:, :LATENT] + torch.as_tensor(np.asarray(eps)).to(dtype) * torch.exp(0.5 * h[:, LATENT:])


def scores(weights, z, users=None):
    """z . Wp^T + bp for `users` (default all) -> ([n, I] scores, [n, I] sum_k |z_k w_k| for the rounding cap)."""
    Wp, bp = (torch.as_tensor(np.asarray(w)).to(z.dtype) for w in weights[2:])
    zz = z if users is None else z[torch.as_tensor(np.asarray(users))]
    return zz @ Wp.t() + bp, zz.abs() @ Wp.abs().t()


def ranklist_check(ranks, weights, z, hist_rowptr, hist_col, topk=50, chunk=2048, users=None):
    """The ranking condition: `ranks` [n, topk] LOCAL item ids of `users` (default all, in order) against the fp64 scores
    (history -> 1e-6).  -> (share of positions that differ from the fp64 list, the number of differing positions that are
    NOT a swap inside a score gap below 8 * 2^-24 * (sum_k |z_k w_k| + |b|): 65 terms, one rounding each, both rows)."""
    ranks = torch.as_tensor(np.asarray(ranks)).long()
    users = np.arange(ranks.shape[0]) if users is None else np.asarray(users)
    bp = torch.as_tensor(np.asarray(weights[3])).double().abs()
    differ = bad = 0
    for o in range(0, len(users), chunk):
        us = users[o:o + chunk]
        sc, mag = scores(weights, z, us)
        tol = 8.0 * ULP24 * (mag + bp[None, :])
        for r, u in enumerate(us):
            c = torch.as_tensor(hist_col[hist_rowptr[u]:hist_rowptr[u + 1]]).long()
            sc[r, c] = 1e-6
            tol[r, c] = 0.0
        want = torch.topk(sc, topk, dim=1)[1]
        got = ranks[o:o + chunk]
        diff = got != want
        differ += int(diff.sum())
        # a differing position holds an item whose fp64 score is within the gap of the score the fp64 list has there
        gap = (torch.gather(sc, 1, got) - torch.gather(sc, 1, want)).abs()
        allowed = torch.maximum(torch.gather(tol, 1, got), torch.gather(tol, 1, want))
        bad += int((diff & (gap > allowed)).sum())
    return differ / float(ranks.numel()), bad


def load_fixture(golden_dir, name):
    """tests/golden/multvae_<name>.npz as a dict, with the edges (sports: from sports_interactions.npz), the history CSR
    and the unpacked keep flags."""
    import os
    g = dict(np.load(os.path.join(golden_dir, f"multvae_{name}.npz"), allow_pickle=False))
    if "edges" not in g:
        g["edges"] = np.load(os.path.join(golden_dir, f"{name}_interactions.npz"))["train"]
    g["U"], g["I"] = int(g["U"]), int(g["I"])
    g["edges"] = np.asarray(g["edges"], dtype=np.int64)
    g["rowptr"], g["col"] = hist_csr(g["edges"], g["U"])
    g["keep"] = np.unpackbits(g["keep_bits"])[:int(g["n_keep"])]
    if "traj_keep_bits" in g:
        flat, o, g["traj_keeps"] = np.unpackbits(g["traj_keep_bits"]), 0, []
        for n in g["traj_keep_n"]:
            g["traj_keeps"].append(flat[o:o + int(n)])
            o += int(n)
    return g


def replay_draws(seed, B, I):
    """(keep mask [B, I], eps [B, 64]) as the reference's loss() draws them after torch.manual_seed(seed): the generator's
    own recipe (tests/golden/gen_multvae.py), for the fixtures too large to carry eps."""
    torch.manual_seed(int(seed))
    mask = F.dropout(torch.ones(B, I), 0.5) != 0
    return mask.numpy(), torch.randn(B, LATENT).numpy()
