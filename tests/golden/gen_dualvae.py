#!/usr/bin/env python
"""Generate tests/golden/dualvae_small.npz (and dualvae_sports.npz) by running the REFERENCE's DualVAE class on the CPU.

Nothing of the reference is copied: this script imports Model/DualVAE.py from the reference checkout at run time
(CHAOREC_REFERENCE, default /root/reference), feeds it seeded inputs and stores inputs + outputs as .npz data.

    python tests/golden/gen_dualvae.py [small] [sports]

Every reference quantity is stored next to its own fp32-vs-fp64 deviation from the restatement (tests/dualvae_host.py)
on the same weights and draws, relative to the quantity's largest element.  The draws are not stored: replaying
torch.manual_seed + randn in the reference's order (dualvae_host.replay_draws) gives them; their sums are stored.
"""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("CHAOREC_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import dualvae_host as dh  # noqa: E402
import Model.DualVAE as refmod  # noqa: E402

THREADS = 8
torch.set_num_threads(THREADS)
DEV = torch.device("cpu")
TOPK = 50
PROBE = 20
GRAD_ROWS = 128
RANK_CAP = 0.02


def small_case():
    """U 300, I 257 (one row past two 128-tiles, nothing a multiple of a tile); degree-1 users and items; the last user and
    the last item are each other's only edge; B 200 with repeated users and items, one of each four times; every batch
    pair is an edge, so the batch's users lie in the batch items' rows and the reverse."""
    U, I, B = 300, 257, 200
    rng = np.random.default_rng(20260318)
    pairs = {(U - 1, I - 1)}
    for u in range(U - 1):                        # users 0 .. 9 and items 0 .. 9 of degree 1
        n = 1 if u < 10 else int(rng.integers(2, 14))
        for i in rng.choice(np.arange(10, I - 1), size=n, replace=False).tolist():
            pairs.add((u, int(i)))
    for i in range(10):
        pairs.add((10 + i, i))
    e = np.array(sorted(pairs), dtype=np.int64)
    pick = rng.choice(len(e), size=B, replace=True)
    pick[:4] = int(np.nonzero(e[:, 0] == 20)[0][0])                         # user 20 and its first item, four times
    pick[4] = int(np.nonzero((e[:, 0] == U - 1))[0][0])                     # the mutual-only pair
    pick[5] = int(np.nonzero(e[:, 0] == 3)[0][0])                           # a degree-1 user
    pick[6] = int(np.nonzero(e[:, 1] == 4)[0][0])                           # a degree-1 item
    pick[B - 1] = int(np.nonzero(e[:, 0] == 20)[0][-1])                     # user 20 again at the last position (another item)
    rng.shuffle(pick[:B - 1])
    edges = np.stack([e[:, 0], e[:, 1] + U], 1).astype(np.int32)
    return U, I, edges, edges[pick, 0].astype(np.int64), edges[pick, 1].astype(np.int64)


def sports_case():
    g = np.load(os.path.join(HERE, "sports_interactions.npz"))
    U, I, edges = int(g["U"]), int(g["I"]), g["train"].astype(np.int32)
    rng = np.random.default_rng(7)
    pick = rng.choice(len(edges), size=2048, replace=False)
    return U, I, edges, edges[pick, 0].astype(np.int64), edges[pick, 1].astype(np.int64)


def weights_of(model):
    sd = model.state_dict()
    assert tuple(sd.keys()) == dh.NAMES, tuple(sd.keys())
    return [v.detach().numpy().copy() for v in sd.values()]


def tables_of(model):
    return tuple(t.detach().numpy().copy() for t in (model.theta, model.beta, model.mu_theta, model.mu_beta))


def ref_step(model, users, pos):
    """The reference's loss() with its two sides' pieces recorded (contrast_loss's arguments are z and nei)."""
    rec = []
    inner = model.contrast_loss

    def recording(x, x_):
        rec.append((x.detach().numpy().copy(), x_.detach().numpy().copy()))
        return inner(x, x_)

    sides = []
    fwd = model.forward

    def forward(*a, **kw):
        torch.set_num_threads(THREADS)
        if kw.get("theta") is not None:
            # loss() writes theta[users] through .data before backward() runs, and autograd has saved VIEWS of the table:
            # as written, the item side's backward would read rows its forward never saw.  The fixture holds the gradient of
            # the loss the forward computed, so the item side is given a copy that stays as it was.
            kw["theta"] = kw["theta"].clone()
        out = fwd(*a, **kw)
        sides.append((float(out[3].detach()), float(out[4].detach())))
        # the table write-back that follows is an index_put_ with repeated ids: on one thread the highest batch position
        # wins; on several, each aspect's winner is whichever thread came last
        torch.set_num_threads(1)
        return out

    lo = model._loss

    def _loss(x, x_, kl, kl_beta, cl, cl_gama):
        out = lo(x, x_, kl, kl_beta, cl, cl_gama)
        sides[-1] = sides[-1] + (float(torch.mean(torch.sum(x * torch.log(x_ + refmod.EPS) - x_, dim=-1))), float(out))
        return out

    model.contrast_loss, model.forward, model._loss = recording, forward, _loss
    try:
        loss = model.loss(torch.from_numpy(users), torch.from_numpy(pos), torch.from_numpy(pos))
    finally:
        del model.contrast_loss, model.forward, model._loss
        torch.set_num_threads(THREADS)
    out = {"loss": loss}
    for name, (z, nei), (kl, cl, ll, sl) in zip(("item", "user"), rec, sides):
        out[name] = dict(z=z, nei=nei, kl=kl, cl=cl, ll=ll, loss=sl)
    return out


def generate(name):
    U, I, edges, users, pos = small_case() if name == "small" else sports_case()
    seed, draw_seed, B = 11, 1234, len(users)
    hist = dh.user_item_dict(edges)
    torch.manual_seed(seed)
    model = refmod.DualVAE(U, I, edges.astype(np.int64), hist, 64, dh.KL_WEIGHT, dh.SSL_REG, DEV)
    w0, t0 = weights_of(model), tables_of(model)
    X = dh.dense_matrix(edges, U, I)
    g = dict(U=U, I=I, edges=edges, users=users, pos=pos, seed=seed, draw_seed=draw_seed, topk=TOPK,
             w_sum=np.array([float(x.astype(np.float64).sum()) for x in w0]),
             w_probe=np.stack([x.reshape(-1)[:PROBE] for x in w0]),
             t_sum=np.array([float(x.astype(np.float64).sum()) for x in t0]))

    # one step
    torch.manual_seed(draw_seed)
    ref = ref_step(model, users, pos)
    ref["loss"].backward()
    ref_grads = [p.grad.detach().numpy().copy() for _, p in model.named_parameters()]
    ei, eu = dh.replay_draws(draw_seed, B)
    g["draw_sums"] = dh.draw_sums((ei, eu))
    out = dh.step(w0, t0, X, users, pos - U, ei, eu)
    g["ref_loss"], g["dev_loss"] = float(ref["loss"]), dh.rel_dev(float(ref["loss"]), out["loss"])
    for s in ("item", "user"):
        for k in ("kl", "ll", "cl", "loss"):
            g[f"ref_{s}_{k}"], g[f"dev_{s}_{k}"] = ref[s][k], dh.rel_dev(ref[s][k], out[s][k])
        for k in ("z", "nei"):
            g[f"dev_{s}_{k}"] = dh.rel_dev(ref[s][k], out[s][k])
            g[f"ref_{s}_{k}"] = ref[s][k] if name == "small" else ref[s][k][:GRAD_ROWS]
        print(name, s, {k: (g[f"ref_{s}_{k}"], g[f"dev_{s}_{k}"]) for k in ("kl", "ll", "cl")}, g[f"dev_{s}_z"], g[f"dev_{s}_nei"])
    rng = np.random.default_rng(3)
    g["grad_rows_user"] = np.sort(rng.choice(I, size=min(I, GRAD_ROWS), replace=False))      # columns of user_encoder.fc0.weight
    g["grad_rows_item"] = np.sort(rng.choice(U, size=min(U, GRAD_ROWS), replace=False))
    devs = []
    for k, n in enumerate(dh.NAMES):
        devs.append(dh.rel_dev(ref_grads[k], out["grads"][k]))
        r = ref_grads[k]
        if n == "user_encoder.fc0.weight":
            r = r[:, g["grad_rows_user"]]
        elif n == "item_encoder.fc0.weight":
            r = r[:, g["grad_rows_item"]]
        g[f"ref_grad_{k}"] = r
        print(name, n, "grad deviation", devs[-1], "scale", float(np.abs(out["grads"][k]).max()))
    g["dev_grads"] = np.array(devs)
    g["gnorm"] = np.array([float(np.linalg.norm(x)) for x in out["grads"]])
    # the write-back: the reference's tables against the restatement's (highest batch position wins), sampled at the batch ids
    t1 = tables_of(model)
    for k, (ids, n) in enumerate(((users, "theta"), (pos - U, "beta"), (users, "mu_theta"), (pos - U, "mu_beta"))):
        ids = np.unique(ids)[:GRAD_ROWS]
        g[f"tab_ids_{n}"], g[f"ref_tab_{n}"] = ids, t1[k][ids]
        g[f"dev_tab_{n}"] = dh.rel_dev(t1[k], out["tables"][k])
        assert g[f"dev_tab_{n}"] < 1e-4, (n, g[f"dev_tab_{n}"])      # (another winner would be a whole draw away)

    if name == "small":
        # ten Adam steps (torch.optim.Adam at the YAML's learning rate x 10, so that ten steps move the weights)
        T, lr, seed0 = 10, 0.01, 5000
        torch.manual_seed(seed)
        tmodel = refmod.DualVAE(U, I, edges.astype(np.int64), hist, 64, dh.KL_WEIGHT, dh.SSL_REG, DEV)
        opt = torch.optim.Adam(tmodel.parameters(), lr=lr)
        rng = np.random.default_rng(99)
        batches, losses = [], []
        for t in range(T):
            pick = rng.choice(len(edges), size=B, replace=True)
            bu, bp = edges[pick, 0].astype(np.int64), edges[pick, 1].astype(np.int64)
            batches.append((bu, bp - U))
            torch.manual_seed(seed0 + t)
            opt.zero_grad()
            loss = ref_step(tmodel, bu, bp)["loss"]
            loss.backward()
            opt.step()
            losses.append(float(loss))
        hl, hw, ht = dh.adam_trajectory(w0, t0, X, batches, seed0, lr)
        wT, tT = weights_of(tmodel), tables_of(tmodel)
        g.update(traj_users=np.stack([b[0] for b in batches]), traj_pos=np.stack([b[1] + U for b in batches]), traj_seed0=seed0,
                 traj_lr=lr, traj_ref_losses=np.array(losses), traj_dev_losses=dh.rel_dev(losses, hl),
                 traj_ref_probe=np.stack([x.reshape(-1)[:PROBE] for x in wT]),
                 traj_dev_weights=np.array([dh.rel_dev(a, b) for a, b in zip(wT, hw)]),
                 traj_dev_tables=np.array([dh.rel_dev(a, b) for a, b in zip(tT, ht)]))
        print(name, "trajectory deviations", g["traj_dev_losses"], g["traj_dev_weights"].max(), g["traj_dev_tables"])

    # ranking with ASSIGNED mu tables (after few steps most rows are zero and the scores tie at 0.0 exactly)
    rank_users = np.arange(U) if name == "small" else np.sort(np.random.default_rng(5).choice(U, size=512, replace=False))
    g["rank_users"] = rank_users
    for tag, scale in (("s01", 0.1), ("s10", 1.0)):
        gen = torch.Generator().manual_seed(77)
        model.mu_theta = torch.randn(U, dh.A, dh.K, generator=gen) * scale
        model.mu_beta = torch.randn(I, dh.A, dh.K, generator=gen) * scale
        with torch.no_grad():
            ranks = model.gene_ranklist(TOPK).numpy()[rank_users]
        sc = dh.scores(weights_of(model), model.mu_theta.numpy(), model.mu_beta.numpy(), rank_users)
        share, bad = dh.ranklist_check(ranks, sc, hist, rank_users, TOPK, U)
        print(name, tag, "reference fp32 list vs fp64 list: share", share, "outside the gap", bad)
        if share > RANK_CAP or bad:
            raise SystemExit(f"{name} {tag}: the reference's own list differs at {share:.4f} of positions ({bad} outside the gap)")
        g[f"rank_{tag}"], g[f"rank_share_{tag}"] = (ranks - U).astype(np.int16), share

    if name == "sports":
        del g["edges"]                       # (dualvae_host.load_fixture reads them from sports_interactions.npz)
    path = os.path.join(HERE, f"dualvae_{name}.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    for case in (sys.argv[1:] or ["small", "sports"]):
        generate(case)
