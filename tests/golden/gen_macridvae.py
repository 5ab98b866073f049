#!/usr/bin/env python3
"""Generate tests/golden/macridvae_small.npz and macridvae_sports.npz by running the REFERENCE's MacridVAE class on the CPU.

Runs only where the reference checkout is (CHAOREC_REFERENCE); nothing from it is copied: this script imports its
Model/MacridVAE.py, feeds it seeded inputs and stores inputs + outputs as .npz data.

    python tests/golden/gen_macridvae.py [small] [sports]

The draws are recovered without touching the reference: after torch.manual_seed(s) one training forward consumes the
generator as a dropout Bernoulli over [B, I], exponential_ over [I, K] and normal_(0, std) over [B, D] once per concept;
replaying the three calls with the same seed (tests/macridvae_host.py replay_draws) gives the keep mask, the Gumbel noise
and eps -- the fixtures store only their checksums.  What the reference's forward() keeps to itself (the concept weights,
the normalised latents) is recorded by wrapping the two torch.nn.functional calls it makes.  Every reference quantity is
stored with its deviation from the float64 restatement on the same weights and draws: 4 x that deviation is the bound
the tests use.  The eval-mode rank list is checked against the ranking cap here, and a fixture whose reference list
breaks it is not written.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("CHAOREC_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import macridvae_host as mh  # noqa: E402
import Model.MacridVAE as refmod  # noqa: E402

torch.set_num_threads(8)
DEV = torch.device("cpu")
TOPK = 50
D = 64
RECORD = {"normalize": [], "gumbel": []}


def _recording(name, fn):
    def wrapped(*a, **kw):
        out = fn(*a, **kw)
        RECORD[name].append(out.detach())
        return out
    return wrapped


# the reference module's `F`: torch.nn.functional with two calls recorded
refmod.F = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith("__")})
refmod.F.normalize = _recording("normalize", F.normalize)
refmod.F.gumbel_softmax = _recording("gumbel", F.gumbel_softmax)


def weights_of(model):
    sd = model.state_dict()
    assert tuple(sd.keys()) == mh.NAMES, tuple(sd.keys())
    return tuple(v.detach().numpy().copy() for v in sd.values())


def ref_step(model, users, seed, update_before):
    """One reference loss() + backward() -> fp32 loss, gradients, and the parts loss() hides."""
    model.train()
    model.training = True
    model.zero_grad()
    model.update = int(update_before)
    dummy = torch.full_like(users, model.num_user)
    for v in RECORD.values():
        v.clear()
    torch.manual_seed(seed)
    loss = model.loss(users, dummy, dummy)
    loss.backward()
    assert model.update == update_before + 1
    grads = tuple(p.grad.numpy().copy() for p in model.parameters())
    norm, cates = list(RECORD["normalize"]), RECORD["gumbel"][0]
    assert len(norm) == 3 + 2 * mh.K
    zh = torch.stack([norm[3 + 2 * k + 1] for k in range(mh.K)], 1)           # cores, items, rows, then (mu, z) per concept
    with torch.no_grad():                        # its forward() once more on the same draws, for the logits it returns
        rows = model.rating_matrix.to_dense()[users]
        torch.manual_seed(seed)
        logits, _, logvar = model.forward(rows)
    # ce and kl in the restatement's own formulation (tests/macridvae_host.py), evaluated in fp32 on the reference's outputs
    n = rows.sum(1)
    lse = torch.logsumexp(logits, dim=1)
    ce = (n * lse - (logits * rows).sum(1)).mean()
    lv = torch.stack(logvar, 1)
    kl = (-0.5 * (1 + lv - lv.exp()).sum(2).mean(0)).sum()
    return {"loss": float(loss.detach()), "ce": float(ce), "kl": float(kl), "lse": lse.numpy(), "z": zh.numpy(),
            "cates": cates.numpy(), "grads": grads}


def make(name, edges, U, I, users, seed, sports):
    edges = np.asarray(edges, dtype=np.int64)
    assert edges[:, 1].min() >= U and edges[:, 1].max() < U + I
    rowptr, col = mh.hist_csr(edges, U)
    g = {"I": I, "D": D, "rowptr": rowptr, "col": col}
    B = len(users)
    out = {"U": U, "I": I, "D": D, "edges": edges.astype(np.int32), "users": users.astype(np.int64), "seed": seed, "topk": TOPK}
    torch.manual_seed(seed)
    model = refmod.MacridVAE(U, I, edges.copy(), mh.user_item_dict(edges), D, 0.0, DEV)   # (its constructor shifts the item ids of the array it is given, in place)
    w0 = weights_of(model)
    out["w_sum"] = np.asarray([w.astype(np.float64).sum() for w in w0])
    out["w_probe"] = np.stack([w.reshape(-1)[:64] for w in w0])

    # eval-mode rank list, checked against the ranking cap (row-independent: sports takes 512 sampled users' dense rows)
    rank_users = np.arange(0, U, max(1, U // 512))[:512] if sports else np.arange(U)
    model.training = False
    with torch.no_grad():
        if sports:
            sc = model.forward(model.rating_matrix.to_dense()[torch.from_numpy(rank_users)])[0].detach()
            for r, u in enumerate(rank_users):                    # its mask and topk statement on those rows
                sc[r][torch.LongTensor(list(model.user_item_dict[int(u)])) - U] = 1e-6
            ranks = torch.topk(sc, TOPK)[1].numpy()
        else:
            ranks = model.gene_ranklist(TOPK).numpy() - U
    assert model.training is False
    share, bad = mh.ranklist_check(ranks, w0, rowptr, col, rowptr, col, rank_users, TOPK)
    print(f"{name}: reference fp32 list differs from fp64 at {share:.4%} of positions, {bad} outside the gap")
    if share > 0.02 or bad:
        raise SystemExit(f"{name}: the reference's own list breaks the ranking cap on seed {seed}: no fixture written")
    out.update(rank_users=rank_users, ranks=ranks.astype(np.int16), rank_ref_share=share)

    # one training step at update 0 (anneal 1 / 200 000) and one where the anneal sits at its cap
    draw_seed = seed + 1
    keep, gumbel, eps = mh.case_draws(g, draw_seed, users)
    out.update(draw_seed=draw_seed, draw_sums=mh.draw_sums(keep, gumbel, eps))
    for tag, upd in (("", 0), ("a_", 123456)):
        ref = ref_step(model, torch.from_numpy(users), draw_seed, upd)
        f64 = mh.step(w0, rowptr, col, users, keep, gumbel, eps, upd)
        for k in ("loss", "ce", "kl"):
            out[f"{tag}ref_{k}"], out[f"{tag}dev_{k}"] = ref[k], mh.rel_dev(ref[k], f64[k])
        for k in ("lse", "z", "cates"):
            out[f"{tag}dev_{k}"] = mh.rel_dev(ref[k], f64[k])
        out[f"{tag}dev_grads"] = np.asarray([mh.rel_dev(a, b) for a, b in zip(ref["grads"], f64["grads"])])
        out[f"{tag}ref_gnorm"] = np.asarray([float(np.linalg.norm(x.astype(np.float64))) for x in ref["grads"]])
        print(name, tag, {k: (out[f"{tag}ref_{k}"], out[f"{tag}dev_{k}"]) for k in ("loss", "ce", "kl")},
              {k: out[f"{tag}dev_{k}"] for k in ("lse", "z", "cates")}, out[f"{tag}dev_grads"])
        assert out[f"{tag}dev_loss"] < 1e-4, "the fp64 restatement does not meet the reference"
    out.update(ref_lse=ref["lse"])
    rng = np.random.default_rng(seed)
    rows = np.sort(rng.choice(I, min(I, 128), replace=False))
    out.update(grad_rows=rows, ref_dW1_rows=ref["grads"][0][:, rows].T.copy(), ref_dE_rows=ref["grads"][4][rows],
               ref_db1=ref["grads"][1], ref_dK=ref["grads"][5], ref_cates_rows=ref["cates"][rows])

    if not sports:
        assert len(set(users.tolist())) < B, "the batch must repeat users"
        # 10 Adam steps from update 39 994: the anneal (read AFTER the increment) reaches its cap inside the run
        lr, u0, T, TB = 0.01, 39994, 10, 64
        torch.manual_seed(seed)
        model = refmod.MacridVAE(U, I, edges.copy(), mh.user_item_dict(edges), D, 0.0, DEV)   # (its constructor shifts the item ids of the array it is given, in place)
        opt = torch.optim.Adam(model.parameters(), lr=lr)
        rng = np.random.default_rng(seed + 7)
        batches = [rng.integers(0, U, TB).astype(np.int64) for _ in range(T)]
        draws = [mh.case_draws(g, draw_seed + 100 + t, batches[t]) for t in range(T)]
        keeps, gumbels, epss, losses = [d[0] for d in draws], [d[1] for d in draws], [d[2] for d in draws], []
        model.train()
        model.training = True
        model.update = u0
        for t in range(T):
            opt.zero_grad()
            torch.manual_seed(draw_seed + 100 + t)
            dummy = torch.full((TB,), U, dtype=torch.int64)
            loss = model.loss(torch.from_numpy(batches[t]), dummy, dummy)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        assert model.update == u0 + T
        wT = weights_of(model)
        l64, w64 = mh.adam_trajectory(w0, rowptr, col, batches, keeps, gumbels, epss, u0, lr)
        out.update(traj_lr=lr, traj_update=u0, traj_batches=np.stack(batches), traj_seed0=draw_seed + 100,
                   traj_ref_losses=np.asarray(losses), traj_dev_losses=mh.rel_dev(losses, l64),
                   traj_ref_wsum=np.asarray([w.astype(np.float64).sum() for w in wT]),
                   traj_ref_probe=np.stack([w.reshape(-1)[:64] for w in wT]),
                   traj_dev_weights=np.asarray([mh.rel_dev(a, b) for a, b in zip(wT, w64)]))
        print(name, "trajectory", losses, out["traj_dev_losses"], out["traj_dev_weights"])
    path = os.path.join(HERE, f"macridvae_{name}.npz")
    if sports:
        del out["edges"]          # (tests/golden/sports_interactions.npz has them)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def small():
    rng = np.random.default_rng(5)
    U, I = 300, 257
    edges = set()
    for u in range(U):
        deg = 1 if u < 12 else int(rng.integers(2, 14))
        for i in rng.choice(I - 1, deg, replace=False):      # item I - 1 is left to user 299 alone
            edges.add((u, U + int(i)))
    edges.add((U - 1, U + I - 1))
    edges = np.asarray(sorted(edges))
    users = rng.integers(0, U - 1, 200)
    users[:8] = [3, 3, 3, 3, 5, 5, 5, 5]                      # degree-1 users, repeated
    make("small", edges, U, I, users.astype(np.int64), 11, sports=False)


def sports():
    d = np.load(os.path.join(HERE, "sports_interactions.npz"))
    U, I = int(d["U"]), int(d["I"])
    rng = np.random.default_rng(3)
    users = rng.integers(0, U, 2048).astype(np.int64)
    make("sports", d["train"], U, I, users, 21, sports=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["small", "sports"]
    if "small" in which:
        small()
    if "sports" in which:
        sports()
