#!/usr/bin/env python3
"""Generate tests/golden/multvae_small.npz and multvae_sports.npz by running the REFERENCE's MultVAE class on the CPU.

Runs only where the reference checkout is (CHAOREC_REFERENCE); nothing from it is copied: this script imports its
Model/MultVAE.py (pure torch + scipy), feeds it seeded inputs and stores inputs + outputs as .npz data.

    python tests/golden/gen_multvae.py [small] [sports]

The draws are recovered without touching the reference: after torch.manual_seed(s), loss() consumes the generator as
dropout(normalize(x)) -- a Bernoulli draw per element of [B, I], whatever the values -- and then randn(B, 64); replaying
the two calls with the same seed gives the keep mask and eps.  Every reference quantity is stored with its deviation
from the float64 restatement (tests/multvae_host.py) on the same weights and draws: 4 x that deviation is the bound the
tests use.  The eval-mode rank list is checked against the ranking cap here, and a fixture whose reference list breaks
it is not written.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REF = os.environ.get("CHAOREC_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, REF)

import multvae_host as mh  # noqa: E402
from Model.MultVAE import MultVAE  # noqa: E402

torch.set_num_threads(8)
DEV = torch.device("cpu")
TOPK = 50


def uid(edges):
    d = {}
    for u, i in np.asarray(edges).tolist():
        d.setdefault(u, []).append(i)
    return d


def weights_of(model):
    return tuple(p.detach().numpy().copy() for p in (model.layers_q[0].weight, model.layers_q[0].bias,
                                                     model.layers_p[0].weight, model.layers_p[0].bias))


def draws(seed, B, I):
    torch.manual_seed(seed)
    mask = F.dropout(torch.ones(B, I), 0.5) != 0
    eps = torch.randn(B, mh.LATENT)
    return mask.numpy(), eps.numpy()


def ref_step(model, users, seed, update_count):
    """One reference loss() + backward() -> fp32 loss parts, lse, z, gradients."""
    model.train()
    model.zero_grad()
    model.update_count = float(update_count)
    dummy = torch.full_like(users, model.num_user)
    torch.manual_seed(seed)
    loss = model.loss(users, dummy, dummy)
    loss.backward()
    grads = tuple(p.grad.numpy().copy() for p in (model.layers_q[0].weight, model.layers_q[0].bias,
                                                  model.layers_p[0].weight, model.layers_p[0].bias))
    with torch.no_grad():                       # the same calls in the same order once more, for the parts loss() hides
        x = torch.from_numpy(model.train_csr_mat[users.numpy()].toarray()).float()
        torch.manual_seed(seed)
        mu, std, kl = model.q_graph(x)
        z = mu + torch.randn_like(std) * std
        logits = model.p_graph(z)
        lse = torch.logsumexp(logits, dim=-1)
        neg_ll = -torch.mul(F.log_softmax(logits, dim=-1), x).sum(dim=-1).mean()
    return {"loss": float(loss.detach()), "neg_ll": float(neg_ll), "kl": float(kl), "lse": lse.numpy(), "z": z.numpy(), "grads": grads}


def make(name, edges, U, I, users, reg_weight, seed, sports):
    edges = np.asarray(edges, dtype=np.int64)
    assert edges[:, 1].min() >= U and edges[:, 1].max() < U + I
    rowptr, col = mh.hist_csr(edges, U)
    B = len(users)
    out = {"U": U, "I": I, "edges": edges.astype(np.int32), "users": users.astype(np.int64), "reg_weight": reg_weight,
           "seed": seed, "topk": TOPK}
    torch.manual_seed(seed)
    model = MultVAE(U, I, edges, uid(edges), 64, reg_weight, DEV)
    w0 = weights_of(model)
    names = ("layers_q.0.weight", "layers_q.0.bias", "layers_p.0.weight", "layers_p.0.bias")
    assert tuple(model.state_dict().keys()) == names
    out["w_sum"] = np.asarray([w.astype(np.float64).sum() for w in w0])
    out["w_probe"] = np.stack([w.reshape(-1)[:64] for w in w0])
    if not sports:
        out.update(Wq=w0[0], bq=w0[1], Wp=w0[2], bp=w0[3])

    # eval-mode rank list (dropout off, eps drawn: Model/MultVAE.py:113), checked against the ranking cap
    rank_seed = seed + 1000
    while True:
        model.eval()
        torch.manual_seed(rank_seed)
        ranks = model.gene_ranklist(TOPK).numpy() - U
        torch.manual_seed(rank_seed)
        eps_rank = torch.randn(U, mh.LATENT).numpy()
        z64 = mh.latent_all(w0, rowptr, col, U, eps_rank)
        share, bad = mh.ranklist_check(ranks, w0, z64, rowptr, col, TOPK)
        print(f"{name}: rank seed {rank_seed}: reference fp32 list differs from fp64 at {share:.4%} of positions, {bad} outside the gap")
        if share <= 0.02 and bad == 0:
            break
        rank_seed += 1
    out.update(rank_seed=rank_seed, rank_ref_share=share, eps_rank_sum=float(eps_rank.astype(np.float64).sum()))
    if sports:
        rank_users = np.arange(0, U, max(1, U // 512))[:512]
        out.update(rank_users=rank_users, ranks=ranks[rank_users].astype(np.int16))
    else:
        out.update(ranks=ranks.astype(np.int16), eps_rank=eps_rank)

    # one training step
    draw_seed = seed + 1
    ref = ref_step(model, torch.from_numpy(users), draw_seed, 0.0)
    mask, eps = draws(draw_seed, B, I)
    keep = mh.flags_from_mask(mask, rowptr, col, users)
    f64 = mh.step(w0, rowptr, col, users, keep, eps, 0, reg_weight)
    # a second step where anneal * kl is live (update_count 0 switches the KL term off)
    ref_a = ref_step(model, torch.from_numpy(users), draw_seed, 123456.0)
    f64_a = mh.step(w0, rowptr, col, users, keep, eps, 123456, reg_weight)
    out.update(draw_seed=draw_seed, keep_bits=np.packbits(keep), n_keep=len(keep), eps_sum=float(eps.astype(np.float64).sum()))
    for tag, r, f in (("", ref, f64), ("a_", ref_a, f64_a)):
        for k in ("loss", "neg_ll", "kl"):
            out[f"{tag}ref_{k}"], out[f"{tag}dev_{k}"] = r[k], mh.rel_dev(r[k], f[k])
        out[f"{tag}dev_grads"] = np.asarray([mh.rel_dev(a, b) for a, b in zip(r["grads"], f["grads"])])
        out[f"{tag}ref_gnorm"] = np.asarray([float(np.linalg.norm(g.astype(np.float64))) for g in r["grads"]])
        print(name, tag, {k: (out[f"{tag}ref_{k}"], out[f"{tag}dev_{k}"]) for k in ("loss", "neg_ll", "kl")}, out[f"{tag}dev_grads"])
        assert out[f"{tag}dev_loss"] < 1e-4, "the fp64 restatement does not meet the reference"
    out.update(ref_lse=ref["lse"], dev_lse=mh.rel_dev(ref["lse"], f64["lse"]), dev_z=mh.rel_dev(ref["z"], f64["z"]))
    cnt = np.diff(rowptr)[users]
    touched = np.zeros(I, dtype=bool)
    for u in users:
        touched[col[rowptr[u]:rowptr[u + 1]]] = True
    if sports:
        rng = np.random.default_rng(seed)
        rows = np.sort(rng.choice(I, 256, replace=False))
        out.update(grad_rows=rows, ref_dWq_rows=ref_a["grads"][0][:, rows].T.copy(), ref_dWp_rows=ref_a["grads"][2][rows],
                   ref_dbp_rows=ref_a["grads"][3][rows], ref_dbq=ref_a["grads"][1])
    else:
        out.update(eps=eps, ref_z=ref["z"], ref_dWq=ref_a["grads"][0], ref_dbq=ref_a["grads"][1], ref_dWp=ref_a["grads"][2],
                   ref_dbp=ref_a["grads"][3])
        off = np.cumsum(cnt) - cnt
        dropped = [b for b in range(B) if cnt[b] > 0 and not keep[off[b]:off[b] + cnt[b]].any()]
        assert len(set(users.tolist())) < B, "the batch must repeat users"
        assert dropped, "no sample whose whole row is dropped: pick another seed"
        assert (~touched).any(), "every item is touched by the batch"
        out.update(dropped_sample=dropped[0], untouched_item=int(np.nonzero(~touched)[0][0]))

        # 10 Adam steps from update_count 39 995: anneal crosses its cap at 40 000
        lr, uc0, T, TB = 0.01, 39995, 10, 64        # (a smaller batch: ten steps' eps stay within the fixture size)
        torch.manual_seed(seed)
        model = MultVAE(U, I, edges, uid(edges), 64, reg_weight, DEV)
        opt = torch.optim.Adam(model.parameters(), lr=lr)
        rng = np.random.default_rng(seed + 7)
        batches = [rng.integers(0, U, TB).astype(np.int64) for _ in range(T)]
        keeps, epss, losses = [], [], []
        model.train()
        model.update_count = float(uc0)
        for t in range(T):
            m_t, e_t = draws(draw_seed + 100 + t, TB, I)
            keeps.append(mh.flags_from_mask(m_t, rowptr, col, batches[t]))
            epss.append(e_t)
            opt.zero_grad()
            torch.manual_seed(draw_seed + 100 + t)
            dummy = torch.full((TB,), U, dtype=torch.int64)
            loss = model.loss(torch.from_numpy(batches[t]), dummy, dummy)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        assert model.update_count == uc0 + T
        wT = weights_of(model)
        l64, w64 = mh.adam_trajectory(w0, rowptr, col, batches, keeps, epss, uc0, reg_weight, lr)
        out.update(traj_lr=lr, traj_update_count=uc0, traj_batches=np.stack(batches), traj_eps=np.stack(epss),
                   traj_keep_bits=np.packbits(np.concatenate(keeps)), traj_keep_n=np.asarray([len(k) for k in keeps]),
                   traj_ref_losses=np.asarray(losses), traj_dev_losses=mh.rel_dev(losses, l64),
                   traj_ref_Wq=wT[0], traj_ref_bq=wT[1], traj_ref_Wp=wT[2], traj_ref_bp=wT[3],
                   traj_dev_weights=np.asarray([mh.rel_dev(a, b) for a, b in zip(wT, w64)]))
        print(name, "trajectory", losses, out["traj_dev_losses"], out["traj_dev_weights"])
    path = os.path.join(HERE, f"multvae_{name}.npz")
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
    users[:8] = [3, 3, 3, 3, 5, 5, 5, 5]                      # degree-1 users, repeated: some row is dropped whole
    make("small", edges, U, I, users.astype(np.int64), 0.01, 11, sports=False)


def sports():
    d = np.load(os.path.join(HERE, "sports_interactions.npz"))
    U, I = int(d["U"]), int(d["I"])
    rng = np.random.default_rng(3)
    users = rng.integers(0, U, 2048).astype(np.int64)
    make("sports", d["train"], U, I, users, 0.01, 21, sports=True)


if __name__ == "__main__":
    which = sys.argv[1:] or ["small", "sports"]
    if "small" in which:
        small()
    if "sports" in which:
        sports()
