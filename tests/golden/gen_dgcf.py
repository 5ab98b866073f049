#!/usr/bin/env python3
"""Generate tests/golden/dgcf_small.npz and dgcf_baby.npz by running the REFERENCE's DGCF class.

Runs only where the reference checkout is (CHAOREC_REFERENCE); nothing from it is copied: this script imports its
Model/DGCF.py and utils.py, feeds them seeded inputs and stores inputs + outputs as .npz data.

    python tests/golden/gen_dgcf.py [small] [baby]

Model/DGCF.py imports torch_geometric (not installed): oracle/pyg_standin.py provides the restated propagate / degree, as
for gen_golden.py.  DGCF also imports GCNConv, which it never uses; this script supplies that name (a placeholder class)
without touching the stand-in.
"""
import os
import sys
import warnings

import numpy as np
import torch

REF = os.environ.get("CHAOREC_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle import pyg_standin  # noqa: E402

pyg_standin.install()


class _UnusedGCNConv(torch.nn.Module):
    """Model/DGCF.py:11 imports GCNConv and never uses it."""


sys.modules["torch_geometric.nn"].GCNConv = _UnusedGCNConv
sys.path.insert(0, REF)
_argv = sys.argv
sys.argv = ["main.py", "--Model", "DGCF", "--data_path", "baby"]
warnings.filterwarnings("ignore")
from Model.DGCF import DGCF  # noqa: E402

sys.argv = _argv
torch.set_num_threads(8)
DEV = torch.device("cpu")
CASES = ((1, 1), (2, 2), (4, 1), (4, 3))     # (n_factors, n_iterations)


def uid(edges):
    d = {}
    for u, i in edges.tolist():
        d.setdefault(u, []).append(i)
    return d


def small_graph(U, I, deg_lo, deg_hi, seed):
    """gen_golden.small_graph, plus repeated interactions (the edge list keeps them) and a user / an item with no edge."""
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(U - 1):                        # the last user has no interaction
        k = int(rng.integers(deg_lo, deg_hi + 1))
        for i in rng.choice(I - 1, k, replace=False):       # the last item has none either
            rows.append((u, int(i) + U))
    rows += [rows[3], rows[10], rows[10]]         # repeats
    return np.array(rows, dtype=np.int32)


def batch(e, U, I, B, seed):
    rng = np.random.default_rng(seed)
    b = rng.choice(len(e), B, replace=False)
    return (e[b, 0].astype(np.int64), e[b, 1].astype(np.int64), rng.integers(U, U + I, B).astype(np.int64))


def run_case(U, I, e, D, K, T, L, reg, cor, users, pos, neg, steps, lr, topk):
    torch.manual_seed(0)
    m = DGCF(U, I, e, uid(e), D, reg, cor, K, T, L, "add", DEV)
    out = {"p_user": m.user_intent_embeddings.weight.detach().numpy().copy(),
           "p_item": m.item_intent_embeddings.weight.detach().numpy().copy()}
    bt = tuple(torch.from_numpy(t) for t in (users, pos, neg))
    loss = m.loss(*bt)
    loss.backward()
    out.update(result=m.result.detach().numpy().copy(), S=m.S.detach().numpy().copy(), loss=np.float64(loss.item()),
               loss_shape=np.array(loss.shape, dtype=np.int64),
               g_user=m.user_intent_embeddings.weight.grad.numpy().copy(),
               g_item=m.item_intent_embeddings.weight.grad.numpy().copy(),
               cor=np.float64((m.cor_loss(bt[0], bt[1] - U)).item()))
    if topk:
        DGCF.gene_ranklist.__defaults__ = (topk,)
        out["rank"] = m.gene_ranklist().numpy()
        DGCF.gene_ranklist.__defaults__ = (50,)
    if steps:
        torch.manual_seed(0)
        m = DGCF(U, I, e, uid(e), D, reg, cor, K, T, L, "add", DEV)
        opt = torch.optim.Adam([{"params": m.parameters(), "lr": lr}])
        tl, ts = [], []
        for _ in range(steps):
            opt.zero_grad()
            loss = m.loss(*bt)
            loss.backward()
            opt.step()
            tl.append(loss.item())
            ts.append(m.S.detach().numpy().copy())
        out.update(traj_loss=np.array(tl), traj_S=np.stack(ts), traj_user=m.user_intent_embeddings.weight.detach().numpy(),
                   traj_item=m.item_intent_embeddings.weight.detach().numpy())
    return out


def gen_small():
    U, I, D, L, reg, cor = 48, 40, 16, 3, 1e-3, 0.01
    e = small_graph(U, I, 3, 7, 31)
    users, pos, neg = batch(e, U, I, 32, 32)
    data = dict(U=U, I=I, edges=e, D=D, L=L, reg=reg, corDecay=cor, users=users, pos=pos, neg=neg, lr=1e-2, topk=10,
                cases=np.array(CASES, dtype=np.int64))
    for K, T in CASES:
        out = run_case(U, I, e, D, K, T, L, reg, cor, users, pos, neg, 3, 1e-2, 10)
        data.update({f"k{K}t{T}_{k}": v for k, v in out.items()})
    np.savez_compressed(os.path.join(HERE, "dgcf_small.npz"), **data)


def gen_baby():
    z = np.load(os.path.join(HERE, "baby_interactions.npz"))
    U, I, e = int(z["U"]), int(z["I"]), z["train"].astype(np.int32)
    D, K, T, L, reg, cor, B = 64, 4, 3, 3, 1e-3, 0.001, 256
    users, pos, neg = batch(e, U, I, B, 41)
    out = run_case(U, I, e, D, K, T, L, reg, cor, users, pos, neg, 0, 0.0, 0)
    rng = np.random.default_rng(42)
    rows = np.sort(rng.choice(U + I, 256, replace=False))
    grows = np.unique(np.concatenate([users, pos])).astype(np.int64)[:256]
    edges_s = np.sort(rng.choice(len(e), 1024, replace=False))
    np.savez_compressed(os.path.join(HERE, "dgcf_baby.npz"), U=U, I=I, D=D, K=K, T=T, L=L, reg=reg, corDecay=cor,
                        users=users, pos=pos, neg=neg, loss=out["loss"], cor=out["cor"],
                        init_rows=np.concatenate([out["p_user"], out["p_item"]])[rows], rows=rows, result_rows=out["result"][rows], edge_sample=edges_s,
                        S_sample=out["S"][:, edges_s], grad_rows=grows,
                        g_rows=np.concatenate([out["g_user"], out["g_item"]])[grows])


if __name__ == "__main__":
    which = sys.argv[1:] or ["small", "baby"]
    if "small" in which:
        gen_small()
    if "baby" in which:
        gen_baby()
