#!/usr/bin/env python3
"""MacridVAE's training step at sports (B 2 048, dim_E 64, 10 concepts) on the MI355X: the captured and the eager step of
this repository against the SAME model in plain float32 torch ops on the GPU (per concept the [B, I] weighted input,
logits and probabilities materialised, eager).

    python tools/bench_macridvae.py [--steps 100] [--profile]      # --profile: fewer steps, for a rocprofv3 --kernel-trace run

Prints one JSON line.  Both sides draw on the device; the torch side's dense batch rows are built once, outside the timed
loop."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chaorec_amd import graph  # noqa: E402
from chaorec_amd.Model import MacridVAE  # noqa: E402
from chaorec_amd.optim import FusedAdam, GraphedTrainStep  # noqa: E402


def timed(fn, steps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    d = np.load(os.path.join(ROOT, "tests", "golden", "sports_interactions.npz"))
    U, I, edges = int(d["U"]), int(d["I"]), d["train"]
    torch.manual_seed(0)
    m = MacridVAE(U, I, edges, graph.user_item_dict_from_edges(edges), 64, 0.0, dev)
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.01}])
    users = torch.from_numpy(np.random.default_rng(0).integers(0, U, a.batch)).to(dev)
    m.train()
    steps = 10 if a.profile else a.steps
    K, D, tau = m.kfac, m.dim_E, m.tau
    out = {"U": U, "I": I, "B": a.batch, "steps": steps, "logit_pass_gflop": 2 * a.batch * I * K * D / 1e9}

    def eager():
        opt.zero_grad()
        loss = m.loss(users, users, users)
        loss.backward()
        opt.step()

    out["eager_ms"] = timed(eager, steps)
    g = GraphedTrainStep(m, opt, example_batch=(users, users, users))
    out["captured_ms"] = timed(lambda: g(users, users, users), steps)
    out["ranklist_ms"] = timed(lambda: m.gene_ranklist(to_cpu=False), 2, warmup=1)
    m.train()

    if not a.profile:
        params = [torch.nn.Parameter(p.detach().clone().contiguous()) for p in m.parameters()]
        topt = torch.optim.Adam(params, lr=0.01, fused=True)
        s = m.structure
        rows = torch.repeat_interleave(torch.arange(a.batch, device=dev), s.rowptr[users + 1] - s.rowptr[users])
        cols = torch.cat([s.col[s.rowptr[u]:s.rowptr[u + 1]] for u in users.tolist()]).long()
        x = torch.zeros((a.batch, I), device=dev)
        x[rows, cols] = 1.0
        torch.cuda.reset_peak_memory_stats()

        def torch_step():
            W1, b1, W2, b2, E, Ke = params
            topt.zero_grad()
            items, cores = F.normalize(E, dim=1), F.normalize(Ke, dim=1)
            xs = F.dropout(F.normalize(x, dim=1), 0.5)
            cates = F.gumbel_softmax(items @ cores.t() / tau, tau=1, hard=False, dim=-1)
            p, lvs = None, []
            for k in range(K):
                h = torch.tanh((xs * cates[:, k][None, :]) @ W1.t() + b1) @ W2.t() + b2
                mu, lv = F.normalize(h[:, :D], dim=1), h[:, D:]
                z = F.normalize(mu + torch.randn_like(mu) * 0.01 * torch.exp(0.5 * lv), dim=1)
                pk = torch.exp(z @ items.t() / tau) * cates[:, k][None, :]
                p = pk if p is None else p + pk
                lvs.append(lv)
            lv = torch.stack(lvs, 1)
            kl = 0.5 * (torch.expm1(lv) - lv).sum() / a.batch
            ce = (x.sum(1) * torch.log(p.sum(1)) - (torch.log(p) * x).sum(1)).mean()
            (ce + 0.2 * kl).backward()
            topt.step()

        out["torch_eager_ms"] = timed(torch_step, max(5, steps // 5), warmup=2)
        out["torch_peak_MiB"] = torch.cuda.max_memory_allocated() / 2 ** 20
    print(json.dumps(out))


if __name__ == "__main__":
    main()
