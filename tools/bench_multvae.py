#!/usr/bin/env python3
"""MultVAE's training step at sports (B 2 048, latent 64) on the MI355X: the captured step of this repository against
the SAME model in plain float32 torch ops on the GPU (the [B, I] rows, logits and log_softmax materialised, eager).

    python tools/bench_multvae.py [--steps 200] [--profile]      # --profile: fewer steps, for a rocprofv3 --kernel-trace run

Prints one JSON line.  Both sides draw on the device; the torch side's dense batch rows are built once, outside the
timed loop (the reference builds them on the host every step)."""
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
from chaorec_amd.Model import MultVAE  # noqa: E402
from chaorec_amd.optim import FusedAdam, GraphedTrainStep  # noqa: E402


def timed(fn, steps, warmup=10):
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    d = np.load(os.path.join(ROOT, "tests", "golden", "sports_interactions.npz"))
    U, I, edges = int(d["U"]), int(d["I"]), d["train"]
    torch.manual_seed(0)
    m = MultVAE(U, I, edges, graph.user_item_dict_from_edges(edges), 64, 0.01, dev)
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.01}])
    users = torch.from_numpy(np.random.default_rng(0).integers(0, U, a.batch)).to(dev)
    m.train()
    steps = 20 if a.profile else a.steps
    out = {"U": U, "I": I, "B": a.batch, "steps": steps}

    def eager():
        opt.zero_grad()
        loss = m.loss(users, users, users)
        loss.backward()
        opt.step()

    out["eager_ms"] = timed(eager, steps)
    g = GraphedTrainStep(m, opt, example_batch=(users, users, users))
    out["captured_ms"] = timed(lambda: g(users, users, users), steps)
    out["ranklist_ms"] = timed(lambda: m.gene_ranklist(to_cpu=False), 5, warmup=2)

    if not a.profile:
        # the same model in plain torch ops, float32, [B, I] materialised
        params = [torch.nn.Parameter(p.detach().clone().contiguous()) for p in (m.layers_q[0].weight, m.layers_q[0].bias,
                                                                                m.layers_p[0].weight, m.layers_p[0].bias)]
        topt = torch.optim.Adam(params, lr=0.01, fused=True)
        s = m.structure
        rows = torch.repeat_interleave(torch.arange(a.batch, device=dev), s.rowptr[users + 1] - s.rowptr[users])
        cols = torch.cat([s.col[s.rowptr[u]:s.rowptr[u + 1]] for u in users.tolist()]).long()
        x = torch.zeros((a.batch, I), device=dev)
        x[rows, cols] = 1.0
        torch.cuda.reset_peak_memory_stats()

        def torch_step():
            Wq, bq, Wp, bp = params
            topt.zero_grad()
            h = F.dropout(F.normalize(x, dim=1), 0.5) @ Wq.t() + bq
            mu, logvar = h[:, :64], h[:, 64:]
            kl = torch.sum(0.5 * (-logvar + logvar.exp() + mu.pow(2) - 1), dim=1).mean()
            z = mu + torch.randn_like(mu) * torch.exp(0.5 * logvar)
            neg_ll = -(F.log_softmax(z @ Wp.t() + bp, dim=-1) * x).sum(-1).mean()
            loss = neg_ll + 0.2 * kl + 1e-4 * sum((p ** 2).sum() for p in params)
            loss.backward()
            topt.step()

        out["torch_eager_ms"] = timed(torch_step, steps)
        out["torch_peak_MiB"] = torch.cuda.max_memory_allocated() / 2 ** 20
    print(json.dumps(out))


if __name__ == "__main__":
    main()
