#!/usr/bin/env python3
"""DualVAE's training step at sports (B 2 048, k 25, 5 aspects, hidden 20) on the MI355X: the captured and the eager step of
this repository and gene_ranklist() against the SAME model in plain float32 torch ops on the GPU (per aspect the [B, U] /
[B, I] weighted input, decoder output and weighted copy materialised, eager).

    python tools/bench_dualvae.py [--steps 100] [--profile]      # --profile: fewer steps, for a rocprofv3 --kernel-trace run

Prints one JSON line.  Both sides draw on the device; the torch side's dense batch rows are built once, outside the timed
loop."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chaorec_amd import graph  # noqa: E402
from chaorec_amd.Model import DualVAE  # noqa: E402
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


def contrast(x, x_):
    x, x_ = torch.nn.functional.normalize(x, dim=-1), torch.nn.functional.normalize(x_, dim=-1)
    pos = torch.exp((x_ * x).sum(-1) / 0.2)
    acl = torch.exp(torch.bmm(x_, x.transpose(1, 2)) / 0.2).sum(-1)
    ncl = torch.exp(torch.bmm(x_.transpose(0, 1), x.transpose(0, 1).transpose(1, 2)).transpose(0, 1) / 0.2).sum(-1)
    return -torch.log(pos / (acl + ncl)).sum(-1).mean()


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
    m = DualVAE(U, I, edges, graph.user_item_dict_from_edges(edges), 64, 0.5, 0.01, dev)
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.001}])
    pick = np.random.default_rng(0).choice(len(edges), size=a.batch, replace=False)
    users, pos = torch.from_numpy(edges[pick, 0].astype(np.int64)).to(dev), torch.from_numpy(edges[pick, 1].astype(np.int64)).to(dev)
    m.train()
    steps = 10 if a.profile else a.steps
    B = a.batch
    out = {"U": U, "I": I, "B": B, "steps": steps,
           "fwd_pass_gflop": {"item_side": 2 * B * U * 5 * (26 + 20) / 1e9, "user_side": 2 * B * I * 5 * (26 + 20) / 1e9},
           "bwd_pass_gflop": {"item_side": 2 * B * U * 5 * (26 + 20 + 26) / 1e9, "user_side": 2 * B * I * 5 * (26 + 20 + 26) / 1e9}}

    def eager():
        opt.zero_grad()
        loss = m.loss(users, pos, pos)
        loss.backward()
        opt.step()

    out["eager_ms"] = timed(eager, steps)
    g = GraphedTrainStep(m, opt, example_batch=(users, pos, pos))
    out["captured_ms"] = timed(lambda: g(users, pos, pos), steps)
    out["ranklist_ms"] = timed(lambda: m.gene_ranklist(to_cpu=False), 2, warmup=1)
    m.train()

    if not a.profile:
        P = {n: torch.nn.Parameter(p.detach().clone().contiguous()) for n, p in m.named_parameters()}
        topt = torch.optim.Adam(list(P.values()), lr=0.001, fused=True)
        X = torch.zeros((U, I), device=dev)
        e = torch.from_numpy(edges.astype(np.int64)).to(dev)
        X[e[:, 0], e[:, 1] - U] = 1.0
        xi, xu = X.t()[pos - U].contiguous(), X[users].contiguous()
        del X
        theta, beta = m.theta.clone(), m.beta.clone()
        torch.cuda.reset_peak_memory_stats()

        def side(s, t, x, table, pref):
            w = torch.softmax((table * pref).sum(-1), dim=1)
            zs, neis, kl, probs = [], [], 0.0, 0.0
            for k in range(5):
                h = torch.tanh((x * w[:, k]) @ P[f"{s}_encoder.fc0.weight"].t() + P[f"{s}_encoder.fc0.bias"])
                mu = h @ P[f"{s}_mu.weight"].t() + P[f"{s}_mu.bias"]
                std = torch.sigmoid(h @ P[f"{s}_std.weight"].t() + P[f"{s}_std.bias"])
                kl = kl + (-0.5 * (1 + 2.0 * torch.log(std) - mu ** 2 - std ** 2)).sum(-1).mean()
                z = mu + torch.randn_like(mu) * std
                zh = torch.tanh(z @ P[f"{s}_decoder.fc_out0.weight"].t() + P[f"{s}_decoder.fc_out0.bias"])
                th = torch.tanh(table[:, k] @ P[f"{t}_decoder.fc_out0.weight"].t() + P[f"{t}_decoder.fc_out0.bias"])
                pa = torch.sigmoid(z @ table[:, k].t() + torch.tanh(zh @ th.t())) * w[:, k]
                probs = probs + pa
                zs.append(z)
                neis.append(pa @ table[:, k])
            z = torch.stack(zs, 1)
            ll = (x * torch.log(probs + 1e-10) - probs).sum(-1).mean()
            return 0.5 * kl / 5 - ll + 0.01 * contrast(z, torch.stack(neis, 1)), z.detach()

        def torch_step():
            topt.zero_grad()
            li, zi = side("item", "user", xi, theta.clone(), P["user_preferences"])
            beta[pos - U] = zi
            lu, zu = side("user", "item", xu, beta, P["item_topics"])
            theta[users] = zu
            (li + lu).backward()
            topt.step()

        out["torch_eager_ms"] = timed(torch_step, max(5, steps // 5), warmup=2)
        out["torch_peak_MiB"] = torch.cuda.max_memory_allocated() / 2 ** 20
    print(json.dumps(out))


if __name__ == "__main__":
    main()
