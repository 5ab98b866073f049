#!/usr/bin/env python3
"""DRAGON at sports on the MI355X (measurement only): the device build of the user-user co-occurrence graph, one
pre_epoch_processing(), and the eager training step with the fused aggregation against the SAME step with the aggregation
as the reference writes it (features[user_graph] gathered to [U, k, 2 D], matmul with the weights) in plain torch.

    python tools/bench_dragon.py [--steps 50] [--uu_topk 40] [--dataset sports]

Prints one JSON line.  Features are the seeded synthetic ones every multimodal model gets for the committed datasets."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chaorec_amd import dataload, ops_extra  # noqa: E402
from chaorec_amd.Model import DRAGON  # noqa: E402
from chaorec_amd.optim import FusedAdam  # noqa: E402


def timed(fn, steps, warmup=3):
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--uu_topk", type=int, default=40)
    ap.add_argument("--dataset", default="sports")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    train, _, _, uid, U, I, v_feat, t_feat = dataload.data_load(a.dataset, data_root=os.path.join(ROOT, "Data"))
    torch.manual_seed(0)
    np.random.seed(0)
    DRAGON.user_graph_path = None
    m = DRAGON(U, I, train, uid, v_feat, t_feat, 64, 64, 0.01, 2, 10, a.uu_topk, 0.6, "add", dev).to(dev)
    out = {"dataset": a.dataset, "U": U, "I": I, "E": int(len(train)), "B": a.batch, "k": a.uu_topk, "steps": a.steps}

    rowptr, col = m.hist[0].to(torch.int64).contiguous(), m.hist[1].to(torch.int32).contiguous()
    s = m.graph_structure
    out["build_ms"] = timed(lambda: ops_extra.usergraph_build(rowptr, col, I, out=(s.nbr_idx, s.nbr_cnt, s.nbr_len)), 5, warmup=1)
    out["neighbours_mean"] = float(s.nbr_len.float().mean())
    out["users_cut_at_200"] = int((s.nbr_len == s.n).sum())
    out["pre_epoch_ms"] = timed(m.pre_epoch_processing, 10, warmup=2)

    opt = FusedAdam([{"params": m.parameters(), "lr": 0.001}])
    pick = np.random.default_rng(0).choice(len(train), size=a.batch, replace=False)
    users = torch.from_numpy(train[pick, 0].astype(np.int64)).to(dev)
    pos = torch.from_numpy(train[pick, 1].astype(np.int64)).to(dev)
    neg = torch.from_numpy(np.random.default_rng(1).integers(U, U + I, a.batch)).to(dev)

    def step():
        opt.zero_grad()
        loss = m.loss(users, pos, neg)
        loss.backward()
        opt.step()

    for name, fused in (("step_fused_ms", True), ("step_torch_gather_ms", False)):
        m.fused_aggregation = fused
        torch.cuda.reset_peak_memory_stats()
        out[name] = timed(step, a.steps)
        out[name.replace("_ms", "_peak_MiB")] = torch.cuda.max_memory_allocated() / 2 ** 20

    # the aggregation alone, forward + backward, on the tables of the last forward
    v, t = m.v_rep[:U].detach().clone().requires_grad_(True), m.t_rep[:U].detach().clone().requires_grad_(True)
    wu = m.weight_u.detach().clone().requires_grad_(True)
    g = torch.randn(U, 128, device=dev)

    def agg_fused():
        ops_extra.usergraph_aggregate(v, t, wu, s).backward(g)

    def agg_torch():
        x = torch.cat((wu[:, 0] * v, wu[:, 1] * t), dim=1)
        (x + torch.matmul(s.epoch_w.unsqueeze(1), x[s.epoch_idx.long()]).squeeze(1)).backward(g)

    out["aggregate_fused_ms"] = timed(agg_fused, a.steps)
    out["aggregate_torch_ms"] = timed(agg_torch, a.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
