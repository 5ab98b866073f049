#!/usr/bin/env python3
"""DualGNN at sports on the MI355X (measurement only): the eager training step with the fused node (ops_extra.dualgnn_fuse)
against the SAME model with `fused_aggregation = False`, i.e. the reference's lines in plain torch (cat(v_rep[:U], t_rep[:U])
[U, D, 2] x weight_u, features[user_graph] gathered to [U, k, D], matmul with the weights, the final cat); the node alone,
forward + backward, both ways; peak memory of each.

    python tools/bench_dualgnn.py [--steps 50] [--uu_topk 40] [--dataset sports]

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
from chaorec_amd.Model import DualGNN  # noqa: E402
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
    DualGNN.user_graph_path = None
    m = DualGNN(U, I, train, uid, v_feat, t_feat, 64, 64, 0.01, a.uu_topk, "add", dev).to(dev)
    out = {"dataset": a.dataset, "U": U, "I": I, "E": int(len(train)), "B": a.batch, "k": a.uu_topk, "steps": a.steps}
    s = m.graph_structure
    out["pre_epoch_ms"] = timed(m.pre_epoch_processing, 10, warmup=2)

    opt = FusedAdam([{"params": m.parameters(), "lr": 0.0001}])
    pick = np.random.default_rng(0).choice(len(train), size=a.batch, replace=False)
    users = torch.from_numpy(train[pick, 0].astype(np.int64)).to(dev)
    pos = torch.from_numpy(train[pick, 1].astype(np.int64)).to(dev)
    neg = torch.from_numpy(np.random.default_rng(1).integers(U, U + I, a.batch)).to(dev)

    def step():
        opt.zero_grad()
        loss = m.loss(users, pos, neg)
        loss.backward()
        opt.step()

    # alternate the two versions: two timed blocks each, the second one reported, both kept
    for rep in range(2):
        for name, fused in (("step_fused_ms", True), ("step_plain_torch_ms", False)):
            m.fused_aggregation = fused
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            ms = timed(step, a.steps)
            out.setdefault(name + "_blocks", []).append(round(ms, 4))
            out[name] = ms
            out[name.replace("_ms", "_peak_MiB")] = torch.cuda.max_memory_allocated() / 2 ** 20
    out["step_speedup"] = out["step_plain_torch_ms"] / out["step_fused_ms"]

    # the node alone, forward + backward, on the tables of the last forward
    m.fused_aggregation = True
    v, t = m.v_rep.detach().clone().requires_grad_(True), m.t_rep.detach().clone().requires_grad_(True)
    wu = m.weight_u.detach().clone().requires_grad_(True)
    g = torch.randn(U + I, 64, device=dev)
    idx = s.epoch_idx.long()

    def node_fused():
        ops_extra.dualgnn_fuse(v, t, wu, s, U).backward(g)

    def node_torch():       # Model/DualGNN.py:189-239
        rep = v + t
        x = torch.matmul(torch.cat((v[:U].unsqueeze(2), t[:U].unsqueeze(2)), dim=2), wu).squeeze(2)
        h = torch.matmul(s.epoch_w.unsqueeze(1), x[idx]).squeeze(1)
        torch.cat((x + h, rep[U:]), dim=0).backward(g)

    for name, fn in (("node_fused", node_fused), ("node_plain_torch", node_torch)):
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out[name + "_ms"] = timed(fn, a.steps)
        out[name + "_extra_peak_MiB"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    out["node_speedup"] = out["node_plain_torch_ms"] / out["node_fused_ms"]
    # bytes the fused launches must move (gathered rows come from L2): forward reads (k + 1) rows of v and t per user and
    # both tables' item rows, writes the result; backward reads g along the reverse lists, v, t, writes dv, dt
    k, D = a.uu_topk, 64
    out["node_fwd_MB"] = (U * (k + 1) * 2 * D * 4 + I * 2 * D * 4 + (U + I) * D * 4 + U * k * 8) / 1e6
    out["node_bwd_MB"] = (U * (k + 1) * D * 4 + I * D * 4 + U * 2 * D * 4 + (U + I) * 2 * D * 4 + U * k * 8) / 1e6
    print(json.dumps(out))


if __name__ == "__main__":
    main()
