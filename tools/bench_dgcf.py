#!/usr/bin/env python3
"""DGCF on sports at the CLI defaults (D 64, K 4, T 3, L 3, B 1024): epoch time and ms per batch, captured and eager, and the
ms per batch of an fp32 torch restatement of the reference's per-factor step (eager, the same GPU) for comparison.

    python tools/bench_dgcf.py            -> one JSON line
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from chaorec_amd import dataload, graph, train_and_evaluate as te  # noqa: E402
from chaorec_amd.Model import DGCF  # noqa: E402
from chaorec_amd.optim import FusedAdam  # noqa: E402
from test_dgcf_host import dgcf_forward, dgcf_loss  # noqa: E402

D, K, T, L, B = 64, 4, 3, 3, 1024
dev = torch.device("cuda:0")
g = np.load(os.path.join(ROOT, "tests", "golden", "sports_interactions.npz"))
U, I, train = int(g["U"]), int(g["I"]), g["train"]
uid = graph.user_item_dict_from_edges(train)
out = {"dataset": "sports", "D": D, "K": K, "T": T, "L": L, "B": B, "edges": int(train.shape[0])}


def epochs(captured, n=4):
    torch.manual_seed(0)
    m = DGCF(U, I, train, uid, D, 1e-3, 1e-3, K, T, L, "add", dev).to(dev)
    loader = dataload.DeviceBatchSampler(U, I, uid, train, B, dev, "DGCF", 42)
    opt = FusedAdam([{"params": m.parameters(), "lr": 1e-3}])
    graphed = te._capture_step(m, loader, opt, "DGCF") if captured else None
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        te.train(m, loader, opt, "DGCF", graphed)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ep = float(np.median(ts[1:]))
    return {"epoch_s": ep, "ms_per_batch": ep / len(loader) * 1e3, "batches": len(loader), "captured": graphed is not None}


out["captured"] = epochs(True)
out["eager"] = epochs(False)

# the reference's step restated in fp32 torch (per-factor propagates, dense distance matrices), eager
torch.manual_seed(0)
tu = torch.nn.Parameter(torch.nn.init.xavier_uniform_(torch.empty(U, D, device=dev)))
ti = torch.nn.Parameter(torch.nn.init.xavier_uniform_(torch.empty(I, D, device=dev)))
opt = torch.optim.Adam([tu, ti], lr=1e-3)
S = torch.ones((train.shape[0], K), device=dev)
rng = np.random.default_rng(0)
ts = []
for s in range(8):
    b = rng.choice(len(train), B, replace=False)
    users = torch.as_tensor(train[b, 0], device=dev).long()
    pos = torch.as_tensor(train[b, 1], device=dev).long()
    neg = torch.as_tensor(rng.integers(U, U + I, B), device=dev).long()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    opt.zero_grad()
    result, S = dgcf_forward(torch.cat([tu, ti]), train, K, T, L, S)
    loss = dgcf_loss(result, users, pos, neg, K, 1e-3, 1e-3)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
out["torch_fp32_restatement_ms_per_batch"] = float(np.median(ts[2:])) * 1e3
print(json.dumps(out))
