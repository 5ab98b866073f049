#!/usr/bin/env python3
"""MVGAE at sports on the MI355X (measurement only): the eager training step with the fused tail and conv epilogue
(ops_extra.mvgae_tail / mvgae_conv_tail) against the SAME model with `fused_tail = fused_conv = False`, i.e. the reference's
lines in plain torch; the tail node alone and the conv epilogue alone, forward + backward, both ways; peak memory of each.

    python tools/bench_mvgae.py [--blocks 7] [--batch 1024] [--dataset sports] [--trace]

Every time is the median of `--blocks` timed blocks of at least 50 ms each, the two sides alternating block by block; the
blocks and their spread (largest - smallest) are kept; every block of the step starts from the same weight snapshot.
Prints one JSON line.  --trace runs only a few passes of the two nodes, for `rocprofv3 --kernel-trace --stats -- python tools/bench_mvgae.py --trace` (kernel times come from the trace, in a
run of its own).  Features are the seeded synthetic ones every multimodal model gets for the committed datasets."""
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
from chaorec_amd import dataload, ops_extra  # noqa: E402
from chaorec_amd.Model import MVGAE  # noqa: E402
from chaorec_amd.optim import FusedAdam  # noqa: E402


def block_ms(fn, min_ms=50.0):
    """One timed block of at least min_ms -> milliseconds per call."""
    n, total = 0, 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while total < min_ms:
        for _ in range(4):
            fn()
        n += 4
        torch.cuda.synchronize()
        total = (time.perf_counter() - t0) * 1e3
    return total / n


def compare(out, sides, blocks, before=None):
    """sides: [(name, fn)], alternating block by block after a warm-up of each."""
    for _, fn in sides:
        for _ in range(3):
            fn()
    times = {name: [] for name, _ in sides}
    for name, fn in sides:                       # peak memory: one block each, from a trimmed allocator
        if before:
            before(name)
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        block_ms(fn)
        out[name + "_peak_MiB"] = torch.cuda.max_memory_allocated() / 2 ** 20
        out[name + "_extra_peak_MiB"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for _ in range(blocks):
        for name, fn in sides:
            if before:
                before(name)
            times[name].append(block_ms(fn))
    for name, t in times.items():
        out[name + "_ms"] = float(np.median(t))
        out[name + "_ms_spread"] = float(max(t) - min(t))
        out[name + "_ms_blocks"] = [round(x, 4) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dataset", default="sports")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    train, _, _, uid, U, I, v_feat, t_feat = dataload.data_load(a.dataset, data_root=os.path.join(ROOT, "Data"))
    torch.manual_seed(0)
    np.random.seed(0)
    m = MVGAE(U, I, train, uid, v_feat, t_feat, 64, 0.1, 2, dev)      # Model_YAML/MVGAE.yaml: reg_weight 0.1, n_layers 2
    N, D, B = U + I, 64, a.batch
    out = {"dataset": a.dataset, "U": U, "I": I, "N": N, "E": int(len(train)), "B": B, "blocks": a.blocks}
    pick = np.random.default_rng(0).choice(len(train), size=B, replace=False)
    users = torch.from_numpy(train[pick, 0].astype(np.int64)).to(dev)
    pos = torch.from_numpy(train[pick, 1].astype(np.int64)).to(dev)
    neg = torch.from_numpy(np.random.default_rng(1).integers(U, N, B)).to(dev)
    m.train()
    with torch.no_grad():
        ops_extra.mvgae_tick(m._state)
        tabs = [t.detach().clone().requires_grad_(True) for t in m._tables()]      # the six tables the tail is timed on
    s = torch.randn(N, D, device=dev, requires_grad=True)
    bias = (0.1 * torch.randn(D, device=dev)).requires_grad_(True)
    gy = torch.randn(N, D, device=dev)

    def tail_fused():
        ops_extra.mvgae_tail(*tabs, users, pos, neg, m.kl_weight, m._state, m.seed, True, row_ids=m._row_ids)[0].backward()

    def tail_torch():            # Model/MVGAE.py:317-342, :398-414
        m._plain_tail(tabs, users, pos, neg, None)[0].backward()

    def conv_fused():
        ops_extra.mvgae_conv_tail(s, bias, m._state, m.seed, 3, True).backward(gy)

    def conv_torch():            # Model/MVGAE.py:60-65 and the leaky_relu around it
        F.leaky_relu(F.dropout(F.normalize(s + bias, p=2, dim=-1), p=0.1, training=True)).backward(gy)

    if a.trace:
        for _ in range(5):
            tail_fused()
            conv_fused()
        torch.cuda.synchronize()
        print(json.dumps(out))
        return

    opt = FusedAdam([{"params": m.parameters(), "lr": 0.1}])

    def step():
        opt.zero_grad()
        loss = m.loss(users, pos, neg)
        loss.backward()
        opt.step()

    snapshot = [p.detach().clone() for p in m.parameters()]

    def set_flags(name):
        """Both sides start every block from the same weights: at lr 0.1 a few hundred steps on one batch would otherwise
        carry one drifting trajectory through the blocks (the optimizer's moments are left as they are)."""
        m.fused_tail = m.fused_conv = name == "step_fused"
        with torch.no_grad():
            for p, w in zip(m.parameters(), snapshot):
                p.copy_(w)

    compare(out, [("step_fused", step), ("step_plain_torch", step)], a.blocks, before=set_flags)
    m.fused_tail = m.fused_conv = True
    compare(out, [("tail_fused", tail_fused), ("tail_plain_torch", tail_torch)], a.blocks)
    compare(out, [("conv_fused", conv_fused), ("conv_plain_torch", conv_torch)], a.blocks)
    for k in ("step", "tail", "conv"):
        out[k + "_speedup"] = out[k + "_plain_torch_ms"] / out[k + "_fused_ms"]
        out[k + "_fused_wins"] = bool(out[k + "_plain_torch_ms"] - out[k + "_fused_ms"] > out[k + "_plain_torch_ms_spread"])
    # bytes the fused launches must move: a table pass is N * 64 * 4 bytes
    table = N * D * 4
    out["table_MB"] = table / 1e6
    out["tail_rows_MB"] = 7 * table / 1e6                                   # six reads, Pm written
    out["tail_batch_MB"] = (3 * B * 6 * D * 4 + 12 * B * D * 4) / 1e6       # the gathered rows, the z rows written
    out["tail_bwd_MB"] = (12 * table + (N + 1) * 8 + 3 * B * (8 + 4 * 3 * D * 4)) / 1e6      # six reads, six writes, the slot walk
    out["conv_fwd_MB"], out["conv_bwd_MB"] = 2 * table / 1e6, 3 * table / 1e6
    print(json.dumps(out))


if __name__ == "__main__":
    main()
