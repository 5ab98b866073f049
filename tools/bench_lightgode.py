#!/usr/bin/env python3
"""LightGODE at sports on the MI355X (measurement only): the loss node of csrc/lightgode.hip against the reference's lines in
plain torch, and the Euler step of one evaluation.

  step    one eager training step (zero_grad, loss, backward, Adam) on a fixed batch of training pairs: fused against fused = False
  node    the loss and the backward into the two tables alone: ops.lightgode_loss against ops.lightgode_loss_plain
  euler   the one SpMM launch behind an evaluation's tables (ops.lightgode_euler), and the literal x + t (A x + x) on the same
          kernel's plain SpMM beside it

    python tools/bench_lightgode.py [--blocks 7] [--batch 1024] [--dataset sports] [--out profiles/lightgode_sports_bench.json]

Every time is the median of `--blocks` timed blocks of at least 50 ms each, the sides alternating block by block, with the
spread (largest - smallest); peak memory of each side from a trimmed allocator, above a baseline that holds the tables, the
optimizer state and the batch but NO gradients (they are dropped before the baseline is read, so a side's figure counts its
table gradients, 10.8 MiB at sports, and every transient: workspace, row gradients, pdist vectors).  Prints one JSON line and writes it to --out.
`fused_default` is true only where the fused step's median is below the plain step's by more than both spreads together: the
class default follows it."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from chaorec_amd import dataload, ops  # noqa: E402
from chaorec_amd.Model.LightGODE import LightGODE  # noqa: E402
from tools.bench_mvgae import compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dataset", default="sports")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightgode_sports_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    train, _, _, uid, U, I, _, _ = dataload.data_load(a.dataset, has_v=False, has_t=False, data_root=os.path.join(ROOT, "Data"))
    torch.manual_seed(0)
    np.random.seed(0)
    m = LightGODE(U, I, train, uid, 64, 0.5, 1.8, dev).to(dev)       # Model_YAML/LightGODE.yaml of the reference: gamma 0.5, t 1.8
    B = a.batch
    out = {"dataset": a.dataset, "U": U, "I": I, "D": 64, "E": int(len(train)), "B": B, "gamma": 0.5, "t": 1.8, "blocks": a.blocks}
    pick = np.random.default_rng(0).choice(len(train), size=B, replace=False)
    users = torch.from_numpy(train[pick, 0].astype(np.int64)).to(dev)
    pos = torch.from_numpy(train[pick, 1].astype(np.int64)).to(dev)
    out["repeated_users"], out["repeated_items"] = B - int(users.unique().numel()), B - int(pos.unique().numel())
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    snapshot = [p.detach().clone() for p in m.parameters()]

    def step():
        opt.zero_grad()
        m.loss(users, pos, pos).backward()
        opt.step()

    def set_flag(name):
        m.fused = name.endswith("_fused")
        opt.zero_grad(set_to_none=True)
        with torch.no_grad():
            for p, w in zip(m.parameters(), snapshot):
                p.copy_(w)

    compare(out, [("step_fused", step), ("step_plain_torch", step)], a.blocks, before=set_flag)
    set_flag("_fused")

    # the node alone
    W_u, W_i, items = m.user_embedding.weight, m.item_embedding.weight, pos - U

    def node(fn):
        def run():
            W_u.grad = W_i.grad = None
            fn(W_u, W_i, users, items, m.gamma)[0].backward()
        return run

    def drop_grads(_name):
        W_u.grad = W_i.grad = None

    compare(out, [("node_fused", node(ops.lightgode_loss)), ("node_plain_torch", node(ops.lightgode_loss_plain))], a.blocks,
            before=drop_grads)
    out["node_fused_workspace_MiB"] = ops.lightgode_workspace(B) * 4 / 2 ** 20
    out["table_gradients_MiB"] = (U + I) * 64 * 4 / 2 ** 20
    with torch.no_grad():
        lf, lp = ops.lightgode_loss(W_u, W_i, users, items, m.gamma)[1], ops.lightgode_loss_plain(W_u, W_i, users, items, m.gamma)[1]
    out["parts_fused"], out["parts_plain_torch"] = lf.tolist(), lp.tolist()

    # one evaluation's Euler step
    x = m.get_ego_embeddings().detach()
    t = float(m.t[1] - m.t[0])

    def euler_fused():
        ops.lightgode_euler(m.norm_adj, x, t)

    def euler_literal():
        x + t * (ops.spmm_raw(m.norm_adj, x) + x)

    with torch.no_grad():
        compare(out, [("euler_one_launch", euler_fused), ("euler_literal", euler_literal)], a.blocks)

    for k, fast, slow in (("step", "step_fused", "step_plain_torch"), ("node", "node_fused", "node_plain_torch"),
                          ("euler", "euler_one_launch", "euler_literal")):
        out[k + "_speedup"] = out[slow + "_ms"] / out[fast + "_ms"]
        out[k + "_wins"] = bool(out[slow + "_ms"] - out[fast + "_ms"] > out[slow + "_ms_spread"] + out[fast + "_ms_spread"])
    out["fused_default"] = out["step_wins"]
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
