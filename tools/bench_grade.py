#!/usr/bin/env python3
"""Grade at sports on the MI355X (measurement only): one eager training step (three losses, four Adam optimizers, as
epochs._train_epoch_grade runs it) with the fused three-view node (ops_extra.grade_views) against the SAME model with
`fused_edges = False`, i.e. the reference's per-edge lines in plain torch over gathered [E, 64] rows; the three-view node alone
both ways; the node at G = 3 against three G = 1 calls; the step's SpMM share (the same step with its propagates alone); peak
memory of each.

    python tools/bench_grade.py [--blocks 7] [--batch 1024] [--layers 5] [--dataset sports] [--trace]

Every time is the median of `--blocks` timed blocks of at least 50 ms each, the sides alternating block by block; the blocks
and their spread (largest - smallest) are kept; every block of the step starts from the same weight snapshot.  Prints one JSON
line.  --trace runs only a few passes of the node, for `rocprofv3 --kernel-trace --stats -- python tools/bench_grade.py --trace`
(kernel times come from the trace, in a run of its own)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chaorec_amd import dataload, ops_extra, sparse  # noqa: E402
from chaorec_amd.Model import Grade  # noqa: E402
from chaorec_amd.Model.Grade import plain_view_values  # noqa: E402
from tools.bench_mvgae import compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--dataset", default="sports")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    train, _, _, uid, U, I, v_feat, t_feat = dataload.data_load(a.dataset, data_root=os.path.join(ROOT, "Data"))
    torch.manual_seed(0)
    np.random.seed(0)
    m = Grade(U, I, train, uid, v_feat, t_feat, 64, 0.1, a.layers, 0.3, 0.2, 0.3, 0.2, dev).train()      # Model_YAML/Grade.yaml
    st = m.norm_adj_mat
    N, D, B, E = U + I, 64, a.batch, st.nnz
    out = {"dataset": a.dataset, "U": U, "I": I, "N": N, "E": E, "P": int(st.pair_owner.numel()), "B": B, "n_layers": a.layers,
           "blocks": a.blocks, "longest_row": int((st.rowptr[1:] - st.rowptr[:-1]).max())}
    pick = np.random.default_rng(0).choice(len(train), size=B, replace=False)
    users = torch.from_numpy(train[pick, 0].astype(np.int64))
    pos = torch.from_numpy(train[pick, 1].astype(np.int64))
    neg = torch.from_numpy(np.random.default_rng(1).integers(U, N, B))
    gens = (m.generator_1, m.generator_2, m.generator_3)
    with torch.no_grad():
        z = torch.stack([g.encoder(st)[0] for g in gens])
        mlps = [g.mlp() for g in gens]
        W1, b1, w2, b2 = (torch.stack([p[k].reshape(-1) for p in mlps]) for k in range(4))
        W1, b2 = W1.reshape(3, 64, 64), b2.reshape(-1)
        kept = ops_extra.grade_views(st, z, W1, b1, w2, b2, return_parts=True)[2]
    out["kept_fraction"] = [float(k) / E for k in kept.tolist()]

    def node_fused():
        ops_extra.grade_views(st, z, W1, b1, w2, b2)

    def node_single_calls():
        for g in range(3):
            ops_extra.grade_views(st, z[g], W1[g:g + 1], b1[g:g + 1], w2[g:g + 1], b2[g:g + 1])

    def node_plain():                      # Model/Grade.py:119-151 with the normalisation on the device
        with torch.no_grad():
            for g, gen in enumerate(gens):
                plain_view_values(gen.decoder, z[g], st)

    if a.trace:
        for _ in range(5):
            node_fused()
        torch.cuda.synchronize()
        print(json.dumps(out))
        return

    opt = torch.optim.Adam(m.parameters(), lr=0.001, weight_decay=0)
    opt_gens = [torch.optim.Adam(g.parameters(), lr=0.001, weight_decay=0) for g in gens]

    def step():                            # epochs._train_epoch_grade's body
        opt.zero_grad()
        m.loss_1(users, pos, neg).backward()
        opt.step()
        opt.zero_grad()
        m.bpr_reg_loss(users, pos, neg).backward()
        opt.step()
        for o in opt_gens:
            o.zero_grad()
        m.gen_loss(users, pos, neg).backward()
        for o in opt_gens:
            o.step()

    # the step's propagates alone: 12 forwards of n_layers SpMMs with a generated or the fixed graph, 3 of them (the views'
    # encoders) without a backward, and the item-graph SpMMs of all but the two noise forwards
    x0 = torch.randn(N, D, device=dev)
    xi = torch.randn(I, D, device=dev)
    view = sparse.DroppedAdj(st, st.val, st.val)

    def spmm_only():
        for with_grad, adj, n, item_graph in ((False, st, 3, True), (True, view, 3, True), (True, view, 2, False), (True, st, 4, True)):
            for _ in range(n):
                y = x0.clone().requires_grad_(with_grad)
                h = xi.clone().requires_grad_(with_grad)
                with torch.set_grad_enabled(with_grad):
                    total = sparse.mm(m.mm_adj, h).sum() if item_graph else None
                    for _ in range(a.layers):
                        y = sparse.mm(adj, y)
                    if with_grad:
                        (y.sum() if total is None else y.sum() + total).backward()

    snapshot = [p.detach().clone() for p in m.parameters()]

    def set_flags(name):
        m.fused_edges = name == "step_fused"
        with torch.no_grad():
            for p, w in zip(m.parameters(), snapshot):
                p.copy_(w)

    compare(out, [("step_fused", step), ("step_plain_torch", step)], a.blocks, before=set_flags)
    m.fused_edges = True
    compare(out, [("node_fused", node_fused), ("node_plain_torch", node_plain)], a.blocks)
    compare(out, [("node_g3", node_fused), ("node_3x_g1", node_single_calls)], a.blocks)
    compare(out, [("step_spmm_only", spmm_only)], a.blocks)
    for k in ("step", "node"):
        out[k + "_speedup"] = out[k + "_plain_torch_ms"] / out[k + "_fused_ms"]
        out[k + "_fused_wins"] = bool(out[k + "_plain_torch_ms"] - out[k + "_fused_ms"] > out[k + "_plain_torch_ms_spread"])
    # the default's rule: fused unless it is slower than the plain step by more than the blocks' spread
    out["step_fused_not_slower"] = bool(out["step_fused_ms"] - out["step_plain_torch_ms"]
                                        <= max(out["step_fused_ms_spread"], out["step_plain_torch_ms_spread"]))
    out["g3_over_3x_g1"] = out["node_3x_g1_ms"] / out["node_g3_ms"]
    out["spmm_share_of_fused_step"] = out["step_spmm_only_ms"] / out["step_fused_ms"]
    out["propagates_per_step"] = 21 * a.layers + 17                       # 3 + 2 x (5 + 1 + 3) forwards of n_layers, 17 on the item graph
    out["edge_table_MB"] = E * D * 4 / 1e6                                 # one gathered [E, 64] fp32 tensor
    out["node_gather_MB"] = 3 * 2 * (E // 2) * D * 4 / 1e6                 # two rows per undirected pair and generator (through L2)
    out["node_GFLOP"] = 3 * 2 * (E // 2) * D * D / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
