#!/usr/bin/env python3
"""AdaGCL at sports on the MI355X (measurement only): one eager training step (four losses, three Adam optimizers, as
epochs._train_epoch_adagcl runs it) with the fused edge work (ops_extra.adagcl_edge_gate / adagcl_edge_keep) against the
SAME model with `fused_edges = False`, i.e. the reference's per-edge lines in plain torch over gathered [E, 64] rows; the
gate node alone (training form, forward + backward) both ways; the keep decision alone both ways; peak memory of each.

    python tools/bench_adagcl.py [--blocks 7] [--batch 1024] [--dataset sports] [--trace]

Every time is the median of `--blocks` timed blocks of at least 50 ms each, the two sides alternating block by block; the
blocks and their spread (largest - smallest) are kept; every block of the step starts from the same weight snapshot.
Prints one JSON line.  --trace runs only a few passes of the two nodes, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_adagcl.py --trace` (kernel times come from the trace, in a run of
its own)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chaorec_amd import dataload, ops_extra  # noqa: E402
from chaorec_amd.Model import AdaGCL  # noqa: E402
from tools.bench_mvgae import compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dataset", default="sports")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    train, _, _, uid, U, I, _, _ = dataload.data_load(a.dataset, has_v=False, has_t=False, data_root=os.path.join(ROOT, "Data"))
    torch.manual_seed(0)
    np.random.seed(0)
    m = AdaGCL(U, I, train, uid, 64, 0.001, 2, 0.5, 0.1, dev).train()      # Model_YAML/AdaGCL.yaml
    st = m.norm_adj_mat
    N, D, B, E = U + I, 64, a.batch, st.nnz
    out = {"dataset": a.dataset, "U": U, "I": I, "N": N, "E": E, "B": B, "blocks": a.blocks,
           "longest_row": int((st.rowptr[1:] - st.rowptr[:-1]).max())}
    pick = np.random.default_rng(0).choice(len(train), size=B, replace=False)
    users = torch.from_numpy(train[pick, 0].astype(np.int64))
    pos = torch.from_numpy(train[pick, 1].astype(np.int64))
    neg = torch.from_numpy(np.random.default_rng(1).integers(U, N, B))
    g2 = m.generator_2
    x = g2.features
    g_val = torch.randn(E, device=dev)
    ops_extra.adagcl_tick(m._state)
    with torch.no_grad():
        z = m.generator_1.encoder(st)[0]

    def gate(fused):
        def run():
            g2.fused = fused
            g2.zero_grad()
            val, l0 = g2.gate(x, 0, m.ssl_temp, True)
            ((g_val * val).sum() + l0).backward()
        return run

    def keep(fused):
        lin1, lin2 = m.generator_1.decoder.decoder[1], m.generator_1.decoder.decoder[3]

        def run():
            with torch.no_grad():
                if fused:
                    ops_extra.adagcl_edge_keep(st, z, lin1.weight, lin1.bias, lin2.weight, lin2.bias, st.val)
                else:                      # Model/AdaGCL.py:488-498
                    p = m.generator_1.decoder.sigmoid(m.generator_1.decoder.decoder(z[st.entry_row.long()] * z[st.col.long()]))[:, 0]
                    mask = ((p + 0.5).floor()).type(torch.bool)
                    kept = st.val[mask]
                    kept / (kept.shape[0] / st.val.shape[0])
        return run

    if a.trace:
        for _ in range(5):
            gate(True)()
            keep(True)()
        torch.cuda.synchronize()
        print(json.dumps(out))
        return

    opt = torch.optim.Adam(m.parameters(), lr=0.001, weight_decay=0)
    opt_gen_1 = torch.optim.Adam(m.generator_1.parameters(), lr=0.001, weight_decay=0)
    opt_gen_2 = torch.optim.Adam(filter(lambda p: p.requires_grad, m.generator_2.parameters()), lr=0.001, weight_decay=0, eps=0.001)

    def step():                            # epochs._train_epoch_adagcl's body
        opt.zero_grad()
        opt_gen_1.zero_grad()
        opt_gen_2.zero_grad()
        loss_1, out1, out2 = m.loss_1(users, pos, neg)
        loss_1.backward()
        opt.step()
        opt.zero_grad()
        m.loss_2(users, pos, neg, out1, out2).backward()
        opt.step()
        opt.zero_grad()
        m.bpr_reg_loss(users, pos, neg).backward()
        m.gen_loss(users, pos, neg).backward()
        opt.step()
        opt_gen_1.step()
        opt_gen_2.step()

    snapshot = [p.detach().clone() for p in m.parameters()]

    def set_flags(name):
        m.fused_edges = name == "step_fused"
        with torch.no_grad():
            for p, w in zip(m.parameters(), snapshot):
                p.copy_(w)

    compare(out, [("step_fused", step), ("step_plain_torch", step)], a.blocks, before=set_flags)
    m.fused_edges = True
    compare(out, [("gate_fused", gate(True)), ("gate_plain_torch", gate(False))], a.blocks)
    compare(out, [("keep_fused", keep(True)), ("keep_plain_torch", keep(False))], a.blocks)
    for k in ("step", "gate", "keep"):
        out[k + "_speedup"] = out[k + "_plain_torch_ms"] / out[k + "_fused_ms"]
        out[k + "_fused_wins"] = bool(out[k + "_plain_torch_ms"] - out[k + "_fused_ms"] > out[k + "_plain_torch_ms_spread"])
    out["edge_table_MB"] = E * D * 4 / 1e6                                 # one gathered [E, 64] fp32 tensor
    out["gate_fwd_MB"] = (E * (4 + 4 + 4 + 4) + 4 * N * 4) / 1e6          # col, u, m, val; four N-sized vectors
    out["keep_gather_MB"] = 2 * E * D * 4 / 1e6                            # the two rows per entry (through L2: the table is N * 256 B)
    out["keep_GFLOP"] = 2 * E * D * D / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
