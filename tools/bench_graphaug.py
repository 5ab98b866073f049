#!/usr/bin/env python3
"""GraphAug at sports on the MI355X (measurement only): one eager training step (loss, backward, Adam: the plain loop of
train_and_evaluate) with both kernels (`fused_edges`, `fused_contrast`) against the SAME model with both flags off, i.e. the
reference's per-edge and [B, M] lines in plain torch; the edge sampler alone -- its two N-sized GEMMs included -- against the
per-edge torch lines; the log-sum-exp node forward + backward (users' table and items' table) against the torch contrastLoss
denominator; the sampler with and without the kernel's own transposed store; peak memory of each.

    python tools/bench_graphaug.py [--blocks 7] [--batch 1024] [--dataset sports] [--trace]

Every time is the median of `--blocks` timed blocks of at least 50 ms each, the sides alternating block by block; the blocks
and their spread (largest - smallest) are kept; every block of the step starts from the same weight snapshot.  Prints one
JSON line.  --trace runs only a few passes of the kernels, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_graphaug.py --trace` (kernel times come from the trace, in a run of
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
from chaorec_amd.Model import GraphAug  # noqa: E402
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
    m = GraphAug(U, I, train, uid, 64, 0.001, 3, 0.2, 0.01, dev).train()      # Model_YAML/GraphAug.yaml
    st = m.norm_adj_mat
    N, D, B, E = U + I, 64, a.batch, st.nnz
    out = {"dataset": a.dataset, "U": U, "I": I, "N": N, "E": E, "B": B, "blocks": a.blocks,
           "longest_row": int((st.rowptr[1:] - st.rowptr[:-1]).max())}
    pick = np.random.default_rng(0).choice(len(train), size=B, replace=False)
    users = torch.from_numpy(train[pick, 0].astype(np.int64))
    pos = torch.from_numpy(train[pick, 1].astype(np.int64))
    neg = torch.from_numpy(np.random.default_rng(1).integers(U, N, B))
    ops_extra.adagcl_tick(m._state)
    z = torch.randn(N, D, device=dev)
    vl = m.view_learner
    draws = dict(state=m._state, seed=m.seed, salt=0)

    def sampler(fused):
        def run():
            vl.sample(z, st, fused, **(draws if fused else {}))
        return run

    def sampler_gather():                      # the kernel without its transposed store, then torch's gather
        lin1, lin2 = vl.mlp_edge_model[0], vl.mlp_edge_model[2]
        with torch.no_grad():
            P, Q = z @ lin1.weight[:, :D].t(), z @ lin1.weight[:, D:].t()
            val = ops_extra.graphaug_edge_sample(st, P, Q, lin1.bias, lin2.weight, lin2.bias, want_val_t=False, **draws)[0]
            val[st.transpose_entry.long()]

    tables = {}
    for name, M, ids in (("users", U, users), ("items", I, pos - U)):
        e1 = torch.nn.functional.normalize(torch.randn(M, D, device=dev)).requires_grad_(True)
        e2 = torch.nn.functional.normalize(torch.randn(M, D, device=dev)).requires_grad_(True)
        tables[name] = (e1, e2, ids.to(dev))

    def lse(fused):
        def run():
            for e1, e2, ids in tables.values():
                e1.grad = e2.grad = None
                p1 = e1[ids]
                if fused:
                    ops_extra.graphaug_lse(p1, e2, 1.0 / m.ssl_temp).mean().backward()
                else:                          # Model/GraphAug.py:540
                    torch.log(torch.exp(p1 @ e2.T / m.ssl_temp).sum(-1)).mean().backward()
        return run

    if a.trace:
        for _ in range(5):
            sampler(True)()
            lse(True)()
        torch.cuda.synchronize()
        print(json.dumps(out))
        return

    opt = torch.optim.Adam(m.parameters(), lr=0.001)

    def step():                                # train_and_evaluate.train's plain branch
        opt.zero_grad()
        m.loss(users, pos, neg).backward()
        opt.step()

    snapshot = [p.detach().clone() for p in m.parameters()]

    def set_flags(name):
        m.fused_edges = m.fused_contrast = name == "step_fused"
        m.fused_edges = m.fused_edges or name == "step_edges_only"
        m.fused_contrast = m.fused_contrast or name == "step_contrast_only"
        with torch.no_grad():
            for p, w in zip(m.parameters(), snapshot):
                p.copy_(w)

    compare(out, [("step_fused", step), ("step_plain_torch", step), ("step_edges_only", step), ("step_contrast_only", step)], a.blocks,
            before=set_flags)
    m.fused_edges = m.fused_contrast = True
    compare(out, [("sampler_fused", sampler(True)), ("sampler_plain_torch", sampler(False)), ("sampler_fused_torch_gather", sampler_gather)],
            a.blocks)
    compare(out, [("lse_fused", lse(True)), ("lse_plain_torch", lse(False))], a.blocks)
    for k in ("step", "sampler", "lse"):
        out[k + "_speedup"] = out[k + "_plain_torch_ms"] / out[k + "_fused_ms"]
        out[k + "_fused_wins"] = bool(out[k + "_plain_torch_ms"] - out[k + "_fused_ms"] > out[k + "_plain_torch_ms_spread"])
    out["edge_table_MB"] = E * 2 * D * 4 / 1e6                             # one gathered [E, 128] fp32 tensor
    out["edge_GEMM_GFLOP"] = 2 * E * 2 * D * D / 1e9                       # the per-edge Linear(128, 64) the split removes
    out["contrast_matrix_MB"] = B * (U + I) * 4 / 1e6                      # the two [B, M] matrices, once
    print(json.dumps(out))


if __name__ == "__main__":
    main()
