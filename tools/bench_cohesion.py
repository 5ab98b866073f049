#!/usr/bin/env python3
"""COHESION at sports on the MI355X (measurement only): the eager training step with the fused node (ops_extra.cohesion_fuse)
against the SAME model with `fused_aggregation = False`, i.e. the reference's lines in plain torch (the [N, 192] concatenation,
features[user_graph] gathered to [U, k, 192], matmul with the weights, the 192-wide item-graph product, the final cat); the node
alone, forward + backward, both ways and at chunk = 64 and chunk = 0 (the unchunked walk); peak memory of each;
pre_epoch_processing() with the chunk index.

    python tools/bench_cohesion.py [--steps 50] [--dataset sports] [--trace]

Prints one JSON line.  --trace runs only a few forward / backward passes of the node at chunk 64 and chunk 0, for
`rocprofv3 --kernel-trace --stats -- python tools/bench_cohesion.py --trace` (kernel times come from the trace, in a run of its
own).  Features are the seeded synthetic ones every multimodal model gets for the committed datasets."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chaorec_amd import dataload, ops_extra, sparse  # noqa: E402
from chaorec_amd.Model import COHESION  # noqa: E402
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
    ap.add_argument("--dataset", default="sports")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    train, _, _, uid, U, I, v_feat, t_feat = dataload.data_load(a.dataset, data_root=os.path.join(ROOT, "Data"))
    torch.manual_seed(0)
    np.random.seed(0)
    COHESION.user_graph_path = None
    # Model_YAML/COHESION.yaml: reg_weight 0.001, dropout 0, n_layers 1, mm_layers 1, ii_topk 10, mm_image_weight 0.1
    m = COHESION(U, I, train, uid, v_feat, t_feat, 64, 0.001, 0.0, 1, 1, 10, 0.1, dev).to(dev)
    s, k, D = m.graph_structure, m.k, 64
    out = {"dataset": a.dataset, "U": U, "I": I, "E": int(len(train)), "B": a.batch, "k": k, "steps": a.steps}
    m.pre_epoch_processing()
    lengths = (s.rev_ptr[1:] - s.rev_ptr[:-1]).cpu().numpy()
    out["longest_reverse_list"], out["median_reverse_list"] = int(lengths.max()), float(np.median(lengths))
    out["n_chunks_64"], out["n_chunks_0"] = s.rev_chunks[64].n_chunks, ops_extra.usergraph_rev_chunks(s, 0).n_chunks

    pick = np.random.default_rng(0).choice(len(train), size=a.batch, replace=False)
    users = torch.from_numpy(train[pick, 0].astype(np.int64)).to(dev)
    pos = torch.from_numpy(train[pick, 1].astype(np.int64)).to(dev)
    neg = torch.from_numpy(np.random.default_rng(1).integers(U, U + I, a.batch)).to(dev)
    m.loss(users, pos, neg)       # one forward: the three tables the node is timed on
    idr = m.id_rep.detach().clone()
    v, t = m.v_rep.detach().clone().requires_grad_(True), m.t_rep.detach().clone().requires_grad_(True)
    h_id = m._item_graph(idr, False)
    g = torch.randn(U + I, 3 * D, device=dev)
    idx = s.epoch_idx.long()

    def node_fused(chunk=64):
        h_v, h_t = m._item_graph(v), m._item_graph(t)
        ops_extra.cohesion_fuse(idr, v, t, h_id, h_v, h_t, s, U, chunk=chunk).backward(g)

    def node_torch():       # Model/COHESION.py:340-359
        rep = torch.cat((idr, v, t), dim=1)
        user_rep, item_rep = rep[:U], rep[U:]
        h_i = item_rep
        for _ in range(m.n_layers):
            h_i = sparse.mm(m.mm_adj, h_i)
        h_u = torch.matmul(s.epoch_w.unsqueeze(1), user_rep[idx]).squeeze(1)
        torch.cat((user_rep + h_u, item_rep + h_i), dim=0).backward(g)

    if a.trace:
        for chunk in (64, 0):
            for _ in range(5):
                node_fused(chunk)
        torch.cuda.synchronize()
        print(json.dumps(out))
        return

    out["pre_epoch_ms"] = timed(m.pre_epoch_processing, 10, warmup=2)
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.001}])

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
    m.fused_aggregation = True

    # the node alone (with its item-graph products), forward + backward, on the tables of the last forward
    for rep in range(2):
        for name, fn in (("node_fused_chunk64", node_fused), ("node_fused_chunk0", lambda: node_fused(0)), ("node_plain_torch", node_torch)):
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ms = timed(fn, a.steps)
            out.setdefault(name + "_ms_blocks", []).append(round(ms, 4))
            out[name + "_ms"] = ms
            out[name + "_extra_peak_MiB"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    out["node_speedup"] = out["node_plain_torch_ms"] / out["node_fused_chunk64_ms"]
    # bytes the fused launches must move (gathered rows come from L2): forward reads (k + 1) rows of three tables per user and
    # the item rows of the tables and of the h tables, writes the result; the chunk launch reads 512 B of g per reverse entry
    # and writes the partials; the row launch reads g's live columns and the partials, writes dv, dt, dh_v, dh_t
    n_chunks = s.rev_chunks[64].n_chunks
    out["node_fwd_MB"] = (U * (k + 1) * 3 * D * 4 + I * 6 * D * 4 + (U + I) * 3 * D * 4 + U * k * 8) / 1e6
    out["node_bwd_chunk_MB"] = (U * k * (2 * D * 4 + 8) + n_chunks * (2 * D * 4 + 12)) / 1e6
    out["node_bwd_rows_MB"] = ((U + I) * 2 * D * 4 * 2 + I * 2 * D * 4 + n_chunks * 2 * D * 4) / 1e6
    print(json.dumps(out))


if __name__ == "__main__":
    main()
