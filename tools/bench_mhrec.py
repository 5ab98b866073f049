#!/usr/bin/env python3
"""MHRec on the MI355X (measurement only): the hypergraph attention layer, forward + backward, as the fused node
(ops_extra.mhrec_hyper_layer, csrc/mhrec.hip) against the plain-torch restatement on the same HyperGraph
(ops_extra.mhrec_hyper_layer_torch: gathers, a [nnz, 128] concatenation, two index_adds); and one epoch of
epochs._train_epoch_mhrec split into its three phases -- the two diffusion passes, the rebuild, the BPR steps -- with
`fused_hyper` on and off.  The hypergraph is the one the untrained denoisers rebuild (hub-heavy, as the model's own are).

    python tools/bench_mhrec.py [--blocks 7] [--batch 1024] [--dataset baby] [--num_hypernodes 10] [--epochs 2] [--out FILE]

Layer times: the median of `--blocks` timed blocks of at least 50 ms each, the sides alternating block by block; the blocks and
their spread (largest - smallest) are kept.  Phase times: wall time per phase with a device synchronisation at each end, the
median over `--epochs` epochs after one warm-up epoch, the sides alternating.  Prints one JSON line and writes it to --out
(default profiles/mhrec_<dataset>_bench.json).  The plain-torch side is slow on hub rows (double atomics): at baby allow the run
more than 400 s, or pass --epochs 1."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chaorec_amd import dataload, epochs, ops_extra  # noqa: E402
from chaorec_amd.Model import MHRec  # noqa: E402
from chaorec_amd.optim import FusedAdam  # noqa: E402
from tools.bench_mvgae import compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dataset", default="baby")
    ap.add_argument("--num_hypernodes", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    train, _, _, uid, U, I, v_feat, t_feat = dataload.data_load(a.dataset, data_root=os.path.join(ROOT, "Data"))
    torch.manual_seed(0)
    np.random.seed(0)
    # Model_YAML/MHRec.yaml but for num_hypernodes (the command line's default, 10: the larger incidence list)
    m = MHRec(U, I, train, uid, v_feat, t_feat, 64, 1e-4, 10, 10, a.num_hypernodes, 3, 2, 0.1, 0.01, 0.5, 0.5, dev).train()
    N, D = U + I, 64
    loader = dataload.DeviceBatchSampler(U, I, uid, train, a.batch, dev, "MHRec", 42)
    n_in = int(m.diffusion_tables()[0].shape[0])
    diff_loaders = tuple(dataload.DeviceUserBatches(n_in, a.batch, dev, 42 + k) for k in range(2))
    Hv, _ = m.rebuild_hypergraphs(*diff_loaders)
    deg = Hv.degrees()
    out = {"dataset": a.dataset, "U": U, "I": I, "N": N, "E": Hv.num_edges, "k": Hv.k, "nnz": Hv.num_edges * Hv.k, "B": a.batch,
           "blocks": a.blocks, "longest_row": int(deg.max()), "rows_without_entries": int((deg == 0).sum()),
           "median_row_of_the_others": int(deg[deg > 0].median()), "long_rows": Hv.n_long, "chunks": Hv.n_chunks,
           "long_row_threshold": ops_extra.mhrec_long_row(), "steps_per_epoch": len(loader), "diffusion_batches": len(diff_loaders[0])}

    X0 = (0.1 * torch.randn(N, D, device=dev))
    a0 = m.hypergraphLayersVisual[0].a.detach().clone()
    g = torch.randn(N, D, device=dev)
    state = torch.zeros(2, dtype=torch.int64, device=dev)

    def layer_fused():
        X, av = X0.clone().requires_grad_(True), a0.clone().requires_grad_(True)
        ops_extra.mhrec_hyper_layer(Hv, X, av, None, state, 1, 0, True).backward(g)

    def layer_plain():
        X, av = X0.clone().requires_grad_(True), a0.clone().requires_grad_(True)
        ops_extra.mhrec_hyper_layer_torch(Hv, X, av, None, True).backward(g)

    compare(out, [("layer_fused", layer_fused), ("layer_plain_torch", layer_plain)], a.blocks)
    out["layer_speedup"] = out["layer_plain_torch_ms"] / out["layer_fused_ms"]
    # the default's rule: fused unless it is slower than the plain layer by more than the blocks' spread
    out["layer_fused_not_slower"] = bool(out["layer_fused_ms"] - out["layer_plain_torch_ms"]
                                         <= max(out["layer_fused_ms_spread"], out["layer_plain_torch_ms_spread"]))
    out["layer_gather_MB"] = 2 * 2 * out["nnz"] * D * 4 / 1e6          # each way: X rows per ELL entry, Eo / dE rows per CSR entry

    opt = FusedAdam([{'params': m.parameters(), 'lr': 1e-3}])
    snapshot = [p.detach().clone() for p in m.parameters()]
    phases = {True: [], False: []}
    for ep in range(1 + a.epochs):
        for fused in (True, False):
            m.fused_hyper = fused
            with torch.no_grad():
                for p, w in zip(m.parameters(), snapshot):
                    p.copy_(w)
            times = {}
            epochs._train_epoch_mhrec(m, loader, opt, diff_loaders, times)
            if ep:
                phases[fused].append(times)
    m.fused_hyper = True
    for fused, name in ((True, "fused"), (False, "plain_torch")):
        for ph in ("diffusion", "rebuild", "bpr"):
            ts = [t[ph] * 1e3 for t in phases[fused]]
            out[f"epoch_{name}_{ph}_ms"] = float(np.median(ts))
            out[f"epoch_{name}_{ph}_ms_all"] = [round(x, 2) for x in ts]
        out[f"epoch_{name}_ms"] = sum(out[f"epoch_{name}_{ph}_ms"] for ph in ("diffusion", "rebuild", "bpr"))
        out[f"epoch_{name}_bpr_step_ms"] = out[f"epoch_{name}_bpr_ms"] / len(loader)
    out["denoiser_share_of_fused_epoch"] = (out["epoch_fused_diffusion_ms"] + out["epoch_fused_rebuild_ms"]) / out["epoch_fused_ms"]
    # a denoiser forward is 2 x 1000 x (2 N + 10) FLOP per row; per epoch and modality the diffusion pass runs it three times over
    # (forward, input and weight gradients), the rebuild twenty times
    fwd = 2 * 1000 * (2 * N + 10)
    out["denoiser_GFLOP_per_epoch"] = 2 * n_in * fwd * (3 + 20) / 1e9
    line = json.dumps(out)
    print(line)
    path = a.out or os.path.join(ROOT, "profiles", f"mhrec_{a.dataset}_bench.json")
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
