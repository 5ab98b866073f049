#!/usr/bin/env python3
"""DiffMM at sports on the MI355X (measurement only): every item with the fused kernels (ops_extra.diffmm_rows /
diffmm_denoise_loss) against the SAME model with `fused_denoise = False`, i.e. the reference's lines in plain torch:

  step     one diffusion step (both modalities, backward, both Adam steps) on a fixed batch of users; the plain side is fed
           from device-resident rows (Model.batch_rows from the history CSR), so the loader is not credited
  node     the out-layer, both losses and the backward into h, W_out, b_out alone, on a fixed h
  rows     the noised, dropped-out rows alone: one launch against randn_like + q_sample + dropout on device rows
  rebuild  rebuild_graphs over all users
  epoch    _train_epoch_diffmm: the diffusion pass, the rebuild, the BPR steps (--epoch; minutes on the plain side)

    python tools/bench_diffmm.py [--blocks 7] [--batch 1024] [--dataset sports] [--epoch]

Every time is the median of `--blocks` timed blocks of at least 50 ms each, the two sides alternating block by block, with
the spread (largest - smallest); peak memory of each side from a trimmed allocator.  Prints one JSON line.  Features are the
seeded synthetic ones every multimodal model gets for the committed datasets."""
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
from chaorec_amd import dataload, epochs, ops_extra  # noqa: E402
from chaorec_amd.Model import DiffMM  # noqa: E402
from chaorec_amd.optim import FusedAdam  # noqa: E402
from tools.bench_mvgae import compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dataset", default="sports")
    ap.add_argument("--epoch", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    train, _, _, uid, U, I, v_feat, t_feat = dataload.data_load(a.dataset, data_root=os.path.join(ROOT, "Data"))
    torch.manual_seed(0)
    np.random.seed(0)
    # Model_YAML/DiffMM.yaml
    m = DiffMM(U, I, train, uid, v_feat, t_feat, 64, 1e-4, 1, 0.01, 0.1, 0.5, 0.01, 1, dev)
    B = a.batch
    out = {"dataset": a.dataset, "U": U, "I": I, "E": int(len(train)), "B": B, "blocks": a.blocks}
    users = torch.from_numpy(np.random.default_rng(0).permutation(U)[:B].astype(np.int64)).to(dev)
    m.train()
    opts = [torch.optim.Adam(d.parameters(), lr=1e-3, weight_decay=0) for d in (m.denoise_model_image, m.denoise_model_text)]
    snapshot = [p.detach().clone() for d in (m.denoise_model_image, m.denoise_model_text) for p in d.parameters()]

    def step():
        for o in opts:
            o.zero_grad()
        li, lt = m.diffusion_step(users)
        (li + lt).backward()
        for o in opts:
            o.step()

    def set_flag(name):
        m.fused_denoise = name.endswith("_fused")
        with torch.no_grad():
            for p, w in zip((p for d in (m.denoise_model_image, m.denoise_model_text) for p in d.parameters()), snapshot):
                p.copy_(w)

    compare(out, [("step_fused", step), ("step_plain_torch", step)], a.blocks, before=set_flag)

    # the node alone
    dn, dm = m.denoise_model_image, m.diffusion_model
    W, b = dn.out_layers[0].weight, dn.out_layers[0].bias
    h = torch.tanh(torch.randn(B, 1000, device=dev)).requires_grad_(True)
    ts = torch.randint(0, 5, (B,), device=dev)
    wt = dm.weight(ts)
    feat, iE = m.getImageFeats().detach().contiguous(), m.iEmbeds.detach()
    x0v, bits = ops_extra.diffmm_rows(users, m.hist[0], m.hist[1], I, plain=True)
    x0 = x0v.contiguous()
    x0E = (x0 @ iE).contiguous()

    def node_fused():
        ops_extra.diffmm_denoise_loss(h, W, b, bits, x0E, feat, wt, m.e_loss)[0].backward()

    def node_torch():            # Model/DiffMM.py:468-471, :640-658
        o = F.linear(h, W, b)
        diff = wt * ((x0 - o) ** 2).mean(1)
        gc = ((o @ feat - x0 @ iE) ** 2).mean(1)
        (diff.mean() + gc.mean() * m.e_loss).backward()

    compare(out, [("node_fused", node_fused), ("node_plain_torch", node_torch)], a.blocks)

    # the rows alone
    a_row, s_row = dm.sqrt_alphas_cumprod[ts].float().contiguous(), dm.sqrt_one_minus_alphas_cumprod[ts].float().contiguous()
    step_no = [0]

    def rows_fused():
        step_no[0] += 1
        ops_extra.diffmm_rows(users, m.hist[0], m.hist[1], I, a_row, s_row, seed=1, step=step_no[0], salt=0)

    def rows_torch():            # Model/DiffMM.py:629-632, :458-459 on device-resident rows
        F.dropout(dm.q_sample(x0, ts, torch.randn_like(x0)), 0.5, True)

    compare(out, [("rows_fused", rows_fused), ("rows_plain_torch", rows_torch)], a.blocks)

    # the rebuild (one call is far above 50 ms on the plain side: timed per call)
    loader = dataload.DeviceUserBatches(U, B, dev, seed=0, shuffle=False)
    for name, flag in (("rebuild_fused", True), ("rebuild_plain_torch", False)):
        m.fused_denoise = flag
        m.rebuild_graphs(loader)
        ts_ = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.rebuild_graphs(loader)
            torch.cuda.synchronize()
            ts_.append((time.perf_counter() - t0) * 1e3)
        out[name + "_ms"], out[name + "_ms_spread"] = float(np.median(ts_)), float(max(ts_) - min(ts_))

    if a.epoch:
        sampler = dataload.DeviceBatchSampler(U, I, uid, train, 2048, dev, "DiffMM", 42)
        opt = FusedAdam([{"params": m.parameters(), "lr": 1e-3}])
        for name, flag in (("epoch_fused", True), ("epoch_plain_torch", False)):
            m.fused_denoise = flag
            ts_ = []
            for k in range(3):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                epochs._train_epoch_diffmm(m, sampler, opt)
                torch.cuda.synchronize()
                if k:
                    ts_.append(time.perf_counter() - t0)
            out[name + "_s"], out[name + "_s_spread"] = float(np.median(ts_)), float(max(ts_) - min(ts_))
            out[name + "_peak_MiB"] = torch.cuda.max_memory_allocated() / 2 ** 20
    m.fused_denoise = True
    for k in ("step", "node", "rows"):
        out[k + "_speedup"] = out[k + "_plain_torch_ms"] / out[k + "_fused_ms"]
        spread = max(out[k + "_plain_torch_ms_spread"], out[k + "_fused_ms_spread"])
        out[k + "_fused_wins"] = bool(out[k + "_plain_torch_ms"] - out[k + "_fused_ms"] > spread)
    # what the one-pass launch must do and move, from the shapes
    out["node_GFLOP"] = 2.0 * B * I * (1000 + 64) / 1e9
    out["node_MB"] = (I * 1000 * 4 + B * 1000 * 4 + B * I * 4 + I * 64 * 4) / 1e6
    print(json.dumps(out))


if __name__ == "__main__":
    main()
