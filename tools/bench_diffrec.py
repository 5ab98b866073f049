#!/usr/bin/env python3
"""DiffRec at sports on the MI355X (measurement only): the kernels of csrc/diffrec.hip against the same model's plain routes.

  step    one training step (rows, in-layer, loss, backward, AdamW) on a fixed batch of users: fused against fused = False,
          the reference's training_losses lines in plain torch on device-resident rows (the loader is not credited)
  node    the out-layer, the loss and the backward into h, W_out, b_out alone, on a fixed h: ops.diffrec_x0_loss against
          ops.diffmm_denoise_loss(e_loss = 0) with zero F / x0E, and against plain torch
  eval    one gene_ranklist over all users: collapsed (the chain in hidden space) against the literal chain on the device
  dev     both sampling routes against the literal chain in float64 on the CPU, for the first 64 users: the deviation
          relative to the largest score, and the plain-torch fp32 chain's own deviation on the CPU beside it

    python tools/bench_diffrec.py [--blocks 7] [--batch 1024] [--dataset sports] [--out profiles/diffrec_sports_bench.json]

Every time is the median of `--blocks` timed blocks of at least 50 ms each, the sides alternating block by block, with the
spread (largest - smallest); peak memory of each side from a trimmed allocator.  Prints one JSON line and writes it to --out.
`fused_default` / `collapsed_default` say which route won by more than the spread: the class defaults follow them."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from accept import ULP24, bound_of  # noqa: E402  (the tests' acceptance rule; numpy alone)
from chaorec_amd import dataload, ops  # noqa: E402
from chaorec_amd.Model.DiffRec import DiffRec  # noqa: E402
from tools.bench_mvgae import compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--dataset", default="sports")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diffrec_sports_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    train, _, _, uid, U, I, _, _ = dataload.data_load(a.dataset, has_v=False, has_t=False, data_root=os.path.join(ROOT, "Data"))
    torch.manual_seed(0)
    np.random.seed(0)
    # Model_YAML/DiffRec.yaml of the reference: noise_scale 0.001, noise_min = noise_max = 0.005, steps 5, dims [1000], lr 5e-4
    m = DiffRec(U, I, uid, 0.001, 0.005, 0.005, 5, "[1000]", 0.0005, dev, seed=0)
    B, H = a.batch, m.hidden_width
    out = {"dataset": a.dataset, "U": U, "I": I, "H": H, "E": int(len(train)), "B": B, "steps": m.steps, "blocks": a.blocks}
    users = torch.from_numpy(np.random.default_rng(0).permutation(U)[:B].astype(np.int64)).to(dev)
    m.train()
    opt = torch.optim.AdamW(m.dnn.parameters(), lr=m.learning_rate, weight_decay=0)
    snapshot = [p.detach().clone() for p in m.dnn.parameters()]

    def step():
        opt.zero_grad()
        m.diffusion_step(users).backward()
        opt.step()

    def set_flag(name):
        m.fused = name.endswith("_fused")
        with torch.no_grad():
            for p, w in zip(m.dnn.parameters(), snapshot):
                p.copy_(w)

    compare(out, [("step_fused", step), ("step_plain_torch", step)], a.blocks, before=set_flag)
    set_flag("_fused")

    # the node alone
    W, b = m.dnn.out_layers[0].weight, m.dnn.out_layers[0].bias
    h = torch.tanh(torch.randn(B, H, device=dev)).requires_grad_(True)
    ts = torch.randint(0, m.steps, (B,), device=dev)
    wt, pt = m.weight(ts), torch.rand(B, device=dev, dtype=torch.float64) + 0.5
    x0v, bits = ops.diffmm_rows(users, m.hist[0], m.hist[1], I, plain=True)
    x0 = x0v.contiguous()
    zF, zE = torch.zeros(I, ops.DIFFMM_D, device=dev), torch.zeros(B, ops.DIFFMM_D, device=dev)

    def node_fused():
        ops.diffrec_x0_loss(h, W, b, bits, wt, pt)[0].backward()

    def node_diffmm():           # the DiffMM node with its second term multiplied by zero (no importance weight: pt = 1 there)
        ops.diffmm_denoise_loss(h, W, b, bits, zE, zF, wt, 0.0)[0].backward()

    def node_torch():
        ops.diffrec_x0_loss_plain(h, W, b, x0, wt, pt)[0].backward()

    compare(out, [("node_fused", node_fused), ("node_diffmm_e0", node_diffmm), ("node_plain_torch", node_torch)], a.blocks)

    # one evaluation (a call is far above 50 ms: timed per call)
    for name, flag in (("eval_collapsed", True), ("eval_literal", False)):
        m.collapsed = flag
        m.gene_ranklist(50, to_cpu=False, batch_size=B)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        ts_ = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.gene_ranklist(50, to_cpu=False, batch_size=B)
            torch.cuda.synchronize()
            ts_.append((time.perf_counter() - t0) * 1e3)
        out[name + "_ms"], out[name + "_ms_spread"] = float(np.median(ts_)), float(max(ts_) - min(ts_))
        out[name + "_peak_MiB"] = torch.cuda.max_memory_allocated() / 2 ** 20
    m.collapsed = True

    # both routes against the float64 literal chain on the CPU, 64 users
    m.eval()
    first = torch.arange(64, device=dev)
    with torch.no_grad():
        xs = m.batch_rows(first).contiguous()
        col, lit = m.p_sample(xs).cpu().double(), m.p_sample_literal(xs).cpu().double()
        sd = {n: t.detach().cpu() for n, t in m.dnn.state_dict().items()}
        c1, c2, _, _ = m.posterior_coefs()

        def literal(dtype):
            w = {n: t.to(dtype) for n, t in sd.items()}
            x = xs.cpu().to(dtype)
            for t in range(m.steps - 1, -1, -1):
                emb = F.linear(m.dnn.time_embedding(torch.full((64,), t)).to(dtype), w["emb_layer.weight"], w["emb_layer.bias"])
                hid = torch.tanh(F.linear(torch.cat([x, emb], -1), w["in_layers.0.weight"], w["in_layers.0.bias"]))
                x = c1[t] * F.linear(hid, w["out_layers.0.weight"], w["out_layers.0.bias"]) + c2[t] * x
            return x.double()

        ref, own = literal(torch.float64), literal(torch.float32)
    scale = float(ref.abs().max())
    out["dev_collapsed"], out["dev_literal"] = float((col - ref).abs().max()) / scale, float((lit - ref).abs().max()) / scale
    out["dev_plain_fp32_cpu"] = float((own - ref).abs().max()) / scale
    out["dev_bound"] = bound_of(out["dev_plain_fp32_cpu"], ULP24)

    for k, fast, slow in (("step", "step_fused", "step_plain_torch"), ("node", "node_fused", "node_plain_torch"),
                          ("node_vs_diffmm", "node_fused", "node_diffmm_e0"), ("eval", "eval_collapsed", "eval_literal")):
        out[k + "_speedup"] = out[slow + "_ms"] / out[fast + "_ms"]
        spread = max(out[slow + "_ms_spread"], out[fast + "_ms_spread"])
        out[k + "_wins"] = bool(out[slow + "_ms"] - out[fast + "_ms"] > spread)
    out["fused_default"] = bool(out["step_plain_torch_ms"] >= out["step_fused_ms"])
    out["collapsed_default"] = bool(out["eval_literal_ms"] >= out["eval_collapsed_ms"])
    # what one evaluation must do, from the shapes
    nb = (U + B - 1) // B
    out["eval_literal_TFLOP"] = nb * m.steps * 2 * 2.0 * B * (I + 10) * H / 1e12
    out["eval_collapsed_TFLOP"] = (nb * (2.0 * B * H * I + (m.steps - 1) * 2.0 * B * H * H) + 2.0 * H * I * H) / 1e12
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
