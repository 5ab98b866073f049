#!/usr/bin/env python3
"""CF_Diff's attention core on the MI355X (measurement only): `ops.cfdiff_attention` (csrc/cfdiff.hip) forward + backward in
training mode against `ops.cfdiff_attention_plain` (the same function as torch operations, P materialised) and against
nn.MultiheadAttention(16, 4, dropout = 0.5, batch_first = True) called as the reference calls it (need_weights left at its
default), at L = 1034.

    python tools/bench_cfdiff.py [--blocks 7] [--start 64] [--big 1024] [--out FILE]

B for the comparison is the largest power of two from --start upwards at which both plain routes run one forward + backward
without running out of memory (found by trying; each failure empties the allocator).  The fused node alone is also timed at
--big.  Every time is the median of `--blocks` timed blocks of at least 50 ms each, the sides alternating block by block; the
blocks, their spread (largest - smallest) and each side's peak memory are kept.  `fused_default`: the rule Model/CF_Diff.py's
default follows -- True only when the fused node is faster than the faster plain route by more than the larger of the two
spreads.  Prints one JSON line and writes it to --out (default profiles/cfdiff_attention_bench.json)."""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chaorec_amd import ops  # noqa: E402
from tools.bench_mvgae import compare  # noqa: E402

L = 1034


def sides(B, dev, mha, state):
    gen = torch.Generator(device=dev).manual_seed(B)
    q, k, v, go = (torch.randn(B, L, 16, device=dev, generator=gen) * 0.5 for _ in range(4))
    q, k, v = (t.requires_grad_() for t in (q, k, v))

    def fused():
        ops.cfdiff_attention(q, k, v, True, 7, state, 0).backward(go)

    def plain():
        ops.cfdiff_attention_plain(q, k, v, True, keep=torch.rand(B, 4, L, L, device=dev) < 0.5).backward(go)

    def module():
        mha(q, k, k)[0].backward(go)

    return fused, plain, module


def fits(fn):
    try:
        fn()
        torch.cuda.synchronize()
        return True
    except torch.cuda.OutOfMemoryError:
        return False
    finally:
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--start", type=int, default=64)
    ap.add_argument("--big", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    mha = nn.MultiheadAttention(16, 4, dropout=0.5, batch_first=True).to(dev).train()
    state = torch.zeros(2, dtype=torch.int64, device=dev)
    ops.step_tick(state)
    out = {"L": L, "blocks": a.blocks, "max_len": ops.cfdiff_max_len(), "device_GiB": torch.cuda.get_device_properties(0).total_memory / 2 ** 30}
    B = a.start
    while B * 2 <= a.big:
        _, plain, module = sides(B * 2, dev, mha, state)
        if not (fits(plain) and fits(module)):
            break
        B *= 2
        print(f"both plain routes fit at B = {B}", file=sys.stderr, flush=True)
    out["B"] = B
    fused, plain, module = sides(B, dev, mha, state)
    compare(out, [("fused", fused), ("plain", plain), ("module", module)], a.blocks)
    print(f"B = {B}: fused {out['fused_ms']:.3f} ms, plain {out['plain_ms']:.3f} ms, module {out['module_ms']:.3f} ms", file=sys.stderr, flush=True)
    del plain, module
    torch.cuda.empty_cache()
    out["B_big"] = a.big
    big = sides(a.big, dev, mha, state)[0]
    compare(out, [("fused_big", big)], a.blocks)
    best_plain = min(("plain", "module"), key=lambda n: out[n + "_ms"])
    gain = out[best_plain + "_ms"] - out["fused_ms"]
    out["speedup_over_plain"] = out["plain_ms"] / out["fused_ms"]
    out["speedup_over_module"] = out["module_ms"] / out["fused_ms"]
    out["fused_default"] = bool(gain > max(out["fused_ms_spread"], out[best_plain + "_ms_spread"]))
    line = json.dumps(out)
    print(line)
    path = a.out or os.path.join(ROOT, "profiles", "cfdiff_attention_bench.json")
    with open(path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
