#!/usr/bin/env python3
"""BSPM on the MI355X (measurement only): the launches of csrc/bspm.hip for one full tile of 1024 users -- project, seed,
last step -- against the launches ops.bspm_scores_plain composes for the same work, one SpMM step at D = 1024 (the middle
Euler steps; nobody had measured the SpMM at that width), and the whole ranking of every user, fused against plain.

    python tools/bench_bspm.py [--blocks 7] [--dataset sports] [--K_s 1] [--out FILE]

Every time is the median of `--blocks` timed blocks of at least 50 ms each, the sides alternating block by block; the blocks
and their spread (largest - smallest) are kept.  `fused_default`: the rule Model/BSPM.py's default follows -- True only when the
fused ranking is faster than the plain one by more than the larger of the two spreads.  The model's construction (host: degrees,
the item-item product, the truncated SVD) is timed once, apart.  Prints one JSON line and writes it to --out (default
profiles/bspm_<dataset>_bench.json)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chaorec_amd import dataload, ops  # noqa: E402
from chaorec_amd.Model import BSPM  # noqa: E402
from tools.bench_mvgae import compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--dataset", default="sports")
    ap.add_argument("--K_s", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    train, _, _, uid, U, I, _, _ = dataload.data_load(a.dataset, has_v=False, has_t=False, data_root=os.path.join(ROOT, "Data"))
    t0 = time.perf_counter()
    m = BSPM(U, I, train, uid, a.K_s, 1.0, 1, 1, 1.0, dev)               # the parser's defaults but for --K_s
    construct_s = time.perf_counter() - t0
    f, P = m.filter, m.filter.P
    deg = P.rowptr[1:] - P.rowptr[:-1]
    B = ops.BSPM_MAX_TILE
    tile = m.tile(torch.arange(B, dtype=torch.int64, device=dev))
    long_row = ops.bspm_long_row()
    out = {"dataset": a.dataset, "U": U, "I": I, "E": int(len(train)), "B": B, "m": f.m, "K_s": a.K_s, "blocks": a.blocks,
           "P_nnz": P.nnz, "P_longest_row": int(deg.max()), "P_median_row": int(deg.median()), "long_row": long_row,
           "P_rows_past_long_row": int((deg > long_row).sum()), "P_entries_in_them": int(deg[deg > long_row].sum()),
           "tile_entries": tile.nnz, "tiles": (U + B - 1) // B, "construct_s": round(construct_s, 2)}
    h = ops.bspm_step_sizes(a.K_s, 1.0)[-1]
    Z = ops.bspm_project(tile, f.F)
    idlT = ops.bspm_idl(f, Z)
    Yt = ops.bspm_seed(P, tile, 1.0, idlT)
    Y2, sc = torch.empty_like(Yt), torch.empty((B, I), dtype=torch.float32, device=dev)
    Xt = torch.zeros((I, B), dtype=torch.float32, device=dev)
    slot = tile.xt_slot.to(torch.int64)

    def seed_plain():
        Xt.zero_()
        Xt[tile.xt_item, slot] = tile.xt_val
        y = ops.spmm_raw(P, Xt, y=Y2)
        return idlT.mul(1.0).add_(y)

    def end_plain():
        y = ops.spmm_raw(P, Yt, y=Y2, alpha=-h, z=Yt, beta=1.0)
        sc.copy_(y.t())
        sc[slot, tile.xt_item] = 1e-6

    compare(out, [("project", lambda: ops.bspm_project(tile, f.F, out=Z)), ("project_plain_mm", lambda: torch.mm(Xt.t(), f.F))], a.blocks)
    compare(out, [("idl_mm", lambda: ops.bspm_idl(f, Z))], a.blocks)
    compare(out, [("seed", lambda: ops.bspm_seed(P, tile, 1.0, idlT, out=Y2)), ("seed_plain", seed_plain)], a.blocks)
    compare(out, [("last_step", lambda: ops.bspm_last_step(P, Yt, h, tile, 1e-6, out=sc)), ("end_plain", end_plain),
                  ("spmm_step_D1024", lambda: ops.spmm_raw(P, Yt, y=Y2, alpha=-h, z=Yt, beta=1.0))], a.blocks)
    out["last_step_gather_GB"] = P.nnz * B * 4 / 1e9
    out["last_step_gather_TBps"] = out["last_step_gather_GB"] / out["last_step_ms"]
    out["spmm_step_gather_TBps"] = out["last_step_gather_GB"] / out["spmm_step_D1024_ms"]

    def ranking(fused):
        def run():
            m.fused = fused
            m.gene_ranklist(50, to_cpu=False)
        return run

    m.fused = True
    fused_rank = m.gene_ranklist(50, to_cpu=False)
    m.fused = False
    plain_rank = m.gene_ranklist(50, to_cpu=False)
    out["rank_rows_identical"] = float((fused_rank == plain_rank).all(1).float().mean())
    compare(out, [("ranking_fused", ranking(True)), ("ranking_plain", ranking(False))], a.blocks)
    m.fused = True
    gain = out["ranking_plain_ms"] - out["ranking_fused_ms"]
    out["ranking_speedup"] = out["ranking_plain_ms"] / out["ranking_fused_ms"]
    out["fused_default"] = bool(gain > max(out["ranking_fused_ms_spread"], out["ranking_plain_ms_spread"]))
    line = json.dumps(out)
    print(line)
    path = a.out or os.path.join(ROOT, "profiles", f"bspm_{a.dataset}_bench.json")
    with open(path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
