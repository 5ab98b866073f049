#!/usr/bin/env python3
"""Rank lists past 64 columns on the MI355X (measurement only): ops.score_topk at K = 100 and K = 1000 -- the whole call
(user ranges: chaorec_score_rows_f32 into the staging block, chaorec_rows_topk_wide_f32 out of it) and its two launches alone
on one range -- beside the existing K = 50 call, for scale, and the plain-torch composition the reference would use: chunked
matmul, history mask, torch.topk, over the same user ranges.

    python tools/bench_wide_topk.py [--blocks 5] [--dataset sports] [--D 64] [--out FILE]

Seeded synthetic tables of the dataset's shape (Gaussian x 0.1) and the history of the synthetic interaction graph.  Every time
is the median of `--blocks` timed blocks of at least 50 ms each, the sides alternating block by block; the blocks, their spread
(largest - smallest) and the peak memory of one block are kept (tools/bench_mvgae.compare).  score_rows_TFLOPs is 2 n I D over
the launch's time: the f32 MFMA chain it is bound by.  Prints one JSON line and writes it to --out (default
profiles/wide_topk_bench.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chaorec_amd import ops  # noqa: E402
from chaorec_amd.synthetic import DATASET_SHAPES, synthetic_interactions  # noqa: E402
from tools.bench_mvgae import compare  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--dataset", default="sports")
    ap.add_argument("--D", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    U, I, E = DATASET_SHAPES[a.dataset]
    D = a.D
    edges = synthetic_interactions(U, I, E, seed=42).astype(np.int64)
    order = np.lexsort((edges[:, 1], edges[:, 0]))
    rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(edges[:, 0], minlength=U))]).astype(np.int64)).to(dev)
    col = torch.from_numpy((edges[order, 1] - U).astype(np.int32)).to(dev)
    hist = (rowptr, col)
    g = torch.Generator().manual_seed(0)
    ue = (torch.randn(U, D, generator=g) * 0.1).to(dev)
    ie = (torch.randn(I, D, generator=g) * 0.1).to(dev)
    ld = (I + 3) // 4 * 4
    per = min(U, ops.wide_range_users(ld))
    ranges = [(u0, min(U, u0 + per)) for u0 in range(0, U, per)]
    out = {"dataset": a.dataset, "U": U, "I": I, "D": D, "E": E, "blocks": a.blocks, "staging_bytes": ops.WIDE_STAGING_BYTES,
           "range_users": per, "ranges": len(ranges), "score_matrix_GB": U * I * 4 / 1e9}

    # the torch composition's mask, per range, built once (the reference rebuilds it in a python loop per call)
    rows_of = torch.repeat_interleave(torch.arange(U, device=dev), rowptr[1:] - rowptr[:-1])
    masks = []
    for u0, u1 in ranges:
        sel = (rows_of >= u0) & (rows_of < u1)
        masks.append((rows_of[sel] - u0, col[sel].long()))

    def torch_rank(K):
        def run():
            res = torch.empty((U, K), dtype=torch.int64, device=dev)
            for (u0, u1), (r, c) in zip(ranges, masks):
                s = ue[u0:u1] @ ie.t()
                s[r, c] = 1e-6
                res[u0:u1] = torch.topk(s, K, dim=1)[1] + U
            return res
        return run

    stage = torch.empty(per * ld, dtype=torch.float32, device=dev)
    n0 = ranges[0][1] - ranges[0][0]
    sc = ops.score_rows(ue, ie, hist, 1e-6, 0, n0, out=stage, ld=ld)
    narrow = ops.score_topk(ue, ie, hist, 1e-6, 50, id_offset=U)[0]
    compare(out, [("narrow_K50", lambda: ops.score_topk(ue, ie, hist, 1e-6, 50, id_offset=U)),
                  ("score_rows_one_range", lambda: ops.score_rows(ue, ie, hist, 1e-6, 0, n0, out=stage, ld=ld))], a.blocks)
    out["score_rows_TFLOPs"] = 2.0 * n0 * I * D / (out["score_rows_one_range_ms"] * 1e-3) / 1e12
    for K in (100, 1000):
        wide = ops.score_topk(ue, ie, hist, 1e-6, K, id_offset=U)[0]
        ref = torch_rank(K)()
        out[f"K{K}_first_50_equal_narrow"] = bool(torch.equal(wide[:, :50], narrow))
        out[f"K{K}_rows_identical_to_torch"] = float((wide == ref).all(1).float().mean())
        compare(out, [(f"wide_K{K}", lambda: ops.score_topk(ue, ie, hist, 1e-6, K, id_offset=U)),
                      (f"torch_K{K}", torch_rank(K)),
                      (f"rows_topk_wide_K{K}_one_range", lambda: ops.rows_topk_wide(sc, K, U, n_cols=I))], a.blocks)
        out[f"K{K}_torch_over_wide"] = out[f"torch_K{K}_ms"] / out[f"wide_K{K}_ms"]
    line = json.dumps(out)
    print(line)
    path = a.out or os.path.join(ROOT, "profiles", "wide_topk_bench.json")
    with open(path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
