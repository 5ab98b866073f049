#!/usr/bin/env python3
"""Records chaorec_score_topk_workspace_bytes over a grid of (users, items, K, D) that flips every condition of
plan_score (score_topk.hip) at least once -> score_workspace_bytes.json, which tests/test_host_logic.py pins.

The number is what ops.score_topk and benchlib cut users into ranges with, and it is device-independent by design (the
candidate region is sized for kPfMaxSplits).  The committed file was recorded at feb0de9, before the ranking host code
was cut into one function per route; run this again only when a change MEANS to move the layout:
    python3 tests/golden/gen_score_workspace.py      (no GPU needed)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CLS_ENV = ("CHAOREC_PF_CLS_MIN_ITEMS", "CHAOREC_PF_CLS_STRIDE", "CHAOREC_PF_CLS_RANK")

GRID = [
    (100, 1000, 50, 64),                                    # neither prefilter nor sampling
    (63, 5000, 50, 32), (64, 5000, 50, 32),                 # the packed table, from 64 users on
    (4096, 4064, 50, 64), (4096, 4096, 50, 64),             # 127 and 128 tiles: the prefilter appears
    (4096, 16384, 50, 128), (4096, 16416, 50, 128),         # 512 and 513 tiles: the long sampler
    (4096, 131071, 50, 64), (4096, 131072, 50, 64),         # pass C and the grouped fallback
    (1024, 524320, 50, 64), (1024, 1048608, 50, 64),        # sample stride 8 and 16
    (440000, 524288, 50, 64), (500000, 524288, 50, 64),     # the sorted table by size: 1.48e13 and 1.68e13 against 1.5e13
    (4096, 20000, 1, 64), (4096, 20000, 50, 64), (4096, 20000, 64, 64),                                       # K
    (4096, 20000, 50, 8), (4096, 20000, 50, 16), (4096, 20000, 50, 32), (4096, 20000, 50, 192), (4096, 20000, 50, 256),  # D
    (32, 200000, 50, 256),                                  # many splits with few users
    (28940, 15207, 50, 64),                                 # sports
]
ENV_ROWS = [
    ((2048, 20000, 50, 64), {"CHAOREC_PF_CLS_MIN_ITEMS": "4096"}),                                 # the sorted layout by environment
    ((2048, 20000, 50, 64), {"CHAOREC_PF_CLS_MIN_ITEMS": "4096", "CHAOREC_PF_CLS_STRIDE": "3"}),   # the sampler's own table
]


def main():
    sys.path.insert(0, ROOT)
    from chaorec_amd import _lib
    _lib.ensure_built()
    query = _lib.load().chaorec_score_topk_workspace_bytes
    rows = []
    for shape, env in [(s, {}) for s in GRID] + ENV_ROWS:
        for name in CLS_ENV:
            os.environ.pop(name, None)
        os.environ.update(env)       # (read per call by the library)
        users, items, k, d = shape
        rows.append({"users": users, "items": items, "K": k, "D": d, "env": env, "bytes": query(users, items, k, d)})
    with open(os.path.join(HERE, "score_workspace_bytes.json"), "w") as f:
        f.write("[\n" + ",\n".join(" " + json.dumps(r) for r in rows) + "\n]\n")
    print(f"{len(rows)} rows")


if __name__ == "__main__":
    main()
