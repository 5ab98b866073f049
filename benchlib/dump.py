"""--dump-outputs DIR: what the timed path computed in its last step, as DIR/<name>.npy (float32), for comparing two builds
output for output.  At most LIMIT_BYTES in all: when the arrays are larger, every 2-D array keeps a fixed sample of its rows
(same rows for the same shape, run after run: numpy's default_rng(0)); the sampled row numbers are not written."""
import os

import numpy as np
import torch

LIMIT_BYTES = 64 << 20


def sample_rows(n_rows, k):
    """-> sorted int64 row numbers: a seeded sample of k of n_rows (all of them when k >= n_rows)."""
    if k >= n_rows:
        return np.arange(n_rows, dtype=np.int64)
    return np.sort(np.random.default_rng(0).choice(n_rows, size=k, replace=False)).astype(np.int64)


def write(out_dir, arrays):
    """arrays: {name: tensor (any device)} -> DIR/<name>.npy in float32, sampled by rows to stay within LIMIT_BYTES.
    -> {name: [shape written, rows of the full array]}."""
    os.makedirs(out_dir, exist_ok=True)
    budget = LIMIT_BYTES - 256 * len(arrays)            # (room for the .npy headers)
    total = sum(t.numel() * 4 for t in arrays.values())
    small = sum(t.numel() * 4 for t in arrays.values() if t.dim() != 2)
    scale = 1.0 if total <= budget else (budget - small) / max(total - small, 1)
    written = {}
    for name, t in arrays.items():
        t = t.detach()
        if t.dim() == 2 and scale < 1.0:
            rows = sample_rows(t.shape[0], max(1, int(t.shape[0] * scale)))
            t = t.index_select(0, torch.from_numpy(rows).to(t.device))
        a = t.to(torch.float32).cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = [list(a.shape), int(arrays[name].shape[0]) if arrays[name].dim() else 1]
    return written
