"""The smallest bipartite graph with every kind of SpMM row, shared by tests/test_gpu_gated_z.py and
tests/test_gpu_inner_mean_rows.py: N = 151 rows (no multiple of the 4 rows of a wave or of a 32-bit bitmap word, the bitmap's
last word partly used), one row above the long-row threshold, one just past the six inline entries of a descriptor, one of a
single entry and an empty one."""
import numpy as np

N_USER, N_ITEM = 90, 61
N = N_USER + N_ITEM
LONG_ROW, MID_ROW, ONE_ROW, EMPTY_ROW = 0, 1, 2, N_USER - 1      # users of 40, 9, 1 and 0 entries


def small_edges():
    """int64 [E, 2] (user, N_USER + item) pairs in a fixed shuffled order."""
    rng = np.random.default_rng(151)
    pairs = [(LONG_ROW, i) for i in rng.permutation(N_ITEM)[:40]]
    pairs += [(MID_ROW, i) for i in rng.permutation(N_ITEM)[:9]]
    pairs += [(ONE_ROW, N_ITEM - 1)]
    for u in range(3, N_USER - 1):
        pairs += [(u, i) for i in rng.permutation(N_ITEM)[:int(rng.integers(2, 5))]]
    e = np.asarray(pairs, dtype=np.int64)[rng.permutation(len(pairs))]
    e[:, 1] += N_USER
    return e
