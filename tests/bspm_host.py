"""BSPM on the host, in float64: the synthetic small case and two restatements of Model/BSPM.py:87-181 -- the reference's own
route over the full (U + I) x (U + I) adjacency, and the item-block route the kernels take (DESIGN: "BSPM").  Shared by
tests/golden/gen_bspm.py, tests/test_bspm_host.py and tests/test_gpu_bspm.py; numpy, and torch for the time grid alone."""
import os

import numpy as np
import torch
from accept import EPS32 as ULP, rel_dev, user_item_dict  # noqa: F401

U, FACTOR, TOPK, EMPTY_ITEMS = 70, 16, 50, 10
CASES = ((1, 1.0, 1.0), (2, 1.5, 0.7), (3, 1.0, 0.0))          # (K_s, T_s, idl_beta)
MASK = 1e-6
FIXTURE = "bspm_small.npz"


def num_items(long_row):
    """The case's item count: the full row of the item every user holds is longer than the kernel's long-row length."""
    return max(150, int(long_row) + EMPTY_ITEMS)


def small_case(I, seed):
    """Edges [E, 2] (global item ids) over U users and I items: item 0 held by every user with a history, the last user without
    one, the last EMPTY_ITEMS items without users, every other item held by someone."""
    rng = np.random.RandomState(seed)
    live = I - EMPTY_ITEMS
    rows = []
    for u in range(U - 1):
        own = set(rng.choice(np.arange(1, live), size=rng.randint(3, 13), replace=False).tolist()) | {0}
        own |= {k for k in range(1, live) if k % (U - 1) == u}
        rows += [(u, U + i) for i in sorted(own)]
    edges = np.asarray(rows, dtype=np.int64)
    return edges[rng.permutation(len(edges))]


def step_sizes(K_s, T_s):
    """The Euler steps of sharpening_times = linspace(0, T_s, K_s + 1).float() (:58), each the fp32 difference of two fp32 times."""
    t = torch.linspace(0, T_s, int(K_s) + 1).float()          # (torch's fp32 grid: 2/3 comes out one ulp above numpy's)
    return [float(x) for x in (t[1:] - t[:-1]).tolist()]


def degrees(edges, I):
    R = np.zeros((U, I))
    R[edges[:, 0], edges[:, 1] - U] = 1.0
    return R, np.power(R.sum(1) + 1e-7, -0.5), np.power(R.sum(0) + 1e-7, -0.5)


def normalised(edges, I):
    """Rn = D_U R D_I in float64, ((d_u * 1) * d_i as D @ A @ D forms it), with the two diagonals."""
    R, du, di = degrees(edges, I)
    return (du[:, None] * R) * di[None, :], du, di


def euler(Y0, P, K_s, T_s):
    Y = Y0
    for h in step_sizes(K_s, T_s):
        Y = Y + h * (-(Y @ P))
    return Y


def full_route(edges, I, K_s, T_s, beta, factor=FACTOR):
    """The reference's lines over N = U + I: -> (all_ratings [U, N], the top `factor` right singular vectors vt [factor, N])."""
    N = U + I
    Rn, du, di = normalised(edges, I)
    d = np.concatenate([du, di])
    L = np.zeros((N, N))
    L[:U, U:], L[U:, :U] = Rn, Rn.T
    P = L.T @ L
    vt = np.linalg.svd(L)[2][:factor]
    left, right = d[:, None] * vt.T, vt * (1.0 / d)[None, :]
    X = L[:U]
    return euler(beta * (X @ (left @ right)) + X @ P, P, K_s, T_s), vt


def item_factors(Rn, m):
    """The top m right singular vectors of Rn, [I, m], and the gap sigma_m - sigma_{m + 1} relative to sigma_1."""
    _, s, vt = np.linalg.svd(Rn, full_matrices=False)
    return vt[:m].T.copy(), float((s[m - 1] - s[m]) / s[0])


def item_route(edges, I, K_s, T_s, beta, Vi, P=None, X=None, parts=False):
    """The item-block route: Y0 = beta X (D_I Vi)(Vi^T D_I^-1) + X P_II, Euler over P_II -> [U, I].  P / X: given (rounded)
    operands instead of the float64 ones.  parts: also (Z, Y0, the state before the last step)."""
    Rn, _, di = normalised(edges, I)
    P = Rn.T @ Rn if P is None else np.asarray(P, np.float64)
    X = Rn if X is None else np.asarray(X, np.float64)
    Vi = np.asarray(Vi, np.float64)
    Z = X @ (di[:, None] * Vi)
    Y0 = beta * (Z @ (Vi.T * (1.0 / di)[None, :])) + X @ P
    hs = step_sizes(K_s, T_s)
    Y = Y0
    for h in hs[:-1]:
        Y = Y + h * (-(Y @ P))
    out = Y + hs[-1] * (-(Y @ P))
    return (out, Z, Y0, Y) if parts else out


def masked(scores, edges):
    s = np.array(scores, copy=True)
    s[edges[:, 0], edges[:, 1] - U] = MASK
    return s


def top_lists(scores, k=TOPK):
    """Exact top-k per row, ties to the lowest index -> (ids [U, k], values)."""
    idx = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(scores, idx, 1)


def load_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, FIXTURE), allow_pickle=False)
