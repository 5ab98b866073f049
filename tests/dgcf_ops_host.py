"""Inputs and references shared by tests/test_dgcf_ops_host.py (CPU) and tests/test_gpu_dgcf_ops.py (GPU): one planted graph
with every kind of row the row kernel of csrc/dgcf.hip can meet, one seeded builder of x / P / z per (D, K), the 19 supported
(D, K) pairs, a numpy float32 emulation of the kernel's `acc` (bit for bit, and two WRONG variants the bit comparison must be
able to tell from it), the derived bound of the routing scores, and the case table of the distance correlation with its fp64
reference and the float32 emulation of the ordered scatter.  The fp64 references are those of tests/test_dgcf_host.py."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bpr_multi_host import GUARD, SENTINEL, U24, Guarded, bits  # noqa: E402,F401
from test_dgcf_host import distance_correlation, edge_operator, intent_propagate, routing_scores  # noqa: E402,F401


# ---- the planted graph ---------------------------------------------------------------------------------------------------
U, I = 37, 29                                     # U is no multiple of any RPW (1, 2, 4, 8, 16)
N = U + I
EMPTY_USERS = (0, 4, 6, 20, U - 1)                # rows without entries: the first, the last, the hub's two neighbours, one more
HUB = 5                                           # I - 1 entries between the empty rows 4 and 6
REPEAT_USERS = {9: 3, 12: 2}                      # user 9's first interaction occurs three times in train_data, user 12's twice
ZERO_ITEM, SLICE0_ITEM = 3, 7                     # x rows U + 3 (all zero) and U + 7 (slice 0 zero); both have edges (the hub's)

_PLANTED = {}


def planted():
    """-> dict(edges [E, 2] int32 (user, GLOBAL item id) shuffled, g = graph.dgcf_structure(...) on the CPU, E, repeats)."""
    if _PLANTED:
        return _PLANTED
    from chaorec_amd import graph
    rng = np.random.default_rng(3705)
    pairs = [(HUB, U + i) for i in range(I - 1)]              # the last item keeps no edge
    first_of = {}
    for u in range(U):
        if u in EMPTY_USERS or u == HUB:
            continue
        deg = int(rng.choice([1, 2, 3, 4], p=[0.1, 0.2, 0.3, 0.4]))
        items = rng.choice(I - 1, size=deg, replace=False)
        first_of[u] = (u, U + int(items[0]))
        pairs += [(u, U + int(i)) for i in items]
    repeats = {first_of[u]: times for u, times in REPEAT_USERS.items()}
    for pair, times in repeats.items():
        pairs += [pair] * (times - 1)
    e = np.asarray(pairs, dtype=np.int32)
    e = e[rng.permutation(len(e))]
    _PLANTED.update(edges=e, g=graph.dgcf_structure(e, U, N), E=len(e), repeats=repeats)
    return _PLANTED


# every (D, K) chaorec_dgcf_check_shape accepts with D >= 16: K in {1, 2, 4, 8}, D a power of two <= 256, D % (4 K) == 0
DK_GRID = [(D, K) for D in (16, 32, 64, 128, 256) for K in (1, 2, 4, 8) if D % (4 * K) == 0]


def dk_id(dk):
    return "D%d-K%d" % dk


_INPUTS = {}


def build_inputs(D, K):
    """Seeded float32 inputs of one (D, K) on the planted graph: x [N, D] = 0.1 * normal with item row ZERO_ITEM all zero and
    slice 0 of item row SLICE0_ITEM zero (normalize's max(norm, 1e-12)); P [E, K] = softmax(3 * normal); z [N, D] = normal."""
    if (D, K) not in _INPUTS:
        rng = np.random.default_rng([D, K])
        E = planted()["E"]
        x = (0.1 * rng.standard_normal((N, D))).astype(np.float32)
        x[U + ZERO_ITEM] = 0.0
        x[U + SLICE0_ITEM, :D // K] = 0.0
        s = 3.0 * rng.standard_normal((E, K))
        p = np.exp(s - s.max(1, keepdims=True))
        P = (p / p.sum(1, keepdims=True)).astype(np.float32)
        z = rng.standard_normal((N, D)).astype(np.float32)
        _INPUTS[(D, K)] = dict(x=x, P=P, z=z)
    return _INPUTS[(D, K)]


def propagate_f32(g, P, x, K, variant=None):
    """The `acc` of dgcf_rows_kernel in numpy float32, every row: entries ascending,
        w = f32(norm_e * P[eid_e, k]),   acc = f32(acc + f32(w * x[col_e]))        (k the slice of the column).
    variant = "norm_x_first": f32(f32(norm_e * x[col_e]) * P[eid_e, k]) -- the same real number, other bits;
    variant = "edge_major_p": slice k reads P as if it were stored [K, E] (element k * E + eid_e of the buffer).
    Both are mistakes a kernel could make; for K = 1 both ARE the defined computation (P is one column of ones)."""
    assert variant in (None, "norm_x_first", "edge_major_p")
    rowptr, col, val, eid = (np.asarray(t) for t in (g.rowptr, g.col, g.val, g.eid))
    P, x = np.ascontiguousarray(P, np.float32), np.ascontiguousarray(x, np.float32)
    n_rows, D = x.shape
    E, W = P.shape[0], D // K
    flat = P.reshape(-1)
    out = np.zeros((n_rows, D), np.float32)
    for r in range(n_rows):
        acc = np.zeros(D, np.float32)
        for e in range(int(rowptr[r]), int(rowptr[r + 1])):
            p = flat[np.arange(K) * E + eid[e]] if variant == "edge_major_p" else P[eid[e]]
            p, xv, nrm = np.repeat(p, W), x[col[e]], np.float32(val[e])
            term = (nrm * xv) * p if variant == "norm_x_first" else (nrm * p) * xv
            assert term.dtype == np.float32
            acc = acc + term
        out[r] = acc
    return out


def route_bound(W):
    """Absolute bound on S = P + score of the kernel against the fp64 routing_scores fed the SAME float32 acc and x, W = D / K
    columns per slice: (W + 16) 2^-23.  In units of u = 2^-24, on values bounded by 1:
      each normalise (W squares, W - 1 additions, sqrt, one division per element; the norm's relative error is halved by
                      the square root)                                               <= W/2 + 3   per element, two of them
      tanhf                                                                          <= 4
      the W-term dot of a unit vector with a vector of norm <= 1                     <= W
      the final add P + score                                                        <= 2
    in all (2 W + 12) u <= (W + 16) 2^-23.  P_next = softmax(S) gets route_bound(W) + 8 u: softmax is 1-Lipschitz in the max norm
    and expf, the K-term sum and the division add a few units on values <= 1."""
    return (W + 16) * 2.0 ** -23


def pnext_bound(W):
    return route_bound(W) + 8 * U24


def routing_ref(acc32, x, P, K):
    """fp64 S and P_next of every edge from the float32 acc (all N rows) and x: (P + routing_scores, its softmax), numpy."""
    et = torch.as_tensor(planted()["edges"]).long()
    S = torch.from_numpy(P).double() + routing_scores(torch.from_numpy(acc32).double(), torch.from_numpy(x).double(), et, K)
    return S.numpy(), torch.softmax(S, 1).numpy()


def sentinel(*shape):
    """A float32 array whose every word is SENTINEL (what an output buffer holds before a launch)."""
    return np.full(shape, SENTINEL, np.int32).view(np.float32)


# ---- distance correlation -------------------------------------------------------------------------------------------------
# (n, D, K, table rows, kind)
DCOR_CASES = [
    (1, 16, 2, 5, "random"),
    (2, 16, 4, 5, "random"),
    (15, 32, 8, 40, "random"),
    (16, 64, 8, 40, "random"),
    (17, 128, 4, 9, "random"),         # 9 table rows: heavy repeats
    (33, 256, 8, 50, "random"),
    (31, 256, 2, 50, "random"),
    (40, 16, 2, 7, "equal"),           # all idx equal
    (48, 64, 4, 50, "zero"),           # every second table row zero, slice 1 zero in every row
    (300, 32, 8, 100, "random"),
    (4112, 16, 2, 6000, "random"),     # 257 workgroups: the combine's second trip over the partials
]
DCOR_GRAD_OUT = 3.0


def dcor_id(case):
    return "n%d-D%d-K%d-rows%d-%s" % case


def dcor_grad_checked(case):
    """The cases whose gradient is held to the bar: n >= 15 and not `all idx equal` (there, and for n = 1, it is exactly 0;
    for n = 2 the reference gradient is ~1e-9 of the loss and only finiteness is asked)."""
    return case[0] >= 15 and case[4] != "equal"


_DCOR = {}


def build_dcor(case):
    """-> dict(table [rows, D] float32 = 0.3 * normal, idx [n] int64 = randint(rows)).  No near-duplicate rows that are not exact
    duplicates: r_i - 2 <x_i, x_j> + r_j cancels in float32 in every float reference too, which tests conditioning, not the kernel."""
    if case not in _DCOR:
        n, D, K, rows, kind = case
        rng = np.random.default_rng([n, D, K, rows])
        table = (0.3 * rng.standard_normal((rows, D))).astype(np.float32)
        idx = rng.integers(0, rows, n).astype(np.int64)
        if kind == "equal":
            idx[:] = 4
        if kind == "zero":
            W = D // K
            table[::2] = 0.0
            table[:, W:2 * W] = 0.0
        _DCOR[case] = dict(table=table, idx=idx)
    return _DCOR[case]


def dcor_loss_torch(x, K):
    """DGCF.cor_loss of the gathered rows x [n, D] (any dtype): sum of the K - 1 consecutive pairs / ((K + 1) K / 2)."""
    W = x.shape[1] // K
    total = sum(distance_correlation(x[:, k * W:(k + 1) * W], x[:, (k + 1) * W:(k + 2) * W]) for k in range(K - 1))
    return total / ((K + 1) * K / 2)


def dcor_ref64(case):
    """-> (loss, d loss / d table) in fp64, computed once per case and left unchanged."""
    c = build_dcor(case)
    if "ref" not in c:
        t = torch.from_numpy(c["table"]).double().requires_grad_(True)
        loss = dcor_loss_torch(t[torch.from_numpy(c["idx"])], case[2])
        loss.backward()
        c["ref"] = (float(loss.item()), t.grad.numpy().copy())
    return c["ref"]


def stable_sort(idx):
    """-> (sorted idx, perm) of a stable sort, int64: what chaorec_dgcf_dcor_bwd_f32 is handed."""
    perm = np.argsort(idx, kind="stable").astype(np.int64)
    return np.ascontiguousarray(idx[perm]), perm


def scatter_f32(grad_rows, idx, n_table_rows):
    """grad_table of dcor_scatter_kernel from the launch's own grad_rows, float32: row idx[p] = ((0 + g[p1]) + g[p2]) + ... over
    the gathered rows p1 < p2 < ... with that index (a stable sort's `perm` order); every other row +0."""
    out = np.zeros((n_table_rows, grad_rows.shape[1]), np.float32)
    for p in range(len(idx)):
        out[idx[p]] = out[idx[p]] + grad_rows[p]
    return out
