"""What tests/test_gpu_dgcf_ops.py leans on, checked on the CPU first: the planted graph has the rows it claims, the float32
emulation of the row kernel's `acc` agrees with the fp64 restatement and differs in bits from two plausible mistakes, the float32
torch routing meets the derived bound, dgcf_p_schedule never hands a launch a buffer another reader still needs, and the float32
distance correlation meets the loss bar (and why it is NOT the measure of the gradient bar)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgcf_ops_host as H  # noqa: E402


def test_the_planted_graph_has_every_row_kind():
    pl = H.planted()
    e, g, E = pl["edges"], pl["g"], pl["E"]
    assert (H.U, H.I) == (37, 29) and 100 <= E <= 140
    assert all(H.U % rpw for rpw in (2, 4, 8, 16))
    deg = np.diff(np.asarray(g.rowptr))
    assert len(deg) == H.N and deg.sum() == 2 * E
    assert H.EMPTY_USERS == (0, 4, 6, 20, H.U - 1) and all(deg[u] == 0 for u in H.EMPTY_USERS)
    assert deg[H.N - 1] == 0                                            # the last item
    # the hub: every item but the last, once each, between two empty rows
    assert deg[H.HUB] == H.I - 1 and deg[H.HUB - 1] == 0 and deg[H.HUB + 1] == 0
    assert set(e[e[:, 0] == H.HUB, 1]) == set(range(H.U, H.N - 1))
    # the other users: 1 .. 4 interactions (the copies of a repeated one are further entries of the row)
    others = [u for u in range(H.U) if u != H.HUB and u not in H.EMPTY_USERS]
    extra = lambda u: H.REPEAT_USERS.get(u, 1) - 1  # noqa: E731
    assert all(1 <= deg[u] - extra(u) <= 4 for u in others) and {int(deg[u] - extra(u)) for u in others} == {1, 2, 3, 4}
    # two interactions occur more than once: distinct edges with distinct eid's, the same (row, col)
    pairs, counts = np.unique(e, axis=0, return_counts=True)
    assert sorted(counts[counts > 1]) == [2, 3] and sorted(pl["repeats"].values()) == [2, 3]
    eid, col, rowptr = np.asarray(g.eid), np.asarray(g.col), np.asarray(g.rowptr)
    for (u, i), times in pl["repeats"].items():
        seg = slice(rowptr[u], rowptr[u + 1])
        copies = eid[seg][col[seg] == i]
        assert len(copies) == times == len(set(copies)) and np.all(np.diff(copies) > 0)
    # every item row but the last has entries (so the zero rows of x are read), and the edge list is not in user order
    assert np.all(deg[H.U:H.N - 1] >= 1) and deg[H.U + H.ZERO_ITEM] >= 1 and deg[H.U + H.SLICE0_ITEM] >= 1
    assert np.any(np.diff(e[:, 0]) < 0) and not np.array_equal(e, e[np.lexsort((e[:, 1], e[:, 0]))])
    # row 14 lies strictly inside a wave's row group counted from row_begin = 3 for every RPW > 1
    assert all((14 - 3) % rpw for rpw in (2, 4, 8, 16))
    assert len(H.DK_GRID) == 19 and all(D >= 16 for D, _ in H.DK_GRID)


def test_the_input_builder_plants_its_zero_rows():
    for D, K in ((16, 4), (256, 1), (64, 8)):
        inp = H.build_inputs(D, K)
        x, P = inp["x"], inp["P"]
        assert x.dtype == P.dtype == np.float32 and x.shape == (H.N, D) and P.shape == (H.planted()["E"], K)
        assert not x[H.U + H.ZERO_ITEM].any()
        assert not x[H.U + H.SLICE0_ITEM, :D // K].any() and (K == 1 or x[H.U + H.SLICE0_ITEM, D // K:].all())
        assert np.abs(P.sum(1) - 1).max() <= K * H.U24 and (K == 1 or P.min() < 0.01)
        assert H.build_inputs(D, K) is inp


@pytest.mark.parametrize("dk", H.DK_GRID, ids=H.dk_id)
def test_propagate_emulation_against_fp64_and_against_its_wrong_variants(dk):
    """propagate_f32 within deg_max 2^-22 max|term| of intent_propagate in fp64 (two roundings per term and the running sum; here
    about 2e-8).  For K > 1 both wrong variants differ from it in bits, and the [K, E] reading of P by far more than the routing
    bound: a kernel that made either mistake could not pass the bit comparison of the GPU test."""
    D, K = dk
    pl, inp = H.planted(), H.build_inputs(D, K)
    g, x, P = pl["g"], inp["x"], inp["P"]
    acc = H.propagate_f32(g, P, x, K)
    et, src, dst, base = H.edge_operator(pl["edges"], H.N)
    x64, P64 = torch.from_numpy(x).double(), torch.from_numpy(P).double()
    y64 = H.intent_propagate(x64, P64, src, dst, base).numpy()
    term = ((base[:, None] * torch.cat([P64, P64])).repeat_interleave(D // K, dim=1) * x64[src]).abs().max().item()
    deg_max = int(np.diff(np.asarray(g.rowptr)).max())
    err = np.abs(acc.astype(np.float64) - y64).max()
    print(f"{H.dk_id(dk)}: |propagate_f32 - fp64| = {err:.2e}, bound {deg_max * 2.0 ** -22 * term:.2e}")
    assert err <= deg_max * 2.0 ** -22 * term and np.abs(y64).max() > 1e-3
    empty = [u for u in H.EMPTY_USERS] + [H.N - 1]
    assert not acc[empty].any()
    if K == 1:
        for v in ("norm_x_first", "edge_major_p"):
            assert np.array_equal(H.bits(H.propagate_f32(g, P, x, K, v)), H.bits(acc))
        return
    swapped = H.propagate_f32(g, P, x, K, "norm_x_first")
    assert (H.bits(swapped) != H.bits(acc)).sum() > 0
    assert np.abs(swapped.astype(np.float64) - y64).max() <= deg_max * 2.0 ** -22 * term      # (the same real number)
    edge_major = H.propagate_f32(g, P, x, K, "edge_major_p")
    assert (H.bits(edge_major) != H.bits(acc)).sum() > 0
    assert np.abs(edge_major - acc).max() > 100 * H.route_bound(D // K)


@pytest.mark.parametrize("dk", H.DK_GRID, ids=H.dk_id)
def test_float32_routing_meets_the_derived_bound(dk):
    """The float32 torch run of routing_scores on the float32 acc, P + score and its softmax, against the fp64 run on the same
    inputs: within route_bound(W) / pnext_bound(W) on every edge of the planted graph (the zero rows of x included)."""
    D, K = dk
    pl, inp = H.planted(), H.build_inputs(D, K)
    acc = H.propagate_f32(pl["g"], inp["P"], inp["x"], K)
    S64, Pn64 = H.routing_ref(acc, inp["x"], inp["P"], K)
    et = torch.as_tensor(pl["edges"]).long()
    S32 = torch.from_numpy(inp["P"]) + H.routing_scores(torch.from_numpy(acc), torch.from_numpy(inp["x"]), et, K)
    assert S32.dtype == torch.float32
    dS = np.abs(S32.double().numpy() - S64).max()
    dP = np.abs(torch.softmax(S32, 1).double().numpy() - Pn64).max()
    W = D // K
    print(f"{H.dk_id(dk)}: dS / bound = {dS / H.route_bound(W):.3f}, dP / bound = {dP / H.pnext_bound(W):.3f}")
    assert dS <= H.route_bound(W) and dP <= H.pnext_bound(W)
    assert np.abs(S64 - inp["P"]).max() > 0.1            # the scores are not all small: the bound is not met by a zero score


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_p_schedule_never_overwrites_what_is_still_read(L, T):
    from chaorec_amd.ops_dgcf import dgcf_p_schedule
    src, dst = dgcf_p_schedule(L, T)
    LT = L * T
    assert len(src) == len(dst) == LT
    assert all(src[j] != dst[j] for j in range(LT))
    assert all(src[j + 1] == dst[j] for j in range(LT - 1))
    assert dst[-1] == "state"
    assert src[0] == ("state" if T > 1 else ("saved", 0))
    names = {"state"} | {("saved", l) for l in range(L)} | {("scratch", i) for i in range(min(2, max(T - 1, 0)))}
    assert set(src) | set(dst) <= names                   # only the buffers dgcf_forward_raw allocates
    for l in range(L):
        last = l * T + T - 1
        assert src[last] == ("saved", l)
        assert all(dst[j] != ("saved", l) for j in range(last, LT))           # the backward reads it after the forward
    # a scratch buffer is never read after a later launch wrote it: the last write before launch j's read is launch j - 1's
    for j in range(1, LT):
        if src[j][0] == "scratch":
            assert max(i for i in range(j) if dst[i] == src[j]) == j - 1
    # ... and the same, by running the schedule on version numbers: launch j reads P_j and writes P_{j+1}
    held = {src[0]: 0}
    for j in range(LT):
        assert held.get(src[j]) == j, (j, src[j])
        held[dst[j]] = j + 1
    assert held["state"] == LT
    assert all(held[("saved", l)] == l * T + T - 1 for l in range(L))


@pytest.mark.parametrize("case", H.DCOR_CASES, ids=H.dcor_id)
def test_float32_distance_correlation_meets_the_loss_bar(case):
    """The float32 run of the restatement is within 1e-5 max(1, |ref|) of the fp64 loss on every case (measured: at most 2.8e-6).

    It does NOT meet the gradient bar 1e-3 max|ref grad| the kernel is held to: its gradient error reaches 4.1e-3 of the scale at
    (300, 32, 8) and 3.3e-3 at (31, 256, 2).  float32 torch computes a noisy q_ii = r_i - 2 <x_i, x_i> + r_i on the diagonal (and
    on exact duplicates) and divides by a_ii of about 1e-4.  The kernel forms the gather's r and the tile's dot with the same
    fmaf order, so its diagonal q is exactly 0 (no gradient) and its x_i - x_j is exactly 0: that is why the kernel is held to
    the bar and this restatement is not.  The figures are printed, not asserted."""
    n, D, K, rows, kind = case
    c = H.build_dcor(case)
    ref, gref = H.dcor_ref64(case)
    assert c["idx"].shape == (n,) and c["table"].shape == (rows, D) and 0 <= c["idx"].min() and c["idx"].max() < rows
    if kind == "equal":
        assert len(set(c["idx"])) == 1
    if kind == "zero":
        assert not c["table"][::2].any() and not c["table"][:, D // K:2 * D // K].any() and c["table"][1::2, :D // K].all()
    if rows == 9:
        assert np.bincount(c["idx"], minlength=rows).max() >= 3
    t = torch.from_numpy(c["table"]).clone().requires_grad_(True)
    loss = H.dcor_loss_torch(t[torch.from_numpy(c["idx"])], K)
    assert loss.dtype == torch.float32
    loss.backward()
    err = abs(float(loss.item()) - ref)
    scale = float(np.abs(gref).max())
    gerr = float(np.abs(t.grad.double().numpy() - gref).max())
    print(f"{H.dcor_id(case)}: float32 loss error {err:.2e} (bar {1e-5 * max(1.0, abs(ref)):.1e}); "
          f"gradient error / scale = {gerr / max(scale, 1e-300):.2e}, scale {scale:.2e}")
    assert np.isfinite(ref) and err <= 1e-5 * max(1.0, abs(ref))
    if n == 1 or kind == "equal":
        assert scale == 0.0
    if H.dcor_grad_checked(case):
        assert scale > 1e-6


def test_scatter_emulation_is_the_ordered_sum():
    """scatter_f32 adds the rows of one index in gathered order from +0, leaves the other rows +0, and a stable sort's perm is
    that order."""
    rng = np.random.default_rng(5)
    idx = np.array([3, 1, 3, 3, 0, 1], np.int64)
    g = rng.standard_normal((6, 4)).astype(np.float32) * np.float32(1e3) ** rng.integers(-2, 3, (6, 1)).astype(np.float32)
    out = H.scatter_f32(g, idx, 5)
    assert np.array_equal(H.bits(out[3]), H.bits((g[0] + g[2]) + g[3])) and np.array_equal(H.bits(out[1]), H.bits(g[1] + g[5]))
    assert np.array_equal(H.bits(out[0]), H.bits(g[4])) and not H.bits(out[[2, 4]]).any()
    s, perm = H.stable_sort(idx)
    assert list(s) == [0, 1, 1, 3, 3, 3] and list(perm) == [4, 1, 5, 0, 2, 3]
