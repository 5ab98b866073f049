"""The references of the multi-term BPR launches, checked on the CPU before the GPU tests lean on them
(tests/test_gpu_bpr_multi.py): oracle.bpr_multi_fwd / bpr_multi_bwd (fp64) and oracle.bpr_multi_bwd_ordered (float, defined
order) against each other, against the single-term oracle, and against deliberately wrong orders of the same addends."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpr_multi_host as H  # noqa: E402

_CACHE = {}


def _case(oracle, case):
    """Inputs, the fp64 forward's coefficients rounded to float (what a launch would hand its backward), both backwards."""
    if case not in _CACHE:
        inp = H.build_case(case)
        _, _, coef64 = oracle.bpr_multi_fwd(inp["tab_u"], inp["users"], inp["tabs"], inp["pos"], inp["neg"], inp["variant"],
                                            inp["wvec"])
        coef = coef64.astype(np.float32)
        go = np.float32(H.GRAD_OUT)
        souts = None if inp["scatter_rows"] is None else [None if s is None else np.zeros_like(s) for s in inp["init_s"]]
        ordered = oracle.bpr_multi_bwd_ordered(inp["tab_u"], inp["users"], inp["tabs"], inp["pos"], inp["neg"], coef,
                                               inp["wvec"], go, scatter_rows=inp["scatter_rows"], scatter_out=souts)
        if ordered[2] is None:
            ordered = (ordered[0], ordered[1], [None] * inp["T"])
        exact = oracle.bpr_multi_bwd(inp["tab_u"], inp["users"], inp["tabs"], inp["pos"], inp["neg"], coef, inp["wvec"],
                                     float(go), inp["scatter_rows"], inp["scatter_sizes"])
        _CACHE[case] = (inp, coef, go, ordered, exact)
    return _CACHE[case]


def test_the_case_table_reaches_what_it_claims():
    """The geometry the GPU tests rely on, stated once: which cases the ordered launch takes, where its key table passes
    48 KiB, the exact slot limit, duplicated destinations everywhere, all users equal once, pos == neg in some samples."""
    assert [c for c in H.CASES if not H.is_ordered(c)] == [(1, 40, 260, 1), (4, 4097, 64, 1)]
    assert max(4, 2) * 4096 == H.ORD_MAX_SLOTS and 4 * 4097 > H.ORD_MAX_SLOTS
    assert 3 * 2049 * 8 == 49176 > 48 * 1024 >= 3 * 2048 * 8
    assert {D for T, B, D, _ in H.CASES if B == 2049} == {64, 128, 256}
    assert {T for T, *_ in H.CASES} == {1, 2, 3, 4} and {v for *_, v in H.CASES} == {0, 1, 2}
    assert any(T * B % 4 for T, B, _, _ in H.CASES)
    inp = H.build_case((2, 5, 16, 0))
    assert len(set(inp["users"])) == 1
    inp = H.build_case((3, 257, 64, 1))
    assert all((p == n).sum() >= 37 for p, n in zip(inp["pos"], inp["neg"]))
    assert [r is not None for r in inp["scatter_rows"]] == [False, True, True]
    assert np.bincount(inp["scatter_rows"][1], minlength=H.TABLE_ROWS).min() >= 2       # scatter targets repeat
    assert all(np.all(a != 0) for a in [inp["init_u"]] + inp["init_i"])


def test_one_term_is_the_single_term_oracle_bit_for_bit(oracle):
    """T = 1, separate tables, no scatter, w = 1: oracle_bpr_multi_bwd_ordered_f32 is oracle_bpr_bwd_ordered_f32 with
    reg_weight = 0 (user rows, then pos, then neg, batch order)."""
    rng = np.random.default_rng(7)
    for B, D in ((1, 4), (40, 260), (300, 64)):
        tu = (rng.standard_normal((H.U_ROWS, D)) * 0.3).astype(np.float32)
        ti = (rng.standard_normal((H.I_ROWS, D)) * 0.3).astype(np.float32)
        users, pos, neg = rng.integers(0, H.U_ROWS, B), rng.integers(0, H.I_ROWS, B), rng.integers(0, H.I_ROWS, B)
        coef = (-rng.random(B) / B).astype(np.float32)
        go = np.float32(0.7)
        one_u, one_i = oracle.bpr_bwd_ordered(tu, ti, users, pos, neg, coef, 0.0, grad_out=go)
        g_u, g_i, _ = oracle.bpr_multi_bwd_ordered(tu, users, [ti], [pos], [neg], coef, [1.0], go)
        assert np.array_equal(g_u.view(np.int32), one_u.view(np.int32))
        assert np.array_equal(g_i[0].view(np.int32), one_i.view(np.int32))
        assert np.abs(one_i).max() > 0


def test_the_ordered_oracle_adds_into_what_it_is_given(oracle):
    inp, coef, go, ordered, _ = _case(oracle, (3, 257, 64, 1))
    souts = [None if s is None else s.copy() for s in inp["init_s"]]
    g_u, g_i, g_s = oracle.bpr_multi_bwd_ordered(inp["tab_u"], inp["users"], inp["tabs"], inp["pos"], inp["neg"], coef,
                                                 inp["wvec"], go, g_u=inp["init_u"].copy(),
                                                 g_i=[g.copy() for g in inp["init_i"]], scatter_rows=inp["scatter_rows"],
                                                 scatter_out=souts)
    assert not np.array_equal(g_u, ordered[0])
    # a row nobody lands in keeps its bits; the others moved by the gradient
    idle = np.setdiff1d(np.arange(H.U_ROWS), inp["users"])
    assert len(idle) == 0 or np.array_equal(g_u[idle], inp["init_u"][idle])
    assert np.allclose(g_u - inp["init_u"], ordered[0], rtol=0, atol=1e-7)
    assert np.allclose(g_s[1] - inp["init_s"][1], ordered[2][1], rtol=0, atol=1e-7)


@pytest.mark.parametrize("case", H.CASES, ids=H.case_id)
def test_float_oracle_within_the_derived_bound_of_the_fp64_oracle(oracle, case):
    """Every buffer of oracle_bpr_multi_bwd_ordered_f32 within (n + 4) 2^-24 S of the fp64 index_add (bpr_multi_host.sum_bound),
    and the scattered rows equal to index_add of the fp64 item gradient through scatter_rows within the same bound."""
    inp, _, _, ordered, (g64, abs64, cnt) = _case(oracle, case)
    got, want, bound = H.flat(ordered), H.flat(g64), H.sum_bound(H.flat(abs64), H.flat(cnt))
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"{H.case_id(case)}: worst error / bound = {worst:.3f}")
    for k in range(inp["T"]):
        rows = None if inp["scatter_rows"] is None else inp["scatter_rows"][k]
        if rows is None:
            continue
        via_index_add = np.zeros((H.TABLE_ROWS, inp["D"]))
        np.add.at(via_index_add, rows, g64[1][k])
        assert np.allclose(via_index_add, g64[2][k], rtol=1e-12, atol=1e-18)
        err = np.abs(ordered[2][k].astype(np.float64) - via_index_add)
        assert np.all(err <= H.sum_bound(abs64[2][k], cnt[2][k]) + 1e-12 * np.abs(via_index_add))
    # ... and from the pre-filled buffers the GPU tests use, for both values of grad_out they use
    for go in (np.float32(H.GRAD_OUT), np.float32(1.0)):
        coef = _case(oracle, case)[1]
        souts = None if inp["scatter_rows"] is None else [None if s is None else s.copy() for s in inp["init_s"]]
        g = oracle.bpr_multi_bwd_ordered(inp["tab_u"], inp["users"], inp["tabs"], inp["pos"], inp["neg"], coef, inp["wvec"], go,
                                         g_u=inp["init_u"].copy(), g_i=[x.copy() for x in inp["init_i"]],
                                         scatter_rows=inp["scatter_rows"], scatter_out=souts)
        g = (g[0], g[1], g[2] if g[2] is not None else [None] * inp["T"])
        e64, a64, c64 = oracle.bpr_multi_bwd(inp["tab_u"], inp["users"], inp["tabs"], inp["pos"], inp["neg"], coef, inp["wvec"],
                                             float(go), inp["scatter_rows"], inp["scatter_sizes"])
        init = H.flat((inp["init_u"], inp["init_i"], inp["init_s"]))
        err = np.abs(H.flat(g).astype(np.float64) - (init.astype(np.float64) + H.flat(e64)))
        bound = H.sum_bound(H.flat(a64), H.flat(c64), init)
        print(f"{H.case_id(case)} pre-filled, grad_out {go}: worst error / bound = {float((err / bound).max()):.3f}")
        assert np.all(err <= bound)
    # the counts are the slots of each group
    assert cnt[0].sum() == inp["T"] * inp["B"] * inp["D"]
    assert all(c.sum() == 2 * inp["B"] * inp["D"] for c in cnt[1])


@pytest.mark.parametrize("case", [c for c in H.CASES if H.is_ordered(c)], ids=H.case_id)
def test_the_inputs_tell_the_defined_order_from_its_neighbours(oracle, case):
    """The C oracle is the numpy restatement of the defined order bit for bit, and the case's inputs separate that order from
    (a) negative slots before positive slots, (b) the user rows sample-major, (c) the fp64 sums rounded to float, (d) the
    term's weight applied after the sum -- so a kernel that made one of these mistakes could not pass the bit comparison.
    Where an alternative is the SAME computation it cannot differ and is not asked to: (a) and (b) reorder a sum, which
    needs three addends in one row (B >= 3; for (b) also T >= 2); (d) differs only for a weight that is not 1 (T >= 2)."""
    inp, coef, go, ordered, (g64, _, _) = _case(oracle, case)
    T, B = inp["T"], inp["B"]
    bits = lambda g: H.flat(g).view(np.int32)
    want = bits(ordered)
    assert np.array_equal(bits(H.ordered_numpy(inp, coef, go)), want)
    differ = lambda other: int((bits(other) != want).sum())
    if B >= 3:
        g = H.ordered_numpy(inp, coef, go, "neg_first")
        assert differ(g) > 0
        assert np.array_equal(g[0], ordered[0])                       # (the user rows have no such roles)
    if B >= 3 and T >= 2:
        g = H.ordered_numpy(inp, coef, go, "sample_major")
        assert (g[0].view(np.int32) != ordered[0].view(np.int32)).sum() > 0
    if T >= 2:
        g = H.ordered_numpy(inp, coef, go, "w_after")
        assert (g[0].view(np.int32) != ordered[0].view(np.int32)).sum() > 0       # the shared user rows
        assert (g[1][1].view(np.int32) != ordered[1][1].view(np.int32)).sum() > 0  # the table of the 1e-3 term
    rounded = (g64[0].astype(np.float32), [g.astype(np.float32) for g in g64[1]],
               [None if g is None else g.astype(np.float32) for g in g64[2]])
    assert differ(rounded) > 0
