"""The multi-term BPR launches (FREEDOM's loss: chaorec_bpr_multi_fwd_f32 / _bwd_f32 / _bwd_ordered_f32, csrc/bpr.hip) against
an independent reference, through the C ABI, at every shape at which the code takes another path:

  T B    D   variant   reaches
  1 1    4   1         one wave, one sample
  2 5    16  0         T B = 10: idle waves behind `k >= A.T`; a partial 16-slot workgroup of the ordered launch; all users equal
  3 257  64  1         FREEDOM's form: terms 1, 2 gathered + scattered, term 0 not (an empty group between live ones); <1>
  4 300  128 2         T = 4 (nine groups), bpr_bwd_ordered_kernel<2>
  3 100  192 1         <4> with the quarter lane + 192 >= D masked
  2 64   256 0         <4> full
  1 40   260 1         D > 256: the ordered entry falls back to the atomic launch
  3 2049 64/128/256 1  49 176 B of keys: the dynamic-LDS opt-in of <1>, <2>, <4>
  4 4096 64  1         exactly kOrdMaxSlots = 16 384 slots (128 KiB of keys)
  4 4097 64  1         the first size past it: atomic fallback

each with grad_out a device scalar 0.7 and NULL, weights (1, 1e-3, 0, -0.37), gradient buffers that already hold values and lie
between guard words.  The references are oracle.bpr_multi_fwd / bpr_multi_bwd (fp64) and oracle.bpr_multi_bwd_ordered (float,
the defined order; tests/test_bpr_multi_host.py shows that these inputs tell it from its neighbours).  The backwards are fed
the coefficients the forward launch left, so each is compared alone."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpr_multi_host as H  # noqa: E402
from accept import lib as _lib, ptr as _ptr, ptrs as _ptrs, stream as _stream  # noqa: E402

pytestmark = pytest.mark.gpu

Guarded = H.Guarded
GRAD_OUTS = [pytest.param(H.GRAD_OUT, id="go0.7"), pytest.param(None, id="goNULL")]
INVALID = r"failed \(-1\)"     # CHAOREC_E_INVALID as the binding raises it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from chaorec_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


_bits = H.bits


class State:
    pass


_STATES = {}


def _state(dev, case):
    """The case's inputs on the device and ONE multi-term forward launch over them (shared by every test of the case)."""
    if case in _STATES:
        return _STATES[case]
    st = State()
    st.inp = inp = H.build_case(case)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    T, B, D = inp["T"], inp["B"], inp["D"]
    st.tab_u, st.users, st.wvec = up(inp["tab_u"]), up(inp["users"].astype(np.int64)), up(inp["wvec"])
    st.tabs, st.pos, st.neg = [up(t) for t in inp["tabs"]], [up(p) for p in inp["pos"]], [up(n) for n in inp["neg"]]
    st.srows = None if inp["scatter_rows"] is None else [up(None if r is None else r.astype(np.int64)) for r in inp["scatter_rows"]]
    st.losses = torch.full((T,), float("nan"), device=dev)
    st.total = torch.full((1,), float("nan"), device=dev)
    st.coef = torch.full((T, B), float("nan"), device=dev)
    st.ws = torch.empty(4 * B * T, device=dev)
    _lib().chaorec_bpr_multi_fwd_f32(_ptr(st.tab_u), _ptr(st.users), T, _ptrs(st.tabs), _ptrs(st.pos), _ptrs(st.neg), B, D,
                                     inp["variant"], _ptr(st.wvec), _ptr(st.losses), _ptr(st.total), _ptr(st.coef), _ptr(st.ws),
                                     _stream())
    torch.cuda.synchronize()
    st.coef_np = st.coef.cpu().numpy()
    st.go_dev = torch.tensor([H.GRAD_OUT], dtype=torch.float32, device=dev)
    st.exact = {}
    _STATES[case] = st
    return st


def _backward(dev, st, name, go):
    """One backward launch `name` into pre-filled, guarded buffers -> (g_u, [g_i], [scattered or None])."""
    inp = st.inp
    T = inp["T"]
    inits = [inp["init_u"]] + inp["init_i"] + [s for s in inp["init_s"] if s is not None]
    buf = Guarded(dev, inits)
    g_u, g_i, rest = buf.views[0], buf.views[1:1 + T], list(buf.views[1 + T:])
    souts = None if st.srows is None else [None if r is None else rest.pop(0) for r in st.srows]
    getattr(_lib(), name)(_ptr(st.tab_u), _ptr(st.users), T, _ptrs(st.tabs), _ptrs(st.pos), _ptrs(st.neg), inp["B"], inp["D"],
                          _ptr(st.coef), _ptr(st.wvec), _ptr(st.go_dev if go is not None else None), _ptr(g_u), _ptrs(g_i),
                          None if st.srows is None else _ptrs(st.srows), None if souts is None else _ptrs(souts), _stream())
    torch.cuda.synchronize()
    out = buf.read()
    got_s, rest = [], out[1 + T:]
    for k in range(T):
        got_s.append(rest.pop(0) if inp["init_s"][k] is not None else None)
    return out[0], out[1:1 + T], got_s


def _initial(inp):
    return inp["init_u"], inp["init_i"], inp["init_s"]


def _assert_within_bound(st, got, go, what):
    """|got - (initial + fp64 gradient)| <= (n + 4) 2^-24 S + |initial| 2^-24 per element (bpr_multi_host.sum_bound), the fp64
    gradient formed from the launch's own float coefficients; an element no sample lands in keeps its bits."""
    inp = st.inp
    if go not in st.exact:
        st.exact[go] = oracle_mod().bpr_multi_bwd(inp["tab_u"], inp["users"], inp["tabs"], inp["pos"], inp["neg"], st.coef_np,
                                                  inp["wvec"], float(np.float32(go if go is not None else 1.0)),
                                                  inp["scatter_rows"], inp["scatter_sizes"])
    g64, abs64, cnt = (H.flat(x) for x in st.exact[go])
    init, got = H.flat(_initial(inp)), H.flat(got)
    err = np.abs(got.astype(np.float64) - (init.astype(np.float64) + g64))
    bound = H.sum_bound(abs64, cnt, init)
    ratio = float((err / bound).max())
    print(f"{what} {H.case_id(inp['case'])} grad_out={go}: worst error / bound = {ratio:.3f}")
    assert np.all(err <= bound), ratio
    idle = cnt == 0
    assert np.array_equal(got[idle].view(np.int32), init[idle].view(np.int32))
    assert np.abs(g64).max() > 0


def oracle_mod():
    from oracle import oracle as o
    return o


@pytest.mark.parametrize("case", H.CASES, ids=H.case_id)
def test_forward_is_the_single_term_launch_per_term_and_the_stated_weighted_sum(dev, oracle, case):
    """losses[k], coef[k] bit-identical to chaorec_bpr_fwd_f32 (reg_weight 0) on term k; out_total bit-identical to
    ((w0 l0 + w1 l1) + w2 l2) + ... in float32 from the launch's own losses; losses and coef against the fp64 oracle to the
    tolerances the single-term launch is held to (rtol 3e-6 / atol 1e-8, rtol 2e-5)."""
    st = _state(dev, case)
    inp = st.inp
    T, B, D = inp["T"], inp["B"], inp["D"]
    losses, total = st.losses.cpu().numpy(), st.total.cpu().numpy()
    assert np.all(np.isfinite(losses)) and np.all(np.isfinite(st.coef_np)) and np.isfinite(total[0])
    out, coef1, ws1 = torch.empty(3, device=dev), torch.empty(B, device=dev), torch.empty(4 * B, device=dev)
    for k in range(T):
        _lib().chaorec_bpr_fwd_f32(_ptr(st.tab_u), _ptr(st.tabs[k]), _ptr(st.users), _ptr(st.pos[k]), _ptr(st.neg[k]), B, D,
                                   inp["variant"], 0.0, _ptr(out), None, _ptr(coef1), _ptr(ws1), _stream())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()[1:2]), _bits(losses[k:k + 1])), k
        assert np.array_equal(_bits(coef1.cpu().numpy()), _bits(st.coef_np[k])), k
    w = inp["wvec"]
    want = np.float32(losses[0] * w[0])
    for k in range(1, T):
        want = np.float32(want + np.float32(losses[k] * w[k]))
    assert _bits(total)[0] == _bits(want).ravel()[0], (total, want)
    total64, losses64, coef64 = oracle.bpr_multi_fwd(inp["tab_u"], inp["users"], inp["tabs"], inp["pos"], inp["neg"],
                                                     inp["variant"], inp["wvec"])
    print(f"fwd {H.case_id(case)}: loss rel err {np.abs(losses / losses64 - 1).max():.2e}, "
          f"coef rel err {np.abs(st.coef_np / coef64 - 1).max():.2e}")
    assert np.allclose(losses, losses64, rtol=3e-6, atol=1e-8)
    assert np.allclose(total[0], total64, rtol=3e-6, atol=1e-8)
    assert np.allclose(st.coef_np, coef64, rtol=2e-5, atol=0)


@pytest.mark.parametrize("go", GRAD_OUTS)
@pytest.mark.parametrize("case", [c for c in H.CASES if H.is_ordered(c)], ids=H.case_id)
def test_ordered_backward_is_the_defined_order_bit_for_bit(dev, oracle, case, go):
    """g_u, every g_i[k] and every scatter_out[k] of chaorec_bpr_multi_bwd_ordered_f32 have the bits of
    oracle_bpr_multi_bwd_ordered_f32 fed the launch's own coefficients and the same pre-filled buffers; rows no sample lands in
    and the guard words around the buffers keep theirs; a second launch gives the same bits."""
    st = _state(dev, case)
    inp = st.inp
    first = _backward(dev, st, "chaorec_bpr_multi_bwd_ordered_f32", go)
    souts = None if inp["scatter_rows"] is None else [None if s is None else s.copy() for s in inp["init_s"]]
    w_u, w_i, w_s = oracle.bpr_multi_bwd_ordered(inp["tab_u"], inp["users"], inp["tabs"], inp["pos"], inp["neg"], st.coef_np,
                                                 inp["wvec"], np.float32(go if go is not None else 1.0),
                                                 g_u=inp["init_u"].copy(), g_i=[g.copy() for g in inp["init_i"]],
                                                 scatter_rows=inp["scatter_rows"], scatter_out=souts)
    want = (w_u, w_i, w_s if w_s is not None else [None] * inp["T"])
    diff = _bits(H.flat(first)) != _bits(H.flat(want))
    assert not diff.any(), (int(diff.sum()), float(np.abs(H.flat(first) - H.flat(want)).max()))
    assert not np.array_equal(_bits(H.flat(first)), _bits(H.flat(_initial(inp))))
    again = _backward(dev, st, "chaorec_bpr_multi_bwd_ordered_f32", go)
    assert np.array_equal(_bits(H.flat(again)), _bits(H.flat(first)))
    _assert_within_bound(st, first, go, "ordered")


@pytest.mark.parametrize("go", GRAD_OUTS)
@pytest.mark.parametrize("case", H.CASES, ids=H.case_id)
def test_atomic_backward_within_the_derived_bound_of_fp64(dev, oracle, case, go):
    """chaorec_bpr_multi_bwd_f32 (atomic row adds, any order): every element within (n + 4) 2^-24 S + |initial| 2^-24 of the fp64
    index_add -- n addends of total magnitude S, at most four roundings each, n - 1 float additions.  A missing, doubled or
    unweighted addend exceeds this by orders of magnitude."""
    st = _state(dev, case)
    _assert_within_bound(st, _backward(dev, st, "chaorec_bpr_multi_bwd_f32", go), go, "atomic")


@pytest.mark.parametrize("go", GRAD_OUTS)
@pytest.mark.parametrize("case", [c for c in H.CASES if not H.is_ordered(c)], ids=H.case_id)
def test_ordered_entry_falls_back_to_the_atomic_launch_past_its_limits(dev, oracle, case, go):
    """D = 260 > 256 and T B = 16 388 > 16 384 slots: chaorec_bpr_multi_bwd_ordered_f32 hands the call to the atomic launch;
    the sums are complete (same bound), nothing is written outside the buffers."""
    st = _state(dev, case)
    _assert_within_bound(st, _backward(dev, st, "chaorec_bpr_multi_bwd_ordered_f32", go), go, "fallback")


def test_argument_checks_launch_nothing(dev):
    """CHAOREC_E_INVALID for T = 0, T = 5, a term with one of scatter_rows / scatter_out, one of the two arrays, variant 3 and
    B = 0 -- and the gradient buffers untouched afterwards."""
    st = _state(dev, (3, 257, 64, 1))
    inp = st.inp
    T, B, D = inp["T"], inp["B"], inp["D"]
    lib = _lib()
    buf = Guarded(dev, [inp["init_u"]] + inp["init_i"] + [s for s in inp["init_s"] if s is not None])
    g_u, g_i, s1, s2 = buf.views[0], buf.views[1:1 + T], buf.views[1 + T], buf.views[2 + T]
    srows, souts = _ptrs(st.srows), _ptrs([None, s1, s2])

    def fwd(T_=T, B_=B, variant=1):
        lib.chaorec_bpr_multi_fwd_f32(_ptr(st.tab_u), _ptr(st.users), T_, _ptrs(st.tabs), _ptrs(st.pos), _ptrs(st.neg), B_, D,
                                      variant, _ptr(st.wvec), _ptr(st.losses), _ptr(st.total), _ptr(st.coef), _ptr(st.ws), _stream())

    def bwd(name, T_=T, B_=B, rows=srows, outs=souts):
        getattr(lib, name)(_ptr(st.tab_u), _ptr(st.users), T_, _ptrs(st.tabs), _ptrs(st.pos), _ptrs(st.neg), B_, D, _ptr(st.coef),
                           _ptr(st.wvec), None, _ptr(g_u), _ptrs(g_i), rows, outs, _stream())

    before = (st.losses.clone(), st.total.clone(), st.coef.clone())
    for kw in (dict(T_=0), dict(T_=5), dict(variant=3), dict(variant=-1), dict(B_=0)):
        with pytest.raises(RuntimeError, match=INVALID):
            fwd(**kw)
    for name in ("chaorec_bpr_multi_bwd_f32", "chaorec_bpr_multi_bwd_ordered_f32"):
        for kw in (dict(T_=0), dict(T_=5), dict(B_=0), dict(rows=None), dict(outs=None),
                   dict(outs=_ptrs([None, s1, None])), dict(rows=_ptrs([None, None, st.srows[2]]))):
            with pytest.raises(RuntimeError, match=INVALID):
                bwd(name, **kw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (st.losses, st.total, st.coef)))
    got = buf.read()
    for a, b in zip(got, [inp["init_u"]] + inp["init_i"] + [s for s in inp["init_s"] if s is not None]):
        assert np.array_equal(_bits(a), _bits(b))


def test_ops_path_hands_the_scattered_rows_to_linear_rows(dev, oracle):
    """ops.bpr_loss_multi over ops.linear_rows (FREEDOM.loss): the gradients of the user and item tables have the bits of the
    ordered oracle; the scattered [rows, D] gradient reaches linear_rows' backward through its token (put once, taken once),
    so the feature table's gradient is (oracle's scattered rows) W within the float dot-product bound (D + 1) 2^-24 |S| |W|."""
    from chaorec_amd import ops
    assert ops.BPR_ORDERED
    rng = np.random.default_rng(11)
    B, D, Kt = 96, 64, 32
    f32 = lambda *s: (rng.standard_normal(s) * 0.3).astype(np.float32)
    tu, ti, table, W, bias = f32(H.U_ROWS, D), f32(H.I_ROWS, D), f32(H.TABLE_ROWS, Kt), f32(D, Kt), f32(D)
    users, pos, neg = rng.integers(0, H.U_ROWS, B), rng.integers(0, H.I_ROWS, B), rng.integers(0, H.I_ROWS, B)
    rows = rng.integers(0, H.TABLE_ROWS, 2 * B)
    up = lambda a: torch.from_numpy(a).to(dev)
    a, b, tab, w, bs = (up(x).requires_grad_(True) for x in (tu, ti, table, W, bias))
    rows_d, idx = up(rows), torch.arange(B, device=dev)
    proj = ops.linear_rows(tab, rows_d, w, bs)
    token = proj._chaorec_row_scatter
    wvec = np.asarray([1.0, 1e-3], np.float32)
    loss = ops.bpr_loss_multi(a, up(users), ops.VARIANT_LOGSIGMOID, [(b, up(pos), up(neg)), (proj, idx, idx + B)], up(wvec),
                              gathered=[None, (rows_d, H.TABLE_ROWS)])
    coef = loss.grad_fn.saved_tensors[2].cpu().numpy()
    (loss * 0.7).backward()
    torch.cuda.synchronize()
    assert token.puts == token.hits == 1 and token._held is None
    ids = np.arange(B, dtype=np.int64)
    g_u, g_i, g_s = oracle.bpr_multi_bwd_ordered(tu, users, [ti, proj.detach().cpu().numpy()], [pos, ids], [neg, ids + B], coef,
                                                 wvec, np.float32(0.7), scatter_rows=[None, rows],
                                                 scatter_out=[None, np.zeros((H.TABLE_ROWS, D), np.float32)])
    assert np.array_equal(_bits(a.grad.cpu().numpy()), _bits(g_u))
    assert np.array_equal(_bits(b.grad.cpu().numpy()), _bits(g_i[0]))
    want = g_s[1].astype(np.float64) @ W.astype(np.float64)
    bound = (D + 1) * H.U24 * (np.abs(g_s[1]).astype(np.float64) @ np.abs(W).astype(np.float64))
    assert np.all(np.abs(tab.grad.cpu().numpy() - want) <= bound) and np.abs(want).max() > 0


# ---- the single-term ordered launch: the two paths tests/test_gpu_round6.py does not run -------------------------------
def _single(dev, B, D, joined, go=0.7, reg=1e-3):
    rng = np.random.default_rng([B, D, int(joined)])
    U, I = H.U_ROWS, H.I_ROWS
    tab = (rng.standard_normal((U + I, D)) * 0.3).astype(np.float32)
    users, pos, neg = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    neg[::7] = pos[::7]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t, ids = up(tab), [up(x) for x in (users, pos, neg)]
    tab_i = ctypes.c_void_p(t.data_ptr() + U * D * 4)
    out, coef, ws = torch.empty(3, device=dev), torch.empty(B, device=dev), torch.empty(4 * B, device=dev)
    lib = _lib()
    lib.chaorec_bpr_fwd_f32(_ptr(t), tab_i, *[_ptr(x) for x in ids], B, D, 0, reg, _ptr(out), None, _ptr(coef), _ptr(ws), _stream())
    buf = Guarded(dev, [np.zeros((U + I, D), np.float32)] if joined else [np.zeros((U, D), np.float32), np.zeros((I, D), np.float32)])
    g_u = buf.views[0]
    g_i = ctypes.c_void_p(g_u.data_ptr() + U * D * 4) if joined else _ptr(buf.views[1])
    go_dev = torch.tensor([go], dtype=torch.float32, device=dev)
    lib.chaorec_bpr_bwd_ordered_f32(_ptr(t), tab_i, *[_ptr(x) for x in ids], B, D, _ptr(coef), reg, _ptr(go_dev), _ptr(g_u), g_i,
                                    _stream())
    torch.cuda.synchronize()
    return tab, users, pos, neg, coef.cpu().numpy(), np.concatenate(buf.read())


@pytest.mark.parametrize("D", [128, 256])
def test_single_term_ordered_launch_opts_into_large_lds_for_wide_rows(dev, oracle, D):
    """One joined table, B = 2100: 3 B = 6300 slots = 50 400 B of keys, the hipFuncSetAttribute of bpr_bwd_ordered_kernel<2>
    (D = 128) and <4> (D = 256); bit-identical to oracle_bpr_bwd_ordered_f32."""
    tab, users, pos, neg, coef, got = _single(dev, 2100, D, joined=True)
    want, _ = oracle.bpr_bwd_ordered(tab, None, users, pos, neg, coef, 1e-3, grad_out=np.float32(0.7), item_offset=H.U_ROWS)
    assert np.array_equal(_bits(got), _bits(want)) and np.abs(want).max() > 0


def test_single_term_ordered_launch_at_its_slot_limit(dev, oracle):
    """B = 5461: 16 383 slots, the last size the ordered launch takes (bit-identical to the oracle)."""
    tab, users, pos, neg, coef, got = _single(dev, 5461, 64, joined=False)
    U = H.U_ROWS
    g_u, g_i = oracle.bpr_bwd_ordered(tab[:U], tab[U:], users, pos, neg, coef, 1e-3, grad_out=np.float32(0.7))
    assert np.array_equal(_bits(got), _bits(np.concatenate([g_u, g_i]))) and np.abs(g_i).max() > 0


def test_single_term_ordered_launch_past_its_slot_limit_falls_back(dev, oracle):
    """B = 5462: 16 386 slots, the atomic launch.  Every slot adds  c (p - n) + r2 u  (or c u + r2 p, -c u + r2 n): two addends
    per slot, each with at most four roundings (c = coef * grad_out, the difference, the product -- r2 = grad_out * 2 * reg /
    (B D) two, its product one -- and their sum), so the bound is (n + 4) 2^-24 S with n = 2 slots and S both magnitudes."""
    B, D, reg, go = 5462, 64, 1e-3, float(np.float32(0.7))
    tab, users, pos, neg, coef, got = _single(dev, B, D, joined=False)
    U = H.U_ROWS
    t64 = tab.astype(np.float64)
    u, p, n = t64[users], t64[U + pos], t64[U + neg]
    c = (coef.astype(np.float64) * go)[:, None]
    r2 = go * 2.0 * float(np.float32(reg)) / (B * D)
    g, s, cnt = (np.zeros(tab.shape) for _ in range(3))
    for rows, a, b in ((users, c * (p - n), r2 * u), (U + pos, c * u, r2 * p), (U + neg, -c * u, r2 * n)):
        np.add.at(g, rows, a + b)
        np.add.at(s, rows, np.abs(a) + np.abs(b))
        np.add.at(cnt, rows, 2.0)
    err, bound = np.abs(got - g), H.sum_bound(s, cnt)
    print(f"single-term fallback: worst error / bound = {float((err[bound > 0] / bound[bound > 0]).max()):.3f}")
    assert np.all(err <= bound) and np.abs(g).max() > 0
    g_u, g_i = oracle.bpr_bwd(tab[:U], tab[U:], users, pos, neg, coef.astype(np.float64), reg, grad_out=go)
    assert np.allclose(np.concatenate([g_u, g_i]), g, rtol=1e-9, atol=1e-15)
