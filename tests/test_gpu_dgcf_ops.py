"""The DGCF kernels (csrc/dgcf.hip) op by op through the C ABI, called the way chaorec_amd/ops_dgcf.py calls them, every output
inside guard words and pre-filled with a NaN sentinel (tests/dgcf_ops_host.py; tests/test_dgcf_ops_host.py checks the references
used here on the CPU).

chaorec_dgcf_propagate_f32, all 19 supported (D, K) -- LPR = D / 4 lanes per row, RPW = 64 / LPR rows per wave, LPS = LPR / K
lanes per slice; D = 256 has RPW = 1 (no cross-row shuffle), D = 16 has RPW = 16, K = 1, 2 at D = 256 have LPS = 64, 32 -- on a
planted graph of 37 users (no multiple of any RPW) with empty rows at both ends and a 28-entry hub between two empty rows, in
eight launch forms:

  1  all rows, y only, no routing                       5  all rows, route_end = U, y and zout
  2  all rows, zout only (y = NULL)                     6  rows [3, 35), route_end = 14 (inside a wave's row group for every RPW > 1)
  3  all rows, y and zout aliased to z (in place)       7  rows [0, 20), route_end = U (past row_end)
  4  rows [0, U), route_end = U, y only                 8  rows [9, 9): status OK, nothing written

y / zout are held to the BITS of the float32 emulation of the defined order (propagate_f32); S and P_next to the derived
route_bound of the fp64 routing fed that float32 acc; rows outside the range, S / P_next of edges whose user row was not routed
and every guard word keep the sentinel.

chaorec_dgcf_softmax_f32 at E around the 256-thread workgroup and past one grid (16 384 workgroups); chaorec_dgcf_dcor_fwd_f32 /
_bwd_f32 over a case table with partial 16-row tiles on both axes, every K, D = 16 .. 256, 257 workgroups (the second trip of
the combine over the partials), a dirty grad_table of 65 600 rows (the second trip of the zero kernel), dirty workspaces, and the
scatter held to the bits of the ordered float32 sum; ops.dgcf_forward with autograd for L, T in {1, 2, 3} (dgcf_p_schedule's one
and two `egos` buffers) against the fp64 restatement.

Not covered: the grid-stride trips of the propagate (more than 262 140 waves) and of the dcor gather and scatter (n of about
16 385 at D = 256: no CPU fp64 reference of that size fits a test of a few seconds)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dgcf_ops_host as H  # noqa: E402
from accept import lib as _lib, ptr as _ptr, stream as _stream, up as _up  # noqa: E402
from test_dgcf_host import dgcf_forward as dgcf_forward64  # noqa: E402

pytestmark = pytest.mark.gpu

Guarded, _bits = H.Guarded, H.bits
INVALID = r"failed \(-1\)"     # CHAOREC_E_INVALID as the binding raises it
U, N = H.U, H.N


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from chaorec_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _is_sentinel(a):
    return _bits(a) == H.SENTINEL


# ---- propagate -------------------------------------------------------------------------------------------------------------
# form -> (row_begin, row_end, route_end, y, zout, zout aliased to z)
FORMS = {
    1: (0, N, 0, True, False, False),
    2: (0, N, 0, False, True, False),
    3: (0, N, 0, True, True, True),
    4: (0, U, U, True, False, False),
    5: (0, N, U, True, True, False),
    6: (3, 35, 14, True, True, False),
    7: (0, 20, U, True, False, False),
    8: (9, 9, U, True, True, False),
}


class State:
    pass


_STATES = {}


def _state(dev, dk):
    """The (D, K) inputs on the device, the float32 acc of every row and the fp64 routing of every edge from it (computed once),
    and the launches already made."""
    if dk in _STATES:
        return _STATES[dk]
    D, K = dk
    st = State()
    st.D, st.K = D, K
    pl, st.inp = H.planted(), H.build_inputs(D, K)
    st.E, st.users = pl["E"], pl["edges"][:, 0]
    st.g = pl["g"].to(dev)
    st.x, st.P, st.z = (_up(dev, st.inp[k]) for k in ("x", "P", "z"))
    st.acc = H.propagate_f32(pl["g"], st.inp["P"], st.inp["x"], K)
    st.zacc = st.inp["z"] + st.acc
    st.S64, st.Pn64 = H.routing_ref(st.acc, st.inp["x"], st.inp["P"], K)
    st.runs = {}
    _STATES[dk] = st
    return st


def _propagate(dev, st, form):
    """One chaorec_dgcf_propagate_f32 launch of `form` into fresh guarded sentinel buffers -> [y, zout, S, P_next] as read back."""
    r0, r1, rend, has_y, has_zout, inplace = FORMS[form]
    E, g = st.E, st.g
    buf = Guarded(dev, [H.sentinel(N, st.D), st.inp["z"].copy() if inplace else H.sentinel(N, st.D),
                        H.sentinel(E, st.K), H.sentinel(E, st.K)])
    y, zout, S, Pn = buf.views
    assert y.data_ptr() % 16 == 0 and zout.data_ptr() % 16 == 0
    z = zout if inplace else st.z
    _lib().chaorec_dgcf_propagate_f32(_ptr(g.rowptr), _ptr(g.col), _ptr(g.val), _ptr(g.eid), _ptr(st.P), _ptr(st.x),
                                      _ptr(y if has_y else None), _ptr(z if has_zout else None),
                                      _ptr(zout if has_zout else None), r0, r1, rend, st.D, st.K, _ptr(S), _ptr(Pn), _stream())
    torch.cuda.synchronize()
    return buf.read()


def _run(dev, st, form):
    if form not in st.runs:
        st.runs[form] = _propagate(dev, st, form)
    return st.runs[form]


def _check_form(st, form, got):
    """Every assertion on one launch's four buffers."""
    r0, r1, rend, has_y, has_zout, inplace = FORMS[form]
    y, zout, S, Pn = got
    D, K, W = st.D, st.K, st.D // st.K
    inside = np.zeros(N, bool)
    inside[r0:r1] = True
    # y / zout: bits of the defined order inside the range, the sentinel (in place: z) outside
    if has_y:
        diff = _bits(y[inside]) != _bits(st.acc[inside])
        assert not diff.any(), (form, int(diff.sum()), float(np.nanmax(np.abs(y[inside] - st.acc[inside]))))
        assert _is_sentinel(y[~inside]).all()
    else:
        assert _is_sentinel(y).all()
    if has_zout:
        diff = _bits(zout[inside]) != _bits(st.zacc[inside])
        assert not diff.any(), (form, int(diff.sum()))
        assert _is_sentinel(zout[~inside]).all()
    else:
        assert _is_sentinel(zout).all()
    # S / P_next: exactly the edges of the routed user rows
    routed = (st.users >= r0) & (st.users < min(r1, rend))
    assert _is_sentinel(S[~routed]).all() and _is_sentinel(Pn[~routed]).all()
    if not routed.any():
        return
    dS = np.abs(S[routed].astype(np.float64) - st.S64[routed])
    dP = np.abs(Pn[routed].astype(np.float64) - st.Pn64[routed])
    print(f"propagate {H.dk_id((D, K))} form {form}: dS / route_bound = {np.nanmax(dS) / H.route_bound(W):.3f}, "
          f"dP / bound = {np.nanmax(dP) / H.pnext_bound(W):.3f} over {int(routed.sum())} edges")
    assert np.all(dS <= H.route_bound(W)), float(dS.max() / H.route_bound(W))
    assert np.all(dP <= H.pnext_bound(W)), float(dP.max() / H.pnext_bound(W))
    assert np.all(np.abs(Pn[routed].astype(np.float64).sum(1) - 1.0) <= K * 2.0 ** -23)
    if K == 1:
        assert np.all(Pn[routed] == np.float32(1.0))


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("dk", H.DK_GRID, ids=H.dk_id)
def test_propagate_forms(dev, dk, form):
    """One launch form at one (D, K): y / zout bit for bit, S / P_next within the derived bound and only where routed, nothing
    outside the row range or the buffers, and a second launch with the same bits."""
    st = _state(dev, dk)
    got = _run(dev, st, form)
    _check_form(st, form, got)
    again = _propagate(dev, st, form)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))
    if form == 8:
        assert all(_is_sentinel(a).all() for a in got)
    if form == 3:       # in place (the model's layers after the first): the same bits as the separate buffers of form 2
        assert np.array_equal(_bits(got[1]), _bits(_run(dev, st, 2)[1]))
    if form == 5:       # the last iteration's form against the user-row form and the plain propagate
        y4, _, S4, Pn4 = _run(dev, st, 4)
        y1 = _run(dev, st, 1)[0]
        assert np.array_equal(_bits(got[0][:U]), _bits(y4[:U]))
        assert np.array_equal(_bits(got[2]), _bits(S4)) and np.array_equal(_bits(got[3]), _bits(Pn4))
        assert np.array_equal(_bits(got[0]), _bits(y1))
        assert not _is_sentinel(got[2]).any() and not _is_sentinel(got[3]).any()      # every edge has a user row in [0, U)


def test_propagate_refusals_launch_nothing(dev):
    """CHAOREC_E_INVALID for D = 8 with K = 2, K = 3, routing without S, P_next aliased to P, x offset by one float and
    row_end < row_begin -- and every output still the sentinel, P unchanged."""
    st = _state(dev, (16, 2))
    before = st.P.clone()
    x_off = ctypes.c_void_p(st.x.data_ptr() + 4)
    lib, g = _lib(), st.g
    buf = Guarded(dev, [H.sentinel(N, 16), H.sentinel(N, 16), H.sentinel(st.E, 2), H.sentinel(st.E, 2)])
    y, zout, S, Pn = buf.views
    base = dict(P=_ptr(st.P), x=_ptr(st.x), r0=0, r1=N, rend=U, D=16, K=2, S=_ptr(S), Pn=_ptr(Pn))
    for kw in (dict(D=8), dict(K=3), dict(S=_ptr(None)), dict(Pn=_ptr(st.P)), dict(x=x_off), dict(r0=9, r1=3)):
        a = dict(base, **kw)
        with pytest.raises(RuntimeError, match=INVALID):
            lib.chaorec_dgcf_propagate_f32(_ptr(g.rowptr), _ptr(g.col), _ptr(g.val), _ptr(g.eid), a["P"], a["x"], _ptr(y),
                                           _ptr(st.z), _ptr(zout), a["r0"], a["r1"], a["rend"], a["D"], a["K"], a["S"], a["Pn"],
                                           _stream())
    torch.cuda.synchronize()
    assert all(_is_sentinel(a).all() for a in buf.read())
    assert torch.equal(st.P, before)


# ---- softmax ---------------------------------------------------------------------------------------------------------------
def _softmax(dev, S):
    buf = Guarded(dev, [H.sentinel(*S.shape)])
    S_dev = _up(dev, S)
    _lib().chaorec_dgcf_softmax_f32(_ptr(S_dev), _ptr(buf.views[0]), S.shape[0], S.shape[1], _stream())
    torch.cuda.synchronize()
    assert np.array_equal(S_dev.cpu().numpy().view(np.int32), S.view(np.int32))
    return buf.read()[0]


def _softmax64(S):
    return torch.softmax(torch.from_numpy(S).double(), 1).numpy()


def _extreme_row(K):
    return np.asarray([80.0] + [-80.0] * (K - 1), np.float32)


@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("E", [1, 255, 256, 257, 1000])
def test_softmax_against_fp64(dev, E, K):
    """Within (K + 16) 2^-24 of the fp64 softmax of the float32 input; an all-equal row is exactly 1 / K, the row (80, -80, ...)
    exactly (1, 0, ...), K = 1 exactly 1.0; the guards stay."""
    rng = np.random.default_rng([E, K])
    S = (3.0 * rng.standard_normal((E, K))).astype(np.float32)
    one = np.zeros((1, K), np.float32)
    if E == 1:          # one row: the two planted rows in launches of their own
        one[0] = 1.25
        assert np.all(_softmax(dev, one) == np.float32(1.0 / K))
        one[0] = _extreme_row(K)
        assert np.array_equal(_softmax(dev, one)[0], np.eye(K, dtype=np.float32)[0])
    else:
        S[0], S[E - 1] = -2.5, _extreme_row(K)
    P = _softmax(dev, S)
    err = np.abs(P.astype(np.float64) - _softmax64(S)).max()
    print(f"softmax E={E} K={K}: error / bound = {err / ((K + 16) * H.U24):.3f}")
    assert np.all(np.abs(P.astype(np.float64) - _softmax64(S)) <= (K + 16) * H.U24)
    if E > 1:
        assert np.all(P[0] == np.float32(1.0 / K)) and np.array_equal(P[E - 1], np.eye(K, dtype=np.float32)[0])
    if K == 1:
        assert np.all(P == np.float32(1.0))


def test_softmax_second_trip_of_the_grid_stride_loop(dev):
    """E = 4 194 312, K = 2: eight edges past the 16 384 x 256 threads of one grid."""
    E, K = 4_194_312, 2
    assert E > 16384 * 256
    rng = np.random.default_rng(41)
    S = (3.0 * rng.standard_normal((E, K), dtype=np.float32))
    P = _softmax(dev, S)
    err = np.abs(P.astype(np.float64) - _softmax64(S))
    print(f"softmax E={E} K={K}: error / bound = {err.max() / ((K + 16) * H.U24):.3f}; the last 8 rows {err[-8:].max():.1e}")
    assert np.all(err <= (K + 16) * H.U24)


# ---- distance correlation --------------------------------------------------------------------------------------------------
WS_PAD, WS_GUARD = 256, 0xA5


def _dcor(dev, table_dev, n_table_rows, idx, D, K, ws_fill):
    """chaorec_dgcf_dcor_fwd_f32 then _bwd_f32 (grad_out 3.0) with a workspace pre-filled with `ws_fill` between guard bytes and
    outputs pre-filled with the sentinel -> (loss [1], grad_rows [n, D], grad_table [rows, D])."""
    lib, n = _lib(), len(idx)
    nbytes = lib.chaorec_dgcf_dcor_workspace_bytes(n, D, K)
    ws_all = torch.full((nbytes + 2 * WS_PAD,), WS_GUARD, dtype=torch.uint8, device=dev)
    ws = ws_all[WS_PAD:WS_PAD + nbytes]
    ws.fill_(ws_fill)
    assert ws.data_ptr() % 256 == 0
    buf = Guarded(dev, [H.sentinel(n_table_rows, D), H.sentinel(n, D), H.sentinel(1)])
    grad_table, grad_rows, loss = buf.views
    assert grad_table.data_ptr() % 16 == 0
    s, perm = H.stable_sort(idx)
    idx_d, s_d, perm_d = _up(dev, idx), _up(dev, s), _up(dev, perm)
    go = torch.tensor([H.DCOR_GRAD_OUT], dtype=torch.float32, device=dev)
    lib.chaorec_dgcf_dcor_fwd_f32(_ptr(table_dev), _ptr(idx_d), n, D, K, _ptr(loss), _ptr(ws), nbytes, _stream())
    lib.chaorec_dgcf_dcor_bwd_f32(_ptr(s_d), _ptr(perm_d), n, D, K, _ptr(go), _ptr(ws), _ptr(grad_rows), _ptr(grad_table),
                                  n_table_rows, _stream())
    torch.cuda.synchronize()
    assert bool((ws_all[:WS_PAD] == WS_GUARD).all()) and bool((ws_all[WS_PAD + nbytes:] == WS_GUARD).all())
    grad_table, grad_rows, loss = buf.read()
    return loss, grad_rows, grad_table


def _check_dcor(name, n, kind, grad_checked, ref, gref, idx, got, again):
    loss, grad_rows, grad_table = got
    # loss
    bar = 1e-5 * max(1.0, abs(ref))
    err = abs(float(loss[0]) - ref)
    line = f"dcor {name}: loss {float(loss[0]):.6f}, error / bar = {err / bar:.3f}"
    assert np.isfinite(loss[0]) and np.isfinite(grad_rows).all() and np.isfinite(grad_table).all()
    # scatter: bits of the ordered float32 sum of the launch's own grad_rows; every other row exactly +0
    want = H.scatter_f32(grad_rows, idx, grad_table.shape[0])
    assert np.array_equal(_bits(grad_table), _bits(want))
    idle = np.setdiff1d(np.arange(grad_table.shape[0]), idx)
    assert not _bits(grad_table[idle]).any()
    # gradient
    if n == 1 or kind == "equal":
        assert np.all(grad_rows == 0.0) and np.all(grad_table == 0.0)
    if grad_checked:
        scale = float(np.abs(gref).max())
        gbar = 1e-3 * H.DCOR_GRAD_OUT * scale
        gerr = float(np.abs(grad_table.astype(np.float64) - H.DCOR_GRAD_OUT * gref).max())
        line += f", gradient error / bar = {gerr / gbar:.3f} (scale {scale:.2e})"
    print(line)
    assert err <= bar
    if grad_checked:
        assert scale > 0 and gerr <= gbar
    # two runs, the workspaces pre-filled with 0x00 and 0xFF: the same bits
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))


@pytest.mark.parametrize("case", H.DCOR_CASES, ids=H.dcor_id)
def test_dcor_against_fp64(dev, case):
    """Loss within 1e-5 max(1, |ref|) of fp64; grad_table (grad_out 3.0) within 1e-3 * 3 * max|ref grad| for n >= 15 (exactly 0
    for n = 1 and for all idx equal; finite for n = 2); the scatter bit for bit the ordered sum of grad_rows with every untouched
    row +0 although grad_table held the sentinel; the same bits from a 0x00 and a 0xFF workspace; no write outside any buffer."""
    n, D, K, rows, kind = case
    c = H.build_dcor(case)
    ref, gref = H.dcor_ref64(case)
    table_dev = _up(dev, c["table"])
    got = _dcor(dev, table_dev, rows, c["idx"], D, K, 0x00)
    again = _dcor(dev, table_dev, rows, c["idx"], D, K, 0xFF)
    _check_dcor(H.dcor_id(case), n, kind, H.dcor_grad_checked(case), ref, gref, c["idx"], got, again)


def test_dcor_large_table_is_zeroed_by_the_launch(dev):
    """n = 17, D = 256, K = 2 over a table of 65 600 rows: 4 198 400 float4 of grad_table, past the 16 384 x 256 threads of
    dcor_zero_kernel's grid.  Only the gathered rows are read: every other table row is NaN."""
    n, D, K, rows = 17, 256, 2, 65_600
    assert rows * D // 4 > 16384 * 256
    rng = np.random.default_rng(65600)
    small = (0.3 * rng.standard_normal((12, D))).astype(np.float32)
    where = np.sort(np.concatenate([[0, rows - 1], rng.choice(np.arange(1, rows - 1), 10, replace=False)]))
    idx_small = rng.integers(0, 12, n)
    idx_small[:2] = (0, 11)                                 # the first and the last table row are gathered
    idx = where[idx_small].astype(np.int64)
    t = torch.from_numpy(small).double().requires_grad_(True)
    loss = H.dcor_loss_torch(t[torch.from_numpy(idx_small)], K)
    loss.backward()
    gref = np.zeros((rows, D))
    gref[where] = t.grad.numpy()
    table_dev = torch.full((rows, D), float("nan"), dtype=torch.float32, device=dev)
    table_dev[torch.from_numpy(where).to(dev)] = _up(dev, small)
    got = _dcor(dev, table_dev, rows, idx, D, K, 0x00)
    again = _dcor(dev, table_dev, rows, idx, D, K, 0xFF)
    _check_dcor("n17-D256-K2-rows65600", n, "random", True, float(loss.item()), gref, idx, got, again)


def test_dcor_refusals_touch_nothing(dev):
    """CHAOREC_E_INVALID for K = 1, n = 0, D = 8 with K = 2 and a workspace one byte short; the outputs and the workspace keep
    what they held: a refused call launches nothing.  (D = 8 with K = 2 passes chaorec_dgcf_check_shape; the forward used to
    launch its gather into the workspace before the pass-1 dispatch refused the shape.)"""
    lib = _lib()
    n, D, K, rows = 17, 16, 2, 9
    rng = np.random.default_rng(9)
    table = _up(dev, (0.3 * rng.standard_normal((rows, D))).astype(np.float32))
    idx = rng.integers(0, rows, n).astype(np.int64)
    s, perm = H.stable_sort(idx)
    idx_d, s_d, perm_d = _up(dev, idx), _up(dev, s), _up(dev, perm)
    nbytes = lib.chaorec_dgcf_dcor_workspace_bytes(n, D, K)
    ws = torch.full((nbytes,), WS_GUARD, dtype=torch.uint8, device=dev)
    go = torch.tensor([H.DCOR_GRAD_OUT], dtype=torch.float32, device=dev)
    buf = Guarded(dev, [H.sentinel(rows, D), H.sentinel(n, D), H.sentinel(1)])
    grad_table, grad_rows, loss = buf.views
    for kw in (dict(K=1), dict(n=0), dict(D=8), dict(ws_bytes=nbytes - 1)):
        a = dict(dict(n=n, D=D, K=K, ws_bytes=nbytes), **kw)
        with pytest.raises(RuntimeError, match=INVALID):
            lib.chaorec_dgcf_dcor_fwd_f32(_ptr(table), _ptr(idx_d), a["n"], a["D"], a["K"], _ptr(loss), _ptr(ws), a["ws_bytes"],
                                          _stream())
    for kw in (dict(K=1), dict(n=0), dict(D=8)):
        a = dict(dict(n=n, D=D, K=K), **kw)
        with pytest.raises(RuntimeError, match=INVALID):
            lib.chaorec_dgcf_dcor_bwd_f32(_ptr(s_d), _ptr(perm_d), a["n"], a["D"], a["K"], _ptr(go), _ptr(ws), _ptr(grad_rows),
                                          _ptr(grad_table), rows, _stream())
    torch.cuda.synchronize()
    assert all(_is_sentinel(a).all() for a in buf.read())
    assert bool((ws == WS_GUARD).all())


# ---- the model's forward and backward over dgcf_p_schedule -------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_forward_and_backward_for_every_schedule(dev, L, T):
    """ops.dgcf_forward with autograd on the planted graph at D = 16, K = 4 from S = 1, against dgcf_forward in fp64 and the
    gradient of sum(result * G): L = 1 uses one `egos` buffer, L = 2 alternates two, T = 1 starts from ('saved', 0).  The bars of
    test_golden_one_step: atol 1e-5 for the result and S, 2e-4 max|g| + 1e-7 for the gradient."""
    from chaorec_amd import ops
    D, K = 16, 4
    pl, inp = H.planted(), H.build_inputs(D, K)
    E = pl["E"]
    G = np.random.default_rng(77).standard_normal((N, D)).astype(np.float32)
    x64 = torch.from_numpy(inp["x"]).double().requires_grad_(True)
    out64, S64 = dgcf_forward64(x64, pl["edges"], K, T, L, torch.ones((E, K), dtype=torch.float64))
    (out64 * torch.from_numpy(G).double()).sum().backward()
    g64 = x64.grad.numpy()
    S = torch.ones((E, K), dtype=torch.float32, device=dev)
    P = torch.full((E, K), float("nan"), dtype=torch.float32, device=dev)
    ops.dgcf_softmax(S, P)
    x = _up(dev, inp["x"]).requires_grad_(True)
    result = ops.dgcf_forward(x, pl["g"].to(dev), S, P, L, T)
    (result * _up(dev, G)).sum().backward()
    torch.cuda.synchronize()
    d_res = np.abs(result.detach().cpu().double().numpy() - out64.detach().numpy()).max()
    d_S = np.abs(S.cpu().double().numpy() - S64.numpy()).max()
    d_P = np.abs(P.cpu().double().numpy() - torch.softmax(S64, 1).numpy()).max()
    d_g = np.abs(x.grad.cpu().double().numpy() - g64).max()
    g_bar = 2e-4 * np.abs(g64).max() + 1e-7
    print(f"model L={L} T={T}: |result| {d_res:.1e}, |S| {d_S:.1e}, |P| {d_P:.1e}, gradient error / bar = {d_g / g_bar:.3f}")
    assert d_res <= 1e-5 and d_S <= 1e-5 and d_P <= 1e-5 and d_g <= g_bar
    assert np.abs(S64.numpy() - 1.0).max() > 0.1 and np.abs(g64).max() > 0.1
