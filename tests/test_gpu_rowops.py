"""The elementwise and row kernels around every MMGCN / NGCF layer (csrc/rowops.hip: leaky_cat_add, leaky_split_bwd, leaky_bwd,
mul_pair_bwd, normalize_rows fwd / bwd, rows_mean) against plain references, through the C ABI: numpy float32 expressions
where every output element is ONE rounded operation (compared bit for bit), fp64 where the kernel reduces (compared to a
bound derived from the kernel's operation sequence).  Outputs lie inside a larger allocation of sentinel words, which must
be unchanged on both sides.  Shapes: the smallest, d1 != d2 both ways, NULL id / grad_id, and the first size past ONE grid of
each grid-stride loop (8192 x 256 float4 for the cat kernels, 4096 x 256 for leaky_bwd / mul_pair_bwd, 16 384 x 4 rows for
normalize_rows)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from accept import lib as _lib, ptr as _ptr, same_bits, stream as _stream, up as _up  # noqa: E402
from bpr_multi_host import Guarded, U24, bits  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from chaorec_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _salted(rng, *shape):
    """Normal values salted with +0, -0 and tiny negatives: the masks are `x > 0`, so all three take the slope branch."""
    a = rng.standard_normal(shape, dtype=np.float32)
    flat = a.reshape(-1)
    n = flat.size
    for start, v in ((0, 0.0), (1, -0.0), (2, -1e-30), (3, -1e-45)):      # (-1e-45: the smallest negative subnormal)
        flat[start::13][: max(1, n // 52)] = np.float32(v)
    return a


def _leaky(x, g, slope):
    """x > 0 ? g : g * slope, in float32."""
    return np.where(x > 0, g, g * np.float32(slope)).astype(np.float32)


def _same_bits(got, want):
    """accept.same_bits on the float32 values of both, reporting the first elements that differ"""
    if not same_bits(np.asarray(got, np.float32), np.asarray(want, np.float32)):
        assert got.shape == want.shape
        diff = bits(got) != bits(want)
        raise AssertionError((int(diff.sum()), got[diff][:4], want[diff][:4]))


CAT_CASES = [(1, 4, 4, True), (7, 4, 64, True), (5, 128, 4, True), (33, 64, 64, False), (32771, 192, 64, True)]


@pytest.mark.parametrize("slope", [0.01, 0.2])
@pytest.mark.parametrize("n_rows,d1,d2,with_id", CAT_CASES)
def test_leaky_cat_add_and_split_bwd_are_numpy_float32_bit_for_bit(dev, n_rows, d1, d2, with_id, slope):
    """out = [leaky(s) | u + id], and backwards gs = g[:, :d1] leaky'(cat[:, :d1]), gu = g[:, d1:] leaky'(uy), gid = g[:, d1:]
    (id / grad_id NULL in the 33-row case: out's second half is u, no gid written).  32 771 x 256 floats = 2 097 344 float4,
    just past the 8192 x 256 threads of one grid: the second trip of both grid-stride loops."""
    rng = np.random.default_rng([n_rows, d1, d2])
    assert (n_rows * (d1 + d2) // 4 > 8192 * 256) == (n_rows == 32771)
    s, u = _salted(rng, n_rows, d1), _salted(rng, n_rows, d2)
    idr = _salted(rng, n_rows, d2) if with_id else None
    lib = _lib()
    out = Guarded(dev, [np.full((n_rows, d1 + d2), np.float32(7.0))])
    s_d, u_d, id_d = _up(dev, s), _up(dev, u), _up(dev, idr)
    lib.chaorec_leaky_cat_add_f32(_ptr(s_d), _ptr(u_d), _ptr(id_d), _ptr(out.views[0]), n_rows, d1, d2, slope, _stream())
    torch.cuda.synchronize()
    cat = np.concatenate([_leaky(s, s, slope), u + idr if with_id else u], 1)
    _same_bits(out.read()[0], cat)
    # backwards, from the forward's output (with a few zeros of both signs planted where the mask reads)
    g, uy = _salted(rng, n_rows, d1 + d2), _salted(rng, n_rows, d2)
    grads = Guarded(dev, [np.full((n_rows, d1), np.float32(7.0)), np.full((n_rows, d2), np.float32(7.0)),
                          np.full((n_rows, d2), np.float32(7.0))])
    gs, gu, gid = grads.views
    g_d, cat_d, uy_d = _up(dev, g), _up(dev, cat), _up(dev, uy)
    lib.chaorec_leaky_split_bwd_f32(_ptr(g_d), _ptr(cat_d), _ptr(uy_d), _ptr(gs), _ptr(gu), _ptr(gid if with_id else None),
                                    n_rows, d1, d2, slope, _stream())
    torch.cuda.synchronize()
    got = grads.read()
    _same_bits(got[0], _leaky(cat[:, :d1], g[:, :d1], slope))
    _same_bits(got[1], _leaky(uy, g[:, d1:], slope))
    _same_bits(got[2], g[:, d1:] if with_id else np.full((n_rows, d2), np.float32(7.0)))


@pytest.mark.parametrize("slope", [0.01, 0.2])
@pytest.mark.parametrize("n", [4, 1028, 4194312])
def test_leaky_bwd_is_numpy_float32_bit_for_bit(dev, n, slope):
    """grad_in = y > 0 ? grad_out : grad_out * slope; n = 4 194 312 floats is 1 048 578 float4, past one grid of 4096 x 256."""
    rng = np.random.default_rng(n)
    assert (n // 4 > 4096 * 256) == (n == 4194312)
    y, gy = _salted(rng, n), _salted(rng, n)
    out = Guarded(dev, [np.full(n, np.float32(7.0))])
    y_d, gy_d = _up(dev, y), _up(dev, gy)
    _lib().chaorec_leaky_bwd_f32(_ptr(y_d), _ptr(gy_d), slope, _ptr(out.views[0]), n, _stream())
    torch.cuda.synchronize()
    _same_bits(out.read()[0], _leaky(y, gy, slope))


@pytest.mark.parametrize("n", [4, 1028, 4194312])
def test_mul_pair_bwd_is_numpy_float32_bit_for_bit(dev, n):
    """grad_s += grad_t * x (the product rounded, then the sum rounded: no fused multiply-add), grad_x = grad_t * s."""
    rng = np.random.default_rng(n + 1)
    gt, s, x, gs0 = (_salted(rng, n) for _ in range(4))
    out = Guarded(dev, [gs0, np.full(n, np.float32(7.0))])
    gt_d, s_d, x_d = _up(dev, gt), _up(dev, s), _up(dev, x)
    _lib().chaorec_mul_pair_bwd_f32(_ptr(gt_d), _ptr(s_d), _ptr(x_d), _ptr(out.views[0]), _ptr(out.views[1]), n, _stream())
    torch.cuda.synchronize()
    got = out.read()
    prod = (gt * x).astype(np.float32)
    _same_bits(got[0], gs0 + prod)
    _same_bits(got[1], gt * s)
    fused = (gs0.astype(np.float64) + gt.astype(np.float64) * x.astype(np.float64)).astype(np.float32)
    assert n == 4 or (bits(fused) != bits(gs0 + prod)).any()       # the inputs tell a fused multiply-add from the two roundings


@pytest.mark.parametrize("n_terms", [1, 8])
def test_rows_mean_one_and_eight_terms(dev, n_terms):
    """out = ((w t0 + w t1) + ...) left to right, every product and sum rounded, at n = 4 (one float4) and at n = 1028."""
    rng = np.random.default_rng(n_terms)
    for n in (4, 1028):
        terms = [rng.standard_normal(n, dtype=np.float32) for _ in range(n_terms)]
        dterms = [_up(dev, t) for t in terms]
        w = np.float32(1.0 / 3.0)
        out = Guarded(dev, [np.full(n, np.float32(7.0))])
        arr = (ctypes.c_void_p * n_terms)(*[t.data_ptr() for t in dterms])
        _lib().chaorec_rows_mean_f32(arr, n_terms, float(w), _ptr(out.views[0]), n, _stream())
        torch.cuda.synchronize()
        want = (w * terms[0]).astype(np.float32)
        for t in terms[1:]:
            want = (want + (w * t).astype(np.float32)).astype(np.float32)
        _same_bits(out.read()[0], want)


# ---- normalize_rows ----------------------------------------------------------------------------------------------------
EPS = np.float32(1e-12)
NORM_CASES = [(1, 0, 4), (5, 7, 260), (3, 2, 128), (6, 5, 384), (5, 6, 768), (40000, 30001, 4)]
_NORM = {}


def _norm_inputs(case):
    """a [rows_a, D], b [rows_b, D]; from five rows on: row 1 zero, row 2 all 1e-14 (|x| < eps), row 3 one element equal to
    eps -- the smallest float whose norm is >= eps -- and zeros."""
    rows_a, rows_b, D = case
    rng = np.random.default_rng([rows_a, rows_b, D])
    x = rng.standard_normal((rows_a + rows_b, D), dtype=np.float32) * np.float32(3.0)
    if rows_a + rows_b >= 5:
        x[1] = 0
        x[2] = np.float32(1e-14)
        x[3] = 0
        x[3, D // 2] = EPS
    return x[:rows_a].copy(), x[rows_a:].copy()


def _norm_forward(dev, case):
    """One forward launch per case, shared by the forward and the backward tests (the backward reads its y and norm)."""
    if case not in _NORM:
        rows_a, rows_b, D = case
        n_rows = rows_a + rows_b
        a, b = _norm_inputs(case)
        out = Guarded(dev, [np.full((n_rows, D), np.float32(7.0)), np.full(n_rows, np.float32(7.0))])
        a_d, b_d = _up(dev, a), _up(dev, b) if rows_b else None
        _lib().chaorec_normalize_rows_fwd_f32(_ptr(a_d), _ptr(b_d), rows_a, n_rows, D, float(EPS), _ptr(out.views[0]),
                                              _ptr(out.views[1]), _stream())
        torch.cuda.synchronize()
        y, norm = out.read()
        _NORM[case] = (a, b, y, norm)
    return _NORM[case]


@pytest.mark.parametrize("case", NORM_CASES, ids=lambda c: "a%d-b%d-D%d" % c)
def test_normalize_rows_forward_within_the_derived_bound_of_fp64(dev, case):
    """y = x / max(|x|, eps), norm = |x| against fp64 from the same float inputs.  The kernel's sequence (normalize_rows_fwd_kernel):
    a lane squares four elements (one rounding each), adds them as (xx + yy) + (zz + ww) (two more on the way of each square)
    and adds that to its running sum once per trip of the `c += 64` loop, P = ceil(D / 256) trips (at most P more); six
    butterfly levels add six.  Every square reaches the total through at most P + 9 roundings and all terms are positive, so
    the sum of squares is off by at most k u / (1 - k u) relative, k = P + 9, u = 2^-24.  sqrtf halves that and rounds once
    (correctly rounded): norm within (k / 2 + 1) u; the division by it rounds once more: y within (k / 2 + 2) u of x / |x|.
    Below eps the divisor is eps itself, exactly: one rounding.  A zero row gives exact zeros.
    D = 260 and 384 are dq = 65 and 96 (a second, partial trip), 768 three trips, 128 and 4 dq < 64 with idle lanes; every
    case has a workgroup whose four rows straddle rows_a; 70 001 rows are past the 16 384 x 4 rows of one grid."""
    rows_a, rows_b, D = case
    a, b, y, norm = _norm_forward(dev, case)
    x = np.concatenate([a, b]).astype(np.float64)
    n64 = np.sqrt((x * x).sum(1))
    y64 = x / np.maximum(n64, float(EPS))[:, None]
    k = math.ceil(D / 256) + 9
    rel = k * U24 / (1 - k * U24) / 2
    err_y, err_n = np.abs(y - y64), np.abs(norm - n64)
    bound_y, bound_n = (rel + 2 * U24) * np.abs(y64), (rel + U24) * n64
    ok = bound_y > 0
    print(f"normalize_rows fwd D={D} rows={rows_a}+{rows_b}: worst error / bound: y {float((err_y[ok] / bound_y[ok]).max()):.3f}, "
          f"norm {float((err_n[n64 > 0] / bound_n[n64 > 0]).max()):.3f}")
    assert np.all(err_y <= bound_y) and np.all(err_n <= bound_n)
    if rows_a + rows_b >= 5:
        assert not y[1].any() and norm[1] == 0 and norm[2] < EPS and y64[3, D // 2] == 1.0


@pytest.mark.parametrize("skip", ["0", "rows_a", "n_rows"])
@pytest.mark.parametrize("case", NORM_CASES, ids=lambda c: "a%d-b%d-D%d" % c)
def test_normalize_rows_backward_is_autograd_of_f_normalize_and_skips_rows(dev, case, skip):
    """grad_x against fp64 autograd of F.normalize(cat(a, b), eps) on the same inputs, per row err <= 1e-5 max|want| (the
    criterion of test_normalize_rows_is_f_normalize); grad_x starts as a NaN pattern: rows below skip_rows keep it, no other
    row has any left.  The row whose norm is EXACTLY eps sits on the discontinuity of the clamp's gradient -- whether
    sqrtf(eps * eps) lands on eps or one ulp below decides between two gradients that both are right for a neighbouring
    input -- so it is left out of the comparison of values (it is still written)."""
    rows_a, rows_b, D = case
    n_rows = rows_a + rows_b
    skip_rows = {"0": 0, "rows_a": rows_a, "n_rows": n_rows}[skip]
    a, b, y, norm = _norm_forward(dev, case)
    gy = np.random.default_rng([n_rows, D, 3]).standard_normal((n_rows, D), dtype=np.float32)
    nan_fill = np.full((n_rows, D), np.float32(np.nan))
    gx = Guarded(dev, [nan_fill])
    gy_d, y_d, norm_d = _up(dev, gy), _up(dev, y), _up(dev, norm)
    _lib().chaorec_normalize_rows_bwd_f32(_ptr(gy_d), _ptr(y_d), _ptr(norm_d), skip_rows, n_rows, D, float(EPS),
                                          _ptr(gx.views[0]), _stream())
    torch.cuda.synchronize()
    got = gx.read()[0]
    assert np.array_equal(bits(got[:skip_rows]), bits(nan_fill[:skip_rows]))
    assert not np.isnan(got[skip_rows:]).any()
    x64 = torch.from_numpy(np.concatenate([a, b])).double().requires_grad_(True)
    (torch.nn.functional.normalize(x64, p=2, dim=1, eps=float(EPS)) * torch.from_numpy(gy).double()).sum().backward()
    want = x64.grad.numpy()
    rows = np.arange(skip_rows, n_rows)
    rows = rows[rows != 3] if n_rows >= 5 else rows
    err, scale = np.abs(got[rows] - want[rows]).max(1, initial=0), np.abs(want[rows]).max(1, initial=0)
    if len(rows):
        print(f"normalize_rows bwd D={D} skip={skip_rows}: worst row error / (1e-5 rowmax) = {float((err / (1e-5 * scale)).max()):.3f}")
        assert scale.min() > 0
    assert np.all(err <= 1e-5 * scale)
