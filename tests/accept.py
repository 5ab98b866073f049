"""The acceptance rule of the kernel tests and the helpers every test file used to copy.  Nothing model-specific lives here.

The rule: a tested tensor may deviate from its float64 restatement by at most 4 x max(own, floor), relative to the
restatement's largest magnitude; `own` is what an fp32 reference of the same lines deviates by (measured on the spot by
within_measured, or stored in a fixture), `floor` keeps the bound off zero where that reference happens to be exact.

Imports with numpy alone: the host tests run where there is no GPU, so torch and chaorec_amd are imported inside the functions
that need them."""
import ctypes

import numpy as np

ULP24 = 2.0 ** -24      # unit roundoff of float32: the floor of every family but the three below
EPS32 = 2.0 ** -23      # float32's spacing at 1 (np.finfo(np.float32).eps): the floor of the BSPM and CF_Diff tests
# MultVAE, MacridVAE and DualVAE pass a floor of 0.0 (their rule is 4 x own).  The three floors are inherited from the tests as
# they were written, not chosen here; a new model's tests use ULP24.


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else x


def rel_dev(got, ref, scale=None, zero_ref="strict"):
    """max |got - ref| in float64, relative to the largest |ref| (or to `scale`).  zero_ref "strict": a zero reference divides
    by 1e-300, so only an exact `got` passes; "absolute" (cfdiff_host, and diffrec_host which shares it): a zero reference
    compares absolutely."""
    assert zero_ref in ("strict", "absolute"), zero_ref
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = float(np.abs(ref).max()) if scale is None else float(scale)
    if zero_ref == "absolute":
        return float(np.abs(got - ref).max()) / (scale if scale > 0 else 1.0)
    return float(np.abs(got - ref).max() / max(scale, 1e-300))


def bound_of(own, floor):
    """The rule's relative bound; a test that needs it as an absolute tolerance (a ranking's atol) multiplies it by the scale."""
    return 4 * max(float(own), floor)


def within(what, got, ref64, own, floor, *, scale=None, zero_ref="strict", own_cap=None, failures=None, ratios=None):
    """`got` within 4 x max(own, floor) of `ref64`; prints the figures first.  A miss (a non-finite `got` is one) is appended to
    `failures` where given, so that a test can show all its figures, and asserted otherwise.  -> deviation / bound."""
    got, ref64, own = _np(got), _np(ref64), float(own)
    if own_cap is not None:
        assert own < own_cap, f"{what}: the reference itself deviates by {own:.3e}"
    err, bound = rel_dev(got, ref64, scale, zero_ref), bound_of(own, floor)
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{what}: deviation {err:.3e}, own {own:.3e}, bound {bound:.3e}, ratio {ratio:.3f}")
    if ratios is not None:
        ratios.append(ratio)
    if not (np.isfinite(np.asarray(got, dtype=np.float64)).all() and err <= bound):       # (`not <=`: NaN fails)
        if failures is None:
            raise AssertionError(f"{what}: {err:.3e} > {bound:.3e}")
        failures.append(f"{what}: {err:.3e} > {bound:.3e}")
    return ratio


def within_measured(what, got, ref32, ref64, floor, *, failures=None, ratios=None, own_cap=1e-4):
    """within(), with `own` measured here: the deviation of the fp32 reference `ref32` from `ref64`, itself below own_cap."""
    assert np.isfinite(np.asarray(ref32)).all(), f"{what}: the fp32 reference is not finite"
    return within(what, got, ref64, rel_dev(ref32, ref64), floor, own_cap=own_cap, failures=failures, ratios=ratios)


def same_bits(a, b):
    """numpy arrays: same shape, dtype and bytes"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_bits_t(a, b):
    """torch tensors of a 4-byte dtype: same shape and bits"""
    import torch
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the exact row selection: what rows_topk and rows_topk_wide are compared with ----------------------------------------------
def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def order_key(x):
    """mc_order_key / f32_to_ord: ascending with the float order, by bit pattern (-0 < +0, a NaN by sign and payload)."""
    b = bits(x)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def numpy_topk(x, K):
    comb = (order_key(x).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(x.shape[1], dtype=np.uint64))[None, :]
    idx = np.argsort(comb, axis=1)[:, ::-1][:, :K]          # key descending, then index ascending: the entries are distinct
    return idx.astype(np.int64), np.take_along_axis(x, idx, 1)


def user_item_dict(edges):
    d = {}
    for u, i in np.asarray(edges).tolist():
        d.setdefault(int(u), []).append(int(i))
    return d


# ---- the device and the raw library (C ABI through ctypes) ---------------------------------------------------------------------
def lib():
    from chaorec_amd import _lib as L
    return L.load()


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[(t.data_ptr() if t is not None else None) for t in ts])


def up(dev, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def to_dev(x, dtype, dev):
    import torch
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(dev)
