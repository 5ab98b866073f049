"""The autoencoder kernels on the MI355X, OP BY OP (chaorec_amd/ops_extra.py over csrc/multvae.hip, macridvae.hip,
dualvae.hip and csrc/vae_common.h) against the float64 restatements of tests/vae_ops_host.py, on structures built here
from a seeded numpy generator: signed weights and activations, row scales over two decades, random upstream gradients.

Shapes: B in {1, 128, 129} (the VAE_SB boundary) x I (N for DualVAE) in {63, 64, 65, 129, 257, 8449} (VAE_TW, the one
live item of the last VAE_TI tile, 67 tiles in 34 splits of 2 with a last split of one tile of one item), not the full
product: every B meets 8449 and one I near 64, every I meets B = 129.  The structure (make_structure) has one item held
by 130 users with >= 70 of them in the batch (B >= 128: two passes of the 64-wide owner walk), a user three times in the
batch, a user with an empty row, an item nobody holds, the last item and the last user.

Measure (vae_ops_host.row_dev / bound_of): per output row the largest |error| over the row's largest |fp64 value| (rows
below 1e-3 of the tensor's largest normed by that floor), the maximum over rows; bound = 4 x the same measure of the
float32 run of the SAME restatement on the same inputs, at least 2^-22.  Every comparison prints both deviations; the
largest kernel / bound ratio per op is printed at the end of each test.

One quantity is held to the forward error bound of its fp64 addends, n 2^-24 sum |addends| per element, instead of 4 x:
DualVAE encode's dbias.  It is ops.col_sum of the upstream gradient itself -- additions only, B * 5 signed addends with
row scales over two decades per element -- and the float32 restatement's torch sum is pairwise, so 4 x its deviation is
narrower than an honest fixed-order fp32 sum can meet where an element cancels (measured 0.07 .. 4.8 x that bound over
the ten shapes; 0.0004 .. 0.19 x the forward bound); a dropped or doubled row of average size, sum |addends| / n, is
still 2^24 / n^2 = 40 x outside n 2^-24 sum |addends| at B = 129.

Exact conditions: the encoder-gradient row of the item nobody holds (MultVAE: 2 gsq w bit for bit; MacridVAE's encode
has no sum-of-squares output, its rows of dW and dc are exactly 0); junk (NaN) rows behind I in a larger allocation
leave every result bit-identical; permuting the batch moves every per-sample output with it bit for bit.

Device draws (training, keep=None): the mask the forward used is decoded with one-hot weights and must equal the numpy
restatement of the counter RNG flag for flag; forward AND backward with random weights must then meet float64 under that
decoded mask -- the backward's (slot, item_pos) redraw is the forward's (b, j) draw -- and z is built from eps_out.

Largest kernel deviation / bound per op, measured on the MI355X over all shapes (1.0 = at the bound):
  multvae encode 0.86 (dbq, B=129 I=257)     multvae decode 0.80 (dbp, B=129 I=65)
  macrid concept 0.37 (dE, B=129 I=65)       macrid encode 0.60 (db1, B=129 I=64)      macrid mix 0.70 (dcates, B=1 I=63)
  dualvae encode 0.45 (dw, B=128 N=8449; dbias 0.19 of its forward bound)               dualvae dense 0.43 (dw, B=129 N=8449)
  dualvae_linear 0.25 (at the 2^-22 floor)   dualvae_loss 0.32 (dmu, B=1)
  device draws: multvae 0.31 (h), macrid 0.77 (db1)"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vae_ops_host as vo  # noqa: E402
from accept import ULP24, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(1, 63), (1, 8449), (128, 64), (128, 8449), (129, 63), (129, 64), (129, 65), (129, 129), (129, 257), (129, 8449)]
U = 150                     # users (rows of the sample side); the hot item's 130 holders are users 0 .. 129
HOT_USERS = 130
SEED = 1234                 # the counter RNG's seed in every device-drawn call


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------
# the structure
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_structure(B, I, deg_lo=2, deg_hi=13):
    """-> dict: rowptr, col (ascending per row), users [B], hot / dead item, rep / empty user.  Item `hot` is held by
    users 0 .. 129, item `dead` by nobody, user `empty` holds nothing, user U - 1 holds item I - 1."""
    rng = np.random.default_rng(1000 * B + I)
    hot, dead, rep, empty = 5, I // 2, 3, U - 9
    free = np.array([i for i in range(I) if i not in (hot, dead)])
    rows = []
    for u in range(U):
        if u == empty:
            rows.append(np.zeros(0, dtype=np.int64))
            continue
        r = set(rng.choice(free, size=int(rng.integers(deg_lo, min(deg_hi, len(free)) + 1)), replace=False).tolist())
        if u < HOT_USERS:
            r.add(hot)
        if u == U - 1:
            r.add(I - 1)
        rows.append(np.array(sorted(r), dtype=np.int64))
    rowptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    col = np.concatenate(rows).astype(np.int64)
    if B == 1:
        users = np.array([U - 1], dtype=np.int64)
    else:
        fixed = [rep, rep, rep, empty, U - 1]
        hot_part = rng.choice(np.setdiff1d(np.arange(HOT_USERS), [rep]), size=75, replace=False).tolist()
        rest = rng.integers(0, U, size=B - len(fixed) - len(hot_part)).tolist()
        users = rng.permutation(np.array(fixed + hot_part + rest, dtype=np.int64))
        in_batch = np.isin(np.arange(HOT_USERS), users).sum()
        assert in_batch >= 70 and (users == rep).sum() >= 3 and empty in users and U - 1 in users
    assert len(users) == B and not (col == dead).any() and (col == I - 1).any() and (col == hot).sum() == HOT_USERS
    return dict(rowptr=rowptr, col=col, users=users, hot=hot, dead=dead, rep=rep, empty=empty, I=I, B=B)


def on_device(st, dev, users=None):
    from chaorec_amd import ops_extra as ox
    s = ox.MultVAEStructure(torch.from_numpy(st["rowptr"]), torch.from_numpy(st["col"]), st["I"]).to(dev)
    users = st["users"] if users is None else users
    return s, s.batch(torch.from_numpy(np.asarray(users)).to(dev))


def flags_and_mask(rng, st, users=None):
    """Random GIVEN keep flags (sample 0's row, then sample 1's, ...) and the dense [B, I] mask they mean."""
    users = st["users"] if users is None else users
    n = np.diff(st["rowptr"])[users]
    flags = (rng.random(int(n.sum())) < 0.5).astype(np.uint8)
    mask, off = np.zeros((len(users), st["I"])), 0
    for b, u in enumerate(users):
        mask[b, st["col"][st["rowptr"][u]:st["rowptr"][u + 1]]] = flags[off:off + n[b]]
        off += n[b]
    return flags, mask


# ---------------------------------------------------------------------------------------------------------------
# inputs and the comparison
# ---------------------------------------------------------------------------------------------------------------
def signed(rng, *shape, scale=1.0, decades=2.0):
    """float32 N(0, 1) x scale, every row (first index) times 10^U(-decades, 0)."""
    x = rng.standard_normal(shape) * scale
    if len(shape) > 1 and decades:
        x = x * 10.0 ** rng.uniform(-decades, 0.0, size=(shape[0],) + (1,) * (len(shape) - 1))
    return np.ascontiguousarray(x, dtype=np.float32)


def unit(x):
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=-1, keepdims=True), dtype=np.float32)


def softmax_rows(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return np.ascontiguousarray(e / e.sum(-1, keepdims=True), dtype=np.float32)


def cu(x, dev, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return t.requires_grad_(True) if grad else t


def host(t):
    return t.detach().cpu().numpy()


class Table:
    """Collects kernel deviation / bound per quantity; check() asserts after printing."""

    def __init__(self, op):
        self.op, self.worst, self.failed = op, (0.0, ""), []

    def check(self, got, ref64, ref32, what):
        d, own = vo.row_dev(got, ref64), vo.row_dev(ref32, ref64)
        bound = vo.bound_of(ref32, ref64)
        print(f"{self.op} {what}: kernel deviation {d:.3e}, reference's own {own:.3e}, bound {bound:.3e}, ratio {d / bound:.3f}")
        if not d / bound <= self.worst[0]:
            self.worst = (d / bound, what)
        if not d <= bound:
            self.failed.append(f"{what}: {d:.3e} > {bound:.3e}")

    def check_sum(self, got, ref64, addends, what):
        """A plain fp32 sum over the first axis of `addends` (fp32 inputs, so the fp64 sum's addends are exact): the forward
        error bound n 2^-24 sum |addends| per element."""
        a = np.abs(np.asarray(addends, dtype=np.float64))
        err, bound = np.abs(np.asarray(got, dtype=np.float64) - ref64), a.shape[0] * ULP24 * a.sum(0)
        ratio = float((err / bound).max())
        print(f"{self.op} {what}: largest |error| {err.max():.3e}, forward bound there {bound[np.argmax(err / bound)]:.3e}, ratio {ratio:.3f}")
        if not ratio <= self.worst[0]:
            self.worst = (ratio, what)
        if not ratio <= 1.0:
            self.failed.append(f"{what}: {ratio:.3f} x the forward error bound")

    def done(self):
        print(f"{self.op}: largest kernel / bound ratio {self.worst[0]:.3f} ({self.worst[1]})")
        assert not self.failed, f"{self.op}: " + "; ".join(self.failed)


def both(fwd, inputs, wrt, upstream, **const):
    (o64, g64), (o32, g32) = (vo.run(fwd, inputs, wrt, upstream, dtype=dt, **const) for dt in (torch.float64, torch.float32))
    return o64, g64, o32, g32


def backward(pairs):
    """sum <output, upstream gradient> . backward()"""
    sum((o * g).sum() for o, g in pairs).backward()
    torch.cuda.synchronize()


def with_junk(x, dev, rows=200):
    """x's rows at the front of a larger allocation whose remaining rows are NaN; the returned view is x's shape."""
    big = torch.full((x.shape[0] + rows,) + tuple(x.shape[1:]), float("nan"), dtype=torch.float32, device=dev)
    big[:x.shape[0]] = torch.from_numpy(x).to(dev)
    return big[:x.shape[0]]


def check_plan(splits, I):
    """67 tiles of VAE_TI = 128 in 34 splits: 2 tiles per split, the last split one tile of one item."""
    n_tiles = (I + 127) // 128
    if I == 8449:
        assert splits == 34 and n_tiles == 67 and -(-n_tiles // splits) == 2 and I - 128 * 2 * (splits - 1) == 1
    else:
        assert 1 <= splits <= n_tiles


# ---------------------------------------------------------------------------------------------------------------
# MultVAE
# ---------------------------------------------------------------------------------------------------------------
def multvae_decode_run(ox, dev, st, z, Wp, bp, gnll, gsq, users=None, junk=False):
    s, batch = on_device(st, dev, users)
    zt = cu(z, dev, True)
    Wt, bt = (with_junk(Wp, dev).requires_grad_(True), with_junk(bp, dev).requires_grad_(True)) if junk else (cu(Wp, dev, True), cu(bp, dev, True))
    neg_ll, sq, lse = ox.multvae_decode(zt, Wt, bt, s, batch)
    backward(((neg_ll, gnll), (sq, gsq)))
    return dict(neg_ll=host(neg_ll), sumsq=host(sq), lse=host(lse), z=host(zt.grad), Wp=host(Wt.grad), bp=host(bt.grad))


@pytest.mark.parametrize("B,I", CASES)
def test_multvae_ops(dev, B, I):
    from chaorec_amd import _lib, ops_extra as ox
    st = make_structure(B, I)
    rng = np.random.default_rng(7 * B + I)
    users, x = st["users"], vo.dense_rows(st["rowptr"], st["col"], st["users"], I)
    s, batch = on_device(st, dev)
    state = torch.tensor([8, 7], dtype=torch.int64, device=dev)
    t = Table(f"multvae B={B} I={I}")

    # encode, given keep flags and eps
    Wq_t, bq, eps = signed(rng, I, 128, scale=0.5), signed(rng, 128, scale=0.3), signed(rng, B, 64, decades=0)
    flags, mask = flags_and_mask(rng, st)
    gz, gkl, gsq = signed(rng, B, 64), np.float32(rng.standard_normal()), np.float32(rng.standard_normal())
    Wt, bt = cu(Wq_t, dev, True), cu(bq, dev, True)
    z, kl, sq, h, eps_out = ox.multvae_encode(Wt, bt, s, batch, state, SEED, True, 0.5, cu(flags, dev), s.keep_offsets(batch[0]), cu(eps, dev))
    backward(((z, cu(gz, dev)), (kl, float(gkl)), (sq, float(gsq))))
    o64, g64, o32, g32 = both(vo.multvae_encode_fwd, dict(Wq_t=Wq_t, bq=bq, x=x, mask=mask, eps=eps), ("Wq_t", "bq"),
                              {"z": gz, "kl": gkl, "sumsq": gsq}, keep_prob=0.5, training=True)
    assert same_bits(host(eps_out), eps)
    for k, got in (("h", h), ("z", z), ("kl", kl[0]), ("sumsq", sq[0])):
        t.check(host(got), o64[k], o32[k], f"encode {k}")
    t.check(host(Wt.grad), g64["Wq_t"], g32["Wq_t"], "encode dWq_t")
    t.check(host(bt.grad), g64["bq"], g32["bq"], "encode dbq")
    want = np.float32(2.0) * (gsq * Wq_t[st["dead"]])                      # nobody holds it: 2 gsq w, bit for bit
    assert same_bits(host(Wt.grad)[st["dead"]], want), "the untouched item's encoder-gradient row is not exactly 2 gsq w"

    # decode
    zin, Wp, bp = signed(rng, B, 64, decades=1.0), signed(rng, I, 64, scale=0.5), signed(rng, I, scale=0.5)
    gnll, gsq = float(np.float32(rng.standard_normal())), float(np.float32(rng.standard_normal()))
    splits = int(_lib.load().chaorec_multvae_decode_splits(B, I))
    check_plan(splits, I)
    out = multvae_decode_run(ox, dev, st, zin, Wp, bp, gnll, gsq)
    o64, g64, o32, g32 = both(vo.multvae_decode_fwd, dict(z=zin, Wp=Wp, bp=bp, x=x), ("z", "Wp", "bp"), {"neg_ll": gnll, "sumsq": gsq})
    for k in ("neg_ll", "sumsq", "lse"):
        t.check(out[k].reshape(o64[k].shape), o64[k], o32[k], f"decode {k}")
    for k in ("z", "Wp", "bp"):
        t.check(out[k], g64[k], g32[k], f"decode d{k}")
    # junk rows behind I change no bit
    junk = multvae_decode_run(ox, dev, st, zin, Wp, bp, gnll, gsq, junk=True)
    for k in out:
        assert same_bits(out[k], junk[k]), f"decode {k} moved with junk rows behind I"
    # a permuted batch: per-sample outputs move with it
    if B > 1:
        p = rng.permutation(B)
        perm = multvae_decode_run(ox, dev, st, zin[p], Wp, bp, gnll, gsq, users=users[p])
        assert same_bits(perm["lse"], out["lse"][p]) and same_bits(perm["z"], out["z"][p]), "decode lse / dz do not move with the batch"
        s2, batch2 = on_device(st, dev, users[p])
        z2 = ox.multvae_encode(cu(Wq_t, dev), cu(bq, dev), s2, batch2, state, SEED, False, 0.5, None, None, cu(eps[p], dev))[0]
        z1 = ox.multvae_encode(cu(Wq_t, dev), cu(bq, dev), s, batch, state, SEED, False, 0.5, None, None, cu(eps, dev))[0]
        assert same_bits(host(z2), host(z1)[p]), "encode z does not move with the batch"
    t.done()


# ---------------------------------------------------------------------------------------------------------------
# MacridVAE
# ---------------------------------------------------------------------------------------------------------------
def macrid_mix_run(ox, dev, st, zh, items, cates, gce, users=None, junk=False):
    s, batch = on_device(st, dev, users)
    zt = cu(zh, dev, True)
    it, ct = (with_junk(items, dev).requires_grad_(True), with_junk(cates, dev).requires_grad_(True)) if junk else (cu(items, dev, True), cu(cates, dev, True))
    ce, lse = ox.macrid_mix(zt, it, ct, s, batch, 0.1)
    backward(((ce, gce),))
    return dict(ce=host(ce), lse=host(lse), zh=host(zt.grad), items=host(it.grad), cates=host(ct.grad))


@pytest.mark.parametrize("B,I", CASES)
def test_macrid_ops(dev, B, I):
    from chaorec_amd import _lib, ops_extra as ox
    st = make_structure(B, I)
    rng = np.random.default_rng(11 * B + I)
    users, x = st["users"], vo.dense_rows(st["rowptr"], st["col"], st["users"], I)
    s, batch = on_device(st, dev)
    state = torch.tensor([7, 7], dtype=torch.int64, device=dev)
    K, D, H = vo.MACRID_K, vo.MACRID_D, vo.MACRID_H
    t = Table(f"macrid B={B} I={I}")

    # concept, given Gumbel noise
    E, Kemb = signed(rng, I, D), signed(rng, K, D)
    gumbel = np.ascontiguousarray(-np.log(-np.log(rng.uniform(1e-3, 1 - 1e-3, (I, K)))), dtype=np.float32)
    d_items, d_cates = signed(rng, I, D), signed(rng, I, K)
    Et, Kt = cu(E, dev, True), cu(Kemb, dev, True)
    items_o, cates_o = ox.macrid_concept(Et, Kt, 0.1, state, SEED, True, cu(gumbel, dev))
    backward(((items_o, cu(d_items, dev)), (cates_o, cu(d_cates, dev))))
    o64, g64, o32, g32 = both(vo.macrid_concept_fwd, dict(E=E, Kemb=Kemb, gumbel=gumbel), ("E", "Kemb"),
                              {"items": d_items, "cates": d_cates}, tau=0.1)
    t.check(host(items_o), o64["items"], o32["items"], "concept items")
    t.check(host(cates_o), o64["cates"], o32["cates"], "concept cates")
    t.check(host(Et.grad), g64["E"], g32["E"], "concept dE")
    t.check(host(Kt.grad), g64["Kemb"], g32["Kemb"], "concept dKemb")

    # encode, given keep flags
    W1_t, b1, cates = signed(rng, I, H, scale=0.5), signed(rng, H, scale=0.3), softmax_rows(rng.standard_normal((I, K)) * 2)
    flags, mask = flags_and_mask(rng, st)
    da = signed(rng, B, K, H)
    Wt, bt, ct = cu(W1_t, dev, True), cu(b1, dev, True), cu(cates, dev, True)
    a = ox.macrid_encode(Wt, bt, ct, s, batch, state, SEED, True, 0.5, cu(flags, dev), s.keep_offsets(batch[0]))
    backward(((a, cu(da, dev)),))
    o64, g64, o32, g32 = both(vo.macrid_encode_fwd, dict(W1_t=W1_t, b1=b1, cates=cates, x=x, mask=mask), ("W1_t", "b1", "cates"),
                              {"a": da}, keep_prob=0.5, training=True)
    t.check(host(a), o64["a"], o32["a"], "encode a")
    for k, got in (("W1_t", Wt), ("b1", bt), ("cates", ct)):
        t.check(host(got.grad), g64[k], g32[k], f"encode d{k}")
    assert not host(Wt.grad)[st["dead"]].any() and not host(ct.grad)[st["dead"]].any(), "the untouched item's rows of dW / dc are not 0"

    # mix
    zh, items = unit(rng.standard_normal((B, K, D))), unit(rng.standard_normal((I, D)))
    gce = float(np.float32(rng.standard_normal()))
    check_plan(int(_lib.load().chaorec_macrid_mix_splits(B, I)), I)
    out = macrid_mix_run(ox, dev, st, zh, items, cates, gce)
    o64, g64, o32, g32 = both(vo.macrid_mix_fwd, dict(zh=zh, items=items, cates=cates, x=x), ("zh", "items", "cates"), {"ce": gce}, tau=0.1)
    t.check(out["ce"].reshape(()), o64["ce"], o32["ce"], "mix ce")
    t.check(out["lse"], o64["lse"], o32["lse"], "mix lse")
    for k in ("zh", "items", "cates"):
        t.check(out[k], g64[k], g32[k], f"mix d{k}")
    junk = macrid_mix_run(ox, dev, st, zh, items, cates, gce, junk=True)
    for k in out:
        assert same_bits(out[k], junk[k]), f"mix {k} moved with junk rows behind I"
    if B > 1:
        p = rng.permutation(B)
        perm = macrid_mix_run(ox, dev, st, zh[p], items, cates, gce, users=users[p])
        assert same_bits(perm["lse"], out["lse"][p]) and same_bits(perm["zh"], out["zh"][p]), "mix lse / dzh do not move with the batch"
    t.done()


# ---------------------------------------------------------------------------------------------------------------
# DualVAE
# ---------------------------------------------------------------------------------------------------------------
def dualvae_dense_run(ox, dev, st, z, zh, th, w, table, g1, g2, gN, ids=None, junk=False):
    s, batch = on_device(st, dev, ids)
    zt, zht = cu(z, dev, True), cu(zh, dev, True)
    tht, wt, tab = (with_junk(th, dev).requires_grad_(True), with_junk(w, dev).requires_grad_(True), with_junk(table, dev)) if junk \
        else (cu(th, dev, True), cu(w, dev, True), cu(table, dev))
    sum_p, xlog, nei = ox.dualvae_dense(zt, zht, tht, wt, tab, s, batch)
    backward(((sum_p, cu(g1, dev)), (xlog, cu(g2, dev)), (nei, cu(gN, dev))))
    return dict(sum_p=host(sum_p), xlog=host(xlog), nei=host(nei), z=host(zt.grad), zh=host(zht.grad), th=host(tht.grad), w=host(wt.grad))


@pytest.mark.parametrize("B,N", CASES)
def test_dualvae_ops(dev, B, N):
    from chaorec_amd import _lib, ops_extra as ox
    st = make_structure(B, N)
    rng = np.random.default_rng(13 * B + N)
    ids, x = st["users"], vo.dense_rows(st["rowptr"], st["col"], st["users"], N)
    s, batch = on_device(st, dev)
    A, K, H = vo.DUALVAE_A, vo.DUALVAE_K, vo.DUALVAE_H
    t = Table(f"dualvae B={B} N={N}")

    # encode
    We_t, bias, w = signed(rng, N, H, scale=0.5), signed(rng, H, scale=0.3), softmax_rows(rng.standard_normal((N, A)) * 2)
    dpre = signed(rng, B, A, H)
    Wt, bt, wt = cu(We_t, dev, True), cu(bias, dev, True), cu(w, dev, True)
    pre = ox.dualvae_encode(Wt, bt, wt, s, batch)
    backward(((pre, cu(dpre, dev)),))
    o64, g64, o32, g32 = both(vo.dualvae_encode_fwd, dict(We_t=We_t, bias=bias, w=w, x=x), ("We_t", "bias", "w"), {"pre": dpre})
    t.check(host(pre), o64["pre"], o32["pre"], "encode pre")
    for k, got in (("We_t", Wt), ("w", wt)):
        t.check(host(got.grad), g64[k], g32[k], f"encode d{k}")
    print(f"(encode dbias under the 4 x measure: kernel {vo.row_dev(host(bt.grad), g64['bias']):.3e}, bound {vo.bound_of(g32['bias'], g64['bias']):.3e})")
    t.check_sum(host(bt.grad), g64["bias"], dpre.reshape(B * A, H), "encode dbias")
    assert not host(Wt.grad)[st["dead"]].any() and not host(wt.grad)[st["dead"]].any(), "the untouched row's dWe_t / dw are not 0"

    # dense
    z, table = signed(rng, B, A, K, scale=0.5, decades=1.0), signed(rng, N, A, K, scale=0.5, decades=1.0)
    zh, th = np.tanh(signed(rng, B, A, H, decades=1.0)), np.tanh(signed(rng, N, A, H))
    g1, g2, gN = signed(rng, B), signed(rng, B), signed(rng, B, A, K)
    check_plan(int(_lib.load().chaorec_dualvae_splits(B, N)), N)
    out = dualvae_dense_run(ox, dev, st, z, zh, th, w, table, g1, g2, gN)
    o64, g64, o32, g32 = both(vo.dualvae_dense_fwd, dict(z=z, zh=zh, th=th, w=w, table=table, x=x), ("z", "zh", "th", "w"),
                              {"sum_p": g1, "xlog": g2, "nei": gN})
    for k in ("sum_p", "xlog", "nei"):
        t.check(out[k], o64[k], o32[k], f"dense {k}")
    for k in ("z", "zh", "th", "w"):
        t.check(out[k], g64[k], g32[k], f"dense d{k}")
    junk = dualvae_dense_run(ox, dev, st, z, zh, th, w, table, g1, g2, gN, junk=True)
    for k in out:
        assert same_bits(out[k], junk[k]), f"dense {k} moved with junk rows behind N"
    if B > 1:
        p = rng.permutation(B)
        perm = dualvae_dense_run(ox, dev, st, z[p], zh[p], th, w, table, g1[p], g2[p], gN[p], ids=ids[p])
        for k in ("sum_p", "xlog", "nei", "z", "zh"):
            assert same_bits(perm[k], out[k][p]), f"dense {k} does not move with the batch"
    t.done()


@pytest.mark.parametrize("R", [2047, 2049])
def test_dualvae_linear(dev, R):
    """Both sides of the weight gradient's 2048-row split."""
    from chaorec_amd import ops_extra as ox
    assert R in (vo.DUALVAE_LINEAR_SPLIT - 1, vo.DUALVAE_LINEAR_SPLIT + 1)
    rng = np.random.default_rng(R)
    x, weight, bias, gy = signed(rng, R, 20), signed(rng, 25, 20), signed(rng, 25), signed(rng, R, 25)
    xt, wt, bt = cu(x, dev, True), cu(weight, dev, True), cu(bias, dev, True)
    y = ox.dualvae_linear(xt, wt, bt)
    backward(((y, cu(gy, dev)),))
    o64, g64, o32, g32 = both(vo.dualvae_linear_fwd, dict(x=x, weight=weight, bias=bias), ("x", "weight", "bias"), {"y": gy})
    t = Table(f"dualvae_linear R={R}")
    t.check(host(y), o64["y"], o32["y"], "y")
    for k, got in (("x", xt), ("weight", wt), ("bias", bt)):
        t.check(host(got.grad), g64[k], g32[k], f"d{k}")
    t.done()


@pytest.mark.parametrize("B", [1, 129])
def test_dualvae_loss(dev, B):
    from chaorec_amd import ops_extra as ox
    rng = np.random.default_rng(B)
    A, K = vo.DUALVAE_A, vo.DUALVAE_K
    inp = dict(mu=signed(rng, B * A, K), std_pre=signed(rng, B * A, K, scale=2.0), xlog=signed(rng, B, scale=5.0),
               sum_p=signed(rng, B, scale=5.0), cl=np.float32(rng.standard_normal()))
    g = np.array([rng.standard_normal(), 0.0, 0.0], dtype=np.float32)          # (the gradient of element 0 only)
    ts = {k: cu(v, dev, True) if np.ndim(v) else torch.tensor(float(v), dtype=torch.float32, device=dev, requires_grad=True)
          for k, v in inp.items()}
    out = ox.dualvae_loss(ts["mu"], ts["std_pre"], ts["xlog"], ts["sum_p"], ts["cl"], 0.02, 0.05)
    backward(((out, cu(g, dev)),))
    o64, g64, o32, g32 = both(vo.dualvae_loss_fwd, inp, tuple(inp), {"out": g}, kl_weight=0.02, ssl_reg=0.05)
    t = Table(f"dualvae_loss B={B}")
    t.check(host(out), o64["out"], o32["out"], "out")
    for k in inp:
        t.check(host(ts[k].grad).reshape(g64[k].shape), g64[k], g32[k], f"d{k}")
    t.done()


# ---------------------------------------------------------------------------------------------------------------
# device draws
# ---------------------------------------------------------------------------------------------------------------
DRAW_B, DRAW_I, DRAW_STEP = 129, 100, 41


def draw_structure():
    return make_structure(DRAW_B, DRAW_I, 12, 24)


def check_mask(st, got, salt, bits, other):
    """The decoded [B, I] mask against the numpy restatement, flag for flag; and what a mask has to be."""
    users, x = st["users"], vo.dense_rows(st["rowptr"], st["col"], st["users"], st["I"]) != 0
    want = vo.predict_keep(SEED, DRAW_STEP, salt, bits, 0.5, st["rowptr"], st["col"], users, st["I"])
    assert not (got & ~x).any()
    assert np.array_equal(got, want), f"{(got != want).sum()} keep flags differ from the counter RNG's restatement"
    same_user = np.nonzero(users == st["rep"])[0]
    assert len(same_user) >= 3 and not np.array_equal(got[same_user[0]], got[same_user[1]]), "two samples of one user share a mask"
    assert not np.array_equal(got, other), "another state[1] gives the same mask"
    n, p = int(x.sum()), 0.5
    assert n >= 2000 and abs(got.sum() / n - p) <= 5 * np.sqrt(p * (1 - p) / n), f"kept share {got.sum() / n:.4f} of {n}"


def test_multvae_device_draws(dev):
    from chaorec_amd import ops_extra as ox
    st = draw_structure()
    B, I = DRAW_B, DRAW_I
    rng = np.random.default_rng(99)
    s, batch = on_device(st, dev)
    state = torch.tensor([DRAW_STEP + 1, DRAW_STEP], dtype=torch.int64, device=dev)
    # 1. decode: one-hot Wq_t, zero bias -> h[b, i] = s_b keep(b, i)
    onehot = np.zeros((I, 128), dtype=np.float32)
    onehot[np.arange(I), np.arange(I)] = 1.0
    zero = np.zeros(128, dtype=np.float32)
    h = ox.multvae_encode(cu(onehot, dev), cu(zero, dev), s, batch, state, SEED, True, 0.5)[3]
    got = host(h)[:, :I] != 0
    state2 = torch.tensor([DRAW_STEP + 2, DRAW_STEP + 1], dtype=torch.int64, device=dev)
    other = host(ox.multvae_encode(cu(onehot, dev), cu(zero, dev), s, batch, state2, SEED, True, 0.5)[3])[:, :I] != 0
    # 2. against the restatement
    check_mask(st, got, vo.MULTVAE_SALT_KEEP, vo.MULTVAE_BITS, other)
    # 3. forward and backward under the decoded mask
    Wq_t, bq = signed(rng, I, 128, scale=0.5), signed(rng, 128, scale=0.3)
    gz, gkl, gsq = signed(rng, B, 64), np.float32(rng.standard_normal()), np.float32(rng.standard_normal())
    Wt, bt = cu(Wq_t, dev, True), cu(bq, dev, True)
    z, kl, sq, h, eps_out = ox.multvae_encode(Wt, bt, s, batch, state, SEED, True, 0.5)
    backward(((z, cu(gz, dev)), (kl, float(gkl)), (sq, float(gsq))))
    eps = host(eps_out)
    x = vo.dense_rows(st["rowptr"], st["col"], st["users"], I)
    o64, g64, o32, g32 = both(vo.multvae_encode_fwd, dict(Wq_t=Wq_t, bq=bq, x=x, mask=got.astype(np.float64), eps=eps), ("Wq_t", "bq"),
                              {"z": gz, "kl": gkl, "sumsq": gsq}, keep_prob=0.5, training=True)
    t = Table("multvae device draws")
    t.check(host(h), o64["h"], o32["h"], "h")
    t.check(host(Wt.grad), g64["Wq_t"], g32["Wq_t"], "dWq_t")
    t.check(host(bt.grad), g64["bq"], g32["bq"], "dbq")
    # 4. eps_out is what z was built from; N(0, 1) draws
    t.check(host(z), o64["z"], o32["z"], "z = mu + eps_out exp(logvar / 2)")
    assert np.isfinite(eps).all() and abs(float(eps.mean())) < 0.05 and abs(float(eps.std()) - 1.0) < 0.05
    t.done()


def test_macrid_device_draws(dev):
    from chaorec_amd import ops_extra as ox
    st = draw_structure()
    B, I, K, H = DRAW_B, DRAW_I, vo.MACRID_K, vo.MACRID_H
    rng = np.random.default_rng(98)
    s, batch = on_device(st, dev)
    state = torch.tensor([DRAW_STEP, DRAW_STEP], dtype=torch.int64, device=dev)
    onehot = np.zeros((I, H), dtype=np.float32)
    onehot[np.arange(I), np.arange(I)] = 1.0
    zero, ones = np.zeros(H, dtype=np.float32), np.ones((I, K), dtype=np.float32)
    a = host(ox.macrid_encode(cu(onehot, dev), cu(zero, dev), cu(ones, dev), s, batch, state, SEED, True, 0.5))
    got = a[:, 0, :I] != 0
    for k in range(1, K):
        assert np.array_equal(a[:, k, :I] != 0, got), "the concepts of one sample see different masks"
    state2 = torch.tensor([DRAW_STEP + 1, DRAW_STEP + 1], dtype=torch.int64, device=dev)
    other = host(ox.macrid_encode(cu(onehot, dev), cu(zero, dev), cu(ones, dev), s, batch, state2, SEED, True, 0.5))[:, 0, :I] != 0
    check_mask(st, got, vo.MACRID_SALT_KEEP, vo.MACRID_BITS, other)
    W1_t, b1, cates = signed(rng, I, H, scale=0.5), signed(rng, H, scale=0.3), softmax_rows(rng.standard_normal((I, K)) * 2)
    da = signed(rng, B, K, H)
    Wt, bt, ct = cu(W1_t, dev, True), cu(b1, dev, True), cu(cates, dev, True)
    a = ox.macrid_encode(Wt, bt, ct, s, batch, state, SEED, True, 0.5)
    backward(((a, cu(da, dev)),))
    x = vo.dense_rows(st["rowptr"], st["col"], st["users"], I)
    o64, g64, o32, g32 = both(vo.macrid_encode_fwd, dict(W1_t=W1_t, b1=b1, cates=cates, x=x, mask=got.astype(np.float64)),
                              ("W1_t", "b1", "cates"), {"a": da}, keep_prob=0.5, training=True)
    t = Table("macrid device draws")
    t.check(host(a), o64["a"], o32["a"], "a")
    for k, g in (("W1_t", Wt), ("b1", bt), ("cates", ct)):
        t.check(host(g.grad), g64[k], g32[k], f"d{k}")
    t.done()
