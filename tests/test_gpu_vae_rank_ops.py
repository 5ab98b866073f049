"""The autoencoders' RANKING kernels on the MI355X, op by op: chaorec_macrid_scores_f32 (mc_items_kernel<true> of
csrc/macridvae.hip), chaorec_dualvae_scores_f32 (dv_table_kernel<true> of csrc/dualvae.hip), vae_mask_kernel of
csrc/vae_common.h behind both, chaorec_macrid_topk_f32 (ops.rows_topk, k <= 64) and chaorec_dualvae_writeback_f32 -- the
evaluation half of the files whose training half tests/test_gpu_vae_ops.py covers.  Inputs are built here from a seeded numpy
generator: unit rows for zh / items, a softmax for cates, tau = 0.1; signed z / table at scale 0.5, tanh of Gaussians for
zh / th, a signed w.

Scores.  (n, I): n in {1, 33, 128, 129, 257} (one lane, a wave boundary, VAE_SB, VAE_SB + 1, a third row block -- which
mc_items_kernel loops over inside the workgroup and dv_table_kernel takes as blockIdx.y) x I in {63, 64, 65, 129, 1003}
(VAE_TW and its neighbours, a third tile, 16 tiles with a last one of 43), not the full product: every n meets 1003 and one I
near 64, every I meets n = 129.  Each with user_begin in {0, 37, U_TOTAL - n}: 37 is no multiple of the mask kernel's four
users per workgroup, the last one ends the range at the last user.  The history CSR (int64, 300 users, columns ascending)
gives user u the row type u % 8: random, empty, every item, {0, I - 1}, 130 entries (three trips of the 64-lane walk; drawn
with repeats where I < 130), a stray column -1 in front, a stray column I behind, random.  The block under test is an interior
slice of a sentinel-filled allocation, one spare row before and one after it, and for odd n two more rows than the range
needs: a failed guard lands on a sentinel, never outside the tensor.

Per case: the unmasked entries by accept.within_measured (4 x max(own, 2^-24) of the largest score, `own` = the fp32 run of
vae_ops_host.macrid_scores / dualvae_scores against their fp64 run); the masked entries bit-equal to the mask value exactly
where vae_ops_host.masked() puts them for user user_begin + r and nowhere else; every sentinel row bit for bit as it was; two
runs the same bits; and (at user_begin = 37) the range [37, 37 + n) alone equal to rows 37 .. of the range [0, 37 + n).

Narrow top-k: ops.rows_topk against accept.numpy_topk (the sort by bit-pattern key the wide kernel is held to), ids and
values bit for bit, at I = k, I = k + 1 and both sides of the 256-element pass.  Writeback: the highest batch position wins,
every other row keeps its sentinel.  Refused arguments raise and write nothing.

Largest kernel deviation / bound, measured on the MI355X over all cases (1.0 = at the bound):
  macrid scores  0.74 (n=1 I=63: deviation 4.3e-7 of the largest score, the restatement's own 1.4e-7; 0.21 .. 0.74 over
                 the cases)
  dualvae scores 0.36 (n=33 I=1003: deviation 1.4e-7, own 1.0e-7; 0.25 .. 0.36 over the cases, 0.25 where the kernel
                 deviates exactly as the fp32 restatement does)
Both stay under 1.0 with the plain fp32 run of the restatements as `ref32`; no k-ascending chain was needed."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import vae_ops_host as vo  # noqa: E402
from accept import bits, numpy_topk, same_bits  # noqa: E402
from test_gpu_vae_ops import cu, host, signed, softmax_rows, unit  # noqa: E402

pytestmark = pytest.mark.gpu

U_TOTAL = 300
PRE = 37                    # the odd user_begin, and the rows in front of a range that is also scored from user 0
MASK = 1e-6
SENTINEL = -12345.0
TAU = 0.1
SHAPES = [(1, 63), (1, 1003), (33, 64), (33, 1003), (128, 65), (128, 1003), (129, 63), (129, 64), (129, 65), (129, 129),
          (129, 1003), (257, 64), (257, 1003)]
BEGINS = ["0", "37", "last"]
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------
# the history, the inputs and their references (built once per shape, never written to)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def history(I):
    """-> rowptr [U_TOTAL + 1], col, both int64; user u's row is of type u % 8 (see the file's docstring)."""
    rng = np.random.default_rng(500 + I)

    def some():
        return np.sort(rng.choice(I, size=int(rng.integers(1, min(I, 12) + 1)), replace=False))

    rows = []
    for u in range(U_TOTAL):
        kind = u % 8
        if kind == 1:
            r = np.zeros(0)
        elif kind == 2:
            r = np.arange(I)
        elif kind == 3:
            r = np.array([0, I - 1])
        elif kind == 4:
            r = np.sort(rng.choice(I, size=130, replace=False) if I >= 130 else rng.integers(0, I, size=130))
        elif kind == 5:
            r = np.concatenate(([-1], some()))
        elif kind == 6:
            r = np.concatenate((some(), [I]))
        else:
            r = some()
        rows.append(r.astype(np.int64))
    rowptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    return rowptr, np.concatenate(rows)


def begin_of(which, n):
    return {"0": 0, "37": PRE, "last": U_TOTAL - n}[which]


def run_both(fn, inputs, **const):
    """The restatement `fn` on the float32 inputs in float64 and in float32 -> two float64-comparable numpy arrays."""
    out = []
    for dt in (torch.float64, torch.float32):
        out.append(fn(*(torch.from_numpy(x).to(dt) for x in inputs), **const).numpy())
    return out


@functools.lru_cache(maxsize=None)
def macrid_case(n, I):
    """Inputs for PRE + n users (the first PRE only ride along where the range is also scored from user 0) and the
    references of the last n."""
    rng = np.random.default_rng(17 * n + I)
    K, D = vo.MACRID_K, vo.MACRID_D
    zh, items = unit(rng.standard_normal((PRE + n, K, D))), unit(rng.standard_normal((I, D)))
    cates = softmax_rows(rng.standard_normal((I, K)) * 2)
    ref64, ref32 = run_both(vo.macrid_scores, (zh[PRE:], items, cates), tau=TAU)
    return (zh, items, cates), ref64, ref32


@functools.lru_cache(maxsize=None)
def dualvae_case(n, I):
    rng = np.random.default_rng(19 * n + I)
    A, K, H = vo.DUALVAE_A, vo.DUALVAE_K, vo.DUALVAE_H
    z, table = signed(rng, PRE + n, A, K, scale=0.5, decades=0), signed(rng, I, A, K, scale=0.5, decades=0)
    zh, th = np.tanh(signed(rng, PRE + n, A, H, decades=0)), np.tanh(signed(rng, I, A, H, decades=0))
    w = signed(rng, I, A, decades=0)
    ref64, ref32 = run_both(vo.dualvae_scores, (z[PRE:], zh[PRE:], table, th, w))
    return (z, zh, table, th, w), ref64, ref32


def macrid_launch(ops, dev, inputs, rows, user_begin, hist, out):
    zh, items, cates = inputs
    return ops.macrid_scores(cu(zh[rows], dev), cu(items, dev), cu(cates, dev), TAU, user_begin, hist, MASK, out=out)


def dualvae_launch(ops, dev, inputs, rows, user_begin, hist, out):
    z, zh, table, th, w = inputs
    return ops.dualvae_scores(cu(z[rows], dev), cu(zh[rows], dev), cu(table, dev), cu(th, dev), cu(w, dev), user_begin, hist, MASK,
                              out=out)


def staged(dev, rows, I):
    """-> (the whole allocation [1 + rows + 1, I], filled with the sentinel; its interior [rows, I])."""
    big = torch.full((rows + 2, I), SENTINEL, dtype=torch.float32, device=dev)
    return big, big[1:1 + rows]


def check_scores(op, launch, case, dev, n, I, which):
    from chaorec_amd import ops
    inputs, ref64, ref32 = case(n, I)
    rowptr, col = history(I)
    hist = (cu(rowptr, dev), cu(col, dev))
    ub = begin_of(which, n)
    rows = n if n % 2 == 0 else n + 2                       # odd n: a staging block longer than the range
    tail = slice(PRE, PRE + n)
    big, block = staged(dev, rows, I)
    ret = launch(ops, dev, inputs, tail, ub, hist, block)
    assert ret.data_ptr() == block.data_ptr()
    whole = host(big)
    got = whole[1:1 + n]

    # every row that is not the range's: as it was
    untouched = np.full((1, I), SENTINEL, dtype=np.float32)
    assert same_bits(whole[:1], untouched), "the row in front of the block was written"
    assert same_bits(whole[1 + n:], np.repeat(untouched, rows + 1 - n, 0)), "a row behind the range was written"

    # the mask: user user_begin + r's history in row r, bit-equal, and nowhere else
    pos = vo.masked(np.zeros((n, I), dtype=bool), rowptr, col, ub, True)
    mask_bits = bits(np.float32(MASK))
    assert np.array_equal(bits(got[pos]), np.broadcast_to(mask_bits, (int(pos.sum()),))), "a history entry is not the mask value"
    assert not (bits(got[~pos]) == mask_bits).any(), "the mask value outside the history"
    assert same_bits(got, vo.masked(got, rowptr, col, ub, np.float32(MASK)))

    # the scores
    ratio = accept.within_measured(f"{op} scores n={n} I={I} user_begin={ub}", got[~pos], ref32[~pos], ref64[~pos], accept.ULP24)
    if ratio > WORST.get(op, (0.0, ""))[0]:
        WORST[op] = (ratio, f"n={n} I={I} user_begin={ub}")
    print(f"{op} scores: largest kernel / bound ratio so far {WORST[op][0]:.3f} ({WORST[op][1]})")

    # again: the same bits
    big2, block2 = staged(dev, rows, I)
    launch(ops, dev, inputs, tail, ub, hist, block2)
    assert same_bits(host(big2), whole), "two runs differ"

    # rows do not depend on where the range starts: [0, PRE + n) against [PRE, PRE + n) alone
    if ub == PRE:
        big3, block3 = staged(dev, PRE + n, I)
        launch(ops, dev, inputs, slice(0, PRE + n), 0, hist, block3)
        assert same_bits(host(big3)[1 + PRE:1 + PRE + n], got), "a row moved with the start of its range"


@pytest.mark.parametrize("which", BEGINS)
@pytest.mark.parametrize("n,I", SHAPES)
def test_macrid_scores(dev, n, I, which):
    check_scores("macrid", macrid_launch, macrid_case, dev, n, I, which)


@pytest.mark.parametrize("which", BEGINS)
@pytest.mark.parametrize("n,I", SHAPES)
def test_dualvae_scores(dev, n, I, which):
    check_scores("dualvae", dualvae_launch, dualvae_case, dev, n, I, which)


# ---------------------------------------------------------------------------------------------------------------
# refused arguments: an error, and nothing written
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["macrid", "dualvae"])
def test_scores_refuse_without_a_launch(dev, monkeypatch, op):
    from chaorec_amd import ops, ops_vae
    n, I = 33, 64
    launch, case = (macrid_launch, macrid_case) if op == "macrid" else (dualvae_launch, dualvae_case)
    inputs = case(n, I)[0]
    rowptr, col = history(I)
    hist = (cu(rowptr, dev), cu(col, dev))
    tail = slice(PRE, PRE + n)
    big, block = staged(dev, n, I)

    def refused(exc, match, inputs=inputs, hist=hist, out=block):
        with pytest.raises(exc, match=match):
            launch(ops, dev, inputs, tail, 0, hist, out)
        torch.cuda.synchronize()
        assert bool((big == SENTINEL).all()), f"{match}: refused, and yet something was written"

    refused(RuntimeError, rf"{op}_scores: staging of {n * I * 4} bytes \(given {n * I * 4 - 4}", out=block.view(-1)[:n * I - 1])
    refused(ValueError, "history CSR must be int64", hist=(hist[0], hist[1].to(torch.int32)))
    refused(ValueError, "history CSR must be int64", hist=(hist[0].to(torch.int32), hist[1]))
    if op == "macrid":
        zh, items, cates = inputs
        refused(ValueError, "dim_E=32", inputs=(np.ascontiguousarray(zh[..., :32]), np.ascontiguousarray(items[:, :32]), cates))
        refused(ValueError, "kfac=9", inputs=(np.ascontiguousarray(zh[:, :9]), items, np.ascontiguousarray(cates[:, :9])))
    else:
        z, zh, table, th, w = inputs
        refused(ValueError, r"dualvae: z is \(33, 5, 24\)", inputs=(np.ascontiguousarray(z[..., :24]), zh, table, th, w))
        refused(ValueError, r"dualvae: th is \(64, 5, 19\)", inputs=(z, zh, table, np.ascontiguousarray(th[..., :19]), w))
    monkeypatch.setattr(ops_vae, f"{op.upper()}_STAGING_BYTES", (n - 1) * I * 4)
    refused(ValueError, rf"{n} users x {I} items exceed the staging cap of {(n - 1) * I * 4} bytes")


# ---------------------------------------------------------------------------------------------------------------
# the narrow selection
# ---------------------------------------------------------------------------------------------------------------
def topk_rows(n, I, k):
    """Row r is of kind r % 6: the k-th boundary cutting a tie group; every 7th entry the mask value; +0 and -0 mixed into
    small values of both signs; +inf and -inf; one value; all negative."""
    rng = np.random.default_rng(n + I + k)
    x = rng.standard_normal((n, I)).astype(np.float32)
    for r in range(n):
        kind = r % 6
        if kind == 0:
            above = k // 2                                  # fewer than k values above a tie group that reaches past k
            where = rng.permutation(I)
            x[r] = -3.0 - rng.random(I).astype(np.float32)
            x[r, where[:above]] = 2.0 + rng.random(above).astype(np.float32)
            x[r, where[above:above + min(I - above, k + 5)]] = 1.0
        elif kind == 1:
            x[r, ::7] = MASK
        elif kind == 2:
            where, q = rng.permutation(I), k // 4              # q positive values, q times +0, then -0: the k-th is a -0
            x[r] = -np.abs(x[r]) * 1e-3
            x[r, where[:q]] *= -1.0
            x[r, where[q:2 * q]], x[r, where[2 * q:2 * q + I // 2]] = 0.0, -0.0
        elif kind == 3:
            where = rng.permutation(I)[:8]
            x[r, where[:4]], x[r, where[4:]] = np.inf, -np.inf
        elif kind == 4:
            x[r] = 0.25
        else:
            x[r] = -np.abs(x[r]) - 0.1
    return x


@pytest.mark.parametrize("n,I,k", [(1, 64, 64), (129, 65, 64), (33, 255, 50), (33, 256, 1), (129, 257, 50), (4, 8449, 64)])
def test_rows_topk_narrow_against_numpy(dev, n, I, k):
    from chaorec_amd import ops
    x = topk_rows(n, I, k)
    ref_idx, ref_val = numpy_topk(x, k)
    if I > k:
        more = numpy_topk(x, k + 1)[1]
        assert more[0, k - 1] == more[0, k] == 1.0, "the k-th boundary is meant to cut a tie group"
    if n > 2:
        assert (bits(ref_val[2]) == 0x80000000).any(), "-0 is meant to be among the winners"
    idx, val = ops.rows_topk(cu(x, dev), k, id_offset=11)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (n, k) and val.dtype == torch.float32
    assert np.array_equal(host(idx), ref_idx + 11)
    assert np.array_equal(bits(host(val)), bits(ref_val))
    again = ops.rows_topk(cu(x, dev), k, id_offset=11)
    assert torch.equal(idx, again[0]) and accept.same_bits_t(val, again[1])


# ---------------------------------------------------------------------------------------------------------------
# the write-back behind DualVAE's ranking tables
# ---------------------------------------------------------------------------------------------------------------
def test_dualvae_writeback_highest_position_wins(dev):
    from chaorec_amd import ops
    B, S = 129, 150
    A, K = vo.DUALVAE_A, vo.DUALVAE_K
    rng = np.random.default_rng(B + S)
    thrice, absent = 7, 20
    others = rng.choice(np.setdiff1d(np.arange(S - 1), [thrice, absent]), size=B - 4, replace=False)
    ids = rng.permutation(np.concatenate((others, [thrice] * 3, [S - 1]))).astype(np.int64)
    assert len(ids) == B and (ids == thrice).sum() == 3 and absent not in ids and S - 1 in ids
    z, mu = signed(rng, B, A, K), signed(rng, B, A, K)
    t_ids = torch.from_numpy(ids)
    sorted_ids, perm = torch.sort(t_ids, stable=True)
    slot_ptr = torch.searchsorted(sorted_ids, torch.arange(S + 1, dtype=torch.int64))
    batch = (t_ids.to(dev), slot_ptr.contiguous().to(dev), perm.contiguous().to(dev))
    whole = [torch.full((S + 2, A, K), SENTINEL, dtype=torch.float32, device=dev) for _ in range(2)]
    ops.dualvae_writeback(batch, S, cu(z, dev), cu(mu, dev), whole[0][1:1 + S], whole[1][1:1 + S])
    for name, got, rows in (("table", whole[0], z), ("mu_table", whole[1], mu)):
        want = np.full((S + 2, A, K), SENTINEL, dtype=np.float32)
        for b in range(B):                                  # ascending: the highest position is the last to write
            want[1 + ids[b]] = rows[b]
        assert same_bits(want[1 + thrice], rows[np.nonzero(ids == thrice)[0].max()])
        assert same_bits(host(got), want), f"{name}: rows {np.nonzero((host(got) != want).any((1, 2)))[0] - 1} differ"
