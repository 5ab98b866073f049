"""BSPM on the MI355X: the three launches of csrc/bspm.hip per operand, and the whole model against the golden the reference's
own run left (tests/golden/bspm_small.npz).

Tolerance, measured not chosen (accept.within): for each compared array bound = 4 x max(own, ULP), `own`
the stored fp32 reference's deviation from the float64 restatement and ULP fp32 epsilon, both relative to the largest magnitude
of the float64 array.  Every check prints deviation, own, bound and ratio; the per-operand checks compare against float64
evaluated on the operands the kernel was given (the reference's fp32 Rn and P), so their deviation is the kernel's arithmetic
alone.

The case has the three shapes at which the kernels take another path: item 0's row of P is full (140 entries > the long-row
length 128: shared by the four waves), the other rows are short; tile widths 32 and 8 (70 users = 2 x 32 + 6, the tail padded
with two empty slots); a user without history; ten items with empty rows; I = 150 is 4 tiles of 32 items and a tail of 22.

Measured on the MI355X (deviation / bound): project 0.10, seed 0.21, last step 0.14 at most; the whole model 0.22, 0.58 and 0.28
for the three cases (the plain composition: 0.39, 0.58, 0.28), fused against plain 0.35 at most."""
import functools
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import bspm_host as bh  # noqa: E402
from conftest import GOLDEN, tie_aware_rank_equal  # noqa: E402

from chaorec_amd import ops  # noqa: E402
from chaorec_amd.Model import BSPM  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILES = ((0, 32, 32), (32, 64, 32), (64, 70, 8))        # (first user, one past the last, width B)
WIDTHS = (32, 8)


@functools.lru_cache(maxsize=None)
def case():
    g = bh.load_fixture(GOLDEN)
    edges, I = g["edges"].astype(np.int64), int(g["I"])
    Rn64, _, di = bh.normalised(edges, I)
    ptr = g["p_ptr"].astype(np.int64)
    P = np.zeros((I, I))
    P[np.repeat(np.arange(I), np.diff(ptr)), g["p_col"].astype(np.int64)] = g["p_val"].astype(np.float64)   # the reference's fp32 P
    X = Rn64.astype(np.float32).astype(np.float64)                                                        # ... and its fp32 Rn
    return g, edges, I, P, X, di


@functools.lru_cache(maxsize=None)
def model(c=0, fused=True):
    g, edges, I = case()[:3]
    K_s, T_s, beta = bh.CASES[c]
    return BSPM(bh.U, I, edges, bh.user_item_dict(edges), K_s, T_s, 1, 1, beta, DEV, factor_dim=bh.FACTOR, factors=g["Vi"], fused=fused)


def tiles(width):
    m = model()
    return [(u0, u1, m.tile(torch.arange(u0, u1, dtype=torch.int64, device=DEV), B)) for u0, u1, B in TILES if B == width]


def within(what, got, ref, own, scale=None):
    return accept.within(what, got, ref, own, bh.ULP, scale=scale)


def host_idl(c, u0, u1, B):
    """idlT [I, B] fp32 of the tile, from the float64 projection (an INPUT of the seed's per-operand test)."""
    g, _, I, _, X, di = case()
    Z = X[u0:u1] @ (di[:, None] * g["Vi"])
    out = np.zeros((I, B), dtype=np.float32)
    out[:, :u1 - u0] = ((g["Vi"] / di[:, None]) @ Z.T).astype(np.float32)
    return out


# ---- per operand --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_project(width):
    g, _, I, _, X, _ = case()
    F = model().filter.F
    ref_all = X @ F.cpu().numpy().astype(np.float64)
    for u0, u1, t in tiles(width):
        Z = ops.bspm_project(t, F).cpu().numpy()
        assert Z.shape == (width, bh.FACTOR // 2) and not Z[u1 - u0:].any()               # empty slots: exact zeros
        within(f"project B={width} users {u0}..{u1}", Z[:u1 - u0], ref_all[u0:u1], g["own_project"], np.abs(ref_all).max())
        if u1 == bh.U:
            assert not Z[u1 - u0 - 1].any()                                             # the user without history


@pytest.mark.parametrize("beta,c", [(0.0, 2), (0.7, 1)])
@pytest.mark.parametrize("width", WIDTHS)
def test_seed(width, beta, c):
    g, _, I, P, X, _ = case()
    csr = model().filter.P
    scale = np.abs(g[f"host64_{c}"]).max()
    for u0, u1, t in tiles(width):
        idl = host_idl(c, u0, u1, width)
        Y = ops.bspm_seed(csr, t, beta, torch.from_numpy(idl).to(DEV) if beta else None)
        ref = beta * idl.astype(np.float64)
        ref[:, :u1 - u0] += P @ X[u0:u1].T
        assert Y.shape == (I, width)
        within(f"seed B={width} beta={beta} users {u0}..{u1}", Y.cpu().numpy(), ref, g[f"own_seed_{c}"], scale)
        assert not Y[:, u1 - u0:].any() and not Y[I - bh.EMPTY_ITEMS:].any()             # empty slots, items without users
        again = ops.bspm_seed(csr, t, beta, torch.from_numpy(idl).to(DEV) if beta else None)
        assert torch.equal(Y, again)                                                    # one owner, fixed order: the same bits
    with pytest.raises(ValueError, match="idl_beta=0.5 without idlT"):
        ops.bspm_seed(csr, tiles(width)[0][2], 0.5)


@pytest.mark.parametrize("h", [0.0, 0.75])
@pytest.mark.parametrize("width", WIDTHS)
def test_last_step(width, h):
    g, edges, I, P, X, _ = case()
    csr = model().filter.P
    assert int(csr.rowptr[1] - csr.rowptr[0]) == I - bh.EMPTY_ITEMS > ops.bspm_long_row()        # the full row is present
    seed64 = bh.item_route(edges, I, 2, 1.5, 0.7, g["Vi"], parts=True)[2]                         # case 1's seed: h = 0.75 is its step
    scale = np.abs(g["host64_1"]).max()
    for u0, u1, t in tiles(width):
        Yt = np.zeros((I, width), dtype=np.float32)
        Yt[:, :u1 - u0] = seed64[u0:u1].T
        Yt[:, u1 - u0:] = np.float32(0.03125)                                           # (empty slots: any value must come through)
        Yd = torch.from_numpy(Yt).to(DEV)
        out = ops.bspm_last_step(csr, Yd, h, t, bh.MASK)
        ref = (Yt.astype(np.float64) - h * (P @ Yt.astype(np.float64))).T
        hist = np.zeros((width, I), dtype=bool)
        e = edges[(edges[:, 0] >= u0) & (edges[:, 0] < u1)]
        hist[e[:, 0] - u0, e[:, 1] - bh.U] = True
        got = out.cpu().numpy()
        assert got.shape == (width, I) and (got[hist] == np.float32(bh.MASK)).all() and hist[:u1 - u0 - (u1 == bh.U), 0].all()
        if h:
            within(f"last_step B={width} h={h} users {u0}..{u1}", got[~hist], ref[~hist], g["own_1"], scale)
            unmasked = ops.bspm_last_step(csr, Yd, h).cpu().numpy()
            assert np.array_equal(unmasked[~hist], got[~hist])
            within(f"last_step unmasked B={width} users {u0}..{u1}", unmasked, ref, g["own_1"], scale)
        else:
            expect = Yt.T.copy()
            expect[hist] = np.float32(bh.MASK)
            assert np.array_equal(got.view(np.int32), expect.view(np.int32))            # h = 0: the masked transpose, bit for bit
    with pytest.raises(ValueError, match="B=6; the kernels tile a multiple of 4"):
        ops.bspm_last_step(csr, torch.zeros((I, 6), device=DEV), h)


def test_last_step_is_the_spmm_step():
    """The last step without a mask is the SpMM step the middle steps take (alpha = -h, beta = 1), transposed: the same epilogue,
    sums that may associate differently -- within 4 ULP of the largest entry."""
    g, edges, I, P, X, _ = case()
    csr = model().filter.P
    Yd = torch.randn((I, 32), device=DEV) * 0.05
    spmm = ops.spmm_raw(csr, Yd, alpha=-0.75, z=Yd, beta=1.0).t()
    last = ops.bspm_last_step(csr, Yd, 0.75)
    within("last_step against the SpMM step", last.cpu().numpy(), spmm.cpu().numpy().astype(np.float64), 0.0)


# ---- the whole model ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", range(len(bh.CASES)))
def test_model_against_the_golden(c):
    g, edges, I = case()[:3]
    host64, own = g[f"host64_{c}"], float(g[f"own_{c}"])
    users = np.arange(bh.U)
    fused = model(c).getUsersRating(users)
    assert fused.shape == (bh.U, I) and fused.dtype == torch.float32 and fused.is_cuda
    ratio = within(f"case {c} fused against float64", fused.cpu().numpy(), host64, own)
    within(f"case {c} fused against the reference's fp32", fused.cpu().numpy(), g[f"ref32_{c}"].astype(np.float64), 2 * own, np.abs(host64).max())
    plain = model(c, fused=False).getUsersRating(users)
    within(f"case {c} plain against float64", plain.cpu().numpy(), host64, own)
    within(f"case {c} fused against plain", fused.cpu().numpy(), plain.cpu().numpy().astype(np.float64), own, np.abs(host64).max())
    # the ranking: every row, ties aware, at the scores' bound
    bound = accept.bound_of(own, bh.ULP) * np.abs(host64).max()
    ref_idx = g[f"rank_{c}"].astype(np.int64)
    ref_val = np.take_along_axis(bh.masked(g[f"ref32_{c}"], edges), ref_idx - bh.U, 1)
    for mdl in (model(c), model(c, fused=False)):
        rank = mdl.gene_ranklist(bh.TOPK, to_cpu=False)
        assert rank.shape == (bh.U, bh.TOPK) and rank.dtype == torch.int64 and int(rank.min()) >= bh.U
        idx = rank.cpu().numpy()
        val = np.take_along_axis(bh.masked(fused.cpu().numpy(), edges), idx - bh.U, 1)
        ok, why = tie_aware_rank_equal(idx, val, ref_idx, ref_val, atol=bound)
        assert ok, why
    host_list = model(c).gene_ranklist(bh.TOPK)
    assert np.array_equal(np.asarray(host_list), model(c).gene_ranklist(bh.TOPK, to_cpu=False).cpu().numpy())
    print(f"case {c}: largest ratio {ratio:.3f}")


def test_shuffled_and_duplicated_users_give_the_same_rows():
    m = model(1)
    ordered = m.getUsersRating(np.arange(bh.U))
    ids = np.random.RandomState(3).permutation(bh.U)
    ids[5], ids[40], ids[41] = ids[6], bh.U - 1, ids[6]                                 # duplicates, the user without history twice over
    got = m.getUsersRating(torch.from_numpy(ids))
    assert torch.equal(got, ordered[torch.from_numpy(ids).to(DEV)])
    assert not ordered[bh.U - 1].any()


def test_one_pass_of_the_loop(caplog):
    from chaorec_amd import train_and_evaluate as te
    g, edges, I = case()[:3]
    rng = np.random.RandomState(11)
    val = [[u] + (bh.U + rng.choice(I, 2, replace=False)).tolist() for u in range(bh.U)]
    test = [[u] + (bh.U + rng.choice(I, 3, replace=False)).tolist() for u in range(bh.U)]
    history = []
    with caplog.at_level(logging.INFO):
        out = te.train_and_evaluate(model(0), None, val, test, None, 1000, model_name="BSPM", topk=(5, 10, 20), history=history)
    assert set(out) == {5, 10, 20} and all(np.isfinite(v) for m in out.values() for v in m.values())
    assert out[20]["recall"] > 0 and len(history) == 1 and history[0]["test"] == out
    text = caplog.text
    assert text.count("Validation Metrics:") == 1 and text.count("Test Metrics:") == 1 and "Epoch" not in text
