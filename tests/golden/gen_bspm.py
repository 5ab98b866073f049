#!/usr/bin/env python
"""Generate tests/golden/bspm_small.npz by running the REFERENCE's own Model/BSPM.py on the CPU.

Nothing of the reference is copied: this script imports Model/BSPM.py from the reference checkout at run time (the directory
CHAOREC_REFERENCE names) and stores inputs + outputs as .npz data.

    CHAOREC_REFERENCE=/path/to/reference python tests/golden/gen_bspm.py

Stand-ins for the duration of the run, none of them pinned by this golden:
  * `sparsesvd.sparsesvd(matrix, k)`: numpy.linalg.svd of the dense matrix, truncated to the CASE's factor (the reference asks
    for its hard-coded 256, more than the small adjacency has);
  * `torchdiffeq.odeint(func, y0, t, method)`: fixed-step Euler, y + (t[i + 1] - t[i]) * func(t[i], y), the states stacked --
    it also records the states, which is how the seed y0 of the reference's own lines is read;
  * an empty `torch_sparse` (imported, never called);
  * scipy's private dok_matrix._update (gone from the scipy installed here), restored as "assign every (row, col) -> value".

The case (tests/bspm_host.py): U 70, I = max(150, the kernel's long-row length + 10), factor 16; item 0 held by every user with
a history, so its row of P is full and longer than the long-row length; the last user without history; ten items without users.

Stored: the edges; Rn's and P_II's values as the reference rounded them (fp32, CSR order); Vi = the item block of the reference's
full-adjacency vectors, orthonormalised, with the distance of its projector to theirs; for each (K_s, T_s, idl_beta) of
bspm_host.CASES the reference's item columns (fp32, as it is) and its gene_ranklist, the float64 restatement's item columns,
the reference's deviation from it (`own_*`), the seed's deviation, and the largest user-column magnitude (a record that those
columns exist and are unread); `own_project`, the deviation of an fp32 product X F from the float64 one.
Asserted here: the singular-value gap that makes the projector well defined; the item-block restatement equals the full one;
the reference's fp32 list and the float64 list pass tie_aware_rank_equal at atol = 4 * max(own, ULP) * largest score.
"""
import os
import sys
import types
import warnings

import numpy as np
import scipy.sparse as sp
import torch

REF = os.environ.get("CHAOREC_REFERENCE")
if not REF:
    raise SystemExit("set CHAOREC_REFERENCE to the reference checkout")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import bspm_host as bh  # noqa: E402
from conftest import tie_aware_rank_equal  # noqa: E402

if not hasattr(sp.dok_matrix, "_update"):
    def _update(self, data):
        for (r, c), v in data.items():
            self[r, c] = v
    sp.dok_matrix._update = _update

STATES = []
MIN_GAP = 3e-3          # (sigma_m - sigma_(m + 1)) / sigma_1 of Rn: float64 error / gap stays below 1e-12


def _sparsesvd(matrix, k):
    u, s, vt = np.linalg.svd(np.asarray(matrix.todense(), dtype=np.float64))
    k = min(k, bh.FACTOR)
    return u[:, :k].T, s[:k], vt[:k]


def _odeint(func, y0, t, method=None):
    assert method == "euler"
    ys = [y0]
    for i in range(len(t) - 1):
        ys.append(ys[-1] + (t[i + 1] - t[i]) * func(t[i], ys[-1]))
    STATES[:] = [y.detach().numpy().copy() for y in ys]
    return torch.stack(ys)


def import_reference():
    for name, attrs in (("sparsesvd", {"sparsesvd": _sparsesvd}), ("torchdiffeq", {"odeint": _odeint}), ("torch_sparse", {})):
        mod = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules.setdefault(name, mod)
    import Model.BSPM as refmod
    return refmod


def generate():
    from chaorec_amd import _lib
    _lib.ensure_built()
    long_row = int(_lib.load().chaorec_bspm_long_row())
    I, m = bh.num_items(long_row), bh.FACTOR // 2
    U = bh.U
    for seed in range(1, 200):       # the first seed whose singular-value gap makes the projector well defined (see below)
        edges = bh.small_case(I, seed)
        if bh.item_factors(bh.normalised(edges, I)[0], m)[1] > MIN_GAP:
            break
    else:
        raise SystemExit("no seed accepted")
    refmod = import_reference()
    g = dict(U=U, I=I, seed=seed, factor=bh.FACTOR, long_row=long_row, edges=edges.astype(np.int32))

    Rn64, du, di = bh.normalised(edges, I)
    P64 = Rn64.T @ Rn64
    assert int((P64[0] != 0).sum()) == I - bh.EMPTY_ITEMS > long_row, "item 0's row of P must take the long-row path"
    assert (Rn64[U - 1] == 0).all() and (Rn64[:, I - bh.EMPTY_ITEMS:] == 0).all()
    Vi_own, gap = bh.item_factors(Rn64, m)
    assert gap > MIN_GAP, f"sigma_m - sigma_(m+1) = {gap} sigma_1: the projector is not well defined"

    for c, (K_s, T_s, beta) in enumerate(bh.CASES):
        model = refmod.BSPM(U, I, edges, bh.user_item_dict(edges), K_s, T_s, 1, 1, beta, torch.device("cpu"))
        if c == 0:
            # ---- what the reference built: Rn and P_II as it rounded them, its vectors' item block
            L = model.norm_adj.tocoo().astype(np.float32).toarray()
            Rn32 = L[:U, U:]
            P32 = model.linear_Filter.coalesce().to_dense().numpy()[U:, U:]
            assert np.array_equal(Rn32, Rn64.astype(np.float32)), "Rn is not the float64 product rounded once"
            assert bh.rel_dev(P32, P64) <= bh.ULP and np.array_equal(P32 != 0, P64 != 0)
            ru, ri = np.nonzero(Rn32)
            pr, pc = np.nonzero(P32)
            g["rn_val"], g["p_val"] = Rn32[ru, ri], P32[pr, pc]
            g["p_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(pr, minlength=I))]).astype(np.int32)
            g["p_col"] = pc.astype(np.int16)
            vt_item = np.asarray(model.vt, np.float64)[:, U:]                 # [2 m, I], rank m
            assert model.vt.shape == (bh.FACTOR, U + I)
            Vi = np.linalg.svd(vt_item.T, full_matrices=False)[0][:, :m]
            g["Vi"] = Vi
            g["projector_dev"] = float(np.abs(Vi @ Vi.T - vt_item.T @ vt_item).max())
            g["projector_dev_own"] = float(np.abs(Vi @ Vi.T - Vi_own @ Vi_own.T).max())
            assert g["projector_dev"] < 1e-12 and g["projector_dev_own"] < 1e-10, (g["projector_dev"], g["projector_dev_own"])
            X32, F32 = torch.from_numpy(Rn32), torch.from_numpy((di[:, None] * Vi).astype(np.float32))
            g["own_project"] = bh.rel_dev(torch.mm(X32, F32).numpy(), Rn64 @ (di[:, None] * Vi))
        ratings = model.getUsersRating(np.arange(U)).detach().numpy()
        assert ratings.shape == (U, U + I) and ratings.dtype == np.float32 and len(STATES) == K_s + 1
        seed32 = STATES[0][:, U:]
        ref32 = ratings[:, U:].copy()
        rank = model.gene_ranklist(torch.from_numpy(ratings.copy()), topk=bh.TOPK).numpy()
        full64, _ = bh.full_route(edges, I, K_s, T_s, beta)
        host64, _, seed64, _ = bh.item_route(edges, I, K_s, T_s, beta, g["Vi"], parts=True)
        assert bh.rel_dev(host64, full64[:, U:]) <= 1e-12, "the item-block route is not the full route's item columns"
        own = bh.rel_dev(ref32, host64)
        scale = float(np.abs(host64).max())
        i32, v32 = rank - U, np.take_along_axis(bh.masked(ref32, edges), rank - U, 1)
        i64, v64 = bh.top_lists(bh.masked(host64, edges))
        ok, why = tie_aware_rank_equal(i32, v32, i64, v64, atol=4 * max(own, bh.ULP) * scale)
        assert ok, f"case {c}: the reference's own list against the float64 list: {why}"
        g[f"ref32_{c}"], g[f"host64_{c}"], g[f"rank_{c}"] = ref32, host64, rank.astype(np.int16)
        g[f"own_{c}"], g[f"own_seed_{c}"] = own, bh.rel_dev(seed32, seed64)
        g[f"usercol_max_{c}"] = float(np.abs(ratings[:, :U]).max())
        print(f"case {c} K_s={K_s} T_s={T_s} beta={beta}: own {own:.3e}, seed {g[f'own_seed_{c}']:.3e}, largest score {scale:.4f}, "
              f"negative or zero {np.mean(host64 <= 0):.2f}, user columns up to {g[f'usercol_max_{c}']:.3e}")
    print(f"I={I} long_row={long_row} gap={gap:.3e} projector_dev={g['projector_dev']:.2e} own_project={g['own_project']:.3e}")
    path = os.path.join(HERE, bh.FIXTURE)
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate()
