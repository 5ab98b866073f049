#!/usr/bin/env python
"""Generate tests/golden/lightgode_small.npz by running the REFERENCE's own Model/LightGODE.py on the CPU.

Nothing of the reference is copied: this script imports Model/LightGODE.py from the reference checkout at run time (the
directory CHAOREC_REFERENCE names) and stores inputs + outputs as .npz data.

    CHAOREC_REFERENCE=/path/to/reference python tests/golden/gen_lightgode.py

What had to be supplied around the reference class, and is therefore NOT pinned by this golden:
  * scipy's private dok_matrix._update (gone from the scipy installed here), restored as "assign every (row, col) -> value";
  * a STAND-IN `torchdiffeq` (the package is not installed): `odeint(func, y0, t, method='euler')` without a step size is
    torchdiffeq's fixed-grid Euler on the grid of the time points themselves -- for the two points [0, t] ONE step,
    y1 = y0 + (t[1] - t[0]) func(t[0], y0) -- returned stacked as (y0, y1).  The stand-in does exactly that and nothing else.
The case is lightgode_host's: U 24, I 40, D 64, gamma 0.5, t 1.8, a batch of 70 with repeated users, items and one repeated pair,
the seeded weights shifted by a common vector per table.  Stored: edges, weights, batch, the adjacency's CSR, and from the
reference in fp32 and in float64 the loss, its parts and both table gradients (train mode), the eval-mode tables and the top-10
list, each fp32 result next to its deviation `own_*` from the float64 one.
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
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import lightgode_host as lh  # noqa: E402
from conftest import tie_aware_rank_equal  # noqa: E402

# ---- shim: scipy's private dok_matrix._update -----------------------------------------------------------------------------------
if not hasattr(sp.dok_matrix, "_update"):
    def _update(self, data):
        for (r, c), v in data.items():
            self[r, c] = v
    sp.dok_matrix._update = _update


# ---- stand-in: torchdiffeq.odeint, fixed-grid Euler on the time points ----------------------------------------------------------
def _odeint(func, y0, t, method=None, **kw):
    assert method == "euler" and not kw and t.numel() == 2, "the stand-in covers LightGODE's one call"
    return torch.stack((y0, y0 + (t[1] - t[0]) * func(t[0], y0)))


_tde = types.ModuleType("torchdiffeq")
_tde.odeint = _odeint
sys.modules["torchdiffeq"] = _tde

torch.set_num_threads(8)


def build(edges, w_user=None, w_item=None, double=False):
    import Model.LightGODE as refmod
    torch.manual_seed(lh.SEED)
    m = refmod.LightGODE(lh.U, lh.I, edges, lh.user_item_dict(edges), lh.D, lh.GAMMA, lh.T, torch.device("cpu"))
    if w_user is not None:
        with torch.no_grad():
            m.user_embedding.weight.copy_(torch.from_numpy(w_user))
            m.item_embedding.weight.copy_(torch.from_numpy(w_item))
    if double:
        m = m.double()
        m.odefunc1hop.g = m.norm_adj.double()
    return m


def run(m, users, pos):
    """-> dict(loss, align, unif_u, unif_i, g_u, g_i, tab_u, tab_i, ranks): loss() in train mode, the tables and the list in eval."""
    rec = {}
    alignment, uniformity = m.alignment, m.uniformity
    m.alignment = lambda *a: rec.setdefault("align", alignment(*a))
    unif = []
    m.uniformity = lambda *a: unif.append(uniformity(*a)) or unif[-1]
    m.train()
    loss = m.loss(users, pos, pos)
    loss.backward()
    m.alignment, m.uniformity = alignment, uniformity
    assert m.use_mf is True and len(unif) == 2
    out = dict(loss=loss.detach().numpy(), align=rec["align"].detach().numpy(), unif_u=unif[0].detach().numpy(),
               unif_i=unif[1].detach().numpy(), g_u=m.user_embedding.weight.grad.numpy().copy(),
               g_i=m.item_embedding.weight.grad.numpy().copy())
    m.eval()
    with torch.no_grad():
        ranks = m.gene_ranklist(lh.TOPK).numpy()
        assert m.use_mf is False and m.restore_user_e is not None
        out.update(tab_u=m.restore_user_e.numpy().copy(), tab_i=m.restore_item_e.numpy().copy(), ranks=ranks)
    return out


def generate():
    edges = lh.small_case()
    users, pos = lh.small_batch(edges)
    items = pos - lh.U
    assert lh.U - 1 not in set(edges[:, 0].tolist()) and not set(range(lh.U + lh.I - 4, lh.U + lh.I)) & set(edges[:, 1].tolist())
    assert len(users) - len(set(users.tolist())) >= 20 and len(items) - len(set(items.tolist())) >= 10
    assert users[-1] == users[0] and pos[-1] == pos[0]

    seeded = build(edges)
    assert tuple(n for n, _ in seeded.named_parameters()) == ("user_embedding.weight", "item_embedding.weight")
    su, si = lh.shifts()
    w_user = seeded.user_embedding.weight.detach().numpy() + su
    w_item = seeded.item_embedding.weight.detach().numpy() + si
    g = dict(edges=edges.astype(np.int32), users=users, pos=pos, w_user=w_user, w_item=w_item,
             w_sum_seeded=np.array([float(p.detach().double().sum()) for p in seeded.parameters()]))

    # the adjacency: the reference's coalesced values against the dense restatement
    adj = seeded.norm_adj.coalesce()
    csr = adj.to_sparse_csr()
    g.update(adj_rowptr=csr.crow_indices().numpy().astype(np.int64), adj_col=csr.col_indices().numpy().astype(np.int32),
             adj_val=csr.values().numpy().copy())
    A64 = lh.dense_adj(edges)
    assert np.array_equal(adj.to_dense().numpy(), A64.astype(np.float32)), "the adjacency is not (float32) the fp64 restatement"

    tu, tp = torch.from_numpy(users), torch.from_numpy(pos)
    r32 = run(build(edges, w_user, w_item), tu, tp)
    r64 = run(build(edges, w_user, w_item, double=True), tu, tp)

    # the closed form is the reference's autograd in float64
    c64 = lh.closed_form(w_user, w_item, users, items, lh.GAMMA)
    for k in lh.PARTS + ("g_u", "g_i"):
        dev = lh.rel_dev(c64[k], r64[k])
        print("closed form vs float64 autograd:", k, dev)
        assert dev < 1e-12, k
    # the case spreads: the two uniformity terms differ, e_ij spans two decades
    with torch.no_grad():
        es = [lh.pair_weights(torch.nn.functional.normalize(torch.from_numpy(w).double()[torch.from_numpy(ids)], dim=-1))
              for w, ids in ((w_user, users), (w_item, items))]
    off = ~np.eye(lh.B, dtype=bool)
    e_all = np.concatenate([e.numpy()[off] for e in es])
    print("unif_u", float(r64["unif_u"]), "unif_i", float(r64["unif_i"]), "e_ij in", e_all.min(), e_all.max())
    assert abs(float(r64["unif_u"]) - float(r64["unif_i"])) > 0.1 and e_all.max() >= 100 * e_all.min()

    for k in lh.PARTS + ("g_u", "g_i"):
        g[k + "32"], g[k + "64"], g["own_" + k] = r32[k], r64[k], lh.rel_dev(r32[k], r64[k])
        print(k, "own", g["own_" + k])
        assert g["own_" + k] < 1e-5
    sample32, sample64 = np.concatenate((r32["tab_u"], r32["tab_i"])), np.concatenate((r64["tab_u"], r64["tab_i"]))
    e64 = lh.euler(A64, np.concatenate((w_user, w_item)), lh.T).numpy()
    assert lh.rel_dev(e64, sample64) < 1e-6, "the one Euler step is not what the reference's eval mode computes"
    g.update(sample32=sample32, sample64=sample64, own_euler=lh.rel_dev(sample32, sample64))
    print("own_euler", g["own_euler"])

    # the lists: fp32 against float64, tie-aware, at the rule's bound
    s64 = lh.masked_scores(r64["tab_u"], r64["tab_i"], edges)
    s32 = lh.masked_scores(r32["tab_u"], r32["tab_i"], edges)
    own_scores = lh.rel_dev(s32, s64)
    atol = 4 * max(own_scores, lh.ULP) * float(np.abs(s64).max())
    ok, why = tie_aware_rank_equal(r32["ranks"], lh.rank_values(s32, r32["ranks"]), r64["ranks"], lh.rank_values(s64, r64["ranks"]),
                                   atol=atol)
    assert ok, why
    g.update(ranks32=r32["ranks"].astype(np.int16), ranks64=r64["ranks"].astype(np.int16), own_scores=own_scores)

    path = os.path.join(HERE, lh.FIXTURE)
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate()
