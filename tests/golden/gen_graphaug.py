#!/usr/bin/env python
"""Generate tests/golden/graphaug_small.npz by running the REFERENCE's own Model/GraphAug.py on the CPU.

Nothing of the reference is copied: this script imports Model/GraphAug.py from the reference checkout at run time (the
directory CHAOREC_REFERENCE names) and stores inputs + outputs as .npz data.

    CHAOREC_REFERENCE=/path/to/reference python tests/golden/gen_graphaug.py

The reference class runs on the synthetic graph of graphaug_host.small_case().  What had to be supplied around it, and is
therefore NOT pinned by this golden:
  * a stand-in `torch_sparse` (the package is not installed): `spmm(index, value, m, n, matrix)` as an index_add_,
    `coalesce(index, value, m, n)` through torch's own coalesce;
  * scipy's private dok_matrix._update (gone from the scipy installed here), restored as "assign every (row, col) -> value";
  * `.cuda()`: on a Parameter a differentiable copy that is NOT a Parameter (what a CPU Parameter's .cuda() is on a GPU: the
    bottom MixHop layers' weights are therefore plain tensors, absent from state_dict()), on any other tensor and on modules
    the identity;
  * recorders in place of torch.rand, F.dropout, torch.randint and torch.randint_like while the model runs, which hand out the
    draws of graphaug_host.draws() in call order: the draws are inputs (their checksums are stored), not the reference's streams.
Stored: the state_dict keys, sums and probes of the weights (graphaug_host.init_weights replays the constructor's draws), the
loss and its four parts, the gradients, view 1's values (non-zero mask as packed bits), s and logits, node_emb probes, the
top-10 rank list and a 3-step Adam trajectory -- each next to its relative deviation from the float64 restatement
(graphaug_host) on the same weights and draws.  Asserts that the reference's `_indices()` are row-major, column-ascending;
refuses to write when the loss deviates from the restatement by 1e-4.
"""
import contextlib
import math
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

import graphaug_host as gh  # noqa: E402

if not hasattr(sp.dok_matrix, "_update"):
    def _update(self, data):
        for (r, c), v in data.items():
            self[r, c] = v
    sp.dok_matrix._update = _update


def _spmm(index, value, m, n, matrix):
    return torch.zeros(m, matrix.shape[1], dtype=matrix.dtype).index_add_(0, index[0], value[:, None] * matrix[index[1]])


def _coalesce(index, value, m, n):
    t = torch.sparse_coo_tensor(index, value, (m, n)).coalesce()
    return t.indices(), t.values()


_ts = types.ModuleType("torch_sparse")
_ts.spmm, _ts.coalesce = _spmm, _coalesce
sys.modules["torch_sparse"] = _ts

torch.Tensor.cuda = lambda self, *a, **k: self.clone() if isinstance(self, torch.nn.Parameter) else self
torch.nn.Module.cuda = lambda self, *a, **k: self

torch.set_num_threads(8)
PROBE = 20


@contextlib.contextmanager
def given_draws(drs):
    """torch.rand / F.dropout / torch.randint / torch.randint_like hand out the draws of `drs` (per-step dicts) in call order."""
    rands = [u for d in drs for v in d["views"] for u in (v["u1"], v["u2"])]
    masks = [m for d in drs for v in d["views"] for m in v["masks"]]
    ints = [t for d in drs for t in d["rdm"]]
    real = torch.rand, torch.nn.functional.dropout, torch.randint, torch.randint_like

    def fake_rand(*shape, **kw):
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape)
        u = torch.from_numpy(rands.pop(0))
        assert u.numel() == int(np.prod(shape)), (u.shape, shape)
        return u.reshape(shape)

    def fake_dropout(input, p=0.5, training=True, inplace=False):
        m = torch.from_numpy(masks.pop(0))
        assert training and p == gh.DROP and m.shape == input.shape
        return input * (m.to(input.dtype) / (1.0 - p))

    def fake_randint(high, size, **kw):
        t = torch.from_numpy(ints.pop(0))
        assert t.shape == tuple(size) and int(t.max()) < high
        return t

    def fake_randint_like(like, high, **kw):
        return fake_randint(high, like.shape)

    torch.rand, torch.nn.functional.dropout, torch.randint, torch.randint_like = fake_rand, fake_dropout, fake_randint, fake_randint_like
    try:
        yield
    finally:
        torch.rand, torch.nn.functional.dropout, torch.randint, torch.randint_like = real
    assert not rands and not masks and not ints, "the reference drew fewer times than the restatement expects"


def build(c, weights=None):
    import Model.GraphAug as refmod
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"])
    model = refmod.GraphAug(c["U"], c["I"], c["edges"], gh.user_item_dict(c["edges"]), gh.DIM_E, gh.REG_WEIGHT, gh.N_LAYERS, gh.SSL_TEMP,
                            gh.SSL_ALPHA, torch.device("cpu"))
    if weights is not None:
        model.load_state_dict({n: torch.from_numpy(weights[n.replace("view_learner.encoder.", "backbone_gnn.")]) for n in gh.NAMES})
        with torch.no_grad():
            for k, layer in enumerate(model.backbone_gnn.bottom_layers):
                layer.weight_matrix.copy_(torch.from_numpy(weights[gh.BOTTOM[2 * k]]))
                layer.bias.copy_(torch.from_numpy(weights[gh.BOTTOM[2 * k + 1]]))
    model.train()
    return model


def all_weights(model):
    W = {n: v.detach().numpy().copy() for n, v in model.named_parameters()}
    for k, layer in enumerate(model.backbone_gnn.bottom_layers):
        W[gh.BOTTOM[2 * k]] = layer.weight_matrix.detach().numpy().copy()
        W[gh.BOTTOM[2 * k + 1]] = layer.bias.detach().numpy().copy()
    return W


def generate_small():
    c = gh.small_case()
    G = gh.graph_arrays(c)
    model = build(c)
    assert tuple(model.state_dict().keys()) == gh.NAMES, tuple(model.state_dict().keys())
    assert tuple(n for n, _ in model.named_parameters()) == gh.PARAMS
    weights = all_weights(model)
    replay = gh.init_weights(c)
    for n in gh.PARAMS + gh.BOTTOM:
        assert np.array_equal(weights[n], replay[n]), f"init_weights does not replay {n}"
    idx = model.norm_adj_mat._indices().numpy()
    assert np.array_equal(idx[0], G["row"]) and np.array_equal(idx[1], G["col"]), "_indices() is not row-major, column-ascending"
    assert np.array_equal(model.norm_adj_mat._values().numpy(), G["val"]), "the normalised adjacency's values differ"
    lens = np.bincount(G["row"], minlength=G["N"])
    assert G["E"] % 32 and G["N"] % 32 and (lens == 0).sum() >= 3 and lens.max() >= 70

    users, pos, neg = (torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))
    dr = gh.draws(c, 1)[0]
    host, host_grads = gh.step_with_grads(weights, c, dr)
    every = [u for v in dr["views"] for u in (v["u1"], v["u2"])] + [m for v in dr["views"] for m in v["masks"]] + list(dr["rdm"])
    g = dict(U=c["U"], I=c["I"], seed=c["seed"], E=G["E"], names=np.array(gh.NAMES),
             w_sum=np.array([float(weights[n].astype(np.float64).sum()) for n in gh.PARAMS + gh.BOTTOM]),
             w_probe=np.stack([np.resize(weights[n].reshape(-1)[:PROBE], PROBE) for n in gh.PARAMS + gh.BOTTOM]),
             draw_sums=np.array([float(np.asarray(t, dtype=np.float64).sum()) for t in every]))

    # loss(): the total, its parts (the class's own methods, recorded), the views, the gradients
    rec = dict(views=[], bpr=[], reg=[], cl=[])
    vl_forward, bpr_loss, reg_loss, con_loss = model.view_learner.forward, model.bpr_loss, model.regularization_loss, model.contrastLoss
    model.view_learner.forward = lambda *a, **k: rec["views"].append(vl_forward(*a, **k)) or rec["views"][-1]
    model.bpr_loss = lambda *a: rec["bpr"].append(bpr_loss(*a)) or rec["bpr"][-1]
    model.regularization_loss = lambda *a: rec["reg"].append(reg_loss(*a)) or rec["reg"][-1]
    model.contrastLoss = lambda *a: rec["cl"].append(con_loss(*a)) or rec["cl"][-1]
    with given_draws([dr]):
        loss = model.loss(users, pos, neg)
    loss.backward()
    model.view_learner.forward, model.bpr_loss, model.regularization_loss, model.contrastLoss = vl_forward, bpr_loss, reg_loss, con_loss
    with torch.no_grad():
        ne = torch.mean(torch.stack([v[0] for v in rec["views"]], 0), dim=0)
        std = torch.nn.functional.softplus(ne[:, gh.IB:] - gh.IB, beta=1)
        kl = -0.5 * (1 + 2 * std.log() - ne[:, :gh.IB].pow(2) - std.pow(2)).sum(1).mean().div(math.log(2))
    ref = dict(loss=float(loss.detach()), bpr=float(rec["bpr"][0].detach()), reg=float(rec["reg"][0].detach()),
               cl=float(((rec["cl"][0] + rec["cl"][1]) * gh.SSL_ALPHA).detach()), kl=float(kl))
    for name in ("loss",) + gh.PARTS:
        g[f"ref_{name}"], g[f"dev_{name}"] = ref[name], gh.rel_dev(ref[name], host[name])
        print(name, ref[name], "deviation", g[f"dev_{name}"])
    params = dict(model.named_parameters())
    devs = []
    for k, n in enumerate(gh.WITH_GRAD):
        gr = params[n].grad.detach().numpy().copy()
        assert np.isfinite(gr).all() and gr.any(), n
        g[f"ref_grad_{k}"] = gr
        devs.append(gh.rel_dev(gr, host_grads[n]))
    assert all(params[n].grad is None for n in gh.MLP)
    g["dev_grads"] = np.array(devs)
    print("grad deviations", devs)

    # view 1: logits, s (recomputed by the class's own method on the recorded node_emb and the same draws), values
    v0 = dr["views"][0]
    with torch.no_grad():
        node_emb, val = rec["views"][0][0].detach(), rec["views"][0][1].detach()
        ii = model.norm_adj_mat._indices()
        ref_logits = model.view_learner.mlp_edge_model(torch.cat([node_emb[ii[0]], node_emb[ii[1]]], 1))[:, 0].numpy().copy()
    ref_val = val.numpy().copy()
    s64, val64, lg64, att64 = (host[k][0].numpy() for k in ("s", "val", "logits", "att"))
    nz = ref_val != 0
    assert np.array_equal(nz, ref_val > 0.2)
    abs_dev_s = float(np.abs(np.where(nz, ref_val, s64) - s64).max())          # (s itself is visible where it passed the threshold)
    g.update(nonzero_bits=np.packbits(nz), val=ref_val, logits=ref_logits, dev_logits=gh.rel_dev(ref_logits, lg64),
             dev_val=gh.rel_dev(ref_val[nz == (val64 != 0)], val64[nz == (val64 != 0)]), flips=int((nz != (val64 != 0)).sum()),
             abs_dev_s=abs_dev_s)
    print("view 1: non-zero", int(nz.sum()), "of", G["E"], "flips", g["flips"], "deviation of s (abs)", abs_dev_s, "logit deviation",
          g["dev_logits"], "att at clamps", int((att64 == 0.01).sum()), int((att64 == 0.99).sum()), "smallest |s - 0.2|",
          float(np.abs(s64 - 0.2).min()))
    assert (att64 == 0.01).any() and (att64 == 0.99).any() and nz.any() and not nz.all()
    ne_ref = node_emb.numpy()[:PROBE].copy()
    g.update(node_emb=ne_ref, dev_node_emb=gh.rel_dev(ne_ref, host["node_emb"][0].detach().numpy()[:PROBE]))
    print("node_emb deviation", g["dev_node_emb"])

    # the rank list
    model.eval()
    with torch.no_grad():
        ranks = model.gene_ranklist(gh.TOPK).numpy()
    model.train()
    g["ranklist"] = ranks.astype(np.int16)
    assert np.array_equal(ranks, gh.ranklist(weights, c)), "the rank list differs from the float64 restatement's"

    # a 3-step trajectory of the plain loop (train_and_evaluate.py:41-47) with Adam, one batch repeated
    drs = gh.draws(c, gh.N_STEPS, seed_offset=2)
    model = build(c, weights)
    opt = torch.optim.Adam(model.parameters(), lr=gh.LR)
    traj_losses = []
    with given_draws(drs):
        for _ in drs:
            opt.zero_grad()
            loss = model.loss(users, pos, neg)
            loss.backward()
            opt.step()
            traj_losses.append(float(loss.detach()))
    final = {n: v.detach().numpy().copy() for n, v in model.named_parameters()}
    host_final, host_losses = gh.trajectory(weights, c, drs)
    g["traj_losses"] = np.array(traj_losses)
    g["dev_traj_losses"] = gh.rel_dev(traj_losses, host_losses)
    g["dev_traj"] = np.array([gh.rel_dev(final[n] - weights[n], host_final[n] - weights[n]) for n in gh.WITH_GRAD])
    for k, n in enumerate(gh.WITH_GRAD):
        g[f"traj_{k}"] = final[n]
    assert all(np.array_equal(final[n], weights[n]) for n in gh.MLP), "the edge MLP moved"
    print("trajectory: loss deviation", g["dev_traj_losses"], "update deviations", g["dev_traj"])

    if g["dev_loss"] >= 1e-4:
        raise SystemExit(f"the reference's loss is {g['dev_loss']} from the float64 restatement: not written")
    path = os.path.join(HERE, "graphaug_small.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate_small()
