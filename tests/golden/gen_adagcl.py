#!/usr/bin/env python
"""Generate tests/golden/adagcl_small.npz by running the REFERENCE's own Model/AdaGCL.py on the CPU.

Nothing of the reference is copied: this script imports Model/AdaGCL.py from the reference checkout at run time (the
directory CHAOREC_REFERENCE names) and stores inputs + outputs as .npz data.

    CHAOREC_REFERENCE=/path/to/reference python tests/golden/gen_adagcl.py

The reference class runs on the synthetic graph of adagcl_host.small_case().  What had to be supplied around it, and is
therefore NOT pinned by this golden:
  * a stand-in `torch_sparse` whose `spmm(index, value, m, n, matrix)` is an index_add_ (the package is not installed); it
    also records the values it is handed, which is how DenoisingNet.call's training-form values are read;
  * scipy's private dok_matrix._update (gone from the scipy installed here), restored as "assign every (row, col) -> value";
  * recorders in place of `torch.randn` and `np.random.uniform` while the model runs, which hand out the float32 draws of
    adagcl_host.draws() in call order: the draws are inputs (their checksums are stored), not the reference's streams.
Stored: the state_dict keys, sums and probes of the weights (adagcl_host.init_weights replays the constructor's draws), the four
losses, the gradients each loss alone produces (grads zeroed in between, no optimizer step), generator 1's keep mask (packed
bits) and logits, generator 2's values for both layers in both forms, the top-10 rank list and a 3-step trajectory of the
reference's loop with its three Adam optimizers -- each next to its relative deviation from the float64 restatement
(adagcl_host) on the same weights and draws.  Asserts that the reference's `_indices()` are row-major, column-ascending;
refuses to write when a loss deviates from the restatement by 1e-4.
"""
import contextlib
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

import adagcl_host as ah  # noqa: E402

if not hasattr(sp.dok_matrix, "_update"):
    def _update(self, data):
        for (r, c), v in data.items():
            self[r, c] = v
    sp.dok_matrix._update = _update

SPMM_VALUES = []


def _spmm(index, value, m, n, matrix):
    SPMM_VALUES.append(value.detach().numpy().copy())
    return torch.zeros(m, matrix.shape[1], dtype=matrix.dtype).index_add_(0, index[0], value[:, None] * matrix[index[1]])


_ts = types.ModuleType("torch_sparse")
_ts.spmm = _spmm
sys.modules["torch_sparse"] = _ts

torch.set_num_threads(8)
PROBE = 20


@contextlib.contextmanager
def given_draws(drs):
    """torch.randn / np.random.uniform hand out the draws of `drs` (a list of per-step dicts) in call order."""
    randn = [t for d in drs for t in d["randn"]]
    unif = [t for d in drs for t in d["u"]]
    real_randn, real_uniform = torch.randn, np.random.uniform

    def fake_randn(*shape, **kw):
        t = torch.from_numpy(randn.pop(0))
        assert tuple(t.shape) == tuple(shape[0] if len(shape) == 1 and not isinstance(shape[0], int) else shape)
        return t

    def fake_uniform(low=0.0, high=1.0, size=None):
        u = unif.pop(0).astype(np.float64)
        assert low == 1e-7 and u.min() >= low and u.max() <= high
        return u.reshape(size)

    torch.randn, np.random.uniform = fake_randn, fake_uniform
    try:
        yield
    finally:
        torch.randn, np.random.uniform = real_randn, real_uniform
    assert not randn and not unif, "the reference drew fewer times than the restatement expects"


def build(c, weights=None):
    import Model.AdaGCL as refmod
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"])
    model = refmod.AdaGCL(c["U"], c["I"], c["edges"], ah.user_item_dict(c["edges"]), ah.DIM_E, ah.REG_WEIGHT, ah.N_LAYERS, ah.SSL_TEMP,
                          ah.SSL_ALPHA, torch.device("cpu"))
    if weights is not None:
        model.load_state_dict({n: torch.from_numpy(v) for n, v in weights.items()})
    model.train()
    return model


def generate_small():
    c = ah.small_case()
    G = ah.graph_arrays(c)
    model = build(c)
    sd = model.state_dict()
    assert tuple(sd.keys()) == ah.NAMES, tuple(sd.keys())
    weights = {n: v.detach().numpy().copy() for n, v in sd.items()}
    replay = ah.init_weights(c)
    for n in ah.NAMES:
        assert np.array_equal(weights[n], replay[n]), f"init_weights does not replay {n}"
    idx = model.norm_adj_mat._indices().numpy()
    assert np.array_equal(idx[0], G["row"]) and np.array_equal(idx[1], G["col"]), "_indices() is not row-major, column-ascending"
    assert np.array_equal(model.norm_adj_mat._values().numpy(), G["val"]), "the normalised adjacency's values differ"
    lens = np.bincount(G["row"], minlength=G["N"])
    assert G["E"] % 64 and (lens == 0).sum() >= 2 and lens.max() >= 70

    users, pos, neg = (torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))
    dr = ah.draws(c, 1)[0]
    host = ah.step_losses(weights, c, dr)
    g = dict(U=c["U"], I=c["I"], seed=c["seed"], E=G["E"], names=np.array(ah.NAMES),
             w_sum=np.array([float(weights[n].astype(np.float64).sum()) for n in ah.NAMES]),
             w_probe=np.stack([np.resize(weights[n].reshape(-1)[:PROBE], PROBE) for n in ah.NAMES]),
             draw_sums=np.array([float(t.astype(np.float64).sum()) for t in dr["randn"] + dr["u"]]))
    params = dict(model.named_parameters())

    def grads_of(name):
        out = {n: params[n].grad.detach().numpy().copy() for n in ah.WITH_GRAD[name]}
        assert all(params[n].grad is None or not params[n].grad.any() for n in ah.NAMES if n not in out), name
        model.zero_grad(set_to_none=True)
        return out

    # the four losses on FIXED weights, each alone
    ref_loss, ref_grads = {}, {}
    with given_draws([dr]):
        l1, out1, out2 = model.loss_1(users, pos, neg)
        l1.backward()
        ref_loss["loss_1"], ref_grads["loss_1"] = float(l1.detach()), grads_of("loss_1")
        l2 = model.loss_2(users, pos, neg, out1, out2)
        l2.backward()
        ref_loss["loss_2"], ref_grads["loss_2"] = float(l2.detach()), grads_of("loss_2")
        l3 = model.bpr_reg_loss(users, pos, neg)
        l3.backward()
        ref_loss["bpr_reg_loss"], ref_grads["bpr_reg_loss"] = float(l3.detach()), grads_of("bpr_reg_loss")
        SPMM_VALUES.clear()
        l4 = model.gen_loss(users, pos, neg)
        train_vals = [v.copy() for v in SPMM_VALUES]
        l4.backward()
        ref_loss["gen_loss"], ref_grads["gen_loss"] = float(l4.detach()), grads_of("gen_loss")
    assert len(train_vals) == ah.N_LAYERS
    for name in ah.LOSSES:
        g[f"ref_{name}"] = ref_loss[name]
        g[f"dev_{name}"] = ah.rel_dev(ref_loss[name], host[name])
        print(name, ref_loss[name], "deviation", g[f"dev_{name}"])
        devs = []
        for k, n in enumerate(ah.WITH_GRAD[name]):
            g[f"ref_grad_{name}_{k}"] = ref_grads[name][n]
            devs.append(ah.rel_dev(ref_grads[name][n], host["grads"][name][n]))
            assert np.isfinite(ref_grads[name][n]).all()
        g[f"dev_grads_{name}"] = np.array(devs)
        print("   grad deviations, largest", max(devs))

    # generator 1: the keep mask and its logits, on the first normal table
    W64, Gr = ah.tensors(weights, requires_grad=False), ah.Graph(c)
    with torch.no_grad():
        with given_draws([dict(randn=dr["randn"][:1], u=[])]):
            x, _, _ = model.generator_1.encoder(model.norm_adj_mat)
        idxs = model.norm_adj_mat._indices()
        ref_logits = model.generator_1.decoder.decoder(x[idxs[0]] * x[idxs[1]])[:, 0].numpy().copy()
        with given_draws([dict(randn=dr["randn"][:1], u=[])]):
            view = model.generator_generate(model.generator_1).coalesce()
        vals64, keep64, logits64 = ah.keep_view(W64, Gr, torch.tensor(dr["randn"][0], dtype=torch.float64))
    ref_keep = np.zeros(G["E"], bool)
    vi = view.indices().numpy()
    pos_of = {(int(r), int(cc)): k for k, (r, cc) in enumerate(zip(G["row"], G["col"]))}
    kept_at = np.array([pos_of[(int(r), int(cc))] for r, cc in zip(vi[0], vi[1])], dtype=np.int64)
    ref_keep[kept_at] = True
    ref_keep_vals = np.zeros(G["E"], np.float32)
    ref_keep_vals[kept_at] = view.values().numpy()
    g.update(keep_bits=np.packbits(ref_keep), keep_logits=ref_logits, dev_keep_logits=ah.rel_dev(ref_logits, logits64.numpy()),
             keep_logit_abs_dev=float(np.abs(ref_logits - logits64.numpy()).max()), keep_vals=ref_keep_vals,
             dev_keep_vals=ah.rel_dev(ref_keep_vals, vals64.numpy()), keep_flips=int((ref_keep != keep64.numpy()).sum()))
    print("keep: kept", int(ref_keep.sum()), "of", G["E"], "flips", g["keep_flips"], "logit deviation (abs)", g["keep_logit_abs_dev"],
          "smallest |logit|", float(np.abs(logits64.numpy()).min()))

    # generator 2: the values of both layers in both forms
    with torch.no_grad():
        x0 = torch.concat([model.uEmbeds, model.iEmbeds], 0)
        x1 = torch.spmm(model.generator_2.generate(x0, 0), x0)
        ev = [model.generator_2.generate(x0, 0).coalesce().values().numpy().copy(), model.generator_2.generate(x1, 1).coalesce().values().numpy().copy()]
        x64 = torch.cat([W64["uEmbeds"], W64["iEmbeds"]], 0)
        h0 = ah.gate(W64, Gr, x64, 0, 1.0, False)
        h1 = ah.gate(W64, Gr, ah.spmm(Gr, h0["val"], x64), 1, 1.0, False)
        t0 = ah.gate(W64, Gr, x64, 0, ah.SSL_TEMP, True, dr["u"][0])
        t1 = ah.gate(W64, Gr, ah.spmm(Gr, t0["val"], x64), 1, ah.SSL_TEMP, True, dr["u"][1])
    for k, (ref, mine) in enumerate(zip(ev + train_vals, (h0, h1, t0, t1))):
        tag = ("eval0", "eval1", "train0", "train1")[k]
        g[f"gate_{tag}"] = ref
        g[f"dev_gate_{tag}"] = ah.rel_dev(ref, mine["val"].numpy())
        print("gate", tag, "deviation", g[f"dev_gate_{tag}"], "logit span", float(mine["logit"].min()), float(mine["logit"].max()))

    # the rank list
    model.eval()
    with torch.no_grad():
        ranks = model.gene_ranklist(ah.TOPK).numpy()
    model.train()
    g["ranklist"] = ranks.astype(np.int16)

    # a 3-step trajectory of the reference's loop with its three Adams (train_and_evaluate.py:72-97), one batch repeated
    drs = ah.draws(c, ah.N_STEPS, seed_offset=2)
    model = build(c, weights)
    opt = torch.optim.Adam(model.parameters(), lr=ah.LR, weight_decay=0)
    opt_gen_1 = torch.optim.Adam(model.generator_1.parameters(), lr=ah.LR, weight_decay=0)
    opt_gen_2 = torch.optim.Adam(filter(lambda p: p.requires_grad, model.generator_2.parameters()), lr=ah.LR, weight_decay=0, eps=0.001)
    traj_losses = []
    with given_draws(drs):
        for _ in drs:
            opt.zero_grad()
            opt_gen_1.zero_grad()
            opt_gen_2.zero_grad()
            loss_1, out1, out2 = model.loss_1(users, pos, neg)
            loss_1.backward()
            opt.step()
            opt.zero_grad()
            loss_2 = model.loss_2(users, pos, neg, out1, out2)
            loss_2.backward()
            opt.step()
            opt.zero_grad()
            bpr_reg_loss = model.bpr_reg_loss(users, pos, neg)
            bpr_reg_loss.backward()
            gen_loss = model.gen_loss(users, pos, neg)
            gen_loss.backward()
            opt.step()
            opt_gen_1.step()
            opt_gen_2.step()
            traj_losses.append([float(x.detach()) for x in (loss_1, loss_2, bpr_reg_loss, gen_loss)])
    final = {n: v.detach().numpy().copy() for n, v in model.state_dict().items()}
    host_final, host_losses = ah.trajectory(weights, c, drs)
    g["traj_losses"] = np.array(traj_losses)
    g["dev_traj_losses"] = ah.rel_dev(traj_losses, host_losses)
    g["dev_traj"] = np.array([ah.rel_dev(final[n] - weights[n], host_final[n] - weights[n]) for n in ah.NAMES])
    for k, n in enumerate(ah.NAMES):
        g[f"traj_{k}"] = final[n]
    print("trajectory: loss deviation", g["dev_traj_losses"], "largest update deviation", float(g["dev_traj"].max()))

    worst = max(g[f"dev_{name}"] for name in ah.LOSSES)
    if worst >= 1e-4:
        raise SystemExit(f"a loss of the reference is {worst} from the float64 restatement: not written")
    path = os.path.join(HERE, "adagcl_small.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate_small()
