#!/usr/bin/env python
"""Generate tests/golden/mhrec_small.npz by running the REFERENCE's own Model/MHRec.py on the CPU.

Nothing of the reference is copied: this script imports Model/MHRec.py from the reference checkout at run time (the
directory CHAOREC_REFERENCE names) and stores inputs + outputs as .npz data.

    python tests/golden/gen_mhrec.py

Shims for the duration of the run: a stand-in `torch_sparse` module (the reference imports it; the path that calls it is
never taken), scipy's private dok_matrix._update (gone from the scipy installed here; restored as "assign every (row, col) ->
value of the dict"), Tensor.cuda / Module.cuda as the identity (there is no GPU here).  The reference reads its command line
and ./Data/<data_path>/user_graph_dict.npy at import / construction: both are supplied from the synthetic case of
mhrec_host.small_case() in a temporary directory, where it also leaves its ii_*.pt and hyperedges_*.npy files.
torch.randint, torch.randn_like and F.dropout are replaced by feeders that hand out the tables of mhrec_host.draws() in call
order (every call's shape is checked): the time steps, the noise, the dropout keep flags are INPUTS the tests regenerate.

Stored: the seed, the state_dict names, the two input hyperedge tables as the reference built them; for the layer cases of
mhrec_host.layer_case (k = 3, 10) the reference layer's output, tail and gradients' deviations; the hypergraphs rebuilt from
the initial denoisers; loss() on them with its parts, gradients, tables and the four layers' outputs; the top-10 list; three
BPR steps; one whole epoch (both diffusion passes, the rebuild, three BPR steps) -- each next to its relative deviation from
the float64 restatement (tests/mhrec_host.py) on the same weights and draws, and 8 rows of each large tensor.

A seed is refused, and the next one tried, unless: every loss is within 1e-4 of the restatement; no |s_n + r_j| exceeds 20 (the
reference's unshifted exp is then safe); each rebuilt hypergraph has a node in no hyperedge and one in more than 64; every
row's k-th and (k + 1)-th denoised values are 2e-5 of the largest magnitude apart (300 fp32 ulps of it: the 1000-term
products behind them round at a few ulps, so fp32 and float64 pick the same nodes) and the reference did pick the
restatement's nodes.
"""
import os
import sys
import tempfile
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

import mhrec_host as mh  # noqa: E402

if not hasattr(sp.dok_matrix, "_update"):
    def _update(self, data):
        for (r, c), v in data.items():
            self[r, c] = v
    sp.dok_matrix._update = _update

torch.set_num_threads(8)
ROWS, MIN_GAP, DATASET = 8, 2e-5, "mhrec_small"


class Feeder:
    """Hands out given draws in call order while the reference runs; .cuda() is the identity."""

    def __init__(self):
        self.ts, self.noise, self.keep = [], [], []

    def feed(self, ts=(), noise=(), keep=()):
        self.ts += list(ts)
        self.noise += list(noise)
        self.keep += list(keep)

    def empty(self):
        return not (self.ts or self.noise or self.keep)

    def __enter__(self):
        F = torch.nn.functional
        self._saved = (F.dropout, torch.randn_like, torch.randint, torch.Tensor.cuda, torch.nn.Module.cuda)

        def dropout(x, p=0.5, training=True, inplace=False):
            if not training:
                return x
            assert p == 0.5
            keep = torch.from_numpy(np.asarray(self.keep.pop(0)))
            assert keep.shape == x.shape, (keep.shape, x.shape)
            return x * (keep.to(x.dtype) * 2.0)

        def randn_like(x, *a, **k):
            out = torch.from_numpy(np.asarray(self.noise.pop(0)))
            assert out.shape == x.shape and out.dtype == x.dtype, (out.shape, x.shape)
            return out

        def randint(low, high, size, *a, **k):
            out = torch.from_numpy(np.asarray(self.ts.pop(0)))
            assert tuple(out.shape) == tuple(size) and int(out.min()) >= low and int(out.max()) < high
            return out

        F.dropout, torch.randn_like, torch.randint = dropout, randn_like, randint
        torch.Tensor.cuda = lambda self_, *a, **k: self_
        torch.nn.Module.cuda = lambda self_, *a, **k: self_
        return self

    def __exit__(self, *exc):
        F = torch.nn.functional
        F.dropout, torch.randn_like, torch.randint, torch.Tensor.cuda, torch.nn.Module.cuda = self._saved


def import_reference(c, workdir):
    """Model/MHRec.py of the reference with its import-time needs met: argv, the stand-in torch_sparse, ./Data/<dataset>."""
    os.makedirs(os.path.join(workdir, "Data", DATASET), exist_ok=True)
    np.save(os.path.join(workdir, "Data", DATASET, "user_graph_dict.npy"), np.array(c["user_graph"], dtype=object), allow_pickle=True)
    os.chdir(workdir)
    stub = types.ModuleType("torch_sparse")
    stub.spmm = lambda index, value, m, n, matrix: torch.sparse.mm(torch.sparse_coo_tensor(index, value, (m, n)), matrix)
    sys.modules.setdefault("torch_sparse", stub)
    sys.argv = [sys.argv[0], "--Model", "MHRec", "--data_path", DATASET]
    import Model.MHRec as refmod
    return refmod


def incidence(nodes, N):
    """The reference's H (train_and_evaluate.py:432-448): scipy COO of ones -> torch sparse [N, E]."""
    E, k = nodes.shape
    H = sp.coo_matrix((np.ones(E * k, dtype=np.float32), (nodes.reshape(-1), np.repeat(np.arange(E), k))), shape=(N, E), dtype=np.float32).tocoo()
    return torch.sparse_coo_tensor(torch.from_numpy(np.vstack((H.row, H.col))).long(), torch.from_numpy(H.data).float(), torch.Size(H.shape))


def same_rows(a, b):
    return np.array_equal(np.sort(a, 1), np.sort(b, 1))


def layer_cases(refmod, fd, g, devs):
    for k in (3, 10):
        lc = mh.layer_case(k)
        lyr = refmod.HypergraphAttentionLayer(mh.D, mh.D)
        with torch.no_grad():
            lyr.a.copy_(torch.from_numpy(lc["a"]).reshape(-1, 1))
        X = torch.from_numpy(lc["X"]).requires_grad_(True)
        out = lyr(incidence(lc["nodes"], lc["N"]), X)
        fd.feed(keep=[lc["keep"]])
        y = out + X                                            # (the model's lines after a layer, Model/MHRec.py:725-726)
        y = torch.nn.functional.dropout(y, 0.5)
        (y * torch.from_numpy(lc["g"])).sum().backward()
        h = mh.layer_grads(lc["X"], lc["a"], lc["nodes"], lc["keep"], lc["g"])
        da, da64 = lyr.a.grad.numpy().reshape(-1), np.concatenate([h["da1"], h["da2"]])
        scale = np.abs(da64).max()                             # a is ONE parameter: both halves' gradients against its largest entry
        devs[f"layer{k}_out"] = mh.rel_dev(out.detach().numpy(), h["out"])
        devs[f"layer{k}_y"] = mh.rel_dev(y.detach().numpy(), h["y"])
        devs[f"layer{k}_dX"] = mh.rel_dev(X.grad.numpy(), h["dX"])
        devs[f"layer{k}_da1"] = mh.rel_dev(da[:mh.D], da64[:mh.D], scale)
        devs[f"layer{k}_da2"] = mh.rel_dev(da[mh.D:], da64[mh.D:], scale)
        g[f"layer{k}_out"], g[f"layer{k}_dX"] = out.detach().numpy()[:ROWS], X.grad.numpy()[:ROWS]
        assert h["max_exp"] <= 20


def ref_rebuild(model, c, table, noises, fd):
    """train_and_evaluate.py:394-497 with the loaders' batches in the case's order -> [visual nodes, textual nodes]."""
    N = c["U"] + c["I"]
    out = []
    with torch.no_grad():
        for m, (dm, dn) in enumerate(((model.image_diffusion_model, model.denoise_model_image),
                                      (model.text_diffusion_model, model.denoise_model_text))):
            rows = []
            for b, batch in enumerate(c["batches"]):
                fd.feed(noise=[noises[m][b]])
                denoised = dm.p_sample(dn, torch.from_numpy(mh.dense_rows(table, batch, N)), mh.SAMPLING_STEPS, False)
                rows.append(torch.topk(denoised, k=model.num_hypernodes)[1].numpy())
            out.append(np.concatenate(rows))
    return out


def ref_bpr_steps(model, c, nodes, fwd_keep, fd):
    N = c["U"] + c["I"]
    Hv, Ht = incidence(nodes[0], N), incidence(nodes[1], N)
    users, pos, neg = (torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))
    opt = torch.optim.Adam(model.parameters(), lr=mh.LR)
    losses = []
    for masks in fwd_keep:
        fd.feed(keep=masks)
        opt.zero_grad()
        loss = model.loss(users, pos, neg, Hv, Ht)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    return np.array(losses)


def update_devs(final, host_final, w0):
    return np.array([mh.rel_dev(final[n] - w0[n], host_final[n] - w0[n]) for n in mh.NAMES])


def try_seed(refmod, seed):
    c = mh.small_case(seed)
    U, I, hy = c["U"], c["I"], mh.HYPER
    N = U + I
    dr = mh.draws(c)
    g, devs = dict(U=U, I=I, seed=seed, names=np.array(mh.NAMES)), {}
    with Feeder() as fd:
        torch.manual_seed(seed)
        np.random.seed(seed)
        model = refmod.MHRec(U, I, c["edges"], mh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
                             mh.D, hy["reg_weight"], hy["ii_topk"], hy["uu_topk"], hy["num_hypernodes"], hy["n_layers"], hy["h_layers"],
                             hy["ssl_temp"], hy["ssl_alpha"], hy["beta1"], hy["beta2"], torch.device("cpu"))
        sd = model.state_dict()
        assert tuple(sd.keys()) == mh.NAMES, tuple(sd.keys())
        w0 = {n: v.detach().numpy().copy() for n, v in sd.items()}
        ours = mh.init_weights(c)
        for n in mh.NAMES:
            assert np.array_equal(w0[n], ours[n]), f"our constructor does not replay {n}"
        T = mh.tables()
        for k, attr in (("betas", "betas"), ("alphas_cumprod", "alphas_cumprod"), ("coef1", "posterior_mean_coef1"),
                        ("coef2", "posterior_mean_coef2")):
            assert np.array_equal(T[k], getattr(model.image_diffusion_model, attr).numpy()), k
        hv, ht = np.asarray(model.hyperedges_visual, dtype=np.int64), np.asarray(model.hyperedges_textual, dtype=np.int64)
        assert np.array_equal(hv, mh.input_hyperedges(c)[0]) and np.array_equal(ht, mh.input_hyperedges(c)[1])
        g["hyper_visual"], g["hyper_textual"] = hv.astype(np.int16), ht.astype(np.int16)
        table = hv                                             # both loaders read the visual file (main.py:227-228)

        layer_cases(refmod, fd, g, devs)

        # ---- the hypergraphs of the initial denoisers, loss() on them
        model.train()
        nodes0 = ref_rebuild(model, c, table, dr["rebuild_noise"], fd)
        host_nodes0, gap0 = mh.rebuild(mh.cast(w0, torch.float64), c, table, dr["rebuild_noise"])
        if gap0 < MIN_GAP or not all(same_rows(a, b) for a, b in zip(nodes0, host_nodes0)):
            return f"initial rebuild: gap {gap0:.2e}"
        g["nodes0"] = np.stack(nodes0).astype(np.int16)
        outs = []
        hooks = [lyr.register_forward_hook(lambda mod, inp, out: outs.append(out.detach().numpy().copy()))
                 for lyr in list(model.hypergraphLayersVisual) + list(model.hypergraphLayersTextual)]
        fd.feed(keep=dr["fwd_keep"][0])
        users, pos, neg = (torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))
        model.zero_grad()
        loss = model.loss(users, pos, neg, incidence(nodes0[0], N), incidence(nodes0[1], N))
        loss.backward()
        for hk in hooks:
            hk.remove()
        h = mh.step_losses(w0, c, nodes0[0], nodes0[1], dr["fwd_keep"][0])
        if h["max_exp"] > 20:
            return f"|s + r| reaches {h['max_exp']}"
        g["loss"], devs["loss"] = float(loss), mh.rel_dev(float(loss), h["loss"])
        params = dict(model.named_parameters())
        devs["grads"] = np.array([mh.rel_dev(params[n].grad.numpy(), h["grads"][n]) for n in mh.WITH_GRAD])
        assert all(params[n].grad is None for n in mh.NAMES if n not in mh.WITH_GRAD)
        for n in mh.WITH_GRAD:
            g["grad8_" + n] = params[n].grad.numpy()[:ROWS].copy()
        devs["layer_outs"] = np.array([mh.rel_dev(a, b) for a, b in zip(outs, h["layer_outs"])])
        g["layer_outs8"] = np.stack([o[:ROWS] for o in outs])
        result = model.result.detach().numpy()
        g["result8"], devs["result"] = result[:ROWS], mh.rel_dev(result, h["result"])
        g["rank"] = model.gene_ranklist(topk=mh.TOPK).numpy()
        for nodes in nodes0:
            deg = np.bincount(nodes.reshape(-1), minlength=N)
            if deg.min() > 0 or deg.max() <= 64:
                return f"degrees span [{deg.min()}, {deg.max()}]"

        # ---- three steps of the third phase from the initial weights
        losses3 = ref_bpr_steps(model, c, nodes0, dr["fwd_keep"], fd)
        host3, host_losses3 = mh.three_steps(w0, c, nodes0[0], nodes0[1], dr["fwd_keep"])
        final3 = {n: v.detach().numpy().copy() for n, v in model.state_dict().items()}
        g["steps3_losses"], devs["steps3_losses"] = losses3, mh.rel_dev(losses3, host_losses3)
        devs["steps3"] = update_devs(final3, host3, w0)

        # ---- one whole epoch from the initial weights (train_and_evaluate.py:331-512)
        model.load_state_dict({n: torch.from_numpy(v.copy()) for n, v in w0.items()})
        diff_losses = []
        for m, (dm, dn) in enumerate(((model.image_diffusion_model, model.denoise_model_image),
                                      (model.text_diffusion_model, model.denoise_model_text))):
            opt = torch.optim.Adam(dn.parameters(), lr=mh.LR, weight_decay=0)
            ls = []
            for b, batch in enumerate(c["batches"]):
                fd.feed(ts=[dr["ts"][m][b]], noise=[dr["noise"][m][b]], keep=[dr["keep"][m][b]])
                opt.zero_grad()
                ld = dm.training_losses(dn, torch.from_numpy(mh.dense_rows(table, batch, N)), None, None).mean()
                ld.backward()
                opt.step()
                ls.append(float(ld))
            diff_losses.append(ls)
        nodes1 = ref_rebuild(model, c, table, dr["rebuild_noise"], fd)
        losses1 = ref_bpr_steps(model, c, nodes1, dr["fwd_keep"], fd)
        ep = mh.epoch(w0, c, table, dr)
        if ep["gap"] < MIN_GAP or not all(same_rows(a, b) for a, b in zip(nodes1, ep["nodes"])):
            return f"epoch rebuild: gap {ep['gap']:.2e}"
        for nodes in nodes1:
            deg = np.bincount(nodes.reshape(-1), minlength=N)
            if deg.min() > 0 or deg.max() <= 64:
                return f"epoch degrees span [{deg.min()}, {deg.max()}]"
        final1 = {n: v.detach().numpy().copy() for n, v in model.state_dict().items()}
        g["nodes1"] = np.stack(nodes1).astype(np.int16)
        g["epoch_diff_losses"], devs["epoch_diff_losses"] = np.array(diff_losses), mh.rel_dev(diff_losses, ep["diff_losses"])
        g["epoch_losses"], devs["epoch_losses"] = losses1, mh.rel_dev(losses1, ep["losses"])
        devs["epoch_loss_sum"] = mh.rel_dev(losses1.sum(), ep["losses"].sum())
        devs["epoch"] = update_devs(final1, ep["weights"], w0)
        for n in mh.NAMES:
            g["epoch8_" + n] = final1[n][:ROWS].copy()
        assert fd.empty()
    for k in ("loss", "steps3_losses", "epoch_diff_losses", "epoch_losses"):
        if devs[k] >= 1e-4:
            return f"the reference's {k} is {devs[k]} from the float64 restatement"
    for k, v in devs.items():
        g["dev_" + k] = v
        print(f"{k}: deviation {np.array2string(np.asarray(v), precision=3)}")
    return g


def generate_small():
    home = os.getcwd()
    with tempfile.TemporaryDirectory() as work:
        refmod = import_reference(mh.small_case(1), work)
        try:
            for seed in range(1, 200):
                g = try_seed(refmod, seed)
                if isinstance(g, dict):
                    break
                print(f"seed {seed} refused: {g}")
            else:
                raise SystemExit("no seed accepted")
        finally:
            os.chdir(home)
    path = os.path.join(HERE, "mhrec_small.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes, seed", g["seed"])
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate_small()
