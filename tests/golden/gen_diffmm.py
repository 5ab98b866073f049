#!/usr/bin/env python
"""Generate tests/golden/diffmm_small.npz by running the REFERENCE's own Model/DiffMM.py on the CPU.

Nothing of the reference is copied: this script imports Model/DiffMM.py from the reference checkout at run time (the
directory CHAOREC_REFERENCE names) and stores inputs + outputs as .npz data.

    python tests/golden/gen_diffmm.py

Shims for the duration of the run: scipy's private dok_matrix._update (gone from the scipy installed here; restored as
"assign every (row, col) -> value of the dict"), Tensor.cuda / Module.cuda as the identity (there is no GPU here).
The reference class runs on the synthetic graph of diffmm_host.small_case().  torch.randint, torch.randn_like, F.dropout and
torch.rand are wrapped with recorders: the time steps, the noise, the dropout keep flags (kept where the output is non-zero
or the input was zero) and the uniforms of the two edge drops are stored as INPUTS.  Stored besides: the seed, sums and probes
of the weights (our constructor replays the reference's draws from the seed: the weights themselves would not fit), the
state_dict names; for one diffusion step per modality on 24 users diff_loss, gc_loss, the loss and the denoiser's gradients
(emb_layer and the biases whole; of the two [1000, .] / [., 1000] matrices the hidden units 0, 8, 16, ... -- the whole
matrices would not fit either; the stored deviation is taken over the WHOLE matrix); the five p_sample iterates of all users;
the top-1 indices; both rebuilt adjacencies before the drop (in the reference's entry order, which the recorded uniforms
follow) and after it; loss() on them with its gradients; gene_ranklist -- each next to its relative deviation from the
float64 restatement (tests/diffmm_host.py) on the same weights.
Refuses to write when a loss deviates by 1e-4, or when a row's top-1 to top-2 gap is below 1e-3 of the largest magnitude.
"""
import os
import sys
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

import diffmm_host as mh  # noqa: E402

if not hasattr(sp.dok_matrix, "_update"):
    def _update(self, data):
        for (r, c), v in data.items():
            self[r, c] = v
    sp.dok_matrix._update = _update

torch.set_num_threads(8)
PROBE, STRIDE, TOPK = 20, 8, 20


class Recorder:
    """Wraps the four draws and .cuda() while the reference runs."""

    def __init__(self):
        self.keep, self.noise, self.ts, self.rand = [], [], [], []

    def __enter__(self):
        F = torch.nn.functional
        self._saved = (F.dropout, torch.randn_like, torch.randint, torch.rand, torch.Tensor.cuda, torch.nn.Module.cuda)

        def dropout(x, p=0.5, training=True, inplace=False):
            out = self._saved[0](x, p=p, training=training, inplace=inplace)
            if training:
                self.keep.append(((out != 0) | (x == 0)).detach().numpy().copy())
            return out

        def randn_like(x, *a, **k):
            out = self._saved[1](x, *a, **k)
            self.noise.append(out.detach().numpy().copy())
            return out

        def randint(*a, **k):
            out = self._saved[2](*a, **k)
            self.ts.append(out.numpy().copy())
            return out

        def rand(*a, **k):
            out = self._saved[3](*a, **k)
            self.rand.append(out.numpy().copy())
            return out

        F.dropout, torch.randn_like, torch.randint, torch.rand = dropout, randn_like, randint, rand
        torch.Tensor.cuda = lambda self_, *a, **k: self_
        torch.nn.Module.cuda = lambda self_, *a, **k: self_
        return self

    def __exit__(self, *exc):
        F = torch.nn.functional
        F.dropout, torch.randn_like, torch.randint, torch.rand, torch.Tensor.cuda, torch.nn.Module.cuda = self._saved


def strided(name, a):
    """What is stored of a gradient: the hidden units 0, STRIDE, ... of the two large matrices, everything else whole."""
    if name.endswith("in_layers.0.weight"):
        return a[::STRIDE]
    if name.endswith("out_layers.0.weight"):
        return a[:, ::STRIDE]
    return a


def generate_small():
    c = mh.small_case()
    U, I, edges, hy = c["U"], c["I"], c["edges"], mh.HYPER
    import Model.DiffMM as refmod
    g = dict(U=U, I=I, seed=c["seed"], diff_users=c["diff_users"])
    with Recorder() as rec:
        torch.manual_seed(c["seed"])
        model = refmod.DiffMM(U, I, edges, mh.user_item_dict(edges), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]), mh.D,
                              hy["reg_weight"], hy["n_layers"], hy["ssl_alpha"], hy["ssl_temp"], hy["ris_lambda"], hy["e_loss"],
                              hy["rebuild_k"], torch.device("cpu"))
        sd = model.state_dict()
        assert tuple(sd.keys()) == mh.NAMES, tuple(sd.keys())
        weights = {n: v.detach().numpy().copy() for n, v in sd.items()}
        ours = mh.weights_of(mh.build_model(c))
        for n in mh.NAMES:
            assert np.array_equal(weights[n], ours[n]), f"our constructor does not replay {n}"
        T = mh.tables()
        dm = model.diffusion_model
        for k, attr in (("betas", "betas"), ("alphas_cumprod", "alphas_cumprod"), ("coef1", "posterior_mean_coef1"),
                        ("coef2", "posterior_mean_coef2")):
            assert np.array_equal(T[k], getattr(dm, attr).numpy()), k
        g.update(names=np.array(mh.NAMES), w_sum=np.array([float(weights[n].astype(np.float64).sum()) for n in mh.NAMES]),
                 w_probe=np.stack([np.resize(weights[n].reshape(-1)[:PROBE], PROBE) for n in mh.NAMES]))

        # ---- one diffusion step per modality (train_and_evaluate.py:147-175) on diff_users
        rowptr, col = mh.hist_csr(edges, U)
        x0 = mh.dense_rows(rowptr, col, c["diff_users"], I)
        batch_item, batch_index = torch.from_numpy(x0), torch.from_numpy(c["diff_users"])
        model.train()
        iEmbeds = model.getItemEmbeds().detach()
        feats = (model.getImageFeats().detach(), model.getTextFeats().detach())
        devs = {}
        for m, (dn, f) in enumerate(zip((model.denoise_model_image, model.denoise_model_text), feats)):
            mod = ("image", "text")[m]
            dn.zero_grad()
            diff, gc = dm.training_losses(dn, batch_item, iEmbeds, batch_index, f)
            loss = diff.mean() + gc.mean() * model.e_loss
            loss.backward()
            assert len(rec.ts) == m + 1 and len(rec.noise) == m + 1 and len(rec.keep) == m + 1
            h = mh.diffusion_step(weights, c, mod, x0, rec.ts[m], rec.noise[m], rec.keep[m], hy["e_loss"], torch.float64)
            g[f"step_{mod}_loss"], devs[f"step_{mod}_loss"] = float(loss), mh.rel_dev(float(loss), h["loss"])
            g[f"step_{mod}_diff"], devs[f"step_{mod}_diff"] = diff.detach().numpy(), mh.rel_dev(diff.detach().numpy(), h["diff_loss"])
            g[f"step_{mod}_gc"], devs[f"step_{mod}_gc"] = gc.detach().numpy(), mh.rel_dev(gc.detach().numpy(), h["gc_loss"])
            for n, p in dn.named_parameters():
                name = f"denoise_model_{mod}.{n}"
                g["grad_" + name], devs["grad_" + name] = strided(name, p.grad.numpy().copy()), mh.rel_dev(p.grad.numpy(), h["grads"][name])
        assert sorted(set(np.concatenate(rec.ts).tolist())) == list(range(mh.STEPS)), "the draw misses a time step"
        g.update(ts=np.stack(rec.ts), noise=np.stack(rec.noise), keep_bits=np.packbits(np.stack(rec.keep).reshape(-1)))

        # ---- the rebuild (train_and_evaluate.py:183-235), all users in one batch
        all_users = np.arange(U, dtype=np.int64)
        xa = mh.dense_rows(rowptr, col, all_users, I)
        with torch.no_grad():
            for m, dn in enumerate((model.denoise_model_image, model.denoise_model_text)):
                mod = ("image", "text")[m]
                iterates = []
                real = dm.p_mean_variance

                def noting(mdl, x, t, real=real, iterates=iterates):
                    mean, lv = real(mdl, x, t)
                    iterates.append(mean.numpy().copy())
                    return mean, lv
                dm.p_mean_variance = noting
                denoised = dm.p_sample(dn, torch.from_numpy(xa), 0, False)
                del dm.p_mean_variance
                assert len(iterates) == mh.STEPS and np.array_equal(iterates[-1], denoised.numpy())
                h = mh.p_sample(weights, mod, xa, torch.float64)
                g[f"iter_{mod}"] = np.stack(iterates)
                devs[f"iter_{mod}"] = max(mh.rel_dev(a, b) for a, b in zip(iterates, h))
                top = torch.topk(denoised, k=2)
                gap = float(((top.values[:, 0] - top.values[:, 1]) / denoised.abs().max()).min())
                print(mod, "smallest top-1 to top-2 gap", gap, "of the largest magnitude", float(denoised.abs().max()))
                if gap < 1e-3:
                    raise SystemExit(f"{mod}: a row's top-1 to top-2 gap is {gap} of the largest magnitude: not written")
                assert np.array_equal(np.argmax(h[-1], 1), top.indices[:, 0].numpy())
                top1 = torch.topk(denoised, k=model.rebuild_k).indices.numpy()
                g[f"top_{mod}"] = top1
                u_list, i_list = np.repeat(all_users, top1.shape[1]), top1.reshape(-1)
                n_rand = len(rec.rand)
                built = model.buildUIMatrix(u_list, i_list, np.ones(len(u_list)))
                dropped = model.edgeDropper(built)
                assert len(rec.rand) == n_rand + 1
                pre = built._indices().numpy()
                row, col_, val = mh.build_ui(u_list, i_list, U, I)
                order = np.argsort(pre[0] * (U + I) + pre[1], kind="stable")
                assert np.array_equal(pre[0][order], row) and np.array_equal(pre[1][order], col_)
                devs[f"adj_{mod}"] = mh.rel_dev(built._values().numpy()[order], val)
                g.update({f"adj_{mod}_pre": pre, f"adj_{mod}_pre_val": built._values().numpy(), f"adj_{mod}_rand": rec.rand[-1],
                          f"adj_{mod}_idx": dropped._indices().numpy(), f"adj_{mod}_val": dropped._values().numpy()})
                if m == 0:
                    image_adj = dropped
                else:
                    text_adj = dropped

        # ---- loss() on the rebuilt graphs, its gradients, the rank list
        model.zero_grad()
        users, pos, neg = (torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))
        loss = model.loss(users, pos, neg, image_adj, text_adj)
        loss.backward()
        N = U + I
        dense = [mh.dense_adj(g[f"adj_{mod}_idx"][0], g[f"adj_{mod}_idx"][1], g[f"adj_{mod}_val"], N, torch.float64) for mod in ("image", "text")]
        h = mh.model_loss(weights, c, dense[0], dense[1], c["users"], c["pos"], c["neg"], torch.float64)
        g["loss"], devs["loss"] = float(loss), mh.rel_dev(float(loss), h["loss"])
        g["usr"], devs["usr"] = model.restore_usrEmbeds.detach().numpy(), mh.rel_dev(model.restore_usrEmbeds.detach().numpy(), h["usr"])
        g["itm"], devs["itm"] = model.restore_itmEmbeds.detach().numpy(), mh.rel_dev(model.restore_itmEmbeds.detach().numpy(), h["itm"])
        params = dict(model.named_parameters())
        for n in h["grads"]:
            g["grad_" + n], devs["grad_" + n] = params[n].grad.numpy().copy(), mh.rel_dev(params[n].grad.numpy(), h["grads"][n])
        assert all(params[n].grad is None for n in mh.NAMES if n.startswith("denoise_model_"))
        rank = model.gene_ranklist(topk=TOPK).numpy()
        g["rank"] = rank
    for k, v in devs.items():
        g["dev_" + k] = v
        print(f"{k}: deviation {v:.3e}")
    for k in ("step_image_loss", "step_text_loss", "loss"):
        if devs[k] >= 1e-4:
            raise SystemExit(f"the reference's {k} is {devs[k]} from the float64 restatement: not written")
    path = os.path.join(HERE, "diffmm_small.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate_small()
