#!/usr/bin/env python
"""Generate tests/golden/mvgae_small.npz by running the REFERENCE's own Model/MVGAE.py on the CPU.

Nothing of the reference is copied: this script imports Model/MVGAE.py from the reference checkout at run time (the
directory CHAOREC_REFERENCE names) under oracle.pyg_standin and stores inputs + outputs as .npz data.

    python tests/golden/gen_mvgae.py

The reference class runs on the synthetic graph of mvgae_host.small_case().  For the duration of its loss()
torch.nn.functional.dropout and torch.randn_like are wrapped with recorders: the 12 keep masks (an element is kept where the
output is non-zero or the input was zero) and the four noise tables (P, V, T, C: the order loss() draws them in) are stored
as INPUTS; bpr_loss and kl_loss are wrapped to note the eight parts they return.  Stored besides: the seed, sums and probes
of the weights (mvgae_host.init_weights replays the constructor's draws), the state_dict names, result_embed, the eight loss parts and every gradient in training mode, loss and pd_mu in
evaluation mode -- each next to its relative deviation from the float64 restatement (mvgae_host.step) on the same weights.
Refuses to write when the loss deviates by 1e-4.
"""
import os
import sys
import warnings

import numpy as np
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

from oracle import pyg_standin  # noqa: E402
import mvgae_host as mh  # noqa: E402

pyg_standin.install()
torch.set_num_threads(8)
PROBE = 20


class Recorder:
    """Wraps F.dropout and torch.randn_like while the reference's loss() runs."""

    def __init__(self):
        self.keep, self.noise = [], []

    def __enter__(self):
        F = torch.nn.functional
        self._dropout, self._randn_like = F.dropout, torch.randn_like

        def dropout(x, p=0.5, training=True, inplace=False):
            out = self._dropout(x, p=p, training=training, inplace=inplace)
            if training:
                self.keep.append(((out != 0) | (x == 0)).detach().numpy().copy())
            return out

        def randn_like(x, *a, **k):
            out = self._randn_like(x, *a, **k)
            self.noise.append(out.detach().numpy().copy())
            return out

        F.dropout, torch.randn_like = dropout, randn_like
        return self

    def __exit__(self, *exc):
        torch.nn.functional.dropout, torch.randn_like = self._dropout, self._randn_like


def generate_small():
    c = mh.small_case()
    U, I, edges = c["U"], c["I"], c["edges"]
    import Model.MVGAE as refmod
    torch.manual_seed(c["seed"])
    model = refmod.MVGAE(U, I, edges, mh.user_item_dict(edges), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
                         mh.DIM_E, mh.KL_WEIGHT, mh.N_LAYERS, torch.device("cpu"))
    sd = model.state_dict()
    assert tuple(sd.keys()) == mh.NAMES, tuple(sd.keys())
    weights = {n: v.detach().numpy().copy() for n, v in sd.items()}
    replay, plain = mh.init_weights(c)
    for n in mh.NAMES:
        assert np.array_equal(weights[n], replay[n]), f"init_weights does not replay {n}"
    assert np.array_equal(model.collaborative.detach().numpy(), plain["collaborative"])
    assert np.array_equal(model.v_gcn.preference.detach().numpy(), plain["v_gcn.preference"])
    assert np.array_equal(model.c_gcn.preference.detach().numpy(), plain["c_gcn.preference"])
    assert np.array_equal(model.result_embed.detach().numpy(), plain["result_embed"])

    users, pos, neg = (torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))
    model.train()
    parts = {"bpr": [], "kl": []}
    for name in ("bpr", "kl"):                 # the eight parts: what the reference's own methods return inside its loss()
        def wrap(f, log):
            def g(*a):
                out = f(*a)
                log.append(float(out.detach()))
                return out
            return g
        setattr(model, name + "_loss", wrap(getattr(model, name + "_loss"), parts[name]))
    with Recorder() as rec:
        loss = model.loss(users, pos, neg)
    for name in ("bpr", "kl"):
        delattr(model, name + "_loss")
    ref_parts = np.array(parts["bpr"] + parts["kl"])
    assert len(ref_parts) == 8
    loss.backward()
    n_keep = 3 * (mh.N_LAYERS + 2)
    assert len(rec.keep) == n_keep and len(rec.noise) == 4, (len(rec.keep), len(rec.noise))
    keep, eps = np.stack(rec.keep), np.stack(rec.noise)
    share = 1.0 - keep.mean()
    assert 0.05 < share < 0.15, share
    params = dict(model.named_parameters())
    with_grad = tuple(n for n in mh.NAMES if params[n].grad is not None)
    # (the reference evaluates linear_layer1..n and drops the result: autograd leaves those .grad None as well)
    assert with_grad == mh.with_grad(mh.N_LAYERS), with_grad
    assert len(mh.NAMES) - len(with_grad) == 30
    ref_grads = {n: params[n].grad.detach().numpy().copy() for n in with_grad}
    result = model.result_embed.detach().numpy().copy()
    out = mh.step(weights, plain, c, c["users"], c["pos"], c["neg"], mh.KL_WEIGHT, mh.N_LAYERS, keep, eps, True)
    ref_loss = float(loss.detach())
    g = dict(U=U, I=I, seed=c["seed"], names=np.array(mh.NAMES), keep_n=n_keep, keep_bits=np.packbits(keep.reshape(-1)), eps=eps,
             w_sum=np.array([float(weights[n].astype(np.float64).sum()) for n in mh.NAMES]),
             w_probe=np.stack([np.resize(weights[n].reshape(-1)[:PROBE], PROBE) for n in mh.NAMES]),
             ref_result=result, dev_result=mh.rel_dev(result, out["result"]),
             ref_loss=ref_loss, dev_loss=mh.rel_dev(ref_loss, out["loss"]),
             ref_parts=ref_parts, dev_parts=np.array([mh.rel_dev(a, b) for a, b in zip(ref_parts, out["parts"])]))
    print("result", g["dev_result"], "loss", ref_loss, g["dev_loss"], "parts", g["dev_parts"])
    ref_total = float(ref_parts[:4].sum() + mh.KL_WEIGHT * ref_parts[4:].sum())
    assert abs(ref_total - ref_loss) <= 1e-5 * abs(ref_loss), (ref_total, ref_loss)
    devs = []
    for k, n in enumerate(with_grad):
        devs.append(mh.rel_dev(ref_grads[n], out["grads"][n]))
        g[f"ref_grad_{k}"] = ref_grads[n]
    g["dev_grads"] = np.array(devs)
    g["gscale"] = np.array([float(np.abs(out["grads"][n]).max()) for n in with_grad])
    print("grad deviations: max", max(devs), "at", with_grad[int(np.argmax(devs))])

    model.eval()
    with torch.no_grad():
        ev_loss = float(model.loss(users, pos, neg))
        ev_pm = model.forward()[0].numpy().copy()
    ev = mh.step(weights, plain, c, c["users"], c["pos"], c["neg"], mh.KL_WEIGHT, mh.N_LAYERS, None, None, False)
    g.update(ref_eval_loss=ev_loss, dev_eval_loss=mh.rel_dev(ev_loss, ev["loss"]), ref_eval_result=ev_pm,
             dev_eval_result=mh.rel_dev(ev_pm, ev["result"]))
    print("eval loss", ev_loss, g["dev_eval_loss"], "result", g["dev_eval_result"])
    if g["dev_loss"] >= 1e-4 or g["dev_eval_loss"] >= 1e-4:
        raise SystemExit(f"the reference's loss is {g['dev_loss']} / {g['dev_eval_loss']} from the float64 restatement: not written")
    path = os.path.join(HERE, "mvgae_small.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate_small()
