#!/usr/bin/env python
"""Generate tests/golden/dualgnn_small.npz by running the REFERENCE's own Model/DualGNN.py on the CPU.

Nothing of the reference is copied: this script imports Model/DualGNN.py from the reference checkout at run time (the
directory CHAOREC_REFERENCE names), under oracle.pyg_standin, and stores inputs + outputs as .npz data.

    python tests/golden/gen_dualgnn.py

The reference class runs on the synthetic graph of dragon_host.small_case() in a temporary Data/<name>/ that holds a
user_graph_dict.npy written from dragon_host.cooccurrence / user_graph_dict (the project's tie rule; gen_dragon.py checks that
rule against the reference's own script).  Stored: the seeds and probes of the weights (dualgnn_host.init_weights replays the
constructor's draws), the epoch graph the reference's own topk_sample drew, result, the loss parts and every gradient -- each
next to its relative deviation from the float64 restatement (dualgnn_host.step) on the same weights.  Refuses to write when
the loss deviates by 1e-4.
"""
import contextlib
import os
import sys
import tempfile

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

import dragon_host as dh  # noqa: E402
import dualgnn_host as gh  # noqa: E402

torch.set_num_threads(8)
PROBE = 20


@contextlib.contextmanager
def in_tmp_data(dataset):
    """A temporary working directory with Data/<dataset>/, sys.argv naming the dataset (the reference parses it at import)."""
    cwd, argv = os.getcwd(), sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "Data", dataset))
        os.chdir(tmp)
        sys.argv = ["gen_dualgnn", "--data_path", dataset]
        try:
            yield os.path.join(tmp, "Data", dataset)
        finally:
            os.chdir(cwd)
            sys.argv = argv


def generate_small():
    from oracle import pyg_standin
    pyg_standin.install()
    c = dh.small_case()
    U, I, edges = c["U"], c["I"], c["edges"]
    rowptr, col = dh.history_csr(edges, U)
    C = dh.cooccurrence(rowptr, col, U, I)
    with in_tmp_data("dualgnn_small") as d:
        np.save(os.path.join(d, "user_graph_dict.npy"), dh.user_graph_dict(C), allow_pickle=True)
        import Model.DualGNN as refmod
        torch.manual_seed(c["seed"])
        np.random.seed(c["seed"])
        model = refmod.DualGNN(U, I, edges, dh.user_item_dict(edges), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
                               gh.DIM, gh.DIM, gh.REG_WEIGHT, gh.UU_TOPK, "add", torch.device("cpu"))
    # on the CPU `.to(device)` hands the float64 Parameter back and forward() could not assign over it; on a GPU it is a copy
    # and no Parameter -- that is the surface the port has
    del model.result
    sd = model.state_dict()
    assert tuple(sd.keys()) == gh.NAMES, tuple(sd.keys())
    weights = {n: v.detach().numpy().copy() for n, v in sd.items()}
    replay = gh.init_weights(c)
    for n in gh.NAMES:
        assert np.array_equal(weights[n], replay[n]), f"init_weights does not replay {n}"
    np.random.seed(c["draw_seed"])
    model.pre_epoch_processing()
    epoch_idx = np.asarray(model.epoch_user_graph, dtype=np.int64)
    epoch_w = model.user_weight_matrix.numpy().copy()
    lens = np.diff(C.indptr)
    assert (lens == 0).any() and ((lens > 0) & (lens < gh.UU_TOPK)).any() and (lens > dh.TOPN).sum() == 0
    users, pos, neg = (torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))
    loss = model.loss(users, pos, neg)
    loss.backward()
    result = model.result.detach().numpy().copy()
    bpr = float(model.bpr_loss(users, pos - U, neg - U, model.result).detach())
    reg = float(model.regularization_loss(users).detach())
    # (forward() has re-registered the two preference tables under DualGNN's own v_preference / t_preference as well)
    params = dict(model.named_parameters(remove_duplicate=False))
    with_grad = tuple(n for n in gh.NAMES if params[n].grad is not None)
    assert with_grad == gh.WITH_GRAD, with_grad
    ref_grads = {n: params[n].grad.detach().numpy().copy() for n in with_grad}
    out = gh.step(weights, c["v_feat"], c["t_feat"], edges, U, I, epoch_idx, epoch_w, c["users"], c["pos"] - U, c["neg"] - U,
                  gh.REG_WEIGHT)
    g = dict(seed=c["seed"], draw_seed=c["draw_seed"], epoch_idx=epoch_idx.astype(np.int16), epoch_w=epoch_w,
             w_sum=np.array([float(weights[n].astype(np.float64).sum()) for n in gh.NAMES]),
             w_probe=np.stack([weights[n].reshape(-1)[:PROBE] for n in gh.NAMES]),
             ref_result=result, dev_result=dh.rel_dev(result, out["result"]),
             ref_loss=float(loss.detach()), dev_loss=dh.rel_dev(float(loss.detach()), out["loss"]), ref_bpr=bpr, dev_bpr=dh.rel_dev(bpr, out["bpr"]),
             ref_reg=reg, dev_reg=dh.rel_dev(reg, out["reg"]))
    print("result", g["dev_result"], "loss", g["ref_loss"], g["dev_loss"], "bpr", g["dev_bpr"], "reg", g["dev_reg"])
    devs = []
    for k, n in enumerate(gh.WITH_GRAD):
        devs.append(dh.rel_dev(ref_grads[n], out["grads"][n]))
        r = ref_grads[n]
        g[f"ref_grad_{k}"] = r[gh.GRAD_ROWS] if n.endswith("MLP.weight") else r
        print(n, "grad deviation", devs[-1], "scale", float(np.abs(out["grads"][n]).max()))
    g["dev_grads"] = np.array(devs)
    g["gscale"] = np.array([float(np.abs(out["grads"][n]).max()) for n in gh.WITH_GRAD])
    if g["dev_loss"] >= 1e-4:
        raise SystemExit(f"the reference's loss is {g['dev_loss']} from the float64 restatement: not written")
    path = os.path.join(HERE, "dualgnn_small.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate_small()
