#!/usr/bin/env python
"""Generate tests/golden/cohesion_small.npz by running the REFERENCE's own Model/COHESION.py on the CPU.

Nothing of the reference is copied: this script imports Model/COHESION.py from the reference checkout at run time (the
directory CHAOREC_REFERENCE names) and stores inputs + outputs as .npz data.

    python tests/golden/gen_cohesion.py

The reference class runs on the synthetic graph of dragon_host.small_case() in a temporary Data/<name>/ that holds a
user_graph_dict.npy written from dragon_host.cooccurrence / user_graph_dict.  What had to be supplied around it, and is therefore
not pinned by this golden: an empty `torch_sparse` module (the reference imports it and never uses it), scipy's private
dok_matrix._update (gone from the scipy installed here; restored as "assign every (row, col) -> value of the dict", as
gen_sparse_family.py does), and `model.k = 10` in place of the hard-coded 40 (the synthetic users have few neighbours).
Stored: the seeds and probes of the weights (cohesion_host.init_weights replays the constructor's draws), the epoch graph the
reference's own topk_sample drew, the kNN lists, result_embed, the loss parts and every gradient -- each next to its relative
deviation from the float64 restatement (cohesion_host.step) on the same weights.  Refuses to write when the loss deviates by 1e-4.
"""
import contextlib
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

import dragon_host as dh  # noqa: E402
import cohesion_host as ch  # noqa: E402

if not hasattr(sp.dok_matrix, "_update"):
    def _update(self, data):
        for (r, c), v in data.items():
            self[r, c] = v
    sp.dok_matrix._update = _update
sys.modules.setdefault("torch_sparse", types.ModuleType("torch_sparse"))

torch.set_num_threads(8)
PROBE = 20


@contextlib.contextmanager
def in_tmp_data(dataset):
    """A temporary working directory with Data/<dataset>/, sys.argv naming the dataset (the reference parses it at import)."""
    cwd, argv = os.getcwd(), sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "Data", dataset))
        os.chdir(tmp)
        sys.argv = ["gen_cohesion", "--data_path", dataset]
        try:
            yield os.path.join(tmp, "Data", dataset)
        finally:
            os.chdir(cwd)
            sys.argv = argv


def generate_small():
    c = dh.small_case()
    U, I, edges = c["U"], c["I"], c["edges"]
    rowptr, col = dh.history_csr(edges, U)
    C = dh.cooccurrence(rowptr, col, U, I)
    with in_tmp_data("cohesion_small") as d:
        np.save(os.path.join(d, "user_graph_dict.npy"), dh.user_graph_dict(C), allow_pickle=True)
        import Model.COHESION as refmod
        torch.manual_seed(c["seed"])
        np.random.seed(c["seed"])
        model = refmod.COHESION(U, I, edges, dh.user_item_dict(edges), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
                                ch.DIM_E, ch.REG_WEIGHT, ch.DROPOUT, ch.N_LAYERS, ch.MM_LAYERS, ch.II_TOPK, ch.MM_IMAGE_WEIGHT,
                                torch.device("cpu"))
    # on the CPU `.to(device)` hands the float64 Parameter back and forward() could not assign over it; on a GPU it is a copy
    # and no Parameter -- that is the surface the port has
    del model.result_embed
    model.k = ch.UU_TOPK
    sd = model.state_dict()
    assert tuple(sd.keys()) == ch.NAMES, tuple(sd.keys())
    weights = {n: v.detach().numpy().copy() for n, v in sd.items()}
    replay = ch.init_weights(c)
    for n in ch.NAMES:
        assert np.array_equal(weights[n], replay[n]), f"init_weights does not replay {n}"
    np.random.seed(c["draw_seed"])
    model.pre_epoch_processing()
    epoch_idx = np.asarray(model.epoch_user_graph, dtype=np.int64)
    epoch_w = model.user_weight_matrix.numpy().copy()
    lens = np.diff(C.indptr)
    assert (lens == 0).any() and ((lens > 0) & (lens < ch.UU_TOPK)).any() and (lens > dh.TOPN).sum() == 0
    users, pos, neg = (torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))
    loss = model.loss(users, pos, neg)
    loss.backward()
    result = model.result_embed.detach().numpy().copy()
    params = dict(model.named_parameters(remove_duplicate=False))
    with_grad = tuple(n for n in ch.NAMES if params[n].grad is not None)
    assert with_grad == ch.WITH_GRAD, with_grad
    ref_grads = {n: params[n].grad.detach().numpy().copy() for n in with_grad}
    # the reference's kNN lists (fp32 similarities) against the float64 ones: as sets per item
    knn = {}
    for name, emb in (("v", model.image_embedding), ("t", model.text_embedding)):
        ref_ind = model.get_knn_adj_mat(emb.weight.detach())[0][1].view(I, ch.II_TOPK).numpy()
        mine = dh.knn_indices(c[name + "_feat"], ch.II_TOPK)
        assert np.array_equal(np.sort(ref_ind, 1), np.sort(mine, 1)), f"{name}: the reference's kNN differs from the float64 one"
        knn[name] = np.sort(mine, 1)
    out = ch.step(weights, c["v_feat"], c["t_feat"], edges, U, I, epoch_idx, epoch_w, c["users"], c["pos"] - U, c["neg"] - U,
                  ch.REG_WEIGHT, ch.N_LAYERS, ch.MM_LAYERS, knn["v"], knn["t"], ch.MM_IMAGE_WEIGHT)
    ref_loss = float(loss.detach())
    ref_reg = float(ch.REG_WEIGHT * ((model.v_preference[users] ** 2).mean() + (model.t_preference[users] ** 2).mean()
                                     + (model.weight_u ** 2).mean()).detach())
    ref_bpr = ref_loss - ref_reg
    g = dict(seed=c["seed"], draw_seed=c["draw_seed"], epoch_idx=epoch_idx.astype(np.int16), epoch_w=epoch_w,
             knn_v=knn["v"].astype(np.int16), knn_t=knn["t"].astype(np.int16),
             w_sum=np.array([float(weights[n].astype(np.float64).sum()) for n in ch.NAMES]),
             w_probe=np.stack([np.resize(weights[n].reshape(-1)[:PROBE], PROBE) for n in ch.NAMES]),
             ref_result=result, dev_result=dh.rel_dev(result, out["result"]),
             ref_loss=ref_loss, dev_loss=dh.rel_dev(ref_loss, out["loss"]), ref_bpr=ref_bpr, dev_bpr=dh.rel_dev(ref_bpr, out["bpr"]),
             ref_reg=ref_reg, dev_reg=dh.rel_dev(ref_reg, out["reg"]))
    print("result", g["dev_result"], "loss", g["ref_loss"], g["dev_loss"], "bpr", g["dev_bpr"], "reg", g["dev_reg"])
    devs = []
    for k, n in enumerate(ch.WITH_GRAD):
        devs.append(dh.rel_dev(ref_grads[n], out["grads"][n]))
        r = ref_grads[n]
        g[f"ref_grad_{k}"] = r[ch.GRAD_ROWS] if n.endswith("MLP.weight") else r
        print(n, "grad deviation", devs[-1], "scale", float(np.abs(out["grads"][n]).max()))
    g["dev_grads"] = np.array(devs)
    g["gscale"] = np.array([float(np.abs(out["grads"][n]).max()) for n in ch.WITH_GRAD])
    if g["dev_loss"] >= 1e-4:
        raise SystemExit(f"the reference's loss is {g['dev_loss']} from the float64 restatement: not written")
    path = os.path.join(HERE, "cohesion_small.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate_small()
