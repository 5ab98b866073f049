#!/usr/bin/env python
"""Generate tests/golden/dragon_usergraph_baby.npz and dragon_small.npz by running the REFERENCE's own code on the CPU.

Nothing of the reference is copied: this script runs dualgnn-gen-u-u-matrix.py and imports Model/DRAGON.py from the reference
checkout at run time (the directory CHAOREC_REFERENCE names) and stores inputs + outputs as .npz data.

    python tests/golden/gen_dragon.py [baby] [small]

baby   the reference's script as __main__ (runpy) in a temporary directory holding Data/baby/train.npy written from
       baby_interactions.npz, stdout discarded.  Stored for all 12 351 users: the neighbour count and the count sequence
       (descending); for 512 evenly spaced users the id lists as torch.topk ordered them.
small  the reference DRAGON class under oracle.pyg_standin on a synthetic graph (dragon_host.small_case), its
       user_graph_dict.npy written from the reference's importable gen_user_matrix plus the project's tie rule.  Stored: the
       seed and probes of the weights (dragon_host.init_weights replays the constructor's draws), the epoch graph the
       reference's own topk_sample drew, result, the loss parts and every gradient -- each next to its relative deviation
       from the float64 restatement (dragon_host.step) on the same weights.  Refuses to write when the loss deviates by 1e-4.
"""
import contextlib
import importlib.util
import io
import os
import runpy
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

torch.set_num_threads(8)
PROBE = 20
N_ID_USERS = 512


@contextlib.contextmanager
def in_tmp_data(dataset):
    """A temporary working directory with Data/<dataset>/, sys.argv naming the dataset (the reference parses it at import)."""
    cwd, argv = os.getcwd(), sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "Data", dataset))
        os.chdir(tmp)
        sys.argv = ["gen_dragon", "--data_path", dataset]
        try:
            yield os.path.join(tmp, "Data", dataset)
        finally:
            os.chdir(cwd)
            sys.argv = argv


def generate_baby():
    g = np.load(os.path.join(HERE, "baby_interactions.npz"))
    U, I, train = int(g["U"]), int(g["I"]), g["train"].astype(np.int64)
    with in_tmp_data("baby") as d:
        np.save(os.path.join(d, "train.npy"), train)
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            runpy.run_path(os.path.join(REF, "dualgnn-gen-u-u-matrix.py"), run_name="__main__")
        graph = np.load(os.path.join(d, "user_graph_dict.npy"), allow_pickle=True).item()
    assert len(graph) == U
    length = np.array([len(graph[u][0]) for u in range(U)], dtype=np.int64)
    counts = np.concatenate([np.asarray(graph[u][1], dtype=np.int64) for u in range(U)])
    id_users = np.unique(np.linspace(0, U - 1, N_ID_USERS).astype(np.int64))
    ids = np.concatenate([np.asarray(graph[u][0], dtype=np.int64) for u in id_users])
    # the restatement reproduces it (the same checks tests/test_dragon_host.py makes)
    rowptr, col = dh.history_csr(train, U)
    C = dh.cooccurrence(rowptr, col, U, I)
    off = np.concatenate(([0], np.cumsum(length)))
    for u in range(U):
        bad = dh.check_ids(u, graph[u][0], np.asarray(graph[u][1], dtype=np.int64), C)
        assert bad is None, bad
    assert length.max() <= 255 and counts.max() < 65536 and U < 65536
    path = os.path.join(HERE, "dragon_usergraph_baby.npz")
    np.savez_compressed(path, U=U, I=I, len=length.astype(np.uint8), counts=counts.astype(np.uint8 if counts.max() < 256 else np.uint16),
                        id_users=id_users.astype(np.uint16), ids=ids.astype(np.uint16))
    print(path, os.path.getsize(path), "bytes; longest list", int(length.max()), "largest count", int(counts.max()),
          "users with > 200 neighbours", int((np.diff(C.indptr) > dh.TOPN).sum()), "offsets end", int(off[-1]))
    assert os.path.getsize(path) < (1 << 20)


def generate_small():
    from oracle import pyg_standin
    pyg_standin.install()
    c = dh.small_case()
    U, I, edges = c["U"], c["I"], c["edges"]
    spec = importlib.util.spec_from_file_location("ref_uu", os.path.join(REF, "dualgnn-gen-u-u-matrix.py"))
    with in_tmp_data("dragon_small") as d:
        uu = importlib.util.module_from_spec(spec)
        with contextlib.redirect_stderr(io.StringIO()):
            spec.loader.exec_module(uu)
            M = uu.gen_user_matrix(edges.tolist(), U).numpy()
        rowptr, col = dh.history_csr(edges, U)
        C = dh.cooccurrence(rowptr, col, U, I)
        assert np.array_equal(M.astype(np.int64), C.toarray()), "the reference's matrix differs from R R^T"
        np.save(os.path.join(d, "user_graph_dict.npy"), dh.user_graph_dict(C), allow_pickle=True)
        import Model.DRAGON as refmod
        torch.manual_seed(c["seed"])
        np.random.seed(c["seed"])
        model = refmod.DRAGON(U, I, edges, dh.user_item_dict(edges), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
                              dh.DIM, dh.DIM, dh.REG_WEIGHT, dh.N_LAYERS, dh.II_TOPK, dh.UU_TOPK, dh.MM_IMAGE_WEIGHT, "add",
                              torch.device("cpu"))
    # on the CPU `.to(device)` hands the float64 Parameter back and forward() could not assign over it; on a GPU it is a copy
    # and no Parameter -- that is the surface the port has
    del model.result
    sd = model.state_dict()
    assert tuple(sd.keys()) == dh.NAMES, tuple(sd.keys())
    weights = {n: v.detach().numpy().copy() for n, v in sd.items()}
    replay = dh.init_weights(c)
    for n in dh.NAMES:
        assert np.array_equal(weights[n], replay[n]), f"init_weights does not replay {n}"
    np.random.seed(c["draw_seed"])
    model.pre_epoch_processing()
    epoch_idx = np.asarray(model.epoch_user_graph, dtype=np.int64)
    epoch_w = model.user_weight_matrix.numpy().copy()
    lens = np.diff(C.indptr)
    assert (lens == 0).any() and ((lens > 0) & (lens < dh.UU_TOPK)).any() and (lens > dh.TOPN).sum() == 0
    users, pos, neg = (torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))
    loss = model.loss(users, pos, neg)
    loss.backward()
    result = model.result.detach().numpy().copy()
    bpr = float(model.bpr_loss(users, pos - U, neg - U, model.result).detach())
    reg = float(model.regularization_loss(users).detach())
    # (forward() has re-registered the two preference tables under DRAGON's own v_preference / t_preference as well)
    params = dict(model.named_parameters(remove_duplicate=False))
    with_grad = tuple(n for n in dh.NAMES if params[n].grad is not None)
    assert with_grad == dh.WITH_GRAD, with_grad
    ref_grads = {n: params[n].grad.detach().numpy().copy() for n in with_grad}
    # the reference's kNN lists (fp32 similarities) against the float64 ones: as sets per item
    knn = {}
    for name, emb in (("v", model.image_embedding), ("t", model.text_embedding)):
        ref_ind = model.get_knn_adj_mat(emb.weight.detach())[0][1].view(I, dh.II_TOPK).numpy()
        mine = dh.knn_indices(c[name + "_feat"], dh.II_TOPK)
        assert np.array_equal(np.sort(ref_ind, 1), np.sort(mine, 1)), f"{name}: the reference's kNN differs from the float64 one"
        knn[name] = np.sort(mine, 1)
    out = dh.step(weights, c["v_feat"], c["t_feat"], edges, U, I, epoch_idx, epoch_w, c["users"], c["pos"] - U, c["neg"] - U, dh.REG_WEIGHT,
                  dh.N_LAYERS, knn["v"], knn["t"], dh.MM_IMAGE_WEIGHT)
    g = dict(seed=c["seed"], draw_seed=c["draw_seed"], epoch_idx=epoch_idx.astype(np.int16), epoch_w=epoch_w,
             knn_v=knn["v"].astype(np.int16), knn_t=knn["t"].astype(np.int16),
             w_sum=np.array([float(weights[n].astype(np.float64).sum()) for n in dh.NAMES]),
             w_probe=np.stack([weights[n].reshape(-1)[:PROBE] for n in dh.NAMES]),
             ref_result=result, dev_result=dh.rel_dev(result, out["result"]),
             ref_loss=float(loss), dev_loss=dh.rel_dev(float(loss), out["loss"]), ref_bpr=bpr, dev_bpr=dh.rel_dev(bpr, out["bpr"]),
             ref_reg=reg, dev_reg=dh.rel_dev(reg, out["reg"]))
    print("result", g["dev_result"], "loss", g["ref_loss"], g["dev_loss"], "bpr", g["dev_bpr"], "reg", g["dev_reg"])
    devs = []
    for k, n in enumerate(dh.WITH_GRAD):
        devs.append(dh.rel_dev(ref_grads[n], out["grads"][n]))
        r = ref_grads[n]
        g[f"ref_grad_{k}"] = r[dh.GRAD_ROWS] if n.endswith("MLP.weight") else r
        print(n, "grad deviation", devs[-1], "scale", float(np.abs(out["grads"][n]).max()))
    g["dev_grads"] = np.array(devs)
    g["gscale"] = np.array([float(np.abs(out["grads"][n]).max()) for n in dh.WITH_GRAD])
    if g["dev_loss"] >= 1e-4:
        raise SystemExit(f"the reference's loss is {g['dev_loss']} from the float64 restatement: not written")
    path = os.path.join(HERE, "dragon_small.npz")
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    for case in (sys.argv[1:] or ["baby", "small"]):
        {"baby": generate_baby, "small": generate_small}[case]()
