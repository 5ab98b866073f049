"""MHRec without a GPU: the float64 restatement (tests/mhrec_host.py) against the golden the reference's own run left
(tests/golden/mhrec_small.npz), its written-out layer gradients against autograd, ops_extra.HyperGraph's construction and
validation, the model's names, replayed weights and count-valued diffusion rows, and the glue (CLI options, YAML, loop)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import mhrec_host as mh  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ULP = accept.ULP24


@functools.lru_cache(maxsize=None)
def case():
    g = mh.load_fixture(GOLDEN)
    c = mh.small_case(g["seed"])
    return c, mh.init_weights(c), g, mh.draws(c)


def close(x, ref, dev, what, scale=None):
    accept.within(what, x, ref, dev, ULP, scale=scale)


# ---- the restatement against the golden ----------------------------------------------------------------------------------------
def test_names_and_replayed_weights():
    c, w, g, _ = case()
    assert tuple(g["names"].tolist()) == mh.NAMES == tuple(w.keys()) and len(mh.NAMES) == 31
    assert [n for n in mh.NAMES if n.endswith("W.weight")] == list(mh.HYPER_W)          # the layers' unused W is there
    assert sum(n.startswith("denoise_model_") for n in mh.NAMES) == 12
    assert w["hypergraphLayersVisual.0.a"].shape == (128, 1) and w["denoise_model_text.in_layers.0.weight"].shape == (1000, c["U"] + c["I"] + 10)


def test_input_hyperedges_are_the_reference_s():
    c, _, g, _ = case()
    v, t = mh.input_hyperedges(c)
    assert np.array_equal(v, g["hyper_visual"]) and np.array_equal(t, g["hyper_textual"])
    assert v.shape == (len(c["edges"]), 2 + mh.HYPER["uu_topk"] + mh.HYPER["ii_topk"])
    assert np.array_equal(v[:, 0], c["edges"][:, 0]) and np.array_equal(v[:, 1 + mh.HYPER["uu_topk"]], c["edges"][:, 1])


def test_one_step_meets_the_golden():
    c, w, g, dr = case()
    h = mh.step_losses(w, c, g["nodes0"][0], g["nodes0"][1], dr["fwd_keep"][0])
    close(g["loss"], h["loss"], g["dev_loss"], "loss")
    assert h["max_exp"] <= 20
    close(g["result8"], h["result"][:8], g["dev_result"], "result", np.abs(h["result"]).max())
    for k, n in enumerate(mh.WITH_GRAD):
        close(g["grad8_" + n], h["grads"][n][:8], g["dev_grads"][k], f"grad {n}", np.abs(h["grads"][n]).max())
    for k in range(4):
        close(g["layer_outs8"][k], h["layer_outs"][k][:8], g["dev_layer_outs"][k], f"layer {k}", np.abs(h["layer_outs"][k]).max())
    s = mh.rank_scores(h["result"], c)
    got = g["rank"] - c["U"]
    best = np.sort(s, 1)[:, ::-1][:, :mh.TOPK]
    # (the reference ranks its own fp32 table, off by dev_result ~ 1e-6 per factor: its ten are the float64 best ten to 1e-5)
    assert got.shape == (c["U"], mh.TOPK) and all(len(set(r)) == mh.TOPK for r in got.tolist())
    assert np.abs(np.take_along_axis(s, got, 1) - best).max() <= 1e-5 * np.abs(s).max()


def test_rebuilt_hypergraphs_meet_the_golden():
    c, w, g, dr = case()
    N = c["U"] + c["I"]
    nodes, gap = mh.rebuild(mh.cast(w, torch.float64), c, g["hyper_visual"].astype(np.int64), dr["rebuild_noise"])
    assert gap >= 2e-5
    for k in range(2):
        assert np.array_equal(np.sort(nodes[k], 1), np.sort(g["nodes0"][k], 1))
        for name in ("nodes0", "nodes1"):
            deg = np.bincount(g[name][k].reshape(-1).astype(np.int64), minlength=N)
            assert deg.min() == 0 and deg.max() > 64 and all(len(set(r)) == mh.HYPER["num_hypernodes"] for r in g[name][k].tolist())


def test_epoch_meets_the_golden():
    c, w, g, dr = case()
    ep = mh.epoch(w, c, g["hyper_visual"].astype(np.int64), dr)
    close(g["epoch_diff_losses"], ep["diff_losses"], g["dev_epoch_diff_losses"], "diffusion losses")
    close(g["epoch_losses"], ep["losses"], g["dev_epoch_losses"], "BPR losses")
    for k in range(2):
        assert np.array_equal(np.sort(ep["nodes"][k], 1), np.sort(g["nodes1"][k], 1))
    for k, n in enumerate(mh.NAMES):
        upd = ep["weights"][n] - w[n]
        close(g["epoch8_" + n] - w[n][:8], upd[:8], g["dev_epoch"][k], f"update of {n}", np.abs(upd).max())


# ---- the layer's written-out gradients -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 10])
def test_written_out_gradients_equal_autograd(k):
    lc = mh.layer_case(k)
    a = mh.layer_autograd(lc["X"], lc["a"], lc["nodes"], lc["keep"], lc["g"], torch.float64)
    b = mh.layer_grads(lc["X"], lc["a"], lc["nodes"], lc["keep"], lc["g"])
    da = np.concatenate([b["da1"], b["da2"]])
    assert mh.rel_dev(b["out"], a["out"]) < 1e-12 and mh.rel_dev(b["y"], a["y"]) < 1e-12 and mh.rel_dev(b["dX"], a["dX"]) < 1e-12
    assert mh.rel_dev(da, a["da"]) < 1e-12 and np.abs(b["da1"]).max() < 1e-10 * np.abs(b["da2"]).max()
    assert b["max_exp"] <= 20 and not b["out"][6].any() and b["deg"][6] == 0


def test_closed_form_of_the_node_side_sum():
    """sum_j de_nj = t_n (1 - sum_j alpha_nj) = t_n 1e-16 / (Z_n + 1e-16): what csrc/mhrec.hip evaluates."""
    lc = mh.layer_case(3)
    X, a, g = (np.asarray(v, dtype=np.float64) for v in (lc["X"], lc["a"], lc["g"]))
    h = mh.layer_grads(X, a, lc["nodes"], lc["keep"], g)
    node, hedge = lc["nodes"].reshape(-1), np.repeat(np.arange(len(lc["nodes"])), lc["k"])
    Ej = X[lc["nodes"]].sum(1)
    w = np.exp((X @ a[:64])[node] + (Ej @ a[64:])[hedge])
    Z = np.bincount(node, weights=w, minlength=lc["N"])
    t = (np.where(lc["keep"], 2.0, 0.0) * g * h["out"]).sum(1)
    closed = (X * (t * 1e-16 / (Z + 1e-16))[:, None]).sum(0)
    assert np.abs(closed - h["da1"]).max() <= 1e-12 * np.abs(h["da2"]).max()


# ---- ops_extra.HyperGraph ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 10])
def test_hypergraph_construction(k):
    from chaorec_amd import ops_extra
    lc = mh.layer_case(k)
    nodes, N = lc["nodes"], lc["N"]
    hg = ops_extra.HyperGraph(torch.from_numpy(nodes), N)
    E = len(nodes)
    assert hg.nodes.dtype == torch.int32 and hg.edge.dtype == torch.int32 and hg.rowptr.dtype == torch.int64
    assert (hg.num_nodes, hg.num_edges, hg.k) == (N, E, k) and np.array_equal(hg.nodes.numpy(), nodes)
    deg = np.bincount(nodes.reshape(-1), minlength=N)
    assert np.array_equal(hg.rowptr.numpy(), np.concatenate([[0], np.cumsum(deg)]))
    edge, rowptr = hg.edge.numpy(), hg.rowptr.numpy()
    for n in range(N):
        mine = edge[rowptr[n]:rowptr[n + 1]]
        assert np.array_equal(mine, np.nonzero((nodes == n).any(1))[0]), n              # its hyperedges, ascending
    assert ops_extra.MHREC_LONG_ROW == mh.LONG_ROW
    assert hg.long_node.tolist() == [0, 2] and hg.long_cptr.tolist() == [0, 2, 4] and hg.chunk_node.tolist() == [0, 0, 2, 2]
    assert hg.chunk_beg.tolist() == [0, ops_extra.MHREC_CHUNK, int(rowptr[2]), int(rowptr[2]) + ops_extra.MHREC_CHUNK]
    H = hg.incidence().to_dense().numpy()
    assert H.shape == (N, E) and np.array_equal(H.sum(1), deg) and np.all(H.sum(0) == k)


def test_hypergraph_validation():
    from chaorec_amd import ops_extra
    good = torch.tensor([[0, 1, 2], [2, 3, 4]])
    ops_extra.HyperGraph(good, 5)
    for bad in (torch.tensor([[0, 1, 5], [2, 3, 4]]), torch.tensor([[0, 1, -1], [2, 3, 4]])):
        with pytest.raises(ValueError, match="node ids"):
            ops_extra.HyperGraph(bad, 5)
    with pytest.raises(ValueError, match="twice"):
        ops_extra.HyperGraph(torch.tensor([[0, 1, 2], [3, 4, 3]]), 5)
    with pytest.raises(ValueError):
        ops_extra.HyperGraph(torch.tensor([0, 1, 2]), 5)
    with pytest.raises(ValueError):
        ops_extra.HyperGraph(torch.tensor([[0.0, 1.0]]), 5)
    with pytest.raises(ValueError):
        ops_extra.mhrec_check_shape(32)
    ops_extra.mhrec_check_shape(64)


# ---- the model and the glue ----------------------------------------------------------------------------------------------------
def test_state_dict_keys_and_shared_diffusion_classes():
    import chaorec_amd.Model  # noqa: F401
    dm, mr = sys.modules["chaorec_amd.Model.DiffMM"], sys.modules["chaorec_amd.Model.MHRec"]   # (the package's attributes are the classes)
    c = case()[0]
    m = mh.build_model(c)
    assert tuple(m.state_dict().keys()) == mh.NAMES
    assert mr.Denoise is dm.Denoise and mr.GaussianDiffusion is dm.GaussianDiffusion        # shared, not copied
    assert type(m.denoise_model_image) is dm.Denoise and m.image_diffusion_model.steps == 20 and m.denoise_model_text.time_emb_dim == 10
    T = mh.tables()
    assert np.array_equal(m.text_diffusion_model.posterior_mean_coef1.numpy(), T["coef1"])
    assert m.fused_hyper is True


def test_diffusion_rows_hold_counts():
    c = case()[0]
    N = c["U"] + c["I"]
    m = mh.build_model(c)
    table = np.array([[0, 3, 3, 5], [1, 1, 1, 69], [2, 4, 6, 8]])
    m.set_input_hyperedges(table, table + 0)
    rows = m.diffusion_rows(torch.tensor([1, 0, 2])).numpy()
    assert rows.shape == (3, N) and np.array_equal(rows, mh.dense_rows(table, [1, 0, 2], N))
    assert rows[0, 1] == 3 and rows[1, 3] == 2 and rows.sum() == 12
    v, t = m.diffusion_tables()
    assert v is t                                                               # the reference reads the visual file twice


def test_cli_yaml_and_loop_entries():
    from chaorec_amd import arg_parser, epochs
    from chaorec_amd.registry import MODELS
    a = arg_parser.parse_args(["--Model", "MHRec"])
    assert (a.h_layers, a.num_hypernodes, a.beta1, a.beta2) == (2, 10, 0.5, 0.5)
    cfg = arg_parser.load_yaml_config("MHRec")
    assert set(cfg["hyper_parameters"]) == {"n_layers", "h_layers", "learning_rate", "reg_weight", "uu_topk", "ii_topk", "num_hypernodes",
                                            "ssl_alpha", "ssl_temp", "beta1", "beta2"}
    assert all(isinstance(cfg[k], list) and len(cfg[k]) == 1 for k in cfg["hyper_parameters"])
    assert not MODELS["MHRec"].capture and MODELS["MHRec"].epoch is epochs._train_epoch_mhrec


def test_diffusion_step_in_double_is_the_restatement():
    """diffusion_double: the loss is the float64 restatement's, the fp32 gradients are its gradients rounded once; the switch
    gives the reference's fp32 lines back (the same loss to fp32 rounding)."""
    c, w, g, dr = case()
    N = c["U"] + c["I"]
    m = mh.build_model(c).train()
    m.set_input_hyperedges(g["hyper_visual"], g["hyper_textual"])
    batch = c["batches"][2]
    draws = [torch.from_numpy(np.asarray(dr[k][1][2])) for k in ("ts", "noise", "keep")]
    wt = mh.cast(w, torch.float64, mh.DENOISE)
    ref = mh.diffusion_loss(wt, "text", mh.dense_rows(g["hyper_visual"].astype(np.int64), batch, N), dr["ts"][1][2], dr["noise"][1][2], dr["keep"][1][2])
    ref.backward()
    assert m.diffusion_double is True
    loss = m.diffusion_step(torch.from_numpy(batch), 1, *draws)
    loss.backward()
    assert loss.dtype == torch.float64 and abs(float(loss.detach()) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
    for n, p in m.denoise_model_text.named_parameters():
        assert p.grad.dtype == torch.float32 and mh.rel_dev(p.grad.numpy(), wt["denoise_model_text." + n].grad.numpy()) <= 2 * ULP, n
    assert all(p.grad is None for p in m.denoise_model_image.parameters())
    m.diffusion_double = False
    l32 = m.diffusion_step(torch.from_numpy(batch), 1, *draws)
    assert abs(float(l32.detach()) - float(ref.detach())) <= 1e-5 * abs(float(ref.detach()))
