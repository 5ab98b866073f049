"""The restatements of tests/dualgnn_host.py against the reference fixture of tests/golden/gen_dualgnn.py (no GPU): the
constructor's draws, one DualGNN step against the reference class on the synthetic graph, the epoch sample's law against the
epoch graph the reference's topk_sample drew, the fused node's restatement against plain float64 autograd; and the part of
the model's surface that needs no device (the constructor's arguments, the methods, the plumbing)."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dragon_host as dh  # noqa: E402
import dualgnn_host as gh  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def small():
    c = dh.small_case()
    f = dh.load_fixture(GOLDEN, "dualgnn_small.npz")
    w = gh.init_weights(c)
    return c, f, w


def test_init_replay_matches_the_reference(small):
    c, f, w = small
    assert tuple(w) != () and set(w) == set(gh.NAMES)
    assert int(f["seed"]) == c["seed"] and int(f["draw_seed"]) == c["draw_seed"]
    for k, n in enumerate(gh.NAMES):
        assert np.array_equal(w[n].reshape(-1)[:f["w_probe"].shape[1]], f["w_probe"][k][:w[n].size]), n
        assert abs(float(w[n].astype(np.float64).sum()) - f["w_sum"][k]) <= 1e-9 * max(1.0, abs(f["w_sum"][k])), n
    assert w["v_gcn.preference"].shape == (c["U"], gh.DIM) and w["weight_i"].shape == (c["I"], 2, 1)


def test_step_reproduces_the_reference(small):
    c, f, w = small
    U, I = c["U"], c["I"]
    out = gh.step(w, c["v_feat"], c["t_feat"], c["edges"], U, I, f["epoch_idx"], f["epoch_w"], c["users"], c["pos"] - U, c["neg"] - U,
                  gh.REG_WEIGHT)
    tight = 1.0 + 1e-6
    assert out["result"].shape == (U + I, gh.DIM)
    assert dh.rel_dev(f["ref_result"], out["result"]) <= float(f["dev_result"]) * tight
    for k in ("loss", "bpr", "reg"):
        assert dh.rel_dev(float(f["ref_" + k]), out[k]) <= float(f["dev_" + k]) * tight, k
    assert float(f["dev_loss"]) < 1e-4
    assert len(f["dev_grads"]) == len(gh.WITH_GRAD)
    for k, n in enumerate(gh.WITH_GRAD):
        mine = out["grads"][n]
        scale = float(np.abs(mine).max())
        assert scale > 0 and abs(scale - f["gscale"][k]) <= 1e-9 * scale
        sub = mine[gh.GRAD_ROWS] if n.endswith("MLP.weight") else mine
        assert np.abs(f[f"ref_grad_{k}"] - sub).max() <= float(f["dev_grads"][k]) * scale * tight, n


def test_parameters_without_gradient():
    """'weighted_sum' leaves exactly the three unused Linears without a gradient; weight_i has one, from the regulariser."""
    without = [n for n in gh.NAMES if n not in gh.WITH_GRAD]
    assert without == ["MLP_v.weight", "MLP_t.weight", "MLP_user.weight", "MLP_user.bias"]
    assert "weight_i" in gh.WITH_GRAD and "weight_i" not in dh.WITH_GRAD


def test_weight_i_gradient_is_the_regulariser_alone(small):
    c, f, w = small
    k = gh.WITH_GRAD.index("weight_i")
    want = gh.REG_WEIGHT * 2.0 * w["weight_i"].astype(np.float64) / w["weight_i"].size
    assert np.abs(f[f"ref_grad_{k}"] - want).max() <= 4 * gh.EPS32 * np.abs(want).max()


def test_sample_law_matches_the_reference_draw(small):
    """The epoch graph the reference's topk_sample drew obeys the law the restated sample follows: the first min(len, k)
    slots are the neighbours in order, every later slot repeats an EARLIER slot of the same row, the weights are the softmax
    of the slots' counts, a user without neighbours has indices 0 and weights 0."""
    c, f, _ = small
    U, I, k = c["U"], c["I"], gh.UU_TOPK
    rowptr, col = dh.history_csr(c["edges"], U)
    idx, cnt, length = dh.topn(dh.cooccurrence(rowptr, col, U, I))
    e_idx, e_w = f["epoch_idx"].astype(np.int64), f["epoch_w"].astype(np.float64)
    assert e_idx.shape == (U, k) and e_w.shape == (U, k)
    assert (length == 0).any() and ((length > 0) & (length < k)).any() and (length >= k).any()
    count_of = [dict(zip(idx[u, :length[u]].tolist(), cnt[u, :length[u]].tolist())) for u in range(U)]
    for u in range(U):
        n = min(int(length[u]), k)
        if n == 0:
            assert not e_idx[u].any() and not e_w[u].any()
            continue
        assert np.array_equal(e_idx[u, :n], idx[u, :n])
        for j in range(n, k):
            assert e_idx[u, j] in e_idx[u, :j]
        cs = np.array([count_of[u][int(i)] for i in e_idx[u]], dtype=np.float64)
        sm = np.exp(cs - cs.max())
        assert np.abs(e_w[u] - sm / sm.sum()).max() <= 4 * dh.EPS32
    m_idx, m_w, src, r = dh.sample(idx, cnt, length, k, 7, 0)
    full = length >= k
    assert np.array_equal(m_idx[full], e_idx[full]) and np.abs(m_w[full] - e_w[full]).max() <= 4 * dh.EPS32


@pytest.mark.parametrize("U,I,k", [(5, 0, 1), (9, 4, 3)])
def test_fuse_restatement_against_autograd(U, I, k):
    """fuse_fwd / fuse_bwd (the indices handled by hand, a slot outside [0, U) skipped) = float64 autograd over the plain formula."""
    rng = np.random.default_rng(U * 100 + I)
    N, D = U + I, 8
    v, t, g = (rng.standard_normal((N, D)) for _ in range(3))
    wu = rng.uniform(-1, 1, (U, 2, 1))
    idx = rng.integers(0, U, (U, k))
    w = rng.uniform(0, 1, (U, k))
    idx[U - 1, 0] = U                                                      # names an item row (or nothing): skipped
    idx[0, k - 1] = -1
    out, bound, n = gh.fuse_fwd(v, t, wu, idx, w, U)
    (dv, dt, dw), (b_dv, b_dt, b_dw), n_b = gh.fuse_bwd(g, v, t, wu, idx, w, U)
    tv, tt, tw = (torch.tensor(a, requires_grad=True) for a in (v, t, wu))
    x = tw[:, 0] * tv[:U] + tw[:, 1] * tt[:U]
    ok = torch.as_tensor((idx >= 0) & (idx < U))
    wk = torch.as_tensor(w) * ok
    res = torch.cat((x + (wk.unsqueeze(2) * x[torch.as_tensor(np.where(ok, idx, 0))]).sum(1), (tv + tt)[U:]), 0)
    res.backward(torch.as_tensor(g))
    assert n == k + 1 and out.shape == bound.shape == (N, D) and (bound >= 0).all()
    assert np.allclose(out, res.detach().numpy(), rtol=1e-13, atol=1e-13)
    for mine, ref in ((dv, tv.grad), (dt, tt.grad), (dw, tw.grad.reshape(U, 2))):
        assert np.allclose(mine, ref.numpy(), rtol=1e-13, atol=1e-13)
    assert not b_dv[U:].any() and not b_dt[U:].any() and b_dw.shape == (U, 2) and n_b >= 1


def test_model_surface():
    from chaorec_amd.registry import MODELS
    from chaorec_amd.arg_parser import load_yaml_config, parse_args
    from chaorec_amd.Model import DualGNN
    args = [p for p in inspect.signature(DualGNN.__init__).parameters][1:]
    assert args == ["num_user", "num_item", "edge_index", "user_item_dict", "v_feat", "t_feat", "dim_E", "feature_embedding",
                    "reg_weight", "uu_topk", "aggr_mode", "device"]                                                # main.py:280
    for name in ("forward", "loss", "bpr_loss", "regularization_loss", "pre_epoch_processing", "topk_sample", "init_weight",
                 "gene_ranklist", "set_epoch_graph"):
        assert callable(getattr(DualGNN, name)), name
    assert DualGNN.fused_aggregation is True and DualGNN.user_graph_path is None
    assert MODELS["DualGNN"].pre_epoch
    a = parse_args(["--Model", "DualGNN"])
    assert a.Model == "DualGNN" and a.uu_topk == 10
    cfg = load_yaml_config("DualGNN")
    assert cfg["reg_weight"] == [0.01] and cfg["learning_rate"] == [0.0001]
    assert set(cfg["hyper_parameters"]) == {"reg_weight", "learning_rate"}
    # what build_model hands the constructor and sets on the class (tests/test_model_registry.py replays this record against the table)
    built = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_constructor_args.json")))["DualGNN"]
    assert built[0] == "DualGNN" and built[3] == {"DualGNN.user_graph_path": "DATA_ROOT/sports/user_graph_dict.npy"}
    assert MODELS["DualGNN"].features


def test_model_rejects_unequal_widths():
    from chaorec_amd.Model import DualGNN
    feat = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="feature_embedding"):
        DualGNN(2, 3, np.array([[0, 2], [1, 3]]), {0: [2], 1: [3]}, feat, feat, 64, 32, 0.01, 2, "add", torch.device("cpu"))
    with pytest.raises(ValueError, match="dim_E"):
        DualGNN(2, 3, np.array([[0, 2], [1, 3]]), {0: [2], 1: [3]}, feat, feat, 96, 96, 0.01, 2, "add", torch.device("cpu"))


def test_header_declares_the_entries():
    from chaorec_amd import _lib
    assert {"chaorec_dualgnn_fuse_fwd_f32", "chaorec_dualgnn_fuse_bwd_f32"} <= set(_lib.SIGNATURES)
    assert _lib.ABI_VERSION == 16
    assert len([n for n in _lib.SIGNATURES if n.startswith("chaorec_usergraph_")]) == 6       # DRAGON's exports are untouched
