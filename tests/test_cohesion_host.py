"""The restatements of tests/cohesion_host.py against the reference fixture of tests/golden/gen_cohesion.py (no GPU): the
constructor's draws, one COHESION step against the reference class on the synthetic graph, which parameters the loss reaches,
the fused node's float32 restatement (the contract's order, chunked and unchunked) against its float64 one and against plain
float64 autograd; and the part of the model's surface that needs no device (the constructor's arguments, the methods, the
plumbing)."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dragon_host as dh  # noqa: E402
import cohesion_host as ch  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def small():
    c = dh.small_case()
    f = dh.load_fixture(GOLDEN, "cohesion_small.npz")
    w = ch.init_weights(c)
    return c, f, w


def _step(c, f, w, grads=True):
    U = c["U"]
    return ch.step(w, c["v_feat"], c["t_feat"], c["edges"], U, c["I"], f["epoch_idx"], f["epoch_w"], c["users"], c["pos"] - U,
                   c["neg"] - U, ch.REG_WEIGHT, ch.N_LAYERS, ch.MM_LAYERS, f["knn_v"], f["knn_t"], ch.MM_IMAGE_WEIGHT, grads=grads)


def test_init_replay_matches_the_reference(small):
    c, f, w = small
    assert tuple(w) != () and set(w) == set(ch.NAMES) and len(ch.NAMES) == 23
    assert int(f["seed"]) == c["seed"] and int(f["draw_seed"]) == c["draw_seed"]
    for k, n in enumerate(ch.NAMES):
        assert np.array_equal(w[n].reshape(-1)[:f["w_probe"].shape[1]], f["w_probe"][k][:w[n].size]), n
        assert abs(float(w[n].astype(np.float64).sum()) - f["w_sum"][k]) <= 1e-9 * max(1.0, abs(f["w_sum"][k])), n
    assert w["v_gcn.preference"].shape == (c["U"], ch.D) and w["id_feat"].shape == (c["I"], ch.D)
    assert w["weight_u"].shape == (c["U"], 2, 1) and w["id_gcn.MLP.weight"].shape == (4 * ch.D, ch.D)


def test_step_reproduces_the_reference(small):
    c, f, w = small
    U, I = c["U"], c["I"]
    out = _step(c, f, w)
    tight = 1.0 + 1e-6
    assert out["result"].shape == (U + I, 3 * ch.D)
    assert dh.rel_dev(f["ref_result"], out["result"]) <= float(f["dev_result"]) * tight
    for k in ("loss", "bpr", "reg"):
        assert dh.rel_dev(float(f["ref_" + k]), out[k]) <= float(f["dev_" + k]) * tight, k
    assert float(f["dev_loss"]) < 1e-4
    assert len(f["dev_grads"]) == len(ch.WITH_GRAD)
    for k, n in enumerate(ch.WITH_GRAD):
        mine = out["grads"][n]
        scale = float(np.abs(mine).max())
        assert scale > 0 and abs(scale - f["gscale"][k]) <= 1e-9 * scale
        sub = mine[ch.GRAD_ROWS] if n.endswith("MLP.weight") else mine
        assert np.abs(f[f"ref_grad_{k}"] - sub).max() <= float(f["dev_grads"][k]) * scale * tight, n


def test_parameters_with_a_gradient(small):
    """weight_u, id_feat, both preferences and both encoders' four MLP tensors have a gradient (the generator asserted that
    these are the reference's); the eleven others -- id_gcn.*, the two embeddings, the two projections -- have none."""
    without = [n for n in ch.NAMES if n not in ch.WITH_GRAD]
    assert len(ch.WITH_GRAD) == 12 and len(without) == 11
    assert set(without) == ({"image_embedding.weight", "text_embedding.weight", "image_trs.weight", "image_trs.bias",
                             "text_trs.weight", "text_trs.bias"} | {"id_gcn." + n for n in ch._GCN})
    # weight_u's gradient is the regulariser's alone: the forward never reads it
    c, f, w = small
    k = ch.WITH_GRAD.index("weight_u")
    want = ch.REG_WEIGHT * 2.0 * w["weight_u"].astype(np.float64) / w["weight_u"].size
    assert np.abs(f[f"ref_grad_{k}"] - want).max() <= 4 * ch.EPS32 * np.abs(want).max()


def _node_inputs(U, I, k, seed, fan_in=0):
    rng = np.random.default_rng(seed)
    N = U + I
    idr, v, t, g = ((rng.standard_normal((N, ch.D)) * np.exp(rng.uniform(-2, 2, (N, 1)))).astype(np.float32) for _ in range(4))
    g = np.concatenate((g, rng.standard_normal((N, 2 * ch.D)).astype(np.float32)), axis=1)
    h = tuple(rng.standard_normal((I, ch.D)).astype(np.float32) for _ in range(3))
    idx = rng.integers(0, U, (U, k)).astype(np.int32)
    w = rng.uniform(0, 1, (U, k)).astype(np.float32)
    if fan_in:
        idx.reshape(-1)[rng.choice(U * k, size=fan_in, replace=False)] = 1     # user 1 is named by at least fan_in slots
    return idr, v, t, h, idx, w, g


@pytest.mark.parametrize("U,I,k", [(5, 0, 1), (9, 4, 3), (40, 3, 10)])
def test_node_restatements_agree(U, I, k):
    """The float32 restatement in the contract's order lies within the float64 one's bound, and the float64 one equals plain
    float64 autograd over the reference's formula (a slot outside [0, U) skipped; the id third detached)."""
    idr, v, t, h, idx, w, g = _node_inputs(U, I, k, 100 * U + I)
    idx[U - 1, 0] = U                                                      # names an item row (or nothing): skipped
    idx[0, k - 1] = -1
    hh = h if I else None
    out32 = ch.fuse_fwd32(idr, v, t, hh, idx, w, U)
    out64, b_out, n = ch.fuse_fwd64(idr, v, t, hh, idx, w, U)
    assert n == k + 1 and out32.dtype == np.float32 and out32.shape == (U + I, 3 * ch.D)
    assert (np.abs(out32 - out64) <= b_out).all()
    (dv64, dt64), (b_dv, b_dt), _ = ch.fuse_bwd64(g, idx, w, U)
    for chunk in (0, 2, 64):
        dv, dt, dh_v, dh_t = ch.fuse_bwd32(g, idx, w, U, chunk)
        assert (np.abs(dv - dv64) <= b_dv).all() and (np.abs(dt - dt64) <= b_dt).all()
        assert np.array_equal(dh_v, g[U:, ch.D:2 * ch.D]) and np.array_equal(dh_t, g[U:, 2 * ch.D:])
    tid, tv, tt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (idr, v, t))
    th = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in h]
    x = torch.cat((tid.detach(), tv, tt), dim=1)
    ok = torch.as_tensor((idx >= 0) & (idx < U))
    wk = torch.as_tensor(w, dtype=torch.float64) * ok
    users = x[:U] + (wk.unsqueeze(2) * x[:U][torch.as_tensor(np.where(ok, idx, 0))]).sum(1)
    items = x[U:] + torch.cat((th[0].detach(), th[1], th[2]), dim=1) if I else x[U:]
    res = torch.cat((users, items), 0)
    res.backward(torch.as_tensor(g, dtype=torch.float64))
    assert np.allclose(out64, res.detach().numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(dv64, tv.grad.numpy(), rtol=1e-13, atol=1e-13) and np.allclose(dt64, tt.grad.numpy(), rtol=1e-13, atol=1e-13)
    assert tid.grad is None
    if I:
        assert np.array_equal(th[1].grad.numpy(), g[U:, ch.D:2 * ch.D].astype(np.float64)) and th[0].grad is None


def test_chunked_backward_is_the_single_walk_on_short_lists():
    """Every list at most `chunk` entries long: S_r = p_0, the unchunked walk's bits.  A longer list: other bits, within the bound."""
    U, I, k = 60, 5, 10
    idr, v, t, h, idx, w, g = _node_inputs(U, I, k, 7, fan_in=150)
    longest = int(np.diff(dh.reverse(idx, U)[0]).max())
    assert 150 <= longest <= 256
    single = ch.fuse_bwd32(g, idx, w, U, 0)
    for chunk in (longest, longest + 1, 256):
        for a, b in zip(ch.fuse_bwd32(g, idx, w, U, chunk), single):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), chunk
    cut = ch.fuse_bwd32(g, idx, w, U, 64)
    assert not np.array_equal(cut[0][1], single[0][1]) or not np.array_equal(cut[1][1], single[1][1])
    others = np.diff(dh.reverse(idx, U)[0]) <= 64
    assert others.sum() == U - 1 and np.array_equal(cut[0][:U][others], single[0][:U][others])
    (dv64, dt64), (b_dv, b_dt), n = ch.fuse_bwd64(g, idx, w, U)
    assert n == longest + 1 and (np.abs(cut[0] - dv64) <= b_dv).all() and (np.abs(cut[1] - dt64) <= b_dt).all()
    # the chunk index itself: consecutive, the last chunk of a list the short one
    rev_ptr, _, row_chunk, rows, first, end = ch.rev_chunks(idx, U, 64)
    assert row_chunk[-1] == len(rows) == np.ceil(np.diff(rev_ptr) / 64).sum()
    assert np.array_equal(first[row_chunk[:-1][np.diff(row_chunk) > 0]], rev_ptr[:-1][np.diff(row_chunk) > 0])
    assert ((end - first) <= 64).all() and ((end - first) > 0).all() and (end - first).sum() == rev_ptr[-1] - rev_ptr[0]


def test_nan_in_the_id_columns_of_g_stays_out():
    U, I, k = 12, 3, 4
    idr, v, t, h, idx, w, g = _node_inputs(U, I, k, 3)
    clean = ch.fuse_bwd32(g, idx, w, U, 2)
    g[:, :ch.D] = np.nan
    for a, b in zip(ch.fuse_bwd32(g, idx, w, U, 2), clean):
        assert np.array_equal(a, b) and np.isfinite(a).all()


def test_model_surface():
    from chaorec_amd.registry import MODELS
    from chaorec_amd.arg_parser import load_yaml_config, parse_args
    from chaorec_amd.Model import COHESION
    args = [p for p in inspect.signature(COHESION.__init__).parameters][1:]
    assert args == ["num_user", "num_item", "edge_index", "user_item_dict", "v_feat", "t_feat", "dim_E", "reg_weight", "dropout",
                    "n_layers", "mm_layers", "ii_topk", "mm_image_weight", "device"]                                # main.py:381-383
    for name in ("forward", "loss", "pre_epoch_processing", "topk_sample", "adaptive_optimization", "gene_ranklist", "set_epoch_graph",
                 "build_representation", "process_user_item_representation", "get_knn_adj_mat", "get_norm_adj_mat"):
        assert callable(getattr(COHESION, name)), name
    assert COHESION.fused_aggregation is True and COHESION.user_graph_path is None and COHESION.bwd_chunk == 64
    assert MODELS["COHESION"].pre_epoch
    assert parse_args(["--Model", "COHESION"]).Model == "COHESION"
    cfg = load_yaml_config("COHESION")
    assert cfg["mm_image_weight"] == [0.1] and cfg["reg_weight"] == [0.001] and cfg["dropout"] == [0] and cfg["n_layers"] == [1]
    assert set(cfg["hyper_parameters"]) == {"reg_weight", "learning_rate", "dropout", "n_layers", "mm_image_weight", "ii_topk", "mm_layers"}
    # what build_model hands the constructor and sets on the class (tests/test_model_registry.py replays this record against the table)
    built = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_constructor_args.json")))["COHESION"]
    assert built[0] == "COHESION" and built[3] == {"COHESION.user_graph_path": "DATA_ROOT/sports/user_graph_dict.npy"}
    assert built[1][-2] == cfg["mm_image_weight"][0] and built[1][-1] == "device"
    assert MODELS["COHESION"].features


def test_header_declares_the_entries():
    from chaorec_amd import _lib
    assert {"chaorec_cohesion_fuse_fwd_f32", "chaorec_cohesion_fuse_bwd_f32"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["chaorec_cohesion_fuse_fwd_f32"][1]) == 14 and len(_lib.SIGNATURES["chaorec_cohesion_fuse_bwd_f32"][1]) == 18
    assert _lib.ABI_VERSION == 16                                          # additive: new names only
