"""DiffMM on the CPU: the float64 restatement (tests/diffmm_host.py) against the fixture the reference class wrote
(tests/golden/gen_diffmm.py), the closed-form gradient the fused node rests on against autograd, the model's surface, the
device loader's protocol and the wiring.  No kernel runs here."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffmm_host as mh  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODS = ("image", "text")


@pytest.fixture(scope="module")
def fx():
    g, c = mh.load_fixture(GOLDEN), mh.small_case()
    assert (g["U"], g["I"], g["seed"]) == (c["U"], c["I"], c["seed"]) and np.array_equal(g["diff_users"], c["diff_users"])
    model = mh.build_model(c)
    return g, c, model, mh.weights_of(model)


def test_names_shapes_and_replayed_weights(fx):
    g, c, model, w = fx
    U, I = c["U"], c["I"]
    assert tuple(model.state_dict().keys()) == mh.NAMES == tuple(g["names"].tolist()) and len(mh.NAMES) == 19
    shapes = {"uEmbeds": (U, 64), "iEmbeds": (I, 64), "modal_weight": (2,), "image_trans_l.weight": (64, 128), "text_trans_l.weight": (64, 48),
              "denoise_model_image.in_layers.0.weight": (1000, I + 10), "denoise_model_text.out_layers.0.weight": (I, 1000),
              "denoise_model_text.emb_layer.weight": (10, 10), "denoise_model_image.out_layers.0.bias": (I,)}
    for n, s in shapes.items():
        assert tuple(w[n].shape) == s, n
    for k, n in enumerate(mh.NAMES):        # the constructor's draws replay the reference's
        assert float(w[n].astype(np.float64).sum()) == g["w_sum"][k], n
        assert np.array_equal(np.resize(w[n].reshape(-1)[:20], 20), g["w_probe"][k]), n


def test_tables_are_float64_and_keep_the_quirks(fx):
    _, _, model, _ = fx
    dm, T = model.diffusion_model, mh.tables()
    for k, attr in (("betas", "betas"), ("alphas_cumprod", "alphas_cumprod"), ("sqrt_ac", "sqrt_alphas_cumprod"),
                    ("sqrt_1mac", "sqrt_one_minus_alphas_cumprod"), ("coef1", "posterior_mean_coef1"), ("coef2", "posterior_mean_coef2")):
        t = getattr(dm, attr)       # torch's and numpy's double sqrt / division need not round alike on every CPU: 4 ulp of float64
        assert t.dtype == torch.float64 and np.allclose(t.numpy(), T[k], rtol=2.0 ** -50, atol=0), k
    assert T["betas"][0] == 0.0001                                          # pinned
    ts = torch.tensor([0, 1, 4, 0])
    w = dm.weight(ts)
    assert w.dtype == torch.float64 and np.allclose(w.numpy(), mh.snr_weight(ts.numpy()), rtol=2.0 ** -48, atol=0)
    assert w[0] == 1.0 and float(dm.SNR(ts - 1)[0]) == float(dm.SNR(torch.tensor([4]))[0])      # ts - 1 = -1 is read before the where


def test_restatement_meets_the_reference_diffusion_step(fx):
    g, c, _, w = fx
    rowptr, col = mh.hist_csr(c["edges"], c["U"])
    x0 = mh.dense_rows(rowptr, col, c["diff_users"], c["I"])
    assert set(g["ts"].reshape(-1).tolist()) == set(range(5))
    for m, mod in enumerate(MODS):
        h = mh.diffusion_step(w, c, mod, x0, g["ts"][m], g["noise"][m], g["keep"][m], mh.HYPER["e_loss"], torch.float64)
        assert mh.rel_dev(g[f"step_{mod}_loss"], h["loss"]) < 1e-4 and float(g[f"dev_step_{mod}_loss"]) < 1e-4
        assert mh.rel_dev(g[f"step_{mod}_diff"], h["diff_loss"]) < 1e-6 and mh.rel_dev(g[f"step_{mod}_gc"], h["gc_loss"]) < 1e-6
        for n, ref in h["grads"].items():
            s = ref[::8] if n.endswith("in_layers.0.weight") else ref[:, ::8] if n.endswith("out_layers.0.weight") else ref
            assert g["grad_" + n].shape == s.shape
            assert np.abs(g["grad_" + n] - s).max() <= 1e-5 * np.abs(ref).max() and float(g["dev_grad_" + n]) < 1e-5, n


def test_restatement_meets_the_reference_rebuild_and_loss(fx):
    g, c, _, w = fx
    U, I = c["U"], c["I"]
    rowptr, col = mh.hist_csr(c["edges"], U)
    xa = mh.dense_rows(rowptr, col, np.arange(U), I)
    dense = []
    for mod in MODS:
        its = mh.p_sample(w, mod, xa, torch.float64)
        for k in range(5):
            assert mh.rel_dev(g[f"iter_{mod}"][k], its[k]) < 1e-5
        s = np.sort(its[-1], 1)
        assert ((s[:, -1] - s[:, -2]) / np.abs(its[-1]).max()).min() >= 1e-3
        assert np.array_equal(np.argmax(its[-1], 1), g[f"top_{mod}"][:, 0])
        row, cl, val = mh.build_ui(np.arange(U), g[f"top_{mod}"][:, 0], U, I)
        pre = g[f"adj_{mod}_pre"]
        order = np.argsort(pre[0] * (U + I) + pre[1], kind="stable")
        assert np.array_equal(pre[0][order], row) and np.array_equal(pre[1][order], cl)
        assert np.abs(g[f"adj_{mod}_pre_val"][order] - val).max() <= 2.0 ** -23      # (a double pow may round otherwise elsewhere)
        r2, c2, v2 = mh.edge_drop(pre[0], pre[1], g[f"adj_{mod}_pre_val"], g[f"adj_{mod}_rand"])
        assert np.array_equal(np.stack([r2, c2]), g[f"adj_{mod}_idx"]) and np.array_equal(v2, g[f"adj_{mod}_val"])
        dense.append(mh.dense_adj(r2, c2, v2, U + I, torch.float64))
    h = mh.model_loss(w, c, dense[0], dense[1], c["users"], c["pos"], c["neg"], torch.float64)
    assert mh.rel_dev(g["loss"], h["loss"]) < 1e-4 and mh.rel_dev(g["usr"], h["usr"]) < 1e-5 and mh.rel_dev(g["itm"], h["itm"]) < 1e-5
    for n, ref in h["grads"].items():
        assert mh.rel_dev(g["grad_" + n], ref) < 1e-5, n
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from conftest import tie_aware_rank_equal
    idx, val = mh.ranklist(g["usr"], g["itm"], rowptr, col, U, g["rank"].shape[1])
    s = np.asarray(g["usr"], dtype=np.float64) @ np.asarray(g["itm"], dtype=np.float64).T
    for u in range(U):
        s[u, col[rowptr[u]:rowptr[u + 1]]] = 1e-6
    ok, why = tie_aware_rank_equal(g["rank"], np.take_along_axis(s, g["rank"] - U, 1), idx, val, atol=1e-6)
    assert ok, why


@pytest.mark.parametrize("B,I,Hd", [(1, 1, 4), (5, 33, 8), (24, 97, 1000)])
def test_closed_form_gradient_is_autograd(B, I, Hd):
    """d loss / d out = c_b (out - x0) + k r F^T with r = h M + b_out F - x0 E, M = W_out^T F: dW_out, dh, db_out of the
    closed form equal float64 autograd of the reference's lines to rounding, also under an incoming gradient."""
    rng = np.random.default_rng(B * 1000 + I)
    h, W = np.tanh(rng.standard_normal((B, Hd))), rng.standard_normal((I, Hd)) * 0.05
    b, F, E = rng.standard_normal(I) * 0.01, rng.standard_normal((I, 64)) * 0.3, rng.standard_normal((I, 64)) * 0.1
    x0 = (rng.random((B, I)) < 0.2).astype(np.float64)
    wt = mh.snr_weight(rng.integers(0, 5, B))
    cf = mh.closed_form(h, W, b, x0, x0 @ E, F, wt, 0.01)
    assert np.allclose(cf["r"], (h @ W.T + b) @ F - x0 @ E, rtol=0, atol=1e-13 * max(1.0, np.abs(cf["r"]).max()))
    for g in (1.0, 0.37):
        au = mh.node_all(h, W, b, x0, x0 @ E, F, wt, 0.01, torch.float64, g=g)
        for k in ("dW_out", "dh", "db_out"):
            assert np.abs(g * cf[k] - au[k]).max() <= 1e-13 * max(np.abs(au[k]).max(), 1e-300), k
        assert np.allclose(cf["diff_rows"], au["diff_rows"], rtol=1e-13, atol=0) and np.allclose(cf["gc_rows"], au["gc_rows"], rtol=1e-12, atol=0)


def test_noised_rows_restatement_rounds_twice():
    """x_t = fl(fl(a x0) + fl(s n)) in float32 equals torch's q_sample on float32 tensors bit for bit."""
    rng = np.random.default_rng(3)
    x0 = (rng.random((7, 33)) < 0.3).astype(np.float32)
    n, keep, ts = rng.standard_normal((7, 33)).astype(np.float32), rng.random((7, 33)) < 0.5, rng.integers(0, 5, 7)
    T = mh.tables()
    a, s = (torch.from_numpy(T[k])[torch.from_numpy(ts)].float()[:, None] for k in ("sqrt_ac", "sqrt_1mac"))
    ref = (a * torch.from_numpy(x0) + s * torch.from_numpy(n)) * (torch.from_numpy(keep).float() * 2.0)
    assert np.array_equal(mh.noised_rows(x0, ts, n, keep), ref.numpy())
    bits = mh.bit_table(x0)
    assert bits.shape == (7, 2) and all(((bits[b, i // 32] >> (i % 32)) & 1) == x0[b, i] for b in range(7) for i in range(33))


def test_tensor_op_graph_builders_meet_the_fixture(fx):
    """buildUIMatrix / edgeDropper restated as tensor operations: the reference's adjacency before the drop (indices exactly,
    values to one float32 rounding) and, with the recorded uniforms given in our entry order, after it."""
    g, c, model, _ = fx
    U, I = c["U"], c["I"]
    for mod in MODS:
        built = model.buildUIMatrix(torch.arange(U), torch.from_numpy(g[f"top_{mod}"][:, 0]))
        pre = g[f"adj_{mod}_pre"]
        order = np.argsort(pre[0] * (U + I) + pre[1], kind="stable")           # the reference's entries in row-major order
        assert np.array_equal(built._indices().numpy(), pre[:, order])
        assert np.abs(built._values().numpy() - g[f"adj_{mod}_pre_val"][order]).max() <= 2.0 ** -23
        dropped = model.edgeDropper(built, torch.from_numpy(g[f"adj_{mod}_rand"][order])).coalesce()
        post = g[f"adj_{mod}_idx"]
        o2 = np.argsort(post[0] * (U + I) + post[1], kind="stable")
        assert np.array_equal(dropped.indices().numpy(), post[:, o2])
        assert np.abs(dropped.values().numpy() - g[f"adj_{mod}_val"][o2]).max() <= 2.0 ** -22
        assert 0.3 < post.shape[1] / pre.shape[1] < 0.7


def test_loader_every_user_once_and_no_dense_matrix():
    from chaorec_amd.dataload import DeviceUserBatches
    U, B = 1003, 128
    ld = DeviceUserBatches(U, B, torch.device("cpu"), seed=5)
    for _ in range(2):
        batches = list(ld)
        assert len(batches) == len(ld) == 8 and [len(b) for b in batches] == [128] * 7 + [107]
        assert np.array_equal(np.sort(torch.cat(batches).numpy()), np.arange(U))
    assert not np.array_equal(torch.cat(list(ld)).numpy(), torch.cat(list(ld)).numpy())      # a fresh shuffle per epoch
    assert np.array_equal(torch.cat(list(DeviceUserBatches(U, B, torch.device("cpu"), shuffle=False))).numpy(), np.arange(U))
    # sizes at which a [U, I] fp32 matrix is 4 TB: the loader holds ids only
    big = DeviceUserBatches(10 ** 6, 1024, torch.device("cpu"))
    first = next(iter(big))
    assert first.shape == (1024,) and first.dtype == torch.int64 and len(big) == 977


def test_batch_rows_come_from_the_history_csr(fx):
    _, c, model, _ = fx
    rowptr, col = mh.hist_csr(c["edges"], c["U"])
    users = torch.tensor([5, 0, 5, 52])
    assert np.array_equal(model.batch_rows(users).numpy(), mh.dense_rows(rowptr, col, users.numpy(), c["I"]))
    assert not any(t.numel() >= c["U"] * c["I"] and t.dim() == 2 and t.shape == (c["U"], c["I"])
                   for t in list(model.buffers()) + [v for v in model.__dict__.values() if torch.is_tensor(v)])


def test_wiring():
    from chaorec_amd import epochs, main as cmain
    from chaorec_amd.registry import MODELS
    from chaorec_amd.arg_parser import load_yaml_config, parse_args
    args = parse_args(["--Model", "DiffMM", "--e_loss", "0.5", "--rebuild_k", "3"])
    assert (args.e_loss, args.ris_lambda, args.rebuild_k) == (0.5, 0.5, 3)
    assert parse_args(["--Model", "DiffMM"]).e_loss == 0.1 and parse_args([]).rebuild_k == 1
    cfg = load_yaml_config("DiffMM")
    assert cfg["hyper_parameters"] == ["e_loss", "learning_rate", "reg_weight", "ssl_alpha", "ris_lambda", "ssl_temp", "rebuild_k"]
    assert cfg["e_loss"] == [0.01] and cfg["rebuild_k"] == [1] and cfg["n_layers"] == [1]
    assert not MODELS["DiffMM"].capture and MODELS["DiffMM"].epoch is epochs._train_epoch_diffmm
    c = mh.small_case()
    for p in cfg["hyper_parameters"]:
        setattr(args, p, cfg[p][0])
    args.dim_E = 64
    m = cmain.build_model(args, c["U"], c["I"], c["edges"], mh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]),
                          torch.from_numpy(c["t_feat"]), torch.device("cpu"))
    assert type(m).__name__ == "DiffMM" and m.fused_denoise is True and (m.e_loss, m.rebuild_k, m.ris_lambda) == (0.01, 1, 0.5)
    from chaorec_amd import _lib
    for name in ("chaorec_diffmm_rows_f32", "chaorec_diffmm_out_loss_f32", "chaorec_diffmm_check_shape", "chaorec_diffmm_tiles"):
        assert name in _lib.SIGNATURES
    assert "diffmm.hip" in _lib.SOURCES
