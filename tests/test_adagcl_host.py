"""AdaGCL host logic (no GPU): the float64 restatement (tests/adagcl_host.py) against the REFERENCE golden of
tests/golden/gen_adagcl.py, the model surface (signature, the 26 names in order, bit-equal initial values, the snapshot of
the initial embeddings, CLI, YAML, the training loop's branch), the per-node factorisation of the gate's logit, the C ABI
and the compiled kernels' resources.

Bounds: every reference quantity is stored with its own fp32-vs-fp64 deviation; a check allows 4 x max(that, 2^-24)."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import kernel_meta  # noqa: E402
import adagcl_host as ah  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def within(x, ref, dev, what):
    accept.within(what, x, ref, dev, accept.ULP24)


def make_model(c, device="cpu", n_layers=ah.N_LAYERS, dim=ah.DIM_E):
    from chaorec_amd.Model import AdaGCL
    torch.manual_seed(c["seed"])
    return AdaGCL(c["U"], c["I"], c["edges"], ah.user_item_dict(c["edges"]), dim, ah.REG_WEIGHT, n_layers, ah.SSL_TEMP, ah.SSL_ALPHA,
                  torch.device(device))


def test_small_case_holds_what_it_says():
    c = ah.small_case()
    G = ah.graph_arrays(c)
    lens = np.bincount(G["row"], minlength=G["N"])
    assert (c["U"], c["I"], c["B"]) == (83, 29, 64) and 280 <= G["E"] // 2 <= 340 and G["E"] % 64 and G["E"] % 128
    assert (lens == 0).sum() == 2 and lens.max() >= 70 and lens.max() > 64
    assert np.array_equal(G["row"][G["tentry"]], G["col"]) and np.array_equal(G["col"][G["tentry"]], G["row"])
    assert np.all(np.diff(G["row"] * G["N"] + G["col"]) > 0)                       # row-major, columns ascending, distinct
    assert np.bincount(c["users"]).max() >= 3 and len(set(c["pos"]) & set(c["neg"])) >= 1
    for d in ah.draws(c, 1)[0]["u"]:
        assert d.dtype == np.float32 and d.min() >= np.float32(1e-7) and d.max() <= np.float32(1.0 - 1e-7)


def test_restatement_meets_reference():
    g, c = ah.load_fixture(GOLDEN), ah.small_case()
    G = ah.graph_arrays(c)
    assert (g["U"], g["I"], g["seed"], g["E"]) == (c["U"], c["I"], c["seed"], G["E"]) and tuple(g["names"].tolist()) == ah.NAMES
    weights = ah.init_weights(c)
    for k, n in enumerate(ah.NAMES):
        x = weights[n]
        assert float(x.astype(np.float64).sum()) == float(g["w_sum"][k]), n
        assert np.array_equal(np.resize(x.reshape(-1)[:g["w_probe"].shape[1]], g["w_probe"].shape[1]), g["w_probe"][k]), n
    dr = ah.draws(c, 1)[0]
    assert [float(t.astype(np.float64).sum()) for t in dr["randn"] + dr["u"]] == g["draw_sums"].tolist()
    out = ah.step_losses(weights, c, dr)
    for name in ah.LOSSES:
        within(g[f"ref_{name}"], out[name], g[f"dev_{name}"], name)
        assert g[f"dev_{name}"] < 1e-4 and len(g[f"dev_grads_{name}"]) == len(ah.WITH_GRAD[name])
        for k, n in enumerate(ah.WITH_GRAD[name]):
            assert np.isfinite(g[f"ref_grad_{name}_{k}"]).all()
            within(g[f"ref_grad_{name}_{k}"], out["grads"][name][n], g[f"dev_grads_{name}"][k], f"{name}: grad {n}")
    W, Gr = ah.tensors(weights, requires_grad=False), ah.Graph(c)
    vals, keep, logits = ah.keep_view(W, Gr, torch.tensor(dr["randn"][0], dtype=torch.float64))
    near = np.abs(logits.numpy()) < 16 * g["keep_logit_abs_dev"]
    assert near.sum() <= 0.01 * G["E"] and np.array_equal(keep.numpy()[~near], g["keep"][~near]) and g["keep_flips"] == 0
    assert 0 < g["keep"].sum() < G["E"]
    within(g["keep_logits"], logits.numpy(), g["dev_keep_logits"], "keep logits")
    within(g["keep_vals"], vals.numpy(), g["dev_keep_vals"], "kept values")
    x = torch.cat([W["uEmbeds"], W["iEmbeds"]], 0)
    h0 = ah.gate(W, Gr, x, 0, 1.0, False)
    t0 = ah.gate(W, Gr, x, 0, ah.SSL_TEMP, True, dr["u"][0])
    mine = dict(eval0=h0, eval1=ah.gate(W, Gr, ah.spmm(Gr, h0["val"], x), 1, 1.0, False), train0=t0,
                train1=ah.gate(W, Gr, ah.spmm(Gr, t0["val"], x), 1, ah.SSL_TEMP, True, dr["u"][1]))
    for tag, m in mine.items():
        within(g[f"gate_{tag}"], m["val"].numpy(), g[f"dev_gate_{tag}"], f"gate values {tag}")


def test_trajectory_meets_reference():
    g, c = ah.load_fixture(GOLDEN), ah.small_case()
    weights = ah.init_weights(c)
    final, losses = ah.trajectory(weights, c, ah.draws(c, ah.N_STEPS, seed_offset=2))
    within(g["traj_losses"], losses, g["dev_traj_losses"], "trajectory losses")
    for k, n in enumerate(ah.NAMES):
        within(g[f"traj_{k}"] - weights[n], final[n] - weights[n], g["dev_traj"][k], f"update of {n}")
        assert np.abs(final[n] - weights[n]).max() > 0, n                      # every parameter moved


def test_rank_list_meets_reference():
    g, c = ah.load_fixture(GOLDEN), ah.small_case()
    s = ah.rank_scores(ah.init_weights(c), c)
    ref = g["ranklist"].astype(np.int64) - c["U"]
    assert ref.shape == (c["U"], ah.TOPK)
    mine = np.sort(s, 1)[:, ::-1][:, :ah.TOPK]
    assert np.abs(np.take_along_axis(s, ref, 1) - mine).max() <= 1e-6 * np.abs(s).max()


def test_gate_logit_is_two_node_scores():
    """logit[e] = s_nb[row e] + s_self[col e] + b: the model's node scores against its own per-edge lines and the restatement's."""
    c = ah.small_case()
    m, G = make_model(c), ah.Graph(c)
    w = ah.init_weights(c)
    W = ah.tensors(w, requires_grad=False)
    x32 = torch.cat([m.uEmbeds, m.iEmbeds], 0).detach()
    for layer in (0, 1):
        s_nb, s_self, b = m.generator_2.node_scores(x32, layer)
        per_edge = m.generator_2.get_attention(x32[G.row], x32[G.col], layer)[:, 0]
        ref = ah.gate(W, G, x32.double(), layer, 1.0, False)["logit"]
        assert ah.rel_dev((s_nb[G.row] + s_self[G.col] + b).detach().numpy(), ref.numpy()) <= 1e-5
        assert ah.rel_dev(per_edge.detach().numpy(), ref.numpy()) <= 1e-5


def test_a_third_layer_and_another_width_raise():
    from chaorec_amd import _lib, ops_extra
    c = ah.small_case()
    m = make_model(c, n_layers=3)
    x = torch.cat([m.uEmbeds, m.iEmbeds], 0).detach()
    assert len(m.gcnLayers) == 3
    for call in (lambda: m.generator_2.get_attention(x[:4], x[:4], layer=2), lambda: m.generator_2.node_scores(x, 2),
                 lambda: m.generator_2.gate(x, 2, 1.0, False)):
        with pytest.raises(ValueError, match="Invalid layer value, must be 0 or 1"):
            call()
    with pytest.raises(ValueError, match="the kernels tile D=64"):
        ops_extra.adagcl_check_shape(32)
    ops_extra.adagcl_check_shape(64)
    _lib.build()
    lib = _lib.load()
    assert lib.chaorec_adagcl_check_shape(64) == 0
    with pytest.raises(RuntimeError, match=r"^chaorec_adagcl_check_shape failed \(-1\): adagcl_check_shape: D=128, the kernels tile D=64"):
        lib.chaorec_adagcl_check_shape(128)
    assert lib.chaorec_last_error().decode().startswith("adagcl_check_shape: D=128")
    assert make_model(c, dim=32)._fused() is False and make_model(c)._fused() is True


def test_model_surface():
    g, c = ah.load_fixture(GOLDEN), ah.small_case()
    from chaorec_amd.Model import AdaGCL
    from chaorec_amd import graph
    assert list(inspect.signature(AdaGCL.__init__).parameters) == [
        "self", "num_user", "num_item", "edge_index", "user_item_dict", "dim_E", "reg_weight", "n_layers", "ssl_temp", "ssl_alpha", "device"]
    m = make_model(c)
    sd = m.state_dict()
    assert tuple(sd.keys()) == ah.NAMES == tuple(g["names"].tolist()) and len(sd) == 26
    assert [n for n, _ in m.named_parameters()] == list(ah.NAMES)
    w = ah.init_weights(c)
    for k, n in enumerate(ah.NAMES):
        assert np.array_equal(sd[n].numpy(), w[n]), n
        assert float(w[n].astype(np.float64).sum()) == float(g["w_sum"][k]), n
    assert [n for n, _ in m.generator_1.named_parameters()] == [n[len("generator_1."):] for n in ah.GEN_1]
    assert [n for n, _ in m.generator_2.named_parameters()] == [n[len("generator_2."):] for n in ah.GEN_2]
    for f in ("loss_1", "loss_2", "bpr_reg_loss", "gen_loss", "gene_ranklist", "forward_gcn", "forward_graphcl", "forward_graphcl_",
              "loss_graphcl", "generator_generate", "getEmbeds", "getGCN", "unfreeze"):
        assert callable(getattr(m, f)), f
    assert AdaGCL.fused_edges is True and (m.ib_reg, m.generator_2.lambda0, m.generator_2.gamma, m.generator_2.zeta) == (0.01, 0.0001, -0.45, 1.05)
    # the snapshot of the INITIAL embeddings: a copy, not refreshed when the embeddings move
    feats = m.generator_2.features
    assert not feats.requires_grad and np.array_equal(feats.numpy(), np.concatenate([w["uEmbeds"], w["iEmbeds"]], 0))
    with torch.no_grad():
        m.uEmbeds.add_(1.0)
    assert np.array_equal(m.generator_2.features.numpy(), np.concatenate([w["uEmbeds"], w["iEmbeds"]], 0))
    assert "features" not in dict(m.generator_2.named_buffers())
    # one structure for every view: the reference's entry order, values and the reversed-entry map
    G = ah.graph_arrays(c)
    st = m.norm_adj_mat
    assert isinstance(st, graph.DropoutStructure) and m.generator_2.adj_mat is st
    assert np.array_equal(st.entry_row.numpy(), G["row"]) and np.array_equal(st.col.numpy(), G["col"])
    assert np.array_equal(st.val.numpy(), G["val"]) and np.array_equal(st.transpose_entry.numpy(), G["tentry"])
    assert m._state.dtype == torch.int64 and tuple(m._state.shape) == (2,) and m.seed == c["seed"]
    assert m.full_sort_predict.__func__ is m.gene_ranklist.__func__
    # given draws are consumed in call order
    m.feed_draws(randn=[np.zeros((2, 2), np.float32), np.ones((2, 2), np.float32)], u=[np.full(3, 0.5, np.float32)] * 2)
    assert float(m._take("randn")[0].sum()) == 0.0 and float(m._take("randn")[0].sum()) == 4.0 and m._take("randn") is None
    assert len(m._take("u", 2)) == 2 and m._take("u", 2) is None


def test_cli_yaml_and_training_branch():
    from chaorec_amd import epochs, main as cli
    from chaorec_amd.registry import MODELS
    from chaorec_amd.arg_parser import load_yaml_config, parse_args
    cfg = load_yaml_config("AdaGCL")
    assert cfg["hyper_parameters"] == ["n_layers", "learning_rate", "reg_weight", "ssl_alpha", "ssl_temp"]
    assert all(len(cfg[p]) == 1 for p in cfg["hyper_parameters"]) and cfg["n_layers"] == [2]
    c = ah.small_case()
    args = parse_args(["--Model", "AdaGCL", "--data_path", "sports"])
    for p in cfg["hyper_parameters"]:
        setattr(args, p, cfg[p][0])
    m = cli.build_model(args, c["U"], c["I"], c["edges"], ah.user_item_dict(c["edges"]), None, None, torch.device("cpu"))
    assert type(m).__name__ == "AdaGCL" and (m.ssl_temp, m.ssl_alpha, m.reg_weight, m.n_layers) == (0.5, 0.1, 0.001, 2)
    spec = MODELS["AdaGCL"]
    assert not spec.features
    assert not spec.capture and spec.batch == "triple" and not spec.pre_epoch and spec.before_step is None and not spec.build_first
    src = inspect.getsource(epochs._train_epoch_adagcl)
    assert "eps=0.001" in src and src.count("opt.step()") == 3 and "opt_gen_1.step()" in src and "opt_gen_2.step()" in src
    assert spec.epoch is epochs._train_epoch_adagcl


def test_ops_raise_on_cpu_tensors():
    from chaorec_amd import _lib, ops_extra
    _lib.build()
    c = ah.small_case()
    m = make_model(c)
    st = m.norm_adj_mat
    z = torch.zeros(st.n_rows, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops_extra.adagcl_edge_gate(st, z[:, 0], z[:, 0], torch.zeros(1), 1.0, 0.0, False, None, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops_extra.adagcl_edge_keep(st, z, torch.zeros(64, 64), torch.zeros(64), torch.zeros(1, 64), torch.zeros(1), st.val)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.loss_1(*(torch.from_numpy(c[k]) for k in ("users", "pos", "neg")))


def test_abi_is_additive_and_every_status_is_checked():
    from chaorec_amd import _lib
    new = sorted(n for n in _lib.SIGNATURES if n.startswith("chaorec_adagcl_"))
    assert new == ["chaorec_adagcl_check_shape", "chaorec_adagcl_gate_bwd_f32", "chaorec_adagcl_gate_fwd_f32", "chaorec_adagcl_keep_f32",
                   "chaorec_adagcl_long_row", "chaorec_adagcl_rows_per_block", "chaorec_adagcl_tick"]
    assert _lib.ABI_VERSION == 16 and "adagcl.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "adagcl.hip"
    assert not any(n.startswith("chaorec_adagcl_") for n in _lib.INT_VALUE_EXPORTS)
    assert [n for n in new if _lib.SIGNATURES[n][0] is not ctypes.c_int] == ["chaorec_adagcl_long_row", "chaorec_adagcl_rows_per_block"]
    assert len([n for n in _lib.SIGNATURES if n.startswith("chaorec_mvgae_")]) == 9          # the siblings' exports are untouched
    _lib.build()
    lib = _lib.load()
    assert (lib.chaorec_adagcl_rows_per_block(), lib.chaorec_adagcl_long_row()) == (32, 64)
    with pytest.raises(RuntimeError, match=r"^chaorec_adagcl_tick failed \(-1\): adagcl_tick: NULL argument"):
        lib.chaorec_adagcl_tick(None, None)
    with pytest.raises(RuntimeError, match=r"adagcl_gate_fwd: NULL argument"):
        lib.chaorec_adagcl_gate_fwd_f32(*([None] * 3), 4, 4, *([None] * 3), 1.0, 0.0, 0, None, 0, None, 0, *([None] * 7), 1, None)
    with pytest.raises(RuntimeError, match=r"adagcl_keep: NULL argument"):
        lib.chaorec_adagcl_keep_f32(None, 4, None, None, 4, *([None] * 9), None)


def test_kernels_compile_for_gfx950_without_scratch():
    """Read from the compiler's metadata; no instruction text is inspected."""
    kernels, m = kernel_meta.kernel_metadata(kernel_meta.compile_asm("adagcl.hip"))
    scratch, spills, sspills, lds = m["scratch"], m["spills"], m["sspills"], m["lds"]
    assert len(kernels) == 8 and len(scratch) == len(kernels) == len(spills) == len(sspills) == len(lds)
    assert not any(scratch) and not any(spills) and not any(sspills)
    assert max(lds) == 64 * 64 * 4 + 2 * 64 * 4                 # the keep kernel: W1 and the two 64-float vectors
