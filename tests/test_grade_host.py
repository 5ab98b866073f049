"""Grade host logic (no GPU): the float64 restatement (tests/grade_host.py) against the REFERENCE golden of
tests/golden/gen_grade.py, the model surface (signature, the 46 names in order, bit-equal initial values, the frozen feature
tables, CLI, YAML, the training loop's branch), the owner list of the pair launch, the C ABI and the compiled kernels' resources.

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
import grade_host as gh  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ULP = accept.ULP24


def within(x, ref, dev, what):
    accept.within(what, x, ref, dev, ULP)


def fixture_case():
    g = gh.load_fixture(GOLDEN)
    return g, gh.small_case(g["seed"])


def make_model(c, device="cpu", n_layers=gh.N_LAYERS, dim=gh.DIM_E):
    from chaorec_amd.Model import Grade
    torch.manual_seed(c["seed"])
    return Grade(c["U"], c["I"], c["edges"], gh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]), dim,
                 gh.REG_WEIGHT, n_layers, gh.SSL_TEMP, gh.SSL_ALPHA, gh.SSL_TEMP2, gh.NOISE_ALPHA, torch.device(device))


def test_small_case_holds_what_it_says():
    g, c = fixture_case()
    G = gh.graph_arrays(c)
    lens = np.bincount(G["row"], minlength=G["N"])
    assert (c["U"], c["I"], c["B"]) == (90, 72, 64) and 1350 <= G["E"] <= 1550 and G["E"] % 64 and (G["E"] // 2) % 64
    assert c["v_feat"].shape == (72, gh.FV) and c["t_feat"].shape == (72, gh.FT) and (gh.FV, gh.FT) == (128, 96)
    assert (lens == 0).sum() >= 2 and lens.max() >= 70 and lens.max() > 64
    assert np.array_equal(G["row"][G["tentry"]], G["col"]) and np.array_equal(G["col"][G["tentry"]], G["row"])
    assert np.all(np.diff(G["row"] * G["N"] + G["col"]) > 0)                       # row-major, columns ascending, distinct
    assert np.bincount(c["users"]).max() >= 3 and len(set(c["pos"]) & set(c["neg"])) >= 1
    assert np.all(np.bincount(G["mm_row"], minlength=c["I"]) >= gh.KNN_K) and np.all(np.diff(G["mm_row"] * c["I"] + G["mm_col"]) > 0)
    # what the generator refuses to write without
    fracs = g["keep"].mean(1)
    assert ((fracs >= 0.2) & (fracs <= 0.8)).any() and g["dropped_rows"].max() >= 1 and not g["keep_flips"].any()
    assert g["logit_min_abs"] >= 16 * g["logit_abs_dev"] > 0
    assert os.path.getsize(os.path.join(GOLDEN, "grade_small.npz")) < 600_000


def test_owner_list_reaches_every_entry_once():
    from chaorec_amd import ops_extra
    _, c = fixture_case()
    G = gh.graph_arrays(c)
    st = make_model(c).norm_adj_mat
    owner = st.pair_owner                                                           # built at construction, cached on the structure
    assert ops_extra.grade_pair_owner(st) is owner and owner.dtype == torch.int32
    o = owner.numpy().astype(np.int64)
    assert np.array_equal(o, gh.owner_list(G)) and len(o) == G["E"] // 2              # bipartite: exactly the user rows' entries
    assert np.all(G["row"][o] <= G["col"][o]) and np.all(G["row"][o] < c["U"])
    reached = np.concatenate([o, G["tentry"][o][G["tentry"][o] != o]])
    assert np.array_equal(np.sort(reached), np.arange(G["E"]))
    # a pattern with diagonal entries: they own themselves and are reached once
    from chaorec_amd import graph, sparse
    row, col = np.array([0, 0, 1, 1, 2]), np.array([1, 2, 0, 1, 0])
    st5 = sparse._dropout_structure(graph.coo_to_csr_coalesced(torch.from_numpy(row), torch.from_numpy(col), torch.ones(5), 4, 4, symmetric=True))
    o5 = ops_extra.grade_pair_owner(st5).numpy()
    t5 = st5.transpose_entry.numpy()
    assert o5.tolist() == [0, 1, 3] and t5[3] == 3
    assert sorted(o5.tolist() + [int(t5[e]) for e in o5 if t5[e] != e]) == [0, 1, 2, 3, 4]


def test_restatement_meets_reference():
    g, c = fixture_case()
    G = gh.graph_arrays(c)
    assert (g["U"], g["I"], g["E"]) == (c["U"], c["I"], G["E"]) and tuple(g["names"].tolist()) == gh.NAMES
    weights = gh.init_weights(c)
    for k, n in enumerate(gh.NAMES):
        x = weights[n]
        assert float(x.astype(np.float64).sum()) == float(g["w_sum"][k]), n
        assert np.array_equal(np.resize(x.reshape(-1)[:g["w_probe"].shape[1]], g["w_probe"].shape[1]), g["w_probe"][k]), n
    dr = gh.draws(c, 1)[0]
    assert [float(t.astype(np.float64).sum()) for t in dr["randn1"] + dr["rand"] + dr["randn2"]] == g["draw_sums"].tolist()
    out = gh.step_losses(weights, c, dr)
    for name in gh.LOSSES:
        within(g[f"ref_{name}"], out[name], g[f"dev_{name}"], name)
        assert g[f"dev_{name}"] < 1e-4 and len(g[f"dev_grads_{name}"]) == len(gh.WITH_GRAD[name])
        for k, n in enumerate(gh.WITH_GRAD[name]):
            assert np.isfinite(g[f"ref_grad_{name}_{k}"]).all()
            within(g[f"ref_grad_{name}_{k}"], gh.stored(n, out["grads"][name][n]), g[f"dev_grads_{name}"][k], f"{name}: grad {n}")
    W, Gr = gh.tensors(weights, requires_grad=False), gh.Graph(c)
    lens = np.bincount(G["row"], minlength=G["N"])
    for k in range(3):
        mine = gh.view(W, Gr, k + 1, torch.tensor(dr["randn1"][k], dtype=torch.float64))
        near = np.abs(mine["logit"].numpy()) < 16 * g["logit_abs_dev"]
        assert near.sum() <= 0.01 * G["E"] and np.array_equal(mine["keep"].numpy()[~near], g["keep"][k][~near])
        within(g["view_logits"][k], mine["logit"].numpy(), g["dev_view_logits"][k], f"generator {k + 1} logits")
        within(g["view_vals"][k], mine["val"].numpy(), g["dev_view_vals"][k], f"generator {k + 1} values")
        kept_in_row = np.bincount(G["row"], weights=g["keep"][k], minlength=G["N"])
        assert int(((lens >= 3) & (kept_in_row == 0)).sum()) == int(g["dropped_rows"][k])
        assert not g["view_vals"][k][~g["keep"][k]].any() and (g["view_vals"][k][g["keep"][k]] > 0).all()


def test_trajectory_meets_reference():
    g, c = fixture_case()
    weights = gh.init_weights(c)
    final, losses = gh.trajectory(weights, c, gh.draws(c, gh.N_STEPS, seed_offset=2))
    within(g["traj_losses"], losses, g["dev_traj_losses"], "trajectory losses")
    for k, n in enumerate(gh.NAMES):
        if n in gh.FROZEN:
            assert np.array_equal(final[n], weights[n]) and f"traj_{k}" not in g
            continue
        within(g[f"traj_{k}"] - gh.stored(n, weights[n]), gh.stored(n, final[n] - weights[n]), g["dev_traj"][k], f"update of {n}")
        assert np.abs(final[n] - weights[n]).max() > 0, n                      # every parameter moved


def test_rank_list_meets_reference():
    g, c = fixture_case()
    s = gh.rank_scores(gh.init_weights(c), c)
    ref = g["ranklist"].astype(np.int64) - c["U"]
    assert ref.shape == (c["U"], gh.TOPK)
    mine = np.sort(s, 1)[:, ::-1][:, :gh.TOPK]
    assert np.abs(np.take_along_axis(s, ref, 1) - mine).max() <= 1e-6 * np.abs(s).max()


def test_model_surface():
    g, c = fixture_case()
    from chaorec_amd.Model import Grade
    from chaorec_amd import graph
    assert list(inspect.signature(Grade.__init__).parameters) == [
        "self", "num_user", "num_item", "edge_index", "user_item_dict", "v_feat", "t_feat", "dim_E", "reg_weight", "n_layers", "ssl_temp",
        "ssl_alpha", "ssl_temp2", "noise_alpha", "device"]
    m = make_model(c)
    sd = m.state_dict()
    assert tuple(sd.keys()) == gh.NAMES == tuple(g["names"].tolist()) and len(sd) == 46
    w = gh.init_weights(c)
    for k, n in enumerate(gh.NAMES):
        assert np.array_equal(sd[n].numpy(), w[n]), n
        assert float(w[n].astype(np.float64).sum()) == float(g["w_sum"][k]), n
    # the frozen feature tables: in the state_dict, parameters without gradient, the given values
    params = dict(m.named_parameters())
    assert [n for n in gh.NAMES if not params[n].requires_grad] == list(gh.FROZEN)
    assert np.array_equal(sd["v_feat.weight"].numpy(), c["v_feat"]) and np.array_equal(sd["t_feat.weight"].numpy(), c["t_feat"])
    for k in (1, 2, 3):
        assert [n for n, _ in getattr(m, f"generator_{k}").named_parameters()] == [n[len("generator_1."):] for n in gh.GEN[k]]
    for f in ("loss_1", "bpr_reg_loss", "gen_loss", "gene_ranklist", "forward_gcn", "forward_graphcl", "visual_forward_graphcl",
              "textual_forward_graphcl", "noise_visual_forward_graphcl", "noise_textual_forward_graphcl", "loss_graphcl",
              "generator_generate", "buildItemGraph", "feed_draws"):
        assert callable(getattr(m, f)), f
    assert Grade.fused_edges in (True, False) and (m.knn_k, m.mm_image_weight, m.mm_layers) == (10, 0.5, 1)
    assert m._fused() is bool(Grade.fused_edges) and make_model(c, dim=32)._fused() is False
    # one structure for every view: the reference's entry order, values and the reversed-entry map; the item graph
    G = gh.graph_arrays(c)
    st = m.norm_adj_mat
    assert isinstance(st, graph.DropoutStructure)
    assert np.array_equal(st.entry_row.numpy(), G["row"]) and np.array_equal(st.col.numpy(), G["col"])
    assert np.array_equal(st.val.numpy(), G["val"]) and np.array_equal(st.transpose_entry.numpy(), G["tentry"])
    assert np.array_equal(m.mm_adj.col.numpy(), G["mm_col"]) and gh.rel_dev(m.mm_adj.val.numpy(), G["mm_val"]) <= 2 * ULP
    assert m.full_sort_predict.__func__ is m.gene_ranklist.__func__
    # given draws are consumed in call order
    m.feed_draws(randn=[np.zeros((2, 2), np.float32), np.ones((2, 2), np.float32)], rand=[np.full((2, 2), 0.5, np.float32)])
    assert float(m._take("randn").sum()) == 0.0 and float(m._take("randn").sum()) == 4.0 and m._take("randn") is None
    assert float(m._take("rand").sum()) == 2.0 and m._take("rand") is None
    doc = sys.modules[Grade.__module__].__doc__
    for said in ("[B, 1]", "KL weight is 1", "MSE", "zero_grad", "generator 1's view", "ONE uniform table", "decided ONCE"):
        assert said in doc, said


def test_cli_yaml_and_training_branch():
    from chaorec_amd import epochs, main as cli
    from chaorec_amd.registry import MODELS
    from chaorec_amd.arg_parser import load_yaml_config, parse_args
    cfg = load_yaml_config("Grade")
    assert cfg["hyper_parameters"] == ["n_layers", "learning_rate", "reg_weight", "ssl_alpha", "ssl_temp", "ssl_temp2", "noise_alpha"]
    assert all(len(cfg[p]) == 1 for p in cfg["hyper_parameters"])
    assert [cfg[p][0] for p in cfg["hyper_parameters"]] == [5, 0.001, 0.1, 0.2, 0.3, 0.3, 0.2]
    _, c = fixture_case()
    args = parse_args(["--Model", "Grade", "--data_path", "sports"])
    assert isinstance(args.noise_alpha, float) and (args.noise_alpha, args.ssl_temp2) == (0.3, 0.2)
    assert parse_args(["--Model", "Grade", "--noise_alpha", "0.25"]).noise_alpha == 0.25
    for p in cfg["hyper_parameters"]:
        setattr(args, p, cfg[p][0])
    m = cli.build_model(args, c["U"], c["I"], c["edges"], gh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]),
                        torch.from_numpy(c["t_feat"]), torch.device("cpu"))
    assert type(m).__name__ == "Grade"
    assert (m.ssl_temp, m.ssl_alpha, m.ssl_temp2, m.noise_alpha, m.reg_weight, m.n_layers) == (0.3, 0.2, 0.3, 0.2, 0.1, 5)
    spec = MODELS["Grade"]
    assert spec.features
    assert not spec.capture and spec.batch == "triple" and not spec.pre_epoch and spec.before_step is None and not spec.build_first
    src = inspect.getsource(epochs._train_epoch_grade)
    assert src.count("torch.optim.Adam(") == 4 and src.count("opt.step()") == 2 and "eps=" not in src
    order = [src.index(s) for s in ("model.loss_1(", "model.bpr_reg_loss(", "model.gen_loss(", "opt_gen_1.step()", "opt_gen_2.step()",
                                    "opt_gen_3.step()")]
    assert order == sorted(order) and src.index("opt.step()") < src.index("model.bpr_reg_loss(") < src.rindex("opt.step()") < src.index("model.gen_loss(")
    assert spec.epoch is epochs._train_epoch_grade


def test_training_branch_steps_in_the_reference_s_order():
    """The loop's branch over a stand-in model: which loss is stepped by which optimizer, in which order."""
    from chaorec_amd import epochs as te
    import types

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.ones(1))
            self.generator_1, self.generator_2, self.generator_3 = (torch.nn.Linear(1, 1, bias=False) for _ in range(3))
            self.calls = []

        def _loss(self, name, scale):
            self.calls.append((name, float(self.a.detach()), [float(g.weight.detach()) for g in (self.generator_1, self.generator_2, self.generator_3)]))
            return scale * (self.a.sum() + sum(g.weight.sum() for g in (self.generator_1, self.generator_2, self.generator_3)))

        def loss_1(self, *b):
            return self._loss("loss_1", 1.0)

        def bpr_reg_loss(self, *b):
            return self._loss("bpr_reg_loss", 1.0)

        def gen_loss(self, *b):
            return self._loss("gen_loss", 1.0)

    m = Tiny()
    g0 = [float(g.weight.detach()) for g in (m.generator_1, m.generator_2, m.generator_3)]
    total = te._train_epoch_grade(m, [(None, None, None)] * 2, types.SimpleNamespace(param_groups=[{"lr": 0.5}]))
    assert [c[0] for c in m.calls] == ["loss_1", "bpr_reg_loss", "gen_loss"] * 2 and np.isfinite(total)
    a = [c[1] for c in m.calls]
    # `opt` steps a (and, being over ALL parameters, the generators) after loss_1 and after bpr_reg_loss; gen_loss steps only the generators
    assert a[1] < a[0] and a[2] < a[1] and a[3] == a[2] and a[4] < a[3]
    gens = [c[2] for c in m.calls]
    assert all(x < y for x, y in zip(gens[1], g0)) and all(x < y for x, y in zip(gens[3], gens[2]))      # gen_loss's own step


def test_ops_raise_on_cpu_tensors_and_on_another_width():
    from chaorec_amd import _lib, ops_extra
    _lib.build()
    _, c = fixture_case()
    m = make_model(c)
    st = m.norm_adj_mat
    z = torch.zeros(st.n_rows, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops_extra.grade_views(st, z, torch.zeros(64, 64), torch.zeros(64), torch.zeros(1, 64), torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.loss_1(*(torch.from_numpy(c[k]) for k in ("users", "pos", "neg")))
    with pytest.raises(ValueError, match="the kernels tile D=64"):
        ops_extra.grade_check_shape(32)
    ops_extra.grade_check_shape(64)


def test_abi_is_additive_and_every_status_is_checked():
    from chaorec_amd import _lib
    new = sorted(n for n in _lib.SIGNATURES if n.startswith("chaorec_grade_"))
    assert new == ["chaorec_grade_check_shape", "chaorec_grade_views_f32"]
    assert _lib.ABI_VERSION == 16 and "grade.hip" in _lib.SOURCES and _lib.SOURCES[-1] == "adagcl.hip"
    assert _lib.SOURCES.index("grade.hip") < _lib.SOURCES.index("adagcl.hip")
    assert not any(n.startswith("chaorec_grade_") for n in _lib.INT_VALUE_EXPORTS)
    assert all(_lib.SIGNATURES[n][0] is ctypes.c_int for n in new)
    assert len([n for n in _lib.SIGNATURES if n.startswith("chaorec_adagcl_")]) == 7          # the sibling's exports are untouched
    _lib.build()
    lib = _lib.load()
    assert lib.chaorec_grade_check_shape(64) == 0
    with pytest.raises(RuntimeError, match=r"^chaorec_grade_check_shape failed \(-1\): grade_check_shape: D=128, the kernels tile D=64"):
        lib.chaorec_grade_check_shape(128)
    with pytest.raises(RuntimeError, match=r"^chaorec_grade_views_f32 failed \(-1\): grade_views: NULL argument"):
        lib.chaorec_grade_views_f32(*([None] * 5), 3, 4, *([None] * 4), 4, None, 2, *([None] * 5), None)


def test_kernels_compile_for_gfx950_without_scratch():
    """Read from the compiler's metadata; no instruction text is inspected."""
    kernels, m = kernel_meta.kernel_metadata(kernel_meta.compile_asm("grade.hip"))
    scratch, spills, sspills, lds = m["scratch"], m["spills"], m["sspills"], m["lds"]
    assert len(kernels) == 3 and len(scratch) == len(kernels) == len(spills) == len(sspills) == len(lds)
    assert not any(scratch) and not any(spills) and not any(sspills)
    assert max(lds) == 64 * 64 * 4 + 2 * 64 * 4                 # the pair launch: one generator's W1 and its two 64-float vectors
