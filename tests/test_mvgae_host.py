"""MVGAE host logic (no GPU): the float64 restatements (tests/mvgae_host.py) against the REFERENCE golden of
tests/golden/gen_mvgae.py and against float64 autograd over the reference's lines, the model surface (signature, methods,
the 96 names in order, bit-equal initial values, buffers, CLI, YAML), the C ABI and the compiled kernels' resources.

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
import mvgae_host as mh  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def within(x, ref, dev, what):
    accept.within(what, x, ref, dev, accept.ULP24)


def make_model(c, device="cpu", n_layers=mh.N_LAYERS):
    from chaorec_amd.Model import MVGAE
    torch.manual_seed(c["seed"])
    return MVGAE(c["U"], c["I"], c["edges"], mh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
                 mh.DIM_E, mh.KL_WEIGHT, n_layers, torch.device(device))


def random_tail_case(N, B, U, seed, lo=-8.0, hi=11.5):
    rng = np.random.default_rng(seed)
    tabs = [rng.standard_normal((N, mh.D)) if k % 2 == 0 else rng.uniform(lo, hi, (N, mh.D)) for k in range(6)]
    users = rng.integers(0, U, B)
    pos, neg = rng.integers(U, N, B), rng.integers(U, N, B)
    return tabs, users, pos, neg, rng.standard_normal((4, N, mh.D))


def test_restatement_meets_reference():
    g, c = mh.load_fixture(GOLDEN), mh.small_case()
    assert (g["U"], g["I"], g["seed"]) == (c["U"], c["I"], c["seed"]) and tuple(g["names"].tolist()) == mh.NAMES
    weights, plain = mh.init_weights(c)
    for k, n in enumerate(mh.NAMES):
        x = weights[n]
        assert float(x.astype(np.float64).sum()) == float(g["w_sum"][k]), n
        assert np.array_equal(x.reshape(-1)[:g["w_probe"].shape[1]], g["w_probe"][k][:x.size]), n
    assert g["keep"].shape == (12, c["U"] + c["I"], 64) and g["eps"].shape == (4, c["U"] + c["I"], 64)
    out = mh.step(weights, plain, c, c["users"], c["pos"], c["neg"], mh.KL_WEIGHT, mh.N_LAYERS, g["keep"], g["eps"], True)
    within(g["ref_loss"], out["loss"], g["dev_loss"], "loss")
    within(g["ref_result"], out["result"], g["dev_result"], "result_embed")
    for k in range(8):
        within(g["ref_parts"][k], out["parts"][k], g["dev_parts"][k], f"part {k}")
    names = mh.with_grad(mh.N_LAYERS)
    assert len(names) == 66 and len(g["dev_grads"]) == 66
    for k, n in enumerate(names):
        within(g[f"ref_grad_{k}"], out["grads"][n], g["dev_grads"][k], f"grad {n}")
    ev = mh.step(weights, plain, c, c["users"], c["pos"], c["neg"], mh.KL_WEIGHT, mh.N_LAYERS, None, None, False)
    within(g["ref_eval_loss"], ev["loss"], g["dev_eval_loss"], "eval loss")
    within(g["ref_eval_result"], ev["result"], g["dev_eval_result"], "eval result")
    # the case holds what it says: a user in three samples, an item positive in one sample and negative in another
    assert np.bincount(c["users"]).max() >= 3 and len(set(c["pos"]) & set(c["neg"])) >= 1


@pytest.mark.parametrize("training", [True, False])
def test_tail_backward_is_the_derivative_of_the_references_lines(training):
    tabs, users, pos, neg, eps = random_tail_case(41, 19, 11, 5)
    tabs[1][3, 7] = 10.0                 # the clamp's edge, in a row the batch names and in one it does not
    users[0] = 3
    tabs[3][40, 0] = 10.0
    tabs[5][2, 2] = 10.75
    total, parts, pm, grads = mh.tail_torch(tabs, users, pos, neg, 0.1, eps, training, torch.float64)
    f = mh.tail(tabs, users, pos, neg, 0.1, eps, training)
    mine = mh.tail_bwd(tabs, users, pos, neg, 0.1, eps, training)
    assert abs(f["total"] - total) <= 1e-12 * abs(total) and mh.rel_dev(f["parts"], parts) <= 1e-12 and mh.rel_dev(f["Pm"], pm) <= 1e-12
    for a, b in zip(mine, grads):
        assert mh.rel_dev(a, b) <= 1e-11
    scaled = mh.tail_bwd(tabs, users, pos, neg, 0.1, eps, training, gtotal=-2.5)
    assert all(np.array_equal(s, -2.5 * m) for s, m in zip(scaled, mine))


def test_clamp_passes_gradient_at_ten_and_not_above():
    """torch's clamp(max=10) hands the gradient through where logvar <= 10, equality included.  With kl_weight alone (no
    batch influence: B = 1 elsewhere) view V's own term at an element is kl_weight * (-0.5 / N) * (1 - e^lc) or 0."""
    tabs, users, pos, neg, eps = random_tail_case(9, 1, 3, 9)
    users[:], pos[:], neg[:] = 0, 4, 5
    out = {}
    for name, l in (("at", 10.0), ("above", float(np.nextafter(10.0, 11.0))), ("far", 11.5)):
        t = [x.copy() for x in tabs]
        t[1][8, 1] = l                   # Vl of a row the batch does not name
        out[name] = mh.tail_bwd(t, users, pos, neg, 0.1, eps, True)[1][8, 1]
        ref = mh.tail_torch(t, users, pos, neg, 0.1, eps, True, torch.float64)[3][1][8, 1]
        assert abs(out[name] - ref) <= 1e-12 * max(abs(ref), 1e-30), name
    own = 0.1 * (-0.5 / 9) * (1 - np.exp(10.0))
    assert abs((out["at"] - out["above"]) - own) <= 1e-6 * abs(own) and abs(own) > 100
    assert abs(out["above"]) < 1.0


@pytest.mark.parametrize("training", [True, False])
def test_conv_epilogue_is_the_references_lines(training):
    rng = np.random.default_rng(3)
    N = 21
    s, bias, gy = rng.standard_normal((N, 64)), 0.1 * rng.standard_normal(64), rng.standard_normal((N, 64))
    keep = rng.random((N, 64)) >= 0.1
    keep[4] = False                      # a fully dropped row
    s[6] = -np.abs(s[6]) - 1.0           # a negative-only row
    y, backward = mh.conv_tail_torch(s, bias, keep, training, torch.float64)
    gs, gb = backward(gy)
    assert mh.rel_dev(mh.conv_tail(s, bias, keep, training), y) <= 1e-14
    mine = mh.conv_tail_bwd(gy, s, bias, keep, training)
    assert mh.rel_dev(mine[0], gs) <= 1e-12 and mh.rel_dev(mine[1], gb) <= 1e-12
    if training:
        assert not mh.conv_tail(s, bias, keep, True)[4].any() and not mine[0][4].any()
    assert (mh.conv_tail(s, bias, keep, training)[6][keep[6] | (not training)] < 0).all()
    # a row whose norm is below 1e-12: q = a / 1e-12, and clamp_min hands gq / 1e-12 through
    z = np.zeros((1, 64))
    tiny = mh.conv_tail_bwd(gy[:1], z, z[0], np.ones((1, 64), bool), False)[0]
    assert np.allclose(tiny, gy[:1] * 0.01 / 1e-12)       # (q = 0: the leaky slope's side)


def test_counter_rng_restatement():
    m = mh.keep_mask(1234, 3, 7, 500)
    assert m.shape == (500, 64) and abs(m.mean() - 0.9) <= 5 * np.sqrt(0.09 / m.size)
    assert not np.array_equal(m, mh.keep_mask(1234, 4, 7, 500)) and not np.array_equal(m, mh.keep_mask(1234, 3, 8, 500))
    assert np.array_equal(m, mh.keep_mask(1234, 3, 7, 500))


def test_slot_index_order():
    users, pos, neg = np.array([5, 2, 5]), np.array([7, 5, 7]), np.array([5, 7, 2])
    ptr, perm = mh.slot_index(users, pos, neg, 9)
    assert perm[ptr[5]:ptr[6]].tolist() == [0, 2, 4, 6]           # as user (samples 0, 2), as positive (1), as negative (0)
    assert perm[ptr[7]:ptr[8]].tolist() == [3, 5, 7] and perm[ptr[2]:ptr[3]].tolist() == [1, 8] and ptr[9] == 9


def test_model_surface():
    g, c = mh.load_fixture(GOLDEN), mh.small_case()
    from chaorec_amd.Model import MVGAE
    assert list(inspect.signature(MVGAE.__init__).parameters) == [
        "self", "num_user", "num_item", "edge_index", "user_item_dict", "v_feat", "t_feat", "dim_E", "reg_weight", "n_layers", "device"]
    m = make_model(c)
    sd = m.state_dict()
    assert tuple(sd.keys()) == mh.NAMES == tuple(g["names"].tolist()) and len(sd) == 96
    assert [n for n, _ in m.named_parameters()] == list(mh.NAMES)
    for k, n in enumerate(mh.NAMES):
        x = sd[n].numpy()
        assert float(x.astype(np.float64).sum()) == float(g["w_sum"][k]), n
        assert np.array_equal(x.reshape(-1)[:g["w_probe"].shape[1]], g["w_probe"][k][:x.size]), n
    _, plain = mh.init_weights(c)
    assert np.array_equal(m.collaborative.numpy(), plain["collaborative"]) and np.array_equal(m.result_embed.numpy(), plain["result_embed"])
    for gcn in ("v_gcn", "t_gcn", "c_gcn"):
        assert np.array_equal(getattr(m, gcn).preference.numpy(), plain[f"{gcn}.preference"])
    buffers = dict(m.named_buffers())
    assert sorted(buffers) == ["c_gcn.preference", "collaborative", "t_gcn.preference", "v_gcn.preference"]
    assert not any(b.requires_grad for b in buffers.values()) and m.c_gcn.features is None       # (read through the owner: follows model.to())
    for f in ("forward", "loss", "gene_ranklist", "reparametrize", "kl_loss", "bpr_loss", "recon_loss", "dot_product_decode",
              "dot_product_decode_neg"):
        assert callable(getattr(m, f)), f
    assert MVGAE.fused_tail is True and MVGAE.fused_conv is True and (m.kl_weight, m.n_layers, m.concate, m.aggr_mode) == (0.1, 2, False, "add")
    assert [tuple(t.shape) for t in m.capture_state_tensors()] == [(2,)] and m._state.dtype == torch.int64
    assert m.seed == c["seed"] and m.full_sort_predict.__func__ is m.gene_ranklist.__func__
    assert len(mh.with_grad(2)) == 66 and len(mh.with_grad(1)) == 54 and len(mh.with_grad(3)) == 78
    # the reference's methods in plain torch agree with the restatement on the CPU
    tabs, users, pos, neg, eps = random_tail_case(c["U"] + c["I"], 8, c["U"], 2)
    t32 = [torch.tensor(t, dtype=torch.float32) for t in tabs]
    f = mh.tail([t.numpy() for t in t32], users, pos, neg, 0.1, eps.astype(np.float32), True)
    total, parts, pm = m._plain_tail(t32, *(torch.from_numpy(x) for x in (users, pos, neg)), torch.from_numpy(eps.astype(np.float32)))
    assert mh.rel_dev(float(total), f["total"]) <= 1e-5 and mh.rel_dev(parts.numpy(), f["parts"]) <= 1e-5 and mh.rel_dev(pm.numpy(), f["Pm"]) <= 1e-5


def test_cli_and_yaml():
    from chaorec_amd import main as cli
    from chaorec_amd.arg_parser import load_yaml_config, parse_args
    cfg = load_yaml_config("MVGAE")
    assert cfg["hyper_parameters"] == ["reg_weight", "learning_rate", "n_layers"]
    assert (cfg["learning_rate"], cfg["reg_weight"], cfg["n_layers"]) == ([0.1], [0.1], [2])
    c = mh.small_case()
    args = parse_args(["--Model", "MVGAE", "--data_path", "sports"])
    args.reg_weight, args.n_layers = 0.1, 2
    m = cli.build_model(args, c["U"], c["I"], c["edges"], mh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]),
                        torch.from_numpy(c["t_feat"]), torch.device("cpu"))
    assert type(m).__name__ == "MVGAE" and (m.kl_weight, m.n_layers) == (0.1, 2) and not hasattr(m, "pre_epoch_processing")
    from chaorec_amd.registry import MODELS
    spec = MODELS["MVGAE"]
    assert spec.features
    assert spec.batch == "triple" and not spec.pre_epoch and spec.before_step is None and not spec.build_first


def test_ops_raise_on_cpu_tensors():
    from chaorec_amd import _lib, ops_extra
    _lib.build()
    c = mh.small_case()
    m = make_model(c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.loss(*(torch.from_numpy(c[k]) for k in ("users", "pos", "neg")))
    z = torch.zeros(5, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops_extra.mvgae_conv_tail(z, torch.zeros(64), m._state, 1, 0, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops_extra.mvgae_tail(z, z, z, z, z, z, torch.zeros(2, dtype=torch.int64), torch.ones(2, dtype=torch.int64),
                             torch.ones(2, dtype=torch.int64), 0.1, m._state, 1, True)
    with pytest.raises(ValueError, match="the kernels tile D=64"):
        ops_extra.mvgae_check_shape(32)


def test_abi_is_additive_and_every_status_is_checked():
    from chaorec_amd import _lib
    new = sorted(n for n in _lib.SIGNATURES if n.startswith("chaorec_mvgae_"))
    assert new == ["chaorec_mvgae_check_shape", "chaorec_mvgae_conv_bwd_f32", "chaorec_mvgae_conv_fwd_f32", "chaorec_mvgae_rows_per_block",
                   "chaorec_mvgae_rows_per_wave", "chaorec_mvgae_tail_bwd_f32", "chaorec_mvgae_tail_fwd_f32",
                   "chaorec_mvgae_tail_workspace_bytes", "chaorec_mvgae_tick"]
    assert _lib.ABI_VERSION == 16 and "mvgae.hip" in _lib.SOURCES
    assert _lib.INT_VALUE_EXPORTS == {"chaorec_abi_version", "chaorec_spmm_rows_per_wave", "chaorec_spmm_long_threshold",
                                      "chaorec_adam_lowrank_strips", "chaorec_adam_multi_max", "chaorec_dgcf_check_shape"}
    assert [n for n in new if _lib.SIGNATURES[n][0] is not ctypes.c_int] == ["chaorec_mvgae_rows_per_block", "chaorec_mvgae_rows_per_wave",
                                                                                        "chaorec_mvgae_tail_workspace_bytes"]
    assert len([n for n in _lib.SIGNATURES if n.startswith("chaorec_dualvae_")]) == 12        # the siblings' exports are untouched
    _lib.build()
    lib = _lib.load()
    assert (lib.chaorec_mvgae_rows_per_wave(), lib.chaorec_mvgae_rows_per_block()) == (4, 16)
    assert lib.chaorec_mvgae_check_shape(64) == 0 and lib.chaorec_mvgae_tail_workspace_bytes(17) == 2 * 4 * 8
    with pytest.raises(RuntimeError, match=r"^chaorec_mvgae_tick failed \(-1\): mvgae_tick: NULL argument"):
        lib.chaorec_mvgae_tick(None, None)
    with pytest.raises(RuntimeError, match=r"the kernels tile D=64"):
        lib.chaorec_mvgae_check_shape(128)


def test_kernels_compile_for_gfx950_without_scratch():
    """Read from the compiler's metadata; no instruction text is inspected."""
    kernels, m = kernel_meta.kernel_metadata(kernel_meta.compile_asm("mvgae.hip"))
    scratch, spills, sspills = m["scratch"], m["spills"], m["sspills"]
    assert len(kernels) == 7 and len(scratch) == len(kernels) == len(spills) == len(sspills)
    assert not any(scratch) and not any(spills) and not any(sspills)
