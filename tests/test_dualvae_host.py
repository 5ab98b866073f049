"""DualVAE host logic (no GPU): the float64 restatement (tests/dualvae_host.py) against the REFERENCE goldens of
tests/golden/gen_dualvae.py, the model surface (names, order, shapes, bit-equal initial values, the four tables outside
state_dict, CLI, YAML), the write-back winner, the C ABI and the compiled kernels' resources.

Bounds: every reference quantity is stored with its own fp32-vs-fp64 deviation; a check allows 4 x that (the reference's
own rounding noise is the floor; a formula error shows at 1e-3 and up)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import kernel_meta  # noqa: E402
import dualvae_host as dh  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["small", "sports"]


def within(x, ref, dev, what):
    accept.within(what, x, ref, dev, 0.0)


def make_model(g, device="cpu"):
    from chaorec_amd.Model import DualVAE
    torch.manual_seed(g["seed"])
    return DualVAE(g["U"], g["I"], g["edges"], dh.user_item_dict(g["edges"]), 64, dh.KL_WEIGHT, dh.SSL_REG, torch.device(device))


def host_weights(m):
    return [np.ascontiguousarray(v.detach().cpu().numpy()) for v in m.state_dict().values()]


def host_tables(m):
    return tuple(t.detach().cpu().numpy().copy() for t in (m.theta, m.beta, m.mu_theta, m.mu_beta))


@pytest.mark.parametrize("name", FIXTURES)
def test_parameters_and_tables_equal_the_references_for_the_same_seed(name):
    g = dh.load_fixture(GOLDEN, name)
    m = make_model(g)
    sd = m.state_dict()
    U, I = g["U"], g["I"]
    assert tuple(sd.keys()) == dh.NAMES and [n for n, _ in m.named_parameters()] == list(dh.NAMES) and len(sd) == 18
    enc = lambda n: [(20, n), (20,), (25, 20), (25,), (25, 20), (25,)]   # noqa: E731
    assert [tuple(v.shape) for v in sd.values()] == [(5, 25), (5, 25)] + enc(I) + enc(U) + [(20, 25), (20,), (20, 25), (20,)]
    for k, x in enumerate(host_weights(m)):
        assert float(x.astype(np.float64).sum()) == float(g["w_sum"][k]), dh.NAMES[k]
        assert np.array_equal(x.reshape(-1)[:g["w_probe"].shape[1]], g["w_probe"][k][:x.size]), dh.NAMES[k]
    # the four tables: the reference's values, plain attributes, moved by to()
    for t, s, shape in zip(host_tables(m), g["t_sum"], [(U, 5, 25), (I, 5, 25), (U, 5, 25), (I, 5, 25)]):
        assert t.shape == shape and float(t.astype(np.float64).sum()) == float(s)
    assert not any(n in sd for n in ("theta", "beta", "mu_theta", "mu_beta")) and not list(m.buffers())
    assert m.to(torch.device("cpu")) is m and m.theta.device.type == "cpu"
    # the encoder weights are transposed views of row-major [N, 20] buffers
    assert m.user_encoder.fc0.weight.stride() == (1, 20) and m.item_encoder.fc0.weight.stride() == (1, 20)
    assert (m.k, m.a, m.likelihood, m.dim_E, m.kl_weight, m.ssl_reg, m.aspect_probability) == (25, 5, "pois", 64, 0.5, 0.01, None)
    assert m.full_sort_predict.__func__ is m.gene_ranklist.__func__
    assert [tuple(t.shape) for t in m.capture_state_tensors()] == [(2,), (U, 5, 25), (I, 5, 25), (U, 5, 25), (I, 5, 25)]
    for f in ("encode_user", "encode_item", "reparameterize", "contrast_loss", "forward", "loss", "gene_ranklist"):
        assert callable(getattr(m, f))


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_meets_reference(name):
    g = dh.load_fixture(GOLDEN, name)
    m = make_model(g)
    U = g["U"]
    draws = dh.replay_draws(g["draw_seed"], len(g["users"]))
    assert np.array_equal(dh.draw_sums(draws), g["draw_sums"]), "this torch draws other values than the generator's"
    out = dh.step(host_weights(m), host_tables(m), dh.dense_matrix(g["edges"], U, g["I"]), g["users"], g["pos"] - U, *draws)
    within(g["ref_loss"], out["loss"], g["dev_loss"], f"{name} loss")
    for s in ("item", "user"):
        for k in ("kl", "ll", "cl", "loss"):
            within(g[f"ref_{s}_{k}"], out[s][k], g[f"dev_{s}_{k}"], f"{name} {s} {k}")
        for k in ("z", "nei"):
            ref = g[f"ref_{s}_{k}"]
            got = float(np.abs(ref - out[s][k][:len(ref)]).max()) / float(np.abs(out[s][k]).max())
            print(f"{name} {s} {k}: {got:.3e} (bound {accept.bound_of(g[f'dev_{s}_{k}'], 0.0):.3e})")
            assert got <= accept.bound_of(g[f"dev_{s}_{k}"], 0.0)
    for k, n in enumerate(dh.NAMES):
        got = out["grads"][k]
        if n == "user_encoder.fc0.weight":
            got = got[:, g["grad_rows_user"]]
        elif n == "item_encoder.fc0.weight":
            got = got[:, g["grad_rows_item"]]
        d = float(np.abs(g[f"ref_grad_{k}"] - got).max()) / float(np.abs(out["grads"][k]).max())   # (relative to the WHOLE array's largest element)
        print(f"{name} grad {n}: {d:.3e} (bound {accept.bound_of(g['dev_grads'][k], 0.0):.3e})")
        assert d <= accept.bound_of(g["dev_grads"][k], 0.0), n
        assert abs(float(np.linalg.norm(out["grads"][k])) - float(g["gnorm"][k])) <= 1e-9 * float(g["gnorm"][k]), n
    for k, n in enumerate(("theta", "beta", "mu_theta", "mu_beta")):
        got = float(np.abs(g[f"ref_tab_{n}"] - out["tables"][k][g[f"tab_ids_{n}"]]).max()) / float(np.abs(out["tables"][k]).max())
        assert got <= accept.bound_of(g[f"dev_tab_{n}"], 0.0), n


def test_restatement_trajectory_small():
    g = dh.load_fixture(GOLDEN, "small")
    m = make_model(g)
    U, T = g["U"], len(g["traj_users"])
    batches = [(g["traj_users"][t], g["traj_pos"][t] - U) for t in range(T)]
    losses, wT, tT = dh.adam_trajectory(host_weights(m), host_tables(m), dh.dense_matrix(g["edges"], U, g["I"]), batches,
                                        int(g["traj_seed0"]), float(g["traj_lr"]))
    assert T == 10
    within(g["traj_ref_losses"], losses, g["traj_dev_losses"], "trajectory losses")
    for k, n in enumerate(dh.NAMES):
        got = float(np.abs(wT[k].reshape(-1)[:g["traj_ref_probe"].shape[1]] - g["traj_ref_probe"][k][:wT[k].size]).max()) / float(np.abs(wT[k]).max())
        assert got <= accept.bound_of(g["traj_dev_weights"][k], 0.0), n


def test_write_back_winner_is_the_highest_batch_position():
    g = dh.load_fixture(GOLDEN, "small")
    ids, counts = np.unique(g["users"], return_counts=True)
    assert counts.max() >= 4 and np.unique(g["pos"], return_counts=True)[1].max() >= 2      # one id four times, both sides repeat
    # the batch's users lie in the batch items' rows and the reverse: every batch pair is an edge
    edges = set(map(tuple, g["edges"].tolist()))
    assert all((int(u), int(i)) in edges for u, i in zip(g["users"], g["pos"]))
    t = np.zeros((5, 2))
    dh.write_back(t, np.array([3, 1, 3, 3]), np.arange(8.0).reshape(4, 2))
    assert np.array_equal(t[3], [6.0, 7.0]) and np.array_equal(t[1], [2.0, 3.0])
    # and the reference's own table holds the LAST sample's z for the id that repeats most (test_restatement_meets_reference
    # compares whole rows; here: the stored reference row is the stored reference z of that position)
    u = int(ids[np.argmax(counts)])
    last = int(np.nonzero(g["users"] == u)[0][-1])
    row = g["ref_tab_theta"][int(np.nonzero(g["tab_ids_theta"] == u)[0][0])]
    assert np.array_equal(row, g["ref_user_z"][last])


def test_generator_refused_no_fixture_outside_the_ranking_cap():
    for name in FIXTURES:
        g = dh.load_fixture(GOLDEN, name)
        assert float(g["rank_share_s01"]) <= 0.02 and float(g["rank_share_s10"]) <= 0.02
    # ranklist_check itself: a swapped pair far apart is outside the gap, a tie is not a difference
    sc = np.array([[0.9, 0.5, 0.1, 0.3]])
    assert dh.ranklist_check(np.array([[0, 1]]), sc, {}, [0], 2, 0) == (0.0, 0)
    assert dh.ranklist_check(np.array([[1, 0]]), sc, {}, [0], 2, 0) == (1.0, 2)
    assert dh.ranklist_check(np.array([[0, 3]]), sc, {0: [1]}, [0], 2, 0) == (0.0, 0)          # a history entry holds 1e-6


def test_cli_and_yaml():
    from chaorec_amd import main as cli
    from chaorec_amd.arg_parser import load_yaml_config, parse_args
    cfg = load_yaml_config("DualVAE")
    assert cfg["hyper_parameters"] == ["learning_rate", "reg_weight", "ssl_alpha"]
    assert (cfg["learning_rate"], cfg["reg_weight"], cfg["ssl_alpha"]) == ([0.001], [0.5], [0.01])
    g = dh.load_fixture(GOLDEN, "small")
    args = parse_args(["--Model", "DualVAE", "--data_path", "sports"])
    args.reg_weight, args.ssl_alpha = 0.5, 0.01
    m = cli.build_model(args, g["U"], g["I"], g["edges"], dh.user_item_dict(g["edges"]), None, None, torch.device("cpu"))
    assert type(m).__name__ == "DualVAE" and (m.kl_weight, m.ssl_reg) == (0.5, 0.01) and not hasattr(m, "pre_epoch_processing")


def test_ops_raise_on_cpu_tensors():
    from chaorec_amd import _lib, ops
    _lib.build()
    g = dh.load_fixture(GOLDEN, "small")
    m = make_model(g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.loss(torch.from_numpy(g["users"]), torch.from_numpy(g["pos"]), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.gene_ranklist()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.encode_user(torch.zeros(2, g["I"]))
    s, w = m.user_structure, torch.zeros(g["I"], 5)
    batch = s.batch(torch.from_numpy(g["users"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dualvae_encode(m.user_encoder.fc0.weight.t(), m.user_encoder.fc0.bias, w, s, batch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dualvae_dense(torch.zeros(200, 5, 25), torch.zeros(200, 5, 20), torch.zeros(g["I"], 5, 20), w, m.beta, s, batch)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dualvae_writeback(batch, g["U"], torch.zeros(200, 5, 25), torch.zeros(200, 5, 25), m.theta, m.mu_theta)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.dualvae_scores(m.mu_theta, torch.zeros(g["U"], 5, 20), m.mu_beta, torch.zeros(g["I"], 5, 20), w, 0, m.hist, 1e-6)
    with pytest.raises(ValueError, match="k=25, a=5, hidden=20"):
        ops.dualvae_check_shape(64)


def test_abi_is_additive_and_every_status_is_checked():
    from chaorec_amd import _lib
    new = sorted(n for n in _lib.SIGNATURES if n.startswith("chaorec_dualvae_"))
    assert new == ["chaorec_dualvae_check_shape", "chaorec_dualvae_dense_bwd_f32", "chaorec_dualvae_dense_fwd_f32",
                   "chaorec_dualvae_encode_bwd_f32", "chaorec_dualvae_encode_fwd_f32", "chaorec_dualvae_linear_bwd_f32",
                   "chaorec_dualvae_linear_bwd_workspace_bytes", "chaorec_dualvae_loss_f32", "chaorec_dualvae_scores_f32",
                   "chaorec_dualvae_splits", "chaorec_dualvae_tick", "chaorec_dualvae_writeback_f32"]
    assert _lib.ABI_VERSION == 16 and not any(n in _lib.INT_VALUE_EXPORTS for n in new)
    assert [n for n in new if _lib.SIGNATURES[n][0] is not ctypes.c_int] == ["chaorec_dualvae_linear_bwd_workspace_bytes",
                                                                                        "chaorec_dualvae_splits"]
    assert len([n for n in _lib.SIGNATURES if n.startswith("chaorec_macrid_")]) == 12          # the siblings' exports are untouched
    assert len([n for n in _lib.SIGNATURES if n.startswith("chaorec_multvae_")]) == 7
    _lib.build()
    lib = _lib.load()
    assert 1 <= lib.chaorec_dualvae_splits(2048, 28940) <= 64
    assert lib.chaorec_dualvae_check_shape(25, 5, 20) == 0
    with pytest.raises(RuntimeError, match=r"^chaorec_dualvae_tick failed \(-1\): dualvae_tick: NULL argument"):
        lib.chaorec_dualvae_tick(None, None)
    with pytest.raises(RuntimeError, match=r"the kernels tile k=25 a=5 hidden=20"):
        lib.chaorec_dualvae_check_shape(64, 5, 20)


def test_kernels_compile_for_gfx950_without_scratch():
    """Read from the compiler's metadata; no instruction text is inspected."""
    kernels, m = kernel_meta.kernel_metadata(kernel_meta.compile_asm("dualvae.hip"))
    scratch, spills = m["scratch"], m["spills"]
    assert len(kernels) == 16 and len(scratch) == len(kernels) == len(spills)
    assert not any(scratch) and not any(spills)
