"""MacridVAE host logic (no GPU): the float64 restatement (tests/macridvae_host.py) against the REFERENCE goldens of
tests/golden/gen_macridvae.py, the model surface (names, shapes, bit-equal initial values, CLI, YAML), the C ABI and the
compiled kernels' resources.

Bounds: every reference quantity is stored with its own fp32-vs-fp64 deviation; a check allows 4 x that (the reference's
own rounding noise is the floor; a formula error -- the anneal read before the increment, a mu^2 term in the KL, the
dropped row in the likelihood -- shows at 1e-3 and up)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import kernel_meta  # noqa: E402
import macridvae_host as mh  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def within(x, ref, dev, what):
    accept.within(what, x, ref, dev, 0.0)


def make_model(g, device="cpu"):
    from chaorec_amd.Model import MacridVAE
    torch.manual_seed(int(g["seed"]))
    return MacridVAE(g["U"], g["I"], g["edges"], mh.user_item_dict(g["edges"]), g["D"], 0.0, torch.device(device))


def host_weights(m):
    return tuple(np.ascontiguousarray(v.detach().cpu().numpy()) for v in m.state_dict().values())      # (C order: the sums below add in it)


@pytest.mark.parametrize("name", ["small", "sports"])
def test_parameters_equal_the_references_for_the_same_seed(name):
    g = mh.load_fixture(GOLDEN, name)
    m = make_model(g)
    sd = m.state_dict()
    I, D = g["I"], g["D"]
    assert tuple(sd.keys()) == mh.NAMES and [n for n, _ in m.named_parameters()] == list(mh.NAMES)
    assert [tuple(v.shape) for v in sd.values()] == [(600, I), (600,), (2 * D, 600), (2 * D,), (I, D), (10, D)]
    assert m.encoder[0].weight.stride() == (1, 600)          # the row-major [I, 600] buffer, transposed
    for k, x in enumerate(host_weights(m)):
        assert float(x.astype(np.float64).sum()) == float(g["w_sum"][k]), mh.NAMES[k]
        assert np.array_equal(x.reshape(-1)[:64], g["w_probe"][k]), mh.NAMES[k]
    assert (m.kfac, m.layers, m.tau, m.std, m.drop_out, m.anneal_cap, m.total_anneal_steps, m.regs, m.nogb) == \
        (10, [600], 0.1, 0.01, 0.5, 0.2, 200000, [0.0, 0.0], False)
    assert m.update == 0
    m.update = 39994
    assert m.update == 39994 and [t.shape for t in m.capture_state_tensors()] == [(2,), (1,)]
    assert m.full_sort_predict.__func__ is m.gene_ranklist.__func__ and float(m.reg_loss().detach()) == 0.0
    m.eval()
    assert m.reparameterize(torch.ones(2, 3), torch.zeros(2, 3)).equal(torch.ones(2, 3))


def test_a_width_the_kernels_do_not_tile_is_refused():
    g = mh.load_fixture(GOLDEN, "small")
    from chaorec_amd.Model import MacridVAE
    with pytest.raises(ValueError, match="dim_E=32"):
        MacridVAE(g["U"], g["I"], g["edges"], mh.user_item_dict(g["edges"]), 32, 0.0, torch.device("cpu"))


@pytest.mark.parametrize("name", ["small", "sports"])
def test_restatement_meets_reference(name):
    g = mh.load_fixture(GOLDEN, name)
    w = host_weights(make_model(g))
    keep, gumbel, eps = mh.case_draws(g, int(g["draw_seed"]), g["users"])
    assert mh.draws_match((keep, gumbel, eps), g["draw_sums"]), "this torch draws other values than the generator's"
    for tag, upd in (("", 0), ("a_", 123456)):
        out = mh.step(w, g["rowptr"], g["col"], g["users"], keep, gumbel, eps, upd)
        assert out["anneal"] == min(0.2, (upd + 1) / 200000)          # incremented first
        for k in ("loss", "ce", "kl"):
            within(g[f"{tag}ref_{k}"], out[k], g[f"{tag}dev_{k}"], f"{name} {tag}{k}")
    within(g["ref_lse"], out["lse"], g["a_dev_lse"], f"{name} lse")
    rows, dev = g["grad_rows"], g["a_dev_grads"]
    scale = [float(np.abs(x).max()) for x in out["grads"]]
    for what, ref, got, d, s in (("dW1 rows", g["ref_dW1_rows"], out["grads"][0][:, rows].T, dev[0], scale[0]),
                                ("db1", g["ref_db1"], out["grads"][1], dev[1], scale[1]),
                                ("dE rows", g["ref_dE_rows"], out["grads"][4][rows], dev[4], scale[4]),
                                ("dK", g["ref_dK"], out["grads"][5], dev[5], scale[5]),
                                ("cates rows", g["ref_cates_rows"], out["cates"][rows], g["a_dev_cates"], float(out["cates"].max()))):
        got_dev = float(np.abs(np.asarray(ref, dtype=np.float64) - got).max()) / s      # (relative to the WHOLE array's largest element)
        print(f"{name} {what}: {got_dev:.3e} (bound {4 * d:.3e})")
        assert got_dev <= 4 * d
    for n, ref, got in zip(mh.NAMES, g["a_ref_gnorm"], out["grads"]):
        assert abs(float(np.linalg.norm(got)) - ref) <= 1e-4 * ref, n


def test_restatement_trajectory_small():
    """Ten Adam steps from update 39 994: the anneal, read after the increment, reaches its cap at the sixth step."""
    g = mh.load_fixture(GOLDEN, "small")
    w = host_weights(make_model(g))
    u0, T = int(g["traj_update"]), len(g["traj_batches"])
    assert mh.anneal_of(u0 + 1) < 0.2 and mh.anneal_of(u0 + T) == 0.2
    draws = [mh.case_draws(g, int(g["traj_seed0"]) + t, g["traj_batches"][t]) for t in range(T)]
    losses, wT = mh.adam_trajectory(w, g["rowptr"], g["col"], list(g["traj_batches"]), [d[0] for d in draws], [d[1] for d in draws],
                                    [d[2] for d in draws], u0, float(g["traj_lr"]))
    within(g["traj_ref_losses"], losses, g["traj_dev_losses"], "trajectory losses")
    for k, n in enumerate(mh.NAMES):
        got = float(np.abs(wT[k].reshape(-1)[:64] - g["traj_ref_probe"][k]).max()) / float(np.abs(wT[k]).max())
        assert got <= accept.bound_of(g["traj_dev_weights"][k], 0.0), n


def test_generator_refused_no_fixture_outside_the_ranking_cap():
    for name in ("small", "sports"):
        g = mh.load_fixture(GOLDEN, name)
        assert float(g["rank_ref_share"]) <= 0.02
    g = mh.load_fixture(GOLDEN, "small")
    w = host_weights(make_model(g))
    share, bad = mh.ranklist_check(g["ranks"], w, g["rowptr"], g["col"], g["rowptr"], g["col"], g["rank_users"], int(g["topk"]))
    assert share <= 0.02 and bad == 0


def test_cli_and_yaml():
    from chaorec_amd import main as cli
    from chaorec_amd.arg_parser import load_yaml_config, parse_args
    cfg = load_yaml_config("MacridVAE")
    assert cfg["hyper_parameters"] == ["learning_rate"] and cfg["learning_rate"] == [0.01]
    g = mh.load_fixture(GOLDEN, "small")
    args = parse_args(["--Model", "MacridVAE", "--data_path", "sports"])
    m = cli.build_model(args, g["U"], g["I"], g["edges"], mh.user_item_dict(g["edges"]), None, None, torch.device("cpu"))
    assert type(m).__name__ == "MacridVAE" and m.dim_E == 64 and not hasattr(m, "pre_epoch_processing")


def test_ops_raise_on_cpu_tensors():
    from chaorec_amd import _lib, ops
    _lib.build()
    g = mh.load_fixture(GOLDEN, "small")
    m = make_model(g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.loss(torch.from_numpy(g["users"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.gene_ranklist()
    assert m.training is False
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.macrid_topk(torch.zeros(4, 100), 50)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.macrid_scores(torch.zeros(4, 10, 64), torch.zeros(100, 64), torch.zeros(100, 10), 0.1, 0, m.hist, 1e-6)


def test_abi_is_additive_and_every_status_is_checked():
    from chaorec_amd import _lib
    new = sorted(n for n in _lib.SIGNATURES if n.startswith("chaorec_macrid_"))
    assert new == ["chaorec_macrid_check_shape", "chaorec_macrid_concept_bwd_f32", "chaorec_macrid_concept_fwd_f32",
                   "chaorec_macrid_encode_bwd_f32", "chaorec_macrid_encode_fwd_f32", "chaorec_macrid_mix_bwd_f32",
                   "chaorec_macrid_mix_fwd_f32", "chaorec_macrid_mix_splits", "chaorec_macrid_normal_f32",
                   "chaorec_macrid_scores_f32", "chaorec_macrid_tick", "chaorec_macrid_topk_f32"]
    assert _lib.ABI_VERSION == 16 and not any(n in _lib.INT_VALUE_EXPORTS for n in new)
    assert [n for n in new if _lib.SIGNATURES[n][0] is not ctypes.c_int] == ["chaorec_macrid_mix_splits"]
    assert len([n for n in _lib.SIGNATURES if n.startswith("chaorec_multvae_")]) == 7          # MultVAE's exports are untouched
    _lib.build()
    lib = _lib.load()
    assert 1 <= lib.chaorec_macrid_mix_splits(2048, 18357) <= 64
    assert lib.chaorec_macrid_check_shape(64, 10, 600) == 0
    with pytest.raises(RuntimeError, match=r"^chaorec_macrid_tick failed \(-1\): macrid_tick: NULL argument"):
        lib.chaorec_macrid_tick(None, None, 0.2, 200000, None)
    with pytest.raises(RuntimeError, match=r"the kernels tile D=64 K=10 H=600"):
        lib.chaorec_macrid_check_shape(32, 10, 600)


def test_kernels_compile_for_gfx950_without_scratch():
    text = kernel_meta.compile_asm("macridvae.hip")
    kernels, m = kernel_meta.kernel_metadata(text)
    scratch, spills = m["scratch"], m["spills"]
    assert len(kernels) >= 18 and len(scratch) == len(kernels)
    assert not any(scratch) and not any(spills)
    assert "v_mfma_f32_32x32x2_f32" in text or "v_mfma_f32_32x32x2f32" in text
    assert "atomic" not in text.split(".amdgpu_metadata")[0].lower()
