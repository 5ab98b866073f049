"""MultVAE host logic (no GPU): the float64 restatement (tests/multvae_host.py) against the REFERENCE goldens of
tests/golden/gen_multvae.py, the model surface (names, shapes, bit-equal initial values, CLI, YAML), the C ABI and the
compiled kernels' resources.

Bounds: every reference quantity is stored with its own fp32-vs-fp64 deviation (the restatement is the fp64 twin by
construction); a check allows 4 x that.  The reference's summation order is torch's, unknown and thread-count dependent,
so its own rounding noise is the floor; a formula error (a wrong anneal, a missing 1 / B, reg_weight instead of its
square) shows at 1e-3 and up, two orders of magnitude outside."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import kernel_meta  # noqa: E402
import multvae_host as mh  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("layers_q.0.weight", "layers_q.0.bias", "layers_p.0.weight", "layers_p.0.bias")


def within(x, ref, dev, what):
    accept.within(what, x, ref, dev, 0.0)


def make_model(g, device="cpu"):
    from chaorec_amd.Model import MultVAE
    torch.manual_seed(int(g["seed"]))
    return MultVAE(g["U"], g["I"], g["edges"], mh.user_item_dict(g["edges"]), 64, float(g["reg_weight"]), torch.device(device))


def test_restatement_meets_reference_small():
    g = mh.load_fixture(GOLDEN, "small")
    w = (g["Wq"], g["bq"], g["Wp"], g["bp"])
    for tag, uc in (("", 0), ("a_", 123456)):
        out = mh.step(w, g["rowptr"], g["col"], g["users"], g["keep"], g["eps"], uc, float(g["reg_weight"]))
        for k in ("loss", "neg_ll", "kl"):
            within(g[f"{tag}ref_{k}"], out[k], g[f"{tag}dev_{k}"], f"{tag}{k}")
        assert out["anneal"] == min(0.2, uc / 200000)
        if tag:
            for n, ref, got, dev in zip(NAMES, (g["ref_dWq"], g["ref_dbq"], g["ref_dWp"], g["ref_dbp"]), out["grads"], g["a_dev_grads"]):
                within(ref, got, dev, f"grad {n}")
            # an item no sample touched: its decoder gradient is P^T z + 2 reg^2 w alone, its encoder gradient 2 reg^2 w
            i = int(g["untouched_item"])
            np.testing.assert_allclose(out["grads"][0][:, i], 2 * float(g["reg_weight"]) ** 2 * g["Wq"][:, i].astype(np.float64), rtol=1e-12)
        else:
            within(g["ref_lse"], out["lse"], g["dev_lse"], "lse")
            within(g["ref_z"], out["z"], g["dev_z"], "z")
    # the sample whose whole row was dropped encodes to the bias alone
    b = int(g["dropped_sample"])
    mu = out["z"][b] - g["eps"][b].astype(np.float64) * np.exp(0.5 * g["bq"][64:].astype(np.float64))
    np.testing.assert_allclose(mu, g["bq"][:64].astype(np.float64), rtol=1e-12)


def test_restatement_trajectory_small():
    """Ten Adam steps from update_count 39 995: anneal reaches its cap at 40 000 inside the run."""
    g = mh.load_fixture(GOLDEN, "small")
    w = (g["Wq"], g["bq"], g["Wp"], g["bp"])
    uc0 = int(g["traj_update_count"])
    assert mh.anneal_of(uc0) < 0.2 and mh.anneal_of(uc0 + 9) == 0.2
    losses, wT = mh.adam_trajectory(w, g["rowptr"], g["col"], list(g["traj_batches"]), g["traj_keeps"], list(g["traj_eps"]), uc0,
                                    float(g["reg_weight"]), float(g["traj_lr"]))
    within(g["traj_ref_losses"], losses, g["traj_dev_losses"], "trajectory losses")
    for n, ref, got, dev in zip(NAMES, (g["traj_ref_Wq"], g["traj_ref_bq"], g["traj_ref_Wp"], g["traj_ref_bp"]), wT, g["traj_dev_weights"]):
        within(ref, got, dev, f"trajectory {n}")


def test_restatement_meets_reference_sports():
    g = mh.load_fixture(GOLDEN, "sports")
    m = make_model(g)
    w = tuple(p.detach().numpy() for p in (m.layers_q[0].weight, m.layers_q[0].bias, m.layers_p[0].weight, m.layers_p[0].bias))
    mask, eps = mh.replay_draws(g["draw_seed"], len(g["users"]), g["I"])
    assert abs(float(eps.astype(np.float64).sum()) - float(g["eps_sum"])) < 1e-9, "this torch draws another eps than the generator's"
    assert np.array_equal(mh.flags_from_mask(mask, g["rowptr"], g["col"], g["users"]), g["keep"])
    out = mh.step(w, g["rowptr"], g["col"], g["users"], g["keep"], eps, 123456, float(g["reg_weight"]))
    for k in ("loss", "neg_ll", "kl"):
        within(g[f"a_ref_{k}"], out[k], g[f"a_dev_{k}"], f"sports {k}")
    within(g["ref_lse"], out["lse"], g["dev_lse"], "sports lse")
    rows, dev = g["grad_rows"], g["a_dev_grads"]
    scale = [float(np.abs(x).max()) for x in out["grads"]]
    for what, ref, got, d, s in (("dWq rows", g["ref_dWq_rows"], out["grads"][0][:, rows].T, dev[0], scale[0]),
                                ("dbq", g["ref_dbq"], out["grads"][1], dev[1], scale[1]),
                                ("dWp rows", g["ref_dWp_rows"], out["grads"][2][rows], dev[2], scale[2]),
                                ("dbp rows", g["ref_dbp_rows"], out["grads"][3][rows], dev[3], scale[3])):
        got_dev = float(np.abs(np.asarray(ref, dtype=np.float64) - got).max()) / s      # (relative to the WHOLE gradient's largest element)
        print(f"sports {what}: {got_dev:.3e} (bound {4 * d:.3e})")
        assert got_dev <= 4 * d
    for n, ref, got in zip(NAMES, g["a_ref_gnorm"], out["grads"]):
        assert abs(float(np.linalg.norm(got)) - ref) <= 1e-4 * ref, n


@pytest.mark.parametrize("name", ["small", "sports"])
def test_parameters_equal_the_references_for_the_same_seed(name):
    """Same init calls in the same order: names, shapes and VALUES (bit for bit) of the reference's state_dict."""
    g = mh.load_fixture(GOLDEN, name)
    m = make_model(g)
    sd = m.state_dict()
    assert tuple(sd.keys()) == NAMES
    I = g["I"]
    assert [tuple(v.shape) for v in sd.values()] == [(128, I), (128,), (I, 64), (I,)]
    assert [n for n, _ in m.named_parameters()] == list(NAMES)
    w = [v.detach().cpu().numpy() for v in sd.values()]
    assert m.layers_q[0].weight.stride() == (1, 128)          # the row-major [I, 128] buffer, transposed
    for k, x in enumerate(w):
        assert float(x.astype(np.float64).sum()) == float(g["w_sum"][k])
        assert np.array_equal(x.reshape(-1)[:64], g["w_probe"][k])
    if name == "small":
        for x, ref in zip(w, (g["Wq"], g["bq"], g["Wp"], g["bp"])):
            assert np.array_equal(x, ref)
    assert m.update_count == 0.0 and m.keep_prob == 0.5 and m.anneal_cap == 0.2 and m.total_anneal_steps == 200000
    m.update_count = 39995
    assert m.update_count == 39995.0 and [t.shape for t in m.capture_state_tensors()] == [(2,), (1,)]


def test_generator_refused_no_fixture_outside_the_ranking_cap():
    for name in ("small", "sports"):
        g = mh.load_fixture(GOLDEN, name)
        assert float(g["rank_ref_share"]) <= 0.02
    # ... and the stored list meets the cap against the restatement's scores
    g = mh.load_fixture(GOLDEN, "small")
    w = (g["Wq"], g["bq"], g["Wp"], g["bp"])
    z = mh.latent_all(w, g["rowptr"], g["col"], g["U"], g["eps_rank"])
    share, bad = mh.ranklist_check(g["ranks"], w, z, g["rowptr"], g["col"], int(g["topk"]))
    assert share <= 0.02 and bad == 0


def test_cli_and_yaml():
    from chaorec_amd import main as cli
    from chaorec_amd.arg_parser import load_yaml_config, parse_args
    cfg = load_yaml_config("MultVAE")
    assert cfg["hyper_parameters"] == ["reg_weight", "learning_rate"] and cfg["reg_weight"] == [0.01, 0.001]
    g = mh.load_fixture(GOLDEN, "small")
    args = parse_args(["--Model", "MultVAE", "--data_path", "sports"])
    args.reg_weight = 0.01
    m = cli.build_model(args, g["U"], g["I"], g["edges"], mh.user_item_dict(g["edges"]), None, None, torch.device("cpu"))
    assert type(m).__name__ == "MultVAE" and not hasattr(m, "pre_epoch_processing")


def test_ops_raise_on_cpu_tensors():
    from chaorec_amd import _lib
    _lib.build()
    g = mh.load_fixture(GOLDEN, "small")
    m = make_model(g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.loss(torch.from_numpy(g["users"]))


def test_abi_is_additive_and_every_status_is_checked():
    from chaorec_amd import _lib
    import ctypes
    new = sorted(n for n in _lib.SIGNATURES if n.startswith("chaorec_multvae_"))
    assert new == ["chaorec_multvae_decode_bwd_f32", "chaorec_multvae_decode_fwd_f32", "chaorec_multvae_decode_splits",
                   "chaorec_multvae_encode_bwd_f32", "chaorec_multvae_encode_fwd_f32", "chaorec_multvae_sumsq_f32",
                   "chaorec_multvae_tick"]
    assert _lib.ABI_VERSION == 16 and not any(n in _lib.INT_VALUE_EXPORTS for n in new)
    assert [n for n in new if _lib.SIGNATURES[n][0] is not ctypes.c_int] == ["chaorec_multvae_decode_splits"]
    assert _lib.SIGNATURES["chaorec_multvae_decode_splits"][0] is ctypes.c_int64
    _lib.build()
    lib = _lib.load()
    assert lib.chaorec_multvae_decode_splits(2048, 15207) >= 16
    assert lib.chaorec_multvae_decode_splits(2048, 262144) <= 64
    with pytest.raises(RuntimeError, match=r"^chaorec_multvae_tick failed \(-1\): multvae_tick: NULL argument"):
        lib.chaorec_multvae_tick(None, None, 0.2, 200000, None)


def test_kernels_compile_for_gfx950_without_scratch():
    text = kernel_meta.compile_asm("multvae.hip")
    kernels, m = kernel_meta.kernel_metadata(text)
    scratch, spills = m["scratch"], m["spills"]
    assert len(kernels) >= 12 and len(scratch) == len(kernels)
    assert not any(scratch) and not any(spills)
    assert "v_mfma_f32_32x32x2_f32" in text or "v_mfma_f32_32x32x2f32" in text
    assert "atomic" not in text.split(".amdgpu_metadata")[0].lower()
