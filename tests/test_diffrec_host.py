"""DiffRec on the host: the float64 restatement (tests/diffrec_host.py) and the plain model (CPU) against every array the
reference's own run left in tests/golden/diffrec_small.npz, the collapse of the sampling chain against the literal chain, the
loss history against the reference's loop, and the wiring.  No kernel runs here.

Tolerance (accept.within): bound = 4 x max(own, ULP) relative to the largest magnitude of the float64 array, `own` the stored deviation of the
reference's fp32 run from the float64 restatement.  Every check prints deviation, own, bound and ratio."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import diffrec_host as dh  # noqa: E402
import kernel_meta  # noqa: E402
from conftest import GOLDEN, tie_aware_rank_equal  # noqa: E402

from chaorec_amd import _lib, ops  # noqa: E402
from chaorec_amd.Model.DiffRec import DiffRec  # noqa: E402


def within(what, got, ref, own, scale=None):
    accept.within(what, got, ref, own, dh.ULP, scale=scale, zero_ref=dh.ZERO_REF)


@functools.lru_cache(maxsize=None)
def case():
    g = dh.load_fixture(GOLDEN)
    return g, g["edges"].astype(np.int64)


@functools.lru_cache(maxsize=None)
def model():
    return dh.load_weights(dh.new_model(), case()[0]).eval()


def test_the_case_names_and_replayed_draws():
    g, edges = case()
    assert np.array_equal(edges, dh.small_case()) and dh.U - 1 not in dh.user_item_dict(edges)
    assert tuple(g["names"].tolist()) == dh.NAMES
    torch.manual_seed(dh.SEED)
    m = dh.new_model()
    sd = m.state_dict()
    assert tuple(sd) == dh.NAMES                                                         # Lt_history / Lt_count are no buffers, as there
    for k, n in enumerate(dh.NAMES):                                                     # the same torch seed -> the reference's weights
        assert float(sd[n].double().sum()) == g["w_sum_seeded"][k], n
    assert sd["dnn.in_layers.0.weight"].shape == (dh.HID, dh.I + 10) and sd["dnn.out_layers.0.weight"].shape == (dh.I, dh.HID)
    assert np.array_equal(m.batch_rows(torch.arange(dh.U)).numpy(), dh.dense_rows(edges))
    from chaorec_amd.Model.DiffMM import Denoise
    assert type(m.dnn) is Denoise and m.fused is False and m.collapsed is True
    assert DiffRec(dh.U, dh.I, dh.user_item_dict(edges), 0.1, 0.0005, 0.005, 5, [68], 0.001, "cpu").hidden_width == 68     # a list works too


def test_tables_and_the_weight():
    g, _ = case()
    m, s = model(), dh.schedule64()
    assert m.betas.dtype == torch.float64 and float(m.betas[0]) == 1e-5                  # not DiffMM's 1e-4
    for k, attr in (("betas", "betas"), ("ac", "alphas_cumprod"), ("coef1", "posterior_mean_coef1"), ("coef2", "posterior_mean_coef2")):
        t = getattr(m, attr)
        assert t.dtype == torch.float64 and np.allclose(t.numpy(), g["tab_" + k], rtol=2.0 ** -48, atol=0), k
        assert np.allclose(s[k], g["tab_" + k], rtol=2.0 ** -48, atol=0), k
    ts = torch.from_numpy(g["ts"])
    w = m.weight(ts)
    assert w.dtype == torch.float64 and np.allclose(w.numpy(), dh.snr_weight(g["ts"]), rtol=1e-12, atol=0)
    assert (w[ts == 0] == 1.0).all() and float(m.SNR(ts - 1)[0]) == float(m.SNR(torch.tensor([dh.STEPS - 1]))[0])    # index -1 is read
    c1, c2, a, beta = m.posterior_coefs()
    assert c2[0] == 0.0 and c1[0] == 1.0 and beta == 0.0 and a[0] == 1.0 and not any(a[1:])
    with pytest.raises(NotImplementedError):
        DiffRec(dh.U, dh.I, {}, 0.0, 0.0005, 0.005, 5, "[8]", 0.001, "cpu")


def test_the_shared_lines_are_cf_diffs():
    from chaorec_amd.Model.CF_Diff import CF_Diff
    for name in ("weight", "reweight_loss", "importance_pt", "sample_timesteps", "update_Lt_history", "SNR"):
        assert getattr(DiffRec, name) is getattr(CF_Diff, name), name


def test_restatement_reproduces_the_golden():
    g, edges = case()
    x0 = dh.dense_rows(edges)
    r64 = dh.training_step(dh.weights_of(g), x0, g["ts"], g["noise"], g["keep"])
    assert r64["loss"] == float(g["loss64"]) or dh.rel_dev(r64["loss"], g["loss64"]) < 1e-13
    assert dh.rel_dev(r64["reloss"], g["reloss64"]) < 1e-13
    within("the reference's fp32 reloss", g["reloss32"], r64["reloss"], g["own_reloss"])
    for n in dh.NAMES:
        assert dh.rel_dev(r64["grads"][n], g["grad64_" + n]) < 1e-12, n
        assert float(g["own_grad_" + n]) < 1e-5
    ps64 = dh.p_sample(dh.weights_of(g), x0).numpy()
    assert dh.rel_dev(ps64, g["sample64"]) < 1e-13
    assert dh.rel_dev(g["sample32"], ps64) == pytest.approx(float(g["own_sample"]), rel=1e-6) and float(g["own_sample"]) < 1e-4


def test_collapse_is_the_literal_chain_in_float64():
    g, edges = case()
    x0 = dh.dense_rows(edges)
    col, beta = dh.p_sample_collapsed(dh.weights_of(g), x0)
    assert beta == 0.0 and dh.rel_dev(col.numpy(), g["sample64"]) < 1e-12
    # with tables whose c2[0] is not 0 the general a_t, beta form still holds, beta x_start included
    s = dh.schedule64()
    s["coef2"] = s["coef2"].copy()
    s["coef2"][0] = 0.25
    lit = dh.p_sample(dh.weights_of(g), x0, s).numpy()
    col, beta = dh.p_sample_collapsed(dh.weights_of(g), x0, s)
    assert beta != 0.0 and dh.rel_dev(col.numpy(), lit) < 1e-12
    m = dh.load_weights(dh.new_model(), g).eval()
    m.posterior_mean_coef2 = m.posterior_mean_coef2.clone()
    m.posterior_mean_coef2[0] = 0.25
    with torch.no_grad():
        a, b = m.p_sample(torch.from_numpy(x0)), m.p_sample_literal(torch.from_numpy(x0))
    assert m.posterior_coefs()[3] == beta
    within("model, collapsed, c2[0] = 0.25", a.numpy(), lit, g["own_sample"])
    within("model, literal, c2[0] = 0.25", b.numpy(), lit, g["own_sample"])


def test_plain_training_step_against_float64():
    g, edges = case()
    m = dh.load_weights(dh.new_model(), g).train()
    m.zero_grad()
    loss = m.diffusion_step(torch.arange(dh.U), ts=torch.from_numpy(g["ts"]), noise=torch.from_numpy(g["noise"]), keep=torch.from_numpy(g["keep"]))
    loss.backward()
    assert m.last["reloss"].dtype == torch.float64
    within("loss", float(loss), g["loss64"], g["own_loss"])
    within("reloss", m.last["reloss"].numpy(), g["reloss64"], g["own_reloss"])
    for n, p in m.named_parameters():
        within("grad " + n, p.grad.numpy(), g["grad64_" + n], g["own_grad_" + n])
    assert np.array_equal(m.Lt_count.numpy(), np.bincount(g["ts"], minlength=dh.STEPS))


def test_history_update_is_the_reference_loop():
    g, _ = case()
    m = dh.new_model()
    for tb, lb in dh.lt_sequence():
        m.update_Lt_history(torch.from_numpy(tb), torch.from_numpy(lb))
    assert np.array_equal(m.Lt_count.numpy(), g["Lt_count"]) and np.array_equal(m.Lt_history.numpy(), g["Lt_history"])
    pt_all = m.importance_pt()
    assert np.allclose(pt_all.numpy(), g["pt_all"], rtol=1e-14, atol=0)
    torch.manual_seed(0)
    t, pt = m.sample_timesteps(512, "cpu", "importance")
    assert np.allclose(pt.numpy(), g["pt_all"][t.numpy()] * dh.STEPS) and not bool((pt == 1).all())


@pytest.mark.parametrize("collapsed", [True, False])
def test_p_sample_and_the_ranking(collapsed):
    g, edges = case()
    m = dh.load_weights(dh.new_model(collapsed=collapsed), g).eval()
    assert m.collapse_route("cpu") is collapsed
    x0 = torch.from_numpy(dh.dense_rows(edges))
    with torch.no_grad():
        x = m.p_sample(x0)
    within(f"p_sample collapsed={collapsed} against float64", x.numpy(), g["sample64"], g["own_sample"])
    rank = m.gene_ranklist(dh.TOPK)
    assert rank.shape == (dh.U, dh.TOPK) and rank.dtype == torch.int64 and int(rank.min()) >= dh.U and m.training is False
    i64, v64 = dh.top_lists(dh.masked(g["sample64"], edges))
    val = np.take_along_axis(dh.masked(x.numpy(), edges), rank.numpy() - dh.U, 1)
    atol = accept.bound_of(g["own_sample"], dh.ULP) * np.abs(g["sample64"]).max()
    ok, why = tie_aware_rank_equal(rank.numpy() - dh.U, val, i64, v64, atol=atol)
    assert ok, why
    ref_idx = g["rank"].astype(np.int64)
    ok, why = tie_aware_rank_equal(ref_idx - dh.U, np.take_along_axis(dh.masked(g["sample32"], edges), ref_idx - dh.U, 1), i64, v64, atol=atol)
    assert ok, why
    assert np.isfinite(val).all() and len(set(rank[dh.U - 1].tolist())) == dh.TOPK       # no history item listed; the empty user ranked
    assert m.full_sort_predict.__func__ is m.gene_ranklist.__func__


def test_routes_fall_back_as_documented():
    _, edges = case()
    uid = dh.user_item_dict(edges)
    args = (dh.U, dh.I, uid, dh.NOISE_SCALE, dh.NOISE_MIN, dh.NOISE_MAX, dh.STEPS)
    two = DiffRec(*args, "[8, 12]", 0.001, "cpu")
    assert not two.collapsed and not two.collapse_route("cuda") and len(two.dnn.in_layers) == 2
    assert two.gene_ranklist(3).shape == (dh.U, 3)
    odd = DiffRec(*args, "[6]", 0.001, "cpu")
    assert odd.collapse_route("cpu") and not odd.collapse_route("cuda")                 # H = 6: no multiple of 4 for the SpMM and the tile
    wide = DiffRec(*args, "[1028]", 0.001, "cpu")
    assert not wide.collapse_route("cuda")
    m = dh.new_model()
    m.sampling_noise = True
    assert not m.collapse_route("cpu")
    with pytest.raises(NotImplementedError):
        m.p_sample(torch.zeros(2, dh.I))


def test_exports_sources_and_the_deferred_registry_row():
    new = sorted(n for n in _lib.SIGNATURES if n.startswith("chaorec_diffrec_"))
    assert new == ["chaorec_diffrec_chain_f32", "chaorec_diffrec_check_shape", "chaorec_diffrec_out_loss_f32", "chaorec_diffrec_tiles"]
    assert _lib.ABI_VERSION == 16 and not any(n in _lib.INT_VALUE_EXPORTS for n in new)
    assert _lib.SOURCES.index("diffrec.hip") < _lib.SOURCES.index("bspm.hip") and _lib.SOURCES[-1] == "adagcl.hip"
    with open(os.path.join(kernel_meta.ROOT, "include", "chaorec_hip.h")) as f:
        header = f.read()
    assert all(f"int {n}(" in header for n in new)
    from chaorec_amd import epochs, ops_diffrec, ops_extra, registry
    for name in ops_diffrec.__all__:
        assert getattr(ops, name) is getattr(ops_diffrec, name) and getattr(ops_extra, name) is getattr(ops_diffrec, name)
    assert callable(epochs._train_epoch_diffrec)
    assert "DiffRec" not in registry.MODELS and len(registry.MODELS) == 51             # the row is deferred
    _lib.build()
    lib = _lib.load()
    assert ops.diffrec_tiles() == (128, 128, 16)
    ops.diffrec_check_shape(1, 1, 4)
    ops.diffrec_check_shape(1024, 15207, 1000)
    for B, I, H in ((4, 8, 6), (0, 8, 8), (4, 0, 8), (4, 8, 0), (4, 1 << 31, 8)):
        with pytest.raises(RuntimeError, match=r"^chaorec_diffrec_check_shape failed \(-1\): diffrec: "):
            ops.diffrec_check_shape(B, I, H)
    with pytest.raises(RuntimeError, match="NULL argument"):
        lib.chaorec_diffrec_out_loss_f32(None, 8, None, 8, *([None] * 5), 4, 8, 8, None, 8, None, None, None, None)
    with pytest.raises(RuntimeError, match="NULL argument"):
        lib.chaorec_diffrec_chain_f32(None, 8, None, 8, None, None, 8, None, 1.0, 0.0, 4, 8, 8, None, None, 8, None)
    with pytest.raises(RuntimeError, match="MI355X only"):
        ops.diffrec_chain_step(*(torch.zeros(s) for s in ((2, 4), (3, 4), (3,), (2, 3), (3,))), 1.0, 0.0)


def test_plain_twins_are_the_restatements():
    rng = np.random.default_rng(4)
    B, N, K = 5, 7, 12
    z, G, g0, p, e = (rng.standard_normal(s) for s in ((B, K), (N, K), (N,), (B, N), (N,)))
    ref = dh.chain_step(z, G, g0, p, e, 0.75, 0.25, torch.float64)
    pn, zn = ops.diffrec_chain_step_plain(*(torch.from_numpy(a) for a in (z, G, g0, p, e)), 0.75, 0.25)
    assert np.allclose(pn.numpy(), ref["p_next"], rtol=1e-14) and np.allclose(zn.numpy(), ref["z_next"], rtol=1e-14)
    x0 = (rng.random((B, N)) < 0.3).astype(np.float64)
    wt, pt = rng.uniform(0.5, 2.0, B), rng.uniform(0.2, 3.0, B)
    W, b = rng.standard_normal((N, K)), rng.standard_normal(N)
    ref = dh.loss_node(z, W, b, x0, wt, pt, torch.float64)
    loss, reloss = ops.diffrec_x0_loss_plain(*(torch.from_numpy(a) for a in (z, W, b, x0, wt, pt)))
    assert np.allclose(float(loss), ref["loss"], rtol=1e-14) and np.allclose(reloss.numpy(), ref["reloss_rows"], rtol=1e-14)
    # the closed form the fused node rests on: d loss / d out = 2 w_b / (pt_b B I) err
    err = (z @ W.T + b) - x0
    assert np.allclose((2.0 * wt / (pt * B * N))[:, None] * err, ref["d_out"], rtol=1e-12, atol=1e-15)


def test_kernels_compile_for_gfx950_without_scratch():
    """Read from the compiler's metadata; no instruction text is inspected."""
    kernels, m = kernel_meta.kernel_metadata(kernel_meta.compile_asm("diffrec.hip"))
    scratch, spills, sspills, lds = m["scratch"], m["spills"], m["sspills"], m["lds"]
    print(dict(kernels=kernels, **m))
    assert len(kernels) == 3 and len(scratch) == len(kernels) == len(spills) == len(sspills) == len(lds)
    assert not any(scratch) and not any(spills) and not any(sspills)
    assert max(lds) == 2 * 2 * 16 * (128 + 4) * 4 + 2 * 128 * 4          # both operands double-buffered, the row partials
