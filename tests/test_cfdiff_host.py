"""CF_Diff on the host: the plain model (fused = False, CPU) against every array the reference's own run left in
tests/golden/cfdiff_small.npz, the vectorised loss history against the reference's loop, the shape checks, the keep-bit keying
restated, and the backward identities of csrc/cfdiff.hip in float64 against autograd.

Tolerance (accept.within): bound = 4 x max(own, ULP) relative to the largest magnitude of the float64 array, `own` the deviation of an fp32
computation that is not the code under test (the reference's stored fp32 output; for the small random model the fp32 run of the
restatement) from the float64 restatement.  Every check prints deviation, own, bound and ratio."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import cfdiff_host as ch  # noqa: E402
from conftest import GOLDEN, tie_aware_rank_equal  # noqa: E402

from chaorec_amd import _lib, ops  # noqa: E402
from chaorec_amd.Model import CF_Diff  # noqa: E402


def within(what, got, ref, own, scale=None):
    return accept.within(what, got, ref, own, ch.ULP, scale=scale, zero_ref=ch.ZERO_REF)


@functools.lru_cache(maxsize=None)
def case():
    g = ch.load_fixture(GOLDEN)
    edges = g["edges"].astype(np.int64)
    return g, edges


def new_model(dim_inters=ch.DIM_INTERS, **kw):
    g, edges = case()
    return CF_Diff(ch.U, ch.I, ch.user_item_dict(edges), ch.NOISE_SCALE, ch.NOISE_MIN, ch.NOISE_MAX, ch.STEPS, 0.001, "cpu",
                   fused=False, seed=11, dim_inters=dim_inters, **kw)


@functools.lru_cache(maxsize=None)
def model():
    return ch.load_weights(new_model(), case()[0]).eval()


def test_the_case_and_the_sec_hop_values():
    g, edges = case()
    assert np.array_equal(edges, ch.small_case()) and ch.U - 1 not in ch.user_item_dict(edges)
    m = model()
    users = torch.arange(ch.U)
    assert np.array_equal(m.batch_rows(users).numpy(), ch.dense_rows(edges))
    assert np.array_equal(m.sec_hop_rows(users).numpy(), g["sec_hop"])                   # cnt / U on the history, fp32, exactly
    assert not g["sec_hop"][ch.U - 1].any() and not g["sec_hop"][:, ch.I - ch.EMPTY_ITEMS:].any()
    assert np.all(g["sec_hop"][:ch.U - 1, 0] == np.float32(ch.U - 1) / np.float32(ch.U))
    shuffled = torch.tensor([5, 11, 0, 5])
    assert np.array_equal(m.sec_hop_rows(shuffled).numpy(), g["sec_hop"][shuffled.numpy()])


def test_state_dict_holds_the_used_weights_only():
    names = sorted(model().CAM_AE.state_dict())
    assert names == sorted(ch.WEIGHTS) and len(names) == 24
    assert not any(n.startswith(("in_layers", "out_layers", "encoder2", "final_out", "norm1", "norm2")) for n in names)


def test_schedule_and_q_sample():
    g, _ = case()
    m, s = model(), ch.schedule64()
    assert m.betas.dtype == torch.float64 and float(m.betas[0]) == 1e-5
    assert np.allclose(m.alphas_cumprod.numpy(), s["ac"], rtol=1e-15, atol=0)
    assert np.allclose(m.posterior_mean_coef1.numpy(), s["coef1"], rtol=1e-13, atol=0)
    assert np.allclose(m.posterior_mean_coef2.numpy(), s["coef2"], rtol=1e-13, atol=0)
    x_t = m.q_sample(torch.from_numpy(ch.dense_rows(case()[1])), torch.from_numpy(g["ts"]), torch.from_numpy(g["noise"]))
    assert np.array_equal(x_t.numpy(), g["x_t"])
    w = m.weight(torch.from_numpy(g["ts"]))
    assert w.dtype == torch.float64 and np.allclose(w.numpy(), ch.snr_weight(g["ts"]), rtol=1e-12, atol=0)
    assert (w[torch.from_numpy(g["ts"]) == 0] == 1.0).all()                              # ts = 0 reads index -1 and discards it


def test_cam_ae_eval_against_the_golden():
    g, _ = case()
    m = model()
    users = torch.arange(ch.U)
    with torch.no_grad():
        out = m.CAM_AE(torch.from_numpy(g["x_t"]), m.sec_hop_rows(users), torch.from_numpy(g["ts"]))
    assert out.shape == (ch.U, ch.I) and out.dtype == torch.float32
    within("plain CAM_AE against float64", out.numpy(), g["out64"], g["own_out"])
    within("plain CAM_AE against the reference's fp32", out.numpy(), g["out32"].astype(np.float64), 2 * g["own_out"], np.abs(g["out64"]).max())
    x0 = torch.from_numpy(ch.dense_rows(case()[1]))
    reloss = m.reweight_loss(m.mean_flat((x0 - out) ** 2), torch.from_numpy(g["ts"]))
    assert reloss.dtype == torch.float64
    mse64 = ((ch.dense_rows(case()[1]).astype(np.float64) - g["out64"]) ** 2).mean(1)
    for b in range(ch.U):                                                                # per row: the weights span five decades
        within(f"reweight_loss row {b}", reloss.numpy()[b], ch.snr_weight(g["ts"])[b] * mse64[b], 2 * g["own_out"])
    assert np.allclose(reloss.numpy(), g["reloss"], rtol=8 * g["own_out"], atol=0)


def test_a_batch_of_one_keeps_its_batch_dimension():
    g, _ = case()
    m = model()
    with torch.no_grad():
        out = m.CAM_AE(torch.from_numpy(g["x_t"][3:4]), m.sec_hop_rows(torch.tensor([3])), torch.from_numpy(g["ts"][3:4]))
    assert out.shape == (1, ch.I)
    within("B = 1", out.numpy(), g["out64"][3:4], g["own_out"], np.abs(g["out64"]).max())


def test_history_update_is_the_reference_loop():
    g, _ = case()
    m = new_model(dim_inters=22)
    for tb, lb in ch.lt_sequence():
        m.update_Lt_history(torch.from_numpy(tb), torch.from_numpy(lb))
    assert m.Lt_history.dtype == torch.float64 and m.Lt_count.dtype == torch.int64
    assert np.array_equal(m.Lt_count.numpy(), g["Lt_count"]) and np.array_equal(m.Lt_history.numpy(), g["Lt_history"])
    pt_all = m.importance_pt()
    assert np.allclose(pt_all.numpy(), g["pt_all"], rtol=1e-14, atol=0) and abs(float(pt_all.sum()) - 1.0) < 1e-12
    torch.manual_seed(0)
    t, pt = m.sample_timesteps(4096, "cpu", "importance")
    assert np.allclose(pt.numpy(), g["pt_all"][t.numpy()] * ch.STEPS) and set(t.tolist()) == set(range(ch.STEPS))
    freq = np.bincount(t.numpy(), minlength=ch.STEPS) / 4096.0
    assert np.abs(freq - g["pt_all"]).max() < 6 * 0.5 / np.sqrt(4096)


def test_timesteps_are_uniform_until_every_row_is_full():
    m = new_model(dim_inters=22)
    m.Lt_count[:] = 10
    m.Lt_count[4] = 9
    m.Lt_history[:] = 1.0
    m.Lt_history[0] = 100.0
    t, pt = m.sample_timesteps(2000, "cpu", "importance")
    assert (pt == 1).all() and np.bincount(t.numpy(), minlength=ch.STEPS).max() < 300          # not row 0's importance


def test_shape_checks_raise_value_errors():
    top = ops.cfdiff_max_len()
    assert top == 65536 // 48 and top >= 1034
    ops.cfdiff_check_shape(1, 1)
    ops.cfdiff_check_shape(1024, 1034)
    ops.cfdiff_check_shape(2, top)
    for B, L in ((1, 0), (1, top + 1), (0, 5), (3, -1)):
        with pytest.raises(ValueError, match="cfdiff: "):
            ops.cfdiff_check_shape(B, L)
    lib = _lib.load()
    with pytest.raises(RuntimeError, match=r"^chaorec_cfdiff_check_shape failed \(-1\): cfdiff: L=%d" % (top + 1)):
        lib.chaorec_cfdiff_check_shape(1, top + 1)
    with pytest.raises(RuntimeError, match=r"cfdiff: L=0"):
        lib.chaorec_cfdiff_attn_fwd_f32(None, None, None, 1, 0, 0, None, 0, None, 0, 0, None, None, None)
    with pytest.raises(RuntimeError, match=r"NULL argument"):
        lib.chaorec_cfdiff_attn_bwd_f32(*([None] * 6), 1, 5, 0, None, 0, None, 0, 0, None, None, None, None, None)
    with pytest.raises(ValueError, match="must be \\[B, L, 16\\]"):
        ops.cfdiff_attention_raw(torch.zeros(2, 5, 8), torch.zeros(2, 5, 8), torch.zeros(2, 5, 8), False, 0, None, 0)


def test_exports_and_sources():
    new = ["chaorec_cfdiff_max_len", "chaorec_cfdiff_check_shape", "chaorec_cfdiff_attn_fwd_f32", "chaorec_cfdiff_attn_bwd_f32",
           "chaorec_cfdiff_attn_keep_u8", "chaorec_diffmm_rows_noised_f32"]
    assert all(n in _lib.SIGNATURES for n in new) and "cfdiff.hip" in _lib.SOURCES
    assert _lib.ABI_VERSION == 16 and not any(n in _lib.INT_VALUE_EXPORTS for n in new)
    assert len([n for n in _lib.SIGNATURES if n.startswith("chaorec_cfdiff_")]) == 5
    assert ops.cfdiff_attention is not None and ops.cfdiff_attention_plain is not None and ops.cfdiff_keep is not None
    from chaorec_amd import ops_extra
    assert ops_extra.cfdiff_attention is ops.cfdiff_attention


def test_keep_bit_keying_restated():
    assert ch.mix64(0) == 0xE220A8397B1DCDAF                                             # splitmix64's first output
    L = 70
    k = ch.keep_flags(2, L, seed=7, step=3, salt=1)
    assert k.shape == (2, 4, L, L) and set(np.unique(k)) == {0, 1}
    n = k.size
    assert abs(k.mean() - 0.5) < 6 * 0.5 / np.sqrt(n)
    assert np.array_equal(ch.keep_flags(1, L, 7, 3, 1, b0=1)[0], k[1])                    # a row's flags depend on its slot only
    assert not np.array_equal(k[0], k[1]) and not np.array_equal(k[0, 0], k[0, 1])
    for other in (ch.keep_flags(1, L, 7, 4, 1), ch.keep_flags(1, L, 7, 3, 0), ch.keep_flags(1, L, 8, 3, 1)):
        assert abs((other[0] != k[0]).mean() - 0.5) < 6 * 0.5 / np.sqrt(k[0].size)       # step, salt, seed each re-key
    # one draw per aligned word of 64 keys: keys 0 .. 63 are the bits of one word, key 64 starts the next
    key = ch.mix64((ch.mix64(7 ^ 1) + 3) & ch.M64)
    r = ch.mix64(key ^ ch.mix64((((0 * 4 + 2) << 32) ^ ((5 << 20) | 0)) & ch.M64))
    assert [int(x) for x in k[0, 2, 5, :64]] == [(r >> j) & 1 for j in range(64)]


@pytest.mark.parametrize("L", [1, 9])
def test_backward_identities_against_autograd(L):
    torch.manual_seed(L)
    B = 2
    q, k, v, go = (torch.randn(B, L, 16, dtype=torch.float64) for _ in range(4))
    keep = (torch.rand(B, 4, L, L) < 0.5).to(torch.uint8)
    keep[0, 1, 0] = 0                                                                    # a query with every key dropped
    keep[1, 2, L - 1] = 1
    for kp in (None, keep):
        qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
        out = ch.attention(qa, ka, va, kp)
        out.backward(go)
        o2, dq, dk, dv = ch.attention_backward(q, k, v, go, kp)
        for name, a, b in (("out", o2, out.detach()), ("dq", dq, qa.grad), ("dk", dk, ka.grad), ("dv", dv, va.grad)):
            d = float((a - b).abs().max())
            print(f"L={L} keep={'given' if kp is not None else 'none'} {name}: {d:.2e}")
            assert d < 1e-14
        if kp is not None:
            assert not o2[0, 0, 4:8].any() and torch.isfinite(dq).all()
        plain = ops.cfdiff_attention_plain(q, k, v, kp is not None, keep=kp)
        assert float((plain - o2).abs().max()) < 1e-14


def test_one_step_of_a_small_model_against_float64():
    """fused = False, L = 32: loss and every parameter gradient of one diffusion_step with given ts, noise and flags."""
    g, edges = case()
    torch.manual_seed(5)
    m = new_model(dim_inters=22).train()
    with torch.no_grad():
        for mha in m.CAM_AE.self_attentions:
            mha.in_proj_weight.mul_(4.0)
    L, B = 32, ch.U
    users = torch.arange(B)
    ts = torch.from_numpy(g["ts"])
    noise = torch.from_numpy(g["noise"])
    rng = torch.Generator().manual_seed(9)
    flags = lambda *shape, p=0.5: (torch.rand(shape, generator=rng) >= p).to(torch.uint8)
    keeps = dict(drop=flags(B, 22), attn=[flags(B, 4, L, L) for _ in range(2)], drop1=[flags(B, L, 16, p=0.8) for _ in range(2)],
                 drop2=[flags(B, L, 16) for _ in range(2)])
    keeps["attn"][0][2, 1, 7] = 0
    loss = m.diffusion_step(users, ts=ts, noise=noise, keeps=keeps)
    loss.backward()

    def restated(dtype):
        w = {n: p.detach().to(dtype).requires_grad_() for n, p in m.CAM_AE.state_dict(keep_vars=True).items()}
        out = ch.cam_ae(w, torch.from_numpy(g["x_t"]), torch.from_numpy(g["sec_hop"]), ts, keeps)
        mse = ((torch.from_numpy(ch.dense_rows(edges)).to(dtype) - out) ** 2).mean(1)
        val = (torch.from_numpy(ch.snr_weight(g["ts"])) * mse).mean()
        val.backward()
        return val.detach(), {n: t.grad for n, t in w.items()}

    l64, g64 = restated(torch.float64)
    l32, g32 = restated(torch.float32)
    within("loss", loss.detach().numpy(), l64.numpy(), ch.rel_dev(l32.numpy(), l64.numpy()))
    for n, p in m.CAM_AE.named_parameters():
        within(f"grad {n}", p.grad.numpy(), g64[n].numpy(), ch.rel_dev(g32[n].numpy(), g64[n].numpy()))
    assert np.array_equal(m.Lt_count.numpy(), np.bincount(g["ts"], minlength=ch.STEPS))


def test_p_sample_and_the_ranking():
    g, edges = case()
    m = model()
    users = torch.arange(ch.U)
    with torch.no_grad():
        x = m.p_sample(m.batch_rows(users), users=users)
    within("plain p_sample against float64", x.numpy(), g["sample64"], g["own_sample"])
    rank = m.gene_ranklist(ch.TOPK)
    assert rank.shape == (ch.U, ch.TOPK) and rank.dtype == torch.int64 and int(rank.min()) >= ch.U and m.training is False
    ref_idx = g["rank"].astype(np.int64)
    ref_val = np.take_along_axis(ch.masked(g["sample32"], edges), ref_idx - ch.U, 1)
    val = np.take_along_axis(ch.masked(x.numpy(), edges), rank.numpy() - ch.U, 1)
    ok, why = tie_aware_rank_equal(rank.numpy(), val, ref_idx, ref_val, atol=accept.bound_of(g["own_sample"], ch.ULP) * np.abs(g["sample64"]).max())
    assert ok, why
    assert np.isfinite(val).all()                                                        # no history item is listed
    assert m.full_sort_predict.__func__ is m.gene_ranklist.__func__
