"""CF_Diff on the MI355X: the launches of csrc/cfdiff.hip per operand, on given and on device-drawn flags, and the whole model
against the golden the reference's own run left (tests/golden/cfdiff_small.npz).

Tolerance, measured not chosen (accept.within, the floor ULP = 2^-23 as in tests/test_gpu_bspm.py): for each compared array
bound = 4 x max(own, ULP) relative to the largest magnitude of the float64 array; `own` is the deviation of an fp32 computation
that is not the code under test from the float64 restatement on the same operands -- `ops.cfdiff_attention_plain` in fp32 on the
CPU for the per-operand checks, the reference's stored fp32 output for the golden, the fp32 run of the restatement for the
one-step gradients.  Every check prints deviation, own, bound and ratio.

Shapes: L = 1 (one key, softmax = 1), 33 (one past a 32-term segment and a 32-bit half word), 70 (a lane's second query: 64 + a
tail of 6), 1034 with B = 2 (the model's own length: 8 tiles of 128 and a tail of 10, 16 key words and a tail of 10 bits).

Measured on the MI355X (largest deviation / bound): per operand 0.87 without dropout (dq at L = 70, where the fp32 plain
composition's own deviation is below one ULP and the bound is 4 ULP), 0.95 on given flags (dq, L = 70), 0.40 on device-drawn flags,
0.35 at L = 1034; the whole model 0.32 (eval output), 0.18 for the largest gradient of one step (the plain route: 0.24), 0.60 for
the loss of a device-drawn step, 0.56 for p_sample."""
import functools
import logging
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import cfdiff_host as ch  # noqa: E402
from conftest import GOLDEN, tie_aware_rank_equal  # noqa: E402

from chaorec_amd import ops  # noqa: E402
from chaorec_amd.Model import CF_Diff  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 1), (3, 33), (3, 70), (2, 1034)]
SEED = 20241012


def within(what, got, ref, own, scale=None):
    return accept.within(what, got, ref, own, ch.ULP, scale=scale, zero_ref=ch.ZERO_REF)      # (takes tensors as they are)


@functools.lru_cache(maxsize=None)
def operands(B, L):
    gen = torch.Generator().manual_seed(1000 * L + B)
    return tuple(torch.randn(B, L, 16, generator=gen) for _ in range(4))          # q, k, v, dout


def host_reference(B, L, keep):
    """(float64 out, lse, dq, dk, dv) and the fp32 CPU plain composition's deviations from them (`own` per array)."""
    q, k, v, go = operands(B, L)
    res = {}
    for dt in (torch.float64, torch.float32):
        qa, ka, va = (t.detach().clone().to(dt).requires_grad_() for t in (q, k, v))      # (never the cached operands themselves)
        if dt == torch.float64:
            out = ch.attention(qa, ka, va, keep)
        else:
            out = ops.cfdiff_attention_plain(qa, ka, va, keep is not None, keep=keep)
        out.backward(go.to(dt))
        heads = lambda t: t.detach().reshape(B, L, 4, 4).permute(0, 2, 1, 3)
        lse = torch.logsumexp(heads(qa) @ heads(ka).transpose(2, 3) * 0.5, dim=-1)
        res[dt] = dict(out=out.detach(), lse=lse, dq=qa.grad, dk=ka.grad, dv=va.grad)
    ref = {n: t.numpy() for n, t in res[torch.float64].items()}
    own = {n: ch.rel_dev(res[torch.float32][n].numpy(), ref[n]) for n in ref}
    return ref, own


@functools.lru_cache(maxsize=None)
def eval_reference(B, L):
    return host_reference(B, L, None)


def run_fused(B, L, training, state=None, keep=None, salt=0, b0=0, seed=SEED):
    q, k, v, go = (t.to(DEV) for t in operands(B, L))
    qa, ka, va = (t.detach().clone().requires_grad_() for t in (q, k, v))
    out = ops.cfdiff_attention(qa, ka, va, training, seed, state, salt, None if keep is None else keep.to(DEV), b0)
    out.backward(go)
    lse = ops.cfdiff_attention_raw(q, k, v, training, seed, state, salt, None if keep is None else keep.to(DEV), b0)[1]
    return dict(out=out.detach(), lse=lse, dq=qa.grad, dk=ka.grad, dv=va.grad)


def ticked(n=1):
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    for _ in range(n):
        ops.step_tick(state)
    return state


# ---- per operand ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", SHAPES)
def test_forward_and_backward_without_dropout(B, L):
    ref, own = eval_reference(B, L)
    got = run_fused(B, L, False)
    for n in ("out", "lse", "dq", "dk", "dv"):
        within(f"L={L} eval {n}", got[n], ref[n], own[n])
    again = run_fused(B, L, False)
    assert all(torch.equal(got[n], again[n]) for n in got)                               # one owner, fixed order: the same bits
    if L == 1:
        assert torch.equal(got["out"].cpu(), operands(B, L)[2]) and not got["dq"].any() and not got["dk"].any()


def test_given_flags_with_a_dropped_and_a_kept_row():
    B, L = 3, 70
    gen = torch.Generator().manual_seed(4)
    keep = (torch.rand(B, 4, L, L, generator=gen) < 0.5).to(torch.uint8)
    keep[0, 1, 5] = 0                                                                    # every key dropped
    keep[1, 3, 64:] = 0                                                                  # ... for the whole tail of queries
    keep[2, 2, 69] = 1                                                                   # every key kept
    ref, own = host_reference(B, L, keep)
    got = run_fused(B, L, True, keep=keep)
    for n in ("out", "lse", "dq", "dk", "dv"):
        within(f"L={L} given flags {n}", got[n], ref[n], own[n])
        assert torch.isfinite(got[n]).all()
    out = got["out"].cpu()
    assert not out[0, 5, 4:8].any() and not out[1, 64:, 12:16].any() and out[0, 5, :4].any()      # exact zeros, never NaN
    q, k, v, _ = operands(B, L)
    full = ch.attention(q[2:3].double(), k[2:3].double(), v[2:3].double())[0, 69, 8:12] * 2.0
    within("the fully kept row is 2 P V", out[2, 69, 8:12], full, own["out"], np.abs(ref["out"]).max())


@pytest.mark.parametrize("B,L", [(3, 70), (2, 1034)])
def test_device_drawn_step(B, L):
    state = ticked(3)
    keep = ops.cfdiff_keep(B, L, SEED, state, 1)
    assert keep.shape == (B, 4, L, L) and keep.dtype == torch.uint8 and int(keep.max()) == 1
    assert torch.equal(keep, ops.cfdiff_keep(B, L, SEED, state, 1))                       # the same (seed, step): the same bits
    if L == 70:
        assert np.array_equal(keep.cpu().numpy(), ch.keep_flags(B, L, SEED, 3, 1))        # the keying, as the header states it
    # forward and backward against the plain composition in float64 fed these flags: the backward redraws the forward's bits
    ref, own = host_reference(B, L, keep.cpu())
    got = run_fused(B, L, True, state=state, salt=1)
    for n in ("out", "dq", "dk", "dv"):
        within(f"L={L} drawn {n}", got[n], ref[n], own[n])
    again = run_fused(B, L, True, state=state, salt=1)
    assert all(torch.equal(got[n], again[n]) for n in got)
    # a row's flags depend on its slot, not on the launch: B rows at once = B launches of one row at the same slots
    for b in range(B):
        assert torch.equal(ops.cfdiff_keep(1, L, SEED, state, 1, b0=b)[0], keep[b])
    q, k, v, _ = (t.to(DEV) for t in operands(B, L))
    whole = ops.cfdiff_attention_raw(q, k, v, True, SEED, state, 1)[0]
    for b in range(B):
        one = ops.cfdiff_attention_raw(q[b:b + 1], k[b:b + 1], v[b:b + 1], True, SEED, state, 1, b0=b)[0]
        assert torch.equal(one[0], whole[b])
    # the rate, and a fresh half of the flags at the next step, salt and seed: 6 standard deviations of a fair coin
    n = keep.numel()
    six = 6 * 0.5 / np.sqrt(n)
    frac = float(keep.float().mean())
    nxt = ops.cfdiff_keep(B, L, SEED, ticked(4), 1)
    print(f"L={L}: kept fraction {frac:.6f}, differs from the next step's in {float((nxt != keep).float().mean()):.6f} (6 sigma {six:.2e})")
    assert abs(frac - 0.5) <= six
    assert abs(float((nxt != keep).float().mean()) - 0.5) <= six
    assert abs(float((ops.cfdiff_keep(B, L, SEED, state, 2) != keep).float().mean()) - 0.5) <= six
    assert abs(float((ops.cfdiff_keep(B, L, SEED + 1, state, 1) != keep).float().mean()) - 0.5) <= six


def test_shapes_are_refused_without_a_launch():
    top = ops.cfdiff_max_len()
    for L in (0, top + 1):
        t = torch.zeros(2, L, 16, device=DEV)
        with pytest.raises(ValueError, match=f"cfdiff: L={L}"):
            ops.cfdiff_attention(t, t, t, False, 0, None, 0)
        with pytest.raises(ValueError, match=f"cfdiff: L={L}"):
            ops.cfdiff_keep(2, L, 0, ticked(), 0)
    with pytest.raises(ValueError, match="device draws need state"):
        t = torch.zeros(2, 5, 16, device=DEV)
        ops.cfdiff_attention(t, t, t, True, 0, None, 0)
    torch.cuda.synchronize()


def test_rows_noised_is_q_sample_without_dropout():
    g, edges = case()
    m = model()
    users = torch.tensor([5, 11, 0, 5], device=DEV)
    ts = torch.tensor([0, 9, 4, 0], device=DEV)                                          # (rows 0 and 3: the same user at the same t)
    a, s = m.sqrt_alphas_cumprod[ts].float().contiguous(), m.sqrt_one_minus_alphas_cumprod[ts].float().contiguous()
    noise = torch.from_numpy(g["noise"][:4]).to(DEV).contiguous()
    x_t = ops.diffmm_rows_noised(users, m.hist[0], m.hist[1], ch.I, a, s, noise)
    x0 = torch.from_numpy(ch.dense_rows(edges)).to(DEV)[users]
    assert torch.equal(x_t, m.q_sample(x0, ts, noise))
    drawn = ops.diffmm_rows_noised(users, m.hist[0], m.hist[1], ch.I, a, s, None, seed=3, step=2, salt=7)
    assert torch.equal(drawn[0], drawn[3]) and torch.isfinite(drawn).all()               # keyed by user and item, not by the place
    n = (drawn - a[:, None] * x0) / s[:, None]
    assert abs(float(n.mean())) < 6 / np.sqrt(n.numel()) and abs(float(n.std()) - 1.0) < 0.2


# ---- the whole model --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case():
    g = ch.load_fixture(GOLDEN)
    return g, g["edges"].astype(np.int64)


def new_model(fused=True, dim_inters=ch.DIM_INTERS, num_item=ch.I):
    g, edges = case()
    return CF_Diff(ch.U, num_item, ch.user_item_dict(edges), ch.NOISE_SCALE, ch.NOISE_MIN, ch.NOISE_MAX, ch.STEPS, 0.001, DEV,
                   fused=fused, seed=SEED, dim_inters=dim_inters)


@functools.lru_cache(maxsize=None)
def model(fused=True):
    return ch.load_weights(new_model(fused), case()[0]).eval()


def test_cam_ae_eval_against_the_golden():
    g, _ = case()
    users = torch.arange(ch.U, device=DEV)
    x_t, ts = torch.from_numpy(g["x_t"]).to(DEV), torch.from_numpy(g["ts"]).to(DEV)
    with torch.no_grad():
        fused = model().denoise(x_t, users, ts)
        plain = model(False).denoise(x_t, users, ts)
    assert fused.shape == (ch.U, ch.I) and fused.dtype == torch.float32
    scale = np.abs(g["out64"]).max()
    within("fused CAM_AE against float64", fused, g["out64"], g["own_out"])
    within("fused CAM_AE against the reference's fp32", fused, g["out32"].astype(np.float64), 2 * g["own_out"], scale)
    within("plain CAM_AE against float64", plain, g["out64"], g["own_out"])
    within("fused against plain", fused, plain.double(), g["own_out"], scale)
    h_sec = model().encode_sec_hop(users)
    ref = torch.from_numpy(g["sec_hop"]).double() @ torch.from_numpy(g["w_encoder.weight"]).double().T + torch.from_numpy(g["w_encoder.bias"]).double()
    own = ch.rel_dev((torch.from_numpy(g["sec_hop"]) @ torch.from_numpy(g["w_encoder.weight"]).T + torch.from_numpy(g["w_encoder.bias"])).numpy(), ref.numpy())
    within("encoder(x_sec_hop) as an SpMM", h_sec, ref, own)


def given_keeps(B, L, with_attn=True):
    rng = torch.Generator().manual_seed(9)
    flags = lambda *shape, p=0.5: (torch.rand(shape, generator=rng) >= p).to(torch.uint8)
    keeps = dict(drop=flags(B, L - ch.EMB), drop1=[flags(B, L, 16, p=0.8) for _ in range(2)], drop2=[flags(B, L, 16) for _ in range(2)])
    attn = [flags(B, 4, L, L) for _ in range(2)]
    attn[0][1, 1, 7] = 0
    if with_attn:
        keeps["attn"] = attn
    return keeps


def restated_step(users, ts, keeps, dtype):
    """One training step of the restatement (cfdiff_host.cam_ae) in `dtype` on the CPU -> (loss, {name: gradient})."""
    g, edges = case()
    w = {n: t.clone().requires_grad_() for n, t in ch.weights_of(g, dtype).items()}
    out = ch.cam_ae(w, torch.from_numpy(g["x_t"])[users], torch.from_numpy(g["sec_hop"])[users], ts, keeps)
    mse = ((torch.from_numpy(ch.dense_rows(edges))[users].to(dtype) - out) ** 2).mean(1)
    val = (torch.from_numpy(ch.snr_weight(ts.numpy())) * mse).mean()
    val.backward()
    return val.detach().numpy(), {n: t.grad.numpy() for n, t in w.items()}


def to_dev(keeps):
    return {n: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for n, v in keeps.items()}


def test_one_diffusion_step_against_float64():
    g, edges = case()
    users = torch.from_numpy(ch.STEP_USERS)
    B, L = users.numel(), ch.DIM_INTERS + ch.EMB
    ts, noise = torch.from_numpy(g["ts"])[users], torch.from_numpy(g["noise"])[users]
    keeps = given_keeps(B, L)
    l64, g64 = restated_step(users, ts, keeps, torch.float64)
    l32, g32 = restated_step(users, ts, keeps, torch.float32)
    ratios = {}
    for fused in (True, False):
        m = ch.load_weights(new_model(fused), g).train()
        loss = m.diffusion_step(users, ts=ts, noise=noise, keeps=to_dev(keeps))
        loss.backward()
        tag = "fused" if fused else "plain"
        assert torch.equal(m.last["x_t"].cpu(), torch.from_numpy(g["x_t"])[users])         # the rows launch is q_sample, bit for bit
        within(f"{tag} loss", loss.detach(), l64, ch.rel_dev(l32, l64))
        ratios[tag] = max(within(f"{tag} grad {n}", p.grad, g64[n], ch.rel_dev(g32[n], g64[n])) for n, p in m.CAM_AE.named_parameters())
        assert np.array_equal(m.Lt_count.cpu().numpy(), np.bincount(ts.numpy(), minlength=ch.STEPS))
    print(f"largest gradient ratio: {ratios}")


def test_fused_against_plain_on_the_same_device_draws():
    """The attention's flags drawn on the device (step 1 of SEED, salt = layer); the plain route on the device takes the same flags
    from cfdiff_keep, and so does the float64 restatement here.  `own` of every gradient is the fp32 restatement's deviation from
    the float64 one, as in the test above; fused against plain is measured on the float64 array's scale."""
    g, edges = case()
    users = torch.from_numpy(ch.STEP_USERS)
    B, L = users.numel(), ch.DIM_INTERS + ch.EMB
    ts, noise = torch.from_numpy(g["ts"])[users], torch.from_numpy(g["noise"])[users]
    keeps = given_keeps(B, L, with_attn=False)
    grads, losses = {}, {}
    for fused in (True, False):
        m = ch.load_weights(new_model(fused), g).train()
        loss = m.diffusion_step(users, ts=ts, noise=noise, keeps=to_dev(keeps))
        loss.backward()
        losses[fused], grads[fused] = loss.detach(), {n: p.grad for n, p in m.CAM_AE.named_parameters()}
        assert int(m._state[1]) == 1
    again = ch.load_weights(new_model(True), g).train()
    l2 = again.diffusion_step(users, ts=ts, noise=noise, keeps=to_dev(keeps))
    assert torch.equal(l2.detach(), losses[True])                                        # the same seed and step: the same step
    drawn = dict(keeps, attn=[ops.cfdiff_keep(B, L, SEED, ticked(1), layer).cpu() for layer in range(2)])
    l64, g64 = restated_step(users, ts, drawn, torch.float64)
    l32, g32 = restated_step(users, ts, drawn, torch.float32)
    own = ch.rel_dev(l32, l64)
    within("drawn loss, fused against float64", losses[True], l64, own)
    within("drawn loss, plain against float64", losses[False], l64, own)
    for n in grads[True]:
        own, scale = ch.rel_dev(g32[n], g64[n]), np.abs(g64[n]).max()
        within(f"drawn grad {n}, fused against float64", grads[True][n], g64[n], own)
        within(f"drawn grad {n}, fused against plain", grads[True][n], grads[False][n].double(), own, scale)


def test_p_sample_and_the_ranking():
    g, edges = case()
    users = torch.arange(ch.U, device=DEV)
    scale = np.abs(g["sample64"]).max()
    bound = accept.bound_of(g["own_sample"], ch.ULP) * scale
    ref_idx = g["rank"].astype(np.int64)
    ref_val = np.take_along_axis(ch.masked(g["sample32"], edges), ref_idx - ch.U, 1)
    rows = {}
    for fused in (True, False):
        m = model(fused)
        with torch.no_grad():
            rows[fused] = m.p_sample(m.batch_rows(users), users=users)
        within(f"p_sample fused={fused} against float64", rows[fused], g["sample64"], g["own_sample"])
        rank = m.gene_ranklist(ch.TOPK, to_cpu=False)
        assert rank.shape == (ch.U, ch.TOPK) and rank.dtype == torch.int64 and rank.is_cuda and int(rank.min()) >= ch.U
        idx = rank.cpu().numpy()
        val = np.take_along_axis(ch.masked(rows[fused].cpu().numpy(), edges), idx - ch.U, 1)
        ok, why = tie_aware_rank_equal(idx, val, ref_idx, ref_val, atol=bound)
        assert ok, why
        assert np.isfinite(val).all() and np.array_equal(m.gene_ranklist(ch.TOPK).numpy(), idx)
    within("p_sample fused against plain", rows[True], rows[False].double(), g["own_sample"], scale)


def test_one_epoch_of_the_loop(caplog):
    from chaorec_amd import train_and_evaluate as te
    g, edges = case()
    torch.manual_seed(3)
    I = 64                                                                               # (the loop ranks 50 items per user)
    m = new_model(True, dim_inters=60, num_item=I)                                        # L = 70
    rng = np.random.RandomState(11)
    val = [[u] + (ch.U + rng.choice(I, 2, replace=False)).tolist() for u in range(ch.U)]
    test = [[u] + (ch.U + rng.choice(I, 3, replace=False)).tolist() for u in range(ch.U)]
    before = {n: p.detach().clone() for n, p in m.CAM_AE.named_parameters()}
    history = []
    loader = types.SimpleNamespace(batch_size=5, seed=1)
    with caplog.at_level(logging.INFO):
        out = te.train_and_evaluate(m, loader, val, test, None, 2, model_name="CF_Diff", topk=(5, 10), history=history, graph=False)
    assert set(out) == {5, 10} and all(np.isfinite(v) for mm in out.values() for v in mm.values())
    assert len(history) == 2 and all(np.isfinite(h["loss"]) and h["loss"] > 0 for h in history)
    assert all(not torch.equal(before[n], p.detach()) for n, p in m.CAM_AE.named_parameters())        # every used weight moved
    assert int(m.Lt_count.sum()) == 2 * ch.U and int(m._state[0]) == 2 * 3
