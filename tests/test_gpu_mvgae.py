"""MVGAE's kernels (csrc/mvgae.hip through ops_extra.mvgae_conv_tail / mvgae_tail) and Model/MVGAE.py on the MI355X, against
the float64 restatements of tests/mvgae_host.py and the reference fixture of tests/golden/gen_mvgae.py.

Tolerance of the nodes, measured and not chosen: the reference's own lines run in torch fp32 on the CPU on the same inputs
(mvgae_host.conv_tail_torch / tail_torch), their deviation from the float64 restatement is taken relative to the tensor's
largest magnitude, asserted below 1e-4, and the kernels are allowed 4 x max(that, 2^-24) (the project's rule,
accept.within_measured: another summation order, the device's exp / log).  The four BPR parts are one tensor, the four KL parts another.
The bound is per case and per tensor (each of the six gradient tables its own).  A sample's BPR coefficient follows its
score difference 1 : 1, so the kernel evaluates the z rows, scores and coefficients of the 3B batch rows in double.  The
batches are what a sampler hands out: a sample's negative is never its own positive (where there are two items), so no
sample has a score difference of exactly 0 whose whole gradient cancels.
Every node case runs twice over allocator memory dirtied with NaN, then 1e30: the two runs agree in their bits.
The kernels hold 4 rows per wave and 16 per workgroup: N in {1, 4, 5, 15, 16, 17, 67}.
Model: result_embed, the eight parts and every gradient within 4 x max(the fixture's stored deviation, 2^-24)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mvgae_host as mh  # noqa: E402
from accept import ULP24, same_bits, within, within_measured  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D = mh.D
RW, RB = 4, 16
NS = (1, RW, RW + 1, RB - 1, RB, RB + 1, 4 * RB + 3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    from chaorec_amd import ops_extra
    assert ops_extra.mvgae_rows() == (RW, RB)
    return torch.device("cuda:0")


def _dirty(dev, N, B, fill):
    """Junk where the allocator will hand out the outputs, the z rows, the partials and the gradients."""
    for shape in ((8 * N, D), (12 * B, D), (8 * B,), (N + 16,), (9,)):
        torch.full(shape, fill, device=dev)
    torch.full((N // 4 + 8,), fill, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()


def _state(dev, step=0):
    return torch.tensor([step, step], dtype=torch.int64, device=dev)


# ---- (a) the conv epilogue -------------------------------------------------------------------------------------------------
def conv_case(N, seed):
    """s, bias, gy, a mask with one fully dropped row; one negative-only row (s + bias < 0 everywhere)."""
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal((N, D)) * np.exp(rng.uniform(-2, 2, (N, 1)))).astype(np.float32)
    bias = (0.1 * rng.standard_normal(D)).astype(np.float32)
    gy = rng.standard_normal((N, D)).astype(np.float32)
    keep = rng.random((N, D)) >= 0.1
    keep[N // 2] = False
    s[N - 1] = -np.abs(s[N - 1]) - 1.0
    return s, bias, gy, keep


def run_conv(dev, s, bias, gy, keep, training, fill, state=None, seed=1, salt=0):
    from chaorec_amd import ops_extra
    N = s.shape[0]
    ts, tb = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (s, bias))
    tk = torch.from_numpy(keep).to(dev) if keep is not None else None
    _dirty(dev, N, 1, fill)
    y = ops_extra.mvgae_conv_tail(ts, tb, state if state is not None else _state(dev), seed, salt, training, tk)
    y.backward(torch.from_numpy(gy).to(dev))
    torch.cuda.synchronize()
    return [a.detach().cpu().numpy() for a in (y, ts.grad, tb.grad)]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("N", NS)
def test_conv_epilogue(dev, N, training):
    s, bias, gy, keep = conv_case(N, 100 + N)
    assert not keep[N // 2].any() and ((s[N - 1] + bias) < 0).all()
    runs = [run_conv(dev, s, bias, gy, keep, training, fill) for fill in (float("nan"), 1e30)]
    for name, a, b in zip(("y", "gs", "gbias"), *runs):
        assert same_bits(a, b), f"{name}: two runs differ in their bits"
    y64 = mh.conv_tail(s, bias, keep, training)
    gs64, gb64 = mh.conv_tail_bwd(gy, s, bias, keep, training)
    y32, backward = mh.conv_tail_torch(s, bias, keep, training, torch.float32)
    gs32, gb32 = backward(gy)
    failures = []
    for name, got, r32, r64 in zip(("y", "gs", "gbias"), runs[0], (y32, gs32, gb32), (y64, gs64, gb64)):
        within_measured(f"conv N={N} training={training} {name}", got, r32, r64, ULP24, failures=failures)
    if training:
        assert not runs[0][0][N // 2].any() and not runs[0][1][N // 2].any()           # the fully dropped row
    assert (runs[0][0][N - 1][keep[N - 1] | (not training)] < 0).all()               # the negative-only row
    assert not failures, failures


# ---- (b) the tail ----------------------------------------------------------------------------------------------------------
def tail_case(N, B, U, seed, kind="random"):
    """Six fp32 tables (means N(0, 1), log-variances uniform in [-8, 11.5], one element exactly 10 in a row the batch
    names), a batch of global ids and four noise tables."""
    rng = np.random.default_rng(seed)
    tabs = [(rng.standard_normal((N, D)) if k % 2 == 0 else rng.uniform(-8.0, 11.5, (N, D))).astype(np.float32) for k in range(6)]
    I = N - U
    users = rng.integers(0, U, B)
    pos = rng.integers(U, N, B) if I > 0 else np.zeros(B, dtype=np.int64)
    neg = rng.integers(U, N, B) if I > 0 else np.zeros(B, dtype=np.int64)
    if I > 1:
        same = neg == pos                       # a sampler never hands out a sample's positive as its negative
        neg[same] = U + (pos[same] - U + 1) % I
    if kind == "one_user":
        users[:] = U - 1
    if kind == "pos_and_neg" and B >= 2:
        neg[1] = pos[0]
    tabs[1][users[0], 5] = 10.0
    tabs[5][pos[-1], 63] = 10.0
    eps = rng.standard_normal((4, N, D)).astype(np.float32)
    return tabs, users.astype(np.int64), pos.astype(np.int64), neg.astype(np.int64), eps


def run_tail(dev, tabs, users, pos, neg, eps, training, fill, kl_weight=0.1, state=None, seed=1, return_eps=False, gscale=1.0):
    from chaorec_amd import ops_extra
    N, B = tabs[0].shape[0], len(users)
    tt = [torch.from_numpy(t).to(dev).requires_grad_(True) for t in tabs]
    ids = [torch.from_numpy(a).to(dev) for a in (users, pos, neg)]
    te = torch.from_numpy(eps).to(dev) if eps is not None else None
    _dirty(dev, N, B, fill)
    out = ops_extra.mvgae_tail(*tt, *ids, kl_weight, state if state is not None else _state(dev), seed, training, te, return_eps)
    (out[0] * gscale).sum().backward()
    torch.cuda.synchronize()
    res = dict(total=out[0], parts=out[1], Pm=out[2], grads=[t.grad for t in tt])
    if return_eps:
        res["eps"] = out[3]
    return {k: ([a.detach().cpu().numpy() for a in v] if isinstance(v, list) else v.detach().cpu().numpy()) for k, v in res.items()}


TAIL_CASES = ([(N, 2, max(1, N // 2), "random") for N in NS]
              + [(N, B, U, "random") for (N, U) in ((5, 1), (67, 30)) for B in (1, 2, 63, 64, 65, 300)]
              + [(67, 65, 30, "one_user"), (17, 64, 6, "pos_and_neg"), (16, 300, 2, "one_user")])


GRADS = ("dVm", "dVl", "dTm", "dTl", "dCm", "dCl")


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("N,B,U,kind", TAIL_CASES)
def test_tail(dev, N, B, U, kind, training):
    tabs, users, pos, neg, eps = tail_case(N, B, U, 7 * N + B + U, kind)
    count = np.bincount(np.concatenate([users, pos, neg]), minlength=N)
    if kind == "one_user":
        assert count[U - 1] >= B
    if B == 300 and (U == 1 or kind == "one_user"):
        assert count.max() > 64                    # a row named by more than 64 slots
    if (N, B) == (67, 1):
        assert (count == 0).sum() >= 60            # rows named by none
    if kind == "pos_and_neg":
        assert neg[1] == pos[0]
    assert (np.concatenate(tabs[1::2]) == 10.0).sum() >= 1 and (N < RW or max(t.max() for t in tabs[1::2]) > 10.0)
    runs = [run_tail(dev, tabs, users, pos, neg, eps, training, fill) for fill in (float("nan"), 1e30)]
    for k in ("total", "parts", "Pm"):
        assert same_bits(runs[0][k], runs[1][k]), f"{k}: two runs differ in their bits"
    for k, (a, b) in enumerate(zip(runs[0]["grads"], runs[1]["grads"])):
        assert same_bits(a, b), f"gradient {k}: two runs differ in their bits"
    f = mh.tail(tabs, users, pos, neg, 0.1, eps, training)
    g64 = mh.tail_bwd(tabs, users, pos, neg, 0.1, eps, training)
    total32, parts32, pm32, g32 = mh.tail_torch(tabs, users, pos, neg, 0.1, eps, training, torch.float32)
    failures = []
    tag = f"tail N={N} B={B} U={U} {kind} training={training}"
    got = runs[0]
    within_measured(f"{tag} total", got["total"][0], total32, f["total"], ULP24, failures=failures)
    within_measured(f"{tag} BPR parts", got["parts"][:4], parts32[:4], f["parts"][:4], ULP24, failures=failures)
    within_measured(f"{tag} KL parts", got["parts"][4:], parts32[4:], f["parts"][4:], ULP24, failures=failures)
    within_measured(f"{tag} Pm", got["Pm"], pm32, f["Pm"], ULP24, failures=failures)
    for name, a, r32, r64 in zip(GRADS, got["grads"], g32, g64):
        within_measured(f"{tag} {name}", a, r32, r64, ULP24, failures=failures)
    assert not failures, failures


def test_tail_scales_with_the_incoming_gradient(dev):
    tabs, users, pos, neg, eps = tail_case(17, 9, 6, 3)
    a = run_tail(dev, tabs, users, pos, neg, eps, True, 0.0)
    b = run_tail(dev, tabs, users, pos, neg, eps, True, 0.0, gscale=-2.0)
    for x, y in zip(a["grads"], b["grads"]):
        assert same_bits(-2.0 * x, y)                # (a power of two: exact)


# ---- the device-drawn path -------------------------------------------------------------------------------------------------
def test_device_draws_are_a_function_of_seed_and_step(dev):
    tabs, users, pos, neg, _ = tail_case(67, 65, 30, 11)
    users[1] = users[0]                                   # two slots naming one row
    a = run_tail(dev, tabs, users, pos, neg, None, True, 0.0, state=_state(dev, 5), seed=99, return_eps=True)
    b = run_tail(dev, tabs, users, pos, neg, None, True, float("nan"), state=_state(dev, 5), seed=99, return_eps=True)
    c = run_tail(dev, tabs, users, pos, neg, None, True, 0.0, state=_state(dev, 6), seed=99, return_eps=True)
    for k in ("total", "parts", "Pm", "eps"):
        assert same_bits(a[k], b[k]), k
    assert all(same_bits(x, y) for x, y in zip(a["grads"], b["grads"]))
    assert not same_bits(a["eps"], c["eps"]) and not same_bits(a["total"], c["total"]) and same_bits(a["Pm"], c["Pm"])
    e = a["eps"]                                          # [4, 3, B, 64]
    assert e.shape == (4, 3, 65, D) and same_bits(e[:, 0, 0], e[:, 0, 1])
    for q in np.nonzero(pos == pos[0])[0]:
        assert same_bits(e[:, 1, 0], e[:, 1, q])
    # fed back as GIVEN tables, the returned rows reproduce loss and gradients bit for bit: the backward redrew the forward's
    given = np.zeros((4, 67, D), dtype=np.float32)
    for k, ids in enumerate((users, pos, neg)):
        given[:, ids] = e[:, k]
    d = run_tail(dev, tabs, users, pos, neg, given, True, 0.0, state=_state(dev, 1), seed=3)
    for k in ("total", "parts", "Pm"):
        assert same_bits(a[k], d[k]), k
    assert all(same_bits(x, y) for x, y in zip(a["grads"], d["grads"]))
    # mean and variance of the noise over the distinct rows drawn, within five standard errors of 0 and 1
    rows = np.concatenate([e[:, k][:, np.unique(ids, return_index=True)[1]] for k, ids in enumerate((users, pos, neg))], axis=1)
    n = rows.size
    assert abs(rows.mean()) <= 5 / np.sqrt(n) and abs(rows.var() - 1.0) <= 5 * np.sqrt(2.0 / n), (rows.mean(), rows.var(), n)


def test_device_dropout_redrawn_by_the_backward(dev):
    N = 67
    s, bias, gy, _ = conv_case(N, 5)
    a = run_conv(dev, s, bias, gy, None, True, 0.0, state=_state(dev, 5), seed=99, salt=7)
    b = run_conv(dev, s, bias, gy, None, True, float("nan"), state=_state(dev, 5), seed=99, salt=7)
    c = run_conv(dev, s, bias, gy, None, True, 0.0, state=_state(dev, 6), seed=99, salt=7)
    e = run_conv(dev, s, bias, gy, None, True, 0.0, state=_state(dev, 5), seed=99, salt=8)
    assert all(same_bits(x, y) for x, y in zip(a, b)) and not same_bits(a[0], c[0]) and not same_bits(a[0], e[0])
    implied = a[0] != 0                                                         # (no element of s + bias is 0)
    assert np.array_equal(implied, mh.keep_mask(99, 5, 7, N)), "the device's flags are not the restated counter RNG's"
    d = run_conv(dev, s, bias, gy, implied, True, 0.0, state=_state(dev, 1), seed=3, salt=0)
    assert all(same_bits(x, y) for x, y in zip(a, d))                               # given flags reproduce the drawn run
    big = 4099
    s2, bias2, gy2, _ = conv_case(big, 6)
    frac = float((run_conv(dev, s2, bias2, gy2, None, True, 0.0, state=_state(dev, 2), seed=1234, salt=3)[0] != 0).mean())
    assert abs(frac - 0.9) <= 5 * np.sqrt(0.09 / (big * D)), frac


# ---- the model -------------------------------------------------------------------------------------------------------------
def make_model(c, dev, n_layers=mh.N_LAYERS, fused=True):
    from chaorec_amd.Model import MVGAE
    torch.manual_seed(c["seed"])
    m = MVGAE(c["U"], c["I"], c["edges"], mh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
              mh.DIM_E, mh.KL_WEIGHT, n_layers, dev)
    m.fused_tail = m.fused_conv = fused
    return m


@pytest.mark.parametrize("fused", [True, False])
def test_model_meets_the_reference_fixture(dev, fused):
    g, c = mh.load_fixture(GOLDEN), mh.small_case()
    weights, plain = mh.init_weights(c)
    out = mh.step(weights, plain, c, c["users"], c["pos"], c["neg"], mh.KL_WEIGHT, mh.N_LAYERS, g["keep"], g["eps"], True)
    m = make_model(c, dev, fused=fused)
    for n, p in m.named_parameters():
        assert np.array_equal(p.detach().cpu().numpy(), weights[n]), n
    m.train()
    ids = [torch.from_numpy(c[k]) for k in ("users", "pos", "neg")]
    loss = m.loss(*ids, keep=[torch.from_numpy(k) for k in g["keep"]], eps=torch.from_numpy(g["eps"]))
    loss.backward()
    torch.cuda.synchronize()
    failures = []
    within("loss", float(loss), out["loss"], g["dev_loss"], ULP24, failures=failures)
    within("result_embed", m.result_embed.cpu().numpy(), out["result"], g["dev_result"], ULP24, failures=failures)
    parts = m.last["parts"].cpu().numpy()
    for k in range(8):
        within(f"part {k}", parts[k], out["parts"][k], g["dev_parts"][k], ULP24, failures=failures)
    names = mh.with_grad(mh.N_LAYERS)
    params = dict(m.named_parameters())
    assert tuple(n for n in mh.NAMES if params[n].grad is not None) == names
    for k, n in enumerate(names):
        within(f"grad {n}", params[n].grad.cpu().numpy(), out["grads"][n], g["dev_grads"][k], ULP24, failures=failures)
    # evaluation mode: the means are ranked, result_embed stays the last TRAINING forward's
    kept = m.result_embed.clone()
    m.eval()
    with torch.no_grad():
        ev = m.loss(*ids)
    ev64 = mh.step(weights, plain, c, c["users"], c["pos"], c["neg"], mh.KL_WEIGHT, mh.N_LAYERS, None, None, False)
    within("eval loss", float(ev), ev64["loss"], g["dev_eval_loss"], ULP24, failures=failures)
    within("eval result", m.last["pd_mu"].cpu().numpy(), ev64["result"], g["dev_eval_result"], ULP24, failures=failures)
    assert torch.equal(kept, m.result_embed)
    assert not failures, failures


@pytest.mark.parametrize("fused", [True, False])
def test_model_one_layer(dev, fused):
    """n_layers = 1 against the float64 step; the bound is the fixture's largest stored deviation (the same weights' scale)."""
    g, c = mh.load_fixture(GOLDEN), mh.small_case()
    weights, plain = mh.init_weights(c)
    keep = np.concatenate([g["keep"][4 * i:4 * i + 3] for i in range(3)])            # 3 x (n_layers + 2) masks
    out = mh.step(weights, plain, c, c["users"], c["pos"], c["neg"], mh.KL_WEIGHT, 1, keep, g["eps"], True)
    m = make_model(c, dev, n_layers=1, fused=fused)
    m.train()
    loss = m.loss(*(torch.from_numpy(c[k]) for k in ("users", "pos", "neg")), keep=[torch.from_numpy(k) for k in keep],
                  eps=torch.from_numpy(g["eps"]))
    loss.backward()
    torch.cuda.synchronize()
    failures = []
    within("loss", float(loss), out["loss"], g["dev_loss"], ULP24, failures=failures)
    within("result_embed", m.result_embed.cpu().numpy(), out["result"], g["dev_result"], ULP24, failures=failures)
    parts = m.last["parts"].cpu().numpy()
    for k in range(8):
        within(f"part {k}", parts[k], out["parts"][k], g["dev_parts"][k], ULP24, failures=failures)
    params = dict(m.named_parameters())
    names = mh.with_grad(1)
    assert tuple(n for n in mh.NAMES if params[n].grad is not None) == names
    worst = float(g["dev_grads"].max())
    for n in names:
        within(f"grad {n}", params[n].grad.cpu().numpy(), out["grads"][n], worst, ULP24, failures=failures)
    assert not failures, failures


def _trajectory(c, dev, captured, steps=3):
    from chaorec_amd.optim import FusedAdam, GraphedTrainStep
    m = make_model(c, dev)
    m.seed = 4321
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.01}])
    m.train()
    batch = tuple(torch.from_numpy(c[k]).to(dev) for k in ("users", "pos", "neg"))
    step = GraphedTrainStep(m, opt, example_batch=batch) if captured else None
    assert int(m._state[0]) == 0, "warm-up steps counted"
    losses = []
    for _ in range(steps):
        if captured:
            losses.append(step(*batch).clone())
        else:
            opt.zero_grad()
            loss = m.loss(*batch)
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return m, [float(x) for x in losses]


def test_captured_steps_equal_the_eager_ones(dev):
    """Three FusedAdam steps with device-drawn masks and noise, eager and through GraphedTrainStep: the same losses,
    weights, counter and result_embed."""
    c = mh.small_case()
    (me, le), (mc, lc) = _trajectory(c, dev, False), _trajectory(c, dev, True)
    assert le == lc and all(np.isfinite(le)) and len(set(le)) == 3
    assert torch.equal(me._state.cpu(), mc._state.cpu()) and int(me._state[0]) == 3
    for (n, a), b in zip(me.state_dict().items(), mc.state_dict().values()):
        assert torch.equal(a, b), n
    assert torch.equal(me.result_embed, mc.result_embed)


def test_gene_ranklist_is_topk_over_result_embed(dev):
    c = mh.small_case()
    m = make_model(c, dev)
    m.train()
    m.loss(*(torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))).backward()
    U, I, topk = c["U"], c["I"], 5
    ranks = m.gene_ranklist(topk=topk)
    assert ranks.dtype == torch.int64 and ranks.shape == (U, topk) and not ranks.is_cuda
    table = m.result_embed.cpu().double()
    score = table[:U] @ table[U:].t()
    for u, items in mh.user_item_dict(c["edges"]).items():
        score[u, torch.tensor(sorted(set(items))) - U] = 1e-6
    val, idx = torch.topk(score, topk)
    got = torch.gather(score, 1, ranks - U)
    assert torch.allclose(got, val, rtol=1e-5, atol=1e-7)
    assert float((ranks - U == idx).float().mean()) >= 0.95          # (ties and fp32 scores aside, the same lists)
