"""DiffRec's kernels (csrc/diffrec.hip through ops.diffrec_x0_loss / ops.diffrec_chain_step) and Model/DiffRec.py on the MI355X,
against the restatements of tests/diffrec_host.py and the reference fixture of tests/golden/gen_diffrec.py.

Kernels: the tile is 128 x 128 x 16 with k segments of 64.  B in {1, 127, 128, 129}, N (I of the loss, the output width of the
chain) in {1, 127, 128, 129, 259}, K in {4, 16, 20, 64, 68, 1000}: tile row and column edges, more than one tile each way; one
float4, one k-tile, a partial k-tile, a segment edge, one past it, the default width with a partial last segment; the full
product, 120 cases per kernel.
Tolerance, measured and not chosen: the reference's own lines in torch fp32 on the CPU on the same inputs, their deviation from
float64 relative to the tensor's largest magnitude, asserted below 1e-4; the kernels are allowed 4 x max(that, 2^-24)
(accept.within_measured).  Every case runs twice over allocator memory dirtied with NaN, then 1e30: the two runs agree in their
bits.  pt is not all ones; an incoming gradient of 0.37 is held to the same rule against 0.37 x the float64 gradients.
Every row of the loss node's x0 holds an interaction, for the reason test_gpu_diffmm gives: the rule measures against a
tensor's largest magnitude, and at B = I = 1 a tensor is one number, err = out - 1.  That number is led by the exact term only
while |out| stays well below 1, as it does for a denoiser at the reference's initialisation at dataset sizes (std
sqrt(2 / (I + H)) at I = 15207, H = 1000 gives |out| about 0.2 over tanh-valued h).  W_out is therefore drawn with the std
that gives |out| about 0.2 at the case's own H, not with sqrt(2 / (I + H)) at the case's I: at I = 1 that makes |out| about
0.8, err a difference of two numbers of like size, and the check one of a 64-term fp32 chain's own rounding against a
vectorised host dot product (first run, B = I = 1, H = 64: loss 2.53e-7 against the bound 2.38e-7, ratio 1.06, every
other tensor of that case inside).  The chain's inputs are scaled so that tanh covers its linear and its saturated range, and
for the same reason p[0, 0] has magnitude 8 and the sign of that element's product: there p_next = c1 (z G^T + g0) + c2 p
is led by c2 p, one rounded product, and no difference of two terms of like size; one such element per tensor is enough, the
rule measures against the tensor's largest magnitude.
Without it the one number of the B = N = 1 cases was such a difference at two of the six K (first run: K = 64, p_next =
-0.026 from terms near 0.5, deviation 4.39e-6 where the host's fp32 lines drew 1.5e-7; K = 4, z_next 5.2e-7 against 2.4e-7),
and the host lines' own deviation there differed by a factor of 14 between two CPUs; the other 118 cases passed as they were.
Model: within 4 x max(the fixture's stored deviation, 2^-24) of the float64 restatement.  The largest deviation / bound of a
test is printed as `ratio`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffrec_host as dh  # noqa: E402
from accept import ULP24, bound_of, same_bits, within, within_measured  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BS, NS, KS = (1, 127, 128, 129), (1, 127, 128, 129, 259), (4, 16, 20, 64, 68, 1000)


CASES = [(B, N, K) for B in BS for N in NS for K in KS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _dirty(dev, B, N, K, fill):
    """Junk where the allocator will hand out d_out, the partials, the chain's outputs and the gradients."""
    for shape in ((3 * B, N + 8), (2 * B, K), (2 * N, K), (B, N // 128 + 2), (N + 8,), (B + 8,), (1,)):
        torch.full(shape, fill, device=dev)
    torch.full((B + 8,), fill, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()


# ---- (a) the loss node ----------------------------------------------------------------------------------------------------------
def loss_case(B, I, Hd, seed):
    rng = np.random.default_rng(seed)
    h = np.tanh(rng.standard_normal((B, Hd))).astype(np.float32)
    W = (rng.standard_normal((I, Hd)) * (0.2 / (0.63 * np.sqrt(Hd)))).astype(np.float32)     # |out| about 0.2 (see the module docstring)
    b = (rng.standard_normal(I) * 0.001).astype(np.float32)
    x0 = (rng.random((B, I)) < 0.15).astype(np.float32)
    x0[np.arange(B), np.arange(B) % I] = 1.0      # no empty row (see the module docstring)
    ts = rng.integers(0, dh.STEPS, B)
    ts[0] = 0
    if B > 4:
        ts[1:5] = (1, 2, 3, 4)                    # the whole SNR range
    pt = rng.uniform(0.2, 3.0, B)                 # importance weights: not all ones
    return h, W, b, x0, dh.snr_weight(ts), pt


def run_loss(dev, case, g, fill):
    from chaorec_amd import ops
    h, W, b, x0, wt, pt = case
    B, I, Hd = h.shape[0], W.shape[0], h.shape[1]
    th, tW, tb = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (h, W, b))
    bits = torch.from_numpy(dh.bit_table(x0).view(np.int32)).to(dev)
    tw, tp = torch.from_numpy(wt).to(dev), torch.from_numpy(pt).to(dev)
    _dirty(dev, B, I, Hd, fill)
    raw = ops.diffrec_out_loss_raw(th.detach(), tW.detach(), tb.detach(), bits, tw, tp)
    d_full = raw[2].cpu().numpy()
    assert d_full.shape == (B, ops.diffmm_ld(I)) and not d_full[:, I:].any(), "d_out's pad columns"
    _dirty(dev, B, I, Hd, fill)
    loss, reloss = ops.diffrec_x0_loss(th, tW, tb, bits, tw, tp)
    assert loss.shape == (1,) and reloss.dtype == torch.float64 and not reloss.requires_grad
    (loss.sum() * g).backward()
    torch.cuda.synchronize()
    out = dict(loss=loss.detach(), reloss_rows=reloss, d_out=raw[2][:, :I] * g, dh=th.grad, dW_out=tW.grad, db_out=tb.grad)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("B,I,Hd", CASES)
def test_loss_node(dev, B, I, Hd):
    case = loss_case(B, I, Hd, 10000 * B + 10 * I + Hd)
    runs = [run_loss(dev, case, 1.0, fill) for fill in (float("nan"), 1e30)]
    for k in runs[0]:
        assert same_bits(runs[0][k], runs[1][k]), f"{k}: two runs differ in their bits"
    failures, ratios = [], []
    for g, got in ((1.0, runs[0]), (0.37, run_loss(dev, case, 0.37, 1e30))):
        r64, r32 = dh.loss_node(*case, torch.float64, g=g), dh.loss_node(*case, torch.float32, g=g)
        for k in ("loss", "reloss_rows", "d_out", "dW_out", "db_out", "dh"):
            within_measured(f"loss node B={B} I={I} H={Hd} g={g} {k}", got[k], r32[k], r64[k], ULP24, failures=failures, ratios=ratios)
    print(f"loss node B={B} I={I} H={Hd}: largest ratio {max(ratios):.3f}")
    assert not failures, failures


@pytest.mark.parametrize("Hd", [4, 68, 132])
@pytest.mark.parametrize("I", [1, 129, 259])
@pytest.mark.parametrize("B", [1, 129])
def test_loss_launch_is_the_diffmm_launch_without_its_second_term(dev, B, I, Hd):
    """The two loss launches run one tile loop and one x0-error epilogue (csrc/out_tile.h).  With pt = 1 both c_row are the
    same float; with x0E = 0, F = 0 and e_loss = 0 DiffMM's r and acc2 are exactly 0 and kf = 0: the rows and the loss agree
    in their bits, d_out by value over all ld columns (acc + 0 acc2 turns a -0 into +0, so not by bits).  I = 259 is three
    column tiles, five of the eight dealt workgroups return early; H = 68 and 132 end in a partial segment after one and
    after two full ones; H = 4 is a single short tile."""
    from chaorec_amd import ops
    h, W, b, x0, wt, _ = loss_case(B, I, Hd, 10000 * B + 10 * I + Hd)
    th, tW, tb, tw = (torch.from_numpy(a).to(dev) for a in (h, W, b, wt))
    bits = torch.from_numpy(dh.bit_table(x0).view(np.int32)).to(dev)
    x0E, F = torch.zeros(B, ops.DIFFMM_D, device=dev), torch.zeros(I, ops.DIFFMM_D, device=dev)
    m_loss, m_rows, _, m_d, m_r = ops.diffmm_out_loss_raw(th, tW, tb, bits, x0E, F, tw, 0.0)
    r_loss, r_rows, r_d = ops.diffrec_out_loss_raw(th, tW, tb, bits, tw, torch.ones(B, dtype=torch.float64, device=dev))
    torch.cuda.synchronize()
    assert not m_r.cpu().numpy().any()
    assert same_bits(m_rows.cpu().numpy(), r_rows.cpu().numpy()), "diff_rows against reloss_rows"
    assert same_bits(m_loss.cpu().numpy(), r_loss.cpu().numpy()), "loss"
    assert m_d.shape == r_d.shape == (B, ops.diffmm_ld(I))
    assert np.array_equal(m_d.cpu().numpy(), r_d.cpu().numpy()), "d_out over all ld columns"


# ---- (b) the chain step ---------------------------------------------------------------------------------------------------------
def chain_case(B, N, K, seed):
    rng = np.random.default_rng(seed)
    z = np.tanh(rng.standard_normal((B, K)) * 1.5).astype(np.float32)
    G = (rng.standard_normal((N, K)) * (1.2 / np.sqrt(K))).astype(np.float32)
    g0 = (rng.standard_normal(N) * 0.1).astype(np.float32)
    p = (rng.standard_normal((B, N)) * 1.5).astype(np.float32)
    e = (rng.standard_normal(N) * 0.5).astype(np.float32)
    dot = z.astype(np.float64) @ G.astype(np.float64).T + g0
    p[0, 0] = 8.0 if dot[0, 0] >= 0 else -8.0     # the tensor's one led element (see the module docstring)
    return z, G, g0, p, e, float(np.float32(0.8125 + 0.01 * (seed % 7))), float(np.float32(0.1875))


@pytest.mark.parametrize("B,N,K", CASES)
def test_chain_step(dev, B, N, K):
    from chaorec_amd import ops
    case = chain_case(B, N, K, 7 * B + 3 * N + K)
    t = [torch.from_numpy(a).to(dev) for a in case[:5]]
    runs = []
    for fill in (float("nan"), 1e30):
        _dirty(dev, B, N, K, fill)
        pn, zn = ops.diffrec_chain_step(*t, case[5], case[6])
        torch.cuda.synchronize()
        assert pn.shape == zn.shape == (B, N)
        runs.append(dict(p_next=pn.cpu().numpy(), z_next=zn.cpu().numpy()))
    r64, r32 = dh.chain_step(*case, torch.float64), dh.chain_step(*case, torch.float32)
    failures, ratios = [], []
    for k in ("p_next", "z_next"):
        assert same_bits(runs[0][k], runs[1][k]), f"{k}: two runs differ in their bits"
        within_measured(f"chain B={B} N={N} K={K} {k}", runs[0][k], r32[k], r64[k], ULP24, failures=failures, ratios=ratios)
    sat = np.abs(r64["z_next"])
    assert B * N < 64 or ((sat > 0.9).any() and (sat < 0.3).any())
    print(f"chain B={B} N={N} K={K}: largest ratio {max(ratios):.3f}")
    assert not failures, failures


def test_strided_operands_travel_in_place_or_are_copied(dev):
    """h and W_out as column slices of wider buffers (a row stride that is a multiple of 4, and one that is not)."""
    from chaorec_amd import ops
    case = loss_case(5, 33, 20, 3)
    h, W, b, x0, wt, pt = case
    bits = torch.from_numpy(dh.bit_table(x0).view(np.int32)).to(dev)
    ref = ops.diffrec_out_loss_raw(*(torch.from_numpy(a).to(dev) for a in (h, W, b)), bits, torch.from_numpy(wt).to(dev), torch.from_numpy(pt).to(dev))
    for pad in (4, 3):
        wide_h, wide_W = torch.zeros(5, 20 + pad, device=dev), torch.zeros(33, 20 + pad, device=dev)
        wide_h[:, :20], wide_W[:, :20] = torch.from_numpy(h).to(dev), torch.from_numpy(W).to(dev)
        got = ops.diffrec_out_loss_raw(wide_h[:, :20], wide_W[:, :20], torch.from_numpy(b).to(dev), bits, torch.from_numpy(wt).to(dev),
                                       torch.from_numpy(pt).to(dev))
        for a, c in zip(ref, got):
            assert same_bits(a.cpu().numpy(), c.cpu().numpy())


def test_refused_shapes_raise_without_a_launch(dev):
    from chaorec_amd import ops
    z = lambda *s: torch.zeros(s, device=dev)   # noqa: E731
    out = torch.full((4, 8), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="H=6 is no multiple of 4"):
        ops.diffrec_check_shape(4, 8, 6)
    with pytest.raises(RuntimeError, match="H=6 is no multiple of 4"):
        ops.diffrec_chain_step(z(4, 6), z(8, 6), z(8), z(4, 8), z(8), 1.0, 0.0)
    with pytest.raises(RuntimeError, match="H=6 is no multiple of 4"):
        ops.diffrec_out_loss_raw(z(4, 6), z(8, 6), z(8), torch.zeros(4, 1, dtype=torch.int32, device=dev), z(4).double(), z(4).double() + 1)
    with pytest.raises(RuntimeError, match="diffrec: B=0"):
        ops.diffrec_chain_step(z(0, 8), z(8, 8), z(8), z(0, 8), z(8), 1.0, 0.0)
    with pytest.raises(ValueError, match="bits int32"):
        ops.diffrec_out_loss_raw(z(4, 8), z(8, 8), z(8), torch.zeros(4, 2, dtype=torch.int32, device=dev), z(4).double(), z(4).double() + 1)
    with pytest.raises(ValueError, match="float64"):
        ops.diffrec_out_loss_raw(z(4, 8), z(8, 8), z(8), torch.zeros(4, 1, dtype=torch.int32, device=dev), z(4), z(4) + 1)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and ops.diffrec_tiles() == (128, 128, 16)


# ---- (c) the model --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx(dev):
    g = dh.load_fixture(GOLDEN)
    edges = g["edges"].astype(np.int64)
    assert np.array_equal(edges, dh.small_case())
    model = dh.load_weights(dh.new_model(dev), g)
    assert model.fused and model.collapsed and model.collapse_route("cuda")
    return dict(g=g, edges=edges, model=model)


@pytest.mark.parametrize("fused", [True, False])
def test_model_diffusion_step(fx, dev, fused):
    g, model = fx["g"], fx["model"]
    model.fused = fused
    model.train()
    model.zero_grad()
    model.Lt_count.zero_()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    loss = model.diffusion_step(torch.arange(dh.U, device=dev), ts=t(g["ts"]), noise=t(g["noise"]), keep=t(g["keep"]))
    loss.backward()
    torch.cuda.synchronize()
    model.fused = True
    failures, ratios = [], []
    within("loss", float(loss.detach()), g["loss64"], g["own_loss"], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
    assert model.last["reloss"].dtype == torch.float64
    within("reloss", model.last["reloss"].cpu().numpy(), g["reloss64"], g["own_reloss"], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
    for n, p in model.named_parameters():
        within("grad " + n, p.grad.cpu().numpy(), g["grad64_" + n], g["own_grad_" + n], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
    assert np.array_equal(model.Lt_count.cpu().numpy(), np.bincount(g["ts"], minlength=dh.STEPS))
    print(f"model step fused={fused}: largest ratio {max(ratios):.3f}")
    assert not failures, failures


def test_fused_against_plain_on_the_same_device_draws(fx, dev):
    """The rows launch's own draws (noise and keep flags keyed by seed, step, user, item) under importance sampling, so pt is
    not 1: read back exactly (a = 0, s = 1 without dropout gives n; a = 0, s = 1/2 with it gives kept ? n : 0) and handed to
    the plain route and to the restatement.  Both routes are held to the restatement in float64, `own` from its fp32 run."""
    from chaorec_amd import ops
    g, model = fx["g"], fx["model"]
    model.train()
    users = torch.tensor([3, 11, 0, 7, 3], device=dev)
    B = users.numel()
    for tb, lb in dh.lt_sequence():
        model.update_Lt_history(torch.from_numpy(tb).to(dev), torch.from_numpy(lb).to(dev))
    assert np.array_equal(model.Lt_count.cpu().numpy(), g["Lt_count"]) and np.array_equal(model.Lt_history.cpu().numpy(), g["Lt_history"])
    assert np.allclose(model.importance_pt().cpu().numpy(), g["pt_all"], rtol=1e-14, atol=0)
    hist = (model.Lt_history.clone(), model.Lt_count.clone())
    torch.manual_seed(5)
    model._step = 40
    zero, one = torch.zeros(B, device=dev), torch.ones(B, device=dev)
    noise = ops.diffmm_rows_noised(users, model.hist[0], model.hist[1], dh.I, zero, one, seed=model.seed, step=41, salt=0).contiguous()
    keep = ops.diffmm_rows(users, model.hist[0], model.hist[1], dh.I, zero, one * 0.5, seed=model.seed, step=41, salt=0)[0] != 0
    assert 0.2 < float(keep.float().mean()) < 0.8 and np.array_equal(noise[0].cpu().numpy(), noise[4].cpu().numpy())    # user 3 twice

    def run(fused, given):
        model.Lt_history, model.Lt_count = hist[0].clone(), hist[1].clone()
        model.fused = fused
        model.zero_grad()
        model._step = 40
        if given is not None:       # the first run's timesteps and importance values, by handing sample_timesteps' result back
            model.sample_timesteps = lambda batch_size, device, method='uniform', uniform_prob=0.001: given
        try:
            loss = model.diffusion_step(users) if fused else model.diffusion_step(users, noise=noise, keep=keep)
        finally:
            model.fused = True
            if given is not None:
                del model.sample_timesteps
        loss.backward()
        torch.cuda.synchronize()
        return dict(loss=float(loss.detach()), reloss=model.last["reloss"].cpu().numpy(), **{n: p.grad.cpu().numpy().copy() for n, p in model.named_parameters()})

    fused = run(True, None)
    ts, pt = model.last["ts"], model.last["pt"]
    assert not bool((pt == 1).all()) and pt.dtype == torch.float64
    plain = run(False, (ts, pt))
    x0 = dh.dense_rows(fx["edges"])[users.cpu().numpy()]
    args = (x0, ts.cpu().numpy(), noise.cpu().numpy(), keep.cpu().numpy(), pt.cpu().numpy())
    r64, r32 = dh.training_step(dh.weights_of(g), *args), dh.training_step(dh.weights_of(g, torch.float32), *args)
    failures, ratios = [], []
    for name, got in (("fused", fused), ("plain", plain)):
        within_measured(f"{name} loss", got["loss"], r32["loss"], r64["loss"], ULP24, failures=failures, ratios=ratios)
        within_measured(f"{name} reloss", got["reloss"], r32["reloss"], r64["reloss"], ULP24, failures=failures, ratios=ratios)
        for n in dh.NAMES:
            within_measured(f"{name} grad {n}", got[n], r32["grads"][n], r64["grads"][n], ULP24, failures=failures, ratios=ratios)
    print(f"fused and plain on device draws: largest ratio {max(ratios):.3f}")
    model.Lt_history.zero_()
    model.Lt_count.zero_()
    assert not failures, failures


def test_p_sample_routes_and_the_ranking(fx, dev):
    from conftest import tie_aware_rank_equal
    g, edges, model = fx["g"], fx["edges"], fx["model"]
    c1, c2, a, beta = model.posterior_coefs()
    assert c2[0] == 0.0 and beta == 0.0
    model.eval()
    x0 = torch.from_numpy(dh.dense_rows(edges)).to(dev)
    failures, ratios = [], []
    with torch.no_grad():
        col = model.p_sample(x0)
        lit = model.p_sample_literal(x0)
    within("p_sample collapsed", col.cpu().numpy(), g["sample64"], g["own_sample"], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
    within("p_sample literal", lit.cpu().numpy(), g["sample64"], g["own_sample"], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
    print(f"p_sample: largest ratio {max(ratios):.3f}")
    assert not failures, failures
    i64, v64 = dh.top_lists(dh.masked(g["sample64"], edges))
    atol = bound_of(g["own_sample"], ULP24) * np.abs(g["sample64"]).max()
    for collapsed, scores in ((True, col), (False, lit)):
        model.collapsed = collapsed
        rank = model.gene_ranklist(dh.TOPK, batch_size=5).numpy()              # three user ranges, the last of two users
        model.collapsed = True
        assert rank.shape == (dh.U, dh.TOPK) and rank.min() >= dh.U and rank.max() < dh.U + dh.I      # ids offset by num_user
        val = np.take_along_axis(dh.masked(scores.cpu().numpy(), edges), rank - dh.U, 1)
        assert np.isfinite(val).all()                                            # no history item in any list
        assert len(set(rank[dh.U - 1].tolist())) == dh.TOPK                      # the user without history is ranked
        ok, why = tie_aware_rank_equal(rank - dh.U, val, i64, v64, atol=atol)
        assert ok, f"collapsed={collapsed}: {why}"
    assert model.training is False


def test_two_epochs_move_the_weights_from_fresh_moments(fx, dev):
    from chaorec_amd import epochs as te
    from chaorec_amd.dataload import DeviceUserBatches
    g = fx["g"]
    torch.manual_seed(1)
    model = dh.load_weights(dh.new_model(dev), g).train()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    made = []
    orig = torch.optim.AdamW

    def spy(*a, **kw):
        made.append(orig(*a, **kw))
        return made[-1]
    torch.optim.AdamW = spy
    try:
        loader = DeviceUserBatches(dh.U, 5, dev, seed=2)
        l1 = te._train_epoch_diffrec(model, None, None, loader)
        l2 = te._train_epoch_diffrec(model, None, None, loader)
    finally:
        torch.optim.AdamW = orig
    torch.cuda.synchronize()
    assert np.isfinite(l1) and np.isfinite(l2) and l1 > 0
    assert all(bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), before[n]) for n, p in model.named_parameters())
    assert len(made) == 2 and made[0] is not made[1]
    steps = [[int(s["step"]) for s in o.state.values()] for o in made]
    assert all(s == 3 for s in steps[0]) and all(s == 3 for s in steps[1]), steps     # the second epoch's moments restart
    assert made[0].defaults["weight_decay"] == 0 and made[0].defaults["lr"] == model.learning_rate
    assert int(model.Lt_count.sum()) == 2 * dh.U
