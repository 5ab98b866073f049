"""LightGODE's loss node (csrc/lightgode.hip through ops.lightgode_loss), the Euler step and Model/LightGODE.py on the MI355X,
against the restatements of tests/lightgode_host.py and the reference fixture of tests/golden/gen_lightgode.py.

The node: B in {2, 3, 31, 32, 33, 64, 65, 257} over 300 users and 200 items and B = 1024 over 2000 and 1500 -- the edges of the
32-row blocks, of the 128-column steps and of the waves' 32 columns inside one, one and several column splits (257: 3, 1024: 4);
not the workload.  Ids are drawn with repeats (B <= 3: without, a batch of one id twice has unif = log 1 = 0 and nothing to
measure against).  Tolerance, measured and not chosen: the reference's own lines in torch fp32 on the CPU on the same inputs,
their deviation from float64 relative to the tensor's largest magnitude, asserted below 1e-4; the node is allowed
4 x max(that, 2^-24) (accept.within_measured).  Every case runs twice over allocator memory dirtied with NaN: the two runs agree
in their bits, and so does the joined-table form.  Model: within 4 x max(the fixture's stored deviation, 2^-24) of the
reference's float64 run.  Every check prints deviation, own, bound and ratio."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lightgode_host as lh  # noqa: E402
from accept import ULP24, bound_of, rel_dev, same_bits, within, within_measured  # noqa: E402
from conftest import tie_aware_rank_equal  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = lh.PARTS + ("g_u", "g_i")
NODE_CASES = [(300, 200, B) for B in (2, 3, 31, 32, 33, 64, 65, 257)] + [(2000, 1500, 1024)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture():
    return lh.load_fixture(GOLDEN)


def tables(nU, nI, gen):
    """Rows of std 0.05 around a common vector of the same size: the pair distances spread."""
    return (torch.randn(nU, lh.D, generator=gen) * 0.05 + 0.05 * torch.randn(1, lh.D, generator=gen),
            torch.randn(nI, lh.D, generator=gen) * 0.05 + 0.05 * torch.randn(1, lh.D, generator=gen))


@functools.lru_cache(maxsize=None)
def node_case(nU, nI, B, kind="drawn"):
    """-> (W_u, W_i, users, items, the fp32 lines' results, the float64 lines' results); computed once, left unchanged."""
    gen = torch.Generator().manual_seed(1000 * B + nU)
    W_u, W_i = tables(nU, nI, gen)
    if kind in ("distinct", "zero_row") or B <= 3:
        users, items = torch.randperm(nU, generator=gen)[:B], torch.randperm(nI, generator=gen)[:B]
    else:
        users, items = torch.randint(0, nU, (B,), generator=gen), torch.randint(0, nI, (B,), generator=gen)
    if kind == "one_user":
        users = torch.full((B,), 7, dtype=torch.int64)
    if kind == "zero_row":
        W_u[users[3]] = 0.0
    refs = tuple(lh.reference_loss(W_u, W_i, users, items, lh.GAMMA, dt) for dt in (torch.float32, torch.float64))
    return (W_u, W_i, users, items) + refs


def dirty(dev, B, nU, nI):
    """NaN where the allocator will hand out the workspace, the row gradients and the table gradients."""
    from chaorec_amd import ops
    for n in (ops.lightgode_workspace(B), 2 * B * lh.D, nU * lh.D, nI * lh.D, (nU + nI) * lh.D, 4, 1):
        torch.full((n,), float("nan"), device=dev)
    torch.cuda.synchronize()


def run_node(dev, W_u, W_i, users, items, joined=False):
    from chaorec_amd import ops
    dirty(dev, users.numel(), W_u.shape[0], W_i.shape[0])
    u, i = users.to(dev), items.to(dev)
    if joined:
        T = torch.cat((W_u, W_i)).to(dev).requires_grad_(True)
        loss, parts = ops.lightgode_loss(T, None, u, i, lh.GAMMA, item_offset=W_u.shape[0])
        loss.backward()
        g_u, g_i = T.grad[:W_u.shape[0]], T.grad[W_u.shape[0]:]
    else:
        a, b = W_u.to(dev).requires_grad_(True), W_i.to(dev).requires_grad_(True)
        loss, parts = ops.lightgode_loss(a, b, u, i, lh.GAMMA)
        loss.backward()
        g_u, g_i = a.grad, b.grad
    assert loss.shape == () and parts.shape == (4,) and not parts.requires_grad
    p = parts.cpu().numpy()
    assert same_bits(p[0], loss.detach().cpu().numpy())
    return dict(loss=p[0], align=p[1], unif_u=p[2], unif_i=p[3], g_u=g_u.cpu().numpy(), g_i=g_i.cpu().numpy())


def check_node(what, got, r32, r64, keys=KEYS):
    failures, ratios = [], []
    for k in keys:
        within_measured(f"{what}, {k}", got[k], r32[k], r64[k], ULP24, failures=failures, ratios=ratios)
    print(f"{what}: ratio {max(ratios):.3f}")
    assert not failures, failures


# ---- the node -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nU,nI,B", NODE_CASES)
def test_node_against_float64(dev, nU, nI, B):
    W_u, W_i, users, items, r32, r64 = node_case(nU, nI, B)
    got = run_node(dev, W_u, W_i, users, items)
    check_node(f"B={B}", got, r32, r64)
    again = run_node(dev, W_u, W_i, users, items)
    joined = run_node(dev, W_u, W_i, users, items, joined=True)
    for k in KEYS:
        assert same_bits(got[k], again[k]), f"{k}: two runs differ"
        assert same_bits(got[k], joined[k]), f"{k}: the joined table differs"


@pytest.mark.parametrize("kind", ["one_user", "distinct"])
def test_extreme_batches(dev, kind):
    """All users one id: every user pair is two equal rows, e = 1 enters S (unif_u = log 1 = 0, as the reference has it) and
    nothing enters the gradient.  No repeats at all: every table row has one addend."""
    W_u, W_i, users, items, r32, r64 = node_case(300, 200, 64, kind)
    got = run_node(dev, W_u, W_i, users, items)
    if kind == "one_user":
        assert float(r64["unif_u"]) == 0.0 and float(got["unif_u"]) == 0.0
        assert not got["g_u"][np.arange(300) != 7].any()
        check_node(kind, got, r32, r64, keys=tuple(k for k in KEYS if k != "unif_u"))
    else:
        assert len(set(users.tolist())) == 64 and len(set(items.tolist())) == 64
        check_node(kind, got, r32, r64)


def test_a_zero_embedding_row(dev):
    """F.normalize's 1e-12 clamp scales that row's gradient by 1e12: it is compared on its own and must not set the scale for
    the other rows."""
    W_u, W_i, users, items, r32, r64 = node_case(300, 200, 8, "zero_row")
    row = int(users[3])
    assert not W_u[row].any() and len(set(users.tolist())) == 8
    got = run_node(dev, W_u, W_i, users, items)
    assert np.isfinite(got["g_u"]).all() and np.isfinite(got["g_i"]).all()
    check_node("zero row", got, r32, r64, keys=lh.PARTS + ("g_i",))
    within_measured("zero row, its own gradient", got["g_u"][row], r32["g_u"][row], r64["g_u"][row], ULP24)
    assert np.abs(r64["g_u"][row]).max() > 1e6 * np.abs(np.delete(r64["g_u"], row, 0)).max()
    within_measured("zero row, the other rows", np.delete(got["g_u"], row, 0), np.delete(r32["g_u"], row, 0), np.delete(r64["g_u"], row, 0),
                    ULP24)


def test_gradient_scales_with_the_upstream_gradient(dev):
    from chaorec_amd import ops
    W_u, W_i, users, items, r32, r64 = node_case(300, 200, 33)
    a, b = W_u.to(dev).requires_grad_(True), W_i.to(dev).requires_grad_(True)
    loss, _ = ops.lightgode_loss(a, b, users.to(dev), items.to(dev), lh.GAMMA)
    (0.37 * loss).backward()
    scaled = {k: 0.37 * v for k, v in r64.items()}
    for k, t in (("g_u", a), ("g_i", b)):
        within("upstream 0.37, " + k, t.grad.cpu().numpy(), scaled[k], rel_dev(r32[k], r64[k]), ULP24)
    with torch.no_grad():                                     # no gradient wanted: the same loss, no row gradients kept
        l2, p2 = ops.lightgode_loss(a, b, users.to(dev), items.to(dev), lh.GAMMA)
    assert torch.equal(l2, loss.detach()) and not l2.requires_grad
    for off in (0, 300):                                      # a joined table needs users and items on either side of the offset
        with pytest.raises(ValueError, match="item_offset"):
            ops.lightgode_loss(a, None, users.to(dev), items.to(dev), lh.GAMMA, item_offset=off)


# ---- the fixture: Model.LightGODE against the reference's run -------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_model_reproduces_the_reference(dev, fused, monkeypatch):
    from chaorec_amd import ops
    g = fixture()
    monkeypatch.setattr(ops, "lightgode_loss_plain" if fused else "lightgode_loss", None)      # the other route may not be reached
    m = lh.new_model(g, dev, fused=fused).train()
    users, pos = torch.from_numpy(g["users"]), torch.from_numpy(g["pos"])
    loss = m.loss(users, pos, pos)
    loss.backward()
    assert m.use_mf is True and m.fused is fused
    failures, ratios = [], []
    within("loss", loss.detach(), g["loss64"], g["own_loss"], ULP24, failures=failures, ratios=ratios)
    within("g_u", m.user_embedding.weight.grad, g["g_u64"], g["own_g_u"], ULP24, failures=failures, ratios=ratios)
    within("g_i", m.item_embedding.weight.grad, g["g_i64"], g["own_g_i"], ULP24, failures=failures, ratios=ratios)
    _, parts = m.loss_parts(users.to(dev), (pos - lh.U).to(dev))
    for k, name in enumerate(lh.PARTS):
        within(name, parts[k], g[name + "64"], g["own_" + name], ULP24, failures=failures, ratios=ratios)
    print(f"fused={fused}: ratio {max(ratios):.3f}")
    assert not failures, failures


def test_other_widths_run_the_plain_lines(dev, monkeypatch):
    from chaorec_amd import ops
    monkeypatch.setattr(ops, "lightgode_loss", None)
    g = fixture()
    torch.manual_seed(5)
    m = lh.new_model(g, dev, dim_E=32).train()
    users, pos = torch.from_numpy(g["users"]), torch.from_numpy(g["pos"])
    loss = m.loss(users, pos, pos)
    loss.backward()
    W_u, W_i = m.user_embedding.weight.detach().cpu(), m.item_embedding.weight.detach().cpu()
    r32, r64 = (lh.reference_loss(W_u, W_i, g["users"], g["pos"] - lh.U, lh.GAMMA, dt) for dt in (torch.float32, torch.float64))
    got = dict(loss=loss.detach().cpu().numpy(), g_u=m.user_embedding.weight.grad.cpu().numpy(), g_i=m.item_embedding.weight.grad.cpu().numpy())
    check_node("dim_E=32", got, r32, r64, keys=("loss", "g_u", "g_i"))
    with pytest.raises(RuntimeError, match="chaorec_lightgode_check_shape failed"):
        ops.lightgode_check_shape(70, 32)


# ---- Euler and the ranking ------------------------------------------------------------------------------------------------------
def test_euler_tables_ranking_and_the_cache(dev):
    g = fixture()
    edges = g["edges"].astype(np.int64)
    m = lh.new_model(g, dev).eval()
    calls = []
    euler = m.euler
    m.euler = lambda x: calls.append(1) or euler(x)
    ranks = m.gene_ranklist(lh.TOPK)
    assert m.use_mf is False and len(calls) == 1 and ranks.shape == (lh.U, lh.TOPK) and ranks.dtype == torch.int64 and not ranks.is_cuda
    tab = torch.cat((m.restore_user_e, m.restore_item_e)).cpu().numpy()
    within("eval-mode tables", tab, g["sample64"], g["own_euler"], ULP24)
    s64 = lh.masked_scores(g["sample64"][:lh.U], g["sample64"][lh.U:], edges)
    s_got = lh.masked_scores(tab[:lh.U], tab[lh.U:], edges)
    atol = bound_of(g["own_scores"], ULP24) * float(np.abs(s64).max())
    ok, why = tie_aware_rank_equal(ranks.numpy(), lh.rank_values(s_got, ranks.numpy()), g["ranks64"], lh.rank_values(s64, g["ranks64"]),
                                   atol=atol)
    assert ok, why
    # a second list in eval mode reuses the tables; loss() clears them
    kept = m.restore_user_e
    again = m.gene_ranklist(lh.TOPK)
    assert len(calls) == 1 and m.restore_user_e is kept and torch.equal(again, ranks)
    users, pos = torch.from_numpy(g["users"]), torch.from_numpy(g["pos"])
    m.loss(users, pos, pos)                                    # (eval mode: the loss reads the Euler tables, one joined table)
    assert m.restore_user_e is None and m.restore_item_e is None and len(calls) == 2
    # train mode: the list comes from the raw tables
    m.train()
    ranks_mf = m.gene_ranklist(lh.TOPK).numpy()
    assert m.use_mf is True and len(calls) == 2
    assert torch.equal(m.restore_user_e, m.user_embedding.weight.detach()) and torch.equal(m.restore_item_e, m.item_embedding.weight.detach())
    r64 = lh.masked_scores(g["w_user"].astype(np.float64), g["w_item"].astype(np.float64), edges)
    r32 = lh.masked_scores(g["w_user"], g["w_item"], edges)
    want = np.argsort(-r64, axis=1, kind="stable")[:, :lh.TOPK] + lh.U
    ok, why = tie_aware_rank_equal(ranks_mf, lh.rank_values(r32, ranks_mf), want, lh.rank_values(r64, want),
                                   atol=bound_of(rel_dev(r32, r64), ULP24) * float(np.abs(r64).max()))
    assert ok, why
    assert not np.array_equal(ranks_mf, ranks.numpy())


def test_euler_backward_is_the_same_launch(dev):
    """A is symmetric: d/dx of sum(w * euler(x)) is euler applied to w."""
    from chaorec_amd import ops
    g = fixture()
    m = lh.new_model(g, dev)
    x = torch.cat((m.user_embedding.weight, m.item_embedding.weight)).detach().requires_grad_(True)
    w = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    (ops.lightgode_euler(m.norm_adj, x, lh.T) * w).sum().backward()
    assert torch.equal(x.grad, ops.lightgode_euler(m.norm_adj, w, lh.T))
    A = lh.dense_adj(g["edges"].astype(np.int64))
    within_measured("euler backward", x.grad.cpu().numpy(), lh.euler(A, w.cpu(), lh.T, torch.float32).numpy(), lh.euler(A, w.cpu(), lh.T).numpy(),
                    ULP24)


# ---- train_strategy = 'GODE' ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_gode_training_step(dev, fused, monkeypatch):
    from chaorec_amd import ops
    monkeypatch.setattr(ops, "lightgode_loss_plain" if fused else "lightgode_loss", None)      # the other route may not be reached
    g = fixture()
    m = lh.new_model(g, dev, fused=fused)
    m.train_strategy = "GODE"
    m.train()
    users, pos = torch.from_numpy(g["users"]), torch.from_numpy(g["pos"])
    loss = m.loss(users, pos, pos)
    loss.backward()
    assert m.use_mf is False
    A = lh.dense_adj(g["edges"].astype(np.int64))
    r32, r64 = (lh.gode_loss(g["w_user"], g["w_item"], A, g["users"], g["pos"] - lh.U, lh.GAMMA, lh.T, dt) for dt in (torch.float32, torch.float64))
    got = dict(loss=loss.detach().cpu().numpy(), g_u=m.user_embedding.weight.grad.cpu().numpy(), g_i=m.item_embedding.weight.grad.cpu().numpy())
    check_node(f"GODE, fused={fused}", got, r32, r64, keys=("loss", "g_u", "g_i"))


# ---- capture --------------------------------------------------------------------------------------------------------------------
def _trajectory(dev, captured, steps=3):
    from chaorec_amd.optim import FusedAdam, GraphedTrainStep
    g = fixture()
    m = lh.new_model(g, dev, fused=True).train()
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.01}])
    batch = tuple(torch.from_numpy(g[k]).to(dev) for k in ("users", "pos", "pos"))
    step = GraphedTrainStep(m, opt, example_batch=batch) if captured else None
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
    assert not captured or step.replays == steps
    return m, [float(x) for x in losses]


def test_captured_steps_equal_the_eager_ones(dev, monkeypatch):
    """Three FusedAdam steps, eager and replayed from the step optim.GraphedTrainStep captured: the same losses and tables, bit
    for bit (no host read, no float atomics in the step)."""
    from chaorec_amd import ops
    monkeypatch.setattr(ops, "lightgode_loss_plain", None)      # every step goes through the node
    (me, le), (mc, lc) = _trajectory(dev, False), _trajectory(dev, True)
    assert le == lc and all(np.isfinite(le)) and len(set(le)) == 3
    for (n, a), b in zip(me.state_dict().items(), mc.state_dict().values()):
        assert torch.equal(a, b), n
    g = fixture()
    assert not torch.equal(me.user_embedding.weight.cpu(), torch.from_numpy(g["w_user"]))
