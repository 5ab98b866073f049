"""DualVAE on the MI355X (csrc/dualvae.hip) against the float64 restatement (tests/dualvae_host.py) with GIVEN draws.

Bounds: 4 x the reference's own fp32-vs-fp64 deviation of the same quantity, stored in the fixture by
tests/golden/gen_dualvae.py (the reference's rounding noise; a formula error shows at 1e-3 and up).  Determinism, the
write-back winner, the item side's gradient under the user side's table write, the captured step and the no-[B, N] memory
bound are checked here too."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import dualvae_host as dh  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["small", "sports"]
_CACHE = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def within(x, ref, dev_ref, what, failures):
    accept.within(what, x, ref, dev_ref, 0.0, failures=failures)


def make_model(g, dev):
    from chaorec_amd.Model import DualVAE
    torch.manual_seed(int(g["seed"]))
    return DualVAE(g["U"], g["I"], g["edges"], dh.user_item_dict(g["edges"]), 64, dh.KL_WEIGHT, dh.SSL_REG, dev)


def host_weights(m):
    return [v.detach().cpu().numpy() for v in m.state_dict().values()]


def host_tables(m):
    return tuple(t.detach().cpu().numpy().copy() for t in (m.theta, m.beta, m.mu_theta, m.mu_beta))


def case(name, dev):
    """The fixture, the float64 step on the model's initial weights (computed once, left unchanged) and the given draws."""
    if name not in _CACHE:
        g = dh.load_fixture(GOLDEN, name)
        m = make_model(g, dev)
        draws = dh.replay_draws(g["draw_seed"], len(g["users"]))
        assert np.array_equal(dh.draw_sums(draws), g["draw_sums"]), "this torch draws other values than the generator's"
        ref = dh.step(host_weights(m), host_tables(m), dh.dense_matrix(g["edges"], g["U"], g["I"]), g["users"], g["pos"] - g["U"], *draws)
        _CACHE[name] = (g, draws, ref)
    return _CACHE[name]


def run_step(m, g, draws=None):
    m.train()
    m.zero_grad(set_to_none=True)
    kw = {} if draws is None else {"eps_item": torch.from_numpy(draws[0]), "eps_user": torch.from_numpy(draws[1])}
    loss = m.loss(torch.from_numpy(g["users"]), torch.from_numpy(g["pos"]), torch.from_numpy(g["pos"]), **kw)
    loss.backward()
    torch.cuda.synchronize()
    out = {s: {k: v.cpu().numpy() for k, v in m.last[s].items()} for s in ("item", "user")}
    out.update(loss=float(loss.detach()), grads=[p.grad.detach().cpu().numpy().copy() for p in m.parameters()], tables=host_tables(m))
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_step_with_given_draws_meets_fp64(dev, name):
    g, draws, ref = case(name, dev)
    out = run_step(make_model(g, dev), g, draws)
    failures = []
    within(out["loss"], ref["loss"], g["dev_loss"], f"{name} loss", failures)
    for s in ("item", "user"):
        for k in ("kl", "ll", "cl", "loss", "z", "nei"):
            within(out[s][k], ref[s][k], g[f"dev_{s}_{k}"], f"{name} {s} {k}", failures)
    for n, got, want, d in zip(dh.NAMES, out["grads"], ref["grads"], g["dev_grads"]):
        within(got, want, d, f"{name} grad {n}", failures)
    assert not failures, failures


def test_tables_after_one_loss_with_repeated_ids(dev):
    g, draws, ref = case("small", dev)
    out = run_step(make_model(g, dev), g, draws)
    ids, counts = np.unique(g["users"], return_counts=True)
    assert counts.max() >= 4 and np.unique(g["pos"], return_counts=True)[1].max() >= 2
    failures = []
    for k, n in enumerate(("theta", "beta", "mu_theta", "mu_beta")):
        within(out["tables"][k], ref["tables"][k], g[f"dev_tab_{n}"], f"table {n}", failures)
    # the highest batch position wins, bit for bit: the row IS that sample's z
    u = int(ids[np.argmax(counts)])
    last = int(np.nonzero(g["users"] == u)[0][-1])
    assert np.array_equal(out["tables"][0][u], out["user"]["z"][last]) and np.array_equal(out["tables"][2][u], out["user"]["mu"][last])
    assert not failures, failures


def test_item_side_gradients_do_not_see_the_user_sides_theta_write(dev):
    """user_preferences and the item encoder receive gradient from the item side only; it must be the same whether or not
    the user side has written theta[users] before backward() runs."""
    g, draws, ref = case("small", dev)
    full = run_step(make_model(g, dev), g, draws)
    m = make_model(g, dev)
    m.train()
    m.last = {}
    _, _, sums, kl, cl = m.forward(torch.from_numpy(g["pos"] - g["U"]), user=False, eps=torch.from_numpy(draws[0]), parts=True)
    m._loss(sums, kl, m.kl_weight, cl, m.ssl_reg)[0].backward()
    torch.cuda.synchronize()
    grads = dict(zip(dh.NAMES, full["grads"]))
    for n, p in m.named_parameters():
        if n == "user_preferences" or n.startswith(("item_encoder", "item_mu", "item_std")):
            assert np.array_equal(p.grad.cpu().numpy(), grads[n]), n


def _trajectory(g, dev, captured):
    from chaorec_amd.optim import FusedAdam, GraphedTrainStep
    m = make_model(g, dev)
    m.seed = 4321
    opt = FusedAdam([{"params": m.parameters(), "lr": float(g["traj_lr"])}])
    m.train()
    batches = [(torch.from_numpy(u).to(dev), torch.from_numpy(p).to(dev)) for u, p in zip(g["traj_users"], g["traj_pos"])]
    step = GraphedTrainStep(m, opt, example_batch=(batches[0][0], batches[0][1], batches[0][1])) if captured else None
    assert int(m._state[0]) == 0, "warm-up steps counted"
    losses = []
    for u, p in batches:
        if captured:
            losses.append(step(u, p, p).clone())
        else:
            opt.zero_grad()
            loss = m.loss(u, p, p)
            loss.backward()
            opt.step()
            losses.append(loss.detach().clone())
    torch.cuda.synchronize()
    return m, [float(x) for x in losses]


def test_trajectory_with_given_draws_meets_fp64(dev):
    from chaorec_amd.optim import FusedAdam
    g, _, _ = case("small", dev)
    m = make_model(g, dev)
    w, t = host_weights(m), host_tables(m)
    T, lr, seed0 = len(g["traj_users"]), float(g["traj_lr"]), int(g["traj_seed0"])
    batches = [(g["traj_users"][k], g["traj_pos"][k] - g["U"]) for k in range(T)]
    l64, w64, t64 = dh.adam_trajectory(w, t, dh.dense_matrix(g["edges"], g["U"], g["I"]), batches, seed0, lr)
    opt = FusedAdam([{"params": m.parameters(), "lr": lr}])
    m.train()
    losses = []
    for k in range(T):
        ei, eu = dh.replay_draws(seed0 + k, len(batches[k][0]))
        opt.zero_grad()
        loss = m.loss(torch.from_numpy(g["traj_users"][k]), torch.from_numpy(g["traj_pos"][k]), None, eps_item=torch.from_numpy(ei),
                      eps_user=torch.from_numpy(eu))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    failures = []
    within(losses, l64, g["traj_dev_losses"], "trajectory losses", failures)
    for n, got, want, d in zip(dh.NAMES, host_weights(m), w64, g["traj_dev_weights"]):
        within(got, want, d, f"trajectory {n}", failures)
    for n, got, want, d in zip(("theta", "beta", "mu_theta", "mu_beta"), host_tables(m), t64, g["traj_dev_tables"]):
        within(got, want, d, f"trajectory table {n}", failures)
    assert int(m._state[0]) == T
    assert not failures, failures


def test_captured_trajectory_equals_the_eager_one(dev):
    """Ten FusedAdam steps with device-drawn epsilon, eager and through GraphedTrainStep: the same losses, weights, counter
    and tables (the warm-up steps neither count nor leave their rows behind)."""
    g, _, _ = case("small", dev)
    (me, le), (mc, lc) = _trajectory(g, dev, False), _trajectory(g, dev, True)
    assert le == lc and all(np.isfinite(le))
    assert torch.equal(me._state.cpu(), mc._state.cpu()) and int(me._state[0]) == len(le)
    for a, b in zip(host_tables(me), host_tables(mc)):
        assert np.array_equal(a, b)
    for a, b in zip(host_weights(me), host_weights(mc)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", FIXTURES)
def test_two_runs_with_device_drawn_epsilon_give_the_same_bits(dev, name):
    g, _, _ = case(name, dev)
    runs = []
    for _ in range(2):
        m = make_model(g, dev)
        m.seed = 99
        runs.append(run_step(m, g))
    a, b = runs
    assert a["loss"] == b["loss"] and np.isfinite(a["loss"])
    for x, y in zip(a["grads"] + list(a["tables"]), b["grads"] + list(b["tables"])):
        assert np.array_equal(x, y)
    m.seed = 100                                  # another seed, other draws
    m._state.zero_()
    assert not np.array_equal(run_step(m, g)["user"]["z"], a["user"]["z"])


@pytest.mark.parametrize("name", FIXTURES)
def test_ranklist_meets_the_cap(dev, name):
    g, _, _ = case(name, dev)
    m = make_model(g, dev)
    U, I, topk, users = g["U"], g["I"], g["topk"], g["rank_users"]
    hist = dh.user_item_dict(g["edges"])
    for tag, scale in (("s01", 0.1), ("s10", 1.0)):
        gen = torch.Generator().manual_seed(77)
        m.mu_theta = (torch.randn(U, dh.A, dh.K, generator=gen) * scale).to(dev)
        m.mu_beta = (torch.randn(I, dh.A, dh.K, generator=gen) * scale).to(dev)
        ranks = m.gene_ranklist(topk)
        assert ranks.dtype == torch.int64 and ranks.shape == (U, topk) and not ranks.is_cuda
        sc = dh.scores(host_weights(m), m.mu_theta.cpu().numpy(), m.mu_beta.cpu().numpy(), users)
        share, bad = dh.ranklist_check(ranks.numpy()[users], sc, hist, users, topk, U)
        agree = float((ranks.numpy()[users] - U == g[f"rank_{tag}"]).mean())
        print(f"{name} {tag}: {share:.4%} of the positions differ from the fp64 list (reference's own "
              f"{float(g[f'rank_share_{tag}']):.4%}), {bad} outside the gap; {agree:.4%} equal the reference's list")
        assert share <= 0.02 and bad == 0
        assert torch.equal(torch.softmax((m.mu_beta * m.item_topics).sum(-1), 1), m.aspect_probability)


def test_several_user_ranges_equal_one_range(dev, monkeypatch):
    """A staging cap of 7 rows: 42 ranges of 7 users (user_begin = 7, 14, ...) and a short last one of 6, against the one
    range the small fixture otherwise fits -- the same list for ALL users."""
    from chaorec_amd import ops_vae
    g, _, _ = case("small", dev)
    m = make_model(g, dev)
    U, I, topk = g["U"], g["I"], g["topk"]
    gen = torch.Generator().manual_seed(78)
    m.mu_theta = torch.randn(U, dh.A, dh.K, generator=gen).to(dev)
    m.mu_beta = torch.randn(I, dh.A, dh.K, generator=gen).to(dev)
    assert ops_vae.dualvae_range_users(I) >= U
    one = m.gene_ranklist(topk)
    monkeypatch.setattr(ops_vae, "DUALVAE_STAGING_BYTES", 7 * 4 * I)
    assert ops_vae.dualvae_range_users(I) == 7 and U % 7 == 6
    many = m.gene_ranklist(topk)
    assert many.dtype == torch.int64 and tuple(many.shape) == (U, topk)
    differ = (many != one).any(1).nonzero().flatten().tolist()
    assert not differ, f"users {differ[:10]} ... rank differently in ranges of 7"


def test_no_batch_by_table_buffer(dev):
    """U = I = 131 072, B = 2 048: one [B, I] fp32 matrix is 1 GiB.  Parameters, Adam state and gradients exist BEFORE the
    measured step."""
    from chaorec_amd.Model import DualVAE
    from chaorec_amd.optim import FusedAdam
    U = I = 131072
    B = 2048
    rng = np.random.default_rng(0)
    edges = np.stack([np.repeat(np.arange(U), 8), U + rng.integers(0, I, U * 8)], 1)
    torch.manual_seed(0)
    m = DualVAE(U, I, edges, {}, 64, dh.KL_WEIGHT, dh.SSL_REG, dev)
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.001}])
    pick = rng.choice(len(edges), size=B, replace=False)
    users, pos = torch.from_numpy(edges[pick, 0]).to(dev), torch.from_numpy(edges[pick, 1]).to(dev)
    m.train()

    def one():
        opt.zero_grad(set_to_none=False)
        loss = m.loss(users, pos, pos)
        loss.backward()
        opt.step()
        return loss

    one()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = one()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"step adds {extra / 2 ** 20:.1f} MiB at peak; one [B, I] matrix is {B * I * 4 / 2 ** 20:.0f} MiB")
    assert np.isfinite(float(loss.detach())) and extra < B * I * 4
