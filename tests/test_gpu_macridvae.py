"""MacridVAE on the MI355X (csrc/macridvae.hip) against the float64 restatement (tests/macridvae_host.py) with GIVEN draws.

Bound per quantity = 4 x the deviation of the REFERENCE's fp32 from the same fp64 values, as stored in the fixtures
(tests/golden/gen_macridvae.py).  Determinism, the no-[B, I] memory bound, fresh draws under replay, the increment-first
counter and the ranking cap are conditions, not measurements."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import macridvae_host as mh  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def within(x, ref, dev_ref, what, failures=None):
    """Prints the figure, then asserts -- or, with `failures`, notes the miss so that a test shows ALL its figures first."""
    accept.within(what, x, ref, dev_ref, 0.0, failures=failures)


def make_model(g, dev):
    from chaorec_amd.Model import MacridVAE
    torch.manual_seed(int(g["seed"]))
    return MacridVAE(g["U"], g["I"], g["edges"], mh.user_item_dict(g["edges"]), g["D"], 0.0, dev)


def host_weights(m):
    return tuple(v.detach().cpu().numpy() for v in m.state_dict().values())


def given(draws):
    return {"keep": torch.from_numpy(draws[0]), "gumbel": torch.from_numpy(draws[1]), "eps": torch.from_numpy(draws[2])}


def run_step(m, users, draws, update_before):
    m.train()
    m.zero_grad(set_to_none=True)
    m.update = update_before
    loss = m.loss(torch.from_numpy(np.asarray(users)), **given(draws))
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": float(loss.detach()), "ce": float(m.last["ce"]), "kl": float(m.last["kl"]), "anneal": float(m.last["anneal"]),
            "lse": m.last["lse"].cpu().numpy(), "z": m.last["z"].cpu().numpy(), "cates": m.last["cates"].cpu().numpy(),
            "grads": tuple(p.grad.detach().cpu().numpy() for p in m.parameters())}


@pytest.mark.parametrize("name", ["small", "sports"])
def test_step_with_given_draws_meets_fp64(dev, name):
    g = mh.load_fixture(GOLDEN, name)
    m = make_model(g, dev)
    w = host_weights(m)
    draws = mh.case_draws(g, int(g["draw_seed"]), g["users"])
    assert mh.draws_match(draws, g["draw_sums"]), "this torch draws other values than the generator's"
    failures = []
    for tag, upd in (("", 0), ("a_", 123456)):
        ref = mh.step(w, g["rowptr"], g["col"], g["users"], *draws, upd)
        out = run_step(m, g["users"], draws, upd)
        assert out["anneal"] == np.float32(ref["anneal"]) and m.update == upd + 1
        for k in ("loss", "ce", "kl", "lse", "z", "cates"):
            within(out[k], ref[k], g[f"{tag}dev_{k}"], f"{name} {tag}{k}", failures)
        for n, got, want, d in zip(mh.NAMES, out["grads"], ref["grads"], g[f"{tag}dev_grads"]):
            within(got, want, d, f"{name} {tag}grad {n}", failures)
    assert not failures, failures


def test_update_is_incremented_before_the_anneal_is_read(dev):
    g = mh.load_fixture(GOLDEN, "small")
    m = make_model(g, dev)
    m.train()
    assert m.update == 0
    m.loss(torch.from_numpy(g["users"]))
    assert m.update == 1 and float(m.last["anneal"]) == np.float32(1 / 200000)


def test_trajectory_with_given_draws_meets_fp64(dev):
    from chaorec_amd.optim import FusedAdam
    g = mh.load_fixture(GOLDEN, "small")
    m = make_model(g, dev)
    w = host_weights(m)
    u0, lr, T = int(g["traj_update"]), float(g["traj_lr"]), len(g["traj_batches"])
    draws = [mh.case_draws(g, int(g["traj_seed0"]) + t, g["traj_batches"][t]) for t in range(T)]
    l64, w64 = mh.adam_trajectory(w, g["rowptr"], g["col"], list(g["traj_batches"]), [d[0] for d in draws], [d[1] for d in draws],
                                  [d[2] for d in draws], u0, lr)
    opt = FusedAdam([{"params": m.parameters(), "lr": lr}])
    m.train()
    m.update = u0
    losses = []
    for t in range(T):
        opt.zero_grad()
        loss = m.loss(torch.from_numpy(g["traj_batches"][t]), **given(draws[t]))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert m.update == u0 + T
    failures = []
    within(losses, l64, g["traj_dev_losses"], "trajectory losses", failures)
    for n, got, want, d in zip(mh.NAMES, host_weights(m), w64, g["traj_dev_weights"]):
        within(got, want, d, f"trajectory {n}", failures)
    assert not failures, failures


def _one_step_state(g, dev, captured):
    from chaorec_amd.optim import FusedAdam, GraphedTrainStep
    m = make_model(g, dev)
    m.seed = 1234
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.01}])
    users = torch.from_numpy(g["users"]).to(dev)
    m.train()
    if captured:
        step = GraphedTrainStep(m, opt, example_batch=(users, users, users))
        loss = step(users, users, users).clone()
    else:
        opt.zero_grad()
        loss = m.loss(users, users, users)
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    ps = list(m.parameters())
    return [loss.detach().cpu()] + [p.grad.detach().cpu().clone() for p in ps] + [p.detach().cpu().clone() for p in ps]


@pytest.mark.parametrize("captured", [False, True])
def test_two_runs_give_the_same_bits(dev, captured):
    g = mh.load_fixture(GOLDEN, "small")
    a, b = _one_step_state(g, dev, captured), _one_step_state(g, dev, captured)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_captured_step_equals_eager_step(dev):
    g = mh.load_fixture(GOLDEN, "small")
    for x, y in zip(_one_step_state(g, dev, False), _one_step_state(g, dev, True)):
        assert torch.equal(x, y)


def test_replays_draw_fresh_values_and_advance_the_counter(dev):
    from chaorec_amd.optim import FusedAdam, GraphedTrainStep
    g = mh.load_fixture(GOLDEN, "small")
    m = make_model(g, dev)
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.0}])      # (lr 0: the weights stay, only the draws can move anything)
    users = torch.from_numpy(g["users"]).to(dev)
    m.train()
    m.update = 7
    step = GraphedTrainStep(m, opt, example_batch=(users, users, users))
    assert m.update == 7, "warm-up steps counted"
    step(users, users, users)
    z1, e1, c1 = m.last["z"].clone(), m.last["eps"].clone(), m.last["cates"].clone()
    step(users, users, users)
    z2, e2, c2 = m.last["z"].clone(), m.last["eps"].clone(), m.last["cates"].clone()
    torch.cuda.synchronize()
    assert m.update == 9
    assert not torch.equal(e1, e2) and not torch.equal(z1, z2) and not torch.equal(c1, c2)
    assert abs(float(e1.mean())) < 0.0005 and abs(float(e1.std()) - 0.01) < 0.0005      # N(0, 0.01^2) draws
    # dropout is fresh too: with the Gumbel noise and eps GIVEN, two eager steps differ only through the keep flags
    d = mh.case_draws(g, int(g["draw_seed"]), g["users"])
    m.loss(users, gumbel=torch.from_numpy(d[1]), eps=torch.from_numpy(d[2]))
    za = m.last["z"].clone()
    m.loss(users, gumbel=torch.from_numpy(d[1]), eps=torch.from_numpy(d[2]))
    assert not torch.equal(za, m.last["z"])


def test_no_batch_by_items_buffer(dev):
    """I = 262 144, B = 2 048: one [B, I] fp32 matrix would be 2.0 GiB.  Parameters, Adam state and gradients exist BEFORE
    the measured step; the step itself may add O(B K 600 + splits B K 64)."""
    from chaorec_amd.Model import MacridVAE
    from chaorec_amd.optim import FusedAdam
    U, I, B = 4096, 262144, 2048
    rng = np.random.default_rng(0)
    edges = np.stack([np.repeat(np.arange(U), 8), U + rng.integers(0, I, U * 8)], 1)
    torch.manual_seed(0)
    m = MacridVAE(U, I, edges, mh.user_item_dict(edges), 64, 0.0, dev)
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.01}])
    users = torch.from_numpy(rng.integers(0, U, B)).to(dev)
    m.train()

    def one():
        opt.zero_grad(set_to_none=False)
        loss = m.loss(users, users, users)
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
    assert np.isfinite(float(loss)) and extra < B * I * 4


@pytest.mark.parametrize("name", ["small", "sports"])
def test_ranklist_meets_the_cap(dev, name):
    g = mh.load_fixture(GOLDEN, name)
    m = make_model(g, dev)
    w = host_weights(m)
    U, I, topk = g["U"], g["I"], int(g["topk"])
    m.train()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ranks = m.gene_ranklist(topk)
    extra = torch.cuda.max_memory_allocated() - before
    assert m.training is False, "gene_ranklist leaves training False"
    m.train()
    assert m.training is True
    assert ranks.dtype == torch.int64 and ranks.shape == (U, topk) and not ranks.is_cuda
    if name == "sports":
        print(f"ranking adds {extra / 2 ** 20:.0f} MiB at peak; [U, I] fp32 is {U * I * 4 / 2 ** 20:.0f} MiB")
        assert extra < U * I * 4
    users = g["rank_users"]
    local = ranks.numpy()[users] - U
    hist = (m.hist[0].cpu().numpy(), m.hist[1].cpu().numpy())
    share, bad = mh.ranklist_check(local, w, g["rowptr"], g["col"], hist[0], hist[1], users, topk)
    print(f"{name}: {share:.4%} of the positions differ from the fp64 list (reference's own: {float(g['rank_ref_share']):.4%}), {bad} outside the gap")
    assert share <= 0.02 and bad == 0
    # masked history items appear wherever 1e-6 beats the K-th unmasked score, as in the reference's list
    in_hist = sum(int(np.isin(local[r], hist[1][hist[0][u]:hist[0][u + 1]]).sum()) for r, u in enumerate(users))
    ref_hist = sum(int(np.isin(g["ranks"][r], hist[1][hist[0][u]:hist[0][u + 1]]).sum()) for r, u in enumerate(users))
    assert (in_hist > 0) == (ref_hist > 0) and abs(in_hist - ref_hist) <= 0.02 * local.size      # (the same cap: a borderline row may swap)
    again = m.gene_ranklist(topk, to_cpu=False)
    assert again.is_cuda and torch.equal(again.cpu(), ranks)


def test_several_user_ranges_equal_one_range(dev, monkeypatch):
    """A staging cap of 7 rows: 42 ranges of 7 users (user_begin = 7, 14, ...) and a short last one of 6, against the one
    range the small fixture otherwise fits -- the same list for ALL users."""
    from chaorec_amd import ops_vae
    g = mh.load_fixture(GOLDEN, "small")
    m = make_model(g, dev)
    U, I, topk = g["U"], g["I"], int(g["topk"])
    assert ops_vae.macrid_range_users(I) >= U
    one = m.gene_ranklist(topk)
    monkeypatch.setattr(ops_vae, "MACRID_STAGING_BYTES", 7 * 4 * I)
    assert ops_vae.macrid_range_users(I) == 7 and U % 7 == 6
    many = m.gene_ranklist(topk)
    assert many.dtype == torch.int64 and tuple(many.shape) == (U, topk)
    differ = (many != one).any(1).nonzero().flatten().tolist()
    assert not differ, f"users {differ[:10]} ... rank differently in ranges of 7"


def test_topk_kernel_is_exact_with_ties_to_the_lowest_index(dev):
    from chaorec_amd import ops
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(37, 1000, generator=gen)
    x[:, ::7] = 1e-6                       # many equal values
    x[5] = 0.25                            # a whole row of ties
    x[6, :10] = float("-inf")
    for k in (1, 50, 64):
        idx, val = ops.macrid_topk(x.to(dev), k, id_offset=11)
        order = torch.argsort(-x, dim=1, stable=True)[:, :k]
        assert torch.equal(idx.cpu() - 11, order) and torch.equal(val.cpu(), torch.gather(x, 1, order))


@pytest.mark.parametrize("extra", [[], ["--no_graph"]])
def test_main_runs_macridvae_on_sports(dev, tmp_path, extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    proc = subprocess.run([sys.executable, "-m", "chaorec_amd.main", "--Model", "MacridVAE", "--data_path", "sports", "--num_epoch", "2",
                           "--data_root", str(tmp_path / "Data")] + extra, cwd=tmp_path, env=env, capture_output=True, text=True,
                          timeout=1500)
    assert proc.returncode == 0, proc.stderr[-3000:]
    log = proc.stdout + proc.stderr
    losses = [float(x) for x in re.findall(r"Epoch \d+, Loss: ([-\w.]+)", log)]
    recalls = [float(x) for x in re.findall(r"20: .*?recall: ([\d.]+)", log)]
    print("epoch losses", losses, "recall@20 lines", recalls[-4:])
    assert len(losses) == 2 and all(np.isfinite(losses)) and recalls and all(np.isfinite(recalls))
    assert "Best performance:" in log
