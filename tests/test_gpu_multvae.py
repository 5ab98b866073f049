"""MultVAE on the MI355X (csrc/multvae.hip) against the float64 restatement (tests/multvae_host.py) with GIVEN draws.

Bound per quantity = 4 x the deviation of the REFERENCE's fp32 from the same fp64 values, as stored in the fixtures
(tests/golden/gen_multvae.py): the reference's own rounding noise is the floor, a formula error sits orders of
magnitude outside.  Determinism, the no-[B, I] memory bound, fresh draws under replay and the ranking cap are
conditions, not measurements."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import multvae_host as mh  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("layers_q.0.weight", "layers_q.0.bias", "layers_p.0.weight", "layers_p.0.bias")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def within(x, ref, dev_ref, what):
    accept.within(what, x, ref, dev_ref, 0.0)


def make_model(g, dev):
    from chaorec_amd.Model import MultVAE
    torch.manual_seed(int(g["seed"]))
    return MultVAE(g["U"], g["I"], g["edges"], mh.user_item_dict(g["edges"]), 64, float(g["reg_weight"]), dev)


def params(m):
    return (m.layers_q[0].weight, m.layers_q[0].bias, m.layers_p[0].weight, m.layers_p[0].bias)


def host_weights(m):
    return tuple(p.detach().cpu().numpy() for p in params(m))


def run_step(m, users, keep, eps, update_count):
    m.train()
    m.zero_grad(set_to_none=True)
    m.update_count = update_count
    loss = m.loss(torch.from_numpy(np.asarray(users)), keep=torch.from_numpy(np.asarray(keep)), eps=torch.from_numpy(np.asarray(eps)))
    loss.backward()
    torch.cuda.synchronize()
    return {"loss": float(loss.detach()), "neg_ll": float(m.last["neg_ll"]), "kl": float(m.last["kl"]),
            "anneal": float(m.last["anneal"]), "lse": m.last["lse"].cpu().numpy(), "z": m.last["z"].cpu().numpy(),
            "grads": tuple(p.grad.detach().cpu().numpy() for p in params(m))}


def case_draws(g):
    if "eps" in g:
        return g["keep"], g["eps"]
    mask, eps = mh.replay_draws(g["draw_seed"], len(g["users"]), g["I"])
    assert abs(float(eps.astype(np.float64).sum()) - float(g["eps_sum"])) < 1e-9, "this torch draws another eps than the generator's"
    return g["keep"], eps


@pytest.mark.parametrize("name", ["small", "sports"])
def test_step_with_given_draws_meets_fp64(dev, name):
    g = mh.load_fixture(GOLDEN, name)
    m = make_model(g, dev)
    w = host_weights(m)
    keep, eps = case_draws(g)
    reg = float(g["reg_weight"])
    for tag, uc in (("", 0), ("a_", 123456)):
        ref = mh.step(w, g["rowptr"], g["col"], g["users"], keep, eps, uc, reg)
        out = run_step(m, g["users"], keep, eps, uc)
        assert out["anneal"] == np.float32(ref["anneal"]) and m.update_count == uc + 1
        for k in ("loss", "neg_ll", "kl"):
            within(out[k], ref[k], g[f"{tag}dev_{k}"], f"{name} {tag}{k}")
        within(out["lse"], ref["lse"], g["dev_lse"], f"{name} {tag}lse")
        within(out["z"], ref["z"], g["dev_z"], f"{name} {tag}z")
        for n, got, want, d in zip(NAMES, out["grads"], ref["grads"], g[f"{tag}dev_grads"]):
            within(got, want, d, f"{name} {tag}grad {n}")
    # an item no sample touched: the decoder row is P^T z + 2 reg^2 w alone, the encoder row 2 reg^2 w EXACTLY
    touched = np.zeros(g["I"], dtype=bool)
    for u in g["users"]:
        touched[g["col"][g["rowptr"][u]:g["rowptr"][u + 1]]] = True
    i = int(np.nonzero(~touched)[0][0])
    two_r2 = np.float32(2.0) * np.float32(reg * (reg * 0.5) * 2)          # d loss / d sum||p||^2 = reg^2, times 2 w
    np.testing.assert_allclose(out["grads"][0][:, i], two_r2 * w[0][:, i], rtol=3e-7)
    P_col = (np.diff(g["rowptr"])[g["users"]] / len(g["users"])) * np.exp(ref["z"] @ w[2][i].astype(np.float64) + float(w[3][i]) - ref["lse"])
    want = P_col @ ref["z"] + 2 * reg * reg * w[2][i].astype(np.float64)
    assert np.abs(out["grads"][2][i] - want).max() <= accept.bound_of(g["a_dev_grads"][2], 0.0) * np.abs(ref["grads"][2]).max()


def test_trajectory_with_given_draws_meets_fp64(dev):
    from chaorec_amd.optim import FusedAdam
    g = mh.load_fixture(GOLDEN, "small")
    m = make_model(g, dev)
    w = host_weights(m)
    uc0, lr, reg = int(g["traj_update_count"]), float(g["traj_lr"]), float(g["reg_weight"])
    l64, w64 = mh.adam_trajectory(w, g["rowptr"], g["col"], list(g["traj_batches"]), g["traj_keeps"], list(g["traj_eps"]), uc0, reg, lr)
    opt = FusedAdam([{"params": m.parameters(), "lr": lr}])
    m.train()
    m.update_count = uc0
    losses = []
    for t in range(len(l64)):
        opt.zero_grad()
        loss = m.loss(torch.from_numpy(g["traj_batches"][t]), keep=torch.from_numpy(g["traj_keeps"][t]), eps=torch.from_numpy(g["traj_eps"][t]))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert m.update_count == uc0 + len(l64)
    within(losses, l64, g["traj_dev_losses"], "trajectory losses")
    for n, got, want, d in zip(NAMES, host_weights(m), w64, g["traj_dev_weights"]):
        within(got, want, d, f"trajectory {n}")


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
    return [loss.detach().cpu()] + [p.grad.detach().cpu().clone() for p in params(m)] + [p.detach().cpu().clone() for p in params(m)]


@pytest.mark.parametrize("captured", [False, True])
def test_two_runs_give_the_same_bits(dev, captured):
    g = mh.load_fixture(GOLDEN, "small")
    a, b = _one_step_state(g, dev, captured), _one_step_state(g, dev, captured)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_captured_step_equals_eager_step(dev):
    """Same seed, same counter: the captured step draws what the eager one draws (warm-up steps do not count)."""
    g = mh.load_fixture(GOLDEN, "small")
    for x, y in zip(_one_step_state(g, dev, False), _one_step_state(g, dev, True)):
        assert torch.equal(x, y)


def test_replays_draw_fresh_values_and_advance_the_counter(dev):
    from chaorec_amd.optim import FusedAdam, GraphedTrainStep
    g = mh.load_fixture(GOLDEN, "small")
    m = make_model(g, dev)
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.0}])      # (lr 0: the weights stay, only the draws can move z)
    users = torch.from_numpy(g["users"]).to(dev)
    m.train()
    m.update_count = 7
    step = GraphedTrainStep(m, opt, example_batch=(users, users, users))
    assert m.update_count == 7, "warm-up steps counted"
    step(users, users, users)
    z1, e1 = m.last["z"].clone(), m.last["eps"].clone()
    step(users, users, users)
    z2, e2 = m.last["z"].clone(), m.last["eps"].clone()
    torch.cuda.synchronize()
    assert m.update_count == 9
    assert not torch.equal(e1, e2) and not torch.equal(z1, z2)
    assert abs(float(e1.mean())) < 0.05 and abs(float(e1.std()) - 1.0) < 0.05      # N(0, 1) draws


def test_no_batch_by_items_buffer(dev):
    """I = 262 144, B = 2 048: one [B, I] fp32 matrix would be 2.0 GiB.  Parameters, Adam state and gradients
    (6 x I x 193 x 4 B = 1.2 GB) exist BEFORE the measured step; the step itself may add O(B * 128 + splits * B * 64)."""
    from chaorec_amd.Model import MultVAE
    from chaorec_amd.optim import FusedAdam
    U, I, B = 4096, 262144, 2048
    rng = np.random.default_rng(0)
    edges = np.stack([np.repeat(np.arange(U), 8), U + rng.integers(0, I, U * 8)], 1)
    torch.manual_seed(0)
    m = MultVAE(U, I, edges, mh.user_item_dict(edges), 64, 0.01, dev)
    opt = FusedAdam([{"params": m.parameters(), "lr": 0.01}])
    users = torch.from_numpy(rng.integers(0, U, B)).to(dev)
    m.train()

    def one():
        opt.zero_grad(set_to_none=False)
        loss = m.loss(users, users, users)
        loss.backward()
        opt.step()
        return loss

    one()                                     # gradients and Adam moments now exist
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = one()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"step adds {extra / 2 ** 20:.1f} MiB at peak; one [B, I] matrix is {B * I * 4 / 2 ** 20:.0f} MiB")
    assert np.isfinite(float(loss)) and extra < B * I * 4


@pytest.mark.parametrize("name", ["small", "sports"])
def test_ranklist_with_given_eps_meets_the_cap(dev, name):
    g = mh.load_fixture(GOLDEN, name)
    m = make_model(g, dev)
    w = host_weights(m)
    if "eps_rank" in g:
        eps = g["eps_rank"]
    else:
        torch.manual_seed(int(g["rank_seed"]))
        eps = torch.randn(g["U"], mh.LATENT).numpy()
        assert abs(float(eps.astype(np.float64).sum()) - float(g["eps_rank_sum"])) < 1e-9
    m.eval()
    ranks = m.gene_ranklist(int(g["topk"]), eps=torch.from_numpy(eps)).numpy() - g["U"]
    assert ranks.shape == (g["U"], int(g["topk"])) and m.result.shape == (g["U"] + g["I"], 128)
    z = mh.latent_all(w, g["rowptr"], g["col"], g["U"], eps)
    share, bad = mh.ranklist_check(ranks, w, z, g["rowptr"], g["col"], int(g["topk"]))
    print(f"{name}: {share:.4%} of the positions differ from the fp64 list (reference's own: {float(g['rank_ref_share']):.4%}), {bad} outside the gap")
    assert share <= 0.02 and bad == 0
    # device-side hand-over (train_and_evaluate's on-device metrics) and a stochastic second call
    again = m.gene_ranklist(int(g["topk"]), to_cpu=False)
    assert again.is_cuda and again.shape == ranks.shape


@pytest.mark.parametrize("extra", [[], ["--no_graph"]])
def test_main_runs_multvae_on_sports(dev, tmp_path, extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    proc = subprocess.run([sys.executable, "-m", "chaorec_amd.main", "--Model", "MultVAE", "--data_path", "sports", "--num_epoch", "2",
                           "--data_root", str(tmp_path / "Data")] + extra, cwd=tmp_path, env=env, capture_output=True, text=True,
                          timeout=1500)
    assert proc.returncode == 0, proc.stderr[-3000:]
    log = proc.stdout + proc.stderr
    losses = [float(x) for x in re.findall(r"Epoch \d+, Loss: ([-\w.]+)", log)]
    recalls = re.findall(r"20: .*?recall: ([\d.]+)", log)
    print("epoch losses", losses, "recall@20 lines", recalls[-4:])
    assert len(losses) == 4 and all(np.isfinite(losses))                  # (two YAML combinations x two epochs)
    assert losses[1] < losses[0] and losses[3] < losses[2]
    assert "Best performance:" in log and recalls
