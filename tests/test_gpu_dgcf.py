"""DGCF on the MI355X (csrc/dgcf.hip, Model/DGCF.py): the reference goldens (tests/golden/gen_dgcf.py), the kernels against
the float64 restatement of tests/test_dgcf_host.py on the real sports graph, reproducibility, the captured epoch, the shape
limits and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, load_interactions
from test_dgcf_host import distance_correlation, edge_operator, intent_propagate, routing_scores

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chaorec_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _small_model(z, K, T, dev):
    from chaorec_amd import graph
    from chaorec_amd.Model import DGCF
    U, I, e = int(z["U"]), int(z["I"]), z["edges"]
    torch.manual_seed(0)
    return DGCF(U, I, e, graph.user_item_dict_from_edges(e), int(z["D"]), float(z["reg"]), float(z["corDecay"]), K, T,
                int(z["L"]), "add", dev).to(dev)


def _batch(z, dev):
    return [torch.as_tensor(z[k]).long().to(dev) for k in ("users", "pos", "neg")]


@pytest.mark.parametrize("K,T", [(1, 1), (2, 2), (4, 1), (4, 3)])
def test_golden_one_step(dev, K, T):
    z = load_golden("dgcf_small.npz")
    c = lambda k: z[f"k{K}t{T}_{k}"]  # noqa: E731
    m = _small_model(z, K, T, dev)
    assert [n for n, _ in m.named_parameters()] == ["user_intent_embeddings.weight", "item_intent_embeddings.weight"]
    assert "S" not in dict(m.state_dict()) and "_S" not in dict(m.state_dict())
    assert np.array_equal(m.user_intent_embeddings.weight.detach().cpu().numpy(), c("p_user"))
    assert np.array_equal(m.item_intent_embeddings.weight.detach().cpu().numpy(), c("p_item"))
    assert torch.equal(m.S.cpu(), torch.ones(K, z["edges"].shape[0]))
    loss = m.loss(*_batch(z, dev))
    assert tuple(loss.shape) == tuple(c("loss_shape"))
    loss.backward()
    assert abs(float(loss.item()) - float(c("loss"))) < 1e-5
    np.testing.assert_allclose(m.result.detach().cpu().numpy(), c("result"), rtol=0, atol=1e-5)
    assert tuple(m.S.shape) == (K, z["edges"].shape[0])
    np.testing.assert_allclose(m.S.cpu().numpy(), c("S"), rtol=0, atol=1e-5)
    for name, key in (("user_intent_embeddings.weight", "g_user"), ("item_intent_embeddings.weight", "g_item")):
        g = dict(m.named_parameters())[name].grad.cpu().numpy()
        np.testing.assert_allclose(g, c(key), rtol=0, atol=2e-4 * (np.abs(c(key)).max() + 1e-12) + 1e-7)
    rank = m.gene_ranklist(topk=int(z["topk"]))
    assert rank.shape == c("rank").shape
    assert (np.asarray(rank) == c("rank")).mean() > 0.98


@pytest.mark.parametrize("K,T", [(2, 2), (4, 3)])
def test_golden_trajectory(dev, K, T):
    """Three fixed-batch Adam steps: S persists across forwards (loss and S after every step)."""
    from chaorec_amd.optim import FusedAdam
    z = load_golden("dgcf_small.npz")
    c = lambda k: z[f"k{K}t{T}_{k}"]  # noqa: E731
    m = _small_model(z, K, T, dev)
    opt = FusedAdam([{"params": m.parameters(), "lr": float(z["lr"])}])
    b = _batch(z, dev)
    for s in range(3):
        opt.zero_grad()
        loss = m.loss(*b)
        loss.backward()
        opt.step()
        assert abs(float(loss.item()) - float(c("traj_loss")[s])) < 1e-4, s
        np.testing.assert_allclose(m.S.cpu().numpy(), c("traj_S")[s], rtol=0, atol=2e-4)
    np.testing.assert_allclose(m.user_intent_embeddings.weight.detach().cpu().numpy(), c("traj_user"), rtol=0, atol=1e-4)


def test_one_factor_is_the_layer_sum_of_plain_propagates(dev):
    """K = 1: softmax of one intent is 1, every propagate is the LightGCN operator, result = x0 + A x0 + A^2 x0 + ... (a
    SUM, not a mean) and the correlation term is exactly 0."""
    from chaorec_amd import graph, ops
    z = load_golden("dgcf_small.npz")
    m = _small_model(z, 1, 2, dev)
    b = _batch(z, dev)
    m.loss(*b)
    x = torch.cat([m.user_intent_embeddings.weight, m.item_intent_embeddings.weight]).detach()
    A = graph.lightgcn_csr(z["edges"], int(z["U"]) + int(z["I"])).to(dev)
    ref, y = x.clone(), x
    for _ in range(int(z["L"])):
        y = ops.spmm(A, y)
        ref = ref + y
    torch.testing.assert_close(m.result.detach(), ref, rtol=0, atol=1e-6)
    assert float(m.cor_loss(b[0], b[1] - int(z["U"])).item()) == 0.0


@pytest.fixture(scope="module")
def sports(dev):
    from chaorec_amd import graph
    d = load_interactions("sports")
    U, I, e = d["U"], d["I"], d["train"]
    g = graph.dgcf_structure(e, U, U + I).to(dev)
    return U, I, e, g


@pytest.mark.parametrize("D,K", [(64, 4), (128, 2), (32, 8)])
def test_propagate_and_routing_against_fp64(dev, sports, D, K):
    from chaorec_amd import ops
    U, I, e, g = sports
    N, E = U + I, e.shape[0]
    gen = torch.Generator().manual_seed(D + K)
    x = (torch.randn(N, D, generator=gen) * 0.1).float()
    S = (torch.randn(E, K, generator=gen)).float()
    P = torch.softmax(S, dim=1)
    et, src, dst, base = edge_operator(e, N)
    y64 = intent_propagate(x.double(), P.double(), src, dst, base)
    xd, Pd = x.to(dev), P.to(dev).contiguous()
    # all rows, no routing
    y = ops.dgcf_propagate_raw(g, Pd, xd, y=torch.empty_like(xd))
    np.testing.assert_allclose(y.cpu().double().numpy(), y64.numpy(), rtol=0, atol=2e-6)
    # z + A x epilogue
    zz = torch.randn(N, D, generator=gen).to(dev)
    out = ops.dgcf_propagate_raw(g, Pd, xd, z=zz, zout=torch.empty_like(xd))
    np.testing.assert_allclose(out.cpu().double().numpy(), (zz.cpu().double() + y64).numpy(), rtol=0, atol=4e-6)
    # user rows only, routed: S and the next P for every edge; item rows untouched
    yu = torch.full_like(xd, 7.0)
    S_dev, Pn = torch.empty_like(Pd), torch.empty_like(Pd)
    ops.dgcf_propagate_raw(g, Pd, xd, y=yu, rows=(0, U), route_end=U, S=S_dev, P_next=Pn)
    np.testing.assert_allclose(yu[:U].cpu().double().numpy(), y64[:U].numpy(), rtol=0, atol=2e-6)
    assert bool((yu[U:] == 7.0).all())
    S64 = P.double() + routing_scores(y64, x.double(), et, K)
    np.testing.assert_allclose(S_dev.cpu().double().numpy(), S64.numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(Pn.cpu().double().numpy(), torch.softmax(S64, 1).numpy(), rtol=0, atol=1e-5)
    # the last iteration's form: every row propagated, user rows routed, item rows read the OLD P
    ya, S2, Pn2 = torch.empty_like(xd), torch.empty_like(Pd), torch.empty_like(Pd)
    ops.dgcf_propagate_raw(g, Pd, xd, y=ya, route_end=U, S=S2, P_next=Pn2)
    assert torch.equal(ya[:U], yu[:U]) and torch.equal(S2, S_dev) and torch.equal(Pn2, Pn)
    assert torch.equal(ya, y)


@pytest.mark.parametrize("D,K", [(64, 4), (128, 2)])
def test_dcor_against_fp64(dev, D, K):
    from chaorec_amd import ops
    B, N = 1024, 5000
    gen = torch.Generator().manual_seed(D * 7 + K)
    table = (torch.randn(N, D, generator=gen) * 0.3).float()
    idx = torch.randint(0, N, (2 * B,), generator=gen)          # repeated rows, as a batch has
    t64 = table.double().requires_grad_(True)
    x = t64[idx]
    w = D // K
    ref = sum(distance_correlation(x[:, k * w:(k + 1) * w], x[:, (k + 1) * w:(k + 2) * w]) for k in range(K - 1))
    ref = ref / ((K + 1) * K / 2)
    ref.backward()
    td = table.to(dev).requires_grad_(True)
    out = ops.dgcf_cor_loss(td, idx.to(dev), K)
    assert tuple(out.shape) == (1,)
    (out * 3.0).sum().backward()
    assert abs(float(out.item()) - float(ref.item())) < 1e-5 * max(1.0, abs(float(ref.item())))
    g = td.grad.cpu().double()
    scale = float(t64.grad.abs().max())
    assert float((g - 3.0 * t64.grad).abs().max()) <= 1e-3 * 3.0 * scale
    # ordered reductions: a second run gives the same bits
    td2 = table.to(dev).requires_grad_(True)
    out2 = ops.dgcf_cor_loss(td2, idx.to(dev), K)
    (out2 * 3.0).sum().backward()
    assert torch.equal(out, out2) and torch.equal(td.grad, td2.grad)


def _baby_run(dev, steps, seed=3):
    from chaorec_amd import graph
    from chaorec_amd.Model import DGCF
    from chaorec_amd.optim import FusedAdam
    d = load_interactions("baby")
    U, I, e = d["U"], d["I"], d["train"]
    torch.manual_seed(seed)
    m = DGCF(U, I, e, graph.user_item_dict_from_edges(e), 64, 1e-3, 0.01, 4, 3, 3, "add", dev).to(dev)
    opt = FusedAdam([{"params": m.parameters(), "lr": 1e-3}])
    rng = np.random.default_rng(seed)
    losses = []
    for _ in range(steps):
        b = rng.choice(len(e), 1024, replace=False)
        users = torch.as_tensor(e[b, 0]).long().to(dev)
        pos = torch.as_tensor(e[b, 1]).long().to(dev)
        neg = torch.as_tensor(rng.integers(U, U + I, 1024)).long().to(dev)
        opt.zero_grad()
        loss = m.loss(users, pos, neg)
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return m, torch.cat(losses)


def test_two_runs_bit_identical(dev):
    m1, l1 = _baby_run(dev, 3)
    m2, l2 = _baby_run(dev, 3)
    assert torch.equal(l1, l2)
    for (n, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), n
    assert torch.equal(m1.S, m2.S) and torch.equal(m1.result, m2.result)


def test_captured_epoch_equals_eager_epoch(dev):
    from chaorec_amd import dataload, graph
    from chaorec_amd.Model import DGCF
    from chaorec_amd.optim import FusedAdam
    from chaorec_amd.train_and_evaluate import train_and_evaluate
    from chaorec_amd.utils import setup_seed
    d = load_interactions("baby")
    U, I, e = d["U"], d["I"], d["train"]
    uid = graph.user_item_dict_from_edges(e)
    val, test = np.array(d["val"], dtype=object), np.array(d["test"], dtype=object)
    out = {}
    for captured in (True, False):
        setup_seed(11)
        m = DGCF(U, I, e, uid, 64, 1e-3, 0.001, 4, 2, 3, "add", dev).to(dev)
        loader = dataload.DeviceBatchSampler(U, I, uid, e, 1024, dev, "DGCF", 11)
        opt = FusedAdam([{"params": m.parameters(), "lr": 1e-3}])
        hist = []
        train_and_evaluate(m, loader, val, test, opt, 1, model_name="DGCF", topk=(5, 10, 20), graph=captured, history=hist)
        out[captured] = (hist[0]["loss"], [p.detach().clone() for p in m.parameters()], m.S.clone())
    (lc, pc, sc), (le, pe, se) = out[True], out[False]
    assert lc == pytest.approx(le, rel=1e-5)
    for a, b in zip(pc, pe):
        torch.testing.assert_close(a, b, rtol=0, atol=1e-5)
    torch.testing.assert_close(sc, se, rtol=0, atol=1e-4)
    assert not torch.equal(sc, torch.ones_like(sc))


def test_unsupported_shapes_refused(dev):
    from chaorec_amd import graph, ops
    from chaorec_amd.Model import DGCF
    e = load_golden("dgcf_small.npz")["edges"]
    uid = graph.user_item_dict_from_edges(e)
    for D, K, T, L in ((48, 4, 1, 1), (16, 8, 1, 1), (512, 4, 1, 1), (64, 3, 1, 1), (64, 4, 0, 1), (64, 4, 1, 0)):
        with pytest.raises(ValueError):
            DGCF(48, 40, e, uid, D, 1e-3, 0.01, K, T, L, "add", dev)
    with pytest.raises(ValueError, match="D % \\(4K\\)"):
        ops.dgcf_check_shape(24, 4)


def test_main_runs_dgcf_end_to_end(dev, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    proc = subprocess.run([sys.executable, "-m", "chaorec_amd.main", "--Model", "DGCF", "--data_path", "baby",
                           "--num_epoch", "1", "--data_root", str(tmp_path / "Data")],
                          cwd=tmp_path, env=env, capture_output=True, text=True, timeout=1500)
    assert proc.returncode == 0, proc.stderr[-3000:]
    log = proc.stdout + proc.stderr
    assert "Epoch 1, Loss:" in log and "Test Metrics:" in log and "Best performance:" in log
    assert "recall:" in log
