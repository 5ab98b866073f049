"""DGCF host logic (no GPU): the CLI flags and YAML grid, the entry -> edge map of graph.dgcf_structure, and a float64 torch
restatement of DGCF (Model/DGCF.py + utils.distance_correlation) that reproduces the reference goldens dgcf_small.npz and
dgcf_baby.npz (tests/golden/gen_dgcf.py).  tests/test_gpu_dgcf.py checks the kernels against this restatement at sizes no
golden covers."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from chaorec_amd import graph
from chaorec_amd.arg_parser import load_yaml_config, parse_args

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def init_tables(U, I, D, seed=0):
    """The reference's parameter creation order: two nn.Embedding's (normal init), then xavier_uniform_ on each."""
    torch.manual_seed(seed)
    a, b = torch.nn.Embedding(U, D), torch.nn.Embedding(I, D)
    torch.nn.init.xavier_uniform_(a.weight)
    torch.nn.init.xavier_uniform_(b.weight)
    return a.weight.detach().clone(), b.weight.detach().clone()


def edge_operator(edges, n_nodes):
    """(src, dst, deg^-1/2[src] deg^-1/2[dst]) of both directions of every edge, in the reference's list order."""
    e = torch.as_tensor(np.asarray(edges)).long()
    src, dst = torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])
    deg = torch.bincount(src, minlength=n_nodes).double()
    dis = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    return e, src, dst, dis[src] * dis[dst]


def intent_propagate(ego, P, src, dst, base):
    """y = A_P ego: edge e's weight in slice k is base_e * P[e mod E, k]."""
    K, w = P.shape[1], ego.shape[1] // P.shape[1]
    wt = (base[:, None] * torch.cat([P, P])).repeat_interleave(w, dim=1)
    return torch.zeros_like(ego).index_add(0, dst, wt * ego[src])


def routing_scores(X, ego, e, K):
    """< normalize(X_k[u]), tanh(normalize(ego_k[i])) > per edge and slice -> [E, K]."""
    E, w = e.shape[0], X.shape[1] // K
    un = F.normalize(X[e[:, 0]].reshape(E, K, w), dim=-1, eps=1e-12)
    it = torch.tanh(F.normalize(ego[e[:, 1]].reshape(E, K, w), dim=-1, eps=1e-12))
    return (un * it).sum(-1)


def dgcf_forward(x0, edges, K, T, L, S):
    """-> (result = sum of the layers, S after L * T updates).  S: [E, K], carried state (no autograd history)."""
    e, src, dst, base = (t.to(x0.device) for t in edge_operator(edges, x0.shape[0]))
    base = base.to(x0.dtype)
    ego, out = x0, x0
    S = S.detach()
    for _ in range(L):
        X = None
        for _ in range(T):
            P = torch.softmax(S, dim=1)
            X = intent_propagate(ego, P, src, dst, base)
            S = P + routing_scores(X.detach(), ego.detach(), e, K)
        ego = X
        out = out + ego
    return out, S


def distance_correlation(a, b):
    def centred(x):
        r = (x * x).sum(1, keepdim=True)
        d = torch.sqrt(torch.clamp(r - 2 * x @ x.t() + r.t(), min=0.0) + 1e-8)
        return d - d.mean(0, keepdim=True) - d.mean(1, keepdim=True) + d.mean()

    def dcov(p, q):
        n = p.shape[0]
        return torch.sqrt(torch.clamp((p * q).sum() / (n * n), min=0.0) + 1e-8)

    A, B = centred(a), centred(b)
    return dcov(A, B) / (torch.sqrt(torch.clamp(dcov(A, A) * dcov(B, B), min=0.0)) + 1e-10)


def cor_loss(result, users, pos_global, K):
    x = torch.cat([result[users], result[pos_global]])
    w = x.shape[1] // K
    total = torch.zeros(1, dtype=result.dtype, device=result.device)
    for k in range(K - 1):
        total = total + distance_correlation(x[:, k * w:(k + 1) * w], x[:, (k + 1) * w:(k + 2) * w])
    return total / ((K + 1) * K / 2)


def dgcf_loss(result, users, pos_global, neg_global, K, reg, cor_decay):
    u, p, n = result[users], result[pos_global], result[neg_global]
    bpr = -torch.mean(torch.log(torch.sigmoid((u * p).sum(1) - (u * n).sum(1)) + 1e-5))
    l2 = reg * ((u ** 2).mean() + (p ** 2).mean() + (n ** 2).mean())
    return bpr + l2 + cor_decay * cor_loss(result, users, pos_global, K)


def dgcf_step64(tu, ti, edges, K, T, L, S, users, pos, neg, reg, cor_decay):
    """One loss + backward in float64 -> (loss, result, S, g_user, g_item); pos / neg GLOBAL ids."""
    tu = tu.double().clone().requires_grad_(True)
    ti = ti.double().clone().requires_grad_(True)
    result, S = dgcf_forward(torch.cat([tu, ti]), edges, K, T, L, S.double())
    loss = dgcf_loss(result, *(torch.as_tensor(v).long() for v in (users, pos, neg)), K, reg, cor_decay)
    loss.backward()
    return loss.detach(), result.detach(), S, tu.grad, ti.grad


# ---------------------------------------------------------------------------------------------------------------------
def test_cli_flags_and_yaml_grid():
    a = parse_args(["--Model", "DGCF"])
    assert a.corDecay == 0.001 and a.n_factors == 4 and a.n_iterations == 3
    a = parse_args(["--Model", "DGCF", "--corDecay", "0.01", "--n_factors", "2"])
    assert a.corDecay == 0.01 and a.n_factors == 2
    cfg = load_yaml_config("DGCF")
    assert cfg["learning_rate"] == [0.01, 0.001] and cfg["reg_weight"] == [0.01, 0.001]
    assert cfg["corDecay"] == [0.01, 0.001, 0.0001] and cfg["n_factors"] == [2, 4]
    assert cfg["n_iterations"] == [1, 2] and cfg["n_layers"] == [3]
    assert sorted(cfg["hyper_parameters"]) == sorted(["n_layers", "learning_rate", "reg_weight", "corDecay", "n_factors",
                                                      "n_iterations"])


def test_main_table_has_dgcf():
    from chaorec_amd import registry
    from chaorec_amd.Model import DGCF
    spec = registry.MODELS["DGCF"]
    assert registry.M.DGCF is DGCF and callable(spec.build) and spec.capture and spec.epoch is None and not spec.features


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_entry_edge_map(seed):
    rng = np.random.default_rng(seed)
    U, I = 9, 7
    e = [(int(rng.integers(0, U - 1)), U + int(rng.integers(0, I - 1))) for _ in range(30)]   # last user / item: no edge
    e += [e[0], e[0], e[5]]                                     # repeated interactions
    e = np.array(e, dtype=np.int32)
    E, N = len(e), U + I
    g = graph.dgcf_structure(e, U, N)
    ref = graph.lightgcn_csr(e, N)
    assert torch.equal(g.rowptr, ref.rowptr) and torch.equal(g.col, ref.col) and torch.equal(g.val, ref.val)
    assert g.n_edges == E and g.eid.dtype == torch.int32 and g.eid.numel() == 2 * E
    rows = torch.repeat_interleave(torch.arange(N), g.rowptr[1:] - g.rowptr[:-1])
    eid, col = g.eid.long(), g.col.long()
    # entry (row r, col c) of edge k is (u_k, i_k) in one of its two directions
    eu, ei = torch.as_tensor(e[:, 0]).long()[eid], torch.as_tensor(e[:, 1]).long()[eid]
    assert bool(((rows == eu) & (col == ei) | (rows == ei) & (col == eu)).all())
    # both directions of every edge map to it, each once
    assert torch.equal(torch.bincount(eid, minlength=E), torch.full((E,), 2))
    # exactly one user-row entry per edge
    user = rows < U
    assert torch.equal(torch.sort(eid[user]).values, torch.arange(E))
    # within a row, the entries keep train_data order (the copies of a repeated interaction too)
    for r in range(N):
        seg = eid[g.rowptr[r]:g.rowptr[r + 1]]
        assert bool((seg[1:] > seg[:-1]).all())
    assert int(g.rowptr[U - 1 + 1] - g.rowptr[U - 1]) == 0 and int(g.rowptr[N] - g.rowptr[N - 1]) == 0


def _small():
    return np.load(os.path.join(GOLDEN, "dgcf_small.npz"))


@pytest.mark.parametrize("K,T", [(1, 1), (2, 2), (4, 1), (4, 3)])
def test_restatement_reproduces_small_golden(K, T):
    z = _small()
    U, I, D, L = int(z["U"]), int(z["I"]), int(z["D"]), int(z["L"])
    c = lambda k: z[f"k{K}t{T}_{k}"]  # noqa: E731
    tu, ti = init_tables(U, I, D)
    assert np.array_equal(tu.numpy(), c("p_user")) and np.array_equal(ti.numpy(), c("p_item"))
    E = z["edges"].shape[0]
    S0 = torch.ones((E, K), dtype=torch.float64)
    loss, result, S, gu, gi = dgcf_step64(tu, ti, z["edges"], K, T, L, S0, z["users"], z["pos"], z["neg"],
                                          float(z["reg"]), float(z["corDecay"]))
    assert abs(loss.item() - float(c("loss"))) < 1e-6
    np.testing.assert_allclose(result.numpy(), c("result"), rtol=0, atol=1e-5)
    np.testing.assert_allclose(S.numpy().T, c("S"), rtol=0, atol=1e-5)
    np.testing.assert_allclose(gu.numpy(), c("g_user"), rtol=0, atol=2e-6)
    np.testing.assert_allclose(gi.numpy(), c("g_item"), rtol=0, atol=2e-6)
    assert tuple(c("loss_shape")) == (1,)
    if K == 1:
        assert float(c("cor")) == 0.0


@pytest.mark.parametrize("K,T", [(2, 2), (4, 3)])
def test_restatement_reproduces_small_trajectory(K, T):
    """Three fixed-batch Adam steps: S carries over from step to step (it is never reset)."""
    z = _small()
    U, I, D, L = int(z["U"]), int(z["I"]), int(z["D"]), int(z["L"])
    c = lambda k: z[f"k{K}t{T}_{k}"]  # noqa: E731
    tu, ti = init_tables(U, I, D)
    tu, ti = tu.double().requires_grad_(True), ti.double().requires_grad_(True)
    opt = torch.optim.Adam([tu, ti], lr=float(z["lr"]))
    S = torch.ones((z["edges"].shape[0], K), dtype=torch.float64)
    ids = [torch.as_tensor(z[k]).long() for k in ("users", "pos", "neg")]
    for s in range(3):
        opt.zero_grad()
        result, S = dgcf_forward(torch.cat([tu, ti]), z["edges"], K, T, L, S)
        loss = dgcf_loss(result, *ids, K, float(z["reg"]), float(z["corDecay"]))
        loss.backward()
        opt.step()
        assert abs(loss.item() - float(c("traj_loss")[s])) < 1e-5
        np.testing.assert_allclose(S.numpy().T, c("traj_S")[s], rtol=0, atol=1e-4)
    np.testing.assert_allclose(tu.detach().numpy(), c("traj_user"), rtol=0, atol=1e-5)


def test_restatement_reproduces_baby_golden():
    z = np.load(os.path.join(GOLDEN, "dgcf_baby.npz"))
    ib = np.load(os.path.join(GOLDEN, "baby_interactions.npz"))
    U, I, D, K, T, L = (int(z[k]) for k in ("U", "I", "D", "K", "T", "L"))
    edges = ib["train"]
    tu, ti = init_tables(U, I, D)
    assert np.array_equal(torch.cat([tu, ti]).numpy()[z["rows"]], z["init_rows"])
    S0 = torch.ones((edges.shape[0], K), dtype=torch.float64)
    loss, result, S, gu, gi = dgcf_step64(tu, ti, edges, K, T, L, S0, z["users"], z["pos"], z["neg"], float(z["reg"]),
                                          float(z["corDecay"]))
    assert abs(loss.item() - float(z["loss"])) < 1e-5
    np.testing.assert_allclose(result.numpy()[z["rows"]], z["result_rows"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(S.numpy()[z["edge_sample"]].T, z["S_sample"], rtol=0, atol=1e-5)
    g = torch.cat([gu, gi]).numpy()
    np.testing.assert_allclose(g[z["grad_rows"]], z["g_rows"], rtol=0, atol=1e-6)
