"""FusedLightGCNStep (and the one-rank FusedShardedLightGCNStep) against the fp64 step of oracle/lightgcn_step_fp64.py:
every route, one independent anchor.  Each checked step snapshots the joined table, Adam's moments and step count, runs
the step and holds result, loss, m', v' and W' to the reference's per-element bound (no global tolerance); the batch
gradient buffer must be all-zero again.  A light step leaves only the batch's rows of the propagated table: those are
compared.  CHAOREC_BPR_ORDERED is set before a step is built: a captured step keeps what was set at capture."""
import json

import numpy as np
import pytest
import torch

from conftest import load_interactions
from oracle.lightgcn_step_fp64 import excess, lightgcn_step_fp64

pytestmark = pytest.mark.gpu

LR = 1e-3
_WORST = {}          # route -> {tensor: largest |error| / bound seen}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chaorec_amd import _lib
    _lib.load()
    yield torch.device("cuda:0")
    print("\nlargest |error| / bound per route:\n" + json.dumps(_WORST, indent=1, sort_keys=True))


def _model(dev, U, I, edges, D, L, seed=0):
    from chaorec_amd.Model import LightGCN
    from chaorec_amd.optim import FusedAdam
    torch.manual_seed(seed)
    m = LightGCN(U, I, edges, None, D, 1e-3, L, "add", dev).to(dev)
    return m, FusedAdam(m.parameters(), lr=LR)


def _check_step(route, step, opt, U, I, csr, L, reg, table, result, batch=None, light=False):
    """run ONE step of `step` and hold it to the fp64 reference; table() / result() read the joined table / the layer mean"""
    W0, m0, v0 = table().clone(), step.m.clone(), step.v.clone()
    t = int(opt._step_dev) + 1
    loss = step(*batch, single=True) if batch is not None else step(single=True)
    torch.cuda.synchronize()
    users, pos, neg = (x.cpu() for x in step.ids)
    assert int(users.min()) >= 0 and int(users.max()) < U
    assert int(torch.cat((pos, neg)).min()) >= 0 and int(torch.cat((pos, neg)).max()) < I      # item ids are LOCAL
    assert int(opt._step_dev) == t
    group = opt.param_groups[0]
    assert group["weight_decay"] == 0
    # the kernels receive the betas as fp32 (chaorec_spmm_csr_adam_f32, chaorec_bpr_fwd_bwd_at_f32): Adam with THOSE betas
    # is what they compute -- 1 - beta and beta^t of 0.999f, not of the python float 0.999 (common.h:AdamConsts)
    betas = tuple(float(np.float32(b)) for b in group["betas"])
    ref = lightgcn_step_fp64(csr.rowptr, csr.col, csr.val, W0, users, pos, neg, U, reg, L, m0, v0, t, group["lr"],
                             betas, group["eps"])
    R = result()
    if light:
        rows = torch.unique(torch.cat((users, pos + U, neg + U)))
        r_res = excess(R[rows.to(R.device)], (ref["result"][0][rows], ref["result"][1][rows]))
    else:
        r_res = excess(R, ref["result"])
    r = {"result": r_res, "loss": excess(loss, ref["loss"]), "m": excess(step.m, ref["m"]),
         "v": excess(step.v, ref["v"]), "W": excess(table(), ref["W"])}
    worst = _WORST.setdefault(route, {})
    for k, x in r.items():
        worst[k] = max(worst.get(k, 0.0), x)
    assert not bool(step.G.any()), route                  # the batch-gradient buffer is all-zero between steps
    assert max(r.values()) <= 1.0, (route, t, r)
    return r


def _fused_check_step(route, step, model, opt, batch=None, light=False):
    return _check_step(route, step, opt, model.num_user, model.num_item, model.graph, model.n_layers, model.reg_weight,
                  lambda: model._flat, lambda: step.final if light else model.result, batch, light)


def _drawn(dev, edges):
    return torch.from_numpy(edges.astype(np.int64)).to(dev)


# ---- the step bench.py times ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ordered", ["1", "2"])
def test_bench_step_sports(dev, ordered, monkeypatch):
    """sports, D = 64, L = 3, B = 1024, batch drawn in the launch, captured: steps 1, 2, 3, then 31 and 32"""
    from chaorec_amd.optim import FusedLightGCNStep
    monkeypatch.setenv("CHAOREC_BPR_ORDERED", ordered)
    d = load_interactions("sports")
    model, opt = _model(dev, d["U"], d["I"], d["train"], 64, 3)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    step = FusedLightGCNStep(model, opt, batch_size=1024, edges=_drawn(dev, d["train"]), seed=3, step_dev=cnt)
    assert step.graph is not None and not step.light
    for _ in range(3):
        _fused_check_step(f"bench sports captured, ordered={ordered}", step, model, opt)
    step.run(27)
    for _ in range(2):
        _fused_check_step(f"bench sports captured, ordered={ordered}", step, model, opt)
    assert int(opt._step_dev) == 32


# ---- baby: widths and depths, eager and captured ----------------------------------------------------------------------

@pytest.mark.parametrize("D,L,capture,ordered", [(8, 4, True, "1"), (8, 2, False, "2"), (32, 1, False, "1"),
                                                 (128, 2, True, "2"), (256, 4, False, "1"), (256, 1, True, "2")])
def test_baby_widths_and_depths(dev, D, L, capture, ordered, monkeypatch):
    from chaorec_amd.optim import FusedLightGCNStep
    monkeypatch.setenv("CHAOREC_BPR_ORDERED", ordered)
    monkeypatch.setenv("CHAOREC_SPARSE_BACKWARD", "0")
    d = load_interactions("baby")
    model, opt = _model(dev, d["U"], d["I"], d["train"], D, L, seed=D + L)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    step = FusedLightGCNStep(model, opt, batch_size=1024, edges=_drawn(dev, d["train"]), seed=5, step_dev=cnt,
                             capture=capture)
    route = f"baby D={D} L={L} {'captured' if capture else 'eager'}, ordered={ordered}"
    _fused_check_step(route, step, model, opt)
    step.run(3)
    _fused_check_step(route, step, model, opt)


# ---- batch edges ------------------------------------------------------------------------------------------------------

def _star_graph(U, I, per_user, seed):
    """U users with per_user distinct items each, out of I: the items nobody links to have degree 0"""
    rng = np.random.default_rng(seed)
    return np.array([[u, U + i] for u in range(U) for i in np.sort(rng.choice(I, per_user, replace=False))], dtype=np.int64)


@pytest.mark.parametrize("case", ["repeats_atomic", "isolated_negatives_ordered"])
def test_given_batch_repeats_and_isolated_rows(dev, case, monkeypatch):
    """4 users and 3000 items: every user occurs ~256 times in a batch of 1024 (its gradient row is the sum of all of
    them); the negatives are items of degree 0 (their propagated row is w x0, their gradient w G)"""
    from chaorec_amd.optim import FusedLightGCNStep
    monkeypatch.setenv("CHAOREC_BPR_ORDERED", "1" if case == "repeats_atomic" else "2")
    U, I, B = 4, 3000, 1024
    edges = _star_graph(U, I, 700, seed=6)
    model, opt = _model(dev, U, I, edges, 64, 2, seed=6)
    step = FusedLightGCNStep(model, opt, batch_size=B, given_batch=True, capture=case == "repeats_atomic")
    linked = np.unique(edges[:, 1])
    isolated = np.setdiff1d(np.arange(U, U + I), linked)
    rng = np.random.default_rng(7)
    for _ in range(3):
        sel = rng.integers(0, len(edges), B)
        negs = rng.choice(isolated, B) if case != "repeats_atomic" else rng.integers(U, U + I, B)
        batch = [torch.from_numpy(a.astype(np.int64)).to(dev) for a in (edges[sel, 0], edges[sel, 1], negs)]
        _fused_check_step(f"given batch, {case}", step, model, opt, batch)


@pytest.mark.parametrize("B,ordered", [(1, "1"), (3, "2"), (1023, "1"), (5462, "2")])
def test_batch_sizes(dev, B, ordered, monkeypatch):
    """B % 4 != 0 (the launch grid is (B + 3) / 4 waves of four), one sample, and 3 B > 16384 slots: the ordered mode
    hands that batch to the atomic launch"""
    from chaorec_amd.optim import FusedLightGCNStep
    monkeypatch.setenv("CHAOREC_BPR_ORDERED", ordered)
    d = load_interactions("baby")
    model, opt = _model(dev, d["U"], d["I"], d["train"], 64, 2, seed=B)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    step = FusedLightGCNStep(model, opt, batch_size=B, edges=_drawn(dev, d["train"]), seed=9, step_dev=cnt)
    for _ in range(2):
        _fused_check_step(f"baby B={B}, ordered={ordered}", step, model, opt)


def test_wide_rows_are_refused(dev, monkeypatch):
    """D > 256: the Adam epilogue is not built for it; the step says so instead of computing something else"""
    from chaorec_amd.optim import FusedLightGCNStep
    monkeypatch.setenv("CHAOREC_BPR_ORDERED", "2")
    d = load_interactions("baby")
    model, opt = _model(dev, d["U"], d["I"], d["train"], 272, 2)
    step = FusedLightGCNStep(model, opt, batch_size=256, edges=_drawn(dev, d["train"]), seed=9, capture=False)
    with pytest.raises(RuntimeError, match="D > 256|D=272"):
        step()
    torch.cuda.synchronize()


# ---- the light forward and the row-sparse backward ---------------------------------------------------------------------

@pytest.mark.parametrize("D,L,light,capture", [(64, 3, True, True), (128, 2, True, False), (256, 4, True, True),
                                               (64, 2, False, False), (128, 4, False, True), (256, 3, False, False)])
def test_light_and_row_sparse_routes(dev, D, L, light, capture, monkeypatch):
    from chaorec_amd import _lib
    from chaorec_amd.optim import FusedLightGCNStep
    from chaorec_amd.synthetic import synthetic_interactions
    monkeypatch.setenv("CHAOREC_SPARSE_BACKWARD", "1")
    if light:
        monkeypatch.delenv("CHAOREC_LIGHT_FORWARD", raising=False)
    else:
        monkeypatch.setenv("CHAOREC_LIGHT_FORWARD", "0")
    U, I, E = 4000, 2500, 40000
    edges = synthetic_interactions(U, I, E, seed=D + L)
    model, opt = _model(dev, U, I, edges, D, L, seed=L)
    rp = model.graph.rowptr
    assert int((rp[1:] - rp[:-1]).max()) > _lib.load().chaorec_spmm_long_threshold()    # hub rows: the long-row walk
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    step = FusedLightGCNStep(model, opt, batch_size=1024, edges=_drawn(dev, edges), seed=L, step_dev=cnt, capture=capture)
    assert step.sparse_bwd and step.light == light
    route = f"{'light' if light else 'row-sparse'} D={D} L={L} {'captured' if capture else 'eager'}"
    for _ in range(2):
        _fused_check_step(route, step, model, opt, light=light)


# ---- the one-rank sharded step ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,capture", [(2, False), (3, True)])
def test_one_rank_sharded_step(dev, L, capture):
    from chaorec_amd import dist as cdist
    from chaorec_amd.optim import FusedAdam
    from chaorec_amd.synthetic import synthetic_interactions
    U, I, E, D, B = 3000, 1200, 20000, 64, 256
    edges = synthetic_interactions(U, I, E, seed=2)
    shard = cdist.UserShard(edges, U, I, 1, 0, dev)
    m = cdist.ShardedLightGCN(shard, None, D, 1e-3, L, dev, seed=1).to(dev)
    opt = FusedAdam(m.parameters(), lr=LR)
    step = cdist.FusedShardedLightGCNStep(m, opt, batch_size=B, given_batch=True, capture=capture)
    csr = cdist.joined_shard_csr(shard)
    rng = np.random.default_rng(5)
    for _ in range(3):
        sel = rng.choice(E, B, replace=False)
        batch = [torch.from_numpy(a.astype(np.int64)).to(dev) for a in (edges[sel, 0], edges[sel, 1], rng.integers(U, U + I, B))]
        _check_step(f"one-rank sharded L={L} {'captured' if capture else 'eager'}", step, opt, U, I, csr, L, m.reg_weight,
               lambda: torch.cat((m.user_embedding.weight, m.item_embedding.weight)).detach(),
               lambda: torch.cat((m.result_u, m.result_i)), batch)
