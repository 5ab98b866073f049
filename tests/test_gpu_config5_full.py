"""BASELINE.json configs[4] WHOLE on one GPU: the synthetic 10 M users x 2 M items graph, ~2e8 interactions -> ~4e8
directed edges, dim 128, 3 layers (tables + Adam state + CSR ~55 GB of the 288 GB) -- the N = 1 anchor of the config's
scaling curve.  The graph is generated and laid out on the device (synthetic_interactions_torch, graph.lightgcn_csr on
a CUDA edge list); the host only builds the SpMM row descriptors.  The oracle cannot restate 4e8 edges in seconds, so:
  * SpMM: sampled + heaviest + empty rows against the oracle's ordered sums (bit-exact) and inside the rigorous
    (deg + 1) 2^-24 sum|terms| bound of fp64 rows; determinism; symmetry <Ax, z> = <x, Az> over the whole graph;
  * full-rank top-50 (user-chunked workspace) of sampled + heaviest-history users over all 2 M items against
    oracle.score_topk, bit-exact; sortedness / range / uniqueness over all 1e7 users;
  * the captured FusedLightGCNStep against the same launches issued eagerly.
Set CHAOREC_SKIP_CONFIG5_FULL=1 to skip (the module needs ~110 GB of HBM and several minutes)."""
import os
import time

import numpy as np
import pytest
import torch

from accept import ULP24

pytestmark = pytest.mark.gpu

D, L = 128, 3


@pytest.fixture(scope="module")
def full():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if os.environ.get("CHAOREC_SKIP_CONFIG5_FULL") == "1":
        pytest.skip("CHAOREC_SKIP_CONFIG5_FULL=1")
    from chaorec_amd import _lib, graph
    from chaorec_amd.synthetic import DATASET_SHAPES, synthetic_interactions_torch
    _lib.load()
    dev = torch.device("cuda:0")
    if torch.cuda.get_device_properties(0).total_memory < 200 * (1 << 30):
        pytest.skip("needs the 288 GB of an MI355X")
    U, I, E = DATASET_SHAPES["config5"]
    t0 = time.perf_counter()
    edges = synthetic_interactions_torch(U, I, E, seed=42, device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    csr = graph.lightgcn_csr(edges, U + I)
    hist = graph.user_hist_csr_from_edges(edges, U)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    csr.schedule(D)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print(f"config 5 whole: {len(edges)} interactions generated in {t1 - t0:.1f} s, CSR + history on the device "
          f"{t2 - t1:.1f} s, SpMM schedule on the host {t3 - t2:.1f} s")
    assert abs(len(edges) - E) <= 0.001 * E and csr.nnz == 2 * len(edges)
    g = torch.Generator(device=dev).manual_seed(5)
    a = float(np.sqrt(6.0 / (U + I + D)))
    x = (torch.rand(U + I, D, generator=g, device=dev) * 2 - 1) * a          # xavier_uniform-shaped table
    return dict(dev=dev, U=U, I=I, edges=edges, csr=csr, hist=hist, x=x)


def _rows_sub_csr(csr, rows):
    """(sub_rowptr, col, val) on the host for the given rows of a device CSR."""
    rp = csr.rowptr[torch.from_numpy(np.concatenate([rows, rows + 1])).to(csr.rowptr.device)].cpu().numpy()
    s, e = rp[:len(rows)], rp[len(rows):]
    sub_rp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(e - s, out=sub_rp[1:])
    take = torch.from_numpy(np.concatenate([np.arange(a, b) for a, b in zip(s, e)]) if sub_rp[-1] else np.zeros(0, np.int64))
    take = take.to(csr.col.device)
    return sub_rp, csr.col[take].cpu().numpy(), csr.val[take].cpu().numpy()


def test_spmm_rows_vs_oracle_and_fp64(full, oracle):
    from chaorec_amd import ops
    csr, x = full["csr"], full["x"]
    y = ops.spmm_raw(csr, x)
    assert torch.equal(y, ops.spmm_raw(csr, x))                  # deterministic
    deg = (csr.rowptr[1:] - csr.rowptr[:-1])
    heavy = torch.topk(deg, 24).indices.cpu().numpy()
    empty = torch.nonzero(deg == 0)[:8, 0].cpu().numpy()
    rng = np.random.default_rng(0)
    rows = np.unique(np.concatenate([rng.choice(csr.n_rows, 4000, replace=False), heavy, empty])).astype(np.int64)
    sub_rp, col, val = _rows_sub_csr(csr, rows)
    sdeg = sub_rp[1:] - sub_rp[:-1]
    assert sdeg.max() > 5000                                     # the item hubs are in the sample
    # the oracle gathers from the source rows only: hand it a compacted table
    ucol, inv = np.unique(col, return_inverse=True)
    xs = x[torch.from_numpy(ucol.astype(np.int64)).to(x.device)].cpu().numpy()
    want = oracle.spmm((sub_rp, inv.astype(np.int32), val), xs)
    got = y[torch.from_numpy(rows).to(y.device)].cpu().numpy()
    assert np.array_equal(got, want)
    ref = np.zeros((len(rows), D))
    mass = np.zeros((len(rows), D))
    for k in range(len(rows)):
        s, e = sub_rp[k], sub_rp[k + 1]
        terms = val[s:e].astype(np.float64)[:, None] * xs[inv[s:e]].astype(np.float64)
        ref[k], mass[k] = terms.sum(0), np.abs(terms).sum(0)
    bound = (sdeg[:, None] + 1) * ULP24 * mass
    assert np.all(np.abs(got - ref) <= bound + 1e-30)
    light = sdeg <= 64
    assert np.abs(got - ref)[light].max() <= 2e-6 * np.abs(ref)[light].max()
    # symmetry over the whole graph: <Ax, z> = <x, Az>
    gz = torch.Generator(device=x.device).manual_seed(7)
    z = torch.randn(x.shape, generator=gz, device=x.device) * 0.01
    yz = ops.spmm_raw(csr, z)
    lhs, rhs = float((y.double() * z.double()).sum()), float((x.double() * yz.double()).sum())
    assert lhs == pytest.approx(rhs, rel=1e-6)
    # layer-mean epilogue == the reference's accumulation, on the sampled rows
    del z, yz
    acc = torch.empty_like(x)
    ops.spmm_raw(csr, x, acc=acc, acc_init=x, acc_w=0.25)
    w = np.float32(0.25)
    sel = torch.from_numpy(rows).to(acc.device)
    assert np.array_equal(acc[sel].cpu().numpy(), (w * x[sel].cpu().numpy()) + (w * got))


def test_full_rank_vs_oracle(full, oracle):
    from chaorec_amd import ops
    U, I, dev = full["U"], full["I"], full["dev"]
    res = ops.layer_mean_propagate(full["x"], full["csr"], L)
    st = {}
    t0 = time.perf_counter()
    idx, val = ops.score_topk(res[:U], res[U:], full["hist"], 1e-6, 50, id_offset=U, stats=st)
    torch.cuda.synchronize()
    print(f"config 5 whole: gene_ranklist of {U} users x {I} items (with stats sync) {time.perf_counter() - t0:.2f} s, "
          f"{st.get('user_chunks')} user chunks, {st['fallback_users']} users on the exact route")
    assert st["prefilter_users"] == U and st.get("user_chunks", 1) >= 2      # the workspace was cut by users
    hr, hc = full["hist"]
    hdeg = hr[1:] - hr[:-1]
    rng = np.random.default_rng(1)
    users = np.unique(np.concatenate([rng.choice(U, 240, replace=False), torch.topk(hdeg, 16).indices.cpu().numpy(),
                                      np.array([0, U - 1])])).astype(np.int64)
    ud = torch.from_numpy(users).to(dev)
    rp = torch.stack([hr[ud], hr[ud + 1]], 1).cpu().numpy()
    sub_rp = np.zeros(len(users) + 1, np.int64)
    np.cumsum(rp[:, 1] - rp[:, 0], out=sub_rp[1:])
    sub_col = np.concatenate([hc[a:b].cpu().numpy() for a, b in rp]).astype(np.int32)
    wi, wv = oracle.score_topk(res[:U][ud].cpu().numpy(), res[U:].cpu().numpy(), (sub_rp, sub_col), 1e-6, 50, U)
    assert np.array_equal(idx[ud].cpu().numpy(), wi)
    assert np.array_equal(val[ud].cpu().numpy(), wv)
    assert bool((val[:, 1:] <= val[:, :-1]).all())
    assert int(idx.min()) >= U and int(idx.max()) < U + I
    for u0 in range(0, U, 2_000_000):                            # (row sorts in slices: a [1e7, 50] int64 sort at once is 8 GB)
        srt = idx[u0:u0 + 2_000_000].sort(1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all())


def test_captured_fused_step_equals_eager(full):
    """The step bench.py --dataset config5 times: FusedLightGCNStep captured in a hipGraph == the same launches eager."""
    from chaorec_amd.Model import LightGCN
    from chaorec_amd.optim import FusedAdam, FusedLightGCNStep
    U, I, dev = full["U"], full["I"], full["dev"]

    def make():
        m = LightGCN.__new__(LightGCN)
        torch.nn.Module.__init__(m)
        m.result, m.device, m.num_user, m.num_item = None, dev, U, I
        m.aggr_mode, m.user_item_dict, m.reg_weight, m.dim_embedding, m.n_layers = "add", None, 1e-3, D, L
        m.edge_index = None
        m.graph, m.hist = full["csr"], full["hist"]
        m.user_embedding = torch.nn.Embedding(U, D, device=dev)
        m.item_embedding = torch.nn.Embedding(I, D, device=dev)
        with torch.no_grad():
            m.user_embedding.weight.copy_(full["x"][:U])
            m.item_embedding.weight.copy_(full["x"][U:])
        m._flat = None
        m._join_tables()
        return m, FusedAdam(m.parameters(), lr=1e-3)

    edges_dev = full["edges"].to(torch.int64)
    losses = {}
    rows = torch.from_numpy(np.random.default_rng(3).choice(U + I, 100_000, replace=False)).to(dev)
    kept = {}
    for mode in ("eager", "captured"):
        m, opt = make()
        counter = torch.zeros(1, dtype=torch.int64, device=dev)
        step = FusedLightGCNStep(m, opt, batch_size=1024, edges=edges_dev, seed=42, step_dev=counter,
                                 capture=(mode == "captured"))
        losses[mode] = [float(step()) for _ in range(3)]
        kept[mode] = m._flat[rows].clone()
        del step, m, opt
        torch.cuda.empty_cache()
    assert losses["captured"] == pytest.approx(losses["eager"], rel=1e-6)
    # same kernels, same order; only the BPR backward's float atomics may differ in their last bit between two runs
    assert torch.allclose(kept["captured"], kept["eager"], rtol=0, atol=2e-6)
