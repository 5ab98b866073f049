"""DRAGON's user-graph kernels (csrc/usergraph.hip through chaorec_amd/ops_extra.py) and Model/DRAGON.py on the MI355X, against
the integer / float64 restatements of tests/dragon_host.py and the reference fixtures of tests/golden/gen_dragon.py.

build: exact in idx / cnt / len on a seeded U = 300, I = 257 structure (make_structure: every special row is asserted on the
host restatement), bit-identical with three ragged tiles, twice over dirtied outputs, and on a sparse graph one tile and
1234 users long; on the real baby graph under the id rule of dragon_host.check_ids.
sample: indices exact against the numpy uint64 restatement of the generator, weights within 4 ulp of the fp64 softmax.
aggregation: every output within the forward error bound of an ordered fp32 sum of n rounded products,
(n + 2) 2^-24 sum |addends| per element (dragon_host.aggregate_fwd / aggregate_bwd), never a measured tolerance.
  Largest deviation / bound measured on the MI355X over the 16 shapes (1.0 = at the bound): out 0.46 (U=300 k=1), dv 0.45,
  dt 0.48, dw 0.014; test_aggregate prints every figure.
model: within 4 x the reference's own stored fp32-vs-fp64 deviation (read from the fixture); measured 0.16 x (loss) .. 1.33 x
  (the gradient of t_gcn.MLP_1.weight)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dragon_host as dh  # noqa: E402
from accept import within  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = dh.TOPN


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def make_structure():
    """U = 300, I = 257.  User 0 holds nothing; user 1 holds item 256 alone; item 0 is held by users 2 .. 251 (250 holders:
    four passes of a wave, rows with 249+ neighbours); users 252 / 253 / 254 hold only item 1 / 2 / 3 together with 199 /
    200 / 201 of the users 2 .. 251 (exactly that many neighbours, every count 1: user 254's cut falls inside a run of
    equal counts); users 255 / 256 hold only item 4 and 257 .. 260 only item 5 (1 and 3 neighbours); everyone else holds 2 .. 6 of
    the items 10 .. 255."""
    U, I = 300, 257
    rng = np.random.default_rng(20261018)
    pairs = {(1, 256)}
    for u in range(2, 252):
        pairs.add((u, 0))
    for u, item, n in ((252, 1, 199), (253, 2, 200), (254, 3, 201)):
        pairs.add((u, item))
        for v in rng.choice(np.arange(2, 252), size=n, replace=False).tolist():
            pairs.add((int(v), item))
    for u, item in ((255, 4), (256, 4), (257, 5), (258, 5), (259, 5), (260, 5)):    # 1 and 3 neighbours: padded at every k > 3
        pairs.add((u, item))
    for u in list(range(2, 252)) + list(range(261, U)):
        for i in rng.choice(np.arange(10, 256), size=int(rng.integers(2, 7)), replace=False).tolist():
            pairs.add((u, int(i)))
    e = np.array(sorted(pairs), dtype=np.int64)
    e[:, 1] += U
    return U, I, e


@pytest.fixture(scope="module")
def small():
    U, I, edges = make_structure()
    rowptr, col = dh.history_csr(edges, U)
    C = dh.cooccurrence(rowptr, col, U, I)
    idx, cnt, length = dh.topn(C, N)
    nnz = np.diff(C.indptr)
    assert nnz[0] == 0 and rowptr[1] == rowptr[0]                       # no interactions
    assert nnz[1] == 0 and rowptr[2] - rowptr[1] == 1                   # one item nobody else holds
    assert (nnz[252], nnz[253], nnz[254]) == (199, 200, 201) and (nnz[255], nnz[257]) == (1, 3)
    assert nnz.max() > N and np.bincount(col)[0] == 250
    cut_in_run = [u for u in range(U) if nnz[u] > N and np.sort(C.data[C.indptr[u]:C.indptr[u + 1]])[::-1][N - 1]
                  == np.sort(C.data[C.indptr[u]:C.indptr[u + 1]])[::-1][N]]
    assert 254 in cut_in_run and len(cut_in_run) > 1
    assert any(cnt[u, 0] > cnt[u, N - 1] for u in cut_in_run)           # ... below larger counts that are all taken
    return dict(U=U, I=I, edges=edges, rowptr=rowptr, col=col, C=C, idx=idx, cnt=cnt, len=length)


def _build(dev, rowptr, col, I, tile_users=0, out=None):
    from chaorec_amd import ops_extra
    s = ops_extra.usergraph_build(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), I, n=N, tile_users=tile_users, out=out)
    torch.cuda.synchronize()
    return s


def _host(s):
    return s.nbr_idx.cpu().numpy(), s.nbr_cnt.cpu().numpy(), s.nbr_len.cpu().numpy()


def test_build_small_exact(dev, small):
    got = _host(_build(dev, small["rowptr"], small["col"], small["I"]))
    for name, g, w in zip(("idx", "cnt", "len"), got, (small["idx"], small["cnt"], small["len"])):
        assert np.array_equal(g, w), f"{name}: {int((g != w).sum())} entries differ"


def test_build_tiles_and_dirty_outputs(dev, small):
    from chaorec_amd import ops_extra
    U, I = small["U"], small["I"]
    assert ops_extra.usergraph_tile_users(U, 128) == 128 and ops_extra.usergraph_tile_users(U) == U   # 128 + 128 + 44
    one = _host(_build(dev, small["rowptr"], small["col"], I))
    three = _host(_build(dev, small["rowptr"], small["col"], I, tile_users=128))
    for a, b in zip(one, three):
        assert np.array_equal(a, b), "three tiles differ from one"
    for fill in (-1, 0x7FFFFFFF):
        out = (torch.full((U, N), fill, dtype=torch.int32, device=dev), torch.full((U, N), fill, dtype=torch.int32, device=dev),
               torch.full((U,), fill, dtype=torch.int32, device=dev))
        again = _host(_build(dev, small["rowptr"], small["col"], I, tile_users=128, out=out))
        for a, b in zip(one, again):
            assert np.array_equal(a, b), "a run over dirtied outputs differs"


def test_build_past_one_tile(dev):
    from chaorec_amd import ops_extra
    tile = ops_extra.usergraph_tile_users(1 << 20)
    U, I = tile + 1234, 9973
    u = np.arange(U, dtype=np.int64)
    edges = np.concatenate((np.stack((u, U + u % I), 1), np.stack((u, U + (u * 7 + 3) % I), 1)))
    rowptr, col = dh.history_csr(edges, U)
    idx, cnt, length = dh.topn(dh.cooccurrence(rowptr, col, U, I), N)
    assert length.max() < N and (idx[:tile] >= tile).any() and (idx[tile:] < tile).any()   # neighbours across the tile edge
    got = _host(_build(dev, rowptr, col, I))
    for name, g, w in zip(("idx", "cnt", "len"), got, (idx, cnt, length)):
        assert np.array_equal(g, w), f"{name}: {int((g != w).sum())} entries differ"


def test_build_rejects(dev, small):
    from chaorec_amd import ops_extra
    rp, col = torch.from_numpy(small["rowptr"]).to(dev), torch.from_numpy(small["col"]).to(dev)
    with pytest.raises(ValueError):
        ops_extra.usergraph_build(rp, col, small["I"], n=257)
    with pytest.raises(ValueError):
        ops_extra.usergraph_build(rp, col.to(torch.int64), small["I"])
    with pytest.raises(RuntimeError):       # the library's invalid-argument status beyond the documented largest U
        from chaorec_amd import _lib
        from chaorec_amd.ops import _ptr, _stream
        _lib.load().chaorec_usergraph_build(_ptr(rp), _ptr(col), _ptr(rp), _ptr(col), ops_extra.usergraph_max_users() + 1, small["I"],
                                            N, 0, _ptr(col), _ptr(col), _ptr(col), _stream())


# ---- sample ----------------------------------------------------------------------------------------------------------------
def _ulp_ok(got32, want64, ulps=4):
    want32 = want64.astype(np.float32)
    return np.abs(got32.astype(np.float64) - want64) <= ulps * np.spacing(np.abs(want32)).astype(np.float64)


@pytest.mark.parametrize("k", [1, 10, 40, 200])
def test_sample(dev, small, k):
    from chaorec_amd import ops_extra
    U = small["U"]
    s = _build(dev, small["rowptr"], small["col"], small["I"])
    seed, epoch = 0x1234567890ABCDEF, 3
    e_idx, e_w = (t.cpu().numpy().copy() for t in ops_extra.usergraph_sample(s, k, seed, epoch))
    w_idx, w_w, src, r = dh.sample(small["idx"], small["cnt"], small["len"], k, seed, epoch)
    full, empty = small["len"] >= k, small["len"] == 0
    padded = ~full & ~empty
    assert full.any() and empty.any() and (padded.any() or k == 1)
    assert np.array_equal(e_idx[full], small["idx"][full, :k])
    assert np.array_equal(e_idx, w_idx), "an index differs from the restated generator"
    for u in np.nonzero(padded)[0]:                                  # every padded slot copies the restated earlier slot
        for j in range(int(small["len"][u]), k):
            assert 0 <= r[u, j] < j and e_idx[u, j] == e_idx[u, r[u, j]]
    assert _ulp_ok(e_w, w_w).all(), "a weight is more than 4 ulp from the fp64 softmax"
    assert not e_idx[empty].any() and not e_w[empty].any()
    # the reverse structure = a stable host sort
    rev_ptr, rev_slot = dh.reverse(e_idx, U)
    assert np.array_equal(s.rev_ptr.cpu().numpy(), rev_ptr) and np.array_equal(s.rev_slot.cpu().numpy(), rev_slot)
    assert np.array_equal(s.rev_u.cpu().numpy(), rev_slot // k) and np.array_equal(s.rev_w.cpu().numpy(), e_w.reshape(-1)[rev_slot])
    # a pure function of (seed, epoch), in the same buffers
    ptrs = (s.epoch_idx.data_ptr(), s.epoch_w.data_ptr(), s.rev_ptr.data_ptr(), s.rev_u.data_ptr(), s.rev_w.data_ptr())
    other = ops_extra.usergraph_sample(s, k, seed, epoch + 1)[0].cpu().numpy().copy()
    assert ptrs == (s.epoch_idx.data_ptr(), s.epoch_w.data_ptr(), s.rev_ptr.data_ptr(), s.rev_u.data_ptr(), s.rev_w.data_ptr())
    if padded.any() and k > 2:
        assert not np.array_equal(other, e_idx), "another epoch drew the same graph"
    s.epoch_idx.fill_(-7)
    s.epoch_w.fill_(float("nan"))
    a_idx, a_w = (t.cpu().numpy() for t in ops_extra.usergraph_sample(s, k, seed, epoch))
    assert np.array_equal(a_idx, e_idx) and np.array_equal(a_w.view(np.int32), e_w.view(np.int32))


# ---- aggregation -------------------------------------------------------------------------------------------------------------
def _agg_inputs(U, k, D, seed):
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((U, D)) * np.exp(rng.uniform(-2, 2, (U, 1)))).astype(np.float32)
    t = (rng.standard_normal((U, D)) * np.exp(rng.uniform(-2, 2, (U, 1)))).astype(np.float32)
    wu = rng.uniform(-1, 1, (U, 2, 1)).astype(np.float32)
    idx = rng.integers(0, U, (U, k)).astype(np.int32)
    w = rng.uniform(0, 1, (U, k)).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    idx[0, :] = idx[0, 0]                      # a row that repeats a neighbour (k > 1) ...
    idx[U // 2, 0] = U // 2                    # ... one that names itself
    w[U - 1, :] = 0.0                          # ... one whose weights are all zero
    if U > 70:
        idx[1:72, k - 1] = 5                  # user 5 is neighbour to more than 64 others: an owner list longer than a wave
    g = (rng.standard_normal((U, 2 * D)) * np.exp(rng.uniform(-2, 2, (U, 1)))).astype(np.float32)
    return v, t, wu, idx, w, g


AGG_CASES = [(U, k, 64) for U in (1, 63, 64, 65, 300) for k in (1, 10, 40)] + [(65, 10, 128)]
_worst = {}


@pytest.mark.parametrize("U,k,D", AGG_CASES)
def test_aggregate(dev, U, k, D):
    from chaorec_amd import ops_extra
    v, t, wu, idx, w, g = _agg_inputs(U, k, D, 1000 * U + 10 * k + D)
    if U > 70:
        assert np.bincount(idx.reshape(-1), minlength=U)[5] > 64
    if k > 1:
        assert len(set(idx[0].tolist())) == 1
    assert idx[U // 2, 0] == U // 2 and not w[U - 1].any()
    s = ops_extra.UserGraphStructure(*(torch.zeros(sh, dtype=torch.int32, device=dev) for sh in ((U, 1), (U, 1), (U,))))
    s.set_epoch(torch.from_numpy(idx).to(dev), torch.from_numpy(w).to(dev))
    want, mag, n = dh.aggregate_fwd(v, t, wu, idx, w)
    (w_dv, w_dt, w_dw), (b_dv, b_dt, b_dw), n_b = dh.aggregate_bwd(g, v, t, wu, idx, w)
    runs = []
    for fill in (float("nan"), 1e30):
        tv, tt, tw = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (v, t, wu))
        torch.full((4 * U, 2 * D), fill, device=dev)           # junk where the allocator will hand out the outputs
        torch.cuda.synchronize()
        out = ops_extra.usergraph_aggregate(tv, tt, tw, s)
        out.backward(torch.from_numpy(g).to(dev))
        torch.cuda.synchronize()
        runs.append([a.detach().cpu().numpy() for a in (out, tv.grad, tt.grad, tw.grad)])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "two runs differ in their bits"
    out, dv, dt, dw = runs[0]
    assert dw.shape == wu.shape
    checks = (("out", out, want, (n + 2) * dh.EPS32 * mag), ("dv", dv, w_dv, b_dv), ("dt", dt, w_dt, b_dt),
              ("dw", dw.reshape(U, 2), w_dw, b_dw))
    for name, got, ref, bound in checks:
        err = np.abs(got.astype(np.float64) - ref)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        _worst[name] = max(_worst.get(name, 0.0), ratio)
        print(f"aggregate U={U} k={k} D={D} {name}: max |err| / bound = {ratio:.3f} (n = {n if name == 'out' else n_b})")
        assert (err <= bound).all(), f"{name}: {ratio:.3f} x the bound"
    print("largest deviation / bound so far:", {a: round(b, 3) for a, b in _worst.items()})


def test_aggregate_rejects(dev):
    from chaorec_amd import ops_extra
    U, k = 8, 2
    s = ops_extra.UserGraphStructure(*(torch.zeros(sh, dtype=torch.int32, device=dev) for sh in ((U, 1), (U, 1), (U,))))
    s.set_epoch(torch.zeros((U, k), dtype=torch.int32, device=dev), torch.zeros((U, k), device=dev))
    ok = lambda D=64: torch.zeros((U, D), device=dev)   # noqa: E731
    wu = torch.zeros((U, 2, 1), device=dev)
    ops_extra.usergraph_aggregate(ok(), ok(), wu, s)
    with pytest.raises(ValueError):
        ops_extra.usergraph_aggregate(ok().double(), ok(), wu, s)
    with pytest.raises(ValueError):
        ops_extra.usergraph_aggregate(torch.zeros((U, 128), device=dev)[:, ::2], ok(), wu, s)
    with pytest.raises(ValueError):
        ops_extra.usergraph_aggregate(ok(96), ok(96), wu, s)
    with pytest.raises(ValueError):
        ops_extra.usergraph_aggregate(ok(), ok(), torch.zeros((U, 3), device=dev), s)


# ---- the reference fixture on the real baby graph -------------------------------------------------------------------------------
def test_build_baby_against_the_reference(dev):
    g = np.load(os.path.join(GOLDEN, "baby_interactions.npz"))
    f = dh.load_fixture(GOLDEN, "dragon_usergraph_baby.npz")
    U, I = int(g["U"]), int(g["I"])
    rowptr, col = dh.history_csr(g["train"], U)
    idx, cnt, length = _host(_build(dev, rowptr, col, I))
    assert np.array_equal(length, f["len"].astype(np.int32))                         # all 12 351 users: len ...
    off = np.concatenate(([0], np.cumsum(f["len"].astype(np.int64))))
    keep = np.arange(N)[None, :] < length[:, None]
    assert np.array_equal(cnt[keep], f["counts"].astype(np.int32))                   # ... and the count sequence
    assert not idx[~keep].any() and not cnt[~keep].any()
    C = dh.cooccurrence(rowptr, col, U, I)
    ioff = np.concatenate(([0], np.cumsum(f["len"][f["id_users"]].astype(np.int64))))
    cut = 0
    for n, u in enumerate(f["id_users"].astype(np.int64)):
        ref_ids, ref_counts = f["ids"][ioff[n]:ioff[n + 1]], f["counts"][off[u]:off[u + 1]]
        assert dh.check_ids(u, ref_ids, ref_counts, C) is None
        bad = dh.check_ids(u, idx[u, :length[u]], cnt[u, :length[u]], C)
        assert bad is None, bad
        ours, theirs, last = idx[u, :length[u]], ref_ids.astype(np.int64), ref_counts[-1] if len(ref_counts) else 0
        assert set(ours[cnt[u, :length[u]] > last].tolist()) == set(theirs[ref_counts > last].tolist())
        if C.indptr[u + 1] - C.indptr[u] <= N:
            assert set(ours.tolist()) == set(theirs.tolist())
        else:
            cut += 1
    assert cut > 0, "none of the stored users is cut at 200"


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _new_model(c, dev):
    from chaorec_amd.Model import DRAGON
    DRAGON.user_graph_path = None                       # no .npy: the user graph is built on the device from the edges
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"])
    m = DRAGON(c["U"], c["I"], c["edges"], dh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
               dh.DIM, dh.DIM, dh.REG_WEIGHT, dh.N_LAYERS, dh.II_TOPK, dh.UU_TOPK, dh.MM_IMAGE_WEIGHT, "add", dev)
    return m.to(dev)


@pytest.fixture(scope="module")
def case(dev):
    c = dh.small_case()
    f = dh.load_fixture(GOLDEN, "dragon_small.npz")
    w = dh.init_weights(c)
    U, I = c["U"], c["I"]
    want = dh.step(w, c["v_feat"], c["t_feat"], c["edges"], U, I, f["epoch_idx"], f["epoch_w"], c["users"], c["pos"] - U, c["neg"] - U,
                   dh.REG_WEIGHT, dh.N_LAYERS, f["knn_v"], f["knn_t"], dh.MM_IMAGE_WEIGHT)
    return c, f, w, want


def test_model_initial_state(dev, case):
    c, f, w, _ = case
    m = _new_model(c, dev)
    sd = m.state_dict()
    assert tuple(sd.keys()) == dh.NAMES
    for n in dh.NAMES:                                  # same seed => the weights the reference drew (the fixture's probes)
        assert tuple(sd[n].shape) == w[n].shape and np.array_equal(sd[n].cpu().numpy(), w[n]), n
    for k, n in enumerate(dh.NAMES):
        assert np.array_equal(sd[n].cpu().numpy().reshape(-1)[:f["w_probe"].shape[1]], f["w_probe"][k][:w[n].size]), n
    assert m.result.dtype == torch.float64 and tuple(m.result.shape) == (c["U"] + c["I"], dh.DIM) and "result" not in sd
    # the user graph built on the device from the edges = the restatement, hence the reference's user_graph_dict
    rowptr, col = dh.history_csr(c["edges"], c["U"])
    idx, cnt, length = dh.topn(dh.cooccurrence(rowptr, col, c["U"], c["I"]))
    for g, want in zip(_host(m.graph_structure), (idx, cnt, length)):
        assert np.array_equal(g, want)
    for name, key in (("image", "knn_v"), ("text", "knn_t")):
        assert np.array_equal(np.sort(m.knn_ind[name].cpu().numpy(), 1), f[key]), f"{name}: another kNN graph"


def test_model_reads_user_graph_dict(dev, case, tmp_path):
    """Where Data/<dataset>/user_graph_dict.npy exists (the reference's {user: [[ids], [counts]]}), it is what the model uses."""
    from chaorec_amd.Model import DRAGON
    c = case[0]
    rowptr, col = dh.history_csr(c["edges"], c["U"])
    C = dh.cooccurrence(rowptr, col, c["U"], c["I"])
    d = dh.user_graph_dict(C)
    u = int(np.argmax(np.diff(C.indptr) > 2))
    d[u] = [d[u][0][::-1], d[u][1][::-1]]               # a list no build would produce: it must come back as written
    path = str(tmp_path / "user_graph_dict.npy")
    np.save(path, d, allow_pickle=True)
    try:
        torch.manual_seed(c["seed"])
        DRAGON.user_graph_path = path
        m = DRAGON(c["U"], c["I"], c["edges"], dh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
                   dh.DIM, dh.DIM, dh.REG_WEIGHT, dh.N_LAYERS, dh.II_TOPK, dh.UU_TOPK, dh.MM_IMAGE_WEIGHT, "add", dev).to(dev)
    finally:
        DRAGON.user_graph_path = None
    idx, cnt, length = _host(m.graph_structure)
    assert m.user_graph_dict is not None and length[u] == len(d[u][0])
    assert idx[u, :length[u]].tolist() == d[u][0] and cnt[u, :length[u]].tolist() == [int(x) for x in d[u][1]]
    want = dh.topn(C)
    others = np.arange(c["U"]) != u
    assert np.array_equal(idx[others], want[0][others]) and np.array_equal(length[others], want[2][others])
    m.pre_epoch_processing()
    assert np.isfinite(float(_step(m, c).detach()))


def _step(m, c):
    m.zero_grad(set_to_none=True)
    loss = m.loss(torch.from_numpy(c["users"]), torch.from_numpy(c["pos"]), torch.from_numpy(c["neg"]))
    loss.backward()
    torch.cuda.synchronize()
    return loss


def test_model_step_against_the_reference(dev, case, oracle):
    c, f, w, want = case
    U, I = c["U"], c["I"]
    m = _new_model(c, dev)
    m.set_epoch_graph(f["epoch_idx"], f["epoch_w"])     # the epoch graph the reference's own topk_sample drew
    loss = _step(m, c)
    params = dict(m.named_parameters(remove_duplicate=False))
    assert {n for n in dh.NAMES if params[n].grad is None} == set(dh.NAMES) - set(dh.WITH_GRAD)
    figures = [("result", dh.rel_dev(m.result.detach().cpu().numpy(), want["result"]), float(f["dev_result"])),
               ("loss", dh.rel_dev(float(loss.detach()), want["loss"]), float(f["dev_loss"])),
               ("bpr", dh.rel_dev(float(m.last_bpr.detach()), want["bpr"]), float(f["dev_bpr"])),
               ("reg", dh.rel_dev(float(m.last_reg.detach()), want["reg"]), float(f["dev_reg"]))]
    for k, n in enumerate(dh.WITH_GRAD):
        figures.append(("grad " + n, dh.rel_dev(params[n].grad.cpu().numpy(), want["grads"][n]), float(f["dev_grads"][k])))
    for name, dev_here, dev_ref in figures:
        print(f"{name}: {dev_here:.3e} from fp64, the reference {dev_ref:.3e} ({dev_here / dev_ref:.2f} x)")
    for name, dev_here, dev_ref in figures:
        assert dev_here <= 4 * dev_ref, f"{name}: {dev_here:.3e} > 4 x {dev_ref:.3e}"
    # the ranking of the table this forward left
    rank = m.gene_ranklist(50)
    idx, _ = oracle.gene_ranklist(m.result.detach().cpu().numpy(), U, I, oracle.user_hist_csr(c["edges"], U), 1e-6, 50)
    assert np.array_equal(rank.numpy(), idx), "top-50 differs from the oracle's ranking of model.result"
    # the aggregation as the reference writes it (gather + matmul in plain torch) instead of the fused node
    m.fused_aggregation = False
    plain = _step(m, c)
    within("plain aggregation, loss", float(plain.detach()), want["loss"], f["dev_loss"], 0.0)
    within("plain aggregation, result", m.result.detach().cpu().numpy(), want["result"], f["dev_result"], 0.0)


def test_model_trains_on_a_device_built_graph(dev, case):
    c = case[0]
    m = _new_model(c, dev)
    assert m.user_graph_dict is None                    # nothing was read from a file
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}     # (forward() registers the preference tables twice)
    m.pre_epoch_processing()
    first = m.epoch_user_graph.clone()
    loss = _step(m, c)
    opt.step()
    assert np.isfinite(float(loss.detach()))
    moved = {n for n, p in m.named_parameters(remove_duplicate=False) if n in before and not torch.equal(p.detach(), before[n])}
    assert {"weight_u", "v_gcn.MLP.weight", "t_gcn.MLP_1.bias"} <= moved and "MLP_user.weight" not in moved
    ptr = m.epoch_user_graph.data_ptr()
    m.pre_epoch_processing()                            # the next epoch: same buffers, another padding
    assert m.epoch_user_graph.data_ptr() == ptr and not torch.equal(m.epoch_user_graph, first)
    assert np.isfinite(float(_step(m, c).detach()))
