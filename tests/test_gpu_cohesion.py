"""COHESION's fused node (cf_fuse_fwd / cf_chunk / cf_rows of csrc/usergraph.hip through ops_extra.cohesion_fuse) and
Model/COHESION.py on the MI355X, against the restatements of tests/cohesion_host.py and the reference fixture of
tests/golden/gen_cohesion.py.

node: result, dv, dt, dh_v, dh_t BIT FOR BIT the float32 numpy restatement in the contract's order (cohesion_host.fuse_fwd32 /
  fuse_bwd32 at the same `chunk`), with and without the h tables, twice over dirtied allocator memory; and within the derived
  bound (n + 2) 2^-24 sum |addends| of the float64 restatement, which holds for any fixed order.  The forward puts 16 rows in a
  workgroup and 4 in a wave, the backward's two launches 8 chunks / 8 rows and 2 per wave: the shapes put the user / item
  boundary inside a wave (U 1, 15, 17, 65), on a wave edge (U 300) and on a workgroup edge (U 16), with no item row, one, and
  a ragged last workgroup; U 300 holds a reverse list longer than the default chunk.
chunk edges: one user named by exactly m slots for m around 0, 1, chunk, 2 chunk and 3 chunk + 7, at chunk 4 and 64;
  chunk = 0 is the single walk; two chunk sizes differ from each other within the bound only.
model: result, the loss parts and the twelve gradients within 4 x max(the reference's own stored fp32-vs-fp64 deviation,
  2^-24), both with the fused node and with the reference's lines in plain torch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dragon_host as dh  # noqa: E402
import cohesion_host as ch  # noqa: E402
from accept import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D = ch.D


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _structure(dev, U, idx=None, w=None):
    from chaorec_amd import ops_extra
    s = ops_extra.UserGraphStructure(*(torch.zeros(sh, dtype=torch.int32, device=dev) for sh in ((U, 1), (U, 1), (U,))))
    if idx is not None:
        s.set_epoch(torch.as_tensor(idx).to(dev), torch.as_tensor(w).to(dev))
    return s


# ---- the node ------------------------------------------------------------------------------------------------------------------
def _tables(rng, n, count):
    return [(rng.standard_normal((n, D)) * np.exp(rng.uniform(-2, 2, (n, 1)))).astype(np.float32) for _ in range(count)]


def _fuse_inputs(U, I, k, seed):
    """Whole [U + I, 64] tables, three [I, 64] h tables, g [U + I, 192], and an epoch graph with a row that repeats one
    neighbour, one that names itself, one with all-zero weights, a user named by more than 64 slots (U > 70) and one slot that
    names no user."""
    rng = np.random.default_rng(seed)
    N = U + I
    idr, v, t = _tables(rng, N, 3)
    h = _tables(rng, I, 3)
    g = np.concatenate(_tables(rng, N, 3), axis=1)
    idx = rng.integers(0, U, (U, k)).astype(np.int32)
    w = rng.uniform(0, 1, (U, k)).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    idx[0, :] = idx[0, 0]
    idx[U // 2, 0] = U // 2
    w[U - 1, :] = 0.0
    if U > 70:
        idx[1:72, k - 1] = 5
    oor = (U // 3, 0) if U >= 4 else (U - 1, k - 1)
    idx[oor] = U if I > 0 else -1
    return idr, v, t, h, g, idx, w, oor


def _run_node(dev, s, U, idr, v, t, h, g, chunk, fill):
    """One forward + backward over allocator memory dirtied with `fill` -> (out, dv, dt, dh_v, dh_t) on the host."""
    from chaorec_amd import ops_extra
    N = idr.shape[0]
    tid, tv, tt = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (idr, v, t))
    th = None if h is None else [torch.from_numpy(a).to(dev).requires_grad_(True) for a in h]
    torch.full((2 * N, 3 * D), fill, device=dev)                # junk where the allocator will hand out the outputs ...
    torch.full((4 * N, D), fill, device=dev)
    torch.full((U * s.k + 1, 2 * D), fill, device=dev)          # ... and the partials
    torch.cuda.synchronize()
    hh = (None, None, None) if th is None else th
    out = ops_extra.cohesion_fuse(tid, tv, tt, hh[0], hh[1], hh[2], s, U, chunk=chunk)
    out.backward(torch.from_numpy(g).to(dev))
    torch.cuda.synchronize()
    assert tid.grad is None and (th is None or th[0].grad is None)      # the id third is detached
    got = [out, tv.grad, tt.grad] + ([] if th is None else [th[1].grad, th[2].grad])
    return [a.detach().cpu().numpy() for a in got]


FUSE_CASES = [(U, I, k, with_h) for U in (1, 15, 16, 17, 65, 300) for I in (0, 1, 37) for k in (1, 10, 40)
              for with_h in ((False, True) if I > 0 else (False,))]
_worst = {}


@pytest.mark.parametrize("U,I,k,with_h", FUSE_CASES)
def test_fuse(dev, U, I, k, with_h):
    idr, v, t, h, g, idx, w, oor = _fuse_inputs(U, I, k, 1000 * U + 50 * I + k)
    h = h if with_h else None
    if U > 70:
        assert np.bincount(idx[(idx >= 0) & (idx < U)], minlength=U)[5] > 64      # a list longer than the default chunk
    if U >= 4:
        assert idx[U // 2, 0] == U // 2 and w[oor[0], oor[1]] > 0 and len({0, U // 2, U - 1, oor[0]}) == 4
    assert not w[U - 1].any() and not 0 <= idx[oor] < U
    s = _structure(dev, U, idx, w)
    chunk = 64
    want = [ch.fuse_fwd32(idr, v, t, h, idx, w, U)] + [a for a in ch.fuse_bwd32(g, idx, w, U, chunk, has_h=with_h) if a is not None]
    runs = [_run_node(dev, s, U, idr, v, t, h, g, chunk, fill) for fill in (float("nan"), 1e30)]
    names = ("result", "dv", "dt", "dh_v", "dh_t")
    for name, a, b, ref in zip(names, runs[0], runs[1], want):
        assert same_bits(a, b), f"{name}: two runs differ in their bits"
        assert same_bits(a, ref), f"{name}: differs from the float32 restatement in {int((a != ref).sum())} elements"
    # ... and against float64 within the bound of any fixed order
    out64, b_out, n = ch.fuse_fwd64(idr, v, t, h, idx, w, U)
    (dv64, dt64), (b_dv, b_dt), n_b = ch.fuse_bwd64(g, idx, w, U)
    for name, got, ref, bound in (("result", runs[0][0], out64, b_out), ("dv", runs[0][1], dv64, b_dv), ("dt", runs[0][2], dt64, b_dt)):
        err = np.abs(got.astype(np.float64) - ref)
        ratio = float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0).max())
        _worst[name] = max(_worst.get(name, 0.0), ratio)
        print(f"fuse U={U} I={I} k={k} h={with_h} {name}: max |err| / bound = {ratio:.3f} (n = {n if name == 'result' else n_b})")
        assert (err <= bound).all(), f"{name}: {ratio:.3f} x the bound"
    print("largest deviation / bound so far:", {a: round(b, 3) for a, b in _worst.items()})


def _edge_graph(U, k, m, seed):
    """[U, k] graph in which user 7 is named by exactly m slots; the other slots name the other users at random."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, U - 1, (U, k)).astype(np.int32)
    idx[idx >= 7] += 1                                           # nobody names user 7 ...
    idx.reshape(-1)[rng.choice(U * k, size=m, replace=False)] = 7   # ... but these m slots
    w = rng.uniform(0, 1, (U, k)).astype(np.float32)
    assert int((idx == 7).sum()) == m
    return idx, w


@pytest.mark.parametrize("chunk", [4, 64])
def test_chunk_edges(dev, chunk):
    from chaorec_amd import ops_extra
    U, I, k = 300, 37, 10
    rng = np.random.default_rng(chunk)
    idr, v, t = _tables(rng, U + I, 3)
    g = np.concatenate(_tables(rng, U + I, 3), axis=1)
    for m in (0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 3 * chunk + 7):
        idx, w = _edge_graph(U, k, m, 100 * chunk + m)
        s = _structure(dev, U, idx, w)
        got = _run_node(dev, s, U, idr, v, t, None, g, chunk, float("nan"))
        for name, a, ref in zip(("result", "dv", "dt"), got, [ch.fuse_fwd32(idr, v, t, None, idx, w, U)] + list(ch.fuse_bwd32(g, idx, w, U, chunk, False))):
            assert same_bits(a, ref), f"chunk {chunk}, m {m}: {name} differs from the float32 restatement"
        # the chunk index the wrapper built with tensor ops = the host's
        rev_ptr, _, row_chunk, rows, first, _ = ch.rev_chunks(idx, U, chunk)
        c = s.rev_chunks[chunk]
        assert c.n_chunks == len(rows) and c.chunk == chunk and row_chunk[8] - row_chunk[7] == -(-m // chunk)
        assert np.array_equal(c.row_chunk.cpu().numpy(), row_chunk) and np.array_equal(c.chunk_row.cpu().numpy(), rows)
        assert np.array_equal(c.chunk_first.cpu().numpy(), first) and c.chunk_row.dtype == torch.int32
        assert ops_extra.usergraph_rev_chunks(s, chunk) is s.rev_chunks[chunk]
        s.set_epoch(s.epoch_idx.clone(), s.epoch_w.clone())      # a new epoch graph drops the index of the old one
        assert s.rev_chunks == {}


def test_chunk_sizes_against_each_other(dev):
    """chunk = 0 is the single walk of the same lists; chunk 4 and chunk 64 differ from each other only within the bound."""
    U, I, k = 300, 37, 10
    rng = np.random.default_rng(5)
    idr, v, t = _tables(rng, U + I, 3)
    h = _tables(rng, I, 3)
    g = np.concatenate(_tables(rng, U + I, 3), axis=1)
    idx, w = _edge_graph(U, k, 3 * 64 + 7, 5)
    s = _structure(dev, U, idx, w)
    by_chunk = {c: _run_node(dev, s, U, idr, v, t, h, g, c, 1e30) for c in (0, 4, 64)}
    for a, ref in zip(by_chunk[0][1:], ch.fuse_bwd32(g, idx, w, U, 0)):
        assert same_bits(a, ref), "chunk = 0 differs from the single-walk restatement"
    assert set(s.rev_chunks) == {0, 4, 64} and s.rev_chunks[0].n_chunks == int((np.diff(dh.reverse(idx, U)[0]) > 0).sum())
    (dv64, dt64), (b_dv, b_dt), n = ch.fuse_bwd64(g, idx, w, U)
    assert n == 3 * 64 + 8
    for j, (ref, bound) in enumerate(((dv64, b_dv), (dt64, b_dt)), start=1):
        a, b = by_chunk[4][j].astype(np.float64), by_chunk[64][j].astype(np.float64)
        assert not np.array_equal(a[7], b[7])                    # user 7's 199 entries are summed in another order ...
        assert (np.abs(a - ref) <= bound).all() and (np.abs(b - ref) <= bound).all() and (np.abs(a - b) <= 2 * bound).all()
        assert same_bits(by_chunk[4][j][U:], by_chunk[64][j][U:])    # ... the item rows are copies
    for j in (0, 3, 4):                                          # the forward and the h gradients do not depend on chunk
        assert same_bits(by_chunk[4][j], by_chunk[64][j]) and same_bits(by_chunk[0][j], by_chunk[64][j])


def test_nan_in_the_id_columns_of_g_stays_out(dev):
    U, I, k = 65, 37, 10
    idr, v, t, h, g, idx, w, _ = _fuse_inputs(U, I, k, 11)
    s = _structure(dev, U, idx, w)
    clean = _run_node(dev, s, U, idr, v, t, h, g, 4, 1e30)
    g2 = g.copy()
    g2[:, :D] = np.nan
    for a, b in zip(_run_node(dev, s, U, idr, v, t, h, g2, 4, 1e30)[1:], clean[1:]):
        assert np.isfinite(a).all() and same_bits(a, b)


def test_fuse_rejects(dev):
    from chaorec_amd import _lib, ops_extra
    from chaorec_amd.ops import _ptr, _stream
    U, I, k = 8, 4, 2
    N = U + I
    s = _structure(dev, U, np.zeros((U, k), dtype=np.int32), np.zeros((U, k), dtype=np.float32))
    ok = lambda d=D, n=N: torch.zeros((n, d), device=dev)   # noqa: E731
    hs = [ok(n=I) for _ in range(3)]
    assert tuple(ops_extra.cohesion_fuse(ok(), ok(), ok(), *hs, s, U).shape) == (N, 3 * D)
    assert tuple(ops_extra.cohesion_fuse(ok(n=U), ok(n=U), ok(n=U), None, None, None, s, U).shape) == (U, 3 * D)      # N == U
    with pytest.raises(ValueError):
        ops_extra.cohesion_fuse(ok(), ok().double(), ok(), *hs, s, U)
    with pytest.raises(ValueError):
        ops_extra.cohesion_fuse(ok(128), ok(128), ok(128), None, None, None, s, U)                  # D = 64 only
    with pytest.raises(ValueError):
        ops_extra.cohesion_fuse(ok(), ok(), ok(), hs[0], None, hs[2], s, U)                         # the h tables come together
    with pytest.raises(ValueError):
        ops_extra.cohesion_fuse(ok(), ok(), ok(), ok(n=I + 1), ok(n=I + 1), ok(n=I + 1), s, U)
    with pytest.raises(ValueError):
        ops_extra.cohesion_fuse(ok(n=U - 1), ok(n=U - 1), ok(n=U - 1), None, None, None, s, U)      # N < U
    with pytest.raises(ValueError):
        ops_extra.cohesion_fuse(ok(), ok(), ok(), *hs, _structure(dev, U), U)                       # no epoch graph
    with pytest.raises(ValueError):
        ops_extra.usergraph_rev_chunks(s, -1)
    a, out = ok(), torch.zeros((N, 3 * D), device=dev)
    with pytest.raises(RuntimeError, match="cohesion_fuse_fwd"):                 # the library's invalid-argument status: D = 128
        _lib.load().chaorec_cohesion_fuse_fwd_f32(_ptr(a), _ptr(a), _ptr(a), None, None, None, _ptr(s.epoch_idx), _ptr(s.epoch_w), U, N, k,
                                                  128, _ptr(out), _stream())
    c = ops_extra.usergraph_rev_chunks(s, 64)
    with pytest.raises(RuntimeError, match="cohesion_fuse_bwd"):                 # ... and N < U
        _lib.load().chaorec_cohesion_fuse_bwd_f32(_ptr(out), _ptr(s.rev_ptr), _ptr(s.rev_u), _ptr(s.rev_w), _ptr(c.chunk_row),
                                                  _ptr(c.chunk_first), _ptr(c.row_chunk), c.n_chunks, 64, U, U - 1, D, _ptr(out), _ptr(a),
                                                  _ptr(a), None, None, _stream())


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _new_model(c, dev, dropout=ch.DROPOUT):
    from chaorec_amd.Model import COHESION
    COHESION.user_graph_path = None                     # the user graph is built on the device from the edges
    torch.manual_seed(c["seed"])
    np.random.seed(c["seed"])
    m = COHESION(c["U"], c["I"], c["edges"], dh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
                 ch.DIM_E, ch.REG_WEIGHT, dropout, ch.N_LAYERS, ch.MM_LAYERS, ch.II_TOPK, ch.MM_IMAGE_WEIGHT, dev)
    return m.to(dev)


@pytest.fixture(scope="module")
def case(dev):
    c = dh.small_case()
    f = dh.load_fixture(GOLDEN, "cohesion_small.npz")
    w = ch.init_weights(c)
    U, I = c["U"], c["I"]
    want = ch.step(w, c["v_feat"], c["t_feat"], c["edges"], U, I, f["epoch_idx"], f["epoch_w"], c["users"], c["pos"] - U, c["neg"] - U,
                   ch.REG_WEIGHT, ch.N_LAYERS, ch.MM_LAYERS, f["knn_v"], f["knn_t"], ch.MM_IMAGE_WEIGHT)
    return c, f, w, want


def _step(m, c):
    m.zero_grad(set_to_none=True)
    loss = m.loss(torch.from_numpy(c["users"]), torch.from_numpy(c["pos"]), torch.from_numpy(c["neg"]))
    loss.backward()
    torch.cuda.synchronize()
    return loss


def test_model_initial_state(dev, case):
    c, f, w, _ = case
    m = _new_model(c, dev)
    sd = m.state_dict()
    assert tuple(sd.keys()) == ch.NAMES
    for k, n in enumerate(ch.NAMES):                    # same seed => the weights the reference drew (the fixture's probes)
        assert tuple(sd[n].shape) == w[n].shape and np.array_equal(sd[n].cpu().numpy(), w[n]), n
        assert np.array_equal(sd[n].cpu().numpy().reshape(-1)[:f["w_probe"].shape[1]], f["w_probe"][k][:w[n].size]), n
    assert m.result_embed.dtype == torch.float64 and tuple(m.result_embed.shape) == (c["U"] + c["I"], ch.DIM_E)
    assert "result_embed" not in sd and m.k == 40 and m.dim_latent == 64
    # the item graph: the float64 kNN lists the reference's own agreed with (as sets per item)
    for name, key in (("image", "knn_v"), ("text", "knn_t")):
        assert np.array_equal(np.sort(m.knn_ind[name].cpu().numpy(), 1), f[key])
    # the user graph built on the device from the edges = the restatement, hence the reference's user_graph_dict
    rowptr, col = dh.history_csr(c["edges"], c["U"])
    s = m.graph_structure
    assert m.user_graph_dict is None
    for got, want in zip((s.nbr_idx, s.nbr_cnt, s.nbr_len), dh.topn(dh.cooccurrence(rowptr, col, c["U"], c["I"]))):
        assert np.array_equal(got.cpu().numpy(), want)


def test_model_step_against_the_reference(dev, case, oracle):
    c, f, w, want = case
    U, I = c["U"], c["I"]
    floor = lambda d: max(float(d), ch.EPS32)   # noqa: E731  (an elementwise gradient's stored deviation can be zero)
    m = _new_model(c, dev)
    m.k = ch.UU_TOPK
    m.set_epoch_graph(f["epoch_idx"], f["epoch_w"])     # the epoch graph the reference's own topk_sample drew

    def figures_of(loss):
        params = dict(m.named_parameters(remove_duplicate=False))
        assert {n for n in ch.NAMES if params[n].grad is not None} == set(ch.WITH_GRAD)
        assert tuple(m.result_embed.shape) == (U + I, 3 * D) and m.result_embed.dtype == torch.float32
        figs = [("result", dh.rel_dev(m.result_embed.detach().cpu().numpy(), want["result"]), floor(f["dev_result"])),
                ("loss", dh.rel_dev(float(loss.detach()), want["loss"]), floor(f["dev_loss"])),
                ("bpr", dh.rel_dev(float(m.last_bpr.detach()), want["bpr"]), floor(f["dev_bpr"])),
                ("reg", dh.rel_dev(float(m.last_reg.detach()), want["reg"]), floor(f["dev_reg"]))]
        for k, n in enumerate(ch.WITH_GRAD):
            figs.append(("grad " + n, dh.rel_dev(params[n].grad.cpu().numpy(), want["grads"][n]), floor(f["dev_grads"][k])))
        return figs

    for fused in (True, False):                         # the fused node, then the reference's lines in plain torch
        m.fused_aggregation = fused
        figures = figures_of(_step(m, c))
        for name, dev_here, dev_ref in figures:
            print(f"fused={fused} {name}: {dev_here:.3e} from fp64, the reference (floored at 2^-24) {dev_ref:.3e} ({dev_here / dev_ref:.2f} x)")
        for name, dev_here, dev_ref in figures:
            assert dev_here <= 4 * dev_ref, f"fused={fused} {name}: {dev_here:.3e} > 4 x {dev_ref:.3e}"
        # the ranking of the table this forward left
        rank = m.gene_ranklist(50)
        idx, _ = oracle.gene_ranklist(m.result_embed.detach().cpu().numpy(), U, I, oracle.user_hist_csr(c["edges"], U), 1e-6, 50)
        assert np.array_equal(rank.numpy(), idx), "top-50 differs from the oracle's ranking of model.result_embed"


def test_model_trains_on_a_device_built_graph(dev, case):
    c = case[0]
    m = _new_model(c, dev)
    m.k = ch.UU_TOPK
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    m.pre_epoch_processing()
    assert m.masked_adj is m.norm_adj and set(m.graph_structure.rev_chunks) == {m.bwd_chunk}
    first = m.epoch_user_graph.clone()
    ptr = (m.epoch_user_graph.data_ptr(), m.user_weight_matrix.data_ptr())
    for _ in range(2):
        loss = _step(m, c)
        opt.step()
        assert np.isfinite(float(loss.detach()))
        m.pre_epoch_processing()                        # the next epoch: same buffers, another padding
    assert (m.epoch_user_graph.data_ptr(), m.user_weight_matrix.data_ptr()) == ptr and not torch.equal(m.epoch_user_graph, first)
    # (forward() registers the two preference tables a second time, under COHESION's own v_preference / t_preference)
    moved = {n for n, p in m.named_parameters(remove_duplicate=False) if n in before and not torch.equal(p.detach(), before[n])}
    assert moved == set(ch.WITH_GRAD)


def test_model_dropout_epoch(dev, case):
    """dropout = 0.2: the epoch's graph keeps int(E 0.8) interactions, both directions, under the values of _normalize_adj_m on
    the kept set: (1e-7 + user count)^-1/2 (1e-7 + item count)^-1/2 in fp32.  Against float64: the sum rounds once (2^-24, halved
    by the root), each power is good to an ulp (2^-23) and the product rounds once: 8 x 2^-24 covers it."""
    c = case[0]
    U, I, E = c["U"], c["I"], len(c["edges"])
    m = _new_model(c, dev, dropout=0.2)
    m.k = ch.UU_TOPK
    m.pre_epoch_processing()
    adj = m.masked_adj
    keep = int(E * 0.8)
    assert adj is not m.norm_adj and adj.nnz == 2 * keep and m.norm_adj.nnz == 2 * E
    rowptr, col, val = adj.rowptr.cpu().numpy(), adj.col.cpu().numpy().astype(np.int64), adj.val.cpu().numpy()
    rows = np.repeat(np.arange(U + I), np.diff(rowptr))
    upper = rows < U
    assert upper.sum() == keep and (col[upper] >= U).all()
    kept = set(zip(rows[upper].tolist(), col[upper].tolist()))
    assert len(kept) == keep and kept <= set(map(tuple, c["edges"].tolist()))
    assert kept == set(zip(col[~upper].tolist(), rows[~upper].tolist()))          # symmetric
    deg = np.bincount(rows, minlength=U + I).astype(np.float64)
    want = np.power(1e-7 + deg[rows], -0.5) * np.power(1e-7 + deg[col], -0.5)
    assert (np.abs(val - want) <= 8 * ch.EPS32 * want).all()
    assert np.isfinite(float(_step(m, c).detach()))
    m.pre_epoch_processing()                                                      # another epoch, another kept set of the same size
    assert m.masked_adj.nnz == 2 * keep and not np.array_equal(m.masked_adj.col.cpu().numpy(), col)
