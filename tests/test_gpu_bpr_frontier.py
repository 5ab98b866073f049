"""Inner steps of a k-step replay: the launch that computes the batch's rows of x_L itself (chaorec_bpr_fwd_bwd_frontier_f32)
against the dense propagate + the BPR launch over the layer tables it stands for, bit for bit, with NaN in every table row the
launch has no business reading; its in-launch draw against the BPR launch's; and the step with CHAOREC_INNER_FRONTIER=1 against
=0 after every call of a mixed sequence of replays and single steps.  Two graphs: tests/lightgcn_small_graph.py's (N = 151: a
row above the SpMM's long threshold, one past the inline entries, one of a single entry, an empty one) and one whose items have
CH - 1, CH, CH + 1 and 2 CH + 1 entries, CH the entries the launch gathers per round."""
import ctypes

import numpy as np
import pytest
import torch

import lightgcn_small_graph as small
from accept import same_bits_t

B, D, L = 8, 64, 3
W = 1.0 / (L + 1)


def _round_entries():
    from chaorec_amd import _lib
    return int(_lib.load().chaorec_bpr_frontier_round_entries())


def _edge_graph():
    """-> (edges int64 [E, 2] as (user, n_user + item), n_user, n_item): items 0 .. 3 with CH - 1, CH, CH + 1, 2 CH + 1 users,
    twenty more with 3 .. 8."""
    ch = _round_entries()
    n_user, n_item = 2 * ch + 44, 24
    rng = np.random.default_rng(2 * ch + 1)
    degs = [ch - 1, ch, ch + 1, 2 * ch + 1] + [int(rng.integers(3, 9)) for _ in range(n_item - 4)]
    pairs = [(int(u), i) for i, d in enumerate(degs) for u in rng.permutation(n_user)[:d]]
    e = np.asarray(pairs, dtype=np.int64)[rng.permutation(len(pairs))]
    e[:, 1] += n_user
    return e, n_user, n_item


# graph -> (edges, n_user, n_item, a batch with repeated users and items, a batch of distinct rows): users, positives, negatives
def _cases():
    e, u, i = _edge_graph()
    users = [int(x) for x in e[e[:, 1] == u + 3][:8, 0]]           # eight users of the longest item: rows with entries
    return {
        "small": (small.small_edges(), small.N_USER, small.N_ITEM,
                  ([small.LONG_ROW, small.LONG_ROW, small.MID_ROW, small.ONE_ROW, small.EMPTY_ROW, 11, 12, small.LONG_ROW],
                   [3, 4, 3, 8, 9, 10, 11, 3], [20, 21, 22, 23, 24, 25, 26, 20]),
                  ([small.LONG_ROW, small.MID_ROW, small.ONE_ROW, small.EMPTY_ROW, 10, 11, 12, 13],
                   [3, 4, 5, 8, 9, 10, 11, 12], [20, 21, 22, 23, 24, 25, 26, 27])),
        "edges": (e, u, i,
                  ([users[0], users[0], users[2], users[3], users[4], users[5], users[6], users[0]],
                   [0, 1, 2, 3, 3, 5, 6, 0], [3, 9, 1, 0, 2, 13, 14, 3]),
                  (users, [0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 14, 15])),
    }


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chaorec_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def worlds(dev):
    """Per graph: the CSR, x_0 .. x_L by the dense propagate, the dense adjacency (who may be read) -- computed once, never
    written again."""
    from chaorec_amd import graph, ops
    out = {}
    for name, (edges, n_user, n_item, repeats, distinct) in _cases().items():
        n = n_user + n_item
        csr = graph.lightgcn_csr(edges, n).to(dev)
        xs = [torch.randn(n, D, generator=torch.Generator().manual_seed(9)).to(dev)]
        for _ in range(L):
            xs.append(ops.spmm_raw(csr, xs[-1]))
        adj = torch.zeros(n, n, dtype=torch.bool)
        adj[edges[:, 0], edges[:, 1]] = True
        adj |= adj.t().clone()
        out[name] = dict(csr=csr, xs=xs, adj=adj.to(dev), n_user=n_user, n_item=n_item, n=n, edges=edges, repeats=repeats,
                         distinct=distinct)
    torch.cuda.synchronize()
    return out


def _assert_same(ref, new):
    for a, b in zip(ref, new):
        assert same_bits_t(a, b) if a.dtype == torch.float32 else torch.equal(a, b)


def _launch_pair(dev, wd, batch=None, poison=True, **draw):
    """-> (reference, new): workspace, coef, rows, G, bitmap, ids of the BPR launch over x_0 .. x_L and of the new launch over
    (CSR, x_0 .. x_{L-1}).  batch: given ids; else `draw` draws them in the launch."""
    from chaorec_amd import ops
    xs, n, n_user = wd["xs"], wd["n"], wd["n_user"]
    tabs = xs[:L]
    if batch is not None:
        ids0 = [torch.tensor(c, dtype=torch.int64, device=dev) for c in batch]
        if poison:       # x_{L-1}: NaN outside R0 + nbr(R0); the earlier tables: NaN outside R0
            r0 = torch.zeros(n, dtype=torch.bool, device=dev)
            r0[torch.cat([ids0[0], ids0[1] + n_user, ids0[2] + n_user])] = True
            n1 = r0 | wd["adj"][r0].any(0)
            nan = torch.full_like(xs[0], float("nan"))
            tabs = [torch.where((n1 if l == L - 1 else r0)[:, None], xs[l], nan) for l in range(L)]
    else:
        ids0 = [torch.zeros(B, dtype=torch.int64, device=dev) for _ in range(3)]
    out = []
    for new in (False, True):
        ids = tuple(t.clone() for t in ids0)
        G = torch.zeros(n, D, device=dev)
        coef, ws = torch.empty(B, device=dev), torch.empty(4 * B, device=dev)
        rows = torch.full((3 * B, D), float("nan"), device=dev)
        bits = ops.row_bitmap(n, dev)
        kw = dict(num_user=n_user, num_item=wd["n_item"], row_bits=bits, **draw)
        if new:
            ops.bpr_fwd_bwd_frontier(wd["csr"], tabs, W, rows, n_user, G, B, ops.VARIANT_LOG_SIGMOID_EPS, 1e-3, coef, ws, ids, **kw)
        else:
            ops.bpr_fwd_bwd(None, n_user, G, B, ops.VARIANT_LOG_SIGMOID_EPS, 1e-3, coef, ws, ids, layer_tabs=xs, layer_w=W,
                            rows=rows, **kw)
        torch.cuda.synchronize()
        out.append([ws, coef, rows, G, bits, *ids])
    assert bool(out[0][3].any()) and not bool(torch.isnan(out[0][2]).any())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "edges"])
def test_frontier_launch_ordered_mode_repeated_rows(dev, worlds, name):
    """The suite's ordered gradient launch: every bit is fixed, repeated users and items included."""
    import os
    assert os.environ.get("CHAOREC_BPR_ORDERED") == "2"
    wd = worlds[name]
    deg = wd["adj"].sum(1)
    if name == "small":
        assert [int(deg[r]) for r in (small.LONG_ROW, small.MID_ROW, small.ONE_ROW, small.EMPTY_ROW)] == [40, 9, 1, 0]
    else:
        ch = _round_entries()
        assert [int(deg[wd["n_user"] + i]) for i in range(4)] == [ch - 1, ch, ch + 1, 2 * ch + 1]
        assert set(range(4)) <= set(wd["repeats"][1]) and set(range(4)) <= set(wd["distinct"][1])
    _assert_same(*_launch_pair(dev, wd, wd["repeats"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "edges"])
def test_frontier_launch_atomic_mode_distinct_rows(dev, worlds, name, monkeypatch):
    """The in-launch atomic adds: bits are fixed where no row receives two contributions."""
    monkeypatch.setenv("CHAOREC_BPR_ORDERED", "0")
    wd = worlds[name]
    rows = list(wd["distinct"][0]) + [wd["n_user"] + i for i in wd["distinct"][1] + wd["distinct"][2]]
    assert len(set(rows)) == 3 * B
    _assert_same(*_launch_pair(dev, wd, wd["distinct"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "edges"])
@pytest.mark.parametrize("with_perm", [False, True])
def test_frontier_launch_draws_the_bpr_launchs_batch(dev, worlds, name, with_perm):
    """Same seed, step, device step counter, read position and offset: the same ids (and everything computed from them)."""
    from chaorec_amd import graph
    wd = worlds[name]
    edges_dev = torch.from_numpy(wd["edges"]).to(dev)
    hist = tuple(t.to(dev) for t in graph.user_hist_csr_from_edges(wd["edges"], wd["n_user"]))
    draw = dict(edges=edges_dev, hist=hist, seed=11, step=2, step_dev=torch.tensor([5], dtype=torch.int64, device=dev))
    if with_perm:
        g = torch.Generator().manual_seed(3)
        draw.update(perm=torch.randperm(len(wd["edges"]), generator=g).to(dev),
                    perm_pos=torch.tensor([17], dtype=torch.int64, device=dev), pos_offset=2 * B)
    ref, new = _launch_pair(dev, wd, **draw)
    u, p = ref[5].cpu().numpy(), ref[6].cpu().numpy()
    assert {(int(a), int(b) + wd["n_user"]) for a, b in zip(u, p)} <= {tuple(map(int, e)) for e in wd["edges"]}
    if with_perm:
        want = wd["edges"][draw["perm"].cpu().numpy()[17 + 2 * B:17 + 3 * B]]
        assert np.array_equal(u, want[:, 0]) and np.array_equal(p + wd["n_user"], want[:, 1])
    _assert_same(ref, new)


def test_frontier_argument_checks():
    """Refused before anything is launched (made-up addresses: the host reads the pointer array only)."""
    from chaorec_amd import _lib
    lib = _lib.load()
    p, q = 4096, 8192

    def call(n_tabs=3, rows=q, tabs=(p, p, p, p), D=64, mode=0, rowptr=p, col=p, val=p, coef=q):
        arr = (ctypes.c_void_p * len(tabs))(*tabs)
        return lib.chaorec_bpr_fwd_bwd_frontier_f32(ctypes.cast(arr, ctypes.c_void_p), n_tabs, 0.25, 90, rows, rowptr, col, val,
                                                    151, mode, None, 0, None, None, 90, 61, 0, 0, None, p, p, p, 8, D, 0, 1e-3,
                                                    None, None, None, coef, q, None, None, 0, q, q, None, 0.9, 0.999, None, None,
                                                    0, None)

    err = r"^chaorec_bpr_fwd_bwd_frontier_f32 failed \(-1\): .*"
    for d in (32, 128):
        with pytest.raises(RuntimeError, match=err + "built for D = 64"):
            call(D=d)
    for n_tabs in (0, 4):
        with pytest.raises(RuntimeError, match=err + "layer tables"):
            call(n_tabs=n_tabs)
    with pytest.raises(RuntimeError, match=err + "NULL rows buffer"):
        call(rows=None)
    for k in ("rowptr", "col", "val"):
        with pytest.raises(RuntimeError, match=err + "NULL graph arrays"):
            call(**{k: None})
    with pytest.raises(RuntimeError, match=err + "NULL table 1"):
        call(tabs=(p, None, p))
    with pytest.raises(RuntimeError, match=err + "dynamic values"):
        call(mode=1)
    with pytest.raises(RuntimeError, match=err + "16-byte aligned"):
        call(tabs=(p, p, p + 4))
    with pytest.raises(RuntimeError, match=err + "NULL argument"):
        call(coef=None)
    assert _round_entries() % 16 == 0 and _round_entries() * 256 <= 40 * 1024


def test_inner_frontier_mode_truth_table(monkeypatch):
    from chaorec_amd.optim import _inner_frontier_mode
    ok = dict(inner_mean_rows=True, D=64, dynamic_values=False, batch_size=1024, n_rows=44147, longest_row=624, round_entries=128)
    off_by_rule = [dict(batch_size=3679), dict(longest_row=32 * 128 + 1)]          # 12 B = 44 148 > N; 33 rounds
    not_built = [dict(inner_mean_rows=False), dict(D=128), dict(dynamic_values=True)]
    monkeypatch.delenv("CHAOREC_INNER_FRONTIER", raising=False)
    assert _inner_frontier_mode(**ok) is True
    assert _inner_frontier_mode(**{**ok, "batch_size": 3678, "longest_row": 32 * 128}) is True
    for mode, want_rule, want_unbuilt in (("auto", False, False), ("1", True, False), ("0", False, False)):
        monkeypatch.setenv("CHAOREC_INNER_FRONTIER", mode)
        assert _inner_frontier_mode(**ok) is (mode != "0")
        for change in off_by_rule:
            assert _inner_frontier_mode(**{**ok, **change}) is want_rule, (mode, change)
        for change in not_built:
            assert _inner_frontier_mode(**{**ok, **change}) is want_unbuilt, (mode, change)


@pytest.mark.gpu
@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("name", ["small", "edges"])
def test_step_with_the_frontier_launch_equals_step_without(dev, name, capture, monkeypatch):
    """Two replays of three steps, a single step, one more replay (capture=False: four steps): table, moments, losses,
    counters and model.result after every call; G and R0's bitmap all-zero between calls."""
    from chaorec_amd import graph
    from chaorec_amd.Model import LightGCN
    from chaorec_amd.optim import FusedAdam, FusedLightGCNStep
    edges, n_user, n_item = _cases()[name][:3]
    edges_dev = torch.from_numpy(edges).to(dev)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CHAOREC_INNER_FRONTIER", mode)
        torch.manual_seed(0)
        m = LightGCN(n_user, n_item, edges, graph.user_item_dict_from_edges(edges), D, 1e-3, L, "add", dev).to(dev)
        o = FusedAdam(m.parameters(), lr=1e-3)
        acc = torch.zeros(1, dtype=torch.float32, device=dev)
        step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        step = FusedLightGCNStep(m, o, batch_size=B, edges=edges_dev, seed=11, step_dev=step_dev, loss_accum=acc,
                                 capture=capture, steps_per_replay=3)
        assert step.few_src and not step.light
        assert step.inner_mean_rows == capture and step.inner_frontier == (mode == "1" and capture)
        snaps = []
        for single in (False, False, True, False):
            step(single=single)
            torch.cuda.synchronize()
            assert not bool(step.G.any()) and not bool(step._few_bits.any())
            snaps.append([t.clone() for t in (m._flat, step.m, step.v, acc, step.static_loss, step_dev, o._step_dev, m.result)])
        assert int(o._step_dev) == (10 if capture else 4)
        out[mode] = snaps
    for s0, s1 in zip(out["0"], out["1"]):
        _assert_same(s0, s1)
