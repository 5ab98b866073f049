"""DualGNN's fused node (dg_fuse_fwd / dg_fuse_bwd of csrc/usergraph.hip through ops_extra.dualgnn_fuse) and Model/DualGNN.py on
the MI355X, against the float64 restatements of tests/dualgnn_host.py and the reference fixture of tests/golden/gen_dualgnn.py.

node: every output within the derived per-element bound of an ordered fp32 evaluation (dualgnn_host.fuse_fwd / fuse_bwd:
  (n + 4) 2^-24 sum |w| (|a| |v| + |b| |t|) forward, DRAGON's construction backward), never a measured tolerance; twice over
  dirtied allocator memory with identical bits.  D = 64 puts 16 rows in a workgroup and 4 in a wave, D = 128 8 and 2: the
  shapes put the user / item boundary inside a wave (U 1, 15, 17, 65), on a wave edge (U 300 = 75 waves) and on a workgroup
  edge (U 16), with no item row, one, and a ragged last workgroup.  test_fuse prints every error / bound ratio.
  Largest deviation / bound measured on the MI355X over the 56 shapes (1.0 = at the bound): result's user rows 0.43, dv 0.52,
  dt 0.49, dw 0.018; result's item rows are one rounding against a bound of half an ulp and reach it (1.00).
model: result, the loss parts and the twelve gradients within 4 x max(the reference's own stored fp32-vs-fp64 deviation,
  2^-24), both with the fused node and with the reference's lines in plain torch; measured 0.41 x (bpr) .. 1.11 x (the
  gradient of v_gcn.MLP_1.weight)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dragon_host as dh  # noqa: E402
import dualgnn_host as gh  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
def _fuse_inputs(U, I, k, D, seed):
    """test_gpu_dragon._agg_inputs over whole [U + I, D] tables, plus one index outside [0, U) under a non-zero weight."""
    rng = np.random.default_rng(seed)
    N = U + I
    v = (rng.standard_normal((N, D)) * np.exp(rng.uniform(-2, 2, (N, 1)))).astype(np.float32)
    t = (rng.standard_normal((N, D)) * np.exp(rng.uniform(-2, 2, (N, 1)))).astype(np.float32)
    wu = rng.uniform(-1, 1, (U, 2, 1)).astype(np.float32)
    idx = rng.integers(0, U, (U, k)).astype(np.int32)
    w = rng.uniform(0, 1, (U, k)).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    idx[0, :] = idx[0, 0]                      # a row that repeats a neighbour (k > 1) ...
    idx[U // 2, 0] = U // 2                    # ... one that names itself
    w[U - 1, :] = 0.0                          # ... one whose weights are all zero
    if U > 70:
        idx[1:72, k - 1] = 5                  # user 5 is neighbour to more than 64 others: an owner list longer than a wave
    # ... and a slot that names no user: the first item row where there is one, else -1.  It must be skipped, not read.
    oor = (U // 3, 0) if U >= 4 else (U - 1, k - 1)
    idx[oor] = U if I > 0 else -1
    g = (rng.standard_normal((N, D)) * np.exp(rng.uniform(-2, 2, (N, 1)))).astype(np.float32)
    return v, t, wu, idx, w, g, oor


FUSE_CASES = ([(U, I, k, 64) for U in (1, 15, 16, 17, 65, 300) for I in (0, 1, 37) for k in (1, 10, 40)]
              + [(7, 10, 10, 128), (65, 0, 10, 128)])
_worst = {}


@pytest.mark.parametrize("U,I,k,D", FUSE_CASES)
def test_fuse(dev, U, I, k, D):
    from chaorec_amd import ops_extra
    v, t, wu, idx, w, g, oor = _fuse_inputs(U, I, k, D, 100000 * D + 1000 * U + 50 * I + k)
    N = U + I
    if U > 70:
        assert np.bincount(idx[(idx >= 0) & (idx < U)], minlength=U)[5] > 64
    if k > 1 and U >= 4:
        assert len(set(idx[0].tolist())) == 1
    if U >= 4:
        assert idx[U // 2, 0] == U // 2 and w[oor[0], oor[1]] > 0 and len({0, U // 2, U - 1, oor[0]}) == 4
    assert not w[U - 1].any() and not 0 <= idx[oor] < U
    s = _structure(dev, U, idx, w)
    want, b_out, n = gh.fuse_fwd(v, t, wu, idx, w, U)
    (w_dv, w_dt, w_dw), (b_dv, b_dt, b_dw), n_b = gh.fuse_bwd(g, v, t, wu, idx, w, U)
    runs = []
    for fill in (float("nan"), 1e30):
        tv, tt, tw = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (v, t, wu))
        torch.full((4 * N, D), fill, device=dev)                # junk where the allocator will hand out the outputs
        torch.full((U, 2, 1), fill, device=dev)
        torch.cuda.synchronize()
        out = ops_extra.dualgnn_fuse(tv, tt, tw, s, U)
        out.backward(torch.from_numpy(g).to(dev))
        torch.cuda.synchronize()
        runs.append([a.detach().cpu().numpy() for a in (out, tv.grad, tt.grad, tw.grad)])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "two runs differ in their bits"
    out, dv, dt, dw = runs[0]
    assert out.shape == (N, D) and dv.shape == (N, D) and dt.shape == (N, D) and dw.shape == wu.shape
    if I > 0:                                                   # an item row hands g on unchanged, to both tables
        assert np.array_equal(dv[U:], g[U:]) and np.array_equal(dt[U:], g[U:])
    checks = [("out", out[:U], want[:U], b_out[:U]), ("dv", dv, w_dv, b_dv), ("dt", dt, w_dt, b_dt), ("dw", dw.reshape(U, 2), w_dw, b_dw)]
    if I > 0:                                                   # (one rounding: its bound is half an ulp, reached by design)
        checks.append(("out, item rows", out[U:], want[U:], b_out[U:]))
    for name, got, ref, bound in checks:
        err = np.abs(got.astype(np.float64) - ref)
        ratio = float(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0).max())
        _worst[name] = max(_worst.get(name, 0.0), ratio)
        print(f"fuse U={U} I={I} k={k} D={D} {name}: max |err| / bound = {ratio:.3f} (n = {n if name.startswith('out') else n_b})")
        assert (err <= bound).all(), f"{name}: {ratio:.3f} x the bound"
    print("largest deviation / bound so far:", {a: round(b, 3) for a, b in _worst.items()})


def test_fuse_rejects(dev):
    from chaorec_amd import _lib, ops_extra
    from chaorec_amd.ops import _ptr, _stream
    U, I, k = 8, 4, 2
    N = U + I
    s = _structure(dev, U, np.zeros((U, k), dtype=np.int32), np.zeros((U, k), dtype=np.float32))
    ok = lambda D=64, n=N: torch.zeros((n, D), device=dev)   # noqa: E731
    wu = torch.zeros((U, 2, 1), device=dev)
    assert tuple(ops_extra.dualgnn_fuse(ok(), ok(), wu, s, U).shape) == (N, 64)
    assert tuple(ops_extra.dualgnn_fuse(ok(n=U), ok(n=U), wu.view(U, 2), s, U).shape) == (U, 64)      # N == U, weight_u [U, 2]
    with pytest.raises(ValueError):
        ops_extra.dualgnn_fuse(ok().double(), ok(), wu, s, U)
    with pytest.raises(ValueError):
        ops_extra.dualgnn_fuse(torch.zeros((N, 128), device=dev)[:, ::2], ok(), wu, s, U)
    with pytest.raises(ValueError):
        ops_extra.dualgnn_fuse(ok(96), ok(96), wu, s, U)
    with pytest.raises(ValueError):
        ops_extra.dualgnn_fuse(ok(), ok(128), wu, s, U)                          # v and t of different widths
    with pytest.raises(ValueError):
        ops_extra.dualgnn_fuse(ok(), ok(), torch.zeros((U, 3), device=dev), s, U)
    with pytest.raises(ValueError):
        ops_extra.dualgnn_fuse(ok(), ok(), torch.zeros((N, 2, 1), device=dev), s, U)
    with pytest.raises(ValueError):
        ops_extra.dualgnn_fuse(ok(n=U - 1), ok(n=U - 1), wu, s, U)               # N < U
    with pytest.raises(ValueError):
        ops_extra.dualgnn_fuse(ok(), ok(), wu, _structure(dev, U), U)            # no epoch graph
    out = ok()
    with pytest.raises(RuntimeError, match="dualgnn_fuse_fwd"):                  # the library's invalid-argument status: N < U
        _lib.load().chaorec_dualgnn_fuse_fwd_f32(_ptr(out), _ptr(out), _ptr(wu), _ptr(s.epoch_idx), _ptr(s.epoch_w), U, U - 1, k, 64,
                                                 _ptr(out), _stream())
    with pytest.raises(RuntimeError, match="dualgnn_fuse_bwd"):                  # ... and D = 96
        _lib.load().chaorec_dualgnn_fuse_bwd_f32(_ptr(out), _ptr(out), _ptr(out), _ptr(wu), _ptr(s.rev_ptr), _ptr(s.rev_u),
                                                 _ptr(s.rev_w), U, N, 96, _ptr(out), _ptr(out), _ptr(wu), _stream())


# ---- the model -----------------------------------------------------------------------------------------------------------------
def _new_model(c, dev, path=None):
    from chaorec_amd.Model import DualGNN
    DualGNN.user_graph_path = path                      # None: the user graph is built on the device from the edges
    try:
        torch.manual_seed(c["seed"])
        np.random.seed(c["seed"])
        m = DualGNN(c["U"], c["I"], c["edges"], dh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
                    gh.DIM, gh.DIM, gh.REG_WEIGHT, gh.UU_TOPK, "add", dev)
    finally:
        DualGNN.user_graph_path = None
    return m.to(dev)


def _host(s):
    return s.nbr_idx.cpu().numpy(), s.nbr_cnt.cpu().numpy(), s.nbr_len.cpu().numpy()


@pytest.fixture(scope="module")
def case(dev):
    c = dh.small_case()
    f = dh.load_fixture(GOLDEN, "dualgnn_small.npz")
    w = gh.init_weights(c)
    U, I = c["U"], c["I"]
    want = gh.step(w, c["v_feat"], c["t_feat"], c["edges"], U, I, f["epoch_idx"], f["epoch_w"], c["users"], c["pos"] - U, c["neg"] - U,
                   gh.REG_WEIGHT)
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
    assert tuple(sd.keys()) == gh.NAMES
    for k, n in enumerate(gh.NAMES):                    # same seed => the weights the reference drew (the fixture's probes)
        assert tuple(sd[n].shape) == w[n].shape and np.array_equal(sd[n].cpu().numpy(), w[n]), n
        assert np.array_equal(sd[n].cpu().numpy().reshape(-1)[:f["w_probe"].shape[1]], f["w_probe"][k][:w[n].size]), n
    assert m.result.dtype == torch.float64 and tuple(m.result.shape) == (c["U"] + c["I"], gh.DIM) and "result" not in sd
    assert m.construction == "weighted_sum" and m.user_aggr_mode == "softmax" and m.k == gh.UU_TOPK
    # the user graph built on the device from the edges = the restatement, hence the reference's user_graph_dict
    rowptr, col = dh.history_csr(c["edges"], c["U"])
    idx, cnt, length = dh.topn(dh.cooccurrence(rowptr, col, c["U"], c["I"]))
    assert m.user_graph_dict is None
    for g, want in zip(_host(m.graph_structure), (idx, cnt, length)):
        assert np.array_equal(g, want)


def test_model_reads_user_graph_dict(dev, case, tmp_path):
    """Where Data/<dataset>/user_graph_dict.npy exists (the reference's {user: [[ids], [counts]]}), it is what the model uses."""
    c = case[0]
    rowptr, col = dh.history_csr(c["edges"], c["U"])
    C = dh.cooccurrence(rowptr, col, c["U"], c["I"])
    d = dh.user_graph_dict(C)
    u = int(np.argmax(np.diff(C.indptr) > 2))
    d[u] = [d[u][0][::-1], d[u][1][::-1]]               # a list no build would produce: it must come back as written
    path = str(tmp_path / "user_graph_dict.npy")
    np.save(path, d, allow_pickle=True)
    m = _new_model(c, dev, path)
    idx, cnt, length = _host(m.graph_structure)
    assert m.user_graph_dict is not None and length[u] == len(d[u][0])
    assert idx[u, :length[u]].tolist() == d[u][0] and cnt[u, :length[u]].tolist() == [int(x) for x in d[u][1]]
    want = dh.topn(C)
    others = np.arange(c["U"]) != u
    assert np.array_equal(idx[others], want[0][others]) and np.array_equal(length[others], want[2][others])
    m.pre_epoch_processing()
    assert np.isfinite(float(_step(m, c).detach()))


def test_model_step_against_the_reference(dev, case, oracle):
    c, f, w, want = case
    U, I = c["U"], c["I"]
    floor = lambda d: max(float(d), gh.EPS32)   # noqa: E731  (an elementwise gradient's stored deviation can be zero)
    m = _new_model(c, dev)
    m.set_epoch_graph(f["epoch_idx"], f["epoch_w"])     # the epoch graph the reference's own topk_sample drew
    loss = _step(m, c)
    params = dict(m.named_parameters(remove_duplicate=False))
    assert {n for n in gh.NAMES if params[n].grad is None} == {"MLP_v.weight", "MLP_t.weight", "MLP_user.weight", "MLP_user.bias"}
    assert tuple(m.result.shape) == (U + I, gh.DIM) and m.result.dtype == torch.float32
    figures = [("result", dh.rel_dev(m.result.detach().cpu().numpy(), want["result"]), floor(f["dev_result"])),
               ("loss", dh.rel_dev(float(loss.detach()), want["loss"]), floor(f["dev_loss"])),
               ("bpr", dh.rel_dev(float(m.last_bpr.detach()), want["bpr"]), floor(f["dev_bpr"])),
               ("reg", dh.rel_dev(float(m.last_reg.detach()), want["reg"]), floor(f["dev_reg"]))]
    for k, n in enumerate(gh.WITH_GRAD):
        figures.append(("grad " + n, dh.rel_dev(params[n].grad.cpu().numpy(), want["grads"][n]), floor(f["dev_grads"][k])))
    for name, dev_here, dev_ref in figures:
        print(f"{name}: {dev_here:.3e} from fp64, the reference (floored at 2^-24) {dev_ref:.3e} ({dev_here / dev_ref:.2f} x)")
    for name, dev_here, dev_ref in figures:
        assert dev_here <= 4 * dev_ref, f"{name}: {dev_here:.3e} > 4 x {dev_ref:.3e}"
    # the ranking of the table this forward left
    rank = m.gene_ranklist(50)
    idx, _ = oracle.gene_ranklist(m.result.detach().cpu().numpy(), U, I, oracle.user_hist_csr(c["edges"], U), 1e-6, 50)
    assert np.array_equal(rank.numpy(), idx), "top-50 differs from the oracle's ranking of model.result"
    # the reference's lines in plain torch instead of the fused node
    m.fused_aggregation = False
    plain = _step(m, c)
    d_loss, d_res = dh.rel_dev(float(plain.detach()), want["loss"]), dh.rel_dev(m.result.detach().cpu().numpy(), want["result"])
    print(f"plain torch: loss {d_loss:.3e}, result {d_res:.3e} from fp64")
    assert d_loss <= 4 * floor(f["dev_loss"]) and d_res <= 4 * floor(f["dev_result"])


def test_model_trains_on_a_device_built_graph(dev, case):
    c = case[0]
    m = _new_model(c, dev)
    assert m.user_graph_dict is None                    # nothing was read from a file
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}     # (forward() registers the preference tables twice)
    m.pre_epoch_processing()
    first = m.epoch_user_graph.clone()
    ptr = (m.epoch_user_graph.data_ptr(), m.user_weight_matrix.data_ptr())
    loss = _step(m, c)
    opt.step()
    assert np.isfinite(float(loss.detach()))
    m.pre_epoch_processing()                            # the next epoch: same buffers, another padding
    assert (m.epoch_user_graph.data_ptr(), m.user_weight_matrix.data_ptr()) == ptr and not torch.equal(m.epoch_user_graph, first)
    loss = _step(m, c)
    opt.step()
    assert np.isfinite(float(loss.detach()))
    moved = {n for n, p in m.named_parameters(remove_duplicate=False) if n in before and not torch.equal(p.detach(), before[n])}
    assert {"weight_u", "weight_i", "v_gcn.MLP.weight"} <= moved and "MLP_user.weight" not in moved


def test_model_mean_weights(dev, case):
    """user_aggr_mode = 'mean': 1 / k wherever the user has a neighbour, the rows without stay zero, the reverse list follows."""
    c = case[0]
    m = _new_model(c, dev)
    m.user_aggr_mode = "mean"
    m.pre_epoch_processing()
    s, k = m.graph_structure, gh.UU_TOPK
    has = (s.nbr_len > 0).cpu().numpy()
    w = m.user_weight_matrix.cpu().numpy()
    assert has.any() and not has.all()
    assert np.array_equal(w[has], np.full((int(has.sum()), k), np.float32(1.0) / np.float32(k))) and not w[~has].any()
    assert np.array_equal(s.rev_w.cpu().numpy(), w.reshape(-1)[s.rev_slot.cpu().numpy()])
    assert np.isfinite(float(_step(m, c).detach()))
