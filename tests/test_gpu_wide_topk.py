"""Rank lists past 64 columns on the MI355X (csrc/topk_wide.hip, the wave-per-row kernel of csrc/metrics.hip): staged exact
scores + wide row selection against the oracle bit for bit, the first 64 columns against the narrow route, the range loop,
ops.score_rows alone against the oracle's whole rows (both store paths, the pad columns left alone), ops.rows_topk alone
against a numpy sort by the same bit-pattern key (accept.numpy_topk), the metrics up to k = 1024 against the python loops, four
models' gene_ranklist(topk=100) and the training loop's --topk 20 100.

Shapes: the smallest at which each path is taken -- I = K and K + 1 (a row that is all winners / one loser), item counts that
are no multiple of the 32-item tile or of the 256-element chunk, one user group and several (33, 100 users), every D class of
the scoring kernel (8: shortest register fragment, 64 and 128: the register-resident ones, 192: the streamed one), K that is no
power of two (padding of the sort) and K = 1024 (none)."""
import numpy as np
import pytest
import torch

from accept import bits, numpy_topk, to_dev
from chaorec_amd import ops, ranking, utils

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def t(x, dtype=None):
    return to_dev(x, dtype, DEV)


def history(rng, U, I, per_user=12):
    """A user-history CSR (rowptr int64, col int32 ascending, local item ids); among several users the second has none."""
    rows = [np.sort(rng.choice(I, size=min(I, int(rng.integers(1, per_user + 1))), replace=False)) if u != 1 else np.zeros(0, np.int64)
            for u in range(U)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = (np.concatenate(rows) if rowptr[-1] else np.zeros(0)).astype(np.int32)
    return rowptr, col


def embeddings(rng, U, I, D, regime):
    if regime == "a":
        # Gaussian x 0.2; a constant column pair shifts every score by -1.5, so most are negative and the history's 1e-6
        # entries lie inside the top-K
        ue = (rng.standard_normal((U, D)) * 0.2).astype(np.float32)
        ie = (rng.standard_normal((I, D)) * 0.2).astype(np.float32)
        ue[:, 0], ie[:, 0] = 1.0, -1.5
        return ue, ie
    # small integers: a score is one of a few dozen integers, whole groups of items tie and the K-th boundary cuts a group
    return (rng.integers(-1, 2, (U, D)).astype(np.float32), rng.integers(-1, 2, (I, D)).astype(np.float32))


def case(U, I, D, regime, seed):
    rng = np.random.default_rng(seed)
    ue, ie = embeddings(rng, U, I, D, regime)
    return ue, ie, history(rng, U, I)


def device_call(ue, ie, hist, K, id_offset, **kw):
    idx, val = ops.score_topk(t(ue), t(ie), (t(hist[0]), t(hist[1])), 1e-6, K, id_offset=id_offset, **kw)
    return idx.cpu().numpy(), val.cpu().numpy()


# (U, I, D, K, regime): every U, I class, D and K of the list, not their product
CASES = [(1, 65, 8, 65, "a"), (33, 66, 64, 65, "b"), (100, 1300, 128, 128, "a"), (33, 1300, 192, 200, "b"),
         (100, 201, 64, 200, "a"), (100, 6407, 64, 1000, "a"), (33, 1001, 8, 1000, "b"), (1, 1024, 128, 1024, "a"),
         (33, 1025, 64, 1024, "a"), (100, 6407, 192, 1024, "b"), (33, 6407, 8, 128, "b"), (1, 1300, 192, 65, "a")]


@pytest.mark.parametrize("U,I,D,K,regime", CASES)
def test_wide_score_topk_equals_the_oracle_bit_for_bit(oracle, U, I, D, K, regime):
    ue, ie, hist = case(U, I, D, regime, seed=U * 7 + I + D + K)
    ref_idx, ref_val = oracle.score_topk(ue, ie, hist, 1e-6, K, U)
    if regime == "a":
        assert (ref_val == np.float32(1e-6)).any(), "the masked entries are meant to be inside the top-K"
    elif I > K:
        more = oracle.score_topk(ue, ie, hist, 1e-6, K + 1, U)[1]
        assert (more[:, K - 1] == more[:, K]).any(), "the K-th boundary is meant to cut a tie group"
    stats = {}
    idx, val = device_call(ue, ie, hist, K, U, stats=stats)
    assert stats == {"wide_users": U}
    assert idx.shape == (U, K) and idx.dtype == np.int64
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(bits(val), bits(ref_val))


@pytest.mark.parametrize("regime", ["a", "b"])
def test_first_64_columns_equal_the_narrow_route(regime):
    """The new code against the parent's: columns 0..63 of the K = 65 and K = 1024 lists are the K = 64 list of the existing
    route (I >= 4096 at D = 64: the prefilter route), indices and values bit for bit."""
    U, I, D = 100, 6407, 64
    ue, ie, hist = case(U, I, D, regime, seed=5)
    idx64, val64 = device_call(ue, ie, hist, 64, U)
    for K in (65, 1024):
        idx, val = device_call(ue, ie, hist, K, U)
        assert np.array_equal(idx[:, :64], idx64), K
        assert np.array_equal(bits(val[:, :64]), bits(val64)), K


def test_user_ranges_equal_one_range():
    U, I, D, K = 100, 1300, 64, 200
    ue, ie, hist = case(U, I, D, "a", seed=9)
    ld = (I + 3) // 4 * 4
    assert ops.wide_range_users(ld, 7 * 4 * ld) == 7
    one = device_call(ue, ie, hist, K, U)
    out = torch.full((U, K), -1, dtype=torch.int64, device=DEV)
    many = device_call(ue, ie, hist, K, U, staging_bytes=7 * 4 * ld, idx_out=out)      # 14 ranges of 7 and one of 2
    assert np.array_equal(one[0], many[0]) and np.array_equal(bits(one[1]), bits(many[1]))
    assert np.array_equal(out.cpu().numpy(), one[0])
    host = torch.empty((U, K), dtype=torch.int64, pin_memory=True)
    ops.score_topk(t(ue), t(ie), (t(hist[0]), t(hist[1])), 1e-6, K, id_offset=U, idx_out=host)
    torch.cuda.synchronize()
    assert np.array_equal(host.numpy(), one[0])


SENTINEL = -12345.0


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("U,I,D", [(33, 66, 64), (100, 1001, 8), (33, 1300, 192)])
def test_score_rows_alone_equals_the_oracle_over_the_whole_block(oracle, U, I, D, offset):
    """ops.score_rows without the selection behind it: every staged score, not only the ones a top-K list shows.  The oracle
    sorts whole rows, so K = I returns all of them; scattered back by index they are the block.  offset 1: `out` starts one
    float off a 16-byte boundary, the scalar store path of score_rows_kernel."""
    ue, ie, hist = case(U, I, D, "a", seed=U + I + D)
    idx, val = oracle.score_topk(ue, ie, hist, 1e-6, I, 0)
    assert np.array_equal(np.sort(idx, axis=1), np.broadcast_to(np.arange(I), (U, I)))
    ref = np.empty((U, I), np.float32)
    np.put_along_axis(ref, idx, val, 1)
    in_hist = np.zeros((U, I), bool)
    for u in range(U):
        in_hist[u, hist[1][hist[0][u]:hist[0][u + 1]]] = True
    assert in_hist.any() and np.array_equal(bits(ref[in_hist]), bits(np.full(in_hist.sum(), 1e-6, np.float32)))
    ld = (I + 3) // 4 * 4                                   # 68, 1004 and 1300: two cases have pad columns
    buf = torch.full((U * ld + 4,), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[offset:offset + U * ld]
    assert (out.data_ptr() % 16 == 0) == (offset == 0)
    sc = ops.score_rows(t(ue), t(ie), (t(hist[0]), t(hist[1])), 1e-6, 0, U, out=out, ld=ld)
    assert sc.data_ptr() == out.data_ptr() and tuple(sc.shape) == (U, ld)
    got, whole = sc.cpu().numpy(), buf.cpu().numpy()
    assert np.array_equal(bits(got[:, :I]), bits(ref))
    assert np.array_equal(bits(got[in_hist.nonzero()]), bits(ref[in_hist]))              # (the masked entries, said out loud)
    assert (got[:, I:] == SENTINEL).all(), "a pad column was written"
    assert (whole[:offset] == SENTINEL).all() and (whole[offset + U * ld:] == SENTINEL).all()


def test_wide_call_leaves_hints_and_counters_alone():
    U, I, D, K = 33, 1300, 64, 100
    ue, ie, hist = case(U, I, D, "a", seed=2)
    hint = torch.full((U,), 7.0, device=DEV)
    counters = torch.full((4,), 9, dtype=torch.int32, device=DEV)
    a = device_call(ue, ie, hist, K, U, hint=hint, hint_valid=True, light=True, counters=counters, precision=2)
    b = device_call(ue, ie, hist, K, U)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    assert bool((hint == 7.0).all()) and bool((counters == 9).all())
    with pytest.raises(RuntimeError):
        device_call(ue[:, :8], ie[:100, :8], (hist[0], hist[1][:0]), 101, U)      # K > I, as the narrow route


# ---------------------------------------------------------------------------------------------- ops.rows_topk alone
@pytest.mark.parametrize("n,I,K,pad", [(129, 257, 100, 2), (1, 128, 128, 3), (129, 201, 200, 2), (1, 8449, 1024, 2),
                                       (129, 8449, 1000, 4), (129, 1025, 1024, 0), (1, 257, 65, 0)])
def test_rows_topk_wide_against_numpy(n, I, K, pad):
    rng = np.random.default_rng(n + I + K)
    x = rng.standard_normal((n, I)).astype(np.float32)
    x[0] = 0.25                                             # all equal: columns 0 .. K - 1
    if n > 3:
        tie = min(500, I - (K - 1))                         # exactly K - 1 values above a tie group (of 500 where the row holds it)
        x[1] = -3.0
        where = rng.permutation(I)
        x[1, where[:K - 1]] = 2.0 + rng.random(K - 1).astype(np.float32)
        x[1, where[K - 1:K - 1 + tie]] = 1.0
        x[2, :4] = [0.0, -0.0, np.inf, -np.inf]
        x[3, 5:9] = [-0.0, 0.0, -np.inf, np.inf]
    ld = I + pad + (1 - (I + pad) % 2 if pad else 0)        # pad > 0: ld != I and odd
    buf = torch.zeros(n * ld + 1, dtype=torch.float32, device=DEV)
    sc = buf[1:] if pad else buf[:-1]                       # (and then the block starts 4 bytes off a 16-byte boundary)
    sc = sc.view(n, ld)[:, :I]
    sc.copy_(t(x))
    assert (sc.stride(0) != I and sc.stride(0) % 2 == 1) or not pad
    idx, val = ops.rows_topk(sc, K, id_offset=11)
    ref_idx, ref_val = numpy_topk(x, K)
    assert np.array_equal(ref_idx[0], np.arange(K))
    assert np.array_equal(idx.cpu().numpy(), ref_idx + 11)
    assert np.array_equal(bits(val.cpu().numpy()), bits(ref_val))
    again = ops.rows_topk(sc, K, id_offset=11)
    assert torch.equal(idx, again[0]) and torch.equal(val.view(torch.int32), again[1].view(torch.int32))


def test_rows_topk_dispatch_and_messages():
    x = torch.randn(3, 300, device=DEV)
    with pytest.raises(ValueError, match=r"macrid: topk=0 \(1 \.\. min\(64, I=300\)\)"):
        ops.rows_topk(x, 0)
    with pytest.raises(ValueError, match="1024"):
        ops.rows_topk(torch.randn(2, 2000, device=DEV), 1025)
    with pytest.raises(ValueError):
        ops.rows_topk(x, 301)
    i64, v64 = ops.rows_topk(x, 64)
    i65, v65 = ops.rows_topk(x, 65)
    assert torch.equal(i65[:, :64], i64) and torch.equal(v65[:, :64], v64)


# ---------------------------------------------------------------------------------------------- metrics
def metric_lists(K, I, U=300):
    rng = np.random.default_rng(3)
    rank_np = np.stack([rng.permutation(I)[:K] for _ in range(U)]).astype(np.int64) + U
    rank_np[5, 3] = rank_np[5, 1]                       # duplicate id inside a ranked list
    rank_np[6, :4] = rank_np[6, 0]
    if K > 64:
        rank_np[5, 700] = rank_np[5, 1]                 # ... across mask words
        rank_np[7, 1000] = rank_np[7, 999]
        rank_np[8, 64] = rank_np[8, 63]
    data = []
    for u in rng.permutation(U)[:250]:
        n = int(rng.integers(0, 6))
        pos = list((rng.integers(0, I, n) + U).tolist())
        if n and rng.random() < 0.3:
            pos.append(pos[0])                          # duplicate positive
        if rng.random() < 0.5 and n:
            pos[0] = int(rank_np[u, rng.integers(0, K)])   # make hits likely, at any depth
        data.append([int(u)] + pos)
    data.append([5, int(rank_np[5, 1])])
    data.append([6, int(rank_np[6, 0]), int(rank_np[6, 9])])
    if K > 64:
        data.append([7, int(rank_np[7, 999])])
        data.append([8, int(rank_np[8, 63]), int(rank_np[8, 1023])])
    return rank_np, data


def test_rank_metrics_up_to_1024(oracle):
    rank_np, data = metric_lists(1024, 1500)
    ks = [1, 50, 64, 65, 100, 1000, 1024]
    ref = oracle.gene_metrics(data, rank_np, ks)
    got = utils.gene_metrics_device(utils.EvalLists(data, DEV), t(rank_np), ks)
    again = utils.gene_metrics_device(utils.EvalLists(data, DEV), t(rank_np), ks)
    for k in ks:
        for n in ref[k]:
            print(k, n, got[k][n], ref[k][n])
            assert got[k][n] == pytest.approx(ref[k][n], rel=1e-12, abs=1e-15), (k, n)
            assert got[k][n] == again[k][n]             # fixed-order reduction
    with pytest.raises(RuntimeError):
        ops.rank_metrics(t(rank_np), t([0]), t([0, 0]), t([0]), [1025])


# precision, recall, ndcg, hit_rate, map of metric_lists(64, 400) at k = 1, 5, 10, 20, 50, 64 as the parent commit's
# chaorec_rank_metrics_f64 returned them (float.hex of the [6, 5] fp64 output, read back from the MI355X)
PARENT_64 = [
    ['0x1.8618618618618p-7', '0x1.0410410410410p-7', '0x1.8618618618618p-7', '0x1.8618618618618p-7', '0x1.0410410410410p-7'],
    ['0x1.d41d41d41d41ep-7', '0x1.fc3518a6dfc35p-6', '0x1.e97a2d0c1bdfap-6', '0x1.2492492492492p-4', '0x1.8eed331775bbbp-6'],
    ['0x1.9319319319319p-7', '0x1.66210cbb76621p-5', '0x1.253dbc1d47602p-5', '0x1.a69a69a69a69ap-4', '0x1.bac55ff138c73p-6'],
    ['0x1.8c98c98c98c99p-7', '0x1.5fe5fe5fe5fe7p-4', '0x1.9a504c87dca92p-5', '0x1.b6db6db6db6dbp-3', '0x1.ec54b97c3fcc9p-6'],
    ['0x1.8618618618618p-7', '0x1.ac6d7181c2c6ep-3', '0x1.517663b999b18p-4', '0x1.cb2cb2cb2cb2dp-2', '0x1.1afb3d93aa6acp-5'],
    ['0x1.9861861861862p-7', '0x1.2256256256255p-2', '0x1.967d21dcc25f6p-4', '0x1.228a28a28a28ap-1', '0x1.296772c26abc7p-5']]


def test_rank_metrics_narrow_lists_keep_their_bits():
    rank_np, data = metric_lists(64, 400)
    ks = [1, 5, 10, 20, 50, 64]
    lists = utils.EvalLists(data, DEV)
    out = ops.rank_metrics(t(rank_np), lists.row_user, lists.rowptr, lists.items, ks).cpu().numpy()
    got = [[float(v).hex() for v in row] for row in out]
    print(got)
    assert got == PARENT_64


# ---------------------------------------------------------------------------------------------- models
def small_lightgcn(seed=1):
    from chaorec_amd import graph
    from chaorec_amd.Model import LightGCN
    from chaorec_amd.synthetic import synthetic_interactions
    U, I, E = 200, 300, 1500
    edges = synthetic_interactions(U, I, E, seed=5)
    uid = graph.user_item_dict_from_edges(edges)
    torch.manual_seed(seed)
    m = LightGCN(U, I, edges, uid, 64, 1e-3, 2, "add", DEV).to(DEV)
    return m, edges, uid


def check_prefix(m, **kw):
    U = m.num_user
    r100 = m.gene_ranklist(topk=100, to_cpu=False, **kw)
    r50 = m.gene_ranklist(topk=50, to_cpu=False, **kw)
    assert r100.is_cuda and r100.dtype == torch.int64 and tuple(r100.shape) == (U, 100)
    assert torch.equal(r100[:, :50], r50)
    assert all(len(set(row)) == 100 for row in r100.cpu().tolist())
    return r100


def test_lightgcn_top_100(oracle):
    m, edges, _ = small_lightgcn()
    with torch.no_grad():
        m.forward()
    r100 = check_prefix(m)
    hist = oracle.user_hist_csr(edges, m.num_user)
    ref, _ = oracle.gene_ranklist(m.result.detach().cpu().numpy(), m.num_user, m.num_item, hist, 1e-6, 100)
    assert np.array_equal(r100.cpu().numpy(), ref)
    host = m.gene_ranklist(topk=100)
    assert not host.is_cuda and host.dtype == torch.int64 and np.array_equal(host.numpy(), ref)
    # a narrow call after the wide ones finds the RankState as a fresh model's: same list, and what it left in the state
    fresh, _, _ = small_lightgcn()
    with torch.no_grad():
        fresh.forward()
    w, _, _ = small_lightgcn()
    with torch.no_grad():
        w.forward()
    w.gene_ranklist(topk=100, to_cpu=False)
    st = ranking.state_of(w)
    assert st.hint is None and not st.valid and st.copied is None
    a, b = fresh.gene_ranklist(topk=50, to_cpu=False), w.gene_ranklist(topk=50, to_cpu=False)
    assert torch.equal(a, b)
    sf = ranking.state_of(fresh)
    assert (sf.valid, sf.last_hinted, sf.last_light) == (st.valid, st.last_hinted, st.last_light)


def test_multvae_top_100():
    import multvae_host as mh
    from conftest import load_golden
    from chaorec_amd.Model import MultVAE
    g = load_golden("multvae_small.npz")
    torch.manual_seed(int(g["seed"]))
    m = MultVAE(int(g["U"]), int(g["I"]), g["edges"], mh.user_item_dict(g["edges"]), 64, float(g["reg_weight"]), DEV)
    eps = torch.randn(int(g["U"]), ops.MULTVAE_LATENT, device=DEV)
    check_prefix(m, eps=eps)


def test_macridvae_top_100():
    import macridvae_host as mh
    from conftest import load_golden
    from chaorec_amd.Model import MacridVAE
    g = load_golden("macridvae_small.npz")
    torch.manual_seed(int(g["seed"]))
    m = MacridVAE(int(g["U"]), int(g["I"]), g["edges"], mh.user_item_dict(g["edges"]), int(g["D"]), 0.0, DEV)
    check_prefix(m)


def test_bspm_top_100():
    import bspm_host as bh
    from conftest import GOLDEN
    from chaorec_amd.Model import BSPM
    g = bh.load_fixture(GOLDEN)
    edges, I = g["edges"].astype(np.int64), int(g["I"])
    K_s, T_s, beta = bh.CASES[0]
    m = BSPM(bh.U, I, edges, bh.user_item_dict(edges), K_s, T_s, 1, 1, beta, "cuda", factor_dim=bh.FACTOR, factors=g["Vi"], fused=True)
    check_prefix(m)


# ---------------------------------------------------------------------------------------------- the loop
def test_loop_reports_recall_at_100_of_100_columns(oracle):
    from chaorec_amd import dataload
    from chaorec_amd.optim import FusedAdam
    from chaorec_amd.train_and_evaluate import train_and_evaluate
    m, edges, uid = small_lightgcn(seed=3)
    U, I = m.num_user, m.num_item
    rng = np.random.default_rng(4)
    seen = {(int(u), int(i)) for u, i in edges}
    val, test = [], []
    for u in range(U):
        free = [i for i in rng.permutation(I)[:40] + U if (u, int(i)) not in seen]
        val.append([u] + [int(i) for i in free[:2]])
        test.append([u] + [int(i) for i in free[2:5]])
    loader = dataload.DeviceBatchSampler(U, I, uid, edges, 256, DEV, "LightGCN", 7)
    opt = FusedAdam([{"params": m.parameters(), "lr": 1e-3}])
    h = []
    train_and_evaluate(m, loader, np.array(val, dtype=object), np.array(test, dtype=object), opt, 1, model_name="LightGCN",
                       topk=(20, 100), patience=10 ** 6, graph=False, history=h)
    assert len(h) == 1
    hist = oracle.user_hist_csr(edges, U)
    ref_rank, _ = oracle.gene_ranklist(m.result.detach().cpu().numpy(), U, I, hist, 1e-6, 100)
    ref = oracle.gene_metrics(test, ref_rank, [20, 100])
    short = oracle.gene_metrics(test, ref_rank[:, :50], [100])         # what a 50-column list reports as "@100"
    for n in ("recall", "ndcg", "precision", "map"):
        assert abs(short[100][n] - ref[100][n]) > 1e-3 * ref[100][n], n      # (the data: hits between ranks 50 and 100)
    for k in (20, 100):
        for n in ref[k]:
            print(k, n, h[0]["test"][k][n], ref[k][n])
            assert h[0]["test"][k][n] == pytest.approx(ref[k][n], rel=1e-12, abs=1e-15), (k, n)
    assert h[0]["test"][100]["recall"] != pytest.approx(short[100]["recall"], rel=1e-3)
