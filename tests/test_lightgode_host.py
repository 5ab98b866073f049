"""LightGODE on the host: the float64 restatements (tests/lightgode_host.py) and the CPU model against every array the
reference's own run left in tests/golden/lightgode_small.npz, the adjacency bit for bit, and the wiring.  No kernel runs here.

Tolerance (accept.within): bound = 4 x max(own, ULP24) relative to the largest magnitude of the float64 array, `own` the stored
deviation of the reference's fp32 run from its float64 run.  Every check prints deviation, own, bound and ratio."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import kernel_meta  # noqa: E402
import lightgode_host as lh  # noqa: E402
from conftest import GOLDEN, tie_aware_rank_equal  # noqa: E402

from chaorec_amd import _lib, graph, ops  # noqa: E402
from chaorec_amd.Model.LightGODE import LightGODE  # noqa: E402

NEW = ["chaorec_lightgode_bwd_f32", "chaorec_lightgode_check_shape", "chaorec_lightgode_loss_f32", "chaorec_lightgode_workspace"]


@functools.lru_cache(maxsize=None)
def case():
    g = lh.load_fixture(GOLDEN)
    return g, g["edges"].astype(np.int64)


def test_the_case_and_the_seeded_weights():
    g, edges = case()
    assert np.array_equal(edges, lh.small_case())
    users, pos = lh.small_batch(edges)
    assert np.array_equal(users, g["users"]) and np.array_equal(pos, g["pos"]) and len(users) == lh.B
    assert lh.U - 1 not in set(edges[:, 0].tolist()) and edges[:, 1].max() == lh.U + lh.I - 5
    assert lh.B - len(set(users.tolist())) >= 20 and lh.B - len(set(pos.tolist())) >= 10
    assert (users[-1], pos[-1]) == (users[0], pos[0])
    torch.manual_seed(lh.SEED)                                       # the same torch seed -> the reference's weights
    m = LightGODE(lh.U, lh.I, edges, lh.user_item_dict(edges), lh.D, lh.GAMMA, lh.T, "cpu")
    assert tuple(n for n, _ in m.named_parameters()) == ("user_embedding.weight", "item_embedding.weight")
    assert [float(p.detach().double().sum()) for p in m.parameters()] == g["w_sum_seeded"].tolist()
    su, si = lh.shifts()
    assert np.array_equal(m.user_embedding.weight.detach().numpy() + su, g["w_user"])
    assert np.array_equal(m.item_embedding.weight.detach().numpy() + si, g["w_item"])
    assert (m.train_stage, m.train_strategy, m.use_mf, m.solver) == ("pretrain", "MF_init", None, "euler")
    assert m.t.tolist() == torch.tensor([0, lh.T]).tolist() and m.gamma == lh.GAMMA and m.restore_user_e is None


def test_adjacency_bit_for_bit():
    g, edges = case()
    e = torch.from_numpy(edges)
    csr = graph.binary_sym_norm_csr(e[:, 0], e[:, 1] - lh.U, lh.U, lh.I)
    assert np.array_equal(csr.rowptr.numpy(), g["adj_rowptr"]) and np.array_equal(csr.col.numpy(), g["adj_col"])
    assert accept.same_bits(csr.val.numpy(), g["adj_val"]) and csr.symmetric
    dense = np.zeros((lh.U + lh.I,) * 2, dtype=np.float32)
    rows = np.repeat(np.arange(lh.U + lh.I), np.diff(g["adj_rowptr"]))
    dense[rows, g["adj_col"]] = g["adj_val"]
    assert np.array_equal(dense, lh.dense_adj(edges).astype(np.float32))


def test_restatements_reproduce_the_golden():
    g, edges = case()
    users, items = g["users"], g["pos"] - lh.U
    r64 = lh.reference_loss(g["w_user"], g["w_item"], users, items, lh.GAMMA, torch.float64)
    c64 = lh.closed_form(g["w_user"], g["w_item"], users, items, lh.GAMMA)
    r32 = lh.reference_loss(g["w_user"], g["w_item"], users, items, lh.GAMMA, torch.float32)
    for k in lh.PARTS + ("g_u", "g_i"):
        assert lh.rel_dev(r64[k], g[k + "64"]) < 1e-13, k
        assert lh.rel_dev(c64[k], g[k + "64"]) < 1e-12, k
        accept.within("fp32 lines, " + k, r32[k], g[k + "64"], g["own_" + k], lh.ULP)
        for gram, center in ((False, False), (True, False), (True, True)):
            c32 = lh.closed_form(g["w_user"], g["w_item"], users, items, lh.GAMMA, torch.float32, gram=gram, center=center)
            accept.within(f"fp32 closed form (gram={gram}, center={center}), " + k, c32[k], g[k + "64"], g["own_" + k], lh.ULP)
    e64 = lh.euler(lh.dense_adj(edges), np.concatenate((g["w_user"], g["w_item"])), lh.T).numpy()
    accept.within("one Euler step, float64", e64, g["sample64"], g["own_euler"], lh.ULP)
    assert lh.rel_dev(g["sample32"], g["sample64"]) == pytest.approx(float(g["own_euler"]), rel=1e-6)


def test_equal_rows_enter_the_sum_and_not_the_gradient():
    """Two samples of one id: e = 1 enters S; the pair's share of the gradient, e (z_i - z_j), is zero."""
    W = torch.randn(5, lh.D, dtype=torch.float64)
    z = torch.nn.functional.normalize(W[torch.tensor([0, 1, 1, 2])], dim=-1)
    E = lh.pair_weights(z)
    assert float(E[1, 2]) == 1.0 and float(E[2, 1]) == 1.0 and float(E[1, 1]) == 0.0
    c = lh.closed_form(W, W, [0, 1, 1, 2], [3, 4, 4, 0], 0.5)
    r = lh.reference_loss(W, W, [0, 1, 1, 2], [3, 4, 4, 0], 0.5, torch.float64)
    for k in lh.PARTS + ("g_u", "g_i"):
        assert lh.rel_dev(c[k], r[k]) < 1e-12, k


def test_cpu_model_is_the_reference():
    g, edges = case()
    m = lh.new_model(g).train()
    users, pos = torch.from_numpy(g["users"]), torch.from_numpy(g["pos"])
    loss = m.loss(users, pos, pos)
    loss.backward()
    assert m.use_mf is True
    accept.within("cpu model, loss", loss.detach(), g["loss64"], g["own_loss"], lh.ULP)
    accept.within("cpu model, g_u", m.user_embedding.weight.grad, g["g_u64"], g["own_g_u"], lh.ULP)
    accept.within("cpu model, g_i", m.item_embedding.weight.grad, g["g_i64"], g["own_g_i"], lh.ULP)
    _, parts = m.loss_parts(users, pos - lh.U)
    for k, name in enumerate(lh.PARTS):
        accept.within("cpu model, " + name, parts[k], g[name + "64"], g["own_" + name], lh.ULP)
    x, y = m(users, pos - lh.U)
    assert float(m.alignment(x, y).detach()) == float(parts[1]) and float(m.uniformity(x).detach()) == float(parts[2])
    m.eval()
    assert m.restore_user_e is None
    with torch.no_grad():
        m.use_mf = m._strategy_use_mf(False)
        assert m.use_mf is False
        tab = torch.cat(m.get_all_embeddings())
    accept.within("cpu model, eval-mode tables", tab, g["sample64"], g["own_euler"], lh.ULP)
    # the stored lists agree with the masked scores of the stored tables
    s64 = lh.masked_scores(g["sample64"][:lh.U], g["sample64"][lh.U:], edges)
    s32 = lh.masked_scores(g["sample32"][:lh.U], g["sample32"][lh.U:], edges)
    atol = accept.bound_of(g["own_scores"], lh.ULP) * float(np.abs(s64).max())
    ok, why = tie_aware_rank_equal(g["ranks32"], lh.rank_values(s32, g["ranks32"]), g["ranks64"], lh.rank_values(s64, g["ranks64"]), atol=atol)
    assert ok, why
    want = np.argsort(-s64, axis=1, kind="stable")[:, :lh.TOPK] + lh.U
    ok, why = tie_aware_rank_equal(want, lh.rank_values(s64, want), g["ranks64"], lh.rank_values(s64, g["ranks64"]))
    assert ok, why


def test_strategies():
    g, _ = case()
    m = lh.new_model(g)
    for strategy, training, want in (("MF_init", True, True), ("MF_init", False, False), ("MF", False, True), ("GODE", True, False)):
        m.train_strategy = strategy
        m.train(training)
        assert m._strategy_use_mf(True) is want and m._strategy_use_mf(False) is want, (strategy, training)
    m.train_strategy = "GODE"
    m.train()
    users, pos = torch.from_numpy(g["users"]), torch.from_numpy(g["pos"])
    m.loss(users, pos, pos).backward()                      # through the Euler step
    assert m.use_mf is False and float(m.user_embedding.weight.grad.abs().sum()) > 0
    m.restore_user_e = m.restore_item_e = torch.zeros(1)
    m.loss(users, pos, pos)
    assert m.restore_user_e is None and m.restore_item_e is None
    m.restore_user_e = m.restore_item_e = torch.zeros(1)
    m.eval()
    assert m.restore_user_e is None and m.restore_item_e is None


def test_exports_sources_and_header():
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("chaorec_lightgode_")) == NEW
    assert _lib.ABI_VERSION == 16 and not any(n in _lib.INT_VALUE_EXPORTS for n in NEW)
    assert "lightgode.hip" in _lib.SOURCES
    with open(os.path.join(kernel_meta.ROOT, "include", "chaorec_hip.h")) as f:
        header = f.read()
    assert all(f"int {n}(" in header for n in NEW) and "LightGODE (Model/LightGODE.py:97-146) -- csrc/lightgode.hip.  Additive to ABI 16: new names only." in header
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW)
    from chaorec_amd import ops_extra, ops_lightgode
    assert "ops_lightgode" in ops._FAMILY_MODULES
    for name in ops_lightgode.__all__:
        assert getattr(ops, name) is getattr(ops_lightgode, name) and getattr(ops_extra, name) is getattr(ops_lightgode, name)


def test_shape_checks_refuse_without_a_launch():
    for B, D in ((64, 32), (1, 64), (0, 64), (8193, 64)):
        with pytest.raises(RuntimeError, match="chaorec_lightgode_check_shape failed"):
            ops.lightgode_check_shape(B, D)
        with pytest.raises(RuntimeError, match="chaorec_lightgode_workspace failed"):
            ops.lightgode_workspace(B, D)
    ops.lightgode_check_shape(2, 64)
    ops.lightgode_check_shape(8192, 64)
    # z, the centred z and the G partials, the r partials, the norms, n, the alignment terms and the two shifts; splits bring the
    # grid to 256 workgroups
    assert ops.lightgode_workspace(2) == 2 * 2 * 64 * (2 + 1) + 2 * 4 + 2 * 4 + 2 * 4 + 4 + 128
    assert ops.lightgode_workspace(1024) == 2 * 1024 * 64 * (2 + 4) + 2 * 1024 * (4 + 1 + 1) + 1024 + 128
    assert ops.lightgode_workspace(257) == 2 * 257 * 64 * (2 + 3) + 2 * 260 * (3 + 1 + 1) + 260 + 128
    lib = _lib.load()
    for call in (lambda: lib.chaorec_lightgode_loss_f32(None, None, 1, 1, None, None, 4, 64, 0.5, None, 0, None, None, None, None),
                 lambda: lib.chaorec_lightgode_bwd_f32(None, None, None, 4, 64, 1, 1, None, None, None, None)):
        with pytest.raises(RuntimeError, match="NULL argument"):
            call()


def test_wrappers_have_no_cpu_fallback():
    W = torch.zeros(4, 64)
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lightgode_loss(W, W, ids, ids, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lightgode_euler(None, W, 1.8)
    loss, parts = ops.lightgode_loss_plain(torch.randn(6, 8), None, torch.tensor([0, 1, 2]), torch.tensor([0, 1, 1]), 0.5, item_offset=3)
    assert loss.shape == () and parts.shape == (4,) and float(parts[0]) == float(loss)


def test_kernels_compile_for_gfx950_without_scratch():
    """Read from the compiler's metadata; no instruction text is inspected."""
    kernels, m = kernel_meta.kernel_metadata(kernel_meta.compile_asm("lightgode.hip"))
    print(dict(kernels=kernels, **m))
    assert len(kernels) == 5 and all(len(m[k]) == 5 for k in m)
    assert not any(m["scratch"]) and not any(m["spills"]) and not any(m["sspills"])
    assert max(m["lds"]) == (64 * 129 + 128 + 32 * 65 + 4 * 32) * 4          # the pair launch: the column tile, n, the waves' sums
