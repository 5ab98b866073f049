"""BSPM without a GPU: the float64 item-block restatement (tests/bspm_host.py) against the full-adjacency one and against the
golden the reference's own run left (tests/golden/bspm_small.npz), ops.BSPMTile on CPU tensors, the model's host construction
and refusals, and the glue (registry, YAML, parser, library names)."""
import functools
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import bspm_host as bh  # noqa: E402
from conftest import GOLDEN, tie_aware_rank_equal  # noqa: E402

from chaorec_amd import _lib, ops  # noqa: E402
from chaorec_amd.Model import BSPM  # noqa: E402


@functools.lru_cache(maxsize=None)
def case():
    g = bh.load_fixture(GOLDEN)
    edges = g["edges"].astype(np.int64)
    return g, edges, int(g["I"])


def build(K_s=1, T_s=1.0, beta=1.0, **kw):
    g, edges, I = case()
    kw.setdefault("factors", g["Vi"])
    return BSPM(bh.U, I, edges, bh.user_item_dict(edges), K_s, T_s, 1, 1, beta, "cpu", factor_dim=bh.FACTOR, **kw)


# ---- the restatements and the golden ----------------------------------------------------------------------------------------------
def test_case_is_the_generator_s():
    g, edges, I = case()
    assert I == bh.num_items(int(g["long_row"])) and np.array_equal(edges, bh.small_case(I, int(g["seed"])))
    Rn, _, _ = bh.normalised(edges, I)
    P = Rn.T @ Rn
    assert int((P[0] != 0).sum()) == I - bh.EMPTY_ITEMS > int(g["long_row"])          # the full row takes the long-row path
    assert (Rn[bh.U - 1] == 0).all() and (Rn[:, I - bh.EMPTY_ITEMS:] == 0).all() and (Rn[:bh.U - 1, 0] > 0).all()
    assert bh.item_factors(Rn, bh.FACTOR // 2)[1] > 3e-3


@pytest.mark.parametrize("c", range(len(bh.CASES)))
def test_item_block_route_is_the_full_route(c):
    g, edges, I = case()
    K_s, T_s, beta = bh.CASES[c]
    full, vt = bh.full_route(edges, I, K_s, T_s, beta)
    Vi, _ = bh.item_factors(bh.normalised(edges, I)[0], bh.FACTOR // 2)
    item = bh.item_route(edges, I, K_s, T_s, beta, Vi)
    assert bh.rel_dev(item, full[:, bh.U:]) <= 1e-12
    assert bh.rel_dev(bh.item_route(edges, I, K_s, T_s, beta, g["Vi"]), full[:, bh.U:]) <= 1e-12      # the golden's vectors too
    assert bh.rel_dev(g[f"host64_{c}"], item) <= 1e-12
    # the projector is what is defined: the item block of the full adjacency's vectors spans the same space
    assert np.abs(vt[:, bh.U:].T @ vt[:, bh.U:] - Vi @ Vi.T).max() <= 1e-12
    # the user columns exist (the IDL term's spill) and are small; nobody reads them
    assert np.abs(full[:, :bh.U]).max() <= 1e-9 and float(g[f"usercol_max_{c}"]) <= 1e-9


@pytest.mark.parametrize("c", range(len(bh.CASES)))
def test_golden_against_itself(c):
    g, edges, I = case()
    ref32, host64, own = g[f"ref32_{c}"], g[f"host64_{c}"], float(g[f"own_{c}"])
    assert ref32.dtype == np.float32 and ref32.shape == (bh.U, I) == host64.shape
    assert bh.rel_dev(ref32, host64) <= own * (1 + 1e-12) and 0 < own < 1e-6
    rank = g[f"rank_{c}"].astype(np.int64) - bh.U
    assert rank.shape == (bh.U, bh.TOPK) and all(len(set(r)) == bh.TOPK for r in rank.tolist())
    i64, v64 = bh.top_lists(bh.masked(host64, edges))
    v32 = np.take_along_axis(bh.masked(ref32, edges), rank, 1)
    ok, why = tie_aware_rank_equal(rank, v32, i64, v64, atol=accept.bound_of(own, bh.ULP) * np.abs(host64).max())
    assert ok, why
    # history items carry the VALUE 1e-6 and do rank above the many negative scores
    reaches = bool((((bh.masked(host64, edges) > bh.MASK).sum(1) < bh.TOPK) & (bh.masked(host64, edges) == bh.MASK).any(1)).any())
    assert np.mean(host64 <= 0) > 0.3 and bool((v32 == np.float32(bh.MASK)).any()) == reaches and (reaches or c == 2)


# ---- ops.BSPMTile on CPU tensors --------------------------------------------------------------------------------------------------
def numpy_tile(rowptr, col, val, ids, I):
    trip = [(s, int(col[e]), val[e]) for s, u in enumerate(ids) for e in range(rowptr[u], rowptr[u + 1])]
    by_item = sorted(trip, key=lambda t: (t[1], t[0]))
    return trip, by_item


@pytest.mark.parametrize("width", [None, 32])
def test_tile_on_cpu_tensors(width):
    g, edges, I = case()
    m = build()
    rowptr, col, val = m.hist
    assert np.array_equal(val.numpy(), g["rn_val"])                      # Rn as the reference rounded it, CSR order
    ids = np.array([5, 69, 3, 5, 17, 0, 69, 44, 5, 12, 30], dtype=np.int64)      # shuffled, duplicated, user 69 has no history
    t = ops.BSPMTile(rowptr, col, val, I, torch.from_numpy(ids), width)
    B = 12 if width is None else width
    assert (t.n, t.B, t.num_item) == (len(ids), B, I)
    trip, by_item = numpy_tile(rowptr.numpy(), col.numpy(), val.numpy(), ids, I)
    assert t.nnz == len(trip) and t.x_ptr.dtype == torch.int64 and t.xt_slot.dtype == torch.int32 and t.x_item.dtype == torch.int32
    xp = t.x_ptr.numpy()
    assert xp.shape == (B + 1,) and (np.diff(xp) >= 0).all() and xp[0] == 0 and (xp[len(ids):] == len(trip)).all()
    assert xp[2] - xp[1] == 0                                            # the user without history: an empty slot
    assert [(int(np.searchsorted(xp, e, "right") - 1), int(i), v) for e, (i, v) in enumerate(zip(t.x_item.tolist(), t.x_val.tolist()))] \
        == [(s, i, float(v)) for s, i, v in trip]
    ptr = t.xt_ptr.numpy()
    assert ptr.shape == (I + 1,) and (np.diff(ptr) >= 0).all() and ptr[0] == 0 and ptr[-1] == len(trip)
    items = np.repeat(np.arange(I), np.diff(ptr))
    assert np.array_equal(items, t.xt_item.numpy())
    got = list(zip(t.xt_slot.tolist(), items.tolist(), t.xt_val.tolist()))
    assert got == [(s, i, float(v)) for s, i, v in by_item]
    for j in range(I):
        assert (np.diff(t.xt_slot.numpy()[ptr[j]:ptr[j + 1]]) > 0).all()          # slots ascending within an item
    with pytest.raises(ValueError, match="B=6; the kernels tile a multiple of 4"):
        ops.BSPMTile(rowptr, col, val, I, torch.from_numpy(ids[:5]), 6)
    with pytest.raises(ValueError, match="11 users were given"):
        ops.BSPMTile(rowptr, col, val, I, torch.from_numpy(ids), 8)


# ---- the model's host construction ------------------------------------------------------------------------------------------------
def test_construction_is_the_reference_s():
    g, edges, I = case()
    m = build()
    P = m.filter.P
    assert (P.n_rows, P.n_cols, P.symmetric) == (I, I, True)
    assert np.array_equal(P.rowptr.numpy(), g["p_ptr"].astype(np.int64)) and np.array_equal(P.col.numpy(), g["p_col"].astype(np.int32))
    assert bh.rel_dev(P.val.numpy(), g["p_val"]) <= bh.ULP               # the float64 product rounded once (sum order aside)
    _, _, di = bh.normalised(edges, I)
    assert np.array_equal(m.filter.F.numpy(), (di[:, None] * g["Vi"]).astype(np.float32))
    assert np.array_equal(m.filter.Gt.numpy(), (g["Vi"] / di[:, None]).astype(np.float32))
    for name in ("solver_idl", "solver_blr", "solver_shr", "K_idl", "T_idl", "K_b", "T_b", "K_s", "T_s", "final_sharpening",
                 "sharpening_off", "t_point_combination", "factor_dim", "idl_beta", "idl_times", "blurring_times", "sharpening_times"):
        assert hasattr(m, name), name
    assert m.fused is True and m.full_sort_predict.__func__ is BSPM.gene_ranklist and list(m.parameters()) == []
    assert list(inspect.signature(BSPM.__init__).parameters)[1:] == [
        "num_user", "num_item", "edge_index", "user_item_dict", "K_s", "T_s", "K_b", "T_b", "idl_beta", "device", "factor_dim",
        "factors", "fused"]
    assert ops.bspm_step_sizes(3, 1.0) == bh.step_sizes(3, 1.0) and ops.bspm_step_sizes(2, 1.5) == [0.75, 0.75]


def test_own_factors_span_the_golden_s_space():
    g, edges, I = case()
    m = build(factors=None)                                              # the model's own decomposition
    _, _, di = bh.normalised(edges, I)
    Vi = m.filter.F.numpy().astype(np.float64) / di[:, None]
    assert np.abs(Vi @ Vi.T - g["Vi"] @ g["Vi"].T).max() <= 1e-5         # fp32-rounded factors; vectors themselves are not compared


def test_filter_without_scipy_is_the_same(monkeypatch):
    mod = sys.modules[BSPM.__module__]
    g, edges, I = case()
    m = build()
    rowptr, col, _ = m.hist
    u = np.repeat(np.arange(bh.U), np.diff(rowptr.numpy()))
    i = col.numpy().astype(np.int64)
    Rn, _, _ = bh.normalised(edges, I)
    with_scipy = mod._item_filter(u, i, Rn[u, i], bh.U, I)
    monkeypatch.setitem(sys.modules, "scipy.sparse", None)               # `import scipy.sparse` now raises ImportError
    without = mod._item_filter(u, i, Rn[u, i], bh.U, I)
    assert torch.equal(with_scipy[0], without[0]) and torch.equal(with_scipy[1], without[1])
    assert bh.rel_dev(without[2].numpy(), with_scipy[2].numpy()) <= bh.ULP
    monkeypatch.setattr(mod, "_DENSE_SVD_CELLS", 0)
    with pytest.raises(ImportError, match="factors="):
        mod._right_singular_vectors(u, i, Rn[u, i], bh.U, I, 4)


def test_refusals():
    g, edges, I = case()
    with pytest.raises(ValueError, match="factor_dim=15 is odd"):
        BSPM(bh.U, I, edges, bh.user_item_dict(edges), 1, 1.0, 1, 1, 1.0, "cpu", factor_dim=15)
    with pytest.raises(ValueError, match=r"factors is \(150, 8\), expected \(150, 4\)"):
        BSPM(bh.U, I, edges, bh.user_item_dict(edges), 1, 1.0, 1, 1, 1.0, "cpu", factor_dim=8, factors=g["Vi"])
    d = bh.user_item_dict(edges)
    d[bh.U - 1] = [bh.U + 3]
    with pytest.raises(ValueError, match="hold different pairs"):
        BSPM(bh.U, I, edges, d, 1, 1.0, 1, 1, 1.0, "cpu", factor_dim=bh.FACTOR, factors=g["Vi"])
    for flag, value in (("sharpening_off", True), ("final_sharpening", False), ("t_point_combination", True), ("solver_shr", "rk4")):
        m = build()
        setattr(m, flag, value)
        for call in (lambda: m.getUsersRating([0, 1]), lambda: m.gene_ranklist(10)):
            with pytest.raises(NotImplementedError, match=f"BSPM: {flag}={value!r}; only {flag}="):
                call()
    for B in (0, 6, 1028):
        with pytest.raises(ValueError, match=f"BSPM: B={B}; the kernels tile a multiple of 4 in \\[4, 1024\\]"):
            ops.bspm_check_shape(I, B, 8)
    for mm in (0, 6, 132):
        with pytest.raises(ValueError, match=f"BSPM: m={mm}; the kernels tile a multiple of 4 in \\[4, 128\\]"):
            ops.bspm_check_shape(I, 8, mm)
    ops.bspm_check_shape(I, 1024, 128)
    lib = _lib.load()
    with pytest.raises(RuntimeError, match=r"bspm_check_shape: B=6, the kernels tile a multiple of 4 in \[4, 1024\]"):
        lib.chaorec_bspm_check_shape(I, 6, 8)
    with pytest.raises(RuntimeError, match="chaorec_amd ops run on the MI355X only"):
        build().getUsersRating([0, 1])                                   # no CPU fallback


# ---- glue ---------------------------------------------------------------------------------------------------------------------------
def test_library_names_and_layout():
    assert _lib.ABI_VERSION == 16 and _lib.load().chaorec_abi_version() == 16
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("chaorec_bspm_")) == [
        "chaorec_bspm_check_shape", "chaorec_bspm_last_step_f32", "chaorec_bspm_long_row", "chaorec_bspm_project_f32",
        "chaorec_bspm_seed_f32"]
    assert _lib.SOURCES[-1] == "adagcl.hip" and _lib.SOURCES.index("bspm.hip") == len(_lib.SOURCES) - 2
    assert not any(n.startswith("chaorec_bspm_") for n in _lib.INT_VALUE_EXPORTS)
    import ctypes
    assert _lib.SIGNATURES["chaorec_bspm_long_row"][0] is ctypes.c_int64
    assert ops.bspm_long_row() == int(case()[0]["long_row"]) >= 64
    assert "ops_bspm" in ops._FAMILY_MODULES and ops.BSPMTile.__module__ == "chaorec_amd.ops_bspm"


def test_cli_yaml_registry_and_loop():
    from chaorec_amd import arg_parser, registry
    a = arg_parser.parse_args(["--Model", "BSPM"])
    assert (a.K_s, a.T_s, a.K_b, a.T_b, a.idl_beta) == (1, 1, 1, 1, 1)
    assert isinstance(a.K_s, int) and isinstance(a.K_b, int)
    assert arg_parser.parse_args(["--Model", "BSPM", "--T_s", "2.5", "--idl_beta", "0.3"]).T_s == 2.5
    cfg = arg_parser.load_yaml_config("BSPM")
    assert cfg["hyper_parameters"] == ["K_s", "T_s", "K_b", "T_b", "idl_beta"]
    assert all(isinstance(cfg[k], list) and len(cfg[k]) >= 1 for k in cfg["hyper_parameters"])
    # what build_model hands the constructor at the first point of the grid (tests/test_model_registry.py replays this record against the table)
    built = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_constructor_args.json")))["BSPM"]
    assert built[:3] == ["BSPM", [11, 7, "train_data", "user_item_dict"] + [cfg[k][0] for k in cfg["hyper_parameters"]] + ["device"], {}]
    spec = registry.MODELS["BSPM"]
    assert registry.M.BSPM is BSPM and not spec.trains and not spec.main_optimizer and spec.epoch is None
