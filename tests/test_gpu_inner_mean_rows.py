"""Inner steps of a k-step replay of the fused LightGCN step: the BPR launch over the L + 1 layer tables
(chaorec_bpr_fwd_bwd_layers_f32) against the launch over the layer mean chaorec_spmm_csr_mean_f32 writes, bit for bit, with NaN
in every table row outside the batch; and the step with CHAOREC_GATED_Z / CHAOREC_INNER_MEAN_ROWS on against both off, after
every call of a mixed sequence of replays and single steps.  The graph is tests/lightgcn_small_graph.py's (N = 151)."""
import ctypes

import pytest
import torch

from accept import same_bits_t
from lightgcn_small_graph import N, N_ITEM, N_USER, small_edges

B, D, L = 8, 64, 3
W = 1.0 / (L + 1)
REPEATS = ([5, 5, 7, 9, 5, 11, 12, 13], [3, 4, 3, 8, 9, 10, 11, 3], [20, 21, 22, 23, 24, 25, 26, 20])   # users, positives, negatives
DISTINCT = ([5, 6, 7, 9, 10, 11, 12, 13], [3, 4, 5, 8, 9, 10, 11, 12], [20, 21, 22, 23, 24, 25, 26, 27])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chaorec_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def layers(dev):
    """x_0 .. x_L and the mean the last propagate's epilogue forms from them: computed once, never written again."""
    from chaorec_amd import graph, ops
    csr = graph.lightgcn_csr(small_edges(), N).to(dev)
    xs = [torch.randn(N, D, generator=torch.Generator().manual_seed(9)).to(dev)]
    for _ in range(L):
        xs.append(ops.spmm_raw(csr, xs[-1]))
    final = ops.spmm_mean_raw(csr, xs[L - 1], xs[:L], W, torch.empty_like(xs[0]))
    torch.cuda.synchronize()
    return xs, final


def _bpr_pair(dev, layers, batch):
    """-> (reference, new): workspace, coef, ids, G, bitmap of the launch over `final` and of the one over the layer tables."""
    from chaorec_amd import ops
    xs, final = layers
    ids0 = [torch.tensor(c, dtype=torch.int64, device=dev) for c in batch]
    rows_read = torch.cat([ids0[0], ids0[1] + N_USER, ids0[2] + N_USER])
    inside = torch.zeros(N, dtype=torch.bool, device=dev)
    inside[rows_read] = True
    poisoned = [torch.where(inside[:, None], x, torch.full_like(x, float("nan"))) for x in xs]
    rows = torch.full((3 * B, D), float("nan"), device=dev)
    out = []
    for src in (dict(tab=final), dict(tab=None, layer_tabs=poisoned, layer_w=W, rows=rows)):
        ids = tuple(t.clone() for t in ids0)
        G = torch.zeros(N, D, device=dev)
        coef, ws = torch.empty(B, device=dev), torch.empty(4 * B, device=dev)
        bits = ops.row_bitmap(N, dev)
        ops.bpr_fwd_bwd(src.pop("tab"), N_USER, G, B, ops.VARIANT_LOG_SIGMOID_EPS, 1e-3, coef, ws, ids, num_user=N_USER,
                        num_item=N_ITEM, row_bits=bits, **src)
        torch.cuda.synchronize()
        out.append([ws, coef, G, bits, *ids])
    assert same_bits_t(rows, final[rows_read.view(3, B).t().reshape(-1)])       # triple b's rows at 3 b, 3 b + 1, 3 b + 2
    return out


@pytest.mark.gpu
def test_bpr_over_layer_tables_ordered_mode_repeated_rows(dev, layers):
    """The suite's ordered gradient launch: every bit is fixed, repeated users and items included."""
    import os
    assert os.environ.get("CHAOREC_BPR_ORDERED") == "2"
    ref, new = _bpr_pair(dev, layers, REPEATS)
    assert bool(ref[2].any())
    for a, b in zip(ref, new):
        assert same_bits_t(a, b) if a.dtype == torch.float32 else torch.equal(a, b)


@pytest.mark.gpu
def test_bpr_over_layer_tables_atomic_mode(dev, layers, monkeypatch):
    """The in-launch atomic adds: bits are fixed where no row receives two contributions."""
    monkeypatch.setenv("CHAOREC_BPR_ORDERED", "0")
    ref, new = _bpr_pair(dev, layers, DISTINCT)
    assert bool(ref[2].any())
    for a, b in zip(ref, new):
        assert same_bits_t(a, b) if a.dtype == torch.float32 else torch.equal(a, b)


def test_layer_table_argument_checks():
    """Refused before anything is launched (made-up addresses: the host reads the pointer array only)."""
    from chaorec_amd import _lib
    lib = _lib.load()
    p, q = 4096, 8192

    def call(n_tabs, rows, tabs=(p, p, p, p, p)):
        arr = (ctypes.c_void_p * len(tabs))(*tabs)
        return lib.chaorec_bpr_fwd_bwd_layers_f32(ctypes.cast(arr, ctypes.c_void_p), n_tabs, 0.25, 90, rows, None, 0, None, None,
                                                  90, 61, 0, 0, None, p, p, p, 8, 64, 0, 1e-3, None, None, None, q, q, None,
                                                  None, 0, q, q, None, 0.9, 0.999, None, None, 0, None)

    err = r"^chaorec_bpr_fwd_bwd_layers_f32 failed \(-1\): .*"
    for n_tabs in (0, 5):
        with pytest.raises(RuntimeError, match=err + "layer tables"):
            call(n_tabs, q)
    with pytest.raises(RuntimeError, match=err + "NULL rows buffer"):
        call(4, None)
    with pytest.raises(RuntimeError, match=err + "NULL table 2"):
        call(4, q, tabs=(p, p, None, p))


@pytest.mark.gpu
@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("sparse, light", [("0", "0"), ("1", "0"), ("1", "auto")])
def test_step_with_the_switches_equals_step_without(dev, capture, sparse, light, monkeypatch):
    """Two replays of three steps, a single step, one more replay (capture=False: four steps): table, moments, losses,
    counters and model.result after every call, with both switches off against each alone and both on; on the few-source path
    (12 B = 96 <= N) and with the row-sparse backward forced on (where a light forward leaves only the gate)."""
    from chaorec_amd import graph
    from chaorec_amd.Model import LightGCN
    from chaorec_amd.optim import FusedAdam, FusedLightGCNStep
    edges = small_edges()
    edges_dev = torch.from_numpy(edges).to(dev)
    monkeypatch.setenv("CHAOREC_SPARSE_BACKWARD", sparse)
    monkeypatch.setenv("CHAOREC_LIGHT_FORWARD", light)
    out = {}
    for mode in (("0", "0"), ("1", "0"), ("0", "1"), ("1", "1")):
        monkeypatch.setenv("CHAOREC_GATED_Z", mode[0])
        monkeypatch.setenv("CHAOREC_INNER_MEAN_ROWS", mode[1])
        torch.manual_seed(0)
        m = LightGCN(N_USER, N_ITEM, edges, graph.user_item_dict_from_edges(edges), D, 1e-3, L, "add", dev).to(dev)
        o = FusedAdam(m.parameters(), lr=1e-3)
        acc = torch.zeros(1, dtype=torch.float32, device=dev)
        step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        step = FusedLightGCNStep(m, o, batch_size=B, edges=edges_dev, seed=11, step_dev=step_dev, loss_accum=acc,
                                 capture=capture, steps_per_replay=3)
        assert step.gate_z == (mode[0] == "1") and step.sparse_bwd == (sparse == "1") and step.few_src == (sparse == "0")
        assert step.inner_mean_rows == (mode[1] == "1" and capture and not step.light)
        snaps = []
        for single in (False, False, True, False):
            step(single=single)
            torch.cuda.synchronize()
            assert not bool(step.G.any())
            for b in ([step._bits_all] if step.sparse_bwd else [step._few_bits]) + ([step._ticket] if step.gate_z else []):
                assert not bool(b.any())
            snaps.append([t.clone() for t in (m._flat, step.m, step.v, acc, step.static_loss, step_dev, o._step_dev)]
                         + ([m.result.clone()] if m.result is not None else []))
        assert int(o._step_dev) == (10 if capture else 4)
        out[mode] = snaps
    for mode in list(out)[1:]:
        for s0, s1 in zip(out["0", "0"], out[mode]):
            assert len(s0) == len(s1)
            for a, b in zip(s0, s1):
                assert same_bits_t(a, b) if a.dtype == torch.float32 else torch.equal(a, b), mode
