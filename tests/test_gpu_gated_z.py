"""G read through R0's bitmap by a backward launch that adds w G: the SP launch with z_bits alone (ops.spmm_rowsparse_raw) and
the Adam launch with z_bits, which clears the same bitmap by its last workgroup (chaorec_spmm_csr_adam_gated_f32) -- against
the dense launches bit for bit, with NaN in every row the gate must not touch.  (The step gates its Adam launch only;
tests/test_gpu_inner_mean_rows.py runs it with the switches on against off.)
The graph is the smallest with every kind of row: N = 151 (no multiple of 4 or 32, the bitmap's last word partly used), a row
above the long threshold, one just past the inline entries of a descriptor, one of a single entry and an empty one; the Adam
launch also runs over N = 1601 rows, where its workgroups (101 at D = 64, 201 at D = 128) share the ticket's 64 sub-counters
unevenly."""
import numpy as np
import pytest
import torch

from accept import same_bits_t
from lightgcn_small_graph import EMPTY_ROW, LONG_ROW, MID_ROW, N, ONE_ROW, small_edges

WIDE_USER, WIDE_ITEM = 1000, 601


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chaorec_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _bitmap(flagged, dev):
    words = np.zeros((flagged.size + 31) // 32 + 1, dtype=np.uint32)
    idx = np.nonzero(flagged)[0]
    np.bitwise_or.at(words, idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    return torch.from_numpy(words.view(np.int32)).to(dev)


@pytest.fixture(scope="module")
def wide(dev):
    from chaorec_amd import graph
    rng = np.random.default_rng(1601)
    n = WIDE_USER + WIDE_ITEM
    e = np.stack([rng.integers(0, WIDE_USER, 4000), WIDE_USER + rng.integers(0, WIDE_ITEM, 4000)], 1)
    e = np.unique(e, axis=0)
    flagged = (rng.random(n) < 0.07) | np.isin(np.arange(n), [0, 31, 32, n - 1])
    return dict(N=n, csr=graph.lightgcn_csr(e, n).to(dev), flagged=torch.from_numpy(flagged).to(dev), bits=_bitmap(flagged, dev))


@pytest.fixture(scope="module")
def small(dev):
    from chaorec_amd import _lib, graph
    edges = small_edges()
    csr = graph.lightgcn_csr(edges, N).to(dev)
    deg = np.diff(csr.rowptr.cpu().numpy())
    assert deg[LONG_ROW] == 40 > _lib.load().chaorec_spmm_long_threshold() and deg[MID_ROW] == 9 and deg[ONE_ROW] == 1
    assert deg[EMPTY_ROW] == 0
    flagged = np.isin(np.arange(N), [0, 31, 32, N - 1, LONG_ROW, MID_ROW, 7, 64, 95, 96, 127, 128, 140])
    return dict(N=N, edges=edges, csr=csr, flagged=torch.from_numpy(flagged).to(dev), bits=_bitmap(flagged, dev))


def _operands(dev, gr, D):
    """x, and z twice: zero / NaN outside the flagged rows."""
    g = torch.Generator().manual_seed(D)
    x = torch.randn(gr["N"], D, generator=g).to(dev)
    z = torch.randn(gr["N"], D, generator=g).to(dev)
    keep = gr["flagged"][:, None]
    return x, torch.where(keep, z, torch.zeros_like(z)), torch.where(keep, z, torch.full_like(z, float("nan")))


@pytest.mark.gpu
def test_plain_launch_reads_z_through_its_bitmap(dev, small):
    from chaorec_amd import ops
    csr = small["csr"]
    x, z0, znan = _operands(dev, small, 64)
    ref = ops.spmm_raw(csr, x, alpha=0.25, z=z0, beta=0.75)
    y = torch.full_like(ref, float("nan"))
    ops.spmm_rowsparse_raw(csr, x, y, alpha=0.25, z=znan, beta=0.75, z_bits=small["bits"])
    torch.cuda.synchronize()
    assert same_bits_t(y, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("which", ["small", "wide"])
def test_adam_launch_reads_z_through_its_bitmap_and_clears_it_last(dev, small, wide, which, D):
    """Three launches in a row on the same buffers (a clear that races the read would lose flagged rows): parameters, moments
    and the gradient are the ungated launch's, z is +0 in the flagged rows and untouched -- NaN -- in the others, the bitmap
    and the ticket are clear after every launch."""
    from chaorec_amd import ops
    gr = small if which == "small" else wide
    csr, bits0, keep, n = gr["csr"], gr["bits"], gr["flagged"][:, None], gr["N"]
    x, z0, znan = _operands(dev, gr, D)
    g = torch.Generator().manual_seed(5)
    state = [torch.randn(n, D, generator=g).to(dev), 0.1 * torch.randn(n, D, generator=g).to(dev),
             0.01 * torch.rand(n, D, generator=g).to(dev)]
    bc = torch.tensor([0.1, 0.0316], dtype=torch.float32, device=dev)
    hyper = (bc, 1e-3, (0.9, 0.999), 1e-8, 0.0)
    ref, new = [t.clone() for t in state], [t.clone() for t in state]
    z_ref, z_new = z0.clone(), znan.clone()
    bits_ref, bits_new = bits0.clone(), bits0.clone()
    g_ref, g_new = torch.empty_like(x), torch.empty_like(x)
    ticket = ops.spmm_adam_ticket(dev)
    for launch in range(3):
        z_ref.copy_(z0), z_new.copy_(znan), bits_ref.copy_(bits0), bits_new.copy_(bits0)
        ops.spmm_adam_raw(csr, x, *ref, *hyper, alpha=0.5, z=z_ref, beta=0.25, clear_z=True, grad_out=g_ref,
                          clear_bits=(bits_ref,))
        ops.spmm_adam_raw(csr, x, *new, *hyper, alpha=0.5, z=z_new, beta=0.25, clear_z=True, grad_out=g_new,
                          clear_bits=(bits_new,), z_bits=bits_new, ticket=ticket)
        torch.cuda.synchronize()
        for a, b in zip(ref + [g_ref], new + [g_new]):
            assert same_bits_t(a, b), launch
        assert not bool(z_ref.any())
        assert same_bits_t(z_new, torch.where(keep, torch.zeros_like(znan), znan)), launch
        assert not bool(bits_new.any()) and not bool(bits_ref.any()) and not bool(ticket.any()), launch


def test_gated_adam_argument_checks():
    """Refused before anything is launched (the addresses are made up: the host never reads a device pointer)."""
    from chaorec_amd import _lib, ops
    lib = _lib.load()
    p, q = 4096, 8192

    def call(z, z_bits, n_words_z, ticket, n_words_ticket=ops.SPMM_TICKET_WORDS, n=151):
        return lib.chaorec_spmm_csr_adam_gated_f32(p, p, p, p, None, n, n, 64, 1.0, z, 0.25, p, 0, q, q, q, p, 1e-3, 0.9, 0.999,
                                                   1e-8, 0.0, 1, q, 6, None, 0, z_bits, n_words_z, ticket, n_words_ticket, None)

    err = r"^chaorec_spmm_csr_adam_gated_f32 failed \(-1\): .*"
    with pytest.raises(RuntimeError, match=err + "come together"):
        call(None, q, 6, q)
    with pytest.raises(RuntimeError, match=err + "come together"):
        call(q, None, 0, q)
    with pytest.raises(RuntimeError, match=err + "shorter than the rows"):
        call(q, q, 4, q)                    # 128 bits for 151 rows
    with pytest.raises(RuntimeError, match=err + "ticket of at least"):
        call(q, q, 5, None)
    with pytest.raises(RuntimeError, match=err + "ticket of at least"):
        call(q, q, 5, q, n_words_ticket=1)
