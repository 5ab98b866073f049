"""The first backward propagate of a fused LightGCN step over a small graph (csrc/spmm_fewsrc.hip through ops.spmm_fewsrc_raw):
every row written, only the flagged rows gathered, the bitmap tested in LDS -- against the dense launch, bit for bit, and the
step with the mode forced on against the step with it forced off."""
import numpy as np
import pytest
import torch

from conftest import load_interactions

N_USER, N_ITEM = 212, 299                   # N = 511: neither a multiple of the 4 rows of a wave nor of a bitmap word
DEGREES = (0, 1, 6, 7, 22, 23, 32, 33, 64, 65, 200)      # around the inline entries (6), the column blocks (+16) and the long threshold (32)
MEGA = 280                                  # one user row longer than a whole turn (256 entries) of the workgroup's scan


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from chaorec_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _edges():
    """Users 0 .. 10 and items 0 .. 10 have exactly DEGREES' entries (a special node is linked to filler nodes of the other side
    only), user 11 has MEGA; the fillers' degrees are what that leaves them."""
    rng = np.random.default_rng(511)
    k = len(DEGREES)
    fill_items = np.arange(k, N_ITEM)
    fill_users = np.arange(k + 1, N_USER)
    pairs = []
    for u, d in enumerate(DEGREES + (MEGA,)):
        pairs += [(u, i) for i in rng.permutation(fill_items)[:d]]
    for i, d in enumerate(DEGREES):
        pairs += [(u, i) for u in rng.permutation(fill_users)[:d]]
    e = np.asarray(pairs, dtype=np.int64)[rng.permutation(len(pairs))]
    e[:, 1] += N_USER
    return e


@pytest.fixture(scope="module")
def small(dev):
    from chaorec_amd import graph
    N = N_USER + N_ITEM
    csr = graph.lightgcn_csr(_edges(), N).to(dev)
    rowptr = csr.rowptr.cpu().numpy()
    deg = rowptr[1:] - rowptr[:-1]
    for d in DEGREES:                       # a user and an item of every kind
        assert (deg[:N_USER] == d).any() and (deg[N_USER:] == d).any(), d
    assert deg.max() == MEGA > 256
    col = csr.col.cpu().numpy()
    long_row = int(np.nonzero(deg == 200)[0][0])
    rng = np.random.default_rng(7)
    flags = {
        "none": np.zeros(N, bool),
        "all": np.ones(N, bool),
        "last_of_long": np.isin(np.arange(N), [col[rowptr[long_row + 1] - 1]]),
        "inline": np.isin(np.arange(N), [col[rowptr[long_row] + 2]]),
        "word_edges": np.isin(np.arange(N), [31, 32, N - 1]),
        "random": rng.random(N) < 0.07,
        "random_b": rng.random(N) < 0.07,
    }
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 64, generator=g).to(dev)
    z = torch.randn(N, 64, generator=g).to(dev)
    return dict(csr=csr, N=N, flags=flags, x=x, z=z)


def _bitmap(mask, dev):
    from chaorec_amd import ops
    words = np.zeros(ops.row_bitmap(mask.size, "cpu").numel(), dtype=np.uint32)
    idx = np.nonzero(mask)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return torch.from_numpy(words.view(np.int32)).to(dev)


def _masked(t, mask, fill, dev):
    keep = torch.from_numpy(mask).to(dev)[:, None]
    return torch.where(keep, t, torch.full_like(t, fill))


@pytest.mark.gpu
@pytest.mark.parametrize("with_z", [False, True])
@pytest.mark.parametrize("src, zf", [("none", "none"), ("all", "all"), ("last_of_long", "last_of_long"), ("inline", "inline"),
                                     ("word_edges", "word_edges"), ("random", "random"), ("random", "random_b")])
def test_kernel_equals_dense_launch_bit_for_bit(dev, small, src, zf, with_z):
    """The dense launch on operands that are zero outside the flags against the new one on operands that are NaN there: equal
    bits prove the sums are the dense ones and that no unflagged row of x or z was read.  (random, random_b): z under a bitmap
    of its own, tested in memory instead of in LDS."""
    from chaorec_amd import ops
    csr, x, z = small["csr"], small["x"], small["z"]
    ms, mz = small["flags"][src], small["flags"][zf]
    alpha, beta = 0.25, 0.75
    ref = ops.spmm_raw(csr, _masked(x, ms, 0.0, dev), alpha=alpha, z=_masked(z, mz, 0.0, dev) if with_z else None,
                       beta=beta if with_z else 0.0)
    y = torch.full_like(ref, float("nan"))
    bits = _bitmap(ms, dev)
    ops.spmm_fewsrc_raw(csr, _masked(x, ms, float("nan"), dev), y, bits, alpha=alpha,
                        z=_masked(z, mz, float("nan"), dev) if with_z else None, beta=beta if with_z else 0.0,
                        z_bits=(bits if zf == src else _bitmap(mz, dev)) if with_z else None)
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int32), ref.view(torch.int32))
    if src == "none" and (zf == "none" or not with_z):
        assert not bool(y.view(torch.int32).any())            # all +0: every row was written, none with a sign


def test_argument_checks():
    """Refused before anything is launched (no device pointer is ever read by the host: the addresses below are made up)."""
    from chaorec_amd import _lib, ops
    lib = _lib.load()
    p, q = 4096, 8192

    def call(n, D, bits):
        return lib.chaorec_spmm_csr_fewsrc_f32(p, p, p, q, n, n, D, 1.0, None, 0.0, p, bits, None, None)

    with pytest.raises(RuntimeError, match=r"^chaorec_spmm_csr_fewsrc_f32 failed \(-1\): .*LDS budget"):
        call(ops.FEWSRC_MAX_ROWS + 1, 64, p)
    for D in (32, 128, 60):
        assert D not in ops.FEWSRC_WIDTHS
        with pytest.raises(RuntimeError, match=r"^chaorec_spmm_csr_fewsrc_f32 failed \(-1\): .*built for D = 64"):
            call(512, D, p)
    with pytest.raises(RuntimeError, match=r"^chaorec_spmm_csr_fewsrc_f32 failed \(-1\): .*NULL argument"):
        call(512, 64, None)
    with pytest.raises(RuntimeError, match=r"^chaorec_spmm_csr_fewsrc_f32 failed \(-1\): .*16-byte aligned"):
        lib.chaorec_spmm_csr_fewsrc_f32(p, p, p + 4, q, 512, 512, 64, 1.0, None, 0.0, p, p, None, None)
    with pytest.raises(RuntimeError, match=r"^chaorec_spmm_csr_fewsrc_f32 failed \(-1\): .*come together"):
        lib.chaorec_spmm_csr_fewsrc_f32(p, p, p, q, 512, 512, 64, 1.0, p, 0.0, p, p, None, None)


def _model(dev, d, seed=0):
    from chaorec_amd import graph
    from chaorec_amd.Model import LightGCN
    from chaorec_amd.optim import FusedAdam
    torch.manual_seed(seed)
    m = LightGCN(d["U"], d["I"], d["train"], graph.user_item_dict_from_edges(d["train"]), 64, 1e-3, 3, "add", dev).to(dev)
    return m, FusedAdam(m.parameters(), lr=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("capture, given", [(True, False), (False, False), (False, True)])
def test_step_with_the_mode_equals_step_without(dev, capture, given, monkeypatch):
    """Seven steps with the mode forced on against seven with it forced off (the suite's ordered BPR launch: two runs agree
    bit for bit): captured three steps to a replay, eager with the batch drawn in the launch, eager with a given batch."""
    from chaorec_amd.optim import FusedLightGCNStep
    d = load_interactions("baby")
    edges_dev = torch.from_numpy(d["train"].astype(np.int64)).to(dev)
    batches = [edges_dev[torch.randint(0, edges_dev.shape[0], (1024,), generator=torch.Generator().manual_seed(s)).to(dev)]
               for s in range(7)]
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("CHAOREC_FEW_SOURCE_BACKWARD", mode)
        m, o = _model(dev, d)
        acc = torch.zeros(1, dtype=torch.float32, device=dev)
        kw = dict(given_batch=True) if given else dict(edges=edges_dev, seed=11,
                                                       step_dev=torch.zeros(1, dtype=torch.int64, device=dev))
        step = FusedLightGCNStep(m, o, batch_size=1024, loss_accum=acc, capture=capture,
                                 steps_per_replay=3 if capture else 1, **kw)
        assert step.few_src == (mode == "1") and not step.sparse_bwd and not step.light
        if given:
            for b in batches:
                neg = (b[:, 1] * 7 + 3) % d["I"] + d["U"]
                step(b[:, 0], b[:, 1], neg)
        else:
            step.run(7)
        torch.cuda.synchronize()
        assert int(o._step_dev) == 7
        assert not bool(step.G.any())
        if step.few_src:
            assert not bool(step._few_bits.any())
        out[mode] = [t.clone() for t in (m._flat, step.m, step.v, step.static_loss, acc, m.result)]
    for a, b in zip(out["0"], out["1"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
