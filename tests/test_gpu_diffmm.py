"""DiffMM's kernels (csrc/diffmm.hip through ops_extra.diffmm_rows / diffmm_denoise_loss) and Model/DiffMM.py on the MI355X,
against the restatements of tests/diffmm_host.py and the reference fixture of tests/golden/gen_diffmm.py.

Rows launch, given draws: bit for bit the float32 restatement (two roundings, then the doubling), pad columns 0, the bit
table equal to the CSR; B in {1, R - 1, R, R + 1, 4 R + 3} with R the rows of a workgroup read from the export, I in
{1, 31, 32, 33, 97, 1003}; a user with an empty history, a repeated user, every time step; both modes.
Device draws: keyed (seed, step, salt, user, item) only; over 10^6 kept elements |mean| <= 5 / sqrt(N),
|var - 1| <= 5 sqrt(2 / N), |keep rate - 1/2| <= 5 / (2 sqrt(N)) (five standard errors of the three estimators).
One-pass node: tolerance measured and not chosen -- the reference's own lines in torch fp32 on the CPU on the same inputs
(diffmm_host.node_all), their deviation from float64 relative to the tensor's largest magnitude, asserted below 1e-4; the
kernels are allowed 4 x max(that, 2^-24) (accept.within_measured).  Every case runs twice over allocator memory dirtied with NaN, then 1e30: the two
runs agree in their bits.  An incoming gradient of 0.37 is held to the same rule against 0.37 x the float64 gradients.
Every row of the node's x0 holds an interaction, as every user of a dataset does: the rule measures against a tensor's largest
magnitude, and at I = 1 a tensor is one number per row -- err = out - x0 with x0 = 1 is then a sum led by an exact term,
where with x0 = 0 it is a K-term fp32 dot product whose error relative to ITS OWN value (cancellation included) no fp32
chain, the reference's included, keeps below 4 x 2^-24 (B = I = 1, H = 16 drew sum |h_k W_k| / |out| = 15: the plain
k-ascending fma chain evaluated on the host deviates by 4.0e-7 there, the kernel by 4.2e-7, the reference's lines by 1.3e-8).
Empty rows are the rows launch's business and are covered there.
Model, both settings of fused_denoise: within 4 x max(the fixture's stored deviation, 2^-24) of the float64 restatement.
The largest deviation / bound of a test is printed as `ratio`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffmm_host as mh  # noqa: E402
from accept import ULP24, bound_of, same_bits, within, within_measured  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODS = ("image", "text")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs the MI355X"
    return torch.device("cuda:0")


def _tiles():
    from chaorec_amd import ops_extra
    return ops_extra.diffmm_tiles()


def _dirty(dev, B, I, H, fill):
    """Junk where the allocator will hand out the rows, the bit table, d_out, the partials and the gradients."""
    for shape in ((3 * B, I + 8), (2 * B, H), (2 * I, H), (B, 64), (B, I // 32 + 2), (I + 8,), (B + 8,), (1,)):
        torch.full(shape, fill, device=dev)
    torch.full((B + 8,), fill, dtype=torch.float64, device=dev)
    torch.full((B, I // 32 + 2), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()


# ---- (a) the rows launch -------------------------------------------------------------------------------------------------------
def rows_case(B, I, seed):
    """A history CSR over U = B + 3 users (user 1 empty where there is one, the longest row full where I is small), a batch
    that names user 0 twice where it can, and draws."""
    rng = np.random.default_rng(seed)
    U = B + 3
    rows = [np.sort(rng.choice(I, size=int(rng.integers(1, max(2, min(I, 40)))), replace=False)) for _ in range(U)]
    rows[1] = np.zeros(0, dtype=np.int64)
    rows[U - 1] = np.arange(min(I, 70))
    rowptr = np.zeros(U + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=rowptr[1:])
    col = np.concatenate(rows).astype(np.int32)
    users = rng.permutation(U)[:B].astype(np.int64)
    if B >= 3:
        users[:3] = (0, 1, 0)
    if B >= 4:
        users[3] = U - 1
    ts = ((np.arange(B) + I) % 5).astype(np.int64)
    noise = rng.standard_normal((B, I)).astype(np.float32)
    keep = rng.random((B, I)) < 0.5
    return U, rowptr, col, users, ts, noise, keep


@pytest.mark.parametrize("I", [1, 31, 32, 33, 97, 1003])
@pytest.mark.parametrize("Bk", range(5))
def test_rows_given_draws_bit_for_bit(dev, Bk, I):
    from chaorec_amd import ops_extra
    R = ops_extra.diffmm_rows_per_block()
    B = (1, R - 1, R, R + 1, 4 * R + 3)[Bk]
    U, rowptr, col, users, ts, noise, keep = rows_case(B, I, 1000 * B + I)
    T = mh.tables()
    x0 = mh.dense_rows(rowptr, col, users, I)
    want = mh.noised_rows(x0, ts, noise, keep, T)
    a, s = (torch.from_numpy(T[k][ts].astype(np.float32)).to(dev) for k in ("sqrt_ac", "sqrt_1mac"))
    d = lambda x: torch.from_numpy(x).to(dev)   # noqa: E731
    ld = ops_extra.diffmm_ld(I)
    assert ld % 4 == 0 and I <= ld < I + 4
    for fill in (float("nan"), 1e30):
        _dirty(dev, B, I, 4, fill)
        x, bits = ops_extra.diffmm_rows(d(users), d(rowptr), d(col), I, a, s, d(noise), d(keep), seed=1, step=1, salt=0)
        _dirty(dev, B, I, 4, fill)
        xp, bits_p = ops_extra.diffmm_rows(d(users), d(rowptr), d(col), I, plain=True)
        torch.cuda.synchronize()
        for got, ref, name in ((x, want, "noised"), (xp, x0, "plain")):
            assert tuple(got.shape) == (B, I) and got.stride() == (ld, 1)
            full = got.as_strided((B, ld), (ld, 1)).cpu().numpy()
            assert same_bits(full[:, :I], ref), f"{name}: x_in differs from the float32 restatement"
            assert same_bits(full[:, I:], np.zeros((B, ld - I), dtype=np.float32)), f"{name}: pad columns"
        for b in (bits, bits_p):
            assert same_bits(b.cpu().numpy().view(np.uint32), mh.bit_table(x0)), "bit table"
    if B >= 3:
        assert not x0[1].any() and np.array_equal(x0[0], x0[2])          # the empty row, the repeated user


def test_device_draws_keyed_by_user_and_item(dev):
    from chaorec_amd import ops_extra
    U, rowptr, col, users, _, _, _ = rows_case(19, 1003, 7)
    I, T = 1003, mh.tables()
    d = lambda x: torch.from_numpy(x).to(dev)   # noqa: E731
    ts = np.full(19, 3)
    a, s = (torch.from_numpy(T[k][ts].astype(np.float32)).to(dev) for k in ("sqrt_ac", "sqrt_1mac"))
    x, _ = ops_extra.diffmm_rows(d(users), d(rowptr), d(col), I, a, s, seed=9, step=4, salt=1)
    order = np.random.default_rng(0).permutation(19)
    y, _ = ops_extra.diffmm_rows(d(users[order]), d(rowptr), d(col), I, a, s, seed=9, step=4, salt=1)
    z, _ = ops_extra.diffmm_rows(d(users[order][:7]), d(rowptr), d(col), I, a[:7], s[:7], seed=9, step=4, salt=1)
    assert same_bits(x.cpu().numpy()[order], y.cpu().numpy()) and same_bits(y.cpu().numpy()[:7], z.cpu().numpy())
    for other in (dict(seed=10, step=4, salt=1), dict(seed=9, step=5, salt=1), dict(seed=9, step=4, salt=0)):
        o, _ = ops_extra.diffmm_rows(d(users), d(rowptr), d(col), I, a, s, **other)
        assert not same_bits(x.cpu().numpy(), o.cpu().numpy())


def test_device_draws_statistics(dev):
    """Users without history: x_in = kept ? 2 s n : 0, so n = x_in / (2 s) where kept.  2048 x 1003 elements, about half kept."""
    from chaorec_amd import ops_extra
    B, I = 2048, 1003
    rowptr, col = torch.zeros(B + 1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    s32 = np.float32(mh.tables()["sqrt_1mac"][4])
    a, s = torch.ones(B, device=dev), torch.full((B,), float(s32), device=dev)
    x, bits = ops_extra.diffmm_rows(torch.arange(B, device=dev), rowptr, col, I, a, s, seed=123, step=2, salt=0)
    x = x.cpu().numpy().astype(np.float64)
    assert not bits.any()
    kept = x != 0
    N, n = x.size, x[kept] / (2.0 * float(s32))
    assert n.size >= 10 ** 6
    mean, var, rate = n.mean(), n.var(), kept.mean()
    print(f"draws: N {n.size}, mean {mean:.3e} (bound {5 / np.sqrt(n.size):.3e}), var - 1 {var - 1:.3e} (bound {5 * np.sqrt(2 / n.size):.3e}), "
          f"keep rate - 1/2 {rate - 0.5:.3e} (bound {2.5 / np.sqrt(N):.3e})")
    assert abs(mean) <= 5 / np.sqrt(n.size) and abs(var - 1) <= 5 * np.sqrt(2 / n.size) and abs(rate - 0.5) <= 2.5 / np.sqrt(N)


def test_device_draws_are_the_host_generator(dev):
    """Users without history at B = 5, I = 33, a = 1, s = 1/2: x_in = kept ? n : 0 with no rounding of its own.  The non-zero
    pattern is uniform(keep key, user, item) < 1/2 exactly; the kept n against the Box-Muller of the noise key's two uniforms in
    float64, under test_gpu_vae_ops's rule: 4 x the same lines' deviation in float32, at least 2^-22, per row."""
    import re
    import vae_ops_host as vo
    from chaorec_amd import ops_extra
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "chaorec_amd", "csrc", "diffmm.hip")) as f:
        nbits = int(re.search(r"constexpr int DM_BITS = (\d+);", f.read()).group(1))
    B, I, seed, step, salt = 5, 33, 123, 2, 1
    rowptr, col = torch.zeros(B + 1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    x, bits = ops_extra.diffmm_rows(torch.arange(B, device=dev), rowptr, col, I, torch.ones(B, device=dev), torch.full((B,), 0.5, device=dev),
                                    seed=seed, step=step, salt=salt)
    x = x.cpu().numpy()
    u, i = np.arange(B)[:, None], np.arange(I)[None, :]
    kept = vo.vae_uniform(vo.vae_key(seed, step, 2 * salt + 1), u, i, nbits) < np.float32(0.5)
    assert not bits.any() and kept.any() and not kept.all() and np.array_equal(x != 0, kept)
    key = vo.vae_key(seed, step, 2 * salt)
    u1, u2 = vo.vae_uniform(key, u, 2 * i, nbits), vo.vae_uniform(key, u, 2 * i + 1, nbits)
    n64 = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))
    n32 = np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(2.0 * np.pi) * u2)
    assert n32.dtype == np.float32
    got, ref64, ref32 = np.where(kept, x, 0), np.where(kept, n64, 0), np.where(kept, n32, 0)
    d, bound = vo.row_dev(got, ref64), vo.bound_of(ref32, ref64)
    print(f"device normal: deviation {d:.3e}, the float32 lines' own {vo.row_dev(ref32, ref64):.3e}, bound {bound:.3e}")
    assert d <= bound


# ---- (b) the one-pass node -----------------------------------------------------------------------------------------------------
def node_case(B, I, Hd, seed):
    rng = np.random.default_rng(seed)
    h = np.tanh(rng.standard_normal((B, Hd))).astype(np.float32)
    W = (rng.standard_normal((I, Hd)) * np.sqrt(2.0 / (I + Hd))).astype(np.float32)
    b = (rng.standard_normal(I) * 0.001).astype(np.float32)
    F = (rng.standard_normal((I, 64)) * 0.3).astype(np.float32)
    E = (rng.standard_normal((I, 64)) * 0.1).astype(np.float32)
    x0 = (rng.random((B, I)) < 0.15).astype(np.float32)
    x0[np.arange(B), np.arange(B) % I] = 1.0      # no empty row: a batch's users come from the interaction list (see above)
    ts = rng.integers(0, 5, B)
    ts[0] = 0
    if B > 4:
        ts[1:5] = (1, 2, 3, 4)          # the whole SNR range: weights from 1 down to the last step's
    x0E = (x0.astype(np.float64) @ E.astype(np.float64)).astype(np.float32)
    return h, W, b, x0, x0E, F, mh.snr_weight(ts)


def run_node(dev, case, e_loss, g, fill):
    from chaorec_amd import ops_extra
    h, W, b, x0, x0E, F, wt = case
    B, I, Hd = h.shape[0], W.shape[0], h.shape[1]
    th, tW, tb = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (h, W, b))
    bits = torch.from_numpy(mh.bit_table(x0).view(np.int32)).to(dev)
    tx, tF, tw = torch.from_numpy(x0E).to(dev), torch.from_numpy(F).to(dev), torch.from_numpy(wt).to(dev)
    _dirty(dev, B, I, Hd, fill)
    raw = ops_extra.diffmm_out_loss_raw(th.detach(), tW.detach(), tb.detach(), bits, tx, tF, tw, e_loss)
    d_full = raw[3].cpu().numpy()
    assert not d_full[:, I:].any(), "d_out's pad columns"
    _dirty(dev, B, I, Hd, fill)
    loss, diff, gc = ops_extra.diffmm_denoise_loss(th, tW, tb, bits, tx, tF, tw, e_loss)
    assert loss.shape == (1,) and diff.dtype == torch.float64 and not diff.requires_grad and not gc.requires_grad
    (loss.sum() * g).backward()
    torch.cuda.synchronize()
    out = dict(loss=loss.detach(), diff_rows=diff, gc_rows=gc, d_out=raw[3][:, :I] * g, dh=th.grad, dW_out=tW.grad, db_out=tb.grad)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("Hk", range(4))
@pytest.mark.parametrize("Ik", range(5))
@pytest.mark.parametrize("Bk", range(4))
def test_one_pass_node(dev, Bk, Ik, Hk):
    bm, bn, bk = _tiles()
    B, I, Hd = (1, bm - 1, bm, bm + 1)[Bk], (1, bn - 1, bn, bn + 1, 2 * bn + 3)[Ik], (4, bk, bk + 4, 1000)[Hk]
    case, e_loss = node_case(B, I, Hd, 10000 * B + 10 * I + Hk), 0.01
    runs = [run_node(dev, case, e_loss, 1.0, fill) for fill in (float("nan"), 1e30)]
    for k in runs[0]:
        assert same_bits(runs[0][k], runs[1][k]), f"{k}: two runs differ in their bits"
    failures, ratios = [], []
    for g, got in ((1.0, runs[0]), (0.37, run_node(dev, case, e_loss, 0.37, 1e30))):
        r64, r32 = mh.node_all(*case, e_loss, torch.float64, g=g), mh.node_all(*case, e_loss, torch.float32, g=g)
        for k in ("loss", "diff_rows", "gc_rows", "d_out", "dW_out", "db_out", "dh"):
            within_measured(f"node B={B} I={I} H={Hd} g={g} {k}", got[k], r32[k], r64[k], ULP24, failures=failures, ratios=ratios)
    print(f"node B={B} I={I} H={Hd}: largest ratio {max(ratios):.3f}")
    assert not failures, failures


def test_node_rejects_what_it_does_not_tile(dev):
    from chaorec_amd import ops_extra
    with pytest.raises(RuntimeError):
        ops_extra.diffmm_check_shape(4, 8, 6)          # H no multiple of 4
    with pytest.raises(RuntimeError):
        ops_extra.diffmm_check_shape(4, 8, 8, D=32)
    assert _tiles() == (128, 128, 16)


# ---- (c) the model --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx(dev):
    g, c = mh.load_fixture(GOLDEN), mh.small_case()
    model = mh.build_model(c, dev)
    w = mh.weights_of(model)
    for k, n in enumerate(mh.NAMES):
        assert float(w[n].astype(np.float64).sum()) == g["w_sum"][k], n
    rowptr, col = mh.hist_csr(c["edges"], c["U"])
    x0 = mh.dense_rows(rowptr, col, c["diff_users"], c["I"])
    steps = [mh.diffusion_step(w, c, mod, x0, g["ts"][m], g["noise"][m], g["keep"][m], mh.HYPER["e_loss"], torch.float64)
             for m, mod in enumerate(MODS)]
    return dict(g=g, c=c, model=model, w=w, steps=steps, hist=(rowptr, col))


@pytest.mark.parametrize("fused", [True, False])
def test_model_diffusion_step(fx, dev, fused):
    g, c, model = fx["g"], fx["c"], fx["model"]
    model.fused_denoise = fused
    model.train()
    model.zero_grad()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    li, lt = model.diffusion_step(t(c["diff_users"]), ts=(t(g["ts"][0]), t(g["ts"][1])), noise=(t(g["noise"][0]), t(g["noise"][1])),
                                  keep=(t(g["keep"][0]), t(g["keep"][1])))
    (li + lt).backward()
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    failures, ratios = [], []
    for m, (mod, loss) in enumerate(zip(MODS, (li, lt))):
        h = fx["steps"][m]
        within(f"{mod} loss", float(loss), h["loss"], g[f"dev_step_{mod}_loss"], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
        within(f"{mod} diff_loss", model.last[mod]["diff_loss"].cpu().numpy(), h["diff_loss"], g[f"dev_step_{mod}_diff"], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
        within(f"{mod} gc_loss", model.last[mod]["gc_loss"].cpu().numpy(), h["gc_loss"], g[f"dev_step_{mod}_gc"], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
        for n, ref in h["grads"].items():
            within(n, params[n].grad.cpu().numpy(), ref, g["dev_grad_" + n], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
    assert all(params[n].grad is None for n in mh.NAMES if not n.startswith("denoise_model_"))
    print(f"model step fused={fused}: largest ratio {max(ratios):.3f}")
    model.fused_denoise = True
    assert not failures, failures


@pytest.mark.parametrize("fused", [True, False])
def test_model_rebuild(fx, dev, fused):
    g, c, model = fx["g"], fx["c"], fx["model"]
    U, I = c["U"], c["I"]
    model.fused_denoise = fused
    loader = [torch.arange(0, 20), torch.arange(20, U)]           # two batches, the second longer than the first
    rand = []
    for mod in MODS:                                              # the recorded uniforms in our (row-major) entry order
        pre = g[f"adj_{mod}_pre"]
        rand.append(torch.from_numpy(g[f"adj_{mod}_rand"][np.argsort(pre[0] * (U + I) + pre[1], kind="stable")]))
    with torch.no_grad():
        for m, (mod, dn) in enumerate(zip(MODS, (model.denoise_model_image, model.denoise_model_text))):
            idx, x_t = model.denoised_topk(dn, torch.arange(U, device=dev))
            assert np.array_equal(idx.cpu().numpy(), g[f"top_{mod}"]), f"{mod}: top-1"
            # against the reference's own fp32 iterate: our 4 x max(its deviation, 2^-24) from float64 plus its deviation from it
            assert mh.rel_dev(x_t.cpu().numpy(), g[f"iter_{mod}"][-1]) <= bound_of(g[f"dev_iter_{mod}"], ULP24) + float(g[f"dev_iter_{mod}"])
    adjs = model.rebuild_graphs(loader, rand=rand, as_csr=False)
    csrs = model.rebuild_graphs(loader, rand=rand)
    model.fused_denoise = True
    for mod, adj, csr in zip(MODS, adjs, csrs):
        a = adj.coalesce()
        post = g[f"adj_{mod}_idx"]
        o = np.argsort(post[0] * (U + I) + post[1], kind="stable")
        assert np.array_equal(a.indices().cpu().numpy(), post[:, o]), f"{mod}: rebuilt adjacency"
        assert np.abs(a.values().cpu().numpy() - g[f"adj_{mod}_val"][o]).max() <= 2.0 ** -22
        assert csr.n_rows == U + I and csr.nnz == post.shape[1] and np.array_equal(csr.col.cpu().numpy(), post[1][o])


def test_model_loss_gradients_and_ranking(fx, dev):
    from conftest import tie_aware_rank_equal
    g, c, model = fx["g"], fx["c"], fx["model"]
    U, I, N = c["U"], c["I"], c["U"] + c["I"]
    from chaorec_amd import sparse
    adjs, dense = [], []
    for mod in MODS:
        idx, val = torch.from_numpy(g[f"adj_{mod}_idx"]), torch.from_numpy(g[f"adj_{mod}_val"])
        adjs.append(sparse.from_torch_sparse(torch.sparse_coo_tensor(idx, val, (N, N)).to(dev)))
        dense.append(mh.dense_adj(idx[0], idx[1], val, N, torch.float64))
    h = mh.model_loss(fx["w"], c, dense[0], dense[1], c["users"], c["pos"], c["neg"], torch.float64)
    model.train()
    model.zero_grad()
    loss = model.loss(*(torch.from_numpy(c[k]).to(dev) for k in ("users", "pos", "neg")), adjs[0], adjs[1])
    loss.backward()
    torch.cuda.synchronize()
    failures, ratios = [], []
    within("loss", float(loss), h["loss"], g["dev_loss"], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
    within("usr", model.restore_usrEmbeds.detach().cpu().numpy(), h["usr"], g["dev_usr"], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
    within("itm", model.restore_itmEmbeds.detach().cpu().numpy(), h["itm"], g["dev_itm"], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
    params = dict(model.named_parameters())
    for n, ref in h["grads"].items():
        within("grad " + n, params[n].grad.cpu().numpy(), ref, g["dev_grad_" + n], ULP24, own_cap=1e-4, failures=failures, ratios=ratios)
    print(f"model loss: largest ratio {max(ratios):.3f}")
    assert not failures, failures
    K = g["rank"].shape[1]
    rank = model.gene_ranklist(topk=K).numpy()
    rowptr, col = fx["hist"]
    idx, val = mh.ranklist(h["usr"], h["itm"], rowptr, col, U, K)
    s = h["usr"] @ h["itm"].T
    for u in range(U):
        s[u, col[rowptr[u]:rowptr[u + 1]]] = 1e-6
    ok, why = tie_aware_rank_equal(rank, np.take_along_axis(s, rank - U, 1), idx, val, atol=1e-6)
    assert ok, why
    ok, why = tie_aware_rank_equal(g["rank"], np.take_along_axis(s, g["rank"] - U, 1), idx, val, atol=1e-6)
    assert ok, why


# ---- (d) one epoch ---------------------------------------------------------------------------------------------------------------
def test_epoch_finite_and_no_dense_interaction_matrix(dev):
    """One epoch of _train_epoch_diffmm (all of the diffusion pass and the rebuild, three BPR batches) at U = 131072,
    I = 4096.  A dense [U, I] fp32 matrix is 2 GiB: had any tensor of U I elements been allocated, the peak of allocated
    memory would be at least that.  What the epoch legitimately holds is far below it, from the shapes: the denoisers with
    gradients and Adam moments 4 x 2 x (1000 (I + 10) + 1000 I + ...) x 4 B = 0.26 GB, some dozens of [U + I, 64] tables of the
    graph half at 35 MB each, and a dozen [1024, I] row tensors at 17 MB each."""
    from chaorec_amd import epochs as te
    from chaorec_amd.Model import DiffMM
    from chaorec_amd.dataload import DeviceUserBatches
    from chaorec_amd.optim import FusedAdam
    U, I, B = 131072, 4096, 1024
    rng = np.random.default_rng(5)
    edges = np.stack([np.arange(U), U + rng.integers(0, I, U)], 1).astype(np.int64)
    torch.manual_seed(3)
    hy = mh.HYPER
    model = DiffMM(U, I, edges, None, torch.randn(I, 32), torch.randn(I, 16), 64, hy["reg_weight"], hy["n_layers"], hy["ssl_alpha"],
                   hy["ssl_temp"], hy["ris_lambda"], hy["e_loss"], hy["rebuild_k"], dev)
    opt = FusedAdam([{"params": model.parameters(), "lr": 1e-3}])
    pick = rng.choice(U, (3, 64))
    batches = [(torch.from_numpy(edges[p, 0]).to(dev), torch.from_numpy(edges[p, 1]).to(dev),
                torch.from_numpy(U + rng.integers(0, I, 64)).to(dev)) for p in pick]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    model.train()
    loss = te._train_epoch_diffmm(model, batches, opt, DeviceUserBatches(U, B, dev, seed=1))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"epoch: loss {loss:.5f}, peak {peak / 2 ** 20:.0f} MiB, a dense [U, I] fp32 matrix {4 * U * I / 2 ** 20:.0f} MiB")
    assert np.isfinite(loss) and loss > 0
    assert peak < 4 * U * I
    rank = model.gene_ranklist(topk=5)
    assert rank.shape == (U, 5) and int(rank.min()) >= U and int(rank.max()) < U + I
