"""MHRec on the MI355X: the hypergraph attention layer (csrc/mhrec.hip through ops_extra.mhrec_hyper_layer) and the model (loss
and gradients with the plain-torch switch, three BPR steps, one whole epoch through the training loop's own branch, the
device-built input hyperedges, the rank list) against the float64 restatement of tests/mhrec_host.py.

Bounds: 4 x max(the deviation the golden stores for the reference's own fp32 run, 2^-24), deviations as max |x - ref| over
max |ref|; the two halves of the attention vector's gradient are both measured against the largest entry of the whole gradient
(it is one parameter, and the first half is what is left of a cancellation: 1e-14 of the second).  Nothing is compared with
the code under test.  Every layer case is launched once and shared (kernel_run)."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import mhrec_host as mh  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def within(x, ref, dev, what, scale=None):
    accept.within(what, x, ref, dev, accept.ULP24, scale=scale)


def dev():
    return torch.device("cuda:0")


def t(x, dtype=torch.float32):
    return accept.to_dev(x, dtype, dev())


@functools.lru_cache(maxsize=None)
def case():
    g = mh.load_fixture(GOLDEN)
    c = mh.small_case(g["seed"])
    return c, mh.init_weights(c), g, mh.draws(c)


def hypergraph(nodes, N):
    from chaorec_amd import ops_extra
    return ops_extra.HyperGraph(torch.as_tensor(np.asarray(nodes)).to(dev()), N)


# ---- the layer -----------------------------------------------------------------------------------------------------------------
def _launch(k, keep="given", state=None, seed=0, salt=0, training=True):
    from chaorec_amd import ops_extra
    lc = mh.layer_case(k)
    hg = hypergraph(lc["nodes"], lc["N"])
    X, a = t(lc["X"]).requires_grad_(True), t(lc["a"]).reshape(-1, 1).requires_grad_(True)
    given = t(lc["keep"], torch.uint8) if isinstance(keep, str) else keep
    y, out = ops_extra.mhrec_hyper_layer(hg, X, a, given, state, seed, salt, training, return_out=True)
    (y * t(lc["g"])).sum().backward()
    return dict(y=y.detach().cpu().numpy(), out=out.cpu().numpy(), dX=X.grad.cpu().numpy(), da=a.grad.cpu().numpy().reshape(-1), hg=hg)


@functools.lru_cache(maxsize=None)
def kernel_run(k):
    return _launch(k)


@functools.lru_cache(maxsize=None)
def restated(k):
    lc = mh.layer_case(k)
    return mh.layer_grads(lc["X"], lc["a"], lc["nodes"], lc["keep"], lc["g"])


def test_thresholds_and_shape_check():
    from chaorec_amd import _lib, ops_extra
    lib = _lib.load()
    assert ops_extra.mhrec_long_row() == mh.LONG_ROW == ops_extra.MHREC_LONG_ROW and int(lib.chaorec_mhrec_chunk()) == ops_extra.MHREC_CHUNK
    assert (mh.LONG_ROW + 70) % int(lib.chaorec_mhrec_rows_per_block()) != 0
    with pytest.raises(RuntimeError):
        lib.chaorec_mhrec_check_shape(32)
    lib.chaorec_mhrec_check_shape(64)
    with pytest.raises(ValueError):
        ops_extra.mhrec_check_shape(128)


@pytest.mark.parametrize("k", [3, 10])
def test_layer_case_has_every_row_kind(k):
    hg, h = kernel_run(k)["hg"], restated(k)
    deg = hg.degrees().cpu().numpy()
    assert np.array_equal(deg, h["deg"]) and deg[0] == hg.num_edges and deg[1] == mh.LONG_ROW and deg[2] == mh.LONG_ROW + 1
    assert tuple(deg[3:7]) == (64, 65, 1, 0)
    assert hg.long_node.cpu().tolist() == [0, 2] and hg.n_chunks == 4 and hg.long_cptr.cpu().tolist() == [0, 2, 4]


@pytest.mark.parametrize("k", [3, 10])
def test_layer_forward(k):
    """Measured on the MI355X: largest deviation / bound 0.042 (k = 10, y); 0.24 before the sums ran in double."""
    g, got, h = case()[2], kernel_run(k), restated(k)
    within(got["out"], h["out"], g[f"dev_layer{k}_out"], f"k={k} out")
    within(got["y"], h["y"], g[f"dev_layer{k}_y"], f"k={k} y")


@pytest.mark.parametrize("k", [3, 10])
def test_layer_dX(k):
    """Measured on the MI355X: largest deviation / bound 0.027 (k = 10)."""
    within(kernel_run(k)["dX"], restated(k)["dX"], case()[2][f"dev_layer{k}_dX"], f"k={k} dX")


@pytest.mark.parametrize("k", [3, 10])
def test_layer_da1(k):
    """Measured on the MI355X: deviation 2.5e-14 and 6.3e-16 of the largest entry, deviation / bound below 0.001 (the closed form
    leaves no rounding noise)."""
    h = restated(k)
    scale = np.abs(np.concatenate([h["da1"], h["da2"]])).max()
    within(kernel_run(k)["da"][:mh.D], h["da1"], case()[2][f"dev_layer{k}_da1"], f"k={k} da1", scale)


@pytest.mark.parametrize("k", [3, 10])
def test_layer_da2(k):
    """Measured on the MI355X: largest deviation / bound 0.033 (k = 10)."""
    h = restated(k)
    scale = np.abs(np.concatenate([h["da1"], h["da2"]])).max()
    within(kernel_run(k)["da"][mh.D:], h["da2"], case()[2][f"dev_layer{k}_da2"], f"k={k} da2", scale)


@pytest.mark.parametrize("k", [3, 10])
def test_layer_structure(k):
    got, lc = kernel_run(k), mh.layer_case(k)
    assert not got["out"][6].view(np.uint32).any()                          # the node in no hyperedge: +0 before the residual
    assert np.array_equal(got["y"][6], np.where(lc["keep"][6], 2 * lc["X"][6], 0).astype(np.float32))
    assert not got["y"][~lc["keep"]].view(np.uint32).any()                  # dropped columns are exactly +0
    assert np.isfinite(got["y"]).all() and np.isfinite(got["dX"]).all() and np.isfinite(got["da"]).all()


@pytest.mark.parametrize("k", [3, 10])
def test_two_runs_give_equal_bits(k):
    again, first = _launch(k), kernel_run(k)
    for name in ("y", "out", "dX", "da"):
        assert np.array_equal(again[name].view(np.uint32), first[name].view(np.uint32)), name


def test_no_dropout_without_training():
    got = _launch(3, keep=None, training=False)
    lc = mh.layer_case(3)
    assert np.array_equal(got["y"], got["out"] + lc["X"]) and np.array_equal(got["out"].view(np.uint32), kernel_run(3)["out"].view(np.uint32))


def test_masks_drawn_in_the_launch():
    """The keep rate of the [70, 64] mask is within 4 standard deviations of 1/2; the same key gives the same mask and the
    backward redraws it; another salt or step gives another."""
    state = torch.tensor([7, 7], dtype=torch.int64, device=dev())
    a = _launch(3, keep=None, state=state, seed=11, salt=2)
    b = _launch(3, keep=None, state=state, seed=11, salt=2)
    mask = a["y"] != 0
    rate, sd = mask.mean(), 0.5 / np.sqrt(mask.size)
    print(f"keep rate {rate:.4f}, 4 sd = {4 * sd:.4f}")
    assert abs(rate - 0.5) <= 4 * sd and np.array_equal(mask, b["y"] != 0)
    given = _launch(3, keep=t(mask, torch.uint8))
    for name in ("y", "dX", "da"):
        assert np.array_equal(given[name].view(np.uint32), a[name].view(np.uint32)), name
    other = _launch(3, keep=None, state=state, seed=11, salt=3)
    later = _launch(3, keep=None, state=torch.tensor([8, 8], dtype=torch.int64, device=dev()), seed=11, salt=2)
    assert 0.3 < ((other["y"] != 0) != mask).mean() < 0.7 and 0.3 < ((later["y"] != 0) != mask).mean() < 0.7


# ---- the model -----------------------------------------------------------------------------------------------------------------
def make_model(weights=None, fused=True):
    c, w, g, _ = case()
    m = mh.build_model(c, dev())
    if weights is not None:
        m.load_state_dict({n: torch.from_numpy(np.asarray(v)) for n, v in weights.items()})
    m.set_input_hyperedges(g["hyper_visual"], g["hyper_textual"])
    m.fused_hyper = fused
    return m.train()


def batch():
    c = case()[0]
    return tuple(torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))


@functools.lru_cache(maxsize=None)
def host_step():
    c, w, g, dr = case()
    return mh.step_losses(w, c, g["nodes0"][0], g["nodes0"][1], dr["fwd_keep"][0])


def test_constructor_replays_the_weights_and_names():
    c, w, g, _ = case()
    m = make_model()
    assert tuple(m.state_dict().keys()) == tuple(g["names"].tolist()) == mh.NAMES
    for n, v in m.state_dict().items():
        assert np.array_equal(v.cpu().numpy(), w[n]), n


def test_input_hyperedges_built_on_the_device():
    """No hyperedge files: the tables come from usergraph_build / usergraph_sample and the item kNN, and equal the reference's."""
    g = case()[2]
    m = make_model()
    m.hyperedges_visual = m.hyperedges_textual = None
    m.pre_processing()
    assert m.hyperedges_visual.dtype == torch.int32 and m.hyperedges_visual.is_cuda
    assert np.array_equal(m.hyperedges_visual.cpu().numpy(), g["hyper_visual"]) and np.array_equal(m.hyperedges_textual.cpu().numpy(), g["hyper_textual"])
    v, t_ = m.diffusion_tables()
    assert v is t_ and v is m.hyperedges_visual                            # both loaders read the visual table
    rows = m.diffusion_rows(torch.arange(5)).cpu().numpy()
    assert np.array_equal(rows, mh.dense_rows(g["hyper_visual"].astype(np.int64), np.arange(5), case()[0]["U"] + case()[0]["I"]))


@pytest.mark.parametrize("fused", [True, False])
def test_loss_and_gradients(fused):
    """fused_hyper = True and False, each against the float64 restatement on the same masks under the same bound.

    Measured on the MI355X: largest deviation / bound 0.112 fused (the gradient of modal_weight: 5.2e-8 against 4.6e-7; 2.86
    with fp32 running sums in the layer), 0.388 in plain torch (the gradient of modal_weight; with the restatement's index_adds in fp32 it was 0.30 in one run
    and 0.94 in the next, their atomics adding in another order)."""
    c, w, g, dr = case()
    N = c["U"] + c["I"]
    m = make_model(w, fused)
    m.feed_draws(keep=dr["fwd_keep"][0])
    loss = m.loss(*batch(), hypergraph(g["nodes0"][0], N), hypergraph(g["nodes0"][1], N))
    loss.backward()
    host = host_step()
    assert not m._draws["keep"]
    within(float(loss.detach()), host["loss"], g["dev_loss"], f"loss (fused={fused})")
    within(m.result.detach().cpu().numpy(), host["result"], g["dev_result"], f"result (fused={fused})")
    params = dict(m.named_parameters())
    for k, n in enumerate(mh.WITH_GRAD):
        within(params[n].grad.cpu().numpy(), host["grads"][n], g["dev_grads"][k], f"grad {n} (fused={fused})")
    assert all(params[n].grad is None for n in mh.NAMES if n not in mh.WITH_GRAD)


def test_three_steps_of_the_third_phase():
    """Three BPR steps under Adam over everything, on the hypergraphs of the initial denoisers; updates as final - initial.

    Measured on the MI355X: largest deviation / bound 0.305 (the update of text_trs.weight); the updates of the four `a` are within 7e-5
    of the float64 ones (the reference's own are 2 - 13 % off, its da1 being rounding noise that Adam normalises)."""
    c, w, g, dr = case()
    N = c["U"] + c["I"]
    m = make_model(w)
    Hv, Ht = hypergraph(g["nodes0"][0], N), hypergraph(g["nodes0"][1], N)
    opt = torch.optim.Adam(m.parameters(), lr=mh.LR)
    losses = []
    for s in range(mh.N_STEPS):
        m.feed_draws(keep=dr["fwd_keep"][s])
        opt.zero_grad()
        loss = m.loss(*batch(), Hv, Ht)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    host_final, host_losses = mh.three_steps(w, c, g["nodes0"][0], g["nodes0"][1], dr["fwd_keep"])
    within(np.array(losses), host_losses, g["dev_steps3_losses"], "the three losses")
    sd = {n: v.detach().cpu().numpy() for n, v in m.state_dict().items()}
    for k, n in enumerate(mh.NAMES):
        within(sd[n] - w[n], host_final[n] - w[n], g["dev_steps3"][k], f"update of {n}")


def test_one_epoch_of_the_training_loop():
    """train_and_evaluate's MHRec branch over the small case: both diffusion passes, the rebuild, three BPR steps.

    Measured on the MI355X: largest deviation / bound 0.25 (the updates of modal_weight and of the denoisers' emb_layer.weight,
    where ours and the reference's own deviation coincide); the rebuilt hypergraphs are the golden's.  With the denoisers' training step in fp32 (diffusion_double = False) the update of
    denoise_model_image.in_layers.0.weight was 1.281e-4 of its largest entry from the float64 trajectory against a bound of
    1.278e-4 (4 x the reference's own 3.195e-5), at an entry (hidden unit 247, input column 4) whose gradient is a sum of 128
    terms cancelling about 1000 : 1; the same fp32 lines on the host give 3.7e-5 with 8 threads and 6.3e-5 with one, the f32 MFMA
    GEMMs 4.0e-4.  In float64 it is 8e-6."""
    from chaorec_amd import epochs as te
    c, w, g, dr = case()
    m = make_model(w)
    for mod in range(2):
        m.feed_draws(ts=dr["ts"][mod], noise=dr["noise"][mod], denoise_keep=dr["keep"][mod])
    m.feed_draws(rebuild_noise=dr["rebuild_noise"][0] + dr["rebuild_noise"][1], keep=[k for step in dr["fwd_keep"] for k in step])
    loaders = [torch.from_numpy(b) for b in c["batches"]]
    times = {}
    total = te._train_epoch_mhrec(m, [batch()] * mh.N_STEPS, torch.optim.Adam(m.parameters(), lr=mh.LR), (loaders, loaders), times)
    assert set(times) == {"diffusion", "rebuild", "bpr"} and all(not q for q in m._draws.values())
    host = mh.epoch(w, c, g["hyper_visual"].astype(np.int64), dr)
    for k, G in enumerate((m.G_visual, m.G_textual)):
        assert np.array_equal(np.sort(G.nodes.cpu().numpy(), 1), np.sort(g["nodes1"][k], 1)), f"rebuilt hypergraph {k}"
        assert np.array_equal(np.sort(host["nodes"][k], 1), np.sort(g["nodes1"][k], 1))
    within(total, host["losses"].sum(), g["dev_epoch_loss_sum"], "the epoch's summed loss")
    sd = {n: v.detach().cpu().numpy() for n, v in m.state_dict().items()}
    for k, n in enumerate(mh.NAMES):
        within(sd[n] - w[n], host["weights"][n] - w[n], g["dev_epoch"][k], f"update of {n}")


def test_a_step_without_fed_draws_is_finite():
    c, w, g, _ = case()
    N = c["U"] + c["I"]
    m = make_model(w)
    torch.manual_seed(3)
    loss = m.diffusion_step(torch.arange(40), 0) + m.diffusion_step(torch.arange(40), 1)
    loss.backward()
    Hv, Ht = m.rebuild_hypergraphs([torch.arange(100), torch.arange(100, 300)])
    assert Hv.num_edges == 300 and Ht.k == mh.HYPER["num_hypernodes"]
    l2 = m.loss(*batch(), Hv, Ht)
    l2.backward()
    assert np.isfinite(float(loss.detach())) and np.isfinite(float(l2.detach())) and int(m._state[0]) == 1
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_rank_list():
    c, w, g, dr = case()
    N = c["U"] + c["I"]
    m = make_model(w)
    m.feed_draws(keep=dr["fwd_keep"][0])
    with torch.no_grad():
        m.loss(*batch(), hypergraph(g["nodes0"][0], N), hypergraph(g["nodes0"][1], N))
    got = m.eval().gene_ranklist(topk=mh.TOPK).numpy() - c["U"]
    s = mh.rank_scores(host_step()["result"], c)
    assert got.shape == (c["U"], mh.TOPK) and got.min() >= 0 and got.max() < c["I"]
    assert all(len(set(r)) == mh.TOPK for r in got.tolist())
    best = np.sort(s, 1)[:, ::-1][:, :mh.TOPK]
    tol = 1e-6 * np.abs(s).max()
    assert np.abs(np.take_along_axis(s, got, 1) - best).max() <= tol                  # the float64 scores of the listed items are the best ten
