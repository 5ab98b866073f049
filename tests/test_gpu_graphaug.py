"""GraphAug on the MI355X: the edge sampler (given draws, device draws, val_t, bit-identity), the whole-table log-sum-exp node
(forward and both gradients at the tile edges, bit-identity) and the model (loss parts and gradients with the kernels and with
the plain-torch lines, a 3-step trajectory through the training loop's own branch, the rank list) against the float64
restatement of tests/graphaug_host.py and the golden of the reference class.

Bounds.  Model quantities: 4 x max(the deviation the golden stores for the reference's own fp32 run, 2^-24).  Kernel quantities
the golden has no run of: the same rule with the deviation measured here between the restatement's lines in torch fp32 on the
CPU and its float64 ones.  The sampler's zero / non-zero decision is compared exactly except where the float64 s lies within
delta = 4 x that deviation of 0.2 (at most 0.1 % of E; tests/test_graphaug_host.py asserts it for the cases used here).
Nothing is compared with the code under test."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import graphaug_host as gh  # noqa: E402
import vae_ops_host as vo  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LSE_SHAPES = ((33, 97), (1, 5), (64, 32 * 64 + 1))       # a partial row tile, a table below one tile, a last split of one row
INV_TEMP = 20.0


def within(x, ref, dev, what):
    accept.within(what, x, ref, dev, accept.ULP24)


def dev():
    return torch.device("cuda:0")


def t(x, dtype=torch.float32):
    return accept.to_dev(x, dtype, dev())


@functools.lru_cache(maxsize=None)
def case():
    c = gh.small_case()
    return c, gh.init_weights(c), gh.load_fixture(GOLDEN), gh.draws(c, 1)[0]


@functools.lru_cache(maxsize=None)
def structure():
    from chaorec_amd import graph, sparse
    c = case()[0]
    e = torch.as_tensor(c["edges"]).long()
    st = sparse._dropout_structure(graph.binary_sym_norm_csr(e[:, 0], e[:, 1] - c["U"], c["U"], c["I"])).to(dev())
    G = gh.graph_arrays(c)
    assert np.array_equal(st.col.cpu().numpy(), G["col"]) and np.array_equal(st.transpose_entry.cpu().numpy(), G["tentry"])
    return st


# ---- the edge sampler ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sampler_reference():
    c = case()[0]
    W, z, u1, u2 = gh.sampler_case(c)
    h64 = gh.sampler_host(W, gh.Graph(c), z, u1, u2)
    h32 = gh.sampler_host(W, gh.Graph(c, torch.float32), z, u1, u2, torch.float32)
    return W, z, u1, u2, h64, h32


def run_sampler(u1=None, u2=None, state=None, salt=0, **kw):
    from chaorec_amd import ops_extra
    W, z = sampler_reference()[:2]
    zt, W1 = t(z), t(W[gh.MLP[0]])
    P, Q = zt @ W1[:, :gh.D].t(), zt @ W1[:, gh.D:].t()
    return ops_extra.graphaug_edge_sample(structure(), P, Q, t(W[gh.MLP[1]]), t(W[gh.MLP[2]]), t(W[gh.MLP[3]]),
                                          None if u1 is None else t(u1), None if u2 is None else t(u2), state, 12345, salt, **kw)


def check_values(val, logits, h64, h32, what):
    """val / logits of a launch against the float64 lines, under the fp32 lines' own deviation"""
    E = len(h64["s"])
    delta, band = gh.flip_band(h32["s"], h64["s"])
    assert band.sum() <= 0.001 * E
    within(logits, h64["logits"], gh.rel_dev(h32["logits"], h64["logits"]), f"{what}: logits")
    nz = val != 0
    assert np.array_equal(nz[~band], (h64["val"] != 0)[~band]), f"{what}: a zero / non-zero decision differs outside the band"
    assert nz.any() and not nz.all()
    keep = ~band
    within(val[keep], h64["val"][keep], gh.rel_dev(h32["val"][keep], h64["val"][keep]), f"{what}: values")


def test_sampler_given_draws():
    _, _, u1, u2, h64, h32 = sampler_reference()
    val, val_t, logits, draws = run_sampler(u1, u2, return_logits=True, return_draws=True)
    check_values(val.cpu().numpy(), logits.cpu().numpy(), h64, h32, "given draws")
    assert np.array_equal(draws.cpu().numpy(), np.stack([u1, u2]))
    assert (h64["att"] == 0.01).any() and (h64["att"] == 0.99).any()


def test_sampler_val_t_and_bit_identity():
    _, _, u1, u2, _, _ = sampler_reference()
    a = run_sampler(u1, u2, return_logits=True)
    b = run_sampler(u1, u2, return_logits=True)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    G = gh.graph_arrays(case()[0])
    val, val_t = a[0].cpu().numpy(), a[1].cpu().numpy()
    assert np.array_equal(val_t, val[G["tentry"]])
    assert run_sampler(u1, u2, want_val_t=False)[1] is None


def test_sampler_device_draws():
    from chaorec_amd import ops_extra
    c = case()[0]
    W, z = sampler_reference()[:2]
    state = torch.zeros(2, dtype=torch.int64, device=dev())
    ops_extra.adagcl_tick(state)
    val, _, logits, draws = run_sampler(state=state, return_logits=True, return_draws=True)
    again = run_sampler(state=state, return_draws=True)
    assert torch.equal(val, again[0]) and torch.equal(draws, again[3])              # the same state: the same draws
    other = run_sampler(state=state, salt=1, return_draws=True)
    assert not torch.equal(draws, other[3])                                          # the second view's stream
    u = draws.cpu().numpy()
    assert u.shape == (2, len(val)) and u.min() > 0.0 and u.max() < 1.0
    assert abs(u.mean() - 0.5) < 0.05 and abs(np.corrcoef(u[0], u[1])[0, 1]) < 0.15
    # the restatement evaluated on the draws the launch used must reproduce its values
    h64 = gh.sampler_host(W, gh.Graph(c), z, u[0], u[1])
    h32 = gh.sampler_host(W, gh.Graph(c, torch.float32), z, u[0], u[1], torch.float32)
    check_values(val.cpu().numpy(), logits.cpu().numpy(), h64, h32, "device draws")
    ops_extra.adagcl_tick(state)
    ticked = run_sampler(state=state, return_draws=True)
    assert not torch.equal(draws, ticked[3]) and not torch.equal(val, ticked[0])    # a tick later: fresh draws


@pytest.mark.parametrize("salt", [0, 1])
def test_sampler_device_draws_are_the_host_generator_bit_for_bit(salt):
    """On the ragged 40-node graph of vae_ops_host.ragged_rows (a row of 70 entries, an empty one), two ticks in."""
    from chaorec_amd import ops_extra
    st = vo.ragged_structure(dev())
    E = st.nnz
    state = torch.zeros(2, dtype=torch.int64, device=dev())
    ops_extra.adagcl_tick(state)
    ops_extra.adagcl_tick(state)
    PQ, v = torch.zeros((40, gh.D), device=dev()), torch.zeros(gh.D, device=dev())
    u = ops_extra.graphaug_edge_sample(st, PQ, PQ, v, v, v[:1], None, None, state, 12345, salt, want_val_t=False, return_draws=True)[3].cpu().numpy()
    GA_SALT = 0x6772617068617567
    ref = np.stack([vo.vae_uniform(vo.vae_key(12345, 2, GA_SALT + 2 * salt + k), 0, np.arange(E), 24) for k in (0, 1)])
    assert u.shape == (2, E) and u.dtype == ref.dtype == np.float32 and np.array_equal(u.view(np.uint32), ref.view(np.uint32))


def test_sampler_rejects_other_widths():
    from chaorec_amd import _lib, ops_extra
    with pytest.raises(RuntimeError, match="graphaug_check_shape"):
        _lib.load().chaorec_graphaug_check_shape(32)
    _lib.load().chaorec_graphaug_check_shape(64)
    st = structure()
    x = torch.zeros(st.n_rows, 32, device=dev())
    with pytest.raises(ValueError):
        ops_extra.graphaug_edge_sample(st, x, x, x[0], x[0], x[0, :1], state=torch.zeros(2, dtype=torch.int64, device=dev()))
    with pytest.raises(ValueError):
        ops_extra.graphaug_lse(x, x, 5.0)


# ---- the log-sum-exp node -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lse_reference(B, M):
    A, T, g = gh.lse_case(B, M)
    r64 = gh.lse_host(A, T, INV_TEMP, g)
    r32 = gh.lse_host(A, T, INV_TEMP, g, torch.float32)
    return A, T, g, r64, r32


def run_lse(B, M):
    from chaorec_amd import ops_extra
    A, T, g = lse_reference(B, M)[:3]
    At, Tt = t(A).requires_grad_(True), t(T).requires_grad_(True)
    lse = ops_extra.graphaug_lse(At, Tt, INV_TEMP)
    (lse * t(g)).sum().backward()
    return lse.detach(), At.grad, Tt.grad


@pytest.mark.parametrize("B,M", LSE_SHAPES)
def test_lse_forward_and_gradients(B, M):
    from chaorec_amd import _lib
    _, _, _, r64, r32 = lse_reference(B, M)
    if M > 2000:
        assert int(_lib.load().chaorec_graphaug_lse_splits(B, M)) > 1
    got = run_lse(B, M)
    for x, ref, ref32, what in zip(got, r64, r32, ("lse", "gA", "gT")):
        assert x.shape == ref.shape and torch.isfinite(x).all()
        within(x.cpu().numpy(), ref, gh.rel_dev(ref32, ref), f"[{B}, {M}] {what}")
    assert float(got[0].max()) > INV_TEMP - 1e-3           # the e^20 term is in the sum


def test_lse_bit_identity():
    a, b = run_lse(64, 32 * 64 + 1), run_lse(64, 32 * 64 + 1)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- the model ------------------------------------------------------------------------------------------------------------
def make_model(fused_edges=True, fused_contrast=True, dim_E=gh.DIM_E):
    from chaorec_amd.Model import GraphAug
    c = case()[0]
    torch.manual_seed(c["seed"])
    m = GraphAug(c["U"], c["I"], c["edges"], gh.user_item_dict(c["edges"]), dim_E, gh.REG_WEIGHT, gh.N_LAYERS, gh.SSL_TEMP, gh.SSL_ALPHA, dev())
    m.fused_edges, m.fused_contrast = fused_edges, fused_contrast
    return m.train()


def feed(m, drs):
    for dr in drs:
        m.feed_draws(u1=[v["u1"] for v in dr["views"]], u2=[v["u2"] for v in dr["views"]],
                     masks=[k for v in dr["views"] for k in v["masks"]], rdm=[dr["rdm"]])


def batch():
    c = case()[0]
    return tuple(torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))


def test_model_weights_and_names():
    _, w, g, _ = case()
    m = make_model()
    assert tuple(m.state_dict().keys()) == gh.NAMES == tuple(g["names"].tolist())
    assert tuple(n for n, _ in m.named_parameters()) == gh.PARAMS
    for n, p in m.named_parameters():
        assert np.array_equal(p.detach().cpu().numpy(), w[n]), n
    for k, layer in enumerate(m.backbone_gnn.bottom_layers):
        assert np.array_equal(layer.weight_matrix.cpu().numpy(), w[gh.BOTTOM[2 * k]]) and not layer.weight_matrix.requires_grad
        assert np.array_equal(layer.bias.cpu().numpy(), w[gh.BOTTOM[2 * k + 1]])


@pytest.mark.parametrize("fused_edges,fused_contrast", ((True, True), (False, False), (True, False), (False, True)))
def test_model_loss_and_gradients(fused_edges, fused_contrast):
    _, _, g, dr = case()
    m = make_model(fused_edges, fused_contrast)
    feed(m, [dr])
    loss = m.loss(*batch())
    loss.backward()
    assert not any(m._draws.values())                         # every given draw was consumed
    within(float(loss.detach()), g["ref_loss"], g["dev_loss"], "loss")
    for name, part in zip(gh.PARTS, m.last_parts):
        within(float(part), g[f"ref_{name}"], g[f"dev_{name}"], name)
    params = dict(m.named_parameters())
    for k, n in enumerate(gh.WITH_GRAD):
        within(params[n].grad.cpu().numpy(), g[f"ref_grad_{k}"], g["dev_grads"][k], f"grad {n}")
    assert all(params[n].grad is None for n in gh.MLP)


@pytest.mark.parametrize("fused", (True, False))
def test_model_view_values(fused):
    """view 1 of the step: node_emb, logits and the sampled values against the reference's own run"""
    c, _, g, dr = case()
    m = make_model(fused, True)
    v = dr["views"][0]
    with torch.no_grad():
        ofea = m.getEgoEmbeds({0: m.norm_adj_mat}, 1)
        node_emb, _ = m.backbone_gnn(m.norm_adj_mat, ofea, [t(k) for k in v["masks"]])
        val, val_t, logits, _ = m.view_learner.sample(node_emb, m.norm_adj_mat, fused, u1=t(v["u1"]), u2=t(v["u2"]), return_parts=True)
    within(node_emb.cpu().numpy()[:g["node_emb"].shape[0]], g["node_emb"], g["dev_node_emb"], "node_emb")
    within(logits.cpu().numpy(), g["logits"], g["dev_logits"], "logits")
    val = val.cpu().numpy()
    assert np.array_equal(val != 0, g["nonzero"])             # (no entry of the golden lies in the band: test_graphaug_host.py)
    within(val, g["val"], g["dev_val"], "values")
    assert np.array_equal(val_t.cpu().numpy(), val[gh.graph_arrays(c)["tentry"]])


def test_model_trajectory_through_the_training_loop():
    from chaorec_amd import registry, train_and_evaluate
    c, w, g, _ = case()
    m = make_model()
    feed(m, gh.draws(c, gh.N_STEPS, seed_offset=2))
    assert not registry.MODELS["GraphAug"].capture
    opt = torch.optim.Adam(m.parameters(), lr=gh.LR)
    total = train_and_evaluate.train(m, [batch()] * gh.N_STEPS, opt, "GraphAug")
    within(total, float(g["traj_losses"].sum()), g["dev_traj_losses"], "sum of the trajectory's losses")
    params = dict(m.named_parameters())
    for k, n in enumerate(gh.WITH_GRAD):
        within(params[n].detach().cpu().numpy() - w[n], g[f"traj_{k}"] - w[n], g["dev_traj"][k], f"update of {n}")
    assert all(np.array_equal(params[n].detach().cpu().numpy(), w[n]) for n in gh.MLP)


def test_model_device_draws_step():
    """without given draws: the sampler draws in its launch, the step counter advances once per loss(), the loss is finite"""
    m = make_model()
    before = m._state.clone()
    loss = m.loss(*batch())
    loss.backward()
    assert torch.isfinite(loss) and int(m._state[0]) == int(before[0]) + 1
    assert all(torch.isfinite(p.grad).all() for n, p in m.named_parameters() if n in gh.WITH_GRAD)


def test_model_rank_list():
    c, w, g, _ = case()
    m = make_model().eval()
    got = m.gene_ranklist(topk=gh.TOPK).numpy()
    assert got.shape == (c["U"], gh.TOPK)
    ref = g["ranklist"].astype(np.int64)
    differ = got != ref
    print("positions that differ from the reference's list:", int(differ.sum()))
    if differ.any():          # a tie within fp32: the float64 scores of the listed items must agree
        W = gh.tensors(w, requires_grad=False)
        main = gh.propagate(W, gh.Graph(c), gh.Graph(c).val)
        s = (main[:c["U"]] @ main[c["U"]:].t()).numpy()
        for u, items in gh.user_item_dict(c["edges"]).items():
            s[u, np.array(items) - c["U"]] = 1e-6
        a, b = np.take_along_axis(s, got - c["U"], 1), np.take_along_axis(s, ref - c["U"], 1)
        assert np.abs(a - b)[differ].max() <= 1e-6 * np.abs(s).max()


def test_model_raises_at_other_widths():
    m = make_model(dim_E=32)
    with pytest.raises(ValueError, match="64"):
        m.loss(*batch())
    m.fused_edges, m.fused_contrast = False, True
    with pytest.raises(ValueError, match="64"):
        m.contrastLoss(torch.randn(8, 32, device=dev()), torch.randn(8, 32, device=dev()), torch.arange(4, device=dev()), 0.2)
