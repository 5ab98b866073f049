"""AdaGCL on the MI355X: the edge gate (forward in both forms and both layers, backward, device draws), the edge keep and
the model (four losses with their gradients, the plain-torch switch, a 3-step trajectory through the training loop's own
branch, the rank list) against the float64 restatement of tests/adagcl_host.py.

Bounds.  Model quantities: 4 x max(the deviation the golden stores for the reference's own fp32 run, 2^-24).  Gate quantities at
weights the golden has no run of (the attention rows scaled so that both clamps are taken): the same rule with the deviation
measured here, the restatement's lines in torch fp32 on the CPU -- which keep the reference's float64 island around the
draw -- against the float64 ones.  Nothing is compared with the code under test."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import adagcl_host as ah  # noqa: E402
import vae_ops_host as vo  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ULP = accept.ULP24


def within(x, ref, dev, what):
    accept.within(what, x, ref, dev, ULP)


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case():
    c = ah.small_case()
    return c, ah.init_weights(c), ah.load_fixture(GOLDEN), ah.draws(c, 1)[0]


@functools.lru_cache(maxsize=None)
def host_step():
    c, w, _, dr = case()
    return ah.step_losses(w, c, dr)


def make_model(weights=None, fused=True):
    from chaorec_amd.Model import AdaGCL
    c, w, _, _ = case()
    torch.manual_seed(c["seed"])
    m = AdaGCL(c["U"], c["I"], c["edges"], ah.user_item_dict(c["edges"]), ah.DIM_E, ah.REG_WEIGHT, ah.N_LAYERS, ah.SSL_TEMP, ah.SSL_ALPHA, dev())
    if weights is not None:
        m.load_state_dict({n: torch.from_numpy(np.asarray(v)) for n, v in weights.items()})
    m.fused_edges = fused
    m.generator_2.fused = fused
    return m.train()


def batch():
    c = case()[0]
    return tuple(torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))


def t(x, dtype=torch.float32):
    return accept.to_dev(x, dtype, dev())


# ---- the edge gate ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gate_reference(scaled, layer, training):
    """The float64 restatement of one gate case, the fp32 lines' own deviation per quantity, and the backward's likewise."""
    c, w0, _, dr = case()
    w, x, zero_row = ah.gate_case(c, w0, scaled)
    beta = ah.SSL_TEMP if training else 1.0
    u = dr["u"][layer]
    rng = np.random.default_rng(11 + layer)
    G64 = ah.Graph(c)
    g_val, g_l0 = rng.standard_normal(G64.E), 0.7
    out = {}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        W, G = ah.tensors(w, dtype, False), ah.Graph(c, dtype)
        xx = torch.tensor(x, dtype=dtype)
        with torch.no_grad():
            fwd = ah.gate(W, G, xx, layer, beta, training, u)
        fwd = {k: np.asarray(v.numpy(), dtype=np.float64) for k, v in fwd.items()}
        bwd = ah.gate_backward(W, G, xx, layer, beta, training, u, g_val, g_l0)
        out[name] = dict(fwd, g_nb=bwd[0], g_self=bwd[1], g_b=bwd[2])
    devs = {k: ah.rel_dev(out["f32"][k], out["f64"][k]) for k in ("m", "d", "val", "l0", "g_nb", "g_self", "g_b")}
    return w, x, zero_row, u, g_val, g_l0, out["f64"], devs


def run_gate(m, x, layer, training, u, requires_grad=False):
    from chaorec_amd import ops_extra
    s_nb, s_self, b = m.generator_2.node_scores(x, layer)
    s_nb, s_self, b = (v.detach().clone().requires_grad_(requires_grad) for v in (s_nb, s_self, b))
    beta = ah.SSL_TEMP if training else 1.0
    out = ops_extra.adagcl_edge_gate(m.norm_adj_mat, s_nb, s_self, b, beta, 1e-6 if training else 0.0, training, m._state, m.seed, layer,
                                     t(u) if training else None, return_parts=True)
    return (s_nb, s_self, b), out


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("scaled", [False, True])
def test_gate_forward(scaled, layer, training):
    w, x, zero_row, u, _, _, ref, devs = gate_reference(scaled, layer, training)
    m = make_model(w)
    with torch.no_grad():
        _, (val, l0, mask, d, u_used) = run_gate(m, t(x), layer, training, u)
    for name, got in (("m", mask), ("d", d), ("val", val), ("l0", l0[0])):
        within(got.cpu().numpy(), ref[name], devs[name], f"gate {name} (scaled={scaled}, layer={layer}, training={training})")
    assert (u_used is None) == (not training) and (not training or torch.equal(u_used, t(u)))
    G = ah.graph_arrays(case()[0])
    lens = np.bincount(G["row"], minlength=G["N"])
    mask, d, val = mask.cpu().numpy(), d.cpu().numpy(), val.cpu().numpy()
    assert np.all(d[lens == 0] == 10.0)                                             # an empty row: S = 0 or 1e-6, the factor 10
    if scaled:
        # both clamps are taken, and one row has every mask 0: degree factor 10, every value of the row +0
        assert (mask == 0).sum() > 20 and (mask == 1).sum() > 5 and ((mask > 0) & (mask < 1)).sum() > 20
        assert lens[zero_row] >= 3 and not mask[G["row"] == zero_row].any() and d[zero_row] == 10.0
        assert not val[G["row"] == zero_row].any() and not np.signbit(val[G["row"] == zero_row]).any()
        assert (ref["m"][G["row"] == zero_row] == 0).all()
    else:
        assert training or ((mask > 0) & (mask < 1)).all()                          # init-scale logits reach no clamp without noise


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("layer", [0, 1])
@pytest.mark.parametrize("scaled", [False, True])
def test_gate_backward(scaled, layer, training):
    w, x, _, u, g_val, g_l0, ref, devs = gate_reference(scaled, layer, training)
    near = (np.abs(ref["stretched"]) < 1e-6) | (np.abs(ref["stretched"] - 1.0) < 1e-6)
    assert near.sum() <= 0.01 * near.size
    G = ah.graph_arrays(case()[0])
    keep_row = np.ones(G["N"], bool)
    keep_col = np.ones(G["N"], bool)
    keep_row[G["row"][near]] = False          # an entry at a clamp edge reaches its row's s_nb and its column's s_self: left out
    keep_col[G["col"][near]] = False
    m = make_model(w)
    runs = []
    for _ in range(2):
        (s_nb, s_self, b), (val, l0, *_) = run_gate(m, t(x), layer, training, u, requires_grad=True)
        ((t(g_val) * val).sum() + g_l0 * l0[0]).backward()
        runs.append((s_nb.grad.clone(), s_self.grad.clone(), b.grad.clone()))
    assert all(torch.equal(a, b_) for a, b_ in zip(*runs)), "two runs of the backward differ"
    g_nb, g_self, g_b = (v.cpu().numpy() for v in runs[0])
    tag = f"(scaled={scaled}, layer={layer}, training={training})"
    within(np.where(keep_row, g_nb, 0), np.where(keep_row, ref["g_nb"], 0), devs["g_nb"], f"g_s_nb {tag}")
    within(np.where(keep_col, g_self, 0), np.where(keep_col, ref["g_self"], 0), devs["g_self"], f"g_s_self {tag}")
    if not near.any():
        within(g_b[0], ref["g_b"], devs["g_b"], f"g_b {tag}")
    assert np.abs(ref["g_nb"]).max() > 0 and np.abs(ref["g_self"]).max() > 0


def test_gate_gradient_reaches_the_layers_through_autograd():
    """The node scores stay plain autograd ops: the gate's cotangents arrive at generator 2's parameters of the layer."""
    w, x, _, u, g_val, _, _, _ = gate_reference(False, 0, True)
    m = make_model(w)
    s_nb, s_self, b = m.generator_2.node_scores(t(x), 0)
    from chaorec_amd import ops_extra
    val, l0 = ops_extra.adagcl_edge_gate(m.norm_adj_mat, s_nb, s_self, b, ah.SSL_TEMP, 1e-6, True, m._state, m.seed, 0, t(u))
    ((t(g_val) * val).sum() + l0[0]).backward()
    got = {n for n, p in m.generator_2.named_parameters() if p.grad is not None and bool(p.grad.abs().sum() > 0)}
    assert got == {"nblayers_0.0.weight", "nblayers_0.0.bias", "selflayers_0.0.weight", "selflayers_0.0.bias", "attentions_0.0.weight",
                   "attentions_0.0.bias"}


# ---- device draws -------------------------------------------------------------------------------------------------------------
def test_device_draw():
    from chaorec_amd import graph, ops_extra, sparse
    N = 256                                                                            # the complete pattern: E = 65 536, rows of 256
    r = torch.arange(N).repeat_interleave(N)
    cc = torch.arange(N).repeat(N)
    st = sparse._dropout_structure(graph.coo_to_csr_coalesced(r, cc, torch.ones(N * N), N, N, symmetric=True)).to(dev())
    assert st.nnz == 65536
    state = torch.zeros(2, dtype=torch.int64, device=dev())
    z, b = torch.zeros(N, device=dev()), torch.zeros(1, device=dev())

    def draw(salt=0):
        out = ops_extra.adagcl_edge_gate(st, z, z, b, 0.5, 1e-6, True, state, 1234, salt, None, return_parts=True)
        return out[4].cpu().numpy().astype(np.float64), out[2].cpu().numpy().astype(np.float64)

    ops_extra.adagcl_tick(state)
    assert state.tolist() == [1, 1]
    u1, m1 = draw()
    u1b, _ = draw()
    other_salt, _ = draw(1)
    ops_extra.adagcl_tick(state)
    u2, _ = draw()
    assert np.array_equal(u1, u1b) and not np.array_equal(u1, u2) and not np.array_equal(u1, other_salt)
    assert abs(np.corrcoef(u1, u2)[0, 1]) < 5 / np.sqrt(u1.size)
    for u in (u1, u2):
        assert u.min() >= 1e-7 and u.max() <= 1.0 - 1e-7
        assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / u.size)
        assert abs(u.var() - 1 / 12) <= 5 * np.sqrt((1 / 80 - 1 / 144) / u.size)
    # the mask the launch made of its own draws: logit 0, beta 0.5 -> clamp(1.5 sigmoid(2 (log u - log(1 - u))) - 0.45, 0, 1)
    ref = np.clip(1.5 / (1.0 + np.exp(-2.0 * (np.log(u1) - np.log1p(-u1)))) - 0.45, 0.0, 1.0)
    assert np.abs(m1 - ref).max() <= 4 * ULP
    # the evaluation form draws nothing and hands no u back
    assert ops_extra.adagcl_edge_gate(st, z, z, b, 1.0, 0.0, False, state, 1234, 0, None, return_parts=True)[4] is None


@pytest.mark.parametrize("salt", [0, 1])
def test_device_draw_is_the_host_generator_bit_for_bit(salt):
    """On the ragged 40-node graph of vae_ops_host.ragged_rows, two ticks in: u = clamp(lo + (hi - lo) uniform24, lo, hi) in fp32."""
    from chaorec_amd import ops_extra
    st = vo.ragged_structure(dev())
    lens = np.diff(vo.ragged_rows()[0])
    assert st.n_rows == 40 and lens.max() == 70 and lens.min() == 0 and lens[lens < 70].max() <= 9
    state = torch.zeros(2, dtype=torch.int64, device=dev())
    ops_extra.adagcl_tick(state)
    ops_extra.adagcl_tick(state)
    z, b = torch.zeros(40, device=dev()), torch.zeros(1, device=dev())
    u = ops_extra.adagcl_edge_gate(st, z, z, b, 0.5, 1e-6, True, state, 1234, salt, None, return_parts=True)[4].cpu().numpy()
    lo, hi = np.float32(1e-7), np.float32(0.99999988)
    ref = vo.vae_uniform(vo.vae_key(1234, 2, salt), 0, np.arange(st.nnz), 24)
    ref = np.clip(lo + (hi - lo) * ref, lo, hi)
    assert ref.dtype == np.float32 and u.dtype == np.float32 and np.array_equal(u.view(np.uint32), ref.view(np.uint32))


def test_the_three_step_ticks_count_alike():
    from chaorec_amd import ops_extra
    ticks = (ops_extra.dualvae_tick, ops_extra.mvgae_tick, ops_extra.adagcl_tick)
    states = [torch.zeros(2, dtype=torch.int64, device=dev()) for _ in ticks]
    for step in (1, 2):
        for tick, state in zip(ticks, states):
            tick(state)
        assert all(state.tolist() == [step, step] for state in states)


# ---- the edge keep ------------------------------------------------------------------------------------------------------------
def test_keep_mask_count_and_values_meet_the_reference():
    c, w, g, dr = case()
    m = make_model(w)
    m.feed_draws(randn=dr["randn"][:1])
    view, keep, logits = m.generator_generate(m.generator_1, return_parts=True)
    keep, logits = keep.cpu().numpy(), logits.cpu().numpy()
    _, keep64, logits64 = ah.keep_view(ah.tensors(w, requires_grad=False), ah.Graph(c), torch.tensor(dr["randn"][0], dtype=torch.float64))
    near = np.abs(logits64.numpy()) < 16 * g["keep_logit_abs_dev"]
    print("entries within 16 x the reference's logit deviation of 0:", int(near.sum()), "flips:", int((keep != g["keep"]).sum()))
    assert near.sum() <= 0.01 * g["E"] and np.array_equal(keep[~near], g["keep"][~near]) and np.array_equal(keep64.numpy()[~near], g["keep"][~near])
    within(logits, logits64.numpy(), g["dev_keep_logits"], "keep logits")
    assert int(keep.sum()) == int(g["keep"].sum()) or near.any()
    if not (keep != g["keep"]).any():
        within(view.val.cpu().numpy(), g["keep_vals"].astype(np.float64), max(g["dev_keep_vals"], ULP), "kept values")
    st = m.norm_adj_mat
    assert torch.equal(view.val_t, view.val[st.transpose_entry.long()]) and not view.val[~torch.from_numpy(keep).to(dev())].any()


def _keep_weights(rng, b2=0.0, w2_scale=1.0):
    return (rng.standard_normal((64, 64)) / 8).astype(np.float32), (0.1 * rng.standard_normal(64)).astype(np.float32), \
        (w2_scale * rng.standard_normal((1, 64)) / 8).astype(np.float32), np.array([b2], np.float32)


def _keep_restated(arrays, z, W1, b1, w2, b2, dtype=torch.float64):
    G = ah.Graph(None, dtype, arrays=arrays)
    W = {"generator_1.decoder.decoder.1.weight": W1, "generator_1.decoder.decoder.1.bias": b1, "generator_1.decoder.decoder.3.weight": w2,
         "generator_1.decoder.decoder.3.bias": b2}
    return ah.keep_from_rows(ah.tensors(W, dtype, requires_grad=False), G, torch.tensor(z, dtype=dtype))


def test_keep_on_a_graph_smaller_than_one_tile():
    from chaorec_amd import graph, ops_extra, sparse
    row, col = np.array([0, 0, 1, 1, 2]), np.array([1, 2, 0, 1, 0])                   # 5 entries, symmetric pattern, one diagonal
    val = np.array([0.5, 0.25, 0.5, 1.0, 0.25], np.float32)
    arrays = dict(N=4, E=5, row=row, col=col, val=val, tentry=np.array([2, 4, 0, 3, 1]))
    st = sparse._dropout_structure(graph.coo_to_csr_coalesced(torch.from_numpy(row), torch.from_numpy(col), torch.from_numpy(val), 4, 4,
                                                              symmetric=True)).to(dev())
    assert st.transpose_entry.tolist() == [2, 4, 0, 3, 1]
    rng = np.random.default_rng(5)
    z = rng.standard_normal((4, 64)).astype(np.float32)
    W1, b1, w2, b2 = _keep_weights(rng)
    out, keep, kept, logits = ops_extra.adagcl_edge_keep(st, t(z), t(W1), t(b1), t(w2), t(b2), st.val, return_logits=True)
    vals64, keep64, logits64 = _keep_restated(arrays, z, W1, b1, w2, b2)
    vals32, _, logits32 = _keep_restated(arrays, z, W1, b1, w2, b2, torch.float32)      # the same lines in fp32: their own deviation
    assert np.abs(logits64.numpy()).min() > 1e-3 and 0 < int(keep64.sum()) < 5
    assert np.array_equal(keep.cpu().numpy(), keep64.numpy()) and int(kept) == int(keep64.sum())
    within(logits.cpu().numpy(), logits64.numpy(), ah.rel_dev(logits32.numpy(), logits64.numpy()), "keep logits, 5 entries")
    within(out.cpu().numpy(), vals64.numpy(), ah.rel_dev(vals32.numpy(), vals64.numpy()), "kept values, 5 entries")


def test_keep_that_keeps_nothing_or_everything():
    """A weight set that keeps nothing: every value +0, no NaN, count 0; and one that keeps everything: the values unchanged."""
    from chaorec_amd import ops_extra
    c, w, _, _ = case()
    m = make_model(w)
    st = m.norm_adj_mat
    rng = np.random.default_rng(1)
    z = t(rng.standard_normal((st.n_rows, 64)).astype(np.float32))
    W1, b1, w2, _ = _keep_weights(rng, w2_scale=0.0)
    out, keep, kept = ops_extra.adagcl_edge_keep(st, z, t(W1), t(b1), t(w2), t(np.array([-5.0], np.float32)), st.val)
    assert int(kept) == 0 and not keep.any() and not out.any() and bool(torch.isfinite(out).all()) and not torch.signbit(out).any()
    out, keep, kept = ops_extra.adagcl_edge_keep(st, z, t(W1), t(b1), t(w2), t(np.array([5.0], np.float32)), st.val)
    assert int(kept) == st.nnz and bool(keep.all()) and torch.equal(out, st.val)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _four_losses(m, dr):
    """The four losses on FIXED weights, each alone, with the gradient it produces (as golden/gen_adagcl.py runs the reference)."""
    users, pos, neg = batch()
    m.feed_draws(randn=dr["randn"], u=dr["u"])
    params = dict(m.named_parameters())
    out = {"grads": {}}

    def grads_of(name):
        got = {n: params[n].grad.detach().cpu().numpy().copy() for n in ah.WITH_GRAD[name]}
        assert all(params[n].grad is None or not params[n].grad.any() for n in ah.NAMES if n not in got), name
        m.zero_grad(set_to_none=True)
        return got

    l1, out1, out2 = m.loss_1(users, pos, neg)
    l1.backward()
    out["loss_1"], out["grads"]["loss_1"] = float(l1.detach()), grads_of("loss_1")
    l2 = m.loss_2(users, pos, neg, out1, out2)
    l2.backward()
    out["loss_2"], out["grads"]["loss_2"] = float(l2.detach()), grads_of("loss_2")
    l3 = m.bpr_reg_loss(users, pos, neg)
    l3.backward()
    out["bpr_reg_loss"], out["grads"]["bpr_reg_loss"] = float(l3.detach()), grads_of("bpr_reg_loss")
    l4 = m.gen_loss(users, pos, neg)
    l4.backward()
    out["gen_loss"], out["grads"]["gen_loss"] = float(l4.detach()), grads_of("gen_loss")
    assert not m._draws["randn"] and not m._draws["u"]
    return out


@pytest.mark.parametrize("fused", [True, False])
def test_four_losses_and_their_gradients(fused):
    """fused_edges = True and False, each against the float64 restatement on the same draws under the same bound."""
    c, w, g, dr = case()
    got, host = _four_losses(make_model(w, fused), dr), host_step()
    for name in ah.LOSSES:
        within(got[name], host[name], g[f"dev_{name}"], f"{name} (fused={fused})")
        for k, n in enumerate(ah.WITH_GRAD[name]):
            within(got["grads"][name][n], host["grads"][name][n], g[f"dev_grads_{name}"][k], f"{name}: grad {n} (fused={fused})")


def test_generated_views_meet_the_reference():
    """Generator 2's values for both layers in both forms, through the model's own calls."""
    c, w, g, dr = case()
    m = make_model(w)
    W, G = ah.tensors(w, requires_grad=False), ah.Graph(c)
    x64 = torch.cat([W["uEmbeds"], W["iEmbeds"]], 0)
    with torch.no_grad():
        x0 = torch.cat([m.uEmbeds, m.iEmbeds], 0)
        for training, tag in ((False, "eval"), (True, "train")):
            beta = ah.SSL_TEMP if training else 1.0
            v0 = m.generator_2.gate(x0, 0, beta, training, t(dr["u"][0]) if training else None)[0]
            h0 = ah.gate(W, G, x64, 0, beta, training, dr["u"][0])
            within(v0.cpu().numpy(), h0["val"].numpy(), g[f"dev_gate_{tag}0"], f"generator 2 values {tag}0")
            x1 = m.gcnLayers[0](m.generator_2._view(v0), x0)
            v1 = m.generator_2.gate(x1, 1, beta, training, t(dr["u"][1]) if training else None)[0]
            h1 = ah.gate(W, G, ah.spmm(G, h0["val"], x64), 1, beta, training, dr["u"][1])
            within(v1.cpu().numpy(), h1["val"].numpy(), g[f"dev_gate_{tag}1"], f"generator 2 values {tag}1")


def test_three_steps_of_the_training_loop():
    """train_and_evaluate's AdaGCL branch -- three Adam optimizers, the generators stepped twice -- over one batch three times."""
    from chaorec_amd import epochs as te
    c, w, g, _ = case()
    drs = ah.draws(c, ah.N_STEPS, seed_offset=2)
    m = make_model(w)
    for dr in drs:
        m.feed_draws(randn=dr["randn"], u=dr["u"])
    total = te._train_epoch_adagcl(m, [batch()] * ah.N_STEPS, types.SimpleNamespace(param_groups=[{"lr": ah.LR}]))
    host_final, host_losses = ah.trajectory(w, c, drs)
    within(total, host_losses.sum(), g["dev_traj_losses"], "the epoch's summed loss")
    sd = {n: v.detach().cpu().numpy() for n, v in m.state_dict().items()}
    for k, n in enumerate(ah.NAMES):
        within(sd[n] - w[n], host_final[n] - w[n], g["dev_traj"][k], f"update of {n}")
    assert np.array_equal(m.generator_2.features.cpu().numpy(), np.concatenate([w["uEmbeds"], w["iEmbeds"]], 0))
    assert not m._draws["randn"] and not m._draws["u"]


def test_device_drawn_step_is_finite_and_repeats_by_seed():
    """No given draws: the uniform draws come from the launch, keyed by the step counter gen_loss advances."""
    c, w, _, _ = case()
    users, pos, neg = batch()
    out = []
    for _ in range(2):
        m = make_model(w)
        torch.manual_seed(3)
        l = m.gen_loss(users, pos, neg)
        l.backward()
        out.append((float(l.detach()), m.generator_2.attentions_1[0].weight.grad.cpu().numpy().copy()))
        assert m._state.tolist() == [1, 1] and np.isfinite(out[-1][1]).all() and np.isfinite(out[-1][0])
    # (torch's gathers accumulate their backward in no fixed order: equal draws show as agreement far below a draw's effect)
    assert ah.rel_dev(out[0][0], out[1][0]) <= 1e-5 and ah.rel_dev(out[0][1], out[1][1]) <= 1e-4
    torch.manual_seed(3)
    m.zero_grad()
    l = m.gen_loss(users, pos, neg)                       # the next step: other uniform draws under the same torch seed
    assert m._state.tolist() == [2, 2] and ah.rel_dev(float(l.detach()), out[0][0]) > 1e-4


def test_rank_list():
    c, w, g, _ = case()
    m = make_model(w).eval()
    got = m.gene_ranklist(topk=ah.TOPK).numpy() - c["U"]
    s = ah.rank_scores(w, c)
    assert got.shape == (c["U"], ah.TOPK) and got.min() >= 0 and got.max() < c["I"]
    assert all(len(set(r)) == ah.TOPK for r in got.tolist())
    best = np.sort(s, 1)[:, ::-1][:, :ah.TOPK]
    tol = 1e-6 * np.abs(s).max()
    assert np.abs(np.take_along_axis(s, got, 1) - best).max() <= tol                  # the float64 scores of the listed items are the best ten
    ref = g["ranklist"].astype(np.int64) - c["U"]
    differ = got != ref
    print("positions that differ from the reference's list:", int(differ.sum()))
    assert np.abs(np.take_along_axis(s, got, 1) - np.take_along_axis(s, ref, 1))[differ].max(initial=0.0) <= tol
