"""Grade on the MI355X: the three-view node (csrc/grade.hip: the MLP per undirected pair, the weighted row sums, the values) and
the model (three losses with their gradients, the plain-torch switch, the generated views, a 3-step trajectory through the
training loop's own branch, the rank list) against the float64 restatement of tests/grade_host.py.

Bounds.  Model quantities: 4 x max(the deviation the golden stores for the reference's own fp32 run, 2^-24).  Kernel cases the
golden has no run of: the same rule with the deviation measured here, the restatement's lines in torch fp32 on the CPU against
the float64 ones.  Keep masks match exactly outside the window |logit64| < 16 x that logit deviation, which may hold at most
1 % of E.  Nothing is compared with the code under test.  Every kernel case is launched once and shared (kernel_run)."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import grade_host as gh  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ULP = accept.ULP24
D_EMPTY = float(np.float32(1.0) / np.sqrt(np.float32(1e-7)))          # (1e-7f)^-1/2


def within(x, ref, dev, what):
    accept.within(what, x, ref, dev, ULP)


def dev():
    return torch.device("cuda:0")


def t(x, dtype=torch.float32):
    return accept.to_dev(x, dtype, dev())


@functools.lru_cache(maxsize=None)
def case():
    g = gh.load_fixture(GOLDEN)
    c = gh.small_case(g["seed"])
    return c, gh.init_weights(c), g, gh.draws(c, 1)[0]


@functools.lru_cache(maxsize=None)
def host_step():
    c, w, _, dr = case()
    return gh.step_losses(w, c, dr)


def make_model(weights=None, fused=True):
    from chaorec_amd.Model import Grade
    c, w, _, _ = case()
    torch.manual_seed(c["seed"])
    m = Grade(c["U"], c["I"], c["edges"], gh.user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]),
              gh.DIM_E, gh.REG_WEIGHT, gh.N_LAYERS, gh.SSL_TEMP, gh.SSL_ALPHA, gh.SSL_TEMP2, gh.NOISE_ALPHA, dev())
    if weights is not None:
        m.load_state_dict({n: torch.from_numpy(np.asarray(v)) for n, v in weights.items()})
    m.fused_edges = fused
    return m.train()


def batch():
    c = case()[0]
    return tuple(torch.from_numpy(c[k]) for k in ("users", "pos", "neg"))


# ---- the three-view node ------------------------------------------------------------------------------------------------------
TINY = dict(N=4, E=5, row=np.array([0, 0, 1, 1, 2]), col=np.array([1, 2, 0, 1, 0]), val=np.ones(5, np.float32),
            tentry=np.array([2, 4, 0, 3, 1]))                                 # 5 entries, symmetric pattern, one diagonal, an empty row


def _mlp(rng, b2=0.0, w2_scale=1.0):
    return [(rng.standard_normal((64, 64)) / 8).astype(np.float32), (0.1 * rng.standard_normal(64)).astype(np.float32),
            (w2_scale * rng.standard_normal(64) / 8).astype(np.float32), np.array([b2], np.float32)]


def _restated(arrays, z, mlp, dtype):
    G = gh.Graph(None, dtype, arrays=arrays)
    out = gh.view_from_rows(*(torch.tensor(x, dtype=dtype) for x in mlp), G, torch.tensor(z, dtype=dtype))
    return {k: v.numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def kernel_inputs(name):
    """-> (arrays, z [G, N, 64], [mlp per generator]) of a kernel case."""
    if name == "tiny":
        rng = np.random.default_rng(5)
        return TINY, rng.standard_normal((1, 4, 64)).astype(np.float32), [_mlp(rng)]
    arrays = gh.graph_arrays(case()[0])
    N = arrays["N"]
    rng = np.random.default_rng(77)
    zs = [(0.6 * rng.standard_normal((N, 64))).astype(np.float32) for _ in range(3)]
    mlps = [_mlp(rng) for _ in range(3)]
    if name in ("g1_0", "g1_1", "g1_2"):
        k = int(name[-1])
        return arrays, np.stack(zs[k:k + 1]), mlps[k:k + 1]
    if name == "g3":
        return arrays, np.stack(zs), mlps
    if name == "scaled":
        # the last layer times 30, the bias minus the median logit: about half the entries kept, logits of both signs far from 0
        W1, b1, w2, _ = mlps[0]
        w2 = (30.0 * w2).astype(np.float32)
        # (the median: the middle of the widest gap between the 21 central distinct logits, so that no logit sits at 0)
        u = np.unique(_restated(arrays, zs[0], [W1, b1, w2, np.zeros(1, np.float32)], torch.float64)["logit"])
        mid = u[len(u) // 2 - 10:len(u) // 2 + 11]
        k = int(np.argmax(np.diff(mid)))
        med = float(0.5 * (mid[k] + mid[k + 1]))
        return arrays, np.stack(zs[:1]), [[W1, b1, w2, np.array([-med], np.float32)]]
    W1, b1, w2, _ = _mlp(rng, w2_scale=0.0)
    return arrays, np.stack(zs[:1]), [[W1, b1, w2, np.array([-5.0 if name == "none" else 5.0], np.float32)]]


def _structure(arrays):
    from chaorec_amd import graph, sparse
    csr = graph.coo_to_csr_coalesced(torch.from_numpy(arrays["row"]), torch.from_numpy(arrays["col"]), torch.from_numpy(arrays["val"]),
                                     arrays["N"], arrays["N"], symmetric=True)
    st = sparse._dropout_structure(csr).to(dev())
    assert np.array_equal(st.transpose_entry.cpu().numpy(), arrays["tentry"]) and np.array_equal(st.col.cpu().numpy(), arrays["col"])
    return st


def _launch(st, z, mlps):
    from chaorec_amd import ops_extra
    W1, b1, w2, b2 = (t(np.stack([m[k] for m in mlps])) for k in range(4))
    out = ops_extra.grade_views(st, t(z), W1, b1, w2, b2.reshape(-1), return_parts=True)
    return dict(zip(("val", "keep", "kept", "logit", "d"), (x.cpu().numpy() for x in out)))


@functools.lru_cache(maxsize=None)
def kernel_run(name):
    arrays, z, mlps = kernel_inputs(name)
    return _launch(_structure(arrays), z, mlps)


def check_views(name, min_rows_all_dropped=0):
    """Logits, d, values, keep and count of a kernel case against the float64 restatement."""
    arrays, z, mlps = kernel_inputs(name)
    got = kernel_run(name)
    E, N = arrays["E"], arrays["N"]
    assert got["val"].shape == (len(mlps), E) and got["d"].shape == (len(mlps), N) and got["keep"].dtype == np.bool_
    lens = np.bincount(arrays["row"], minlength=N)
    for g, mlp in enumerate(mlps):
        r64, r32 = _restated(arrays, z[g], mlp, torch.float64), _restated(arrays, z[g], mlp, torch.float32)
        abs_dev = float(np.abs(r32["logit"] - r64["logit"]).max())
        near = np.abs(r64["logit"]) < 16 * max(abs_dev, ULP)
        flips = int((got["keep"][g] != r64["keep"]).sum())
        print(f"{name}[{g}]: kept {int(r64['keep'].sum())} of {E}, in the window {int(near.sum())}, flips {flips}")
        assert near.sum() <= 0.01 * E and np.array_equal(got["keep"][g][~near], r64["keep"][~near])
        within(got["logit"][g], r64["logit"], gh.rel_dev(r32["logit"], r64["logit"]), f"{name}[{g}] logits")
        assert np.array_equal(got["keep"][g], got["val"][g] != 0) and not np.signbit(got["val"][g]).any() and np.isfinite(got["val"][g]).all()
        assert int(got["kept"][g]) == int(got["keep"][g].sum())
        assert np.array_equal(got["val"][g][arrays["tentry"]].view(np.uint32), got["val"][g].view(np.uint32))      # symmetric bit for bit
        kept_in_row = np.bincount(arrays["row"], weights=got["keep"][g], minlength=N)
        assert np.all(got["d"][g][kept_in_row == 0] == np.float32(D_EMPTY))
        assert int(((lens >= 4) & (kept_in_row == 0)).sum()) >= min_rows_all_dropped
        if flips == 0:
            # d is compared where a row keeps something: an all-dropped row's (1e-7)^-1/2 is asserted exactly above
            some = kept_in_row > 0
            if some.any():
                within(got["d"][g][some], r64["d"][some], gh.rel_dev(r32["d"][some], r64["d"][some]), f"{name}[{g}] d")
            within(got["val"][g], r64["val"], gh.rel_dev(r32["val"], r64["val"]), f"{name}[{g}] values")


def test_owner_list_on_the_device():
    from chaorec_amd import ops_extra
    arrays = gh.graph_arrays(case()[0])
    st = _structure(arrays)
    owner = ops_extra.grade_pair_owner(st)
    assert owner.dtype == torch.int32 and owner.is_cuda and ops_extra.grade_pair_owner(st) is owner
    assert np.array_equal(owner.cpu().numpy(), gh.owner_list(arrays)) and owner.numel() == arrays["E"] // 2


def test_views_on_a_graph_smaller_than_one_tile():
    check_views("tiny")
    assert kernel_run("tiny")["d"][0][3] == np.float32(D_EMPTY)                      # node 3 has no entry


@pytest.mark.parametrize("name", ["g1_0", "g1_1", "g1_2", "g3"])
def test_views_on_the_small_case(name):
    check_views(name)


def test_a_slice_of_three_generators_is_the_single_call_bit_for_bit():
    g3 = kernel_run("g3")
    for g in range(3):
        g1 = kernel_run(f"g1_{g}")
        for k in ("val", "logit", "d"):
            assert np.array_equal(g3[k][g].view(np.uint32), g1[k][0].view(np.uint32)), (g, k)
        assert np.array_equal(g3["keep"][g], g1["keep"][0]) and int(g3["kept"][g]) == int(g1["kept"][0])


def test_views_with_about_half_kept_and_rows_all_dropped():
    check_views("scaled", min_rows_all_dropped=1)
    got = kernel_run("scaled")
    assert 0.3 <= got["keep"][0].mean() <= 0.7


def test_views_that_keep_nothing_or_everything():
    none, every = kernel_run("none"), kernel_run("all")
    E = none["val"].shape[1]
    assert int(none["kept"][0]) == 0 and not none["keep"].any() and not none["val"].any() and not np.signbit(none["val"]).any()
    assert np.isfinite(none["val"]).all() and np.isfinite(none["d"]).all() and np.all(none["d"] == np.float32(D_EMPTY))
    assert int(every["kept"][0]) == E and every["keep"].all()
    check_views("all")


def test_two_runs_give_equal_bits():
    arrays, z, mlps = kernel_inputs("g3")
    again, first = _launch(_structure(arrays), z, mlps), kernel_run("g3")
    for k in ("val", "logit", "d"):
        assert np.array_equal(again[k].view(np.uint32), first[k].view(np.uint32)), k
    assert np.array_equal(again["keep"], first["keep"]) and np.array_equal(again["kept"], first["kept"])


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _three_losses(m, dr):
    """The three losses on FIXED weights, each alone, with the gradient it produces (as golden/gen_grade.py runs the reference)."""
    users, pos, neg = batch()
    m.feed_draws(randn=dr["randn1"] + dr["randn2"], rand=dr["rand"])
    params = dict(m.named_parameters())
    out = {"grads": {}}
    for name, call in (("loss_1", m.loss_1), ("bpr_reg_loss", m.bpr_reg_loss), ("gen_loss", m.gen_loss)):
        l = call(users, pos, neg)
        l.backward()
        out[name] = float(l.detach())
        out["grads"][name] = {n: params[n].grad.detach().cpu().numpy().copy() for n in gh.WITH_GRAD[name]}
        assert all(params[n].grad is None for n in gh.NAMES if n not in out["grads"][name]), name          # no gradient where none belongs
        m.zero_grad(set_to_none=True)
    assert not m._draws["randn"] and not m._draws["rand"]
    return out


def test_item_graph_is_the_reference_s():
    c = case()[0]
    G = gh.graph_arrays(c)
    m = make_model()
    rows = np.repeat(np.arange(c["I"]), np.diff(m.mm_adj.rowptr.cpu().numpy()))
    assert np.array_equal(rows, G["mm_row"]) and np.array_equal(m.mm_adj.col.cpu().numpy(), G["mm_col"])
    assert gh.rel_dev(m.mm_adj.val.cpu().numpy(), G["mm_val"]) <= 2 * ULP


@pytest.mark.parametrize("fused", [True, False])
def test_three_losses_and_their_gradients(fused):
    """fused_edges = True and False, each against the float64 restatement on the same draws under the same bound.

    Measured on the MI355X: largest deviation / bound 0.47.  The decoder of gen_loss runs in float64 over positives and negatives
    together (vgae_decoder._pred_pair): as two fp32 calls, generator 3's last-bias gradient -- 128 terms that cancel 41 : 1, each
    half rounded at its own magnitude of 0.25 -- was 1.496e-6 off against a bound of 1.099e-6; now 3.1e-8."""
    c, w, g, dr = case()
    got, host = _three_losses(make_model(w, fused), dr), host_step()
    for name in gh.LOSSES:
        within(got[name], host[name], g[f"dev_{name}"], f"{name} (fused={fused})")
        for k, n in enumerate(gh.WITH_GRAD[name]):
            within(got["grads"][name][n], host["grads"][name][n], g[f"dev_grads_{name}"][k], f"{name}: grad {n} (fused={fused})")


def test_generated_views_meet_the_reference():
    """generator_generate for each generator (the G = 1 call) and loss_1's one call for all three, on loss_1's normal tables."""
    c, w, g, dr = case()
    m = make_model(w)
    W, G = gh.tensors(w, requires_grad=False), gh.Graph(c)
    st = m.norm_adj_mat
    singles = []
    for k, gen in enumerate((m.generator_1, m.generator_2, m.generator_3)):
        m.feed_draws(randn=dr["randn1"][k:k + 1])
        view, keep, logits, d = m.generator_generate(gen, return_parts=True)
        singles.append(view.val)
        keep, logits = keep.cpu().numpy(), logits.cpu().numpy()
        mine = gh.view(W, G, k + 1, torch.tensor(dr["randn1"][k], dtype=torch.float64))
        near = np.abs(mine["logit"].numpy()) < 16 * g["logit_abs_dev"]
        print(f"generator {k + 1}: in the window {int(near.sum())}, flips {int((keep != g['keep'][k]).sum())}")
        assert near.sum() <= 0.01 * g["E"] and np.array_equal(keep[~near], g["keep"][k][~near])
        assert np.array_equal(mine["keep"].numpy()[~near], g["keep"][k][~near])
        within(logits, mine["logit"].numpy(), g["dev_view_logits"][k], f"generator {k + 1} logits")
        if not (keep != g["keep"][k]).any():
            within(view.val.cpu().numpy(), mine["val"].numpy(), g["dev_view_vals"][k], f"generator {k + 1} values")
            within(view.val.cpu().numpy(), g["view_vals"][k].astype(np.float64), max(g["dev_view_vals"][k], ULP), f"generator {k + 1} values, golden")
        assert torch.equal(view.val_t, view.val[st.transpose_entry.long()]) and torch.equal(view.val_t, view.val)
    m.feed_draws(randn=dr["randn1"])
    for k, view in enumerate(m.generate_views()):
        assert torch.equal(view.val, singles[k]) and view.structure is st, k
    assert not m._draws["randn"]


def test_three_steps_of_the_training_loop():
    """train_and_evaluate's Grade branch -- four Adam optimizers -- over one batch three times; updates as final - initial.

    Measured on the MI355X: largest deviation / bound 0.97, at the update of generator_3.decoder.decoder.1.weight (2.075e-4
    against 2.141e-4; 1.73 before the decoder's gradients were accumulated in float64); the next largest is 0.57."""
    from chaorec_amd import epochs as te
    c, w, g, _ = case()
    drs = gh.draws(c, gh.N_STEPS, seed_offset=2)
    m = make_model(w)
    for dr in drs:
        m.feed_draws(randn=dr["randn1"] + dr["randn2"], rand=dr["rand"])
    total = te._train_epoch_grade(m, [batch()] * gh.N_STEPS, types.SimpleNamespace(param_groups=[{"lr": gh.LR}]))
    host_final, host_losses = gh.trajectory(w, c, drs)
    within(total, host_losses.sum(), g["dev_traj_losses"], "the epoch's summed loss")
    sd = {n: v.detach().cpu().numpy() for n, v in m.state_dict().items()}
    for k, n in enumerate(gh.NAMES):
        within(sd[n] - w[n], host_final[n] - w[n], g["dev_traj"][k], f"update of {n}")
    assert not m._draws["randn"] and not m._draws["rand"]


def test_a_step_without_fed_draws_is_finite():
    c, w, _, _ = case()
    users, pos, neg = batch()
    m = make_model(w)
    torch.manual_seed(3)
    for call in (m.loss_1, m.bpr_reg_loss, m.gen_loss):
        l = call(users, pos, neg)
        l.backward()
        assert np.isfinite(float(l.detach()))
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_rank_list():
    c, w, g, _ = case()
    m = make_model(w).eval()
    got = m.gene_ranklist(topk=gh.TOPK).numpy() - c["U"]
    s = gh.rank_scores(w, c)
    assert got.shape == (c["U"], gh.TOPK) and got.min() >= 0 and got.max() < c["I"]
    assert all(len(set(r)) == gh.TOPK for r in got.tolist())
    best = np.sort(s, 1)[:, ::-1][:, :gh.TOPK]
    tol = 1e-6 * np.abs(s).max()
    assert np.abs(np.take_along_axis(s, got, 1) - best).max() <= tol                  # the float64 scores of the listed items are the best ten
