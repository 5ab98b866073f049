"""The per-op restatements of tests/vae_ops_host.py, checked on the CPU: chained into one training step of each model on
the `small` fixtures they must reproduce multvae_host.step, macridvae_host.step and dualvae_host.step -- restatements that
tests/test_*vae_host.py tie to the reference's goldens -- in values and gradients to float64 rounding; the ranking ops
(macrid_scores, dualvae_scores) fed those restatements' own latents give their eval-mode scores, and masked() is checked
by hand; and the numpy restatement of the counter RNG is in range, deterministic and BITS-dependent.  No GPU."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dualvae_host as dh  # noqa: E402
import macridvae_host as ch  # noqa: E402
import multvae_host as mh  # noqa: E402
import vae_ops_host as vo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
RTOL = 1e-13          # float64 rounding of sums of a few hundred terms in another order (measured: at most 3e-15)


def same(got, want, what):
    d = mh.rel_dev(got, want)
    print(f"{what}: {d:.3e}")
    assert d <= RTOL, f"{what}: {d:.3e}"


def t64(x):
    return torch.as_tensor(np.asarray(x)).to(torch.float64)


def test_multvae_ops_chain_into_the_step():
    """Op by op through run(): the decoder's dz is the encoder's upstream gradient, as autograd hands it on the device."""
    g = mh.load_fixture(GOLDEN, "small")
    Wq, bq, Wp, bp = g["Wq"], g["bq"], g["Wp"], g["bp"]
    reg, uc = float(g["reg_weight"]), 123456
    ref = mh.step((Wq, bq, Wp, bp), g["rowptr"], g["col"], g["users"], g["keep"], g["eps"], uc, reg)
    x = vo.dense_rows(g["rowptr"], g["col"], g["users"], g["I"])
    mask = mh.mask_from_flags(g["keep"], g["rowptr"], g["col"], g["users"], g["I"])
    enc_in = dict(Wq_t=np.ascontiguousarray(Wq.T), bq=bq, x=x, mask=mask, eps=g["eps"])
    enc, _ = vo.run(vo.multvae_encode_fwd, enc_in)
    dec, dgr = vo.run(vo.multvae_decode_fwd, dict(z=enc["z"], Wp=Wp, bp=bp, x=x), wrt=("z", "Wp", "bp"),
                      upstream={"neg_ll": 1.0, "sumsq": reg * reg})
    _, egr = vo.run(vo.multvae_encode_fwd, enc_in, wrt=("Wq_t", "bq"),
                    upstream={"z": dgr["z"], "kl": ref["anneal"], "sumsq": reg * reg})
    same(enc["z"], ref["z"], "z")
    same(enc["kl"], ref["kl"], "kl")
    same(dec["lse"], ref["lse"], "lse")
    same(dec["neg_ll"], ref["neg_ll"], "neg_ll")
    same(dec["nll"].mean(), ref["neg_ll"], "mean of nll")
    same(enc["sumsq"] + dec["sumsq"], ref["sumsq"], "sumsq")
    same(dec["neg_ll"] + ref["anneal"] * enc["kl"] + reg * reg * (enc["sumsq"] + dec["sumsq"]), ref["loss"], "loss")
    for n, got, want in zip(("dWq", "dbq", "dWp", "dbp"), (egr["Wq_t"].T, egr["bq"], dgr["Wp"], dgr["bp"]), ref["grads"]):
        same(got, want, n)
    # eval mode: no mask, no 1 / keep_prob
    ev, _ = vo.run(vo.multvae_encode_fwd, enc_in, training=False)
    want = mh.step((Wq, bq, Wp, bp), g["rowptr"], g["col"], g["users"], None, g["eps"], uc, reg, training=False)
    same(ev["z"], want["z"], "eval z")


def _macrid_weights(g):
    """The reference's initial values for the fixture's seed (tests/test_macridvae_host.py checks them bit for bit)."""
    from chaorec_amd.Model import MacridVAE
    torch.manual_seed(int(g["seed"]))
    m = MacridVAE(g["U"], g["I"], g["edges"], ch.user_item_dict(g["edges"]), g["D"], 0.0, torch.device("cpu"))
    return tuple(np.ascontiguousarray(v.detach().numpy()) for v in m.state_dict().values())


def _dual_weights_and_tables(g):
    from chaorec_amd.Model import DualVAE
    torch.manual_seed(g["seed"])
    m = DualVAE(g["U"], g["I"], g["edges"], dh.user_item_dict(g["edges"]), 64, dh.KL_WEIGHT, dh.SSL_REG, torch.device("cpu"))
    return ([np.ascontiguousarray(v.detach().numpy()) for v in m.state_dict().values()],
            tuple(t.detach().numpy().copy() for t in (m.theta, m.beta, m.mu_theta, m.mu_beta)))


def test_macrid_ops_chain_into_the_step():
    g = ch.load_fixture(GOLDEN, "small")
    w = _macrid_weights(g)
    keep, gumbel, eps = ch.case_draws(g, int(g["draw_seed"]), g["users"])
    upd = 123456
    ref = ch.step(w, g["rowptr"], g["col"], g["users"], keep, gumbel, eps, upd)
    W1, b1, W2, b2, E, Kemb = (t64(x).clone().requires_grad_(True) for x in w)
    D, B = g["D"], len(g["users"])
    x = t64(vo.dense_rows(g["rowptr"], g["col"], g["users"], g["I"]))
    mask = t64(ch.mask_from_flags(keep, g["rowptr"], g["col"], g["users"], g["I"]))
    con = vo.macrid_concept_fwd(E, Kemb, t64(gumbel), ch.TAU)
    a = vo.macrid_encode_fwd(W1.t(), b1, con["cates"], x, mask, 1.0 - ch.DROP, True)["a"]
    assert a.shape == (B, ch.K, ch.HIDDEN)
    h = torch.tanh(a) @ W2.t() + b2
    mu, lv = vo.unit_rows(h[..., :D]), h[..., D:]
    zh = vo.unit_rows(mu + t64(eps).permute(1, 0, 2) * torch.exp(0.5 * lv))
    mix = vo.macrid_mix_fwd(zh, con["items"], con["cates"], x, ch.TAU)
    kl = (-0.5 * (1 + lv - lv.exp()).sum(2).mean(0)).sum()
    loss = mix["ce"] + ref["anneal"] * kl
    grads = torch.autograd.grad(loss, (W1, b1, W2, b2, E, Kemb))
    for k, got in (("loss", loss), ("ce", mix["ce"]), ("kl", kl), ("lse", mix["lse"]), ("z", zh), ("cates", con["cates"])):
        same(got.detach().numpy(), ref[k], k)
    for n, got, want in zip(ch.NAMES, grads, ref["grads"]):
        same(got.numpy(), want, f"grad {n}")


def _dual_side(p, user, x, table, eps):
    s, t = ("user", "item") if user else ("item", "user")
    A, K, H = dh.A, dh.K, dh.H
    pref = p["item_topics"] if user else p["user_preferences"]
    B, N = x.shape
    w = torch.softmax((table * pref).sum(-1), dim=1)
    pre = vo.dualvae_encode_fwd(p[f"{s}_encoder.fc0.weight"].t(), p[f"{s}_encoder.fc0.bias"], w, x)["pre"]
    h = torch.tanh(pre).reshape(B * A, H)
    mu = vo.dualvae_linear_fwd(h, p[f"{s}_mu.weight"], p[f"{s}_mu.bias"])["y"]
    std_pre = vo.dualvae_linear_fwd(h, p[f"{s}_std.weight"], p[f"{s}_std.bias"])["y"]
    z = mu + eps.permute(1, 0, 2).reshape(B * A, K) * torch.sigmoid(std_pre)
    zh = torch.tanh(vo.dualvae_linear_fwd(z, p[f"{s}_decoder.fc_out0.weight"], p[f"{s}_decoder.fc_out0.bias"])["y"])
    th = torch.tanh(vo.dualvae_linear_fwd(table.reshape(N * A, K), p[f"{t}_decoder.fc_out0.weight"],
                                          p[f"{t}_decoder.fc_out0.bias"])["y"])
    z3 = z.reshape(B, A, K)
    dense = vo.dualvae_dense_fwd(z3, zh.reshape(B, A, H), th.reshape(N, A, H), w, table, x)
    cl = vo.dualvae_contrast(z3, dense["nei"])
    out = vo.dualvae_loss_fwd(mu, std_pre, dense["xlog"], dense["sum_p"], cl, dh.KL_WEIGHT, dh.SSL_REG)["out"]
    return dict(z=z3, mu=mu.reshape(B, A, K), nei=dense["nei"], cl=cl, loss=out[0], kl=out[1], ll=out[2])


def test_dualvae_ops_chain_into_the_step():
    g = dh.load_fixture(GOLDEN, "small")
    U, I = g["U"], g["I"]
    weights, tables = _dual_weights_and_tables(g)
    ei, eu = dh.replay_draws(g["draw_seed"], len(g["users"]))
    X = dh.dense_matrix(g["edges"], U, I)
    users, pos = np.asarray(g["users"], dtype=np.int64), np.asarray(g["pos"], dtype=np.int64) - U
    ref = dh.step(weights, tables, X, users, pos, ei, eu)
    p = {n: t64(w).clone().requires_grad_(True) for n, w in zip(dh.NAMES, weights)}
    theta, beta = (np.array(t, dtype=np.float64) for t in tables[:2])
    it = _dual_side(p, False, t64(X.T[pos]), t64(theta), t64(ei))
    dh.write_back(beta, pos, it["z"].detach().numpy())
    us = _dual_side(p, True, t64(X[users]), t64(beta), t64(eu))
    loss = it["loss"] + us["loss"]
    grads = torch.autograd.grad(loss, [p[n] for n in dh.NAMES])
    same(loss.item(), ref["loss"], "loss")
    for name, s in (("item", it), ("user", us)):
        for k in ("kl", "ll", "cl", "loss", "z", "mu", "nei"):
            same(s[k].detach().numpy(), ref[name][k], f"{name} {k}")
    for n, got, want in zip(dh.NAMES, grads, ref["grads"]):
        same(got.numpy(), want, f"grad {n}")


def test_macrid_scores_equal_the_model_restatements():
    """The ranking op fed the model restatement's own eval-mode zh, items, cates gives macridvae_host.eval_scores."""
    g = ch.load_fixture(GOLDEN, "small")
    w = _macrid_weights(g)
    W1, b1, W2, b2, E, Kemb = (t64(x) for x in w)
    users = np.arange(g["U"])
    x = t64(vo.dense_rows(g["rowptr"], g["col"], users, g["I"]))
    xs = x / torch.clamp(x.sum(1).sqrt(), min=1e-12)[:, None]
    items, cates = ch.concept_weights(E, Kemb)
    zh, _ = ch.latents(W1, b1, W2, b2, cates, xs, None)
    got = vo.macrid_scores(zh, items, cates, ch.TAU)
    assert got.dtype == torch.float64 and got.shape == (g["U"], g["I"])
    same(got.numpy(), ch.eval_scores(w, g["rowptr"], g["col"], users).numpy(), "macrid scores")
    assert vo.macrid_scores(zh.float(), items.float(), cates.float(), ch.TAU).dtype == torch.float32


def test_dualvae_scores_equal_the_model_restatements():
    """Likewise dualvae_host.scores: z = mu_theta, table = mu_beta, the decoders' tanh rows, the RAW aspect weight."""
    g = dh.load_fixture(GOLDEN, "small")
    weights, _ = _dual_weights_and_tables(g)
    p = {n: t64(w) for n, w in zip(dh.NAMES, weights)}
    gen = torch.Generator().manual_seed(77)
    mt = torch.randn(g["U"], dh.A, dh.K, generator=gen, dtype=torch.float64)
    mb = torch.randn(g["I"], dh.A, dh.K, generator=gen, dtype=torch.float64)
    zh = torch.tanh(mt @ p["user_decoder.fc_out0.weight"].t() + p["user_decoder.fc_out0.bias"])
    th = torch.tanh(mb @ p["item_decoder.fc_out0.weight"].t() + p["item_decoder.fc_out0.bias"])
    w = (mb * p["item_topics"]).sum(-1)
    got = vo.dualvae_scores(mt, zh, mb, th, w)
    assert got.dtype == torch.float64 and got.shape == (g["U"], g["I"])
    same(got.numpy(), dh.scores(weights, mt.numpy(), mb.numpy()), "dualvae scores")
    users = np.array([5, 0, g["U"] - 1])
    same(vo.dualvae_scores(mt[users], zh[users], mb, th, w).numpy(), dh.scores(weights, mt.numpy(), mb.numpy(), users),
         "dualvae scores of three users")


def test_masked_sets_the_history_of_user_begin_plus_row():
    rowptr = np.array([0, 2, 2, 6, 7], dtype=np.int64)
    col = np.array([0, 4, -1, 1, 3, 5, 2], dtype=np.int64)             # user 2 holds the stray columns -1 and I = 5
    sc = np.arange(10, dtype=np.float32).reshape(2, 5) + 1
    got = vo.masked(sc, rowptr, col, 2, 1e-6)
    want = sc.copy()
    want[0, [1, 3]], want[1, 2] = 1e-6, 1e-6
    assert got.dtype == np.float32 and np.array_equal(got, want) and sc[0, 1] == 2           # a copy
    want = sc.copy()
    want[0, [0, 4]] = 7.0                                               # user 0's row, user 1 holds nothing
    assert np.array_equal(vo.masked(sc, rowptr, col, 0, 7.0), want)


def test_counter_rng_restatement():
    # splitmix64's published first outputs from state 0: mix64(0) is the finaliser of 0 + golden gamma
    assert int(vo.mix64(0)) == 0xE220A8397B1DCDAF
    key = vo.vae_key(1234, 7, vo.MULTVAE_SALT_KEEP)
    a, b = np.meshgrid(np.arange(300), np.arange(400), indexing="ij")
    for bits in (23, 24):
        u = vo.vae_uniform(key, a, b, bits)
        assert u.dtype == np.float32 and u.shape == (300, 400)
        # strictly inside (0, 1) -- for BITS = 24 over THESE 120 000 draws only: its top value, 2^24 - 1/2, is no fp32
        # number and rounds to 2^24, so one draw in 2^24 is exactly 1.0 (asserted below); BITS = 23 holds for every draw
        assert float(u.min()) > 0.0 and float(u.max()) < 1.0
        assert np.array_equal(u, vo.vae_uniform(key, a, b, bits))                  # a draw depends on its counters only
        assert np.array_equal(u[17, 5], vo.vae_uniform(key, 17, 5, bits))
        # BITS random bits + one half: u 2^BITS - 1/2 is a whole number below 2^BITS wherever the sum fits fp32's 24 bits
        # (all of BITS = 23; the lower half of BITS = 24, whose upper half rounds the tie to even -- a keep flag compares
        # against keep_prob <= 1/2 ... 1 and is decided by the top bits either way)
        k = (u.astype(np.float64) * (1 << bits) - 0.5)[u < 0.5 if bits == 24 else u < 2.0]
        assert np.array_equal(k, np.floor(k)) and k.min() >= 0 and k.max() < (1 << bits)
        assert abs(float(u.mean()) - 0.5) < 5 * np.sqrt(1 / 12 / u.size)
    top = lambda bits: (np.float32((1 << bits) - 1) + np.float32(0.5)) * np.float32(1.0 / (1 << bits))   # noqa: E731
    assert top(23) < 1.0 and top(24) == 1.0              # the header's "exact in fp32 for BITS <= 24" holds up to 23 only
    u23, u24 = vo.vae_uniform(key, a, b, 23), vo.vae_uniform(key, a, b, 24)
    assert not np.array_equal(u23, u24)                                            # another stream ...
    low = u24 < 0.5                                                                # ... of the same bits, one fewer
    assert np.array_equal(np.floor(u24[low].astype(np.float64) * (1 << 23)), u23[low].astype(np.float64) * (1 << 23) - 0.5)
    # the counters, the step and the salt all enter
    assert not np.array_equal(u24, vo.vae_uniform(key, b, a, 24))
    assert not np.array_equal(u24, vo.vae_uniform(vo.vae_key(1234, 8, vo.MULTVAE_SALT_KEEP), a, b, 24))
    assert not np.array_equal(u24, vo.vae_uniform(vo.vae_key(1234, 7, vo.MACRID_SALT_KEEP), a, b, 24))
    # a keep flag has no rounding: u < 1/2 iff the top random bit is 0
    with np.errstate(over="ignore"):
        r = vo.mix64(key ^ vo.mix64((a.astype(np.uint64) << np.uint64(32)) ^ b.astype(np.uint64)))
    assert np.array_equal(u24 < np.float32(0.5), (r >> np.uint64(63)) == 0)
    assert np.array_equal(u23 < np.float32(0.5), (r >> np.uint64(63)) == 0)


def test_predicted_mask_follows_the_history_rows():
    g = mh.load_fixture(GOLDEN, "small")
    users = g["users"][:40]
    m = vo.predict_keep(99, 3, vo.MULTVAE_SALT_KEEP, vo.MULTVAE_BITS, 0.5, g["rowptr"], g["col"], users, g["I"])
    x = vo.dense_rows(g["rowptr"], g["col"], users, g["I"]) != 0
    assert m.shape == x.shape and not (m & ~x).any() and 0 < m.sum() < x.sum()
    assert not np.array_equal(m, vo.predict_keep(99, 4, vo.MULTVAE_SALT_KEEP, vo.MULTVAE_BITS, 0.5, g["rowptr"], g["col"], users, g["I"]))


def test_row_measure():
    ref = np.array([[1.0, 2.0], [2.0 ** -20, 0.0], [0.125, 0.25]])
    x = ref + np.array([[0.0, 2.0 ** -9], [2.0 ** -20, 0.0], [2.0 ** -9, 0.0]])
    # row 0: 2^-9 / 2; row 1 is below the floor 1e-3 x 2 and normed by it: 2^-20 / 2e-3; row 2: 2^-9 / 0.25
    assert vo.row_dev(x, ref) == 2.0 ** -7
    assert vo.row_dev(x[:2], ref[:2]) == 2.0 ** -10
    assert vo.row_dev(x[1:2], ref[1:2]) == 1.0                                     # alone, the small row is its own scale
    assert vo.row_dev(np.array([1.0, 0.5]), np.array([1.0, 0.25])) == 1.0          # a vector: every element a row
    assert vo.row_dev(3.0, 2.0) == 0.5
    assert vo.bound_of(ref, ref) == 2.0 ** -22 and vo.bound_of(x, ref) == 2.0 ** -5
    assert np.isnan(vo.row_dev(np.array([np.nan, 1.0]), np.array([1.0, 1.0])))
