"""GraphAug on the CPU: the float64 restatement (tests/graphaug_host.py) against the golden the reference class wrote
(tests/golden/gen_graphaug.py), the state_dict keys, and the condition under which the sampler tests compare zero / non-zero
decisions exactly -- checked on the reference's values and on the restatement's fp32 lines, never on a kernel."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accept  # noqa: E402
import graphaug_host as gh  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def within(x, ref, dev, what):
    """x is the float64 restatement, `ref` the reference's stored fp32 tensor: the stored tensor is held to the restatement."""
    accept.within(what, ref, x, dev, accept.ULP24)


@functools.lru_cache(maxsize=None)
def case():
    c = gh.small_case()
    return c, gh.init_weights(c), gh.load_fixture(GOLDEN), gh.draws(c, 1)[0]


@functools.lru_cache(maxsize=None)
def host_step():
    c, w, _, dr = case()
    return gh.step_with_grads(w, c, dr)


def test_small_case_reaches_every_path():
    c = case()[0]
    G = gh.graph_arrays(c)
    lens = np.bincount(G["row"], minlength=G["N"])
    assert lens.max() > 64                                     # a row for the whole wave
    assert (lens[:c["U"]] == 0).any() and (lens[c["U"]:] == 0).any()      # a user and an item without interaction
    assert G["N"] % 32 and G["E"] % 32 and G["E"] % 8
    assert np.array_equal(G["tentry"][G["tentry"]], np.arange(G["E"]))


def test_state_dict_keys_and_weights():
    c, w, g, dr = case()
    assert tuple(g["names"].tolist()) == gh.NAMES
    assert not any("bottom_layers" in n for n in gh.NAMES)     # untrained plain tensors in the reference: not in state_dict()
    assert len(gh.PARAMS) == 14 and set(gh.PARAMS) <= set(gh.NAMES)
    names = gh.PARAMS + gh.BOTTOM
    assert np.array_equal(g["w_sum"], np.array([float(w[n].astype(np.float64).sum()) for n in names]))
    assert np.array_equal(g["w_probe"], np.stack([np.resize(w[n].reshape(-1)[:g["w_probe"].shape[1]], g["w_probe"].shape[1]) for n in names]))
    every = [u for v in dr["views"] for u in (v["u1"], v["u2"])] + [m for v in dr["views"] for m in v["masks"]] + list(dr["rdm"])
    assert np.array_equal(g["draw_sums"], np.array([float(np.asarray(t, dtype=np.float64).sum()) for t in every]))


def test_restatement_matches_golden_loss_and_gradients():
    g = case()[2]
    host, grads = host_step()
    for name in ("loss",) + gh.PARTS:
        within(host[name], g[f"ref_{name}"], g[f"dev_{name}"], name)
        assert g[f"dev_{name}"] < 1e-5
    for k, n in enumerate(gh.WITH_GRAD):
        within(grads[n], g[f"ref_grad_{k}"], g["dev_grads"][k], f"grad {n}")
        assert g["dev_grads"][k] < 1e-5


def test_restatement_matches_golden_view():
    g = case()[2]
    host = host_step()[0]
    within(host["logits"][0].numpy(), g["logits"], g["dev_logits"], "logits")
    within(host["node_emb"][0].detach().numpy()[:g["node_emb"].shape[0]], g["node_emb"], g["dev_node_emb"], "node_emb")
    val64 = host["val"][0].numpy()
    assert np.array_equal(val64 != 0, g["nonzero"]) and g["flips"] == 0
    within(val64, g["val"], g["dev_val"], "values")
    att = host["att"][0].numpy()
    assert (att == 0.01).any() and (att == 0.99).any() and g["nonzero"].any() and not g["nonzero"].all()


def test_flip_condition_on_the_reference():
    """An entry whose float64 s lies within delta = 4 x the fp32 lines' deviation of s from 0.2 may fall on either side; at
    most 0.1 % of E may be such entries, and on every other entry the reference's decision is the float64 one."""
    c, _, g, _ = case()
    s64 = host_step()[0]["s"][0].numpy()
    delta = 4 * float(g["abs_dev_s"])
    band = np.abs(s64 - 0.2) < delta
    print("golden: delta", delta, "entries in the band", int(band.sum()), "of", g["E"])
    assert band.sum() <= 0.001 * g["E"]
    assert np.array_equal((s64 > 0.2)[~band], g["nonzero"][~band])
    # the sampler tests' own case, through the restatement's fp32 lines
    W, z, u1, u2 = gh.sampler_case(c)
    h64 = gh.sampler_host(W, gh.Graph(c), z, u1, u2)
    h32 = gh.sampler_host(W, gh.Graph(c, torch.float32), z, u1, u2, torch.float32)
    delta, band = gh.flip_band(h32["s"], h64["s"])
    print("sampler case: delta", delta, "entries in the band", int(band.sum()), "logit span", h64["logits"].min(), h64["logits"].max())
    assert band.sum() <= 0.001 * len(band)
    assert np.array_equal((h32["val"] != 0)[~band], (h64["val"] != 0)[~band])
    assert (h64["att"] == 0.01).any() and (h64["att"] == 0.99).any() and (h64["val"] != 0).any() and (h64["val"] == 0).any()
    assert h64["logits"].min() < -4.6 and h64["logits"].max() > 4.6      # logit(0.99): the logit alone reaches both clamps


def test_trajectory_and_rank_list():
    c, w, g, _ = case()
    final, losses = gh.trajectory(w, c, gh.draws(c, gh.N_STEPS, seed_offset=2))
    within(losses, g["traj_losses"], g["dev_traj_losses"], "trajectory losses")
    for k, n in enumerate(gh.WITH_GRAD):
        within(final[n] - w[n], g[f"traj_{k}"] - w[n], g["dev_traj"][k], f"update of {n}")
    assert all(np.array_equal(final[n], w[n]) for n in gh.MLP)
    assert np.array_equal(gh.ranklist(w, c), g["ranklist"].astype(np.int64))


def test_lse_cases_are_what_they_claim():
    for B, M in ((33, 97), (1, 5), (64, 2049)):
        A, T, _ = gh.lse_case(B, M)
        lse, _, _ = gh.lse_host(A, T, 20.0)
        assert np.isfinite(lse).all() and np.abs(A[0] @ T.T).max() > 1 - 1e-6      # a term e^20 is present
