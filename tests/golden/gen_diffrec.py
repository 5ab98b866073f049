#!/usr/bin/env python
"""Generate tests/golden/diffrec_small.npz by running the REFERENCE's own Model/DiffRec.py on the CPU.

Nothing of the reference is copied: this script imports the class from the reference checkout at run time (the directory
CHAOREC_REFERENCE names) and stores inputs + outputs as .npz data.

    CHAOREC_REFERENCE=/path/to/reference python tests/golden/gen_diffrec.py

The case (tests/diffrec_host.py): U 12, I 48, steps 5, dims "[68]"; user 11 without history, items 44 .. 47 without users, item 0
held by every user with a history; the weights spread (diffrec_host.spread) so that the tanh's are not linear.

Stored: the edges; the state_dict's names and the six weights (w_<name>); the diffusion tables; given ts (0 and steps - 1 twice
each), noise and keep flags; training_losses' reloss and loss with nn.Dropout replaced by the given flags, in fp32 (the
reference's) and from the float64 restatement, with the reference's deviations `own_*` (loss, reloss, every gradient);
Lt_history / Lt_count after the crafted sequence of diffrec_host.lt_sequence() through the reference's loop; pt_all from that
history (the argument the reference hands torch.multinomial); p_sample's rows in fp32 and float64 with `own_sample`; the
reference loop's top-k list.
Asserted here: the hidden units saturate somewhere and not everywhere; the collapsed restatement equals the literal one in
float64; the fp32 and float64 lists pass tie_aware_rank_equal at atol = 4 * max(own_sample, ULP) * largest score.
"""
import os
import sys
import warnings

import numpy as np
import torch

REF = os.environ.get("CHAOREC_REFERENCE")
if not REF:
    raise SystemExit("set CHAOREC_REFERENCE to the reference checkout")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

import diffrec_host as dh  # noqa: E402
from conftest import tie_aware_rank_equal  # noqa: E402


class GivenDrop(torch.nn.Module):
    """nn.Dropout(0.5) with given flags."""

    def __init__(self, keep):
        super().__init__()
        self.keep = keep

    def forward(self, x):
        return x * (self.keep.to(x.dtype) * 2.0)


def generate():
    import Model.DiffRec as refmod
    edges = dh.small_case()
    U, I = dh.U, dh.I
    uid = dh.user_item_dict(edges)
    assert U - 1 not in uid and not (edges[:, 1] - U >= I - 4).any() and (np.bincount(edges[:, 1] - U)[0] == U - 1)
    g = dict(U=U, I=I, edges=edges.astype(np.int32))

    torch.manual_seed(dh.SEED)
    model = refmod.DiffRec(U, I, uid, dh.NOISE_SCALE, dh.NOISE_MIN, dh.NOISE_MAX, dh.STEPS, dh.DIMS, 0.001, torch.device("cpu"))
    sd = model.state_dict()
    assert tuple(sd) == dh.NAMES, tuple(sd)
    g["names"] = np.array(list(sd))
    g["w_sum_seeded"] = np.array([float(sd[n].double().sum()) for n in dh.NAMES])      # the constructor's draws, before the spread
    torch.manual_seed(dh.SEED + 1)
    dh.spread(model)
    sd = model.state_dict()
    for n in dh.NAMES:
        g["w_" + n] = sd[n].numpy().copy()
    w64, w32 = ({n: sd[n].to(dt) for n in dh.NAMES} for dt in (torch.float64, torch.float32))

    s = dh.schedule64()
    for k, attr in (("betas", "betas"), ("ac", "alphas_cumprod"), ("coef1", "posterior_mean_coef1"), ("coef2", "posterior_mean_coef2")):
        t = getattr(model, attr)
        assert t.dtype == torch.float64 and np.allclose(t.numpy(), s[k], rtol=1e-13, atol=0), k
        g["tab_" + k] = t.numpy().copy()
    assert float(model.posterior_mean_coef2[0]) == 0.0 and float(model.posterior_mean_coef1.float()[0]) == 1.0

    x0 = torch.from_numpy(dh.dense_rows(edges))
    ts = torch.from_numpy(dh.TS)
    rs = np.random.RandomState(3)
    noise = torch.from_numpy(rs.standard_normal((U, I)).astype(np.float32))
    keep = torch.from_numpy(rs.random_sample((U, I)) < 0.5)
    g["ts"], g["noise"], g["keep_bits"] = dh.TS, noise.numpy(), np.packbits(keep.numpy().reshape(-1))

    # ---- training_losses with the given draws: the reference's own lines, its dropout module replaced
    model.train()
    model.dnn.drop = GivenDrop(keep)
    model.sample_timesteps = lambda batch_size, device, method='uniform', uniform_prob=0.001: (ts, torch.ones_like(ts).float())
    orig_randn = torch.randn_like
    torch.randn_like = lambda x, **kw: noise
    seen = []
    orig_update = model.update_Lt_history
    model.update_Lt_history = lambda t, r: seen.append(r.detach().clone())
    try:
        model.zero_grad()
        loss = model.training_losses(x0)
        loss.backward()
    finally:
        torch.randn_like = orig_randn
    model.update_Lt_history = orig_update
    del model.sample_timesteps
    reloss = seen[0]
    assert reloss.dtype == torch.float64 and loss.dtype == torch.float64
    r64 = dh.training_step(w64, x0.numpy(), dh.TS, noise.numpy(), keep.numpy())
    r32 = dh.training_step(w32, x0.numpy(), dh.TS, noise.numpy(), keep.numpy())
    assert dh.rel_dev(r32["reloss"], reloss.numpy()) < 1e-5, "the restatement in fp32 is not the reference's training_losses"
    g["loss32"], g["loss64"], g["own_loss"] = float(loss), r64["loss"], dh.rel_dev(float(loss), r64["loss"])
    g["reloss32"], g["reloss64"], g["own_reloss"] = reloss.numpy(), r64["reloss"], dh.rel_dev(reloss.numpy(), r64["reloss"])
    params = dict(model.named_parameters())
    for n in dh.NAMES:
        g["grad64_" + n] = r64["grads"][n]
        g["own_grad_" + n] = dh.rel_dev(params[n].grad.numpy(), r64["grads"][n])
    with torch.no_grad():
        hid = dh.hidden(w64, dh.noised_input(x0.numpy(), dh.TS, noise.numpy(), keep.numpy(), torch.float64), dh.TS).abs()
    print(f"training_losses: loss {float(loss):.6e} own {g['own_loss']:.3e}, own reloss {g['own_reloss']:.3e}, "
          f"|h| > 0.9: {float((hid > 0.9).double().mean()):.3f}, |h| < 0.3: {float((hid < 0.3).double().mean()):.3f}")
    assert 0.05 < float((hid > 0.9).double().mean()) < 0.95

    model.eval()
    with torch.no_grad():
        # ---- the loss history through the reference's loop, and the importance distribution it leads to
        for tb, lb in dh.lt_sequence():
            model.update_Lt_history(torch.from_numpy(tb), torch.from_numpy(lb))
        g["Lt_history"], g["Lt_count"] = model.Lt_history.numpy().copy(), model.Lt_count.numpy().copy()
        assert (model.Lt_count == 10).all()
        got, orig = [], torch.multinomial
        torch.multinomial = lambda p, **kw: (got.append(p.clone()), orig(p, **kw))[1]
        try:
            t_imp, pt = model.sample_timesteps(64, torch.device("cpu"), 'importance')
        finally:
            torch.multinomial = orig
        g["pt_all"] = got[0].numpy()
        assert abs(g["pt_all"].sum() - 1.0) < 1e-12 and np.allclose(pt.numpy(), g["pt_all"][t_imp.numpy()] * dh.STEPS)

        # ---- p_sample and the ranking, as train_and_evaluate.py:578-613
        model.dnn.drop = torch.nn.Dropout(0.5)
        model.eval()
        ps32 = model.p_sample(x0)
        ps64 = dh.p_sample(w64, x0.numpy())
        col64, beta = dh.p_sample_collapsed(w64, x0.numpy())
        assert beta == 0.0 and dh.rel_dev(col64.numpy(), ps64.numpy()) < 1e-12, "the collapsed chain is not the literal one"
        own = dh.rel_dev(ps32.numpy(), ps64.numpy())
        pred = ps32.clone()
        mask = torch.zeros_like(pred, dtype=torch.bool)
        for u in range(U):
            items = uid.get(u, [])
            if len(items) > 0:
                mask[u, torch.tensor(items, dtype=torch.long) - U] = True
        pred.masked_fill_(mask, -np.inf)
        rank = (torch.topk(pred, dh.TOPK, dim=1)[1] + U).numpy()
        scale = float(np.abs(ps64.numpy()).max())
        i32, v32 = rank - U, np.take_along_axis(dh.masked(ps32.numpy(), edges), rank - U, 1)
        i64, v64 = dh.top_lists(dh.masked(ps64.numpy(), edges))
        ok, why = tie_aware_rank_equal(i32, v32, i64, v64, atol=4 * max(own, dh.ULP) * scale)
        assert ok, f"the reference's own list against the float64 list: {why}"
        g["sample32"], g["sample64"], g["own_sample"], g["rank"] = ps32.numpy(), ps64.numpy(), own, rank.astype(np.int16)
        print(f"p_sample: own {own:.3e}, largest |x| {scale:.4f}")
    path = os.path.join(HERE, dh.FIXTURE)
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate()
