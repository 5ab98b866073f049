#!/usr/bin/env python
"""Generate tests/golden/cfdiff_small.npz by running the REFERENCE's own Model/CF_Diff.py and dataload.py on the CPU.

Nothing of the reference is copied: this script imports both from the reference checkout at run time (the directory
CHAOREC_REFERENCE names) and stores inputs + outputs as .npz data.

    CHAOREC_REFERENCE=/path/to/reference python tests/golden/gen_cfdiff.py

The case (tests/cfdiff_host.py): U 12, I 48, steps 10; user 11 without history, items 44 .. 47 without users, item 0 held by every
user with a history.  dim_inters is the reference's hard-coded 1024, so L = 1034.

Stored: the edges; DiffusionData_sec_hop's rows; the CAM_AE weights that its forward reads (w_<name>); given ts (0 and steps - 1
included) and noise; q_sample's x_t; the eval-mode CAM_AE output in fp32 (the reference's) and from the float64 restatement
(cfdiff_host.cam_ae) with the first's deviation `own_out`; reweight_loss of that output; Lt_history / Lt_count after the crafted
sequence of cfdiff_host.lt_sequence() through the reference's loop; pt_all from that history (the argument the reference hands
torch.multinomial); p_sample's rows in fp32 and float64 with `own_sample`; the reference loop's top-k list.
Asserted here: the restated sec-hop rows equal the reference's; the fp32 and float64 lists pass tie_aware_rank_equal at
atol = 4 * max(own_sample, ULP) * largest score.
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

import cfdiff_host as ch  # noqa: E402
from conftest import tie_aware_rank_equal  # noqa: E402


def generate():
    import dataload as refdata
    import Model.CF_Diff as refmod
    edges = ch.small_case()
    U, I = ch.U, ch.I
    uid = ch.user_item_dict(edges)
    assert U - 1 not in uid and not (edges[:, 1] - U >= I - ch.EMPTY_ITEMS).any() and (np.bincount(edges[:, 1] - U)[0] == U - 1)
    g = dict(U=U, I=I, edges=edges.astype(np.int32))

    sec = refdata.DiffusionData_sec_hop(U, I, edges).data
    assert sec.dtype == torch.float32 and np.array_equal(sec.numpy(), ch.sec_hop_rows(edges)), "the sec-hop rows are not cnt / U on the history"
    g["sec_hop"] = sec.numpy()

    torch.manual_seed(20241012)
    model = refmod.CF_Diff(U, I, uid, ch.NOISE_SCALE, ch.NOISE_MIN, ch.NOISE_MAX, ch.STEPS, 0.001, torch.device("cpu"))
    with torch.no_grad():          # the default initialisation leaves the attention nearly uniform: spread the in-projections
        for mha in model.CAM_AE.self_attentions:
            mha.in_proj_weight.mul_(4.0)
            mha.in_proj_bias.normal_(0.0, 0.3)
        model.CAM_AE.first_hop_embedding.weight.mul_(2.0)
        model.CAM_AE.second_hop_embedding.weight.mul_(2.0)
    sd = model.CAM_AE.state_dict()
    for n in ch.WEIGHTS:
        g["w_" + n] = sd[n].numpy().copy()
    w64 = {n: sd[n].double() for n in ch.WEIGHTS}

    x0 = torch.from_numpy(ch.dense_rows(edges))
    ts = torch.from_numpy(ch.TS)
    noise = torch.from_numpy(np.random.RandomState(3).standard_normal((U, I)).astype(np.float32))
    x_t = model.q_sample(x0, ts, noise)
    s = ch.schedule64()
    assert np.allclose(model.alphas_cumprod.numpy(), s["ac"], rtol=1e-14, atol=0) and np.allclose(model.posterior_mean_coef1.numpy(), s["coef1"], rtol=1e-13, atol=0)
    g["ts"], g["noise"], g["x_t"] = ch.TS, noise.numpy(), x_t.numpy()

    model.eval()
    with torch.no_grad():
        out32 = model.CAM_AE(x_t, sec, ts)
        out64 = ch.cam_ae(w64, x_t, sec, ts)
        g["out32"], g["out64"], g["own_out"] = out32.numpy(), out64.numpy(), ch.rel_dev(out32.numpy(), out64.numpy())
        mse = model.mean_flat((x0 - out32) ** 2)
        reloss = model.reweight_loss(x0, x_t, mse, ts, x0, out32, torch.device("cpu"))
        g["reloss"] = reloss.numpy()
        assert reloss.dtype == torch.float64
        print(f"CAM_AE eval: own {g['own_out']:.3e}, largest |out| {np.abs(out64.numpy()).max():.4f}, reloss {reloss.numpy().round(4)}")

        # ---- the loss history through the reference's loop, and the importance distribution it leads to
        for tb, lb in ch.lt_sequence():
            model.update_Lt_history(torch.from_numpy(tb), torch.from_numpy(lb))
        g["Lt_history"], g["Lt_count"] = model.Lt_history.numpy().copy(), model.Lt_count.numpy().copy()
        assert (model.Lt_count == 10).all()
        seen, orig = [], torch.multinomial
        torch.multinomial = lambda p, **kw: (seen.append(p.clone()), orig(p, **kw))[1]
        try:
            t_imp, pt = model.sample_timesteps(64, torch.device("cpu"), 'importance')
        finally:
            torch.multinomial = orig
        g["pt_all"] = seen[0].numpy()
        assert abs(g["pt_all"].sum() - 1.0) < 1e-12 and np.allclose(pt.numpy(), g["pt_all"][t_imp.numpy()] * ch.STEPS)

        # ---- p_sample and the ranking, as train_and_evaluate.py:614-650
        ps32 = model.p_sample(x0, sec)
        ps64 = ch.p_sample(w64, x0, sec)
        own = ch.rel_dev(ps32.numpy(), ps64.numpy())
        pred = ps32.clone()
        mask = torch.zeros_like(pred, dtype=torch.bool)
        for u in range(U):
            items = uid.get(u, [])
            if len(items) > 0:
                mask[u, torch.tensor(items, dtype=torch.long) - U] = True
        pred.masked_fill_(mask, -np.inf)
        rank = (torch.topk(pred, ch.TOPK, dim=1)[1] + U).numpy()
        scale = float(np.abs(ps64.numpy()).max())
        i32, v32 = rank - U, np.take_along_axis(ch.masked(ps32.numpy(), edges), rank - U, 1)
        i64, v64 = ch.top_lists(ch.masked(ps64.numpy(), edges))
        ok, why = tie_aware_rank_equal(i32, v32, i64, v64, atol=4 * max(own, ch.ULP) * scale)
        assert ok, f"the reference's own list against the float64 list: {why}"
        g["sample32"], g["sample64"], g["own_sample"], g["rank"] = ps32.numpy(), ps64.numpy(), own, rank.astype(np.int16)
        print(f"p_sample: own {own:.3e}, largest |x| {scale:.4f}")
    path = os.path.join(HERE, ch.FIXTURE)
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    generate()
