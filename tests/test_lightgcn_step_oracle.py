"""oracle/lightgcn_step_fp64.py: the fp64 training step with its own error bound, checked on the CPU.

* its value pass is the autograd gradient of oracle/torch_ref.py:TorchRefLightGCN in float64;
* an independent fp32 step (TorchRefLightGCN in float32 + torch.optim.Adam) stays inside the bound;
* that fp32 step with one of eight plausible mistakes leaves it;
* the bound is tight enough to mean something (thresholds below, measured on sports).
tests/test_gpu_lightgcn_step_oracle.py holds the kernels of the fused step to the same bound."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_interactions
from oracle.lightgcn_step_fp64 import excess, lightgcn_step_fp64, torch_ref_csr
from oracle.torch_ref import TorchRefLightGCN

LR, REG = 1e-3, 1e-3

MUTATIONS = ["layer_weight_1_over_L", "bpr_eps_dropped", "l2_on_ego_rows", "bias_correction_at_t_minus_1",
             "user_repeat_dropped_from_gradient", "wG_missing_from_last_backward_layer", "edge_of_densest_row_dropped",
             "zero_gradient_rows_not_updated"]


class Fp32Step(TorchRefLightGCN):
    """TorchRefLightGCN + torch.optim.Adam, with one optional mistake (`mutation`, one of MUTATIONS)."""

    def __init__(self, U, I, edges, D, L):
        super().__init__(U, I, edges, None, D, REG, L)
        self.mutation = None
        self.drop_sample = None
        N = U + I
        row, col = self.edge_index
        hub = int(torch.bincount(col, minlength=N).argmax())
        self.hub, self.hub_entry = hub, int((col == hub).nonzero()[0])

    def csr(self):
        """the operator conv applies, with conv's own fp32 norms (the reference takes these values as exact)"""
        return torch_ref_csr(self.edge_index, self.num_user + self.num_item, torch.float32)

    def conv(self, x):
        if self.mutation != "edge_of_densest_row_dropped":
            return super().conv(x)
        row, col = self.edge_index.long()
        deg = torch.zeros(x.size(0), dtype=x.dtype).scatter_add_(0, row, torch.ones(row.numel(), dtype=x.dtype))
        dis = deg.pow(-0.5)
        norm = dis[row] * dis[col]
        norm[self.hub_entry] = 0.0
        msg = norm.view(-1, 1) * x.index_select(0, row)
        return torch.zeros_like(x).scatter_add_(0, col.view(-1, 1).expand_as(msg), msg)

    def forward(self):
        x = torch.cat((self.user_embedding.weight, self.item_embedding.weight), dim=0)
        embs = [x]
        for _ in range(self.n_layers):
            embs.append(self.conv(embs[-1]))
        w = 1.0 / (self.n_layers if self.mutation == "layer_weight_1_over_L" else len(embs))
        final = torch.zeros_like(embs[0])
        for i, e in enumerate(embs):
            if i == 0 and self.mutation == "wG_missing_from_last_backward_layer":
                e = e.detach()              # same forward; the backward's last layer lacks its w G term
            final = final + w * e
        self.result = final
        self.ego = x
        return final

    def loss(self, users, pos_items, neg_items):
        pos_items, neg_items = pos_items - self.num_user, neg_items - self.num_user
        emb = self.forward()
        u, p, n = emb[users], emb[self.num_user + pos_items], emb[self.num_user + neg_items]
        if self.mutation == "user_repeat_dropped_from_gradient":
            keep = torch.ones(len(users), 1, dtype=torch.bool)
            keep[self.drop_sample] = False
            u = torch.where(keep, u, u.detach())
        eps = 0.0 if self.mutation == "bpr_eps_dropped" else 1e-5
        d = torch.sum(u * p, dim=1) - torch.sum(u * n, dim=1)
        bpr = -torch.mean(torch.log(torch.sigmoid(d) + eps))
        if self.mutation == "l2_on_ego_rows":
            x = self.ego
            u, p, n = x[users], x[self.num_user + pos_items], x[self.num_user + neg_items]
        return bpr + self.reg_weight * (torch.mean(u ** 2) + torch.mean(p ** 2) + torch.mean(n ** 2))

    def table(self):
        return torch.cat((self.user_embedding.weight, self.item_embedding.weight), 0).detach().clone()

    def moments(self, opt):
        out = []
        for key in ("exp_avg", "exp_avg_sq"):
            parts = []
            for p in (self.user_embedding.weight, self.item_embedding.weight):
                st = opt.state.get(p, {})
                parts.append(st[key].clone() if key in st else torch.zeros_like(p.detach()))
            out.append(torch.cat(parts, 0))
        return out

    def step(self, opt, users, pos, neg):
        opt.zero_grad()
        loss = self.loss(users, pos, neg)
        loss.backward()
        params = (self.user_embedding.weight, self.item_embedding.weight)
        if self.mutation == "bias_correction_at_t_minus_1":
            for p in params:
                opt.state[p]["step"] -= 1
        saved = None
        if self.mutation == "zero_gradient_rows_not_updated":
            saved = [(p, (p.grad == 0).all(1), p.detach().clone(), opt.state[p]["exp_avg"].clone(),
                      opt.state[p]["exp_avg_sq"].clone()) for p in params]
        opt.step()
        if saved:
            with torch.no_grad():
                for p, z, w0, m0, v0 in saved:
                    p[z] = w0[z]
                    opt.state[p]["exp_avg"][z] = m0[z]
                    opt.state[p]["exp_avg_sq"][z] = v0[z]
        return loss.detach()


def _batch(rng, edges, U, I, B):
    sel = rng.integers(0, len(edges), B)
    return (torch.from_numpy(edges[sel, 0].astype(np.int64)), torch.from_numpy(edges[sel, 1].astype(np.int64)),
            torch.from_numpy(rng.integers(U, U + I, B)))


def _reference(model, opt, users, pos, neg):
    """the fp64 reference of the NEXT step of (model, opt) on this batch"""
    m, v = model.moments(opt)
    st = opt.state.get(model.user_embedding.weight, {})
    t = int(st["step"]) + 1 if "step" in st else 1
    rowptr, col, val = model.csr()
    return lightgcn_step_fp64(rowptr, col, val, model.table(), users, pos - model.num_user, neg - model.num_user,
                              model.num_user, model.reg_weight, model.n_layers, m, v, t, LR)


def _ratios(model, opt, loss, ref):
    m, v = model.moments(opt)
    return {"result": excess(model.result, ref["result"]), "loss": excess(loss, ref["loss"]),
            "m": excess(m, ref["m"]), "v": excess(v, ref["v"]), "W": excess(model.table(), ref["W"])}


# ---- the value pass is autograd's ---------------------------------------------------------------------------------------

def _tiny_with_isolated_rows():
    """6 users, 8 items; user 5 and items 6, 7 (global 12, 13) have no edge"""
    U, I = 6, 8
    edges = np.array([[0, 6], [0, 7], [0, 9], [1, 6], [1, 8], [2, 10], [2, 11], [3, 6], [3, 9], [3, 10], [4, 11], [4, 8]])
    users = torch.tensor([0, 5, 3, 3, 1, 5, 2])
    pos = torch.tensor([6, 7, 9, 10, 8, 12, 11])
    neg = torch.tensor([12, 13, 8, 13, 13, 6, 12])
    return U, I, edges, users, pos, neg


@pytest.mark.parametrize("graph", ["tiny_isolated_rows", "baby"])
def test_reference_equals_autograd_fp64(graph):
    if graph == "baby":
        d = load_interactions("baby")
        U, I, edges = d["U"], d["I"], d["train"]
        users, pos, neg = _batch(np.random.default_rng(1), edges, U, I, 512)
        D, L = 16, 3
    else:
        U, I, edges, users, pos, neg = _tiny_with_isolated_rows()
        D, L = 8, 2
    torch.manual_seed(4)
    model = TorchRefLightGCN(U, I, edges, None, D, REG, L).double()
    loss = model.loss(users, pos, neg)
    loss.backward()
    grad = torch.cat((model.user_embedding.weight.grad, model.item_embedding.weight.grad), 0)
    W = torch.cat((model.user_embedding.weight, model.item_embedding.weight), 0).detach()
    rowptr, col, val = torch_ref_csr(model.edge_index, U + I, torch.float64)
    z = torch.zeros_like(W)
    ref = lightgcn_step_fp64(rowptr, col, val, W, users, pos - U, neg - U, U, REG, L, z, z, 1, LR)

    def close(a, b):
        return float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())

    assert close(ref["result"][0], model.result.detach())
    assert abs(float(ref["loss"][0]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert close(ref["grad"][0], grad)
    if graph == "tiny_isolated_rows":
        # the isolated rows: propagated row = w x0, gradient = w G (nothing else reaches them)
        iso = torch.tensor([5, 12, 13])
        assert close(ref["result"][0][iso], W[iso] / (L + 1))
        assert close(ref["grad"][0][iso], ref["G"][0][iso] / (L + 1))
        assert bool((ref["G"][0][iso] != 0).all(1).all())


# ---- sports, D = 64, L = 3, B = 1024: an independent fp32 step against the bound ----------------------------------------

@pytest.fixture(scope="module")
def sports_states():
    """{"t1": ..., "warm": ...}: an fp32 model + Adam about to take step 1 / step 31 (after 30 warm-up steps), the batch of
    that step and the fp64 reference of it."""
    d = load_interactions("sports")
    U, I, edges = d["U"], d["I"], d["train"]
    torch.manual_seed(11)
    model = Fp32Step(U, I, edges, 64, 3)
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    rng = np.random.default_rng(12)
    out = {}
    for t in range(31):
        batch = _batch(rng, edges, U, I, 1024)
        if t in (0, 30):
            model.result = model.ego = None
            out["t1" if t == 0 else "warm"] = (copy.deepcopy(model), copy.deepcopy(opt.state_dict()), batch,
                                               _reference(model, opt, *batch))
        if t < 30:
            model.step(opt, *batch)
    return out


def _fresh(state):
    model, opt_state, batch, ref = state
    model = copy.deepcopy(model)
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    opt.load_state_dict(copy.deepcopy(opt_state))
    return model, opt, batch, ref


@pytest.mark.parametrize("when", ["t1", "warm"])
def test_fp32_step_stays_inside_the_bound(sports_states, when):
    model, opt, batch, ref = _fresh(sports_states[when])
    loss = model.step(opt, *batch)
    r = _ratios(model, opt, loss, ref)
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_mutated_fp32_step_leaves_the_bound(sports_states, mutation):
    model, opt, batch, ref = _fresh(sports_states["warm"])
    users = batch[0]
    if mutation == "user_repeat_dropped_from_gradient":
        cnt = torch.bincount(users)
        top = int(cnt.argmax())
        assert int(cnt[top]) >= 2                        # a user that occurs more than once in the batch
        model.drop_sample = int((users == top).nonzero()[0])
    if mutation == "zero_gradient_rows_not_updated":
        # rows with no gradient this step (isolated items outside the batch) that still carry momentum
        m, _ = model.moments(opt)
        assert bool(((ref["grad"][0] == 0).all(1) & (m != 0).any(1)).any())
    model.mutation = mutation
    loss = model.step(opt, *batch)
    r = _ratios(model, opt, loss, ref)
    assert max(r.values()) > 1.0, r


# Measured on sports (D = 64, L = 3, B = 1024, lr 1e-3), step 1 / step 31: median bound / median |value| is 2.7e-6 / 2.2e-6
# (result), 4.4e-5 / 3.9e-6 (m'), 8.5e-5 / 8.0e-7 (v'), 1.1e-6 / 2.0e-7 (W'); no W' element has a bound above 0.1 lr, the
# loss bound is 6e-5 of the loss.  The thresholds are a few times that: a bound that grew loose enough to hide a real
# mistake fails here.
NOT_VACUOUS = {"result": 1e-5, "m": 2e-4, "v": 4e-4, "W": 5e-6}
W_LOOSE_SHARE = 1e-3


@pytest.mark.parametrize("when", ["t1", "warm"])
def test_bounds_are_not_vacuous(sports_states, when):
    ref = sports_states[when][3]
    for key, lim in NOT_VACUOUS.items():
        value, bound = ref[key]
        rel = float(bound.median()) / max(float(value.abs().median()), 1e-30)
        assert rel <= lim, (key, rel)
    value, bound = ref["loss"]
    assert float(bound) <= 1e-4 * abs(float(value))
    share = float((ref["W"][1] > 0.1 * LR).double().mean())
    assert share <= W_LOOSE_SHARE, share
