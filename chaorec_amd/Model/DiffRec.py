"""DiffRec with the reference's surface (Model/DiffRec.py:16-546): the time-conditioned MLP denoiser and the Gaussian
diffusion around it, the training loss and the sampling chain on csrc/diffrec.hip.

Same constructor, method names and state_dict names (`dnn.emb_layer`, `dnn.in_layers.0`, `dnn.out_layers.0`, weight and
bias each) in the reference's order, drawn call for call: the same torch seed gives the same weights.  `dnn` is DiffMM's
Denoise, which is the reference's DNN line for line (time embedding as a 10-wide second product, input dropout 0.5, one tanh
layer each way, init_weights' order).  The diffusion tables are float64 with betas[0] = 1e-5; the timestep importance
sampling, update_Lt_history and the SNR weight (which reads index ts - 1 = -1 at ts = 0 before the where replaces it) are
CF_Diff's functions themselves, bound here as methods.  noise_scale = 0 raises as in CF_Diff: the reference builds no betas
for it and fails in calculate_for_diffusion.

What changed underneath.

Training.  No dense [U, I] matrix exists: `diffusion_step(users)` writes the noised, dropped-out rows of a batch and the bit
table of x0 from the history CSR in one launch (ops.diffmm_rows, noise and keep flags from the counter RNG keyed by user
and item), runs the in-layer on the MFMA GEMMs (Denoise.hidden) and the out-layer with the importance-weighted x0 loss and
d loss / d out in one pass (ops.diffrec_x0_loss): model_output never exists.

Sampling.  norm = False, sampling_steps = 0 and sampling_noise = False are fixed in the reference's constructor, so between
the tanh's the whole chain x^(T) = x_start, x^(t) = c1[t] (Wo tanh(W1x x^(t+1) + e_t) + bo) + c2[t] x^(t+1) is linear in item
space.  With p^(t) = W1x x^(t), G = W1x Wo [H, H], g0 = W1x bo, e_t = W1e emb(t) + b1:
    p^(T) = the history rows' sum of W1x's columns (an SpMM),  z_t = tanh(p^(t+1) + e_t),
    p^(t) = c1[t] (G z_t + g0) + c2[t] p^(t+1),
    x^(0) = Wo (sum_t a_t z_t) + (sum_t a_t) bo + beta x_start,   a_t = c1[t] prod_{s<t} c2[s],  beta = prod_s c2[s]
(DESIGN 3.23).  `gene_ranklist` computes G, g0, the e_t and W1x^T once per call, then per user range steps - 1 launches of
ops.diffrec_chain_step and ONE [B, H] x [H, I] product instead of `steps` passes of two such products on dense rows.  The
general a_t, beta form is kept although the reference's tables give c2[0] = 0, hence beta = 0 and x^(0) = Wo z_0 + bo.

Fall-backs.  The literal chain (`steps` denoiser passes on dense rows, on the device through Denoise.denoise) runs when
collapsed = False, when sampling_steps != 0 or sampling_noise is set, when `dims` has more than one entry, and on the device
when H is no multiple of 4 or above 1024 (what ops.spmm and the tile take).  fused = False runs the reference's
training_losses lines in plain torch on dense rows.  A CPU model runs every route in plain torch (ops.*_plain).

fused and collapsed default to True because the measurement says so (profiles/diffrec_sports_bench.json, `fused_default` and
`collapsed_default`, written by tools/bench_diffrec.py: at sports, B = 1024, H = 1000 one training step takes 3.26 ms fused
against 3.49 ms plain, one evaluation 35 ms collapsed against 115 ms for the literal chain).
"""
import ast

import numpy as np
import torch
import torch.nn as nn

from .. import graph, ops
from ..ops_dense import _linear_fwd_raw, gemm_raw
from .CF_Diff import CF_Diff
from .DiffMM import Denoise

SPMM_MAX_WIDTH = 1024           # the widest table ops.spmm takes (multiples of 4)


class DiffRec(nn.Module):
    def __init__(self, num_user, num_item, user_item_dict, noise_scale, noise_min, noise_max, steps, dims, learning_rate, device,
                 seed=None, fused=True, collapsed=True):
        super(DiffRec, self).__init__()
        self.num_user = num_user
        self.num_item = num_item
        self.user_item_dict = user_item_dict
        self.device = device
        self.learning_rate = learning_rate
        self.noise_schedule = "linear"
        self.noise_scale = noise_scale
        self.noise_min = noise_min
        self.noise_max = noise_max
        self.steps = steps
        self.sampling_steps = 0
        self.sampling_noise = False
        self.reweight = noise_scale != 0.0
        self.mean_type = 'x0'
        self.beta_fixed = True
        self.history_num_per_term = 10
        self.Lt_history = torch.zeros(steps, self.history_num_per_term, dtype=torch.float64).to(device)
        self.Lt_count = torch.zeros(steps, dtype=torch.long).to(device)
        if noise_scale == 0.0:
            raise NotImplementedError("DiffRec: noise_scale = 0 (the reference builds no betas for it and fails in calculate_for_diffusion)")
        self.betas = torch.tensor(self.get_betas(), dtype=torch.float64).to(self.device)
        if self.beta_fixed:
            self.betas[0] = 0.00001
        assert len(self.betas.shape) == 1 and len(self.betas) == self.steps
        self.calculate_for_diffusion()

        self.dims = dims
        self.emb_size = 10
        self.norm = False
        out_dims = list(ast.literal_eval(dims) if isinstance(dims, str) else dims) + [num_item]
        in_dims = out_dims[::-1]
        self.dnn = Denoise(in_dims, out_dims, self.emb_size, norm=self.norm).to(device)

        dev = torch.device(device)
        self.hidden_width = int(out_dims[0])
        one_layer = len(out_dims) == 2
        self.fused = bool(fused) and dev.type == "cuda" and one_layer and self.hidden_width % 4 == 0
        self.collapsed = bool(collapsed) and one_layer
        self.seed = (int(torch.initial_seed()) if seed is None else int(seed)) & 0x7FFFFFFFFFFFFFFF
        rowptr, col = graph.user_hist_csr(user_item_dict, num_user)
        self._entry_row = torch.repeat_interleave(torch.arange(num_user, dtype=torch.int64), rowptr[1:] - rowptr[:-1]).to(dev)
        self._rowptr_host = rowptr.numpy().copy()
        self.hist = (rowptr.to(dev), col.to(dev))
        self._hist_csr = None           # the history as a unit-valued CSR, built at the first collapsed ranking on the device
        self._step = 0
        self.last = {}

    # ---- the schedule, the importance sampling and the loss history: CF_Diff's functions (Model/CF_Diff.py) -------------------
    get_betas = CF_Diff.get_betas
    calculate_for_diffusion = CF_Diff.calculate_for_diffusion
    mean_flat = CF_Diff.mean_flat
    SNR = CF_Diff.SNR
    _extract_into_tensor = CF_Diff._extract_into_tensor
    q_sample = CF_Diff.q_sample
    q_posterior_mean = CF_Diff.q_posterior_mean
    weight = CF_Diff.weight
    reweight_loss = CF_Diff.reweight_loss
    importance_pt = CF_Diff.importance_pt
    sample_timesteps = CF_Diff.sample_timesteps
    update_Lt_history = CF_Diff.update_Lt_history
    batch_rows = CF_Diff.batch_rows

    # ---- training (:425-463) ---------------------------------------------------------------------------------------------------
    def diffusion_step(self, users, ts=None, noise=None, keep=None):
        """training_losses for a batch of user ids -> the loss.  ts int64 [B], noise fp32 [B, I], keep flags [B, I]: given
        draws (pt is then 1).  Without them: sample_timesteps('importance'), and noise and the input dropout's flags from the
        counter RNG inside the rows launch (fused) or torch.randn and nn.Dropout (plain)."""
        dev = torch.device(self.device)
        users = users.to(dev).to(torch.int64)
        B = users.numel()
        if ts is None:
            ts, pt = self.sample_timesteps(B, dev, 'importance')
        else:
            ts, pt = ts.to(dev).long(), torch.ones(B, device=dev)
        noise = None if noise is None else noise.to(dev)
        keep = None if keep is None else keep.to(dev)
        self._step += 1
        if self.fused:
            a = self.sqrt_alphas_cumprod[ts].float().contiguous()
            s = self.sqrt_one_minus_alphas_cumprod[ts].float().contiguous()
            x_in, bits = ops.diffmm_rows(users, self.hist[0], self.hist[1], self.num_item, a, s, noise, keep, self.seed, self._step, salt=0)
            h = self.dnn.hidden(x_in, ts)
            out = self.dnn.out_layers[0]
            loss, reloss = ops.diffrec_x0_loss(h, out.weight, out.bias, bits, self.weight(ts), pt)
            loss = loss.reshape(())
        else:
            x_start = self.batch_rows(users)
            x_t = self.q_sample(x_start, ts, noise)
            model_output = self.dnn(x_t, ts, True, keep)
            reloss = self.reweight_loss(self.mean_flat((x_start - model_output) ** 2), ts)
            loss = (reloss / pt).mean()
        self.update_Lt_history(ts, reloss)
        self.last = dict(ts=ts, pt=pt, reloss=reloss.detach())
        return loss

    def training_losses(self, x_start):
        """The reference's signature over dense rows (:425-463), in plain torch."""
        ts, pt = self.sample_timesteps(x_start.size(0), x_start.device, 'importance')
        x_t = self.q_sample(x_start, ts, torch.randn_like(x_start))
        model_output = self.dnn(x_t, ts)
        reloss = self.reweight_loss(self.mean_flat((x_start - model_output) ** 2), ts)
        self.update_Lt_history(ts, reloss)
        return (reloss / pt).mean()

    # ---- sampling (:263-303) ---------------------------------------------------------------------------------------------------
    def posterior_coefs(self):
        """(c1, c2, a, beta): the posterior-mean coefficients as _extract_into_tensor's .float() leaves them (Python floats of
        the fp32 values), a_t = c1[t] prod_{s<t} c2[s] and beta = prod_s c2[s] formed from them in double."""
        c1 = [float(v) for v in self.posterior_mean_coef1.float().cpu()]
        c2 = [float(v) for v in self.posterior_mean_coef2.float().cpu()]
        a, prod = [], 1.0
        for t in range(self.steps):
            a.append(c1[t] * prod)
            prod *= c2[t]
        return c1, c2, a, prod

    def collapse_route(self, dev_type):
        """Whether p_sample / gene_ranklist take the hidden-space chain on a device of that type (see the module docstring)."""
        if not self.collapsed or self.sampling_steps != 0 or self.sampling_noise or len(self.dnn.in_layers) != 1 or self.norm:
            return False
        H = self.hidden_width
        return dev_type != "cuda" or (H % 4 == 0 and H <= SPMM_MAX_WIDTH)

    def collapse_tables(self):
        """Once per sampling pass: W1x (a view of the in-layer's weight), W1x^T [I, H] (contiguous: the SpMM's table), G = W1x Wo [H, H], g0 = W1x bo [H], e [steps, H]
        with e[t] = W1e emb_layer(timestep_embedding(t)) + b1, and Wo, bo."""
        I = self.num_item
        W1, b1 = self.dnn.in_layers[0].weight.detach(), self.dnn.in_layers[0].bias.detach()
        Wo, bo = self.dnn.out_layers[0].weight.detach(), self.dnn.out_layers[0].bias.detach()
        W1xT = W1[:, :I].t().contiguous()
        if W1.is_cuda:
            G = gemm_raw(W1xT, Wo, transA=True)                             # [H, I] [I, H]
            g0 = gemm_raw(bo.reshape(1, I), W1xT).reshape(-1)
        else:
            G, g0 = W1xT.t() @ Wo, bo @ W1xT
        t = torch.arange(self.steps, dtype=torch.int64, device=W1.device)
        emb = self.dnn.emb_layer(self.dnn.time_embedding(t)).detach()
        e = (emb @ W1[:, I:].t() + b1).contiguous()
        return dict(W1x=W1[:, :I], W1xT=W1xT, G=G.contiguous(), g0=g0.contiguous(), e=e, Wo=Wo, bo=bo)

    def hidden_chain(self, p, tables):
        """p^(T) [B, H] -> out = Wo (sum_t a_t z_t) + (sum_t a_t) bo [B, I]: steps - 1 chain launches and one output product."""
        c1, c2, a, _ = self.posterior_coefs()
        T, e = self.steps, tables["e"]
        kernels = p.is_cuda
        step = ops.diffrec_chain_step if kernels else ops.diffrec_chain_step_plain
        z = torch.tanh(p + e[T - 1])
        acc = z * a[T - 1]
        for t in range(T - 1, 0, -1):
            p, z = step(z, tables["G"], tables["g0"], p, e[t - 1], c1[t], c2[t])
            if a[t - 1] != 0.0:
                acc = acc + z * a[t - 1]
        bias = tables["bo"] * float(sum(a))
        if kernels:
            return _linear_fwd_raw(acc.contiguous(), tables["Wo"], bias.contiguous(), 0)
        return acc @ tables["Wo"].t() + bias

    def p_sample_literal(self, x_start):
        """The reference's chain on dense rows: `steps` denoiser passes, t = steps - 1 .. 0 (sampling_steps = 0, no noise)."""
        if self.sampling_steps != 0 or self.sampling_noise:
            raise NotImplementedError("DiffRec: the reference fixes sampling_steps = 0 and sampling_noise = False")
        x_t = x_start
        kernels = x_start.is_cuda and len(self.dnn.in_layers) == 1 and self.hidden_width % 4 == 0
        for i in list(range(self.steps))[::-1]:
            t = torch.full((x_t.shape[0],), i, dtype=torch.int64, device=x_start.device)
            out = self.dnn.denoise(x_t, t) if kernels else self.dnn(x_t, t, False)
            x_t = self.q_posterior_mean(out, x_t, t)
        return x_t

    def p_sample(self, x_start):
        """The reference's dense signature -> the dense rows x^(0) [B, I], beta x_start included."""
        if not self.collapse_route(x_start.device.type):
            return self.p_sample_literal(x_start)
        tables = self.collapse_tables()
        if x_start.is_cuda:
            p = _linear_fwd_raw(x_start, tables["W1x"], None, 0)
        else:
            p = x_start @ tables["W1xT"]
        out = self.hidden_chain(p, tables)
        beta = self.posterior_coefs()[3]
        return out + beta * x_start if beta != 0.0 else out

    def gene_ranklist(self, topk=50, to_cpu=True, batch_size=1024):
        """train_and_evaluate.py:578-613: per user range the denoised rows in eval mode, history set to -inf, top-k, + num_user.
        Collapsed: the tables once, p^(T) of every user by one SpMM of the history CSR with W1x^T, then per range the chain
        launches and one output product; beta x_start is left out, it lies on history items only.  Otherwise the literal chain
        on the range's dense rows."""
        dev = torch.device(self.device)
        was_training = self.training
        self.eval()
        out = []
        rowptr, col = self.hist
        with torch.no_grad():
            collapsed = self.collapse_route(dev.type)
            if collapsed:
                tables = self.collapse_tables()
                if dev.type == "cuda":
                    if self._hist_csr is None:
                        ones = torch.ones(col.numel(), dtype=torch.float32, device=dev)
                        self._hist_csr = graph.CSR(rowptr, col, ones, self.num_user, self.num_item)
                    P = ops.spmm(self._hist_csr, tables["W1xT"])
            for u0 in range(0, self.num_user, batch_size):
                u1 = min(u0 + batch_size, self.num_user)
                if collapsed and dev.type == "cuda":
                    pred = self.hidden_chain(P[u0:u1], tables)
                elif collapsed:
                    users = torch.arange(u0, u1, dtype=torch.int64, device=dev)
                    pred = self.hidden_chain(self.batch_rows(users) @ tables["W1xT"], tables)
                else:
                    users = torch.arange(u0, u1, dtype=torch.int64, device=dev)
                    pred = self.p_sample_literal(self.batch_rows(users))
                e0, e1 = int(self._rowptr_host[u0]), int(self._rowptr_host[u1])
                pred[self._entry_row[e0:e1] - u0, col[e0:e1].long()] = -np.inf
                if pred.is_cuda:
                    out.append(ops.rows_topk(pred.contiguous(), topk, self.num_user)[0])
                else:
                    out.append(torch.topk(pred, topk, dim=1)[1] + self.num_user)
        self.train(was_training)
        rank = torch.cat(out, 0)
        return rank.cpu() if to_cpu else rank

    full_sort_predict = gene_ranklist
