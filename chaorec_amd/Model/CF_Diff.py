"""CF_Diff with the reference's surface (Model/CF_Diff.py:16-521): the cross-attention denoiser CAM_AE and the Gaussian
diffusion around it, the attention core on csrc/cfdiff.hip.

CAM_AE.forward keeps the reference's lines (:75-135): ONE encoder for both hops, emb_layer on the sinusoidal embedding,
drop (0.5) AFTER the encoder, the two Linear(1, 16) expansions that turn each of the L = dim_inters + 10 scalars into a token,
per layer [in-projections, attention core with the second-hop tokens as queries, out_proj, drop1 (0.8), the residual, drop2
(0.5) on the whole sum, Linear(16, 16), tanh except after the last layer], then Linear(16, 1), tanh and the decoder.

Not created: in_layers, out_layers, encoder2, final_out, norm1, norm2.  The reference constructs them and never reads them,
so they receive no gradient there and AdamW never moves them; the state_dict here holds the 24 tensors that are read, under
the reference's names.  The reference's bare torch.squeeze after first_hop_decoding also drops a batch of one; the reshape
here is [B, L] explicitly.

What changed underneath.  nn.MultiheadAttention with its default need_weights = True materialises [4 B, L, L] scores, the
softmax, the dropout mask and the dropped product (17.5 GB each at the logged B = 1024); `ops.cfdiff_attention` is one
forward and one backward node that form none of them and redraw the dropout flags from a counter RNG.  No dense [U, I]
matrix exists: x_t rows come from the history CSR through the rows launch of csrc/diffmm.hip (no input dropout), and
DiffusionData_sec_hop (dataload.py:215-256) is the same CSR with the values cnt[i] / U, so encoder(x_sec_hop) is an SpMM with
encoder.weight^T (over all users, the batch's rows selected: the gradient reaches the weight through the transposed CSR).
The reference's two DataLoaders shuffle independently, so its x and x_sec_hop rows of one batch belong to different users;
here both are the batch's users'.  The decoder and the loss stay torch operations.

fused defaults to True because the measurement says so (profiles/cfdiff_attention_bench.json, `fused_default`: at L = 1034,
B = 1024 the fused forward + backward takes 9.1 ms against 93.7 ms for nn.MultiheadAttention and 123 ms for the plain
composition, and 0.3 GB against 67 GB).  fused = False (and every CPU tensor) runs the same lines with `ops.cfdiff_attention_plain` and dense rows; an L above
ops.cfdiff_max_len() takes the plain attention too.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import graph, ops


def _drop(x, p, keep, training):
    """F.dropout(x, p) or, keep given, the same scaling with those flags."""
    if not training:
        return x
    if keep is None:
        return F.dropout(x, p, True)
    return x * (keep.to(device=x.device, dtype=x.dtype) * (1.0 / (1.0 - p)))


class CAM_AE(nn.Module):
    def __init__(self, d_model, num_heads, num_layers, in_dims, emb_size, time_type="cat", norm=False, dropout=0.5, dim_inters=1024):
        super(CAM_AE, self).__init__()
        if (d_model, num_heads) != (ops.CFDIFF_WIDTH, ops.CFDIFF_HEADS):
            raise ValueError(f"CAM_AE: d_model={d_model}, num_heads={num_heads}; the attention is written for 16 and 4")
        self.in_dims = in_dims
        self.time_type = time_type
        self.time_emb_dim = emb_size
        self.norm = norm
        self.num_layers = num_layers
        self.d_model = d_model
        self.dim_inters = int(dim_inters)
        self.emb_layer = nn.Linear(self.time_emb_dim, self.time_emb_dim)
        self.forward_layers = nn.ModuleList([nn.Linear(d_model, d_model) for i in range(num_layers)])
        self.first_hop_embedding = nn.Linear(1, d_model)
        self.first_hop_decoding = nn.Linear(d_model, 1)
        self.second_hop_embedding = nn.Linear(1, d_model)
        self.drop = nn.Dropout(dropout)
        self.drop1 = nn.Dropout(0.8)
        self.drop2 = nn.Dropout(dropout)
        self.encoder = nn.Linear(self.in_dims, self.dim_inters)
        self.decoder = nn.Linear(self.dim_inters + emb_size, self.in_dims)
        self.self_attentions = nn.ModuleList([nn.MultiheadAttention(d_model, num_heads, dropout=0.5, batch_first=True)
                                              for i in range(num_layers)])
        # set by CF_Diff: the route of the attention core and what its device draws are keyed by
        self.fused = False
        self.seed = 0
        self.draw_state = None

    def timestep_embedding(self, timesteps, dim, max_period=10000):
        half = dim // 2
        freqs = torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half).to(timesteps.device)
        args = timesteps[:, None].float() * freqs[None]
        embedding = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
        if dim % 2:
            embedding = torch.cat([embedding, torch.zeros_like(embedding[:, :1])], dim=-1)
        return embedding

    def use_kernels(self, x):
        return bool(self.fused) and x.is_cuda and x.dtype == torch.float32

    def _linear(self, layer, x):
        if self.use_kernels(x):
            return ops.linear(x, layer.weight, layer.bias)
        return layer(x)

    def attention(self, i, h_sec_hop, h, keep=None):
        """self_attentions[i](h_sec_hop, h, h)[0] (:111): F.multi_head_attention_forward's in-projections, core, out_proj."""
        mha, E = self.self_attentions[i], self.d_model
        W, b = mha.in_proj_weight, mha.in_proj_bias
        q, k, v = F.linear(h_sec_hop, W[:E], b[:E]), F.linear(h, W[E:2 * E], b[E:2 * E]), F.linear(h, W[2 * E:], b[2 * E:])
        if self.use_kernels(q) and q.shape[1] <= ops.cfdiff_max_len():
            core = ops.cfdiff_attention(q, k, v, self.training, self.seed, self.draw_state, i, keep)
        else:
            core = ops.cfdiff_attention_plain(q, k, v, self.training, self.seed, self.draw_state, i, keep)
        return F.linear(core, mha.out_proj.weight, mha.out_proj.bias)

    def forward(self, x, x_sec_hop, timesteps, keeps=None, h_sec_hop=None):
        """x [B, I]; x_sec_hop [B, I] or, h_sec_hop given, unused (the encoded second hop, [B, dim_inters]).  keeps: given
        flags {"drop": [B, dim_inters], "attn": [layers x [B, 4, L, L]], "drop1": [layers x [B, L, 16]], "drop2": likewise}."""
        keeps = keeps or {}
        B = x.shape[0]
        x = self._linear(self.encoder, x)
        if h_sec_hop is None:
            h_sec_hop = self._linear(self.encoder, x_sec_hop)
        time_emb = self.timestep_embedding(timesteps, self.time_emb_dim).to(device=x.device, dtype=x.dtype)
        emb = self.emb_layer(time_emb)
        if self.norm:
            x = F.normalize(x)
        x = _drop(x, self.drop.p, keeps.get("drop"), self.training)
        h = self.first_hop_embedding(torch.cat([x, emb], dim=-1).unsqueeze(-1))
        h_sec_hop = self.second_hop_embedding(torch.cat([h_sec_hop, emb], dim=-1).unsqueeze(-1))
        for i in range(self.num_layers):
            given = {name: (keeps[name][i] if name in keeps else None) for name in ("attn", "drop1", "drop2")}
            attention = self.attention(i, h_sec_hop, h, given["attn"])
            attention = _drop(attention, self.drop1.p, given["drop1"], self.training)
            h = h + attention
            h = _drop(h, self.drop2.p, given["drop2"], self.training)
            h = self.forward_layers[i](h)
            if i != self.num_layers - 1:
                h = torch.tanh(h)
        h = self.first_hop_decoding(h).reshape(B, -1)
        h = torch.tanh(h)
        return self._linear(self.decoder, h)


class CF_Diff(nn.Module):
    def __init__(self, num_user, num_item, user_item_dict, noise_scale, noise_min, noise_max, steps, learning_rate, device,
                 fused=True, seed=None, dim_inters=1024):
        super(CF_Diff, self).__init__()
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
            raise NotImplementedError("CF_Diff: noise_scale = 0 (the reference builds no betas for it and fails in calculate_for_diffusion)")
        self.betas = torch.tensor(self.get_betas(), dtype=torch.float64).to(self.device)
        if self.beta_fixed:
            self.betas[0] = 0.00001
        assert len(self.betas.shape) == 1 and len(self.betas) == self.steps
        self.calculate_for_diffusion()
        self.emb_size = 10
        self.CAM_AE = CAM_AE(16, 4, 2, num_item, self.emb_size, dim_inters=dim_inters).to(device)

        dev = torch.device(device)
        self.fused = bool(fused) and dev.type == "cuda"
        if self.fused and int(dim_inters) % 4:
            raise ValueError(f"CF_Diff: dim_inters={dim_inters}; the SpMM of the second hop tiles a multiple of 4 (fused=False has no limit)")
        self.seed = (int(torch.initial_seed()) if seed is None else int(seed)) & 0x7FFFFFFFFFFFFFFF
        rowptr, col = graph.user_hist_csr(user_item_dict, num_user)
        self.hist = (rowptr.to(dev), col.to(dev))
        # DiffusionData_sec_hop's rows (dataload.py:238-256): cnt[i] / U where the user holds item i, in fp32 as torch.sum / U
        cnt = torch.bincount(col.long(), minlength=num_item).to(torch.float32)
        self.sec_hop_val = (cnt / num_user)[col.long()].contiguous().to(dev)
        self._sec_csr = graph.CSR(self.hist[0], self.hist[1], self.sec_hop_val, num_user, num_item) if self.fused else None
        self._state = torch.zeros(2, dtype=torch.int64, device=dev)
        self._step = 0
        self._sec_table = None          # gene_ranklist: the second hop of every user, encoded once per ranking pass
        self.CAM_AE.fused, self.CAM_AE.seed, self.CAM_AE.draw_state = self.fused, self.seed, self._state
        self.last = {}

    # ---- the schedule (:195-274) ------------------------------------------------------------------------------------------
    def get_betas(self):
        start = self.noise_scale * self.noise_min
        end = self.noise_scale * self.noise_max
        return np.linspace(start, end, self.steps, dtype=np.float64)

    def calculate_for_diffusion(self):
        alphas = 1.0 - self.betas
        dev = self.betas.device
        self.alphas_cumprod = torch.cumprod(alphas, dim=0)
        self.alphas_cumprod_prev = torch.cat([torch.tensor([1.0], dtype=torch.float64, device=dev), self.alphas_cumprod[:-1]])
        self.alphas_cumprod_next = torch.cat([self.alphas_cumprod[1:], torch.tensor([0.0], dtype=torch.float64, device=dev)])
        self.sqrt_alphas_cumprod = torch.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = torch.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = torch.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = torch.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = torch.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = self.betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = torch.log(torch.cat([self.posterior_variance[1].unsqueeze(0), self.posterior_variance[1:]]))
        self.posterior_mean_coef1 = self.betas * torch.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * torch.sqrt(alphas) / (1.0 - self.alphas_cumprod)

    def mean_flat(self, tensor):
        return tensor.mean(dim=list(range(1, len(tensor.shape))))

    def SNR(self, t):
        ac = self.alphas_cumprod.to(t.device)
        return ac[t] / (1 - ac[t])

    def _extract_into_tensor(self, arr, timesteps, broadcast_shape):
        res = arr.to(timesteps.device)[timesteps].float()
        while len(res.shape) < len(broadcast_shape):
            res = res[..., None]
        return res.expand(broadcast_shape)

    def q_sample(self, x_start, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_start)
        return (self._extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
                + self._extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise)

    def q_posterior_mean(self, x_start, x_t, t):
        return (self._extract_into_tensor(self.posterior_mean_coef1, t, x_t.shape) * x_start
                + self._extract_into_tensor(self.posterior_mean_coef2, t, x_t.shape) * x_t)

    # ---- rows without a dense [U, I] ---------------------------------------------------------------------------------------
    def batch_rows(self, users, values=None):
        """The rows [B, I] of a batch of users from the history CSR: multi-hot, or `values` (one per CSR entry) scattered."""
        rowptr, col = self.hist
        if values is None and rowptr.is_cuda and self.fused:
            return ops.diffmm_rows(users, rowptr, col, self.num_item, plain=True)[0]
        n = rowptr[users + 1] - rowptr[users]
        rows = torch.repeat_interleave(torch.arange(users.numel(), device=users.device), n)
        pos = torch.arange(int(n.sum()), device=users.device) - torch.repeat_interleave(torch.cumsum(n, 0) - n, n)
        entry = rowptr[users][rows] + pos
        x = torch.zeros((users.numel(), self.num_item), dtype=torch.float32, device=users.device)
        x[rows, col[entry].long()] = 1.0 if values is None else values[entry]
        return x

    def sec_hop_rows(self, users):
        """DiffusionData_sec_hop's rows of the batch, dense (the plain route and the tests)."""
        return self.batch_rows(users, self.sec_hop_val)

    def encode_sec_hop(self, users):
        """encoder(x_sec_hop) for the batch without x_sec_hop: the cnt / U-valued CSR times encoder.weight^T, plus the bias."""
        enc = self.CAM_AE.encoder
        table = self._sec_table if self._sec_table is not None else ops.spmm(self._sec_csr, enc.weight.t().contiguous())
        return table[users] + enc.bias

    def denoise(self, x_t, users, ts, keeps=None):
        """CAM_AE(x_t, x_sec_hop of `users`, ts)."""
        if self.fused:
            return self.CAM_AE(x_t, None, ts, keeps, h_sec_hop=self.encode_sec_hop(users))
        return self.CAM_AE(x_t, self.sec_hop_rows(users), ts, keeps)

    # ---- training (:411-521) -----------------------------------------------------------------------------------------------
    def weight(self, ts):
        """:450-452: float64; SNR(ts - 1) is read at ts = 0 too (index -1, the last step) before the where replaces it."""
        weight = self.SNR(ts - 1) - self.SNR(ts)
        return torch.where((ts == 0), 1.0, weight)

    def reweight_loss(self, mse, ts):
        return (self.weight(ts) if self.reweight else torch.ones_like(mse)) * mse

    def importance_pt(self, uniform_prob=0.001):
        """:502-505: the sampling distribution over timesteps from the loss history."""
        Lt_sqrt = torch.sqrt(torch.mean(self.Lt_history ** 2, dim=-1))
        pt_all = Lt_sqrt / torch.sum(Lt_sqrt)
        pt_all = pt_all * (1 - uniform_prob)
        return pt_all + uniform_prob / len(pt_all)

    def sample_timesteps(self, batch_size, device, method='uniform', uniform_prob=0.001):
        if method == 'importance':
            if not (self.Lt_count == self.history_num_per_term).all():
                return self.sample_timesteps(batch_size, device, method='uniform')
            pt_all = self.importance_pt(uniform_prob)
            t = torch.multinomial(pt_all, num_samples=batch_size, replacement=True)
            pt = pt_all.gather(dim=0, index=t) * len(pt_all)
            return t, pt
        elif method == 'uniform':
            t = torch.randint(0, self.steps, (batch_size,), device=device).long()
            pt = torch.ones_like(t).float()
            return t, pt
        raise ValueError

    def update_Lt_history(self, ts, reloss):
        """:471-486 without a host read per element.  The reference walks the batch in order: an occurrence of timestep t is
        appended at Lt_count[t] while the row has room, and once it is full every further occurrence shifts the row left by
        one and lands in the last slot.  With c = Lt_count[t], r = the occurrence's rank among the batch's occurrences of t
        and m = their number: occurrences with c + r < 10 fill slot c + r; the row ends up shifted by s = max(0, c + m - 10),
        so an old slot j >= s moves to j - s and occurrence r lands in c + r - s when that is >= 0 (else it was shifted out)."""
        H, T = self.history_num_per_term, self.steps
        ts = ts.to(self.Lt_count.device)
        loss = reloss.detach().to(self.Lt_history.dtype).to(self.Lt_count.device)
        onehot = F.one_hot(ts, T)                                                 # [B, T]
        rank = (torch.cumsum(onehot, 0) - onehot).gather(1, ts[:, None]).squeeze(1)    # occurrences of ts[b] before b
        m = onehot.sum(0)                                                         # [T]
        c = self.Lt_count
        shift = torch.clamp(c + m - H, min=0)                                     # [T]
        j = torch.arange(H, device=c.device)
        src = j[None, :] + shift[:, None]                                         # old slot that moves to j
        moved = self.Lt_history.gather(1, src.clamp(max=H - 1))
        new_hist = torch.where(j[None, :] < (c - shift)[:, None], moved, self.Lt_history)    # slots past c + m keep their content
        dst = c[ts] + rank - shift[ts]                 # < 0: shifted out again inside this batch -> a spare column, cut off below
        wide = torch.cat([new_hist, torch.zeros_like(new_hist[:, :1])], 1)
        wide[ts, torch.where(dst >= 0, dst, torch.full_like(dst, H))] = loss       # (index pairs are distinct but for the spare column)
        self.Lt_history = wide[:, :H].contiguous()
        self.Lt_count = torch.clamp(c + m, max=H)

    def diffusion_step(self, users, ts=None, noise=None, keeps=None):
        """training_losses (:411-442) for a batch of user ids -> the loss.  ts int64 [B], noise fp32 [B, I], keeps (see
        CAM_AE.forward): given draws.  Without them: sample_timesteps('importance'), noise from the counter RNG inside the rows
        launch (fused) or torch.randn, F.dropout for the elementwise dropouts and the device draws for the attention."""
        dev = torch.device(self.device)
        users = users.to(dev).to(torch.int64)
        B = users.numel()
        if ts is None:
            ts, pt = self.sample_timesteps(B, dev, 'importance')
        else:
            ts, pt = ts.to(dev).long(), torch.ones(B, device=dev)
        self._step += 1
        if self._state.is_cuda:         # the step the attention's device draws are keyed by (the plain route redraws them too)
            ops.step_tick(self._state)
        x_start = self.batch_rows(users)
        if self.fused:
            a = self.sqrt_alphas_cumprod[ts].float().contiguous()
            s = self.sqrt_one_minus_alphas_cumprod[ts].float().contiguous()
            x_t = ops.diffmm_rows_noised(users, self.hist[0], self.hist[1], self.num_item, a, s,
                                         None if noise is None else noise.to(dev), self.seed, self._step, salt=7)
        else:
            x_t = self.q_sample(x_start, ts, None if noise is None else noise.to(dev))
        model_output = self.denoise(x_t, users, ts, keeps)
        mse = self.mean_flat((x_start - model_output) ** 2)
        reloss = self.reweight_loss(mse, ts)
        self.update_Lt_history(ts, reloss)
        loss = (reloss / pt).mean()
        self.last = dict(ts=ts, reloss=reloss.detach(), x_t=x_t.detach(), model_output=model_output.detach())
        return loss

    def training_losses(self, x_start, x_sec_hop):
        """The reference's signature over dense rows (:411-442), in plain torch or with the fused attention."""
        ts, pt = self.sample_timesteps(x_start.size(0), x_start.device, 'importance')
        if self._state.is_cuda:         # the step the attention's device draws are keyed by (the plain route redraws them too)
            ops.step_tick(self._state)
        x_t = self.q_sample(x_start, ts, torch.randn_like(x_start))
        model_output = self.CAM_AE(x_t, x_sec_hop, ts)
        reloss = self.reweight_loss(self.mean_flat((x_start - model_output) ** 2), ts)
        self.update_Lt_history(ts, reloss)
        return (reloss / pt).mean()

    # ---- sampling (:313-377) -----------------------------------------------------------------------------------------------
    def p_sample(self, x_start, x_sec_hop=None, users=None):
        """sampling_steps = 0 and no sampling noise: x_t = x_start, then `steps` posterior-mean passes, t = steps - 1 .. 0.
        x_sec_hop dense, or None with `users`: the batch's second-hop rows from the CSR."""
        assert self.sampling_steps == 0 and not self.sampling_noise
        x_t = x_start
        h_sec = self.encode_sec_hop(users) if (x_sec_hop is None and self.fused) else None
        if x_sec_hop is None and h_sec is None:
            x_sec_hop = self.sec_hop_rows(users)
        for i in list(range(self.steps))[::-1]:
            t = torch.full((x_t.shape[0],), i, dtype=torch.int64, device=x_start.device)
            out = self.CAM_AE(x_t, x_sec_hop, t, h_sec_hop=h_sec)
            x_t = self.q_posterior_mean(out, x_t, t)
        return x_t

    def gene_ranklist(self, topk=50, to_cpu=True, batch_size=1024):
        """train_and_evaluate.py:614-650: per user batch the rows, p_sample in eval mode, history set to -inf, top-k, + num_user."""
        dev = torch.device(self.device)
        was_training = self.training
        self.eval()
        out = []
        with torch.no_grad():
            if self.fused:
                self._sec_table = ops.spmm(self._sec_csr, self.CAM_AE.encoder.weight.t().contiguous())
            for u0 in range(0, self.num_user, batch_size):
                users = torch.arange(u0, min(u0 + batch_size, self.num_user), dtype=torch.int64, device=dev)
                x = self.batch_rows(users)
                pred = self.p_sample(x, users=users).masked_fill(x > 0, -np.inf)
                if pred.is_cuda and self.fused:
                    out.append(ops.rows_topk(pred.contiguous(), topk, self.num_user)[0])
                else:
                    out.append(torch.topk(pred, topk, dim=1)[1] + self.num_user)
        self._sec_table = None
        self.train(was_training)
        rank = torch.cat(out, 0)
        return rank.cpu() if to_cpu else rank

    full_sort_predict = gene_ranklist
