"""DiffMM with the reference's surface (Model/DiffMM.py:19-670), its diffusion half on HIP kernels (csrc/diffmm.hip).

Same constructor, method names and the 19 state_dict names in the reference's order, drawn call for call (same torch seed
-> same weights): uEmbeds, iEmbeds, the two feature Linears (nn.Linear's own draw, then xavier_uniform_ on the weight),
modal_weight, then per denoiser nn.Linear's draws of emb_layer / in_layers / out_layers followed by init_weights' normal_
draws.  Denoise and GaussianDiffusion keep their lines; the diffusion tables are float64.

Kept as written, on purpose:
  * training_losses indexes SNR(ts - 1) BEFORE the where: ts = 0 reads index -1 (the last step's SNR) and discards it;
  * the weight SNR(ts - 1) - SNR(ts) is float64, so diff_loss is float64 and its mean is cast when the losses are added;
  * p_sample(steps = 0) starts from x_start itself and still walks all five indices 4 .. 0;
  * betas[0] is pinned to 1e-4 (beta_fixed);
  * the main optimizer holds the denoisers' parameters too and never sees a gradient for them (zero_grad sets it to None).

What changed underneath.  The graph half (forward_MM, forward_cl_MM) is nine SpMMs through sparse.mm.  The diffusion half:
no dense [U, I] interaction matrix exists; `diffusion_step(users)` writes the noised, dropped-out rows of a batch straight
from the history CSR in one launch (ops.diffmm_rows), runs the in-layer on the MFMA GEMMs with the time embedding as a
second, 10-wide product (no concatenation), and the out-layer, both losses and d loss / d out in one pass
(ops.diffmm_denoise_loss): model_output never exists.  `rebuild_graphs(loader)` runs the five posterior-mean steps per
batch on the device, takes the top-rebuild_k with chaorec_macrid_topk_f32 and restates buildUIMatrix / edgeDropper as tensor
operations on the device (the reference makes 2 U rebuild_k single-element host round trips and goes through scipy).
fused_denoise = False runs the reference's own lines in plain torch on the device (the measurements' other side).
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import graph, ops, ranking, sparse
from ..ops_dense import gemm_raw, gemm_tn_bf16x3, _linear_fwd_raw


class GCNLayer(nn.Module):
    def forward(self, adj, embeds):
        return sparse.mm(adj, embeds)


class SpAdjDropEdge(nn.Module):
    """Model/DiffMM.py:27-41 over a coalesced torch sparse tensor; rand: given uniforms [nnz] in its entry order."""

    def __init__(self, keepRate):
        super(SpAdjDropEdge, self).__init__()
        self.keepRate = keepRate

    def forward(self, adj, rand=None):
        vals, idxs = adj._values(), adj._indices()
        if rand is None:
            rand = torch.rand(vals.shape[0], device=vals.device)
        mask = (rand.to(vals.device) + self.keepRate).floor().type(torch.bool)
        return torch.sparse_coo_tensor(idxs[:, mask], vals[mask] / self.keepRate, adj.shape)


class _InLayer(torch.autograd.Function):
    """tanh(x_in W[:, :I]^T + emb W[:, I:]^T + b) (Denoise.forward :462-466 without the concatenation): x_in [B, I] carries no
    gradient; dW is written once, both column blocks into one [H, I + E] buffer."""

    @staticmethod
    def forward(ctx, x_in, emb, W, b):
        I = x_in.shape[1]
        pre = _linear_fwd_raw(x_in, W[:, :I], None, 0)
        gemm_raw(emb, W[:, I:], transB=True, bias=b, out=pre, accumulate=True)
        h = torch.tanh(pre)
        ctx.save_for_backward(x_in, emb, W, h)
        return h

    @staticmethod
    def backward(ctx, g):
        x_in, emb, W, h = ctx.saved_tensors
        I = x_in.shape[1]
        gpre = (g * (1.0 - h * h)).contiguous()
        dW = torch.empty_like(W)
        if ops.LINEAR_FORWARD == "bf16x3" and gpre.shape[0] >= 256:
            gemm_tn_bf16x3(gpre, x_in, out=dW[:, :I])
        else:
            dW[:, :I] = gemm_raw(gpre, x_in, transA=True)
        dW[:, I:] = gemm_raw(gpre, emb, transA=True)
        demb = gemm_raw(gpre, W[:, I:]) if ctx.needs_input_grad[1] else None
        return None, demb, dW, ops.col_sum(gpre)


class _ModalMix(torch.autograd.Function):
    """w[0] a + w[1] b (Model/DiffMM.py:248).  The two weight gradients are sums over a whole [U + I, D] table each, and the
    softmax in front of them keeps only their difference: they are summed in double."""

    @staticmethod
    def forward(ctx, w, a, b):
        ctx.save_for_backward(w, a, b)
        return w[0] * a + w[1] * b

    @staticmethod
    def backward(ctx, g):
        w, a, b = ctx.saved_tensors
        gd = g.double()
        gw = torch.stack([(gd * a.double()).sum(), (gd * b.double()).sum()]).to(w.dtype)
        return gw, w[0] * g, w[1] * g


class Denoise(nn.Module):
    def __init__(self, in_dims, out_dims, emb_size, norm=False, dropout=0.5):
        super(Denoise, self).__init__()
        self.in_dims = in_dims
        self.out_dims = out_dims
        self.time_emb_dim = emb_size
        self.norm = norm
        self.emb_layer = nn.Linear(self.time_emb_dim, self.time_emb_dim)
        in_dims_temp = [self.in_dims[0] + self.time_emb_dim] + self.in_dims[1:]
        out_dims_temp = self.out_dims
        self.in_layers = nn.ModuleList([nn.Linear(d_in, d_out) for d_in, d_out in zip(in_dims_temp[:-1], in_dims_temp[1:])])
        self.out_layers = nn.ModuleList([nn.Linear(d_in, d_out) for d_in, d_out in zip(out_dims_temp[:-1], out_dims_temp[1:])])
        self.drop = nn.Dropout(dropout)
        self.init_weights()

    def init_weights(self):
        for layer in list(self.in_layers) + list(self.out_layers) + [self.emb_layer]:
            size = layer.weight.size()
            std = np.sqrt(2.0 / (size[0] + size[1]))
            layer.weight.data.normal_(0.0, std)
            layer.bias.data.normal_(0.0, 0.001)

    def time_embedding(self, timesteps):
        """Model/DiffMM.py:440-451: [cos(t f) | sin(t f)], f_j = exp(-ln 1e4 j / half)."""
        half = self.time_emb_dim // 2
        freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half).to(timesteps.device)
        temp = timesteps[:, None].float() * freqs[None]
        time_emb = torch.cat([torch.cos(temp), torch.sin(temp)], dim=-1)
        if self.time_emb_dim % 2:
            time_emb = torch.cat([time_emb, torch.zeros_like(time_emb[:, :1])], dim=-1)
        return time_emb

    def forward(self, x, timesteps, mess_dropout=True, keep=None):
        """Model/DiffMM.py:437-473 in plain torch.  keep: given dropout flags of x's shape (parity tests)."""
        emb = self.emb_layer(self.time_embedding(timesteps))
        if self.norm:
            x = F.normalize(x)
        if mess_dropout:
            x = x * (keep.to(x.dtype) * 2.0) if keep is not None else self.drop(x)
        h = torch.cat([x, emb], dim=-1)
        for i, layer in enumerate(self.in_layers):
            h = torch.tanh(layer(h))
        for i, layer in enumerate(self.out_layers):
            h = layer(h)
            if i != len(self.out_layers) - 1:
                h = torch.tanh(h)
        return h

    def hidden(self, x_in, timesteps):
        """The in-layer on the HIP GEMMs: x_in [B, I] already noised and dropped out -> h [B, H]."""
        assert len(self.in_layers) == 1 and len(self.out_layers) == 1 and not self.norm
        emb = ops.linear(self.time_embedding(timesteps), self.emb_layer.weight, self.emb_layer.bias)
        return _InLayer.apply(x_in, emb, self.in_layers[0].weight, self.in_layers[0].bias)

    def denoise(self, x, timesteps):
        """forward(x, timesteps, False) on the HIP GEMMs, no tape (p_sample's model call)."""
        h = self.hidden(x, timesteps)
        return _linear_fwd_raw(h, self.out_layers[0].weight, self.out_layers[0].bias, 0)


class GaussianDiffusion(nn.Module):
    def __init__(self, noise_scale, noise_min, noise_max, steps, beta_fixed=True, device=None):
        super(GaussianDiffusion, self).__init__()
        self.noise_scale = noise_scale
        self.noise_min = noise_min
        self.noise_max = noise_max
        self.steps = steps
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        if noise_scale != 0:
            self.betas = torch.tensor(self.get_betas(), dtype=torch.float64).to(self.device)
            if beta_fixed:
                self.betas[0] = 0.0001
            self.calculate_for_diffusion()

    def get_betas(self):
        start = self.noise_scale * self.noise_min
        end = self.noise_scale * self.noise_max
        variance = np.linspace(start, end, self.steps, dtype=np.float64)
        alpha_bar = 1 - variance
        betas = [1 - alpha_bar[0]]
        for i in range(1, self.steps):
            betas.append(min(1 - alpha_bar[i] / alpha_bar[i - 1], 0.999))
        return np.array(betas)

    def calculate_for_diffusion(self):
        alphas = 1.0 - self.betas
        dev = self.betas.device
        self.alphas_cumprod = torch.cumprod(alphas, dim=0)
        self.alphas_cumprod_prev = torch.cat([torch.tensor([1.0]).to(dev), self.alphas_cumprod[:-1]])
        self.alphas_cumprod_next = torch.cat([self.alphas_cumprod[1:], torch.tensor([0.0]).to(dev)])
        self.sqrt_alphas_cumprod = torch.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = torch.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = torch.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = torch.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = torch.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = self.betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = torch.log(
            torch.cat([self.posterior_variance[1].unsqueeze(0), self.posterior_variance[1:]]))
        self.posterior_mean_coef1 = self.betas * torch.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * torch.sqrt(alphas) / (1.0 - self.alphas_cumprod)

    def p_sample(self, model, x_start, steps, sampling_noise=False):
        """Model/DiffMM.py:547-577.  model: a callable (x, t, mess_dropout)."""
        if steps == 0:
            x_t = x_start
        else:
            t = torch.tensor([steps - 1] * x_start.shape[0]).to(x_start.device)
            x_t = self.q_sample(x_start, t)
        for i in list(range(self.steps))[::-1]:
            t = torch.tensor([i] * x_t.shape[0]).to(x_t.device)
            model_mean, model_log_variance = self.p_mean_variance(model, x_t, t)
            if sampling_noise:
                noise = torch.randn_like(x_t)
                nonzero_mask = ((t != 0).float().view(-1, *([1] * (len(x_t.shape) - 1))))
                x_t = model_mean + nonzero_mask * torch.exp(0.5 * model_log_variance) * noise
            else:
                x_t = model_mean
        return x_t

    def q_sample(self, x_start, t, noise=None):
        if noise is None:
            noise = torch.randn_like(x_start)
        alpha_t = self._extract_into_tensor(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
        one_minus_alpha_t = self._extract_into_tensor(self.sqrt_one_minus_alphas_cumprod, t, x_start.shape) * noise
        return alpha_t + one_minus_alpha_t

    def _extract_into_tensor(self, arr, timesteps, broadcast_shape):
        res = arr.to(timesteps.device)[timesteps].float()
        while len(res.shape) < len(broadcast_shape):
            res = res[..., None]
        return res.expand(broadcast_shape)

    def p_mean_variance(self, model, x, t):
        model_output = model(x, t, False)
        model_log_variance = self._extract_into_tensor(self.posterior_log_variance_clipped, t, x.shape)
        model_mean = (self._extract_into_tensor(self.posterior_mean_coef1, t, x.shape) * model_output
                      + self._extract_into_tensor(self.posterior_mean_coef2, t, x.shape) * x)
        return model_mean, model_log_variance

    def weight(self, ts):
        """Model/DiffMM.py:644-646: float64; ts - 1 = -1 is read (the last step) and replaced."""
        weight = self.SNR(ts - 1) - self.SNR(ts)
        return torch.where((ts == 0), 1.0, weight)

    def training_losses(self, model, x_start, itmEmbeds, batch_index, model_feats, ts=None, noise=None, keep=None):
        """Model/DiffMM.py:624-660 in plain torch.  ts, noise, keep: given draws (parity tests)."""
        batch_size = x_start.size(0)
        if ts is None:
            ts = torch.randint(0, self.steps, (batch_size,), device=x_start.device).long()
        if noise is None:
            noise = torch.randn_like(x_start)
        x_t = self.q_sample(x_start, ts, noise) if self.noise_scale != 0 else x_start
        model_output = model(x_t, ts, True, keep) if keep is not None else model(x_t, ts)
        mse = self.mean_flat((x_start - model_output) ** 2)
        diff_loss = self.weight(ts) * mse
        usr_model_embeds = torch.mm(model_output, model_feats)
        usr_id_embeds = torch.mm(x_start, itmEmbeds)
        gc_loss = self.mean_flat((usr_model_embeds - usr_id_embeds) ** 2)
        return diff_loss, gc_loss

    def mean_flat(self, tensor):
        return tensor.mean(dim=list(range(1, len(tensor.shape))))

    def SNR(self, t):
        ac = self.alphas_cumprod.to(t.device)
        return ac[t] / (1 - ac[t])


class DiffMM(nn.Module):
    fused_denoise = True        # False: the reference's training_losses / Denoise.forward lines in plain torch

    def __init__(self, num_user, num_item, edge_index, user_item_dict, v_feat, t_feat, dim_E,
                 reg_weight, n_layers, ssl_alpha, ssl_temp, ris_lambda, e_loss, rebuild_k, device):
        super(DiffMM, self).__init__()
        self.restore_itmEmbeds = None
        self.restore_usrEmbeds = None
        self.num_user = num_user
        self.num_item = num_item
        self.edge_index = edge_index
        self.user_item_dict = user_item_dict
        self.dim_E = dim_E
        self.reg_weight = reg_weight
        self.device = device
        self.ris_adj_lambda = 0.2
        self.ris_lambda = ris_lambda
        self.steps = 5
        self.noise_scale = 0.1
        self.noise_min = 0.0001
        self.noise_max = 0.02
        self.trans = 1
        self.ssl_temp = ssl_temp
        self.ssl_alpha = ssl_alpha
        self.cl_method = 0
        self.n_layers = n_layers
        self.e_loss = e_loss
        self.rebuild_k = rebuild_k

        self.uEmbeds = nn.Parameter(nn.init.xavier_uniform_(torch.empty(num_user, dim_E)))
        self.iEmbeds = nn.Parameter(nn.init.xavier_uniform_(torch.empty(num_item, dim_E)))
        self.gcnLayers = nn.Sequential(*[GCNLayer() for i in range(n_layers)])

        e = np.asarray(edge_index)
        self.adj = self.get_norm_adj_mat(e).to(device)
        self.edgeDropper = SpAdjDropEdge(0.5)

        v_feat = torch.as_tensor(v_feat).clone().detach().float()
        t_feat = torch.as_tensor(t_feat).clone().detach().float()
        self.image_trans_l = nn.Linear(v_feat.shape[1], self.dim_E)
        self.text_trans_l = nn.Linear(t_feat.shape[1], self.dim_E)
        nn.init.xavier_uniform_(self.image_trans_l.weight)
        nn.init.xavier_uniform_(self.text_trans_l.weight)
        self.image_embedding = v_feat.to(device)
        self.text_embedding = t_feat.to(device)
        self.modal_weight = nn.Parameter(torch.Tensor([0.5, 0.5]))
        self.softmax = nn.Softmax(dim=0)
        self.dropout = nn.Dropout(p=0.1)
        self.leakyrelu = nn.LeakyReLU(0.2)

        out_dims = [1000, num_item]
        in_dims = out_dims[::-1]
        self.denoise_model_image = Denoise(in_dims, out_dims, 10, norm=False).to(device)
        self.denoise_model_text = Denoise(in_dims, out_dims, 10, norm=False).to(device)
        self.diffusion_model = GaussianDiffusion(self.noise_scale, self.noise_min, self.noise_max, self.steps, device=device)

        rowptr, col = graph.user_hist_csr_from_edges(e, num_user)
        self.hist = (rowptr.to(device), col.to(device))
        self._hist_csr = graph.CSR(self.hist[0], self.hist[1], torch.ones(col.numel(), dtype=torch.float32, device=device),
                                   num_user, num_item)
        self.seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self._step = 0
        self.last = {}
        self.to(device)

    def get_norm_adj_mat(self, e):
        """Model/DiffMM.py:116-156: binary A, degree + 1e-7, D^-1/2 A D^-1/2 in fp64, stored fp32 -> a coalesced graph.CSR."""
        return graph.binary_sym_norm_csr(torch.from_numpy(e[:, 0].astype(np.int64)), torch.from_numpy(e[:, 1].astype(np.int64)) - self.num_user,
                                         self.num_user, self.num_item)

    def buildUIMatrix(self, u_list, i_list, edge_list=None):
        """Model/DiffMM.py:159-180 as tensor operations on the lists' device: the distinct (u, i) pairs in both directions plus
        the unit diagonal, every entry d_r^-1/2 d_c^-1/2 with d = row sums, evaluated in fp64 and stored fp32.  -> a coalesced
        torch sparse tensor [U + I, U + I] (row-major entry order)."""
        U, I = self.num_user, self.num_item
        N = U + I
        u, i = torch.as_tensor(u_list).long(), torch.as_tensor(i_list).long()
        dev = u.device
        key = torch.unique(u * I + i)
        u, i = torch.div(key, I, rounding_mode="floor"), key % I
        loop = torch.arange(N, dtype=torch.int64, device=dev)
        row, col = torch.cat([u, U + i, loop]), torch.cat([U + i, u, loop])
        deg = torch.bincount(row, minlength=N).to(torch.float64)
        d = deg.pow(-0.5)
        d[torch.isinf(d)] = 0.0
        val = ((1.0 * d[row]) * d[col]).to(torch.float32)
        return torch.sparse_coo_tensor(torch.stack([row, col]), val, (N, N)).coalesce()

    def getItemEmbeds(self):
        return self.iEmbeds

    def getUserEmbeds(self):
        return self.uEmbeds

    def getImageFeats(self):
        return ops.linear(self.image_embedding, self.image_trans_l.weight, self.image_trans_l.bias)

    def getTextFeats(self):
        return ops.linear(self.text_embedding, self.text_trans_l.weight, self.text_trans_l.bias)

    def forward_MM(self, image_adj, text_adj):
        """Model/DiffMM.py:204-262."""
        image_feats, text_feats = self.getImageFeats(), self.getTextFeats()
        weight = self.softmax(self.modal_weight)
        ego = torch.concat([self.uEmbeds, self.iEmbeds])
        embedsImageAdj = sparse.mm(image_adj, ego)
        embedsImage = sparse.mm(self.adj, torch.concat([self.uEmbeds, F.normalize(image_feats)]))
        embedsImage_ = sparse.mm(self.adj, torch.concat([embedsImage[:self.num_user], self.iEmbeds]))
        embedsImage = embedsImage + embedsImage_
        embedsTextAdj = sparse.mm(text_adj, ego)
        embedsText = sparse.mm(self.adj, torch.concat([self.uEmbeds, F.normalize(text_feats)]))
        embedsText_ = sparse.mm(self.adj, torch.concat([embedsText[:self.num_user], self.iEmbeds]))
        embedsText = embedsText + embedsText_
        embedsImage = embedsImage + self.ris_adj_lambda * embedsImageAdj
        embedsText = embedsText + self.ris_adj_lambda * embedsTextAdj
        embedsModal = _ModalMix.apply(weight, embedsImage, embedsText)
        embedsLst = [embedsModal]
        for gcn in self.gcnLayers:
            embedsLst.append(gcn(self.adj, embedsLst[-1]))
        embeds = sum(embedsLst)
        embeds = embeds + self.ris_lambda * F.normalize(embedsModal)
        return embeds[:self.num_user], embeds[self.num_user:]

    def forward_cl_MM(self, image_adj, text_adj):
        """Model/DiffMM.py:264-298."""
        image_feats, text_feats = self.getImageFeats(), self.getTextFeats()
        embedsImage = sparse.mm(image_adj, torch.concat([self.uEmbeds, F.normalize(image_feats)]))
        embedsText = sparse.mm(text_adj, torch.concat([self.uEmbeds, F.normalize(text_feats)]))
        out = []
        for first in (embedsImage, embedsText):
            lst = [first]
            for gcn in self.gcnLayers:
                lst.append(gcn(self.adj, lst[-1]))
            out.append(sum(lst))
        return out[0][:self.num_user], out[0][self.num_user:], out[1][:self.num_user], out[1][self.num_user:]

    def bpr_loss(self, users, pos_items, neg_items, user_emb, item_emb):
        user_embeddings = user_emb[users]
        pos_scores = torch.sum(user_embeddings * item_emb[pos_items], dim=1)
        neg_scores = torch.sum(user_embeddings * item_emb[neg_items], dim=1)
        return -torch.mean(torch.log(torch.sigmoid(pos_scores - neg_scores) + 1e-5))

    def regularization_loss(self, users, pos_items, neg_items, u_g, i_g):
        return self.reg_weight * (torch.mean(u_g[users] ** 2) + torch.mean(i_g[pos_items] ** 2) + torch.mean(i_g[neg_items] ** 2))

    def loss(self, users, pos_items, neg_items, image_adj, text_adj):
        """Model/DiffMM.py:325-352.  image_adj / text_adj: what rebuild_graphs returned (graph.CSR or torch sparse)."""
        pos_items = pos_items - self.num_user
        neg_items = neg_items - self.num_user
        users, pos_items, neg_items = users.to(self.device), pos_items.to(self.device), neg_items.to(self.device)
        usrEmbeds, itmEmbeds = self.forward_MM(image_adj, text_adj)
        self.restore_usrEmbeds = usrEmbeds
        self.restore_itmEmbeds = itmEmbeds
        bpr_loss = self.bpr_loss(users, pos_items, neg_items, usrEmbeds, itmEmbeds)
        reg_loss = self.regularization_loss(users, pos_items, neg_items, usrEmbeds, itmEmbeds)
        usrEmbeds1, itmEmbeds1, usrEmbeds2, itmEmbeds2 = self.forward_cl_MM(image_adj, text_adj)
        clLoss = (self.contrastLoss(usrEmbeds1, usrEmbeds2, users, self.ssl_temp) +
                  self.contrastLoss(itmEmbeds1, itmEmbeds2, pos_items, self.ssl_temp)) * self.ssl_alpha
        if self.cl_method == 1:
            clLoss1 = (self.contrastLoss(usrEmbeds, usrEmbeds1, users, self.ssl_temp) +
                       self.contrastLoss(itmEmbeds, itmEmbeds1, pos_items, self.ssl_temp)) * self.ssl_alpha
            clLoss2 = (self.contrastLoss(usrEmbeds, usrEmbeds2, users, self.ssl_temp) +
                       self.contrastLoss(itmEmbeds, itmEmbeds2, pos_items, self.ssl_temp)) * self.ssl_alpha
            clLoss = clLoss1 + clLoss2
        return bpr_loss + reg_loss + clLoss

    def contrastLoss(self, embeds1, embeds2, nodes, temp):
        embeds1 = F.normalize(embeds1, p=2)
        embeds2 = F.normalize(embeds2, p=2)
        pckEmbeds1 = embeds1[nodes]
        pckEmbeds2 = embeds2[nodes]
        nume = torch.exp(torch.sum(pckEmbeds1 * pckEmbeds2, dim=-1) / temp)
        deno = torch.exp(pckEmbeds1 @ embeds2.T / temp).sum(-1)
        return -torch.log(nume / deno).mean()

    def gene_ranklist(self, topk=50, to_cpu=True):
        """Model/DiffMM.py:363-388: scores of the last loss()'s embeddings, history entries = 1e-6, top-k, + num_user."""
        result = torch.cat((self.restore_usrEmbeds[:self.num_user], self.restore_itmEmbeds[:self.num_item]), 0).detach()
        return ranking.gene_ranklist(result, self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                     state=ranking.state_of(self))

    full_sort_predict = gene_ranklist

    # ---- the diffusion half ------------------------------------------------------------------------------------------
    def batch_rows(self, users):
        """The multi-hot rows [B, I] of a batch of users, from the history CSR (dataload.DiffusionData's rows; no [U, I])."""
        if self.hist[0].is_cuda:
            return ops.diffmm_rows(users, self.hist[0], self.hist[1], self.num_item, plain=True)[0]
        rowptr, col = self.hist
        n = rowptr[users + 1] - rowptr[users]
        rows = torch.repeat_interleave(torch.arange(users.numel(), device=users.device), n)
        pos = torch.arange(int(n.sum()), device=users.device) - torch.repeat_interleave(torch.cumsum(n, 0) - n, n)
        x = torch.zeros((users.numel(), self.num_item), dtype=torch.float32, device=users.device)
        x[rows, col[rowptr[users][rows] + pos].long()] = 1.0
        return x

    def diffusion_step(self, users, ts=None, noise=None, keep=None):
        """One batch of train_and_evaluate.py:147-172, image first -> (loss_image, loss_text), each
        diff_loss.mean() + gc_loss.mean() * e_loss with gradient into its denoiser only (iEmbeds and the projected features
        are detached).  ts, noise, keep: pairs (image, text) of given draws -- int64 [B], fp32 [B, I], flags [B, I]."""
        users = users.to(self.device).to(torch.int64)
        B, I, dm = users.numel(), self.num_item, self.diffusion_model
        iEmbeds = self.getItemEmbeds().detach()
        feats = (self.getImageFeats().detach(), self.getTextFeats().detach())
        fused = self.fused_denoise and int(self.dim_E) == ops.DIFFMM_D
        self._step += 1
        if fused:
            x0E = ops.spmm_raw(self._hist_csr, iEmbeds.contiguous())[users].contiguous()
        else:
            x0 = self.batch_rows(users)
        losses, last = [], {}
        for m, (dn, feat) in enumerate(zip((self.denoise_model_image, self.denoise_model_text), feats)):
            t = ts[m].to(self.device).long() if ts is not None else torch.randint(0, dm.steps, (B,), device=self.device).long()
            n_m = noise[m].to(self.device) if noise is not None else None
            k_m = keep[m].to(self.device) if keep is not None else None
            if fused:
                a = dm.sqrt_alphas_cumprod[t].float().contiguous()
                s = dm.sqrt_one_minus_alphas_cumprod[t].float().contiguous()
                x_in, bits = ops.diffmm_rows(users, self.hist[0], self.hist[1], I, a, s, n_m, k_m, self.seed, self._step, salt=m)
                h = dn.hidden(x_in, t)
                out = dn.out_layers[0]
                loss, diff_rows, gc_rows = ops.diffmm_denoise_loss(h, out.weight, out.bias, bits, x0E, feat.contiguous(),
                                                                         dm.weight(t), self.e_loss)
                loss = loss.reshape(())
            else:
                diff_rows, gc_rows = dm.training_losses(dn, x0, iEmbeds, users, feat, ts=t, noise=n_m, keep=k_m)
                loss = diff_rows.mean() + gc_rows.mean() * self.e_loss
            losses.append(loss)
            last[("image", "text")[m]] = dict(diff_loss=diff_rows.detach(), gc_loss=gc_rows.detach(), ts=t)
        self.last = last
        return losses[0], losses[1]

    def denoised_topk(self, dn, users):
        """train_and_evaluate.py:200-202: p_sample(steps = 0, no sampling noise) of a batch's rows, then top-rebuild_k ->
        (int64 [B, k] local item ids, the denoised rows)."""
        dm = self.diffusion_model
        x = self.batch_rows(users)
        if self.fused_denoise and x.is_cuda:
            x_t = dm.p_sample(lambda xx, t, _drop: dn.denoise(xx, t), x, 0, False).contiguous()
            return ops.rows_topk(x_t, self.rebuild_k)[0], x_t
        x_t = dm.p_sample(dn, x, 0, False)
        return torch.topk(x_t, k=self.rebuild_k)[1], x_t

    def rebuild_graphs(self, loader, rand=None, as_csr=True):
        """train_and_evaluate.py:183-235 without a host round trip per element: per batch the five posterior-mean steps and the
        top-rebuild_k on the device, the edges gathered there, buildUIMatrix and edgeDropper as tensor operations.
        loader: an iterable of user-id batches.  rand: a pair of given uniforms for the two edge drops (in the entry order
        of buildUIMatrix's result).  -> (image_adj, text_adj) as graph.CSR (as_csr) or torch sparse tensors."""
        out = []
        with torch.no_grad():
            lists = ([], [])
            for users in loader:
                users = users.to(self.device).to(torch.int64)
                for m, dn in enumerate((self.denoise_model_image, self.denoise_model_text)):
                    idx = self.denoised_topk(dn, users)[0]
                    lists[m].append((users[:, None].expand_as(idx).reshape(-1), idx.reshape(-1)))
            for m in range(2):
                u = torch.cat([a for a, _ in lists[m]])
                i = torch.cat([b for _, b in lists[m]])
                adj = self.edgeDropper(self.buildUIMatrix(u, i), None if rand is None else rand[m])
                out.append(sparse.from_torch_sparse(adj) if as_csr else adj)
        return out[0], out[1]
