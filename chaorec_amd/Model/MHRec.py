"""MHRec with the reference's surface (Model/MHRec.py:23-891), its hypergraph attention layer on HIP kernels (csrc/mhrec.hip).

Same constructor arguments, method names and the reference's state_dict names in its order -- modal_weight, the two feature
tables and their Linears, the four embedding tables, per hypergraph layer `a` and the unused `W.weight`, the two denoisers --
created in its order (same torch seed -> same weights).  Denoise and GaussianDiffusion are Model/DiffMM.py's (the same
arithmetic; here d_emb_size 10, norm False, steps 20, noise_scale 0.1).

Kept as written, on purpose:
  * F.dropout(., 0.5) after every hypergraph layer is the functional default: active in eval mode too;
  * every hypergraph layer's `W` is created, initialised and never used;
  * gene_ranklist scores the LAST forward's table (self.result), dropout included;
  * p_sample(steps = 5, no sampling noise) still draws the q_sample noise and walks all 20 steps;
  * the diffusion loaders of BOTH modalities read the visual hyperedges (main.py:227-228), see diffusion_tables().

Departure: a denoiser's training step (not the rebuild's p_sample) is evaluated in float64 on the fp32 weights by default
(`diffusion_double`): its weight gradients cancel about 1000 : 1 over the batch and Adam normalises the remainder.

What changed underneath.  A rebuilt hypergraph is an ops.HyperGraph (an ELL table of the top-k nodes and the node CSR,
built on the device), never a torch sparse tensor; a hypergraph layer with the residual and the dropout after it is ONE
autograd node (ops.mhrec_hyper_layer); fused_hyper = False runs the reference's lines in plain torch on the same
HyperGraph.  The input hyperedges ([u] + similar users + [i] + similar items per interaction) are an int32 [E, width] table
in HBM, read from hyperedges_*_u{}_i{}.npy under `MHRec.data_dir` or built on the device from the user co-occurrence graph
and the item kNN; the dense [E, N] matrix of the reference's HyperDiffusionData is never formed: `diffusion_rows(batch)`
scatter-adds a batch's rows (a hyperedge may name a node twice -- padded neighbours, the [0] * k placeholder -- and the
reference's coo.toarray() sums those: the rows hold counts).  gcnLayers go through sparse.mm; the four contrastLoss
denominators through ops.graphaug_lse, the + 1e-8 added afterwards.  `feed_draws` queues GIVEN dropout masks (parity
tests, the diffusion half's draws too), consumed in call order; without them the fused layer draws in its launch, keyed by a device-resident step counter.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import graph, ops, ranking, sparse
from .DiffMM import Denoise, GaussianDiffusion, _ModalMix


class GCNLayer(nn.Module):
    def __init__(self, device=None):
        super(GCNLayer, self).__init__()
        self.device = device

    def forward(self, adj, embeds, flag=True):
        return sparse.mm(adj, embeds)


class HypergraphAttentionLayer(nn.Module):
    def __init__(self, in_dim, out_dim):
        super(HypergraphAttentionLayer, self).__init__()
        self.in_dim = in_dim
        self.out_dim = out_dim
        self.W = nn.Linear(in_dim, out_dim, bias=False)        # (Model/MHRec.py:43, :56: created, never applied)
        self.a = nn.Parameter(torch.Tensor(2 * out_dim, 1))
        self.leakyrelu = nn.LeakyReLU(0.2)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.W.weight)
        nn.init.xavier_uniform_(self.a)

    def forward(self, H, X, fused=True, keep=None, state=None, seed=0, salt=0):
        """Model/MHRec.py:53-89 over an ops.HyperGraph, WITH the two lines the model puts after it (:725-726):
        -> dropout_0.5(layer(H, X) + X)."""
        if fused:
            return ops.mhrec_hyper_layer(H, X, self.a, keep, state, seed, salt, True)
        return ops.mhrec_hyper_layer_torch(H, X, self.a, keep, True)


class MHRec(nn.Module):
    fused_hyper = True        # False: the hypergraph layer's lines in plain torch over gathered [nnz, 128] rows
    fused_contrast = True     # False: contrastLoss's [B, M] matrix in plain torch
    diffusion_double = True   # the denoisers' TRAINING step evaluated in float64 (see _denoise_double); False: the reference's fp32 lines
    data_dir = None           # Data/<dataset> (main.py sets it): user_graph_dict.npy and the hyperedge files are looked up there

    def __init__(self, num_user, num_item, edge_index, user_item_dict, v_feat, t_feat, dim_E, reg_weight, ii_topk,
                 uu_topk, num_hypernodes, n_layers, h_layers, ssl_temp, ssl_alpha, beta1, beta2, device):
        super(MHRec, self).__init__()
        self.num_user = num_user
        self.num_item = num_item
        self.edge_index = edge_index
        self.user_item_dict = user_item_dict
        self.dim_E = dim_E
        self.reg_weight = reg_weight
        self.device = device
        self.item_topk = ii_topk
        self.user_topk = uu_topk
        self.hyperedges_visual = None
        self.hyperedges_textual = None
        self.n_layers = n_layers
        self.h_layers = h_layers
        self.num_hypernodes = num_hypernodes
        self.beta1 = beta1
        self.beta2 = beta2
        self.steps = 20
        self.noise_scale = 0.1
        self.noise_min = 0.0001
        self.noise_max = 0.02
        self.ssl_temp = ssl_temp
        self.ssl_alpha = ssl_alpha

        self.v_feat = torch.as_tensor(v_feat).clone().detach().float().to(self.device)
        self.t_feat = torch.as_tensor(t_feat).clone().detach().float().to(self.device)
        self.image_embedding = nn.Embedding.from_pretrained(self.v_feat, freeze=False)
        self.image_trs = nn.Linear(self.v_feat.shape[1], self.dim_E)
        self.text_embedding = nn.Embedding.from_pretrained(self.t_feat, freeze=False)
        self.text_trs = nn.Linear(self.t_feat.shape[1], self.dim_E)
        nn.init.xavier_uniform_(self.image_trs.weight)
        nn.init.xavier_uniform_(self.text_trs.weight)

        self.modal_weight = nn.Parameter(torch.Tensor([0.5, 0.5]))
        self.softmax = nn.Softmax(dim=0)

        self.user_embedding = nn.Embedding(self.num_user, self.dim_E)
        nn.init.xavier_normal_(self.user_embedding.weight)
        self.user_visual_embedding = nn.Embedding(self.num_user, self.dim_E)
        nn.init.xavier_normal_(self.user_visual_embedding.weight)
        self.user_textual_embedding = nn.Embedding(self.num_user, self.dim_E)
        nn.init.xavier_normal_(self.user_textual_embedding.weight)
        self.item_embedding = nn.Embedding(self.num_item, self.dim_E)
        nn.init.xavier_normal_(self.item_embedding.weight)

        self.gcnLayers = nn.Sequential(*[GCNLayer(self.device) for i in range(self.n_layers)])
        self.hypergraphLayersVisual = nn.Sequential(
            *[HypergraphAttentionLayer(self.dim_E, self.dim_E) for _ in range(self.h_layers)])
        self.hypergraphLayersTextual = nn.Sequential(
            *[HypergraphAttentionLayer(self.dim_E, self.dim_E) for _ in range(self.h_layers)])

        e = np.asarray(edge_index)
        self.adj = self.get_norm_adj_mat(e).to(self.device)
        self.hist = ranking.history_csr(user_item_dict, num_user, device)
        self.seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF

        out_dims = [1000, num_user + num_item]
        in_dims = out_dims[::-1]
        self.denoise_model_image = Denoise(in_dims, out_dims, 10, norm=False).to(self.device)
        self.denoise_model_text = Denoise(in_dims, out_dims, 10, norm=False).to(self.device)
        self.image_diffusion_model = GaussianDiffusion(self.noise_scale, self.noise_min, self.noise_max, self.steps, device=device)
        self.text_diffusion_model = GaussianDiffusion(self.noise_scale, self.noise_min, self.noise_max, self.steps, device=device)

        self._state = torch.zeros(2, dtype=torch.int64, device=device)      # steps taken, the count the draws in flight are keyed by
        self._draws = {"keep": [], "ts": [], "noise": [], "denoise_keep": [], "rebuild_noise": []}
        self.result = None
        self.to(device)

    def get_norm_adj_mat(self, e):
        """Model/MHRec.py:469-497: binary A, degree + 1e-7, D^-1/2 A D^-1/2 in fp64, stored fp32 -> a coalesced graph.CSR."""
        return graph.binary_sym_norm_csr(torch.from_numpy(e[:, 0].astype(np.int64)), torch.from_numpy(e[:, 1].astype(np.int64)) - self.num_user,
                                         self.num_user, self.num_item)

    # ---- the input hyperedges (pre_processing, Model/MHRec.py:575-640) ---------------------------------------------------------
    def _file(self, name):
        d = type(self).data_dir
        return os.path.join(d, name) if d else None

    def get_knn_adj_mat(self, mm_embeddings):
        """Model/MHRec.py:671-678: the item_topk most cosine-similar OTHER items -> int64 [I, item_topk] on the device (scoring
        and top-K are one kernel; the row itself is taken out of item_topk + 1 candidates)."""
        emb = mm_embeddings.to(self.device)
        context_norm = emb.div(torch.norm(emb, p=2, dim=-1, keepdim=True))
        d = context_norm.shape[1]
        d_pad = next(c for c in (8, 16, 32, 64, 128) if c >= d) if d <= 128 else (d + 63) // 64 * 64
        context_norm = F.pad(context_norm, (0, d_pad - d)).contiguous()
        knn_ind, _ = ops.score_topk(context_norm, context_norm, None, 0.0, self.item_topk + 1)
        knn_ind = knn_ind.to(torch.int64)
        own = knn_ind == torch.arange(knn_ind.shape[0], device=knn_ind.device)[:, None]
        order = torch.argsort(own.to(torch.int8), dim=1, stable=True)      # the others first, in score order
        return torch.gather(knn_ind, 1, order)[:, :self.item_topk]

    def topk_sample(self, k):
        """Model/MHRec.py:645-669 -> int32 [U, k] on the device: a user's first k co-occurring users, a shorter list padded with
        repeats of its own members, [0] * k for a user without any (ops.usergraph_sample, one launch)."""
        path = self._file('user_graph_dict.npy')
        if path and os.path.exists(path):
            s = ops.UserGraphStructure.from_dict(np.load(path, allow_pickle=True).item(), self.num_user, device=self.device)
        else:
            rowptr, col = self.hist
            s = ops.usergraph_build(rowptr.to(torch.int64).contiguous(), col.to(torch.int32).contiguous(), self.num_item)
        return ops.usergraph_sample(s, k, self.seed, 0)[0]

    def pre_processing(self):
        """The two int32 [E, 2 + uu_topk + ii_topk] tables, one row per training interaction: read from the reference's files
        where both exist, otherwise built on the device."""
        names = ['hyperedges_{}_u{}_i{}.npy'.format(m, self.user_topk, self.item_topk) for m in ("visual", "textual")]
        paths = [self._file(n) for n in names]
        if all(p and os.path.exists(p) for p in paths):
            tables = [torch.from_numpy(np.asarray(np.load(p, allow_pickle=True).tolist(), dtype=np.int32)) for p in paths]
        else:
            e = torch.as_tensor(np.asarray(self.edge_index)).to(self.device).to(torch.int64)
            u, i = e[:, 0], e[:, 1]
            uu = self.topk_sample(self.user_topk).to(torch.int64)[u]
            tables = []
            for emb in (self.image_embedding.weight.detach(), self.text_embedding.weight.detach()):
                ii = self.get_knn_adj_mat(emb)[i - self.num_user] + self.num_user
                tables.append(torch.cat([u[:, None], uu, i[:, None], ii], 1).to(torch.int32))
        self.set_input_hyperedges(*tables)

    def set_input_hyperedges(self, visual, textual):
        """Install GIVEN input hyperedge tables (integer [E, width])."""
        self.hyperedges_visual = torch.as_tensor(np.asarray(visual) if not torch.is_tensor(visual) else visual).to(torch.int32).to(self.device).contiguous()
        self.hyperedges_textual = torch.as_tensor(np.asarray(textual) if not torch.is_tensor(textual) else textual).to(torch.int32).to(self.device).contiguous()

    def diffusion_tables(self):
        """(visual loader's table, textual loader's table).  The reference loads the VISUAL file for both (main.py:227-228:
        `hyperedges_textual = np.load(visual_file_path ...)`); kept."""
        if self.hyperedges_visual is None:
            self.pre_processing()
        return self.hyperedges_visual, self.hyperedges_visual

    def diffusion_rows(self, batch, modality=0):
        """The dense rows [B, U + I] of a batch of input hyperedges (dataload.HyperDiffusionData's rows): counts, a node named
        twice holds 2."""
        table = self.diffusion_tables()[modality]
        idx = table[batch.to(self.device).long()].long()
        x = torch.zeros((idx.shape[0], self.num_user + self.num_item), dtype=torch.float32, device=self.device)
        return x.scatter_add_(1, idx, torch.ones(idx.shape, dtype=torch.float32, device=self.device))

    # ---- getters ---------------------------------------------------------------------------------------------------------------
    def getItemEmbeds(self):
        return self.item_embedding.weight

    def getUserEmbeds(self):
        return self.user_embedding.weight

    def getUserEmbeds_visual(self):
        return self.user_visual_embedding.weight

    def getUserEmbeds_textual(self):
        return self.user_textual_embedding.weight

    def getImageFeats(self):
        return ops.linear(self.image_embedding.weight, self.image_trs.weight, self.image_trs.bias)

    def getTextFeats(self):
        return ops.linear(self.text_embedding.weight, self.text_trs.weight, self.text_trs.bias)

    # ---- draws -----------------------------------------------------------------------------------------------------------------
    def feed_draws(self, keep=(), ts=(), noise=(), denoise_keep=(), rebuild_noise=()):
        """Queue GIVEN draws, consumed in call order.  keep: dropout masks [U + I, dim_E], per forward() the visual layers', then
        the textual layers'.  ts / noise / denoise_keep: per diffusion_step() its time steps [B], noise and the denoiser's dropout
        flags [B, U + I].  rebuild_noise: per denoised_topk() its q_sample noise [B, U + I]."""
        for kind, given in (("keep", keep), ("ts", ts), ("noise", noise), ("denoise_keep", denoise_keep), ("rebuild_noise", rebuild_noise)):
            self._draws[kind] += [torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).to(self.device) for t in given]

    def _take(self, kind):
        q = self._draws[kind]
        return q.pop(0) if q else None

    # ---- forward ---------------------------------------------------------------------------------------------------------------
    def _hyper_branch(self, layers, H, first, fused, salt0):
        lst = [first]
        for l, layer in enumerate(layers):
            lst.append(layer(H, lst[-1], fused, self._take("keep"), self._state, self.seed, salt0 + l))
        return torch.mean(torch.stack(lst), dim=0)

    def _gcn_branch(self, first):
        lst = [first]
        for gcn in self.gcnLayers:
            lst.append(gcn(self.adj, lst[-1]))
        return torch.mean(torch.stack(lst), dim=0)

    def forward(self):
        """Model/MHRec.py:708-779 over self.G_visual / self.G_textual (ops.HyperGraph)."""
        fused = bool(self.fused_hyper)
        if fused:
            ops.mhrec_check_shape(self.dim_E)
            if not self._draws["keep"]:
                ops.step_tick(self._state)
        v_embedding = self.getImageFeats()
        t_embedding = self.getTextFeats()
        weight = self.softmax(self.modal_weight)

        firstImage = torch.cat([self.user_visual_embedding.weight, F.normalize(v_embedding)], dim=0)
        embedsImage = self._hyper_branch(self.hypergraphLayersVisual, self.G_visual, firstImage, fused, 0)
        embedsImage = embedsImage + self.beta1 * self._gcn_branch(firstImage)

        firstText = torch.cat([self.user_textual_embedding.weight, F.normalize(t_embedding)], dim=0)
        embedsText = self._hyper_branch(self.hypergraphLayersTextual, self.G_textual, firstText, fused, self.h_layers)
        embedsText = embedsText + self.beta1 * self._gcn_branch(firstText)

        embedsModal = _ModalMix.apply(weight, embedsImage, embedsText)
        embeds = self._gcn_branch(torch.concat([self.user_embedding.weight, self.item_embedding.weight]))
        all_embs = embeds + self.beta2 * F.normalize(embedsModal)
        self.result = all_embs
        return all_embs[:self.num_user], all_embs[self.num_user:], embedsImage, embedsText, embeds

    def contrastLoss(self, embeds1, embeds2, nodes):
        """Model/MHRec.py:781-788: batch rows of view 1 against the WHOLE normalised table of view 2, no max-subtraction, + 1e-8."""
        embeds1 = F.normalize(embeds1, p=2)
        embeds2 = F.normalize(embeds2, p=2)
        pckEmbeds1 = embeds1[nodes]
        pckEmbeds2 = embeds2[nodes]
        if self.fused_contrast and int(self.dim_E) == ops.GRAPHAUG_DIM and pckEmbeds1.is_cuda:
            pos = torch.sum(pckEmbeds1 * pckEmbeds2, dim=-1) / self.ssl_temp
            deno = torch.exp(ops.graphaug_lse(pckEmbeds1, embeds2, 1.0 / self.ssl_temp)) + 1e-8
            return (torch.log(deno) - pos).mean()
        nume = torch.exp(torch.sum(pckEmbeds1 * pckEmbeds2, dim=-1) / self.ssl_temp)
        deno = torch.exp(pckEmbeds1 @ embeds2.T / self.ssl_temp).sum(-1) + 1e-8
        return -torch.log(nume / deno).mean()

    def bpr_loss(self, users, pos_items, neg_items, user_emb, item_emb):
        user_embeddings = user_emb[users]
        pos_scores = torch.sum(user_embeddings * item_emb[pos_items], dim=1)
        neg_scores = torch.sum(user_embeddings * item_emb[neg_items], dim=1)
        return -torch.mean(torch.log(torch.sigmoid(pos_scores - neg_scores) + 1e-5))

    def regularization_loss(self, users, pos_items, neg_items, u_g, i_g):
        user_initial_embeddings = torch.cat([self.user_embedding.weight[users], self.user_visual_embedding.weight[users],
                                             self.user_textual_embedding.weight[users]], dim=1)
        pos_item_initial_embeddings = torch.cat([self.item_embedding.weight[pos_items],
                                                 ops.linear(self.image_embedding.weight[pos_items], self.image_trs.weight, self.image_trs.bias),
                                                 ops.linear(self.text_embedding.weight[pos_items], self.text_trs.weight, self.text_trs.bias)], dim=1)
        neg_item_initial_embeddings = torch.cat([self.item_embedding.weight[neg_items],
                                                 ops.linear(self.image_embedding.weight[neg_items], self.image_trs.weight, self.image_trs.bias),
                                                 ops.linear(self.text_embedding.weight[neg_items], self.text_trs.weight, self.text_trs.bias)], dim=1)
        return self.reg_weight * (
            torch.mean(u_g[users] ** 2) + torch.mean(i_g[pos_items] ** 2) + torch.mean(i_g[neg_items] ** 2) +
            torch.mean(user_initial_embeddings ** 2) + torch.mean(pos_item_initial_embeddings ** 2) +
            torch.mean(neg_item_initial_embeddings ** 2))

    def loss(self, users, pos_items, neg_items, G_visual, G_textual):
        """Model/MHRec.py:842-864.  G_visual / G_textual: what rebuild_hypergraphs returned."""
        pos_items = pos_items - self.num_user
        neg_items = neg_items - self.num_user
        users, pos_items, neg_items = users.to(self.device), pos_items.to(self.device), neg_items.to(self.device)
        self.G_visual = G_visual
        self.G_textual = G_textual
        u_embeddings, i_embeddings, embeds_v, embeds_t, embeds_g = self.forward()
        bpr_loss = self.bpr_loss(users, pos_items, neg_items, u_embeddings, i_embeddings)
        reg_loss = self.regularization_loss(users, pos_items, neg_items, u_embeddings, i_embeddings)
        U = self.num_user
        ssl_loss_1 = self.contrastLoss(embeds_g[:U], embeds_t[:U], users) * self.ssl_alpha
        ssl_loss_2 = self.contrastLoss(embeds_g[U:], embeds_v[U:], pos_items) * self.ssl_alpha
        ssl_loss_3 = self.contrastLoss(embeds_g[:U], embeds_v[:U], users) * self.ssl_alpha
        ssl_loss_4 = self.contrastLoss(embeds_g[U:], embeds_t[U:], pos_items) * self.ssl_alpha
        ssl_loss = ssl_loss_3 + ssl_loss_4 + ssl_loss_1 + ssl_loss_2
        self.last_parts = (bpr_loss.detach(), reg_loss.detach(), ssl_loss.detach())
        return bpr_loss + reg_loss + ssl_loss

    def gene_ranklist(self, topk=50, to_cpu=True):
        """Model/MHRec.py:866-891: scores of the last forward's table, history entries = 1e-6, top-k, + num_user."""
        return ranking.gene_ranklist(self.result.detach().float(), self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                     state=ranking.state_of(self))

    full_sort_predict = gene_ranklist

    # ---- the diffusion half (plain torch on the device) ------------------------------------------------------------------------
    def _modality(self, m):
        return ((self.denoise_model_image, self.image_diffusion_model), (self.denoise_model_text, self.text_diffusion_model))[m]

    def diffusion_step(self, batch, modality, ts=None, noise=None, keep=None):
        """One batch of train_and_evaluate.py:338-362 (modality 0) or :365-389 (1): training_losses(...).mean() with gradient
        into that modality's denoiser.  batch: input hyperedge indices.  ts, noise, keep: given draws -- int64 [B], fp32
        [B, U + I], flags [B, U + I]."""
        dn, dm = self._modality(modality)
        x0 = self.diffusion_rows(batch, modality)
        B = x0.shape[0]
        ts = ts if ts is not None else self._take("ts")
        noise = noise if noise is not None else self._take("noise")
        keep = keep if keep is not None else self._take("denoise_keep")
        ts = ts.to(self.device).long() if ts is not None else torch.randint(0, dm.steps, (B,), device=self.device).long()
        noise = noise.to(self.device).float() if noise is not None else torch.randn_like(x0)
        if self.diffusion_double:
            x0 = x0.double()
            x_t = (dm._extract_into_tensor(dm.sqrt_alphas_cumprod, ts, x0.shape).double() * x0
                   + dm._extract_into_tensor(dm.sqrt_one_minus_alphas_cumprod, ts, x0.shape).double() * noise.double())
            out = self._denoise_double(dn, x_t, ts, keep)
        else:
            x_t = dm.q_sample(x0, ts, noise)
            out = dn(x_t, ts, True, keep.to(self.device)) if keep is not None else dn(x_t, ts)
        diff_loss = dm.weight(ts) * dm.mean_flat((x0 - out) ** 2)
        return diff_loss.mean()

    def _denoise_double(self, dn, x, timesteps, keep=None):
        """Denoise.forward(x, timesteps, True) on double copies of the denoiser's fp32 weights (the gradients come back through
        the casts, rounded once).  The in-layer's weight gradient is a sum over the batch whose terms cancel about 1000 : 1, and
        Adam normalises what is left: in fp32 the update of such an entry after three steps moves by 1e-4 of the largest one
        with the GEMM's summation order alone (measured: torch's GEMMs 1.3e-4, the f32 MFMA chain 4.0e-4, float64 8e-6)."""
        emb = F.linear(dn.time_embedding(timesteps).double(), dn.emb_layer.weight.double(), dn.emb_layer.bias.double())
        if dn.norm:
            x = F.normalize(x)
        x = x * (keep.to(self.device).double() * 2.0) if keep is not None else F.dropout(x, dn.drop.p, dn.training)
        h = torch.cat([x, emb], dim=-1)
        for layer in dn.in_layers:
            h = torch.tanh(F.linear(h, layer.weight.double(), layer.bias.double()))
        for i, layer in enumerate(dn.out_layers):
            h = F.linear(h, layer.weight.double(), layer.bias.double())
            if i != len(dn.out_layers) - 1:
                h = torch.tanh(h)
        return h

    def denoised_topk(self, batch, modality, noise=None, sampling_steps=5):
        """train_and_evaluate.py:409-413: p_sample(steps = 5, no sampling noise) of a batch's rows -- q_sample at t = 4, then the
        posterior means of all 20 steps -- and the top-num_hypernodes -> (int64 [B, k] node ids, the denoised rows)."""
        dn, dm = self._modality(modality)
        x0 = self.diffusion_rows(batch, modality)
        t = torch.full((x0.shape[0],), sampling_steps - 1, dtype=torch.int64, device=self.device)
        noise = noise if noise is not None else self._take("rebuild_noise")
        x_t = dm.q_sample(x0, t, noise.to(self.device).float() if noise is not None else None)
        for i in range(dm.steps - 1, -1, -1):
            x_t = dm.p_mean_variance(dn, x_t, torch.full_like(t, i))[0]
        return torch.topk(x_t, k=self.num_hypernodes)[1], x_t

    def rebuild_hypergraphs(self, loader_visual, loader_textual=None, noise=None):
        """train_and_evaluate.py:394-497: per modality, every batch's denoised top-k in loader order (hyperedge j = the j-th row
        the loader handed out) -> (G_visual, G_textual) as ops.HyperGraph.  noise: a pair of lists of given q_sample
        noise, one per batch."""
        out = []
        with torch.no_grad():
            for m, loader in enumerate((loader_visual, loader_textual if loader_textual is not None else loader_visual)):
                nodes = [self.denoised_topk(batch, m, None if noise is None else noise[m][b])[0] for b, batch in enumerate(loader)]
                out.append(ops.HyperGraph(torch.cat(nodes), self.num_user + self.num_item, validate=False))
        return out[0], out[1]
