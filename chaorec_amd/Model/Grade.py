"""Grade with the reference's surface (Model/Grade.py:18-554), the per-edge work of its three view generators -- ID, visual,
textual -- in one fused node on HIP kernels (csrc/grade.hip).

Same constructor, the three losses the training loop calls (`loss_1`, `bpr_reg_loss`, `gen_loss`), `generator_generate`,
`generator_1/2/3` (vgae: encoder + decoder) with the reference's 46 state_dict names in its order, created in its order (same
torch seed -> same weights; nn.Embedding draws its normal table before xavier_uniform_ overwrites it, as there),
`gene_ranklist` through the shared ranking path.

Kept as written, on purpose:
  * loss_rec is [B, 1] and broadcasts against the scalar KL term before the final mean.
  * the KL weight is 1, the reconstruction term is MSE (the BCE member is never called).
  * gen_loss leaves gradients on the embeddings and the projections; the next opt.zero_grad() drops them.
  * the two noise forwards multiply with generator 1's view and use no item graph.
  * delta_noise is ONE uniform table for all layers of a noise forward.

Changed: an undirected pair (u, i) is decided ONCE and both of its stored entries get the same probability.  In the
reference the two directions are two rows of one [E, 64] matmul whose logits can differ in the last bit, so at the
threshold the two directions could disagree; here a view is symmetric bit for bit.  The normalised value too is formed
once per pair, (d[row] p) d[col] at the entry with row <= col, because the two orders differ in the last bit.  And the
decoder of gen_loss's [B, 1] reconstruction term runs in float64 over the positives and the negatives together
(vgae_decoder._pred_pair): the two halves of every decoder gradient cancel, and two fp32 calls round each half first.

What changed underneath.  The graph is ONE graph.DropoutStructure over D^-1/2 A D^-1/2 (row-major, columns ascending: the
order of the reference's `_indices()`); a generated view is that structure with other values (sparse.DroppedAdj) -- a dropped
entry stays in the pattern with the value +0 -- so every propagate of a step shares one SpMM schedule.  vgae.generate keeps
the PROBABILITY as a kept entry's value and renormalises by the weighted row sums, d = (S + 1e-7)^-1/2, val = d[row] p d[col];
the reference sends that through scipy on the host, three times per step.  Here loss_1 runs the three encoders in the
reference's order (so the randn draws are consumed in that order), stacks their z and makes ONE ops.grade_views call:
the MLP per undirected pair (f32 MFMA), the row sums and the values, three launches for the three generators, nothing on the
host.  image_trs(v_feat) and text_trs(t_feat) are `ops.linear`, computed once per loss call and reused where the reference
recomputes them with unchanged weights (same value, same summed gradient).  Noise stays torch.randn / torch.rand on the
device; `feed_draws(randn=, rand=)` queues GIVEN draws (parity tests), consumed in call order: 3 randn + 2 rand tables in
loss_1, 3 randn in gen_loss.  fused_edges = False runs the reference's lines in plain torch over gathered [E, 64] rows on the
same structure, the normalisation by index_add on the device; a dim_E other than 64 does so too.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import graph, ops, ranking, sparse


class vgae_encoder(nn.Module):
    def __init__(self, dim_E, device, forward_graphcl):
        super(vgae_encoder, self).__init__()
        hidden = dim_E
        self.device = device
        self.forward_graphcl = forward_graphcl
        self.encoder_mean = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True), nn.Linear(hidden, hidden))
        self.encoder_std = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True), nn.Linear(hidden, hidden), nn.Softplus())

    def forward(self, adj, noise=None):
        """Model/Grade.py:44-59; noise: a given draw of x_mean's shape."""
        x = self.forward_graphcl(adj)
        x_mean = self.encoder_mean(x)
        x_std = self.encoder_std(x)
        if noise is None:
            noise = torch.randn(x_mean.shape, device=x_mean.device)
        x = noise.to(x_mean.device) * x_std + x_mean
        return x, x_mean, x_std


class vgae_decoder(nn.Module):
    def __init__(self, dim_E, device, num_user, num_item, reg_weight):
        super(vgae_decoder, self).__init__()
        hidden = dim_E
        self.device = device
        self.num_user = num_user
        self.num_item = num_item
        self.reg_weight = reg_weight
        self.decoder = nn.Sequential(nn.ReLU(inplace=True), nn.Linear(hidden, hidden), nn.ReLU(inplace=True), nn.Linear(hidden, 1))
        self.sigmoid = nn.Sigmoid()
        self.mse_loss = nn.MSELoss(reduction='none')
        self.bce_loss = nn.BCELoss(reduction='none')

    def forward(self, x, x_mean, x_std, users, items, neg_items, encoder):
        """Model/Grade.py:85-104 ([B, 64] rows: plain torch)."""
        x_user, x_item = torch.split(x, [self.num_user, self.num_item], dim=0)
        edge_pos_pred, edge_neg_pred = self._pred_pair(x_user[users] * x_item[items], x_user[users] * x_item[neg_items])
        loss_edge_pos = self.mse_loss(edge_pos_pred, torch.ones_like(edge_pos_pred))
        loss_edge_neg = self.mse_loss(edge_neg_pred, torch.zeros_like(edge_neg_pred))
        loss_rec = loss_edge_pos + loss_edge_neg                      # [B, 1]
        kl_divergence = -0.5 * (1 + 2 * torch.log(x_std) - x_mean ** 2 - x_std ** 2).sum(dim=1)
        beta = 1
        return (beta * kl_divergence.mean() + loss_rec).mean().float()

    def _pred_pair(self, rows_pos, rows_neg):
        """sigmoid(decoder(rows)) of the positives and the negatives -> two [B, 1] in float64, from ONE pass over the 2 B rows.
        Near the initial weights every prediction is about 1/2, so a decoder parameter's gradient is a negative sum over the
        positives plus a positive sum over the negatives that cancel (41 : 1 for the last bias on the test case).  Two fp32
        calls round each half at ITS magnitude before autograd adds them, which leaves the sum 1e-6 of itself off; here both
        halves are accumulated in double and every parameter's gradient is rounded once."""
        lin1, lin2 = self.decoder[1], self.decoder[3]
        rows = torch.cat([rows_pos, rows_neg], 0).double()
        h = F.relu(F.linear(F.relu(rows), lin1.weight.double(), lin1.bias.double()))
        pred = self.sigmoid(F.linear(h, lin2.weight.double(), lin2.bias.double()))
        return pred[:rows_pos.shape[0]], pred[rows_pos.shape[0]:]


def plain_view_values(decoder, x, structure, return_parts=False):
    """vgae.generate's lines (Model/Grade.py:119-151) in plain torch over gathered [E, 64] rows, the normalisation on the
    device -> val [E] over the fixed pattern[, keep bool [E], logits [E], d [N]]."""
    row, col = structure.entry_row.long(), structure.col.long()
    logits = decoder.decoder(x[row] * x[col])[:, 0]
    edge_pred = decoder.sigmoid(logits)
    keep = ((edge_pred + 0.5).floor()).type(torch.bool)
    p = torch.where(keep, edge_pred, torch.zeros_like(edge_pred))
    rowsum = torch.zeros(structure.n_rows, dtype=p.dtype, device=p.device).index_add(0, row, p) + 1e-7
    d_inv_sqrt = torch.pow(rowsum, -0.5)
    val = d_inv_sqrt[row] * p * d_inv_sqrt[col]
    return (val, keep, logits, d_inv_sqrt) if return_parts else val


class vgae(nn.Module):
    def __init__(self, encoder, decoder):
        super(vgae, self).__init__()
        self.encoder = encoder
        self.decoder = decoder

    def forward(self, data, users, items, neg_items, noise=None):
        x, x_mean, x_std = self.encoder(data, noise)
        return self.decoder(x, x_mean, x_std, users, items, neg_items, self.encoder)

    def mlp(self):
        """-> (W1 [64, 64], b1 [64], w2 [1, 64], b2 [1]) of the decoder."""
        lin1, lin2 = self.decoder.decoder[1], self.decoder.decoder[3]
        return lin1.weight, lin1.bias, lin2.weight, lin2.bias

    def generate(self, data, structure, fused=True, noise=None, return_parts=False):
        """Model/Grade.py:119-136 -> the view as a sparse.DroppedAdj over `structure` (the G = 1 call of the fused node).
        return_parts: also (keep bool [E], logits [E], d [N])."""
        x, _, _ = self.encoder(data, noise)
        if fused:
            got = ops.grade_views(structure, x, *self.mlp(), return_parts=return_parts)
            val = got[0][0] if return_parts else got[0]
            view = sparse.DroppedAdj(structure, val, val[structure.transpose_entry.long()])
            return (view, got[1][0], got[3][0], got[4][0]) if return_parts else view
        got = plain_view_values(self.decoder, x, structure, return_parts)
        val = got[0] if return_parts else got
        view = sparse.DroppedAdj(structure, val, val[structure.transpose_entry.long()])
        return (view,) + tuple(got[1:]) if return_parts else view


class GCNLayer(nn.Module):
    def __init__(self, device):
        super(GCNLayer, self).__init__()
        self.device = device

    def forward(self, adj, embeds, flag=True):
        """Model/Grade.py:161-174: adj x (either flag: the same SpMM kernel)."""
        return sparse.mm(adj, embeds)


def knn_adj(features, knn_k, device):
    """Model/Grade.py:295-326, FREEDOM's builder: cosine kNN (self included) -> (indices [2, nnz], D^-1/2 A D^-1/2 values with
    row-sum degrees) on the host.  On the GPU the [I, I] similarity matrix is never materialised (ops.score_topk)."""
    emb = features.to(device)
    context_norm = emb.div(torch.norm(emb, p=2, dim=-1, keepdim=True))
    n = context_norm.shape[0]
    if context_norm.is_cuda:
        d = context_norm.shape[1]
        d_pad = next(c for c in (8, 16, 32, 64, 128) if c >= d) if d <= 128 else (d + 63) // 64 * 64
        context_norm = F.pad(context_norm, (0, d_pad - d)).contiguous()   # zero columns leave the cosine unchanged
        knn_ind, _ = ops.score_topk(context_norm, context_norm, None, 0.0, knn_k)
    else:
        knn_ind = torch.cat([torch.topk(context_norm[s:s + 4096] @ context_norm.t(), knn_k, dim=-1)[1] for s in range(0, n, 4096)])
    rows = torch.arange(n, device=knn_ind.device).unsqueeze(1).expand(-1, knn_k).reshape(-1)
    indices = torch.stack((rows, knn_ind.reshape(-1)), 0).cpu()
    return indices, graph.out_degree_normalised_weights(indices[0], indices[1], n)


class Grade(nn.Module):
    fused_edges = True       # False: the three generators' per-edge lines in plain torch over gathered [E, 64] rows

    def __init__(self, num_user, num_item, edge_index, user_item_dict, v_feat, t_feat, dim_E, reg_weight,
                 n_layers, ssl_temp, ssl_alpha, ssl_temp2, noise_alpha, device):
        super(Grade, self).__init__()
        self.num_user = num_user
        self.num_item = num_item
        self.edge_index = edge_index
        self.user_item_dict = user_item_dict
        self.dim_E = dim_E
        self.reg_weight = reg_weight
        self.n_layers = n_layers
        self.device = device
        self.ssl_temp = ssl_temp
        self.ssl_alpha = ssl_alpha
        self.ssl_temp2 = ssl_temp2
        self.knn_k = 10
        self.mm_image_weight = 0.5
        self.mm_layers = 1
        self.noise_alpha = noise_alpha
        self._fusable = int(dim_E) == ops.GRADE_DIM

        self.uEmbeds = nn.Embedding(self.num_user, self.dim_E)
        nn.init.xavier_uniform_(self.uEmbeds.weight)
        self.utEmbeds = nn.Embedding(self.num_user, self.dim_E)
        nn.init.xavier_uniform_(self.utEmbeds.weight)
        self.uvEmbeds = nn.Embedding(self.num_user, self.dim_E)
        nn.init.xavier_uniform_(self.uvEmbeds.weight)
        self.iEmbeds = nn.Embedding(self.num_item, self.dim_E)
        nn.init.xavier_uniform_(self.iEmbeds.weight)

        v_feat = torch.as_tensor(v_feat).detach().float().cpu()
        t_feat = torch.as_tensor(t_feat).detach().float().cpu()
        self.v_feat = nn.Embedding.from_pretrained(v_feat, freeze=True)
        self.t_feat = nn.Embedding.from_pretrained(t_feat, freeze=True)
        self.image_trs = nn.Linear(v_feat.shape[1], self.dim_E)
        self.text_trs = nn.Linear(t_feat.shape[1], self.dim_E)

        image_adj = knn_adj(v_feat, self.knn_k, device)
        text_adj = knn_adj(t_feat, self.knn_k, device)
        self.mm_adj = graph.add_scaled_coo(image_adj, self.mm_image_weight, text_adj, 1.0 - self.mm_image_weight,
                                           self.num_item).to(device)

        self.gcnLayers = nn.Sequential(*[GCNLayer(self.device) for i in range(self.n_layers)])

        e = torch.as_tensor(edge_index).long()
        csr = graph.binary_sym_norm_csr(e[:, 0], e[:, 1] - num_user, num_user, num_item)
        self.norm_adj_mat = sparse._dropout_structure(csr).to(device)       # Model/Grade.py:248-288, and the entry maps
        ops.grade_pair_owner(self.norm_adj_mat)                       # the owner list, once, cached on the structure

        encoder = vgae_encoder(self.dim_E, self.device, self.forward_graphcl)
        decoder = vgae_decoder(self.dim_E, self.device, num_user, num_item, reg_weight)
        self.generator_1 = vgae(encoder, decoder)
        visual_encoder = vgae_encoder(self.dim_E, self.device, self.visual_forward_graphcl)
        visual_decoder = vgae_decoder(self.dim_E, self.device, num_user, num_item, reg_weight)
        self.generator_2 = vgae(visual_encoder, visual_decoder)
        textual_encoder = vgae_encoder(self.dim_E, self.device, self.textual_forward_graphcl)
        textual_decoder = vgae_decoder(self.dim_E, self.device, num_user, num_item, reg_weight)
        self.generator_3 = vgae(textual_encoder, textual_decoder)
        self.to(device)

        self.hist = ranking.history_csr(user_item_dict, num_user, device)
        self._draws = {"randn": [], "rand": []}
        self._proj = None          # (visual, textual) of the loss call in flight

    # ---- draws ------------------------------------------------------------------------------------------------------------
    def feed_draws(self, randn=(), rand=()):
        """Queue GIVEN draws, consumed in call order: randn [N, 64] tables for the encoders (three per loss_1, one per lone
        generator_generate, three per gen_loss), rand [N, 64] tables for the two noise forwards of loss_1."""
        self._draws["randn"] += [torch.as_tensor(t).to(self.device).float() for t in randn]
        self._draws["rand"] += [torch.as_tensor(t).to(self.device).float() for t in rand]

    def _take(self, kind):
        q = self._draws[kind]
        return q.pop(0) if q else None

    def _fused(self):
        return bool(self.fused_edges and self._fusable)

    # ---- propagation ------------------------------------------------------------------------------------------------------
    def buildItemGraph(self, h):
        for i in range(self.mm_layers):
            h = sparse.mm(self.mm_adj, h)
        return h

    def _projections(self):
        """image_trs(v_feat), text_trs(t_feat): once per loss call (self._proj), else computed here."""
        if self._proj is not None:
            return self._proj
        return (ops.linear(self.v_feat.weight, self.image_trs.weight, self.image_trs.bias),
                ops.linear(self.t_feat.weight, self.text_trs.weight, self.text_trs.bias))

    def _layers_sum(self, adj, iniEmbeds, delta_noise=None):
        embedsLst = [iniEmbeds]
        for gcn in self.gcnLayers:
            embeds = gcn(adj, embedsLst[-1])
            if delta_noise is not None:
                embeds = embeds + delta_noise / torch.sqrt(torch.tensor(embedsLst[-1].shape[1], dtype=torch.float32))
            embedsLst.append(embeds)
        return sum(embedsLst)

    def forward_gcn(self, adj):
        h = self.buildItemGraph(self.iEmbeds.weight)
        mainEmbeds = self._layers_sum(adj, torch.concat([self.uEmbeds.weight, self.iEmbeds.weight], dim=0))
        return mainEmbeds[:self.num_user], mainEmbeds[self.num_user:] + h

    def forward_graphcl(self, adj):
        iEmbeds = self.iEmbeds.weight + self.buildItemGraph(self.iEmbeds.weight)
        return self._layers_sum(adj, torch.concat([self.uEmbeds.weight, iEmbeds], dim=0))

    def visual_forward_graphcl(self, adj):
        visual = self._projections()[0]
        visual = visual + self.buildItemGraph(visual)
        return self._layers_sum(adj, torch.concat([self.uvEmbeds.weight, visual], dim=0))

    def textual_forward_graphcl(self, adj):
        textual = self._projections()[1]
        textual = textual + self.buildItemGraph(textual)
        return self._layers_sum(adj, torch.concat([self.utEmbeds.weight, textual], dim=0))

    def _delta_noise(self, like):
        given = self._take("rand")
        return given if given is not None else torch.rand(like.shape, device=like.device)

    def noise_visual_forward_graphcl(self, adj):
        iniEmbeds = torch.concat([self.uvEmbeds.weight, self._projections()[0]], dim=0)
        return self._layers_sum(adj, iniEmbeds, self._delta_noise(iniEmbeds))

    def noise_textual_forward_graphcl(self, adj):
        iniEmbeds = torch.concat([self.utEmbeds.weight, self._projections()[1]], dim=0)
        return self._layers_sum(adj, iniEmbeds, self._delta_noise(iniEmbeds))

    def loss_graphcl(self, x1, x2, users, items, ssl_temp):
        """Model/Grade.py:416-455 -> [2B]: -log(pos / (row sum - pos)) of exp(cos / T) between the two views' batch rows."""
        T = ssl_temp
        u1, i1 = torch.split(x1, [self.num_user, self.num_item], dim=0)
        u2, i2 = torch.split(x2, [self.num_user, self.num_item], dim=0)
        u1, i1, u2, i2 = (F.normalize(t, dim=1) for t in (u1, i1, u2, i2))
        all_embs1 = torch.cat([F.embedding(users, u1), F.embedding(items, i1)], dim=0)
        all_embs2 = torch.cat([F.embedding(users, u2), F.embedding(items, i2)], dim=0)
        all_embs1_abs = all_embs1.norm(dim=1)
        all_embs2_abs = all_embs2.norm(dim=1)
        sim_matrix = torch.einsum('ik,jk->ij', all_embs1, all_embs2) / torch.einsum('i,j->ij', all_embs1_abs, all_embs2_abs)
        sim_matrix = torch.exp(sim_matrix / T)
        pos_sim = torch.diagonal(sim_matrix)
        loss = pos_sim / (sim_matrix.sum(dim=1) - pos_sim)
        return -torch.log(loss)

    def generator_generate(self, generator, return_parts=False):
        """Model/Grade.py:457-465: one generator's view of the normalised adjacency, without gradient (the G = 1 call)."""
        with torch.no_grad():
            return generator.generate(self.norm_adj_mat, self.norm_adj_mat, self._fused(), self._take("randn"), return_parts)

    def generate_views(self, return_parts=False):
        """The three generate calls of loss_1 in the reference's order -> three sparse.DroppedAdj.  Fused: the encoders run one
        after the other (the randn draws in the reference's order), their z stacked into ONE ops.grade_views call.
        return_parts: also the node's (keep [3, E], kept [3], logits [3, E], d [3, N])."""
        gens = (self.generator_1, self.generator_2, self.generator_3)
        st = self.norm_adj_mat
        if not self._fused():
            got = [self.generator_generate(g, return_parts) for g in gens]
            if not return_parts:
                return got
            keep, logits, d = (torch.stack([g[k] for g in got]) for k in (1, 2, 3))
            return [g[0] for g in got], (keep, keep.sum(1), logits, d)
        with torch.no_grad():
            z = torch.stack([g.encoder(st, self._take("randn"))[0] for g in gens])
            mlps = [g.mlp() for g in gens]
            W1, b1, w2, b2 = (torch.stack([m[k].reshape(-1) for m in mlps]) for k in range(4))
            got = ops.grade_views(st, z, W1.reshape(3, self.dim_E, self.dim_E), b1, w2, b2.reshape(-1), return_parts=return_parts)
        val = got[0] if return_parts else got
        views = [sparse.DroppedAdj(st, val[g], val[g]) for g in range(3)]       # val[tentry] == val bit for bit: pairs decided once
        return (views, tuple(got[1:])) if return_parts else views

    # ---- the three losses of a training step --------------------------------------------------------------------------------
    def _ids(self, users, pos_items, neg_items):
        pos_items = pos_items - self.num_user
        neg_items = neg_items - self.num_user
        return users.to(self.device), pos_items.to(self.device), neg_items.to(self.device)

    def loss_1(self, users, pos_items, neg_items):
        users, pos_items, neg_items = self._ids(users, pos_items, neg_items)
        self._proj = self._projections()
        try:
            data1, data2, data3 = self.generate_views()
            out1 = self.forward_graphcl(data1)
            out2 = self.visual_forward_graphcl(data2)
            out3 = self.textual_forward_graphcl(data3)
            loss = (self.loss_graphcl(out1, out2, users, pos_items, self.ssl_temp).mean() +
                    self.loss_graphcl(out1, out3, users, pos_items, self.ssl_temp).mean()) * self.ssl_alpha
            noise_viusal = self.noise_visual_forward_graphcl(data1)
            loss = loss + (self.loss_graphcl(out2, noise_viusal, users, pos_items, self.ssl_temp2).mean()) * self.noise_alpha
            noise_textual = self.noise_textual_forward_graphcl(data1)
            loss = loss + (self.loss_graphcl(out3, noise_textual, users, pos_items, self.ssl_temp2).mean()) * self.noise_alpha
        finally:
            self._proj = None
        return loss

    def bpr_reg_loss(self, users, pos_items, neg_items):
        users, pos_items, neg_items = self._ids(users, pos_items, neg_items)
        self.usrEmbeds, self.itmEmbeds = self.forward_gcn(self.norm_adj_mat)
        ancEmbeds = self.usrEmbeds[users]
        posEmbeds = self.itmEmbeds[pos_items]
        negEmbeds = self.itmEmbeds[neg_items]
        pos_scores = torch.mul(ancEmbeds, posEmbeds).sum(dim=1)
        neg_scores = torch.mul(ancEmbeds, negEmbeds).sum(dim=1)
        bpr_loss = -torch.mean(torch.log(torch.sigmoid(pos_scores - neg_scores) + 1e-5))
        reg_loss = self.reg_weight * (torch.mean(self.uEmbeds(users) ** 2) + torch.mean(self.iEmbeds(pos_items) ** 2)
                                      + torch.mean(self.iEmbeds(neg_items) ** 2) + torch.mean(self.utEmbeds(users) ** 2)
                                      + torch.mean(self.uvEmbeds(users) ** 2))
        return bpr_loss + reg_loss

    def gen_loss(self, users, pos_items, neg_items):
        """Model/Grade.py:516-525: the three generators' own losses over the normalised adjacency."""
        users, pos_items, neg_items = self._ids(users, pos_items, neg_items)
        self._proj = self._projections()
        try:
            loss_1 = self.generator_1(self.norm_adj_mat, users, pos_items, neg_items, self._take("randn"))
            loss_2 = self.generator_2(self.norm_adj_mat, users, pos_items, neg_items, self._take("randn"))
            loss_3 = self.generator_3(self.norm_adj_mat, users, pos_items, neg_items, self._take("randn"))
        finally:
            self._proj = None
        return loss_1 + loss_3 + loss_2

    def gene_ranklist(self, topk=50, to_cpu=True):
        """Model/Grade.py:527-554: scores of forward_gcn over the normalised adjacency, history entries = 1e-6, top-k."""
        with torch.no_grad():
            usrEmbeds, itmEmbeds = self.forward_gcn(self.norm_adj_mat)
            res = torch.cat((usrEmbeds, itmEmbeds), 0)
        return ranking.gene_ranklist(res, self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                     state=ranking.state_of(self))

    full_sort_predict = gene_ranklist
