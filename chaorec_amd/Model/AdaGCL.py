"""AdaGCL with the reference's surface (Model/AdaGCL.py:25-716), the per-edge work of its two view generators on HIP
kernels (csrc/adagcl.hip).

Same constructor, the four losses the training loop calls (`loss_1`, `loss_2`, `bpr_reg_loss`, `gen_loss`), `generator_1`
(vgae: encoder + decoder) and `generator_2` (DenoisingNet) with the reference's 26 parameter names in its order, created
in its order (same torch seed -> same weights), `gene_ranklist` through the shared ranking path.

Kept as written, on purpose:
  * `generator_2.features` is a snapshot of the INITIAL embeddings (a concat at construction), never refreshed.
  * DenoisingNet.generate puts no eps on the row sums, DenoisingNet.call puts 1e-6; a row whose masks are all 0 has the
    degree factor 10 either way.
  * a third layer raises get_attention's ValueError (two sets of gate weights exist).
  * calcRegLoss covers generator 2's twelve parameters in DenoisingNet.forward and the encoder's eight in vgae_decoder.
  * loss_rec is [B, 1] and broadcasts against the scalars before the final mean.
  * the GCN layers have no parameters: freeze / unfreeze are kept and touch nothing.

What changed underneath.  The graph is ONE graph.DropoutStructure over D^-1/2 A D^-1/2 (row-major, columns ascending: the
order of the reference's `_indices()`); a generated view is that structure with other values (sparse.DroppedAdj) -- a dropped
entry stays in the pattern with the value +0 -- so all 18 propagates of a step share one SpMM schedule.  DenoisingNet's last
Linear has ONE output: logit[e] = s_nb[row e] + s_self[col e] + b with two per-NODE scores (plain autograd ops on [N, 64]),
and the gate, the row sums, the degree factors, the values and the l0 term are one autograd node over them
(ops.adagcl_edge_gate) -- no [E, 64] tensor exists.  vgae.generate's per-edge MLP is ops.adagcl_edge_keep (f32
MFMA, the kept count stays on the device).  The uniform draws of the training form come from a counter RNG keyed by a
device-resident step counter; `feed_draws(randn=, u=)` queues GIVEN draws (parity tests), consumed in call order.
fused_edges = False runs the reference's lines in plain torch on the same weights and the same structure (the
measurements' other side); a dim_E other than 64 does so too.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import graph, ops, ranking, sparse

GAMMA, ZETA = -0.45, 1.05


def calcRegLoss(model):
    ret = 0
    for W in model.parameters():
        ret += W.norm(2).square()
    return ret


class GCNLayer(nn.Module):
    def __init__(self, device):
        super(GCNLayer, self).__init__()
        self.device = device

    def forward(self, adj, embeds, flag=True):
        """Model/AdaGCL.py:354-367: adj x (either flag: the same SpMM kernel)."""
        return sparse.mm(adj, embeds)


class vgae_encoder(nn.Module):
    def __init__(self, dim_E, device, forward_graphcl):
        super(vgae_encoder, self).__init__()
        hidden = dim_E
        self.device = device
        self.forward_graphcl = forward_graphcl
        self.encoder_mean = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True), nn.Linear(hidden, hidden))
        self.encoder_std = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True), nn.Linear(hidden, hidden), nn.Softplus())

    def forward(self, adj, noise=None):
        """Model/AdaGCL.py:396-411; noise: a given draw of x_mean's shape."""
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
        self.bceloss = nn.BCELoss(reduction='none')

    def forward(self, x, x_mean, x_std, users, items, neg_items, encoder):
        """Model/AdaGCL.py:436-468 ([B, 64] rows: plain torch)."""
        x_user, x_item = torch.split(x, [self.num_user, self.num_item], dim=0)
        edge_pos_pred = self.sigmoid(self.decoder(x_user[users] * x_item[items]))
        edge_neg_pred = self.sigmoid(self.decoder(x_user[users] * x_item[neg_items]))
        loss_edge_pos = self.bceloss(edge_pos_pred, torch.ones_like(edge_pos_pred))
        loss_edge_neg = self.bceloss(edge_neg_pred, torch.zeros_like(edge_neg_pred))
        loss_rec = loss_edge_pos + loss_edge_neg                      # [B, 1]
        kl_divergence = -0.5 * (1 + 2 * torch.log(x_std) - x_mean ** 2 - x_std ** 2).sum(dim=1)
        ancEmbeds, posEmbeds, negEmbeds = x_user[users], x_item[items], x_item[neg_items]
        pos_scores = torch.mul(ancEmbeds, posEmbeds).sum(dim=1)
        neg_scores = torch.mul(ancEmbeds, negEmbeds).sum(dim=1)
        bpr_loss = -torch.mean(torch.log(torch.sigmoid(pos_scores - neg_scores) + 1e-5))
        reg_loss = calcRegLoss(encoder) * self.reg_weight
        beta = 0.1
        return (loss_rec + beta * kl_divergence.mean() + bpr_loss + reg_loss).mean()


class vgae(nn.Module):
    def __init__(self, encoder, decoder):
        super(vgae, self).__init__()
        self.encoder = encoder
        self.decoder = decoder

    def forward(self, data, users, items, neg_items, noise=None):
        x, x_mean, x_std = self.encoder(data, noise)
        return self.decoder(x, x_mean, x_std, users, items, neg_items, self.encoder)

    def generate(self, data, structure, fused=True, noise=None, return_parts=False):
        """Model/AdaGCL.py:483-501 -> the view as a sparse.DroppedAdj over `structure`: the normalised adjacency's kept
        entries divided by fl32(kept / E), the others +0.  return_parts: also (keep bool [E], logits [E])."""
        x, _, _ = self.encoder(data, noise)
        lin1, lin2 = self.decoder.decoder[1], self.decoder.decoder[3]
        if fused:
            got = ops.adagcl_edge_keep(structure, x, lin1.weight, lin1.bias, lin2.weight, lin2.bias, structure.val,
                                             return_logits=return_parts)
            new_vals, keep = got[0], got[1]
            logits = got[3] if return_parts else None
        else:
            row, col = structure.entry_row.long(), structure.col.long()
            logits = self.decoder.decoder(x[row] * x[col])[:, 0]
            edge_pred = self.decoder.sigmoid(logits)
            vals = structure.val
            keep = ((edge_pred + 0.5).floor()).type(torch.bool)
            kept = vals[keep]
            new_vals = torch.zeros_like(vals)
            if kept.shape[0]:
                new_vals[keep] = kept / (kept.shape[0] / vals.shape[0])
        view = sparse.DroppedAdj(structure, new_vals, new_vals[structure.transpose_entry.long()])
        return (view, keep, logits) if return_parts else view


class DenoisingNet(nn.Module):
    def __init__(self, gcnLayers, features, dim_E, device, num_user, num_item, reg_weight):
        super(DenoisingNet, self).__init__()
        self.device = device
        self.features = features.detach().clone().to(device)       # the INITIAL embeddings, never refreshed
        self.gcnLayers = gcnLayers
        self.num_user = num_user
        self.num_item = num_item
        self.reg_weight = reg_weight
        self.lambda0 = 0.0001
        self.gamma, self.zeta = GAMMA, ZETA
        self.edge_weights = []
        self.l0_terms = []
        hidden = dim_E
        self.nblayers_0 = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True))
        self.nblayers_1 = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True))
        self.selflayers_0 = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True))
        self.selflayers_1 = nn.Sequential(nn.Linear(hidden, hidden), nn.ReLU(inplace=True))
        self.attentions_0 = nn.Sequential(nn.Linear(2 * hidden, 1))
        self.attentions_1 = nn.Sequential(nn.Linear(2 * hidden, 1))
        self.fused = True
        self.owner_state = None          # (state int64 [2], seed): the owner's device step counter

    def freeze(self, layer):
        for child in layer.children():
            for param in child.parameters():
                param.requires_grad = False

    def _layer(self, layer):
        if layer == 0:
            return self.nblayers_0, self.selflayers_0, self.attentions_0
        if layer == 1:
            return self.nblayers_1, self.selflayers_1, self.attentions_1
        raise ValueError("Invalid layer value, must be 0 or 1")

    def get_attention(self, input1, input2, layer=0):
        """Model/AdaGCL.py:545-570 on gathered rows (the plain-torch path) -> [E, 1]."""
        nb_layer, selflayer, att = self._layer(layer)
        return att(torch.concat([nb_layer(input1), selflayer(input2)], dim=1))

    def node_scores(self, x, layer=0):
        """The same logit as two per-node scalars: logit[e] = s_nb[row e] + s_self[col e] + b (one output in the last Linear)."""
        nb_layer, selflayer, att = self._layer(layer)
        w = att[0].weight[0]
        h = w.shape[0] // 2
        return nb_layer(x) @ w[:h], selflayer(x) @ w[h:], att[0].bias

    def hard_concrete_sample(self, log_alpha, beta=1.0, training=True, u=None):
        """Model/AdaGCL.py:572-596 (plain torch); u: the uniform draws in [1e-7, 1 - 1e-7], of log_alpha's shape."""
        if training:
            if u is None:
                u = 1e-7 + (1.0 - 2e-7) * torch.rand(log_alpha.shape, dtype=torch.float64, device=log_alpha.device)
            random_noise = u.to(log_alpha.device).to(torch.float64).reshape(log_alpha.shape)
            gate_inputs = torch.log(random_noise) - torch.log(1.0 - random_noise)
            gate_inputs = torch.sigmoid((gate_inputs + log_alpha) / beta)
        else:
            gate_inputs = torch.sigmoid(log_alpha)
        stretched_values = gate_inputs * (self.zeta - self.gamma) + self.gamma
        return torch.clamp(stretched_values, 0.0, 1.0).float()

    def _plain_values(self, x, layer, beta, training, eps, u):
        """The reference's lines over gathered [E, 64] rows -> (val [E], logit [E, 1], mask [E], d [N])."""
        st = self.adj_mat
        row, col = st.entry_row.long(), st.col.long()
        weight = self.get_attention(x[row, :], x[col, :], layer)
        mask = torch.squeeze(self.hard_concrete_sample(weight, beta, training, u))
        rowsum = torch.zeros(st.n_rows, dtype=mask.dtype, device=mask.device).index_add(0, row, mask) + eps
        d_inv_sqrt = torch.clamp(torch.pow(rowsum, -0.5), 0.0, 10.0)
        values = torch.mul(torch.mul(mask, d_inv_sqrt[row]), d_inv_sqrt[col])
        return values, weight, mask, d_inv_sqrt

    def _view(self, val):
        return sparse.DroppedAdj(self.adj_mat, val, val.detach()[self.adj_mat.transpose_entry.long()])

    def gate(self, x, layer, beta, training, u=None, return_parts=False):
        """-> (val [E], l0 scalar or None[, m, d, u]); training: the noised form with 1e-6 on the row sums."""
        eps = 1e-6 if training else 0.0
        if self.fused:
            s_nb, s_self, b = self.node_scores(x, layer)
            state, seed = self.owner_state if self.owner_state is not None else (None, 0)
            out = ops.adagcl_edge_gate(self.adj_mat, s_nb, s_self, b, beta, eps, training, state, seed, layer, u,
                                             return_parts=return_parts)
            return (out[0], out[1][0]) + tuple(out[2:])
        val, weight, mask, d = self._plain_values(x, layer, beta, training, eps, u)
        l0 = self.l0_norm(weight, beta) if training else None
        return (val, l0, mask, d, u) if return_parts else (val, l0)

    def generate(self, x, layer=0):
        """Model/AdaGCL.py:598-624: the evaluation form (no noise, no eps) -> the view for `sparse.mm`."""
        return self._view(self.gate(x, layer, 1.0, False)[0])

    def l0_norm(self, log_alpha, beta):
        gamma, zeta = torch.tensor(self.gamma), torch.tensor(self.zeta)
        return torch.mean(torch.sigmoid(log_alpha - beta * torch.log(-gamma / zeta)))

    def set_fea_adj(self, nodes, adj):
        self.node_size = nodes
        self.adj_mat = adj              # the owner's graph.DropoutStructure
        self.row, self.col = adj.entry_row, adj.col

    def call(self, inputs, training=None, u=None):
        """Model/AdaGCL.py:647-689; u: one given draw [E] per layer."""
        temperature = inputs if training else 1.0
        x = self.features.detach()
        embedsLst = [x]
        for layer_index, layer in enumerate(self.gcnLayers):
            val, l0 = self.gate(x, layer_index, temperature, bool(training), None if u is None else u[layer_index])
            if l0 is not None:
                self.l0_terms.append(l0)
            x = layer(self._view(val), x, False)
            embedsLst.append(x)
        return sum(embedsLst)

    def lossl0(self, temperature):
        l0_loss = torch.zeros([], device=self.device)
        for term in self.l0_terms:
            l0_loss = l0_loss + term
        self.l0_terms = []
        return l0_loss

    def forward(self, users, items, neg_items, temperature, u=None):
        """Model/AdaGCL.py:699-716."""
        self.freeze(self.gcnLayers)
        x = self.call(temperature, True, u)
        x_user, x_item = torch.split(x, [self.num_user, self.num_item], dim=0)
        ancEmbeds, posEmbeds, negEmbeds = x_user[users], x_item[items], x_item[neg_items]
        pos_scores = torch.mul(ancEmbeds, posEmbeds).sum(dim=1)
        neg_scores = torch.mul(ancEmbeds, negEmbeds).sum(dim=1)
        bpr_loss = -torch.mean(torch.log(torch.sigmoid(pos_scores - neg_scores) + 1e-5))
        reg_loss = calcRegLoss(self) * self.reg_weight
        lossl0 = self.lossl0(temperature) * self.lambda0
        return bpr_loss + reg_loss + lossl0


class AdaGCL(nn.Module):
    fused_edges = True       # False: both generators' per-edge lines in plain torch over gathered [E, 64] rows

    def __init__(self, num_user, num_item, edge_index, user_item_dict, dim_E, reg_weight, n_layers, ssl_temp, ssl_alpha, device):
        super(AdaGCL, self).__init__()
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
        self.ib_reg = 0.01
        self._fusable = int(dim_E) == ops.ADAGCL_DIM

        self.uEmbeds = nn.Parameter(nn.init.xavier_uniform_(torch.empty(num_user, dim_E)))
        self.iEmbeds = nn.Parameter(nn.init.xavier_uniform_(torch.empty(num_item, dim_E)))
        self.gcnLayers = nn.Sequential(*[GCNLayer(self.device) for i in range(self.n_layers)])

        e = torch.as_tensor(edge_index).long()
        csr = graph.binary_sym_norm_csr(e[:, 0], e[:, 1] - num_user, num_user, num_item)
        self.norm_adj_mat = sparse._dropout_structure(csr).to(device)       # Model/AdaGCL.py:65-105, and the entry maps

        encoder = vgae_encoder(self.dim_E, self.device, self.forward_graphcl)
        decoder = vgae_decoder(self.dim_E, self.device, num_user, num_item, reg_weight)
        self.generator_1 = vgae(encoder, decoder)
        self.generator_2 = DenoisingNet(self.getGCN(), self.getEmbeds(), self.dim_E, self.device, num_user, num_item, reg_weight)
        self.generator_2.set_fea_adj(num_user + num_item, self.norm_adj_mat)
        self.to(device)

        self._state = torch.zeros(2, dtype=torch.int64, device=device)     # steps taken, the count the draws in flight are keyed by
        self.seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self.generator_2.owner_state = (self._state, self.seed)
        self.hist = ranking.history_csr(user_item_dict, num_user, device)
        self._draws = {"randn": [], "u": []}

    # ---- draws ------------------------------------------------------------------------------------------------------------
    def feed_draws(self, randn=(), u=()):
        """Queue GIVEN draws, consumed in call order: randn [N, 64] tables for the encoder (one per generator_generate and one
        per gen_loss), u [E] vectors for DenoisingNet.call (n_layers per gen_loss)."""
        self._draws["randn"] += [torch.as_tensor(t).to(self.device).float() for t in randn]
        self._draws["u"] += [torch.as_tensor(t).to(self.device).float().contiguous() for t in u]

    def _take(self, kind, n=1):
        q = self._draws[kind]
        if len(q) < n:
            return None
        out, self._draws[kind] = q[:n], q[n:]
        return out

    def _fused(self):
        return bool(self.fused_edges and self._fusable)

    # ---- propagation ------------------------------------------------------------------------------------------------------
    def forward_gcn(self, adj):
        mainEmbeds = self.forward_graphcl(adj)
        return mainEmbeds[:self.num_user], mainEmbeds[self.num_user:]

    def forward_graphcl(self, adj):
        embedsLst = [torch.concat([self.uEmbeds, self.iEmbeds], dim=0)]
        for gcn in self.gcnLayers:
            embedsLst.append(gcn(adj, embedsLst[-1]))
        return sum(embedsLst)

    def forward_graphcl_(self, generator):
        """Model/AdaGCL.py:133-146: every layer multiplies with the view generated (without gradient) from its own input."""
        generator.fused = self._fused()
        embedsLst = [torch.concat([self.uEmbeds, self.iEmbeds], dim=0)]
        count = 0
        for gcn in self.gcnLayers:
            with torch.no_grad():
                adj = generator.generate(x=embedsLst[-1], layer=count)
            embedsLst.append(gcn(adj, embedsLst[-1]))
            count += 1
        return sum(embedsLst)

    def loss_graphcl(self, x1, x2, users, items):
        """Model/AdaGCL.py:148-187 -> [2B]: -log(pos / (row sum - pos)) of exp(cos / T) between the two views' batch rows."""
        T = self.ssl_temp
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

    def getEmbeds(self):
        self.unfreeze(self.gcnLayers)
        return torch.concat([self.uEmbeds, self.iEmbeds], dim=0)

    def unfreeze(self, layer):
        for child in layer.children():
            for param in child.parameters():
                param.requires_grad = True

    def getGCN(self):
        return self.gcnLayers

    def generator_generate(self, generator, return_parts=False):
        """Model/AdaGCL.py:201-209: generator 1's view of the normalised adjacency, without gradient."""
        noise = self._take("randn")
        with torch.no_grad():
            return generator.generate(self.norm_adj_mat, self.norm_adj_mat, self._fused(), noise[0] if noise else None, return_parts)

    # ---- the four losses of a training step ---------------------------------------------------------------------------------
    def _ids(self, users, pos_items, neg_items):
        pos_items = pos_items - self.num_user
        neg_items = neg_items - self.num_user
        return users.to(self.device), pos_items.to(self.device), neg_items.to(self.device)

    def loss_1(self, users, pos_items, neg_items):
        users, pos_items, neg_items = self._ids(users, pos_items, neg_items)
        data1 = self.generator_generate(self.generator_1)
        out1 = self.forward_graphcl(data1)
        out2 = self.forward_graphcl_(self.generator_2)
        loss = self.loss_graphcl(out1, out2, users, pos_items).mean() * self.ssl_alpha
        return loss, out1, out2

    def loss_2(self, users, pos_items, neg_items, out1, out2):
        users, pos_items, neg_items = self._ids(users, pos_items, neg_items)
        data1 = self.generator_generate(self.generator_1)
        _out1 = self.forward_graphcl(data1)
        _out2 = self.forward_graphcl_(self.generator_2)
        loss_ib = self.loss_graphcl(_out1, out1.detach(), users, pos_items) + self.loss_graphcl(_out2, out2.detach(), users, pos_items)
        return loss_ib.mean() * self.ib_reg

    def bpr_reg_loss(self, users, pos_items, neg_items):
        users, pos_items, neg_items = self._ids(users, pos_items, neg_items)
        usrEmbeds, itmEmbeds = self.forward_gcn(self.norm_adj_mat)
        ancEmbeds, posEmbeds, negEmbeds = usrEmbeds[users], itmEmbeds[pos_items], itmEmbeds[neg_items]
        pos_scores = torch.mul(ancEmbeds, posEmbeds).sum(dim=1)
        neg_scores = torch.mul(ancEmbeds, negEmbeds).sum(dim=1)
        bpr_loss = -torch.mean(torch.log(torch.sigmoid(pos_scores - neg_scores) + 1e-5))
        reg_loss = self.reg_weight * (torch.mean(self.uEmbeds[users] ** 2) + torch.mean(self.iEmbeds[pos_items] ** 2)
                                      + torch.mean(self.iEmbeds[neg_items] ** 2))
        return bpr_loss + reg_loss

    def gen_loss(self, users, pos_items, neg_items):
        """Model/AdaGCL.py:307-315.  Advances the step counter the device draws are keyed by."""
        users, pos_items, neg_items = self._ids(users, pos_items, neg_items)
        noise = self._take("randn")
        loss_1 = self.generator_1(self.norm_adj_mat, users, pos_items, neg_items, noise[0] if noise else None)
        self.generator_2.fused = self._fused()
        u = self._take("u", self.n_layers)
        if u is None and self.generator_2.fused:
            ops.adagcl_tick(self._state)
        loss_2 = self.generator_2(users, pos_items, neg_items, self.ssl_temp, u)
        return loss_1 + loss_2

    def gene_ranklist(self, topk=50, to_cpu=True):
        """Model/AdaGCL.py:317-344: scores of forward_gcn over the normalised adjacency, history entries = 1e-6, top-k."""
        with torch.no_grad():
            usrEmbeds, itmEmbeds = self.forward_gcn(self.norm_adj_mat)
            res = torch.cat((usrEmbeds, itmEmbeds), 0)
        return ranking.gene_ranklist(res, self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                     state=ranking.state_of(self))

    full_sort_predict = gene_ranklist
