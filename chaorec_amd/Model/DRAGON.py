"""DRAGON with the reference's surface (Model/DRAGON.py:23-383), compute on HIP kernels.

Same constructor arguments (main.py:284), the same Parameters under the same state_dict() names created in the same order (so
the same seed gives the same weights), `forward()`, `loss()`, `pre_epoch_processing()`, `gene_ranklist()`.  What changed
underneath:
  * the user-user co-occurrence graph (`Data/<dataset>/user_graph_dict.npy`, which dualgnn-gen-u-u-matrix.py makes from a dense
    [U, U] matrix) is read when `DRAGON.user_graph_path` names an existing file and is otherwise BUILT on the device from the
    training edges (ops.usergraph_build: no [U, U] buffer);
  * `topk_sample` (:231-270, a Python loop over all users per epoch) is one launch (ops.usergraph_sample); the urn that
    pads short neighbour lists draws from the library's counter generator, keyed by (torch seed, epoch), not from numpy;
  * `User_Graph_sample.forward` and the lines around it (:289-302) are one autograd node (ops.usergraph_aggregate):
    neither user_rep, nor features[user_graph] [U, k, 2 D], nor h_u exists in memory, forward or backward;
  * the two GCNConv propagates per modality are the ordered SpMM over one shared normalised CSR, the item-item layers
    `sparse.mm` over the kNN graph built as FREEDOM builds it (no [I, I] similarity matrix), the Linears `ops.linear`, the BPR
    term the fused BPR kernel, the ranking `ranking.gene_ranklist`.
Reference quirks kept on purpose:
  * the two GCN layers apply the SAME conv_embed_1, and x_hat = x + h + h_1 (:87-90);
  * F.normalize runs over the concatenated [preference; MLP_1(leaky_relu(MLP(feat)))] (:83-84);
  * MLP_v, MLP_t, MLP_user, weight_i, image_trs, text_trs, image_embedding and text_embedding are Parameters that never
    receive a gradient;
  * the regulariser is a MEAN over preference[users]^2 of both branches plus (weight_u^2).mean() (:331-341);
  * a user without neighbours aggregates user 0 with an all-zero weight row (:244-246);
  * `self.result` starts as a float64 xavier_normal_ table drawn from numpy and torch (:194-195); the ranking mask is 1e-6.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import graph, ops, ranking, sparse
from ..BasicGCN import GCNConv, _sym_norm_csr


class GCN(torch.nn.Module):
    """Model/DRAGON.py:56-92: one modality's encoder over the interaction graph."""

    def __init__(self, num_user, num_item, dim_latent, feat_embed_dim, aggr_mode, device, feat_size):
        super(GCN, self).__init__()
        self.num_user, self.num_item = num_user, num_item
        self.dim_latent, self.dim_feat = dim_latent, feat_embed_dim
        self.aggr_mode, self.device = aggr_mode, device
        self.preference = nn.Parameter(torch.empty(num_user, self.dim_latent, dtype=torch.float32, requires_grad=True))
        nn.init.xavier_normal_(self.preference)
        self.MLP = nn.Linear(feat_size, 4 * self.dim_latent)
        self.MLP_1 = nn.Linear(4 * self.dim_latent, self.dim_latent)
        self.conv_embed_1 = GCNConv(self.dim_latent, self.dim_latent, aggr=self.aggr_mode)

    def forward(self, edge_index, features):
        temp_features = ops.linear(ops.linear(features, self.MLP.weight, self.MLP.bias, act=1), self.MLP_1.weight, self.MLP_1.bias)
        x = F.normalize(torch.cat((self.preference, temp_features), dim=0))
        h = self.conv_embed_1(x, edge_index)
        h_1 = self.conv_embed_1(h, edge_index)      # (the same conv twice)
        return x + h + h_1, self.preference


class User_Graph_sample(torch.nn.Module):
    """Model/DRAGON.py:95-110, kept for its name and for comparisons: the plain-torch gather + matmul."""

    def __init__(self, num_user, aggr_mode, dim_latent):
        super(User_Graph_sample, self).__init__()
        self.num_user, self.dim_latent, self.aggr_mode = num_user, dim_latent, aggr_mode

    def forward(self, features, user_graph, user_matrix):
        u_features = features[user_graph]
        return torch.matmul(user_matrix.unsqueeze(1), u_features).squeeze(1)


class DRAGON(torch.nn.Module):
    user_graph_path = None        # Data/<dataset>/user_graph_dict.npy (main.py sets it); missing or None: built on the device
    fused_aggregation = True      # False: the reference's gather + matmul in plain torch (tools/bench_dragon.py, the tests)

    def __init__(self, num_user, num_item, edge_index, user_item_dict, v_feat, t_feat, dim_E, feature_embedding,
                 reg_weight, n_layers, ii_topk, uu_topk, mm_image_weight, aggr_mode, device):
        super(DRAGON, self).__init__()
        self.num_user, self.num_item = num_user, num_item
        self.item_topk, self.user_topk = ii_topk, uu_topk
        self.aggr_mode = aggr_mode
        self.construction = 'cat'
        self.reg_weight = reg_weight
        self.user_item_dict = user_item_dict
        self.v_rep = self.t_rep = self.v_preference = self.t_preference = None
        self.device = device
        self.dim_latent, self.dim_feat = dim_E, feature_embedding
        self.user_aggr_mode = 'softmax'
        self.n_layers = n_layers
        self.mm_image_weight = mm_image_weight
        if dim_E not in ops.USERGRAPH_DIMS:
            raise ValueError(f"DRAGON: dim_E = {dim_E}, the aggregation kernels are built for {ops.USERGRAPH_DIMS}")

        self.MLP_v = nn.Linear(self.dim_latent, self.dim_latent, bias=False)
        self.MLP_t = nn.Linear(self.dim_latent, self.dim_latent, bias=False)

        edges = np.asarray(edge_index)
        self.edge_index = torch.as_tensor(edges, dtype=torch.long).t().contiguous()
        self.edge_index = torch.cat((self.edge_index, self.edge_index[[1, 0]]), dim=1)
        # BasicGCN.py:63-87 on the bidirectional list: one normalised CSR for both modalities and both layers
        self.norm_adj = _sym_norm_csr(self.edge_index, num_user + num_item, False).to(device)

        self.weight_u = self.init_weight(self.num_user)
        self.weight_i = self.init_weight(self.num_item)
        self.MLP_user = nn.Linear(self.dim_latent * 2, self.dim_latent)

        self.v_feat = v_feat.clone().detach().to(self.device)
        self.t_feat = t_feat.clone().detach().to(self.device)
        self.v_gcn = GCN(num_user, num_item, self.dim_latent, self.dim_feat, self.aggr_mode, self.device, v_feat.size(1))
        self.t_gcn = GCN(num_user, num_item, self.dim_latent, self.dim_feat, self.aggr_mode, self.device, t_feat.size(1))

        self.user_graph = User_Graph_sample(num_user, 'add', self.dim_latent)
        self._seed, self._epoch = int(torch.initial_seed()) & (2**63 - 1), 0
        self.hist = ranking.history_csr(user_item_dict, num_user, device)
        self.user_graph_dict = None
        self.graph_structure = self._load_or_build_user_graph()

        self.image_embedding = nn.Embedding.from_pretrained(v_feat.clone().detach(), freeze=False)
        self.text_embedding = nn.Embedding.from_pretrained(t_feat.clone().detach(), freeze=False)
        self.image_trs = nn.Linear(self.v_feat.shape[1], self.dim_feat)
        self.text_trs = nn.Linear(self.t_feat.shape[1], self.dim_feat)

        self.knn_ind = {}
        image_adj = self.get_knn_adj_mat(self.image_embedding.weight.detach(), "image")
        text_adj = self.get_knn_adj_mat(self.text_embedding.weight.detach(), "text")
        # :189: mm_adj = w * image_adj + (1 - w) * text_adj (sparse add = union of entries)
        self.mm_adj = graph.add_scaled_coo(image_adj, self.mm_image_weight, text_adj, 1.0 - self.mm_image_weight,
                                           self.num_item).to(self.device)

        # :194-195 (a float64 table the first forward replaces; no Parameter once it has been moved to the device)
        self.result = nn.init.xavier_normal_(torch.tensor(np.random.randn(num_user + num_item, self.dim_latent))).to(self.device)

    def init_weight(self, num_entities):
        weight = nn.Parameter(torch.randn(num_entities, 2, 1), requires_grad=True)
        nn.init.xavier_normal_(weight)
        weight.data = F.softmax(weight.data, dim=1)
        return weight

    # ---- graphs ---------------------------------------------------------------------------------------------------------------
    def _load_or_build_user_graph(self):
        path = type(self).user_graph_path
        if path and os.path.exists(path):
            self.user_graph_dict = np.load(path, allow_pickle=True).item()
            return ops.UserGraphStructure.from_dict(self.user_graph_dict, self.num_user, device=self.device)
        rowptr, col = self.hist
        return ops.usergraph_build(rowptr.to(torch.int64).contiguous(), col.to(torch.int32).contiguous(), self.num_item)

    def get_knn_adj_mat(self, mm_embeddings, name=None):
        """Model/DRAGON.py:204-225 (the code of Model/FREEDOM.py:111-138): cosine kNN, the row itself among them, then
        D^-1/2 A D^-1/2 with row-sum degrees -> (indices [2, nnz], values) on the host; scoring + top-K are one kernel."""
        dev = self.device
        emb = mm_embeddings.to(dev)
        context_norm = emb.div(torch.norm(emb, p=2, dim=-1, keepdim=True))
        d = context_norm.shape[1]
        d_pad = next(c for c in (8, 16, 32, 64, 128) if c >= d) if d <= 128 else (d + 63) // 64 * 64
        context_norm = F.pad(context_norm, (0, d_pad - d)).contiguous()   # zero columns leave the cosine unchanged
        knn_ind, _ = ops.score_topk(context_norm, context_norm, None, 0.0, self.item_topk)
        if name is not None:
            self.knn_ind[name] = knn_ind
        n = context_norm.shape[0]
        rows = torch.arange(n, device=dev).unsqueeze(1).expand(-1, self.item_topk).reshape(-1)
        return self.compute_normalized_laplacian(torch.stack((rows, knn_ind.reshape(-1)), 0).cpu(), (n, n))

    def compute_normalized_laplacian(self, indices, adj_size):
        return indices, graph.out_degree_normalised_weights(indices[0], indices[1], adj_size[0])

    # ---- per epoch ------------------------------------------------------------------------------------------------------------
    def pre_epoch_processing(self):
        """:227-229: this epoch's k neighbours and their softmax weights, written into the structure's fixed buffers."""
        self.epoch_user_graph, self.user_weight_matrix = self.topk_sample(self.user_topk)

    def topk_sample(self, k):
        out = ops.usergraph_sample(self.graph_structure, k, self._seed, self._epoch)
        self._epoch += 1
        return out

    def set_epoch_graph(self, epoch_user_graph, user_weight_matrix):
        """Install a GIVEN epoch graph ([U, k] ids and weights), e.g. the one the reference's own topk_sample drew."""
        idx = torch.as_tensor(np.asarray(epoch_user_graph), dtype=torch.int32).to(self.device)
        w = torch.as_tensor(np.asarray(user_weight_matrix), dtype=torch.float32).to(self.device)
        self.graph_structure.set_epoch(idx, w)
        self.epoch_user_graph, self.user_weight_matrix = self.graph_structure.epoch_idx, self.graph_structure.epoch_w

    # ---- hot path -------------------------------------------------------------------------------------------------------------
    def forward(self):
        U = self.num_user
        self.v_rep, self.v_preference = self.v_gcn(self.norm_adj, self.v_feat)
        self.t_rep, self.t_preference = self.t_gcn(self.norm_adj, self.t_feat)
        item_rep = torch.cat((self.v_rep[U:], self.t_rep[U:]), dim=1)

        if self.fused_aggregation:
            user_rep = ops.usergraph_aggregate(self.v_rep[:U], self.t_rep[:U], self.weight_u, self.graph_structure)
        else:   # :289-302 as written
            user_rep = torch.cat((self.v_rep[:U].unsqueeze(2), self.t_rep[:U].unsqueeze(2)), dim=2)
            user_rep = self.weight_u.transpose(1, 2) * user_rep
            user_rep = torch.cat((user_rep[:, :, 0], user_rep[:, :, 1]), dim=1)
            user_rep = user_rep + self.user_graph(user_rep, self.epoch_user_graph.long(), self.user_weight_matrix)

        h_i = item_rep
        for _ in range(self.n_layers):
            h_i = sparse.mm(self.mm_adj, h_i)
        item_rep = item_rep + h_i

        self.result = torch.cat((user_rep, item_rep), dim=0)
        return self.result

    def bpr_loss(self, users, pos_items, neg_items, embeddings):
        """:316-329 (LOCAL item ids): -mean(log(sigmoid(pos - neg) + 1e-5)) in the fused BPR kernel."""
        return ops.bpr_loss(embeddings, None, users, pos_items, neg_items, ops.VARIANT_LOG_SIGMOID_EPS, 0.0,
                            item_offset=self.num_user)[0]

    def regularization_loss(self, users):
        reg_embedding_loss_v = (self.v_preference[users] ** 2).mean()
        reg_embedding_loss_t = (self.t_preference[users] ** 2).mean()
        reg_loss = self.reg_weight * (reg_embedding_loss_v + reg_embedding_loss_t)
        reg_loss = reg_loss + self.reg_weight * (self.weight_u ** 2).mean()
        return reg_loss

    def loss(self, users, pos_items, neg_items):
        pos_items = pos_items - self.num_user
        neg_items = neg_items - self.num_user
        users, pos_items, neg_items = users.to(self.device), pos_items.to(self.device), neg_items.to(self.device)
        embeddings = self.forward()
        self.last_bpr = self.bpr_loss(users, pos_items, neg_items, embeddings)
        self.last_reg = self.regularization_loss(users)
        return self.last_bpr + self.last_reg

    def gene_ranklist(self, topk=50, to_cpu=True):
        """:358-383 (mask value 1e-6)."""
        return ranking.gene_ranklist(self.result.detach().float(), self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                     state=ranking.state_of(self))

    full_sort_predict = gene_ranklist
