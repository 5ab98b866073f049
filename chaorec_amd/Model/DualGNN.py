"""DualGNN with the reference's surface (Model/DualGNN.py:24-358), compute on HIP kernels.

Same constructor arguments (main.py:280), the same Parameters under the same state_dict() names created in the same order (so
the same seed gives the same weights), `forward()`, `loss()`, `bpr_loss()`, `regularization_loss()`, `pre_epoch_processing()`,
`topk_sample()`, `init_weight()`, `gene_ranklist()`.  What changed underneath:
  * the user-user co-occurrence graph (`Data/<dataset>/user_graph_dict.npy`) is read when `DualGNN.user_graph_path` names an
    existing file and is otherwise BUILT on the device from the training edges (ops.usergraph_build);
  * `topk_sample` (:319-358, a Python loop over all users per epoch) is one launch (ops.usergraph_sample); the urn that
    pads short neighbour lists draws from the library's counter generator, keyed by (torch seed, epoch), not from numpy;
    `set_epoch_graph()` installs a given draw;
  * everything after the two modality encoders (:189-239: representation, the weighted sum, User_Graph_sample.forward, the
    residual, the final cat) is one autograd node (ops.dualgnn_fuse): none of cat(v_rep[:U], t_rep[:U]) [U, D, 2],
    user_rep, features[user_graph] [U, k, D], h_u1 or representation exists in memory, forward or backward;
  * the two propagates per modality are the ordered SpMM over one shared normalised CSR, the Linears `ops.linear`, the BPR
    term the fused BPR kernel, the ranking `ranking.gene_ranklist`.
`construction` is the reference's hard-coded 'weighted_sum' and runs the fused node.  The class switch
`fused_aggregation = False` runs the reference's lines in plain torch; 'mean', 'max' and 'cat_mlp' exist on that path only.
`user_aggr_mode = 'mean'` overwrites the sampled weights with 1 / k (:345-346, :353-354) on the device.
Reference quirks kept on purpose:
  * `preference` is [U, dim_feat] and is concatenated with [I, dim_E] rows (:68-69, :83): the two must be equal (a ValueError
    here, a cat error there);
  * F.normalize runs over the concatenated [preference; MLP_1(leaky_relu(MLP(feat)))] (:83-84);
  * the two GCN layers apply the SAME conv_embed_1, and x_hat = x + h + h_1 (:87-90);
  * MLP_v, MLP_t and MLP_user are Parameters that never receive a gradient ('weighted_sum');
  * weight_i does receive one -- from the regulariser alone (:267; DRAGON's weight_i receives none);
  * the regulariser is reg_weight (mean(v_pref[users]^2) + mean(t_pref[users]^2) + mean(weight_u^2) + mean(weight_i^2));
  * a user without neighbours aggregates user 0 under an all-zero weight row (:327-334);
  * `self.result` starts as a float64 xavier_normal_ table drawn from numpy and torch (:163-164) that is not in
    state_dict(); the ranking mask is 1e-6.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import ops, ranking
from ..BasicGCN import GCNConv, _sym_norm_csr
from .DRAGON import User_Graph_sample  # (Model/DualGNN.py:95-110 is the same class: the plain-torch gather + matmul)


class GCN(torch.nn.Module):
    """Model/DualGNN.py:56-92: one modality's encoder over the interaction graph (DRAGON's but for the width of `preference`)."""

    def __init__(self, num_user, num_item, dim_latent, feat_embed_dim, aggr_mode, device, feat_size):
        super(GCN, self).__init__()
        self.num_user, self.num_item = num_user, num_item
        self.dim_latent, self.dim_feat = dim_latent, feat_embed_dim
        self.aggr_mode, self.device = aggr_mode, device
        self.preference = nn.Parameter(torch.empty(num_user, self.dim_feat, dtype=torch.float32, requires_grad=True))
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


class DualGNN(torch.nn.Module):
    user_graph_path = None        # Data/<dataset>/user_graph_dict.npy (main.py sets it); missing or None: built on the device
    fused_aggregation = True      # False: the reference's lines in plain torch (tools/bench_dualgnn.py, the tests)

    def __init__(self, num_user, num_item, edge_index, user_item_dict, v_feat, t_feat, dim_E, feature_embedding,
                 reg_weight, uu_topk, aggr_mode, device):
        super(DualGNN, self).__init__()
        self.num_user, self.num_item = num_user, num_item
        self.k = uu_topk
        self.aggr_mode = aggr_mode
        self.construction = 'weighted_sum'
        self.reg_weight = reg_weight
        self.user_item_dict = user_item_dict
        self.v_rep = self.t_rep = self.v_preference = self.t_preference = None
        self.device = device
        self.dim_latent, self.dim_feat = dim_E, feature_embedding
        self.user_aggr_mode = 'softmax'
        if dim_E not in ops.USERGRAPH_DIMS:
            raise ValueError(f"DualGNN: dim_E = {dim_E}, the aggregation kernels are built for {ops.USERGRAPH_DIMS}")
        if feature_embedding != dim_E:
            raise ValueError(f"DualGNN: feature_embedding = {feature_embedding} but dim_E = {dim_E}: the [U, feature_embedding] "
                             "preference rows are concatenated with [I, dim_E] item rows, so the two must be equal")

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
        # :163-164 (a float64 table the first forward replaces; no Parameter once it has been moved to the device)
        self.result = nn.init.xavier_normal_(torch.tensor(np.random.randn(num_user + num_item, self.dim_latent))).to(self.device)

        self._seed, self._epoch = int(torch.initial_seed()) & (2**63 - 1), 0
        self.hist = ranking.history_csr(user_item_dict, num_user, device)
        self.user_graph_dict = None
        self.graph_structure = self._load_or_build_user_graph()

    def init_weight(self, num_entities):
        weight = nn.Parameter(torch.randn(num_entities, 2, 1), requires_grad=True)
        nn.init.xavier_normal_(weight)
        weight.data = F.softmax(weight.data, dim=1)
        return weight

    # ---- the user graph -------------------------------------------------------------------------------------------------------
    def _load_or_build_user_graph(self):
        path = type(self).user_graph_path
        if path and os.path.exists(path):
            self.user_graph_dict = np.load(path, allow_pickle=True).item()
            return ops.UserGraphStructure.from_dict(self.user_graph_dict, self.num_user, device=self.device)
        rowptr, col = self.hist
        return ops.usergraph_build(rowptr.to(torch.int64).contiguous(), col.to(torch.int32).contiguous(), self.num_item)

    def pre_epoch_processing(self):
        """:315-317: this epoch's k neighbours and their weights, written into the structure's fixed buffers."""
        self.epoch_user_graph, self.user_weight_matrix = self.topk_sample(self.k)

    def topk_sample(self, k):
        s = self.graph_structure
        idx, w = ops.usergraph_sample(s, k, self._seed, self._epoch)
        self._epoch += 1
        if self.user_aggr_mode == 'mean':       # 1 / k wherever the user has a neighbour; the rows without stay zero
            w.copy_((s.nbr_len > 0).to(torch.float32).unsqueeze(1) * (torch.ones(k, device=w.device) / k))
            s.index_epoch()
        return idx, w

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
        if self.fused_aggregation:
            if self.construction != 'weighted_sum':
                raise ValueError(f"DualGNN: construction = '{self.construction}' exists on the plain-torch path only "
                                 "(fused_aggregation = False)")
            self.result = ops.dualgnn_fuse(self.v_rep, self.t_rep, self.weight_u, self.graph_structure, U)
            return self.result

        # :189-239 as written
        representation = self.v_rep + self.t_rep
        v_rep, t_rep = torch.unsqueeze(self.v_rep, 2), torch.unsqueeze(self.t_rep, 2)
        if self.construction == 'weighted_sum':
            user_rep = torch.matmul(torch.cat((v_rep[:U], t_rep[:U]), dim=2), self.weight_u).squeeze(2)
        elif self.construction == 'mean':
            user_rep = (self.v_rep[:U] + self.t_rep[:U]) / 2
        elif self.construction == 'max':
            user_rep = self.weight_u.transpose(1, 2) * torch.cat((v_rep[:U], t_rep[:U]), dim=2)
            user_rep = torch.max(user_rep, dim=2).values
        elif self.construction == 'cat_mlp':
            user_rep = self.weight_u.transpose(1, 2) * torch.cat((v_rep[:U], t_rep[:U]), dim=2)
            user_rep = self.MLP_user(torch.cat((user_rep[:, :, 0], user_rep[:, :, 1]), dim=1))
        else:
            raise ValueError(f"DualGNN: construction = '{self.construction}'")
        item_rep = representation[U:]
        h_u1 = self.user_graph(user_rep, self.epoch_user_graph.long(), self.user_weight_matrix)
        user_rep = user_rep + h_u1
        self.result = torch.cat((user_rep, item_rep), dim=0)
        return self.result

    def bpr_loss(self, users, pos_items, neg_items, embeddings):
        """:243-256 (LOCAL item ids): -mean(log(sigmoid(pos - neg) + 1e-5)) in the fused BPR kernel."""
        return ops.bpr_loss(embeddings, None, users, pos_items, neg_items, ops.VARIANT_LOG_SIGMOID_EPS, 0.0,
                            item_offset=self.num_user)[0]

    def regularization_loss(self, users):
        reg_embedding_loss_v = (self.v_preference[users] ** 2).mean()
        reg_embedding_loss_t = (self.t_preference[users] ** 2).mean()
        reg_loss = self.reg_weight * (reg_embedding_loss_v + reg_embedding_loss_t)
        if self.construction == 'weighted_sum':
            reg_loss = reg_loss + self.reg_weight * (self.weight_u ** 2).mean()
            reg_loss = reg_loss + self.reg_weight * (self.weight_i ** 2).mean()
        elif self.construction == 'cat_mlp':
            reg_loss = reg_loss + self.reg_weight * (self.MLP_user.weight ** 2).mean()
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
        """:288-313 (mask value 1e-6)."""
        return ranking.gene_ranklist(self.result.detach().float(), self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                     state=ranking.state_of(self))

    full_sort_predict = gene_ranklist
