"""COHESION with the reference's surface (Model/COHESION.py:69-411), compute on HIP kernels.

Same constructor arguments (main.py:381-383), the same Parameters under the same state_dict() names created in the same order
(so the same seed gives the same weights), `forward()`, `loss()`, `pre_epoch_processing()`, `topk_sample()`,
`adaptive_optimization()`, `gene_ranklist()`.  What changed underneath:
  * the user-user co-occurrence graph (`Data/<dataset>/user_graph_dict.npy`) is read when `COHESION.user_graph_path` names an
    existing file and is otherwise BUILT on the device from the training edges (ops.usergraph_build);
  * `topk_sample` (:240-271, a Python loop over all users per epoch) is one launch (ops.usergraph_sample); the urn that
    pads short neighbour lists draws from the library's counter generator, keyed by (torch seed, epoch), not from numpy;
    `set_epoch_graph()` installs a given draw;
  * the tail of the model (:327-359: the [N, 192] concatenation of the three modality tables, user_rep, features[user_graph]
    [U, k, 192], the matmul with the weights, the residual, item_rep + h_i, the final cat) is one autograd node
    (ops.cohesion_fuse) over the three [N, 64] tables; its backward sums each user's reverse list in chunks of
    `bwd_chunk` entries, so no lane group walks the longest list alone;
  * the item-graph term mm_adj^L item_rep is taken per 64-wide table (column-wise the same product) by `sparse.mm` over the
    kNN graph built as FREEDOM / DRAGON build it (no [I, I] similarity matrix);
  * a GCNLayer's propagate is `sparse.mm` + `ops.row_cosine_scale` (LayerGCN's), its Linears `ops.linear`; the id branch,
    whose output the reference detaches, runs under torch.no_grad(); dropout > 0 prunes as LayerGCN does here
    (ops.weighted_sample_keep, then a renormalised CSR); the ranking is `ranking.gene_ranklist` at D = 192.
The class switch `fused_aggregation = False` runs the reference's lines (:340-359) in plain torch.
Reference quirks kept on purpose:
  * the id third of every row is detached (`id_rep.data`, :321): `id_gcn.*` never receives a gradient, and neither do
    `image_embedding`, `text_embedding`, `image_trs`, `text_trs`, which only the constructor reads; `id_feat` receives one
    through the early fusion of the visual and textual encoders;
  * `weight_u` receives a gradient from the regulariser only (:384) -- the forward never reads it;
  * `self.k = 40` is hard-coded (:82), whatever --uu_topk says; `drop_rate` and `dim_E` beyond `image_trs` are unused,
    `dim_latent` is 64 (:92);
  * the loss is -mean(log2(sigmoid(.))) (:379) under adaptive modality weights that are detached (:364);
  * `result_embed` starts as a float64 xavier_normal_ table drawn from numpy and torch (:147-149) that is outside
    state_dict() once it has been moved to the device; the ranking mask is 1e-6;
  * a user without neighbours aggregates user 0 under an all-zero weight row (:250-253).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import graph, ops, ranking, sparse
from .DRAGON import DRAGON, User_Graph_sample
from .LayerGCN import LayerGCN


class GCNLayer(torch.nn.Module):
    """Model/COHESION.py:13-46: one modality's encoder, early-fused with the id features, LayerGCN's propagate."""

    def __init__(self, num_user, num_item, num_layer, dim_latent=None, device=None, features=None):
        super(GCNLayer, self).__init__()
        self.num_user, self.num_item = num_user, num_item
        self.dim_feat = features.size(1)
        self.dim_latent = dim_latent
        self.num_layer = num_layer
        self.device = device
        self.preference = nn.Parameter(
            nn.init.xavier_normal_(torch.empty(num_user, self.dim_latent, dtype=torch.float32), gain=1).to(self.device))
        self.MLP = nn.Linear(self.dim_feat, 4 * self.dim_latent)
        self.MLP_1 = nn.Linear(4 * self.dim_latent, self.dim_latent)

    def forward(self, features, id_embd, adj):
        temp_features = ops.linear(ops.linear(features, self.MLP.weight, self.MLP.bias, act=1), self.MLP_1.weight, self.MLP_1.bias)
        temp_features = torch.abs(((torch.mul(id_embd, id_embd) + torch.mul(temp_features, temp_features)) / 2) + 1e-8).sqrt()
        ego_embeddings = ops.normalize_rows(self.preference, temp_features)      # F.normalize(cat((preference, temp), 0))
        all_embeddings = ego_embeddings
        total = ego_embeddings                                                   # the sum of layers includes layer 0 (:36, :44)
        for _ in range(self.num_layer):
            all_embeddings = ops.row_cosine_scale(sparse.mm(adj, all_embeddings), ego_embeddings)
            total = total + all_embeddings
        return total, self.preference


class COHESION(nn.Module):
    user_graph_path = None        # Data/<dataset>/user_graph_dict.npy (main.py sets it); missing or None: built on the device
    fused_aggregation = True      # False: the reference's lines in plain torch (tools/bench_cohesion.py, the tests)
    bwd_chunk = ops.COHESION_CHUNK     # entries of a reverse list one lane group sums in the node's backward; 0: unchunked

    def __init__(self, num_user, num_item, edge_index, user_item_dict, v_feat, t_feat, dim_E, reg_weight,
                 dropout, n_layers, mm_layers, ii_topk, mm_image_weight, device):
        super(COHESION, self).__init__()
        self.num_user, self.num_item = num_user, num_item
        self.n_nodes = num_user + num_item
        self.dim = dim_E
        self.dim_feat = dim_E
        self.n_layers = mm_layers
        self.knn_k = self.item_topk = ii_topk
        self.mm_image_weight = mm_image_weight
        self.dropout = dropout
        self.k = 40
        self.num_layer = n_layers
        self.drop_rate = 0.1
        self.reg_weight = reg_weight
        self.device = device
        self.user_item_dict = user_item_dict
        self.v_feat = v_feat.clone().detach().to(device)
        self.t_feat = t_feat.clone().detach().to(device)
        self.v_rep = self.t_rep = self.id_rep = None
        self.v_preference = self.t_preference = self.id_preference = None
        self.dim_latent = ops.COHESION_DIM

        self.image_embedding = nn.Embedding.from_pretrained(v_feat.clone().detach(), freeze=False)
        self.text_embedding = nn.Embedding.from_pretrained(t_feat.clone().detach(), freeze=False)
        self.image_trs = nn.Linear(self.v_feat.shape[1], self.dim_feat)
        self.text_trs = nn.Linear(self.t_feat.shape[1], self.dim_feat)

        self.knn_ind = {}
        image_adj = self.get_knn_adj_mat(self.image_embedding.weight.detach(), "image")
        text_adj = self.get_knn_adj_mat(self.text_embedding.weight.detach(), "text")
        # :114: mm_adj = w * image_adj + (1 - w) * text_adj (sparse add = union of entries)
        self.mm_adj = graph.add_scaled_coo(image_adj, self.mm_image_weight, text_adj, 1.0 - self.mm_image_weight,
                                           self.num_item).to(self.device)

        # :118-122 (the reference fills it from numpy first; xavier_normal_ overwrites every value from torch's generator)
        self.weight_u = nn.Parameter(nn.init.xavier_normal_(torch.empty(self.num_user, 2, 1, dtype=torch.float32)))
        self.weight_u.data = F.softmax(self.weight_u.data, dim=1)

        edges = np.asarray(edge_index)
        self._u = torch.from_numpy(edges[:, 0].astype(np.int64))
        self._i = torch.from_numpy(edges[:, 1].astype(np.int64) - num_user)
        self.norm_adj = self.norm_adj_matrix = self.get_norm_adj_mat().to(self.device)
        self.masked_adj = self.norm_adj
        self.edge_indices, self.edge_values = self.get_edge_info()
        self.edge_indices, self.edge_values = self.edge_indices.to(device), self.edge_values.to(device)
        self._prune_seed, self._prune_calls = int(torch.initial_seed()) & (2**63 - 1), 0

        self.create_gcn_layers()

        self.user_graph = User_Graph_sample(num_user, 'add', self.dim_latent)
        # :147-149 (a float64 table the first forward replaces; no Parameter once it has been moved to the device)
        self.result_embed = nn.init.xavier_normal_(torch.tensor(np.random.randn(self.n_nodes, self.dim))).to(self.device)

        self._seed, self._epoch = int(torch.initial_seed()) & (2**63 - 1), 0
        self.hist = ranking.history_csr(user_item_dict, num_user, device)
        self.user_graph_dict = None
        self.graph_structure = self._load_or_build_user_graph()

    def create_gcn_layers(self):
        kw = dict(num_layer=self.num_layer, dim_latent=self.dim_latent, device=self.device)
        self.v_gcn = GCNLayer(self.num_user, self.num_item, features=self.v_feat, **kw)
        self.t_gcn = GCNLayer(self.num_user, self.num_item, features=self.t_feat, **kw)
        self.id_feat = nn.Parameter(
            nn.init.xavier_normal_(torch.empty(self.num_item, self.dim_latent, dtype=torch.float32), gain=1).to(self.device))
        self.id_gcn = GCNLayer(self.num_user, self.num_item, features=self.id_feat, **kw)

    # ---- graphs ---------------------------------------------------------------------------------------------------------------
    # :165-215 are LayerGCN's lines (the binary normalised adjacency in fp64, the interaction list and its pruning weights),
    # :217-238 DRAGON's (FREEDOM's cosine kNN graph): the ports of those classes, unchanged
    get_norm_adj_mat = LayerGCN.get_norm_adj_mat
    get_edge_info = LayerGCN.get_edge_info
    _normalize_adj_m = LayerGCN._normalize_adj_m
    _set_masked_adj = LayerGCN._set_masked_adj
    get_knn_adj_mat = DRAGON.get_knn_adj_mat
    compute_normalized_laplacian = DRAGON.compute_normalized_laplacian
    _load_or_build_user_graph = DRAGON._load_or_build_user_graph

    # ---- per epoch ------------------------------------------------------------------------------------------------------------
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
        if self.fused_aggregation:
            ops.usergraph_rev_chunks(self.graph_structure, self.bwd_chunk)

    def pre_epoch_processing(self):
        """:273-289: this epoch's k neighbours and their weights (and the chunks of their reverse lists), then the pruned
        interaction graph: a degree-sensitive sample without replacement of int(E (1 - dropout)) interactions, renormalised."""
        self.epoch_user_graph, self.user_weight_matrix = self.topk_sample(self.k)
        if self.fused_aggregation:
            ops.usergraph_rev_chunks(self.graph_structure, self.bwd_chunk)
        if self.dropout <= .0:
            self.masked_adj = self.norm_adj
            return
        keep_len = int(self.edge_values.size(0) * (1. - self.dropout))
        keep = ops.weighted_sample_keep(self.edge_values, keep_len, self._prune_seed, step=self._prune_calls)
        self._prune_calls += 1
        self._set_masked_adj(self.edge_indices[:, keep.bool()])

    # ---- hot path -------------------------------------------------------------------------------------------------------------
    def build_representation(self):
        """:319-338 without the concatenation: the three [N, 64] tables, the id one detached."""
        with torch.no_grad():       # :321 takes id_rep.data: nothing reads this branch's gradient
            id_rep, self.id_preference = self.id_gcn(self.id_feat, self.id_feat, self.masked_adj)
        self.v_rep, self.v_preference = self.v_gcn(self.v_feat, self.id_feat, self.masked_adj)
        self.t_rep, self.t_preference = self.t_gcn(self.t_feat, self.id_feat, self.masked_adj)
        self.id_rep = id_rep
        return id_rep, self.v_rep, self.t_rep

    def _item_graph(self, table, grad=True):
        if self.n_layers <= 0:
            return None
        with torch.set_grad_enabled(grad and torch.is_grad_enabled()):
            h = table[self.num_user:]
            for _ in range(self.n_layers):
                h = sparse.mm(self.mm_adj, h)
        return h

    def process_user_item_representation(self, id_rep, v_rep, t_rep):
        U = self.num_user
        if self.fused_aggregation:
            h_id, h_v, h_t = self._item_graph(id_rep, False), self._item_graph(v_rep), self._item_graph(t_rep)
            return ops.cohesion_fuse(id_rep, v_rep, t_rep, h_id, h_v, h_t, self.graph_structure, U, self.bwd_chunk)
        # :340-359 as written
        representation = torch.cat((id_rep, v_rep, t_rep), dim=1)
        user_rep = representation[:U]
        item_rep = representation[U:]
        h_i = item_rep
        for _ in range(self.n_layers):
            h_i = sparse.mm(self.mm_adj, h_i)
        h_u = self.user_graph(user_rep, self.epoch_user_graph.long(), self.user_weight_matrix)
        return torch.cat((user_rep + h_u, item_rep + h_i), dim=0)

    def forward(self, user, pos_items, neg_items):
        """:296-317 (LOCAL item ids) -> (pos_scores, neg_scores) under the adaptive modality weights."""
        self.result_embed = self.process_user_item_representation(*self.build_representation())
        user_tensor = self.result_embed[user]
        pos_item_tensor = self.result_embed[pos_items + self.num_user]
        neg_item_tensor = self.result_embed[neg_items + self.num_user]
        adaptive_weight = self.adaptive_optimization(user_tensor, pos_item_tensor, neg_item_tensor)
        pos_scores = torch.sum(user_tensor * pos_item_tensor * adaptive_weight, dim=1)
        neg_scores = torch.sum(user_tensor * neg_item_tensor * adaptive_weight, dim=1)
        return pos_scores, neg_scores

    def adaptive_optimization(self, user_e, pos_e, neg_e):
        """:361-369: per modality, 1 - softmax over the three score margins, detached, spread over the modality's columns."""
        pos_score_ = torch.mul(user_e, pos_e).view(-1, 3, self.dim_latent).sum(dim=-1)
        neg_score_ = torch.mul(user_e, neg_e).view(-1, 3, self.dim_latent).sum(dim=-1)
        modality_indicator = 1 - (pos_score_ - neg_score_).softmax(-1).detach()
        adaptive_weight = torch.tile(modality_indicator.view(-1, 3, 1), [1, 1, self.dim_latent])
        return adaptive_weight.view(-1, 3 * self.dim_latent)

    def loss(self, users, pos_items, neg_items):
        pos_items = pos_items - self.num_user
        neg_items = neg_items - self.num_user
        user, pos_items, neg_items = users.to(self.device), pos_items.to(self.device), neg_items.to(self.device)
        pos_scores, neg_scores = self.forward(user, pos_items, neg_items)
        self.last_bpr = -torch.mean(torch.log2(torch.sigmoid(pos_scores - neg_scores)))
        reg_embedding_loss_v = (self.v_preference[user] ** 2).mean()
        reg_embedding_loss_t = (self.t_preference[user] ** 2).mean()
        reg_loss = self.reg_weight * (reg_embedding_loss_v + reg_embedding_loss_t)
        self.last_reg = reg_loss + self.reg_weight * (self.weight_u ** 2).mean()
        return self.last_bpr + self.last_reg

    def gene_ranklist(self, topk=50, to_cpu=True):
        """:387-411 (mask value 1e-6)."""
        return ranking.gene_ranklist(self.result_embed.detach().float(), self.num_user, self.num_item, self.hist, 1e-6, topk,
                                     to_cpu=to_cpu, state=ranking.state_of(self))

    full_sort_predict = gene_ranklist
