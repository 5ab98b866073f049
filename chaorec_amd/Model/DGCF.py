"""DGCF with the reference's surface (Model/DGCF.py:49-238), compute on HIP kernels (csrc/dgcf.hip).

Same constructor, `forward()` -> (users, items, S), `bpr_loss()`, `regularization_loss()`, `cor_loss()`, `loss()`,
`gene_ranklist()`; same parameters (`user_intent_embeddings.weight`, `item_intent_embeddings.weight`) created and
initialised in the reference's order (same torch seed -> same weights); same intent state S, a plain attribute (not in
state_dict) created as ones and carried across every forward, updated L * T times per forward.

The reference, per layer l and routing iteration t: P = softmax(S) over the K intents; for every k a PyG propagate of the
width-D/K slice k of ego_l with edge weights deg^-1/2 deg^-1/2 P_k (both directions of an edge share its weight), then
per edge the score < normalize(X_k[u]), tanh(normalize(ego_l,k[i])) > over [E, D/K] gathers, and S = P + score.  At
L = T = 3, K = 4 that is 36 propagates and 36 gather / normalise / dot rounds per batch; the distance correlation builds
K - 1 pairs of dense 2B x 2B distance matrices.

What changed underneath.  The K propagates of one (l, t) are ONE launch over the CSR (each lane reads the weight of its
slice from the entry-major [E, K] P); the routing is fused into the user rows of that launch (the row's new X is in
registers; its entries are walked again for the scores) and writes S and the next P = softmax(S) beside it, so no
gather loop evaluates exp.  Iterations before the last launch over the user rows only (only their X is ever read);
the last one propagates every row and adds the layer into `result`.  The scores are detached in the reference
(nn.Embedding.from_pretrained), so the backward is one launch of the same kernel per layer with that layer's P.  The
distance correlation is two passes over the (i, j) pairs with nothing n x n stored (ops.dgcf_cor_loss).  Same
real-number result; fp32 rounding differs by re-association, so parity is to tolerance (tests/test_gpu_dgcf.py).
"""
import torch
import torch.nn as nn

from .. import graph, ops, ranking


class DGCF(nn.Module):
    def __init__(self, num_user, num_item, edge_index, user_item_dict, dim_E, reg_weight, corDecay, n_factors,
                 n_iterations, n_layers, aggr_mode, device):
        super(DGCF, self).__init__()
        self.result = None
        self.num_user = num_user
        self.num_item = num_item
        self.user_item_dict = user_item_dict
        self.reg_weight = reg_weight
        self.corDecay = corDecay
        self.dim_E = dim_E
        self.n_factors = int(n_factors)
        self.n_iterations = int(n_iterations)
        self.n_layers = int(n_layers)
        self.device = device
        self.aggr_mode = aggr_mode
        ops.dgcf_check_shape(dim_E, self.n_factors, self.n_layers, self.n_iterations)
        assert self.dim_E % self.n_factors == 0

        self.edge_index = graph.bidirectional_edge_index(edge_index)
        self.graph = graph.dgcf_structure(edge_index, num_user, num_user + num_item).to(device)
        rowptr, col = graph.user_hist_csr(user_item_dict, num_user)
        self.hist = (rowptr.to(device), col.to(device))

        # S (Model/DGCF.py:75) entry-major, with P = softmax(S) kept beside it; `S` below is the reference's [K, E] view
        E = self.graph.n_edges
        self._S = torch.ones((E, self.n_factors), dtype=torch.float32, device=device)
        self._P = torch.full((E, self.n_factors), 1.0 / self.n_factors, dtype=torch.float32, device=device)
        if E:
            ops.dgcf_softmax(self._S, self._P)

        self.user_intent_embeddings = nn.Embedding(num_user, dim_E)
        self.item_intent_embeddings = nn.Embedding(num_item, dim_E)
        nn.init.xavier_uniform_(self.user_intent_embeddings.weight)
        nn.init.xavier_uniform_(self.item_intent_embeddings.weight)

    @property
    def S(self):
        """The intent scores in the reference's [K, E] orientation (a view of the entry-major state)."""
        return self._S.t()

    def capture_state_tensors(self):
        """Model state a captured training step updates in place (optim.GraphedTrainStep puts it back after warm-up)."""
        return [self._S, self._P]

    def forward(self):
        """Model/DGCF.py:84-152; result = SUM of the layers ego_0 .. ego_L."""
        ego = torch.cat((self.user_intent_embeddings.weight, self.item_intent_embeddings.weight), dim=0)
        self.result = ops.dgcf_forward(ego, self.graph, self._S, self._P, self.n_layers, self.n_iterations)
        users, items = torch.split(self.result, [self.num_user, self.num_item], dim=0)
        return users, items, self.S

    def bpr_loss(self, users, pos_items, neg_items, final_user_embs, final_item_embs):
        """Model/DGCF.py:154-167."""
        return ops.bpr_loss(final_user_embs, final_item_embs, users, pos_items, neg_items, ops.VARIANT_LOG_SIGMOID_EPS,
                            0.0)[0]

    def regularization_loss(self, users, pos_items, neg_items, final_user_embs, final_item_embs):
        """Model/DGCF.py:169-177."""
        return ops.bpr_loss(final_user_embs, final_item_embs, users, pos_items, neg_items, ops.VARIANT_LOG_SIGMOID_EPS,
                            self.reg_weight)[2]

    def cor_loss(self, user, item):
        """Model/DGCF.py:179-195 (consecutive slice pairs only, / ((K+1) K / 2)); item: LOCAL ids.  -> [1]."""
        idx = torch.cat((user.to(self.device).long(), item.to(self.device).long() + self.num_user))
        return ops.dgcf_cor_loss(self.result, idx, self.n_factors)

    def _total(self, parts, users, pos_items):
        return parts[0] + self.corDecay * self.cor_loss(users, pos_items)

    def loss(self, users, pos_items, neg_items):
        """Model/DGCF.py:197-211 -> [1]."""
        pos_items = pos_items - self.num_user
        neg_items = neg_items - self.num_user
        users, pos_items, neg_items = users.to(self.device), pos_items.to(self.device), neg_items.to(self.device)
        self.forward()
        parts = ops.bpr_loss(self.result, None, users, pos_items, neg_items, ops.VARIANT_LOG_SIGMOID_EPS,
                             self.reg_weight, item_offset=self.num_user)
        return self._total(parts, users, pos_items)

    def loss_drawn(self, edges, B, seed, step, step_dev=None, advance=False, perm=None, perm_pos=None):
        """loss() with the batch drawn inside the fused BPR forward (see LightGCN.loss_drawn)."""
        self.forward()
        parts, users, pos, neg = ops.bpr_loss_drawn(self.result, None, edges, self.hist, B, self.num_user,
                                                    self.num_item, seed, step, ops.VARIANT_LOG_SIGMOID_EPS,
                                                    self.reg_weight, item_offset=self.num_user, step_dev=step_dev,
                                                    advance=advance, perm=perm, perm_pos=perm_pos)
        self.batch = (users, pos, neg)
        return self._total(parts, users, pos)

    def gene_ranklist(self, topk=50, to_cpu=True):
        """Model/DGCF.py:213-238 (mask value 1e-6)."""
        return ranking.gene_ranklist(self.result, self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                      state=ranking.state_of(self))

    full_sort_predict = gene_ranklist
