"""GraphAug with the reference's surface (Model/GraphAug.py:22-616), the per-edge work of its view learner and the
denominators of its two contrastive terms on HIP kernels (csrc/graphaug.hip).

Same constructor, `forward(adjlist, keepRate, l)`, `loss()`, `gene_ranklist` through the shared ranking path, the reference's
14 parameter names in its order, created in its order (same torch seed -> same weights).

Kept as written, on purpose:
  * the bottom MixHop layers' `weight_matrix` and `bias` are NOT parameters (the reference wraps `Parameter(...).cuda()`, which
    on a GPU is a plain tensor): initialised as there, never trained, absent from parameters() and state_dict() -- non-persistent
    buffers; gradient still passes through them to their input.
  * the 100 000 random entries of a view are (rdmUsrs, rdmItms1) with RAW item ids as columns (not offset by num_user),
    value 0.05, drawn once per step and shared by both views; duplicates add.  A view is not symmetric.
  * the view's values carry no gradient; the KL term (weight 1e-5) is the only gradient into the MixHop encoder, and the edge
    MLP gets none at all.
  * all three `aug_data` branches behind keepRate != 1.0 (loss() never reaches them), `reparametrize_n` (unused).

What changed underneath.  The graph is ONE graph.DropoutStructure over D^-1/2 A D^-1/2 (row-major, columns ascending: the
order of the reference's `_indices()`); a view is that structure with the sampled values (sparse.DroppedAdj) PLUS the step's
random entries as a small CSR with its transpose (ops.RandEntries, sorted on the device, no host synchronisation): a
view's GCN layer is LeakyReLU(sparse.mm(view, x) + 0.05 R x) -- no E-sized coalesce per step.  MixHop's three upper and three
bottom linears are one GEMM each (concatenated weights).  MixHopNetwork.forward returns no log_softmax (nothing reads it).
fused_edges: the sampler is ops.graphaug_edge_sample over P = z W1[:, :64]^T and Q = z W1[:, 64:]^T (two N-sized GEMMs
in place of the E-sized one); False: the reference's lines in plain torch over gathered [E, 128] rows.  fused_contrast: the
denominator log sum_m exp(<p1_b, e2_m> / T) is ops.graphaug_lse (no [B, M] matrix); False: the reference's lines.
`feed_draws` queues GIVEN draws (parity tests), consumed in call order; without them the fused sampler draws in its launch,
keyed by a device-resident step counter, and everything else draws from torch on the device.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import graph, ops, ranking, sparse

N_RANDOM = 100000
RANDOM_VALUE = 0.05


class GraphAugView:
    """A generated view: the fixed structure with this step's values, plus the step's random entries."""

    def __init__(self, dropped, rand):
        self.dropped, self.rand = dropped, rand


class SpAdjDropEdge(nn.Module):
    def __init__(self, keepRate):
        super(SpAdjDropEdge, self).__init__()

    def forward(self, adj, keepRate):
        """Model/GraphAug.py:27-44 over the fixed structure: a dropped entry stays in the pattern with the value +0."""
        vals = adj.val
        mask = ((torch.rand(vals.shape, device=vals.device) + keepRate).floor()).type(torch.bool)
        newVals = torch.where(mask, vals / keepRate, torch.zeros((), dtype=vals.dtype, device=vals.device))
        return sparse.DroppedAdj(adj, newVals, newVals[adj.transpose_entry.long()])


class GCNLayer(nn.Module):
    def __init__(self):
        super(GCNLayer, self).__init__()
        self.leaky = 0.5
        self.act = nn.LeakyReLU(negative_slope=self.leaky)

    def forward(self, adj, embeds):
        """Model/GraphAug.py:55-71: act(adj x); a view's random entries are a second, small product."""
        if isinstance(adj, GraphAugView):
            return ops.graphaug_rand_layer(sparse.mm(adj.dropped, embeds), embeds, adj.rand, RANDOM_VALUE, self.leaky)
        return self.act(sparse.mm(adj, embeds))


class ListModule(torch.nn.Module):
    def __init__(self, *args):
        super(ListModule, self).__init__()
        for idx, module in enumerate(args):
            self.add_module(str(idx), module)

    def __getitem__(self, idx):
        if idx < 0 or idx >= len(self._modules):
            raise IndexError('index {} is out of range'.format(idx))
        return list(self._modules.values())[idx]

    def __iter__(self):
        return iter(self._modules.values())

    def __len__(self):
        return len(self._modules)


def _hops(adj, x, n):
    for _ in range(n):
        x = sparse.mm(adj, x)
    return x


class SparseNGCNLayer(torch.nn.Module):
    """Model/GraphAug.py:99-144: relu(dropout(x W + b)), then iterations - 1 propagates."""

    def __init__(self, in_channels, out_channels, iterations, dropout_rate):
        super(SparseNGCNLayer, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.iterations, self.dropout_rate = iterations, dropout_rate
        self.weight_matrix = torch.nn.Parameter(torch.Tensor(in_channels, out_channels))
        self.bias = torch.nn.Parameter(torch.Tensor(1, out_channels))
        torch.nn.init.xavier_uniform_(self.weight_matrix)
        torch.nn.init.xavier_uniform_(self.bias)

    def tail(self, adj, base_features, mask=None):
        """everything after the linear: base_features = x W + b"""
        base_features = _dropout(base_features, self.dropout_rate, self.training, mask)
        return _hops(adj, torch.nn.functional.relu(base_features), self.iterations - 1)

    def forward(self, normalized_adjacency_matrix, features, mask=None):
        return self.tail(normalized_adjacency_matrix, torch.matmul(features, self.weight_matrix) + self.bias, mask)


class DenseNGCNLayer(torch.nn.Module):
    """Model/GraphAug.py:147-186: dropout(x W), iterations - 1 propagates, then + b.  W and b are not parameters (see above)."""

    def __init__(self, in_channels, out_channels, iterations, dropout_rate):
        super(DenseNGCNLayer, self).__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.iterations, self.dropout_rate = iterations, dropout_rate
        self.register_buffer("weight_matrix", torch.nn.init.xavier_uniform_(torch.empty(in_channels, out_channels)), persistent=False)
        self.register_buffer("bias", torch.nn.init.xavier_uniform_(torch.empty(1, out_channels)), persistent=False)

    def tail(self, adj, base_features, mask=None):
        """everything after the linear: base_features = x W"""
        base_features = _dropout(base_features, self.dropout_rate, self.training, mask)
        return _hops(adj, base_features, self.iterations - 1) + self.bias

    def forward(self, normalized_adjacency_matrix, features, mask=None):
        return self.tail(normalized_adjacency_matrix, torch.mm(features, self.weight_matrix), mask)


def _dropout(x, p, training, mask=None):
    """F.dropout, or a GIVEN keep mask (0 / 1) scaled the same way."""
    if mask is None:
        return torch.nn.functional.dropout(x, p=p, training=training)
    return x * (mask.to(x.dtype) * (1.0 / (1.0 - p))) if training else x


class MixHopNetwork(torch.nn.Module):
    """Model/GraphAug.py:189-244.  The three linears of a level are ONE GEMM over the concatenated weights."""

    def __init__(self, feature_number, class_number):
        super(MixHopNetwork, self).__init__()
        self.feature_number = feature_number
        self.class_number = class_number
        self.layers_1 = [200, 200, 200]
        self.layers_2 = [200, 200, 200]
        self.dropout = 0.5
        self.abstract_feature_number_1 = sum(self.layers_1)
        self.abstract_feature_number_2 = sum(self.layers_2)
        self.order_1 = len(self.layers_1)
        self.order_2 = len(self.layers_2)
        self.upper_layers = ListModule(*[
            SparseNGCNLayer(in_channels=self.feature_number, out_channels=self.layers_1[i - 1], iterations=i,
                            dropout_rate=self.dropout) for i in range(1, self.order_1 + 1)])
        self.bottom_layers = ListModule(*[
            DenseNGCNLayer(in_channels=self.abstract_feature_number_1, out_channels=self.layers_2[i - 1], iterations=i,
                           dropout_rate=self.dropout) for i in range(1, self.order_2 + 1)])
        self.fully_connected = torch.nn.Linear(self.abstract_feature_number_2, self.class_number)

    def forward(self, normalized_adjacency_matrix, features, masks=None):
        """-> (node_emb [N, class_number], None).  masks: six given dropout keep masks [N, 200] (upper 0..2, bottom 0..2)."""
        masks = [None] * 6 if masks is None else masks
        adj = normalized_adjacency_matrix
        up = torch.matmul(features, torch.cat([m.weight_matrix for m in self.upper_layers], 1)) + torch.cat([m.bias for m in self.upper_layers], 1)
        abstract_features_1 = torch.cat(
            [m.tail(adj, h, masks[i]) for i, (m, h) in enumerate(zip(self.upper_layers, torch.split(up, self.layers_1, 1)))], dim=1)
        low = torch.mm(abstract_features_1, torch.cat([m.weight_matrix for m in self.bottom_layers], 1))
        abstract_features_2 = torch.cat(
            [m.tail(adj, h, masks[3 + i]) for i, (m, h) in enumerate(zip(self.bottom_layers, torch.split(low, self.layers_2, 1)))], dim=1)
        return self.fully_connected(abstract_features_2), None


def _clamp_probs(p):
    eps = torch.finfo(p.dtype).eps
    return p.clamp(min=eps, max=1 - eps)


class ViewLearner(torch.nn.Module):
    def __init__(self, encoder, mlp_edge_model_dim=32):
        super(ViewLearner, self).__init__()
        self.encoder = encoder
        self.input_dim = mlp_edge_model_dim
        self.mlp_edge_model = nn.Sequential(
            nn.Linear(self.input_dim * 2, mlp_edge_model_dim),
            nn.ReLU(),
            nn.Linear(mlp_edge_model_dim, 1)
        )
        self.init_emb()

    def init_emb(self):
        for m in self.modules():
            if isinstance(m, nn.Linear):
                torch.nn.init.xavier_uniform_(m.weight.data)
                if m.bias is not None:
                    m.bias.data.fill_(0.0)

    def build_prob_neighbourhood(self, edge_wight, temperature=0.1, u=None):
        """Model/GraphAug.py:268-283 (plain torch); RelaxedBernoulli(temperature, probs).rsample() written out, so that a GIVEN
        uniform draw u can take the place of its torch.rand."""
        attention = torch.clamp(edge_wight, 0.01, 0.99)
        temperature = torch.Tensor([temperature]).to(attention.device)
        probs = _clamp_probs(attention)
        uniforms = _clamp_probs(torch.rand(attention.shape, dtype=probs.dtype, device=probs.device) if u is None else u)
        logits = (uniforms.log() - (-uniforms).log1p() + probs.log() - (-probs).log1p()) / temperature
        finfo = torch.finfo(logits.dtype)
        weighted_adjacency_matrix = torch.clamp(torch.sigmoid(logits), min=finfo.tiny, max=1.0 - finfo.eps)
        eps = 0.2
        mask = (weighted_adjacency_matrix > eps).detach().float()
        weighted_adjacency_matrix = weighted_adjacency_matrix * mask + 0.0 * (1 - mask)
        return weighted_adjacency_matrix

    def edge_logits(self, node_emb, structure):
        """the reference's E-sized lines: the MLP over gathered [E, 2 D] rows -> [E, 1]"""
        src, dst = structure.entry_row.long(), structure.col.long()
        edge_emb = torch.cat([node_emb[src], node_emb[dst]], 1)
        return self.mlp_edge_model(edge_emb)

    def sample(self, node_emb, structure, fused, u1=None, u2=None, state=None, seed=0, salt=0, return_parts=False):
        """Model/GraphAug.py:290-308, all detached -> (val [E], val_t [E][, logits [E], draws [2, E] or None])."""
        z = node_emb.detach()
        lin1, lin2 = self.mlp_edge_model[0], self.mlp_edge_model[2]
        if fused:
            d = z.shape[1]
            P, Q = z @ lin1.weight[:, :d].t(), z @ lin1.weight[:, d:].t()
            val, val_t, logits, draws = ops.graphaug_edge_sample(structure, P, Q, lin1.bias, lin2.weight, lin2.bias, u1, u2, state, seed,
                                                                       salt, True, return_parts, return_parts)
        else:
            with torch.no_grad():
                edge_logits = self.edge_logits(z, structure)
                bias = 0.0001
                u1 = torch.rand(edge_logits.size(), device=z.device) if u1 is None else u1.reshape(edge_logits.size())
                eps = (bias - (1 - bias)) * u1 + (1 - bias)
                gate_inputs = torch.log(eps) - torch.log(1 - eps)
                gate_inputs = (gate_inputs + edge_logits) / 1.0
                edge_wight = torch.sigmoid(gate_inputs).squeeze().detach()
                val = self.build_prob_neighbourhood(edge_wight, temperature=0.9, u=u2)
                val_t = val[structure.transpose_entry.long()]
                logits, draws = edge_logits[:, 0], None
        return (val, val_t, logits, draws) if return_parts else (val, val_t)

    def forward(self, x, structure, norm_adjacent_matrix, fused=False, masks=None, **draws):
        node_emb, _ = self.encoder(norm_adjacent_matrix, x, masks)
        val, val_t = self.sample(node_emb, structure, fused, **draws)
        return node_emb, sparse.DroppedAdj(structure, val, val_t)


class GraphAug(nn.Module):
    fused_edges = True        # False: the view learner's per-edge lines in plain torch over gathered [E, 128] rows
    fused_contrast = True     # False: contrastLoss's [B, M] matrix in plain torch

    def __init__(self, num_user, num_item, edge_index, user_item_dict, dim_E, reg_weight, n_layers, ssl_temp,
                 ssl_reg, device):
        super(GraphAug, self).__init__()
        self.num_user = num_user
        self.num_item = num_item
        self.edge_index = edge_index
        self.user_item_dict = user_item_dict
        self.dim_E = dim_E
        self.reg_weight = reg_weight
        self.n_layers = n_layers
        self.ssl_temp = ssl_temp
        self.ssl_reg = ssl_reg
        self.device = device

        self.keepRate = 1.0
        self.aug_data = 'ed'
        self.backbone = "mixhop"
        self.IB_size = 32
        self.gen = 2

        self.uEmbeds = nn.Parameter(nn.init.xavier_uniform_(torch.empty(self.num_user, self.dim_E)))
        self.iEmbeds = nn.Parameter(nn.init.xavier_uniform_(torch.empty(self.num_item, self.dim_E)))

        e = torch.as_tensor(edge_index).long()
        csr = graph.binary_sym_norm_csr(e[:, 0], e[:, 1] - num_user, num_user, num_item)
        self.norm_adj_mat = sparse._dropout_structure(csr).to(device)        # Model/GraphAug.py:354-394, and the entry maps

        self.gcnLayers = nn.Sequential(*[GCNLayer() for i in range(self.n_layers)])
        self.edgeDropper = SpAdjDropEdge(self.keepRate)
        if self.backbone == "mixhop":
            self.backbone_gnn = MixHopNetwork(feature_number=self.dim_E, class_number=self.IB_size * 2)
        self.view_learner = ViewLearner(self.backbone_gnn, mlp_edge_model_dim=self.dim_E)
        self.to(device)

        self._state = torch.zeros(2, dtype=torch.int64, device=device)      # steps taken, the count the draws in flight are keyed by
        self.seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self.hist = ranking.history_csr(user_item_dict, num_user, device)
        self._draws = {"u1": [], "u2": [], "masks": [], "rdm": []}
        self.last_parts = None

    # ---- draws ------------------------------------------------------------------------------------------------------------
    def feed_draws(self, u1=(), u2=(), masks=(), rdm=()):
        """Queue GIVEN draws, consumed in call order: per loss() one rdm pair (rdmUsrs, rdmItms1) and, per view, six dropout
        keep masks [N, 200] (upper 0..2, bottom 0..2), u1 [E] and u2 [E]."""
        self._draws["u1"] += [torch.as_tensor(t).to(self.device).float().contiguous() for t in u1]
        self._draws["u2"] += [torch.as_tensor(t).to(self.device).float().contiguous() for t in u2]
        self._draws["masks"] += [torch.as_tensor(t).to(self.device) for t in masks]
        self._draws["rdm"] += [tuple(torch.as_tensor(t).to(self.device).long() for t in pair) for pair in rdm]

    def _take(self, kind, n=1):
        q = self._draws[kind]
        if len(q) < n:
            return None
        out, self._draws[kind] = q[:n], q[n:]
        return out

    def _fusable(self, flag, what):
        if flag and int(self.dim_E) != ops.GRAPHAUG_DIM:
            raise ValueError(f"GraphAug: {what} tiles dim_E = {ops.GRAPHAUG_DIM}, not {self.dim_E} (the reference's own "
                             f"shapes line up at 64 only)")
        return bool(flag)

    # ---- propagation ------------------------------------------------------------------------------------------------------
    def getEgoEmbeds(self, adjlist, l):
        uEmbeds, iEmbeds = self.forward(adjlist, l=l)
        return torch.concat([uEmbeds, iEmbeds], dim=0)

    def _propagate(self, adj, iniEmbeds, masked=None):
        embedsLst = [iniEmbeds]
        for gcn in self.gcnLayers:
            a = adj() if callable(adj) else adj
            embedsLst.append(gcn(a, embedsLst[-1] if masked is None else embedsLst[-1] * masked))
        return sum(embedsLst)

    def forward(self, adjlist, keepRate=1.0, l=1):
        """Model/GraphAug.py:411-502.  adjlist[0]: the normalised adjacency's structure; [1], [2]: GraphAugViews."""
        adj = adjlist[0]
        iniEmbeds = torch.concat([self.uEmbeds, self.iEmbeds], dim=0)
        U = self.num_user
        mainEmbeds = self._propagate(adj, iniEmbeds)
        if keepRate == 1.0 and l == 1:
            return mainEmbeds[:U], mainEmbeds[U:]
        if keepRate == 1.0 and l == 3:
            embedsView1 = self._propagate(adjlist[1], iniEmbeds)
            embedsView2 = self._propagate(adjlist[2], iniEmbeds)
            return mainEmbeds[:U], mainEmbeds[U:], embedsView1[:U], embedsView1[U:], embedsView2[:U], embedsView2[U:]
        embedsView1 = embedsView2 = None
        if self.aug_data == 'ed' or self.aug_data == 'ED':
            embedsView1 = self._propagate(self.edgeDropper(adj, keepRate), iniEmbeds)
            embedsView2 = self._propagate(self.edgeDropper(adj, keepRate), iniEmbeds)
        elif self.aug_data == 'rw' or self.aug_data == 'RW':
            embedsView1 = self._propagate(lambda: self.edgeDropper(adj, keepRate), iniEmbeds)
            embedsView2 = self._propagate(lambda: self.edgeDropper(adj, keepRate), iniEmbeds)
        elif self.aug_data == 'nd' or self.aug_data == 'ND':
            rdmMask = ((torch.rand(iniEmbeds.shape[0], device=iniEmbeds.device) < keepRate) * 1.0)[:, None]
            embedsView1 = self._propagate(adj, iniEmbeds, rdmMask)
            rdmMask = ((torch.rand(iniEmbeds.shape[0], device=iniEmbeds.device) < keepRate) * 1.0)[:, None]
            embedsView2 = self._propagate(adj, iniEmbeds, rdmMask)
        return mainEmbeds[:U], mainEmbeds[U:], embedsView1[:U], embedsView1[U:], embedsView2[:U], embedsView2[U:]

    # ---- losses -----------------------------------------------------------------------------------------------------------
    def bpr_loss(self, users, pos_items, neg_items, usrEmbeds, itmEmbeds):
        user_embeddings = usrEmbeds[users]
        pos_item_embeddings = itmEmbeds[pos_items]
        neg_item_embeddings = itmEmbeds[neg_items]
        pos_scores = torch.sum(user_embeddings * pos_item_embeddings, dim=1)
        neg_scores = torch.sum(user_embeddings * neg_item_embeddings, dim=1)
        return -torch.mean(torch.log(torch.sigmoid(pos_scores - neg_scores) + 1e-5))

    def regularization_loss(self, users, pos_items, neg_items):
        user_embeddings = self.uEmbeds[users]
        pos_item_embeddings = self.iEmbeds[pos_items]
        neg_item_embeddings = self.iEmbeds[neg_items]
        return self.reg_weight * (torch.mean(user_embeddings ** 2) + torch.mean(pos_item_embeddings ** 2)
                                  + torch.mean(neg_item_embeddings ** 2))

    def reparametrize_n(self, mu, std):
        eps = 0.01
        return mu + eps * std

    def contrastLoss(self, embeds1, embeds2, nodes, temp):
        """Model/GraphAug.py:534-541: batch rows of view 1 against the WHOLE normalised table of view 2, no max-subtraction."""
        embeds1 = F.normalize(embeds1, p=2)
        embeds2 = F.normalize(embeds2, p=2)
        pckEmbeds1 = embeds1[nodes]
        pckEmbeds2 = embeds2[nodes]
        if self._fusable(self.fused_contrast, "the log-sum-exp node"):
            pos = torch.sum(pckEmbeds1 * pckEmbeds2, dim=-1) / temp
            return (ops.graphaug_lse(pckEmbeds1, embeds2, 1.0 / temp) - pos).mean()
        nume = torch.exp(torch.sum(pckEmbeds1 * pckEmbeds2, dim=-1) / temp)
        deno = torch.exp(pckEmbeds1 @ embeds2.T / temp).sum(-1)
        return -torch.log(nume / deno).mean()

    def loss(self, users, pos_items, neg_items):
        pos_items = pos_items - self.num_user
        neg_items = neg_items - self.num_user
        users, pos_items, neg_items = users.to(self.device), pos_items.to(self.device), neg_items.to(self.device)
        fused = self._fusable(self.fused_edges, "the edge sampler")
        st = self.norm_adj_mat

        adjlist = {0: st}
        ofea = self.getEgoEmbeds(adjlist, 1)

        rdm = self._take("rdm")
        if rdm is not None:
            rdmUsrs, rdmItms1 = rdm[0]
        else:
            rdmUsrs = torch.randint(self.num_user, [N_RANDOM], device=self.device)
            rdmItms1 = torch.randint_like(rdmUsrs, self.num_item)
        rand = ops.RandEntries(rdmUsrs, rdmItms1, st.n_rows)          # built once, shared by both views

        node_embs = []
        ticked = False
        for j in range(self.gen):
            masks, u1, u2 = self._take("masks", 6), self._take("u1"), self._take("u2")
            draws = dict(u1=u1[0], u2=u2[0]) if (u1 is not None and u2 is not None) else {}
            if fused and not draws:
                if not ticked:
                    ops.step_tick(self._state)
                    ticked = True
                draws = dict(state=self._state, seed=self.seed, salt=j)
            ant_node, ant_adj = self.view_learner(ofea, st, st, fused, masks, **draws)
            adjlist[j + 1] = GraphAugView(ant_adj, rand)
            node_embs.append(ant_node)
        node_embs = torch.mean(torch.stack(node_embs, 0), dim=0)

        mu = node_embs[:, :self.IB_size]
        std = F.softplus(node_embs[:, self.IB_size:] - self.IB_size, beta=1)
        kl_loss = -0.5 * (1 + 2 * std.log() - mu.pow(2) - std.pow(2)).sum(1).mean().div(math.log(2))

        usrEmbeds, itmEmbeds, usrEmbeds1, itmEmbeds1, usrEmbeds2, itmEmbeds2 = self.forward(adjlist, self.keepRate, 3)

        bpr_loss = self.bpr_loss(users, pos_items, neg_items, usrEmbeds, itmEmbeds)
        reg_loss = self.regularization_loss(users, pos_items, neg_items)
        cl_loss = (self.contrastLoss(usrEmbeds1, usrEmbeds2, users, self.ssl_temp) +
                   self.contrastLoss(itmEmbeds1, itmEmbeds2, pos_items, self.ssl_temp)) * self.ssl_reg
        self.last_parts = (bpr_loss.detach(), reg_loss.detach(), cl_loss.detach(), kl_loss.detach())
        return bpr_loss + reg_loss + cl_loss + 0.00001 * kl_loss

    def gene_ranklist(self, topk=50, to_cpu=True):
        """Model/GraphAug.py:588-616: scores of the main propagate, history entries = 1e-6, top-k."""
        with torch.no_grad():
            usrEmbeds, itmEmbeds = self.forward({0: self.norm_adj_mat}, 1.0)
            res = torch.cat((usrEmbeds, itmEmbeds), 0)
        return ranking.gene_ranklist(res, self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                     state=ranking.state_of(self))

    full_sort_predict = gene_ranklist
