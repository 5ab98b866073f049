"""MVGAE with the reference's surface (Model/MVGAE.py:24-443), compute on HIP kernels (csrc/mvgae.hip).

Same constructor, method names and the 96 state_dict names in the reference's order (three GCNs x (MLP, five times
conv_embed / linear_layer / g_layer)), drawn call for call: torch_geometric's `uniform` on a conv's weight and bias, the weight
then re-drawn by xavier_normal_; g_layer2 / g_layer3 keep nn.Linear's own draw; the torch.rand under every xavier_normal_ of a
plain tensor consumes the generator (same torch seed -> same weights).

Kept as written, on purpose:
  * `preference` (per GCN) and `collaborative` are plain tensors in the reference, never Parameters: no optimiser step
    reaches them.  Here they are non-persistent buffers without gradient (outside state_dict, moved by .to()).
  * concate = False: the reference evaluates linear_layer1..3 and never reads the result.  The port does not evaluate them;
    their .grad stays None, as in the reference.
  * conv_embed_3 / linear_layer3 / g_layer3 exist and are unused at n_layers = 2.
  * result_embed is the product-of-experts mean of the last TRAINING forward (loss()); gene_ranklist ranks it, history
    entries at the value 1e-6.

What changed underneath.  A convolution is x W on the MFMA GEMM, one CSR SpMM over D^-1/2 (A + I) D^-1/2 built once, and
ONE launch for leaky_relu(dropout(normalize(. + bias))) (ops.mvgae_conv_tail).  The tail -- two products of experts,
four reparametrisations, four KL and four BPR terms -- is one autograd node (ops.mvgae_tail): the noise is drawn only
for the 3B rows the batch names, keyed by the table row, and the stacked [2, N, D] tables never exist.  Dropout masks and
noise come from a counter RNG keyed by a device-resident step counter, so a captured step draws fresh values at every
replay.  `loss(..., keep=, eps=)` takes GIVEN draws (parity tests).  fused_conv / fused_tail = False run the reference's
lines in plain torch (the measurements' other side); a dim_E other than 64 does so too.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import graph, ops, ranking

EPS = 1e-15
MAX_LOGVAR = 10


def _uniform(size, tensor):
    """torch_geometric.nn.inits.uniform."""
    if tensor is not None:
        bound = 1.0 / (size ** 0.5)
        tensor.data.uniform_(-bound, bound)


class BaseModel(nn.Module):
    """Model/MVGAE.py:24-68: x W (weight [in, out]) -> D^-1/2 (A + I) D^-1/2 add-aggregate -> + bias, normalize, dropout 0.1.
    forward() includes the leaky_relu every caller puts around it (it is part of the fused epilogue)."""

    def __init__(self, in_channels, out_channels, normalize=True, bias=True, aggr='add', **kwargs):
        super(BaseModel, self).__init__()
        assert aggr == 'add' and normalize and bias, "only the configuration Model/MVGAE.py builds is on the hot path"
        self.aggr = aggr
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.normalize = normalize
        self.weight = nn.Parameter(torch.Tensor(self.in_channels, out_channels))
        self.bias = nn.Parameter(torch.Tensor(out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        _uniform(self.in_channels, self.weight)
        _uniform(self.in_channels, self.bias)

    def forward(self, x, csr, owner, salt, keep=None):
        """-> leaky_relu(update(A (x W))); owner: the MVGAE that holds the flags, the seed and the step counter."""
        s = ops.spmm(csr, ops.linear(x, self.weight.t()))
        if owner.fused_conv and owner._fusable:
            return ops.mvgae_conv_tail(s, self.bias, owner._state, owner.seed, salt, self.training, keep)
        y = F.normalize(s + self.bias, p=2, dim=-1)
        if self.training and keep is not None:
            y = y * (keep.to(y.dtype) * (1.0 / 0.9))
        else:
            y = F.dropout(y, p=0.1, training=self.training)
        return F.leaky_relu(y)


class ProductOfExperts(nn.Module):
    def forward(self, mu, logvar, eps=1e-8):
        """Model/MVGAE.py:75-100 over stacked [M, N, D] tables (the plain-torch path)."""
        var = torch.exp(logvar) + eps
        T = 1. / var
        pd_mu = torch.sum(mu * T, dim=0) / torch.sum(T, dim=0)
        pd_var = 1. / torch.sum(T, dim=0)
        return pd_mu, torch.log(pd_var), pd_var


class GCN(nn.Module):
    def __init__(self, device, features, edge_index, num_user, num_item, dim_id, aggr_mode, concate, num_layer, dim_latent=None,
                 dim_feat=None):
        super(GCN, self).__init__()
        assert dim_latent and not concate, "Model/MVGAE.py builds its GCNs with dim_latent=128 and concate=False"
        self.device = device
        self.num_user = num_user
        self.num_item = num_item
        self.dim_id = dim_id
        self.dim_feat = features.size(1) if features is not None else dim_feat
        self.dim_latent = dim_latent
        self.edge_index = edge_index          # a graph.CSR (D^-1/2 (A+I) D^-1/2) shared by all convs
        self.features = features              # None: the owner's `collaborative` buffer, read through the owner at every forward
        self.aggr_mode = aggr_mode
        self.concate = concate
        self.num_layer = num_layer

        self.register_buffer("preference", nn.init.xavier_normal_(torch.rand((num_user, self.dim_latent))), persistent=False)
        self.MLP = nn.Linear(self.dim_feat, self.dim_latent)
        nn.init.xavier_normal_(self.MLP.weight)
        for k in (1, 2, 3, 4, 5):
            first = self.dim_latent if k == 1 else self.dim_id
            conv = BaseModel(first, self.dim_id, aggr=self.aggr_mode)
            nn.init.xavier_normal_(conv.weight)
            lin = nn.Linear(first, self.dim_id)
            nn.init.xavier_normal_(lin.weight)
            g = nn.Linear(self.dim_id, self.dim_id)
            if k not in (2, 3):                       # (Model/MVGAE.py:153-161: g_layer2 / g_layer3 keep nn.Linear's draw)
                nn.init.xavier_normal_(g.weight)
            setattr(self, f"conv_embed_{k}", conv)
            setattr(self, f"linear_layer{k}", lin)
            setattr(self, f"g_layer{k}", g)

    def forward(self, owner, index, keep=None):
        """Model/MVGAE.py:179-225 -> (mu, logvar).  index: 0 visual, 1 textual, 2 collaborative (the convs' salts are
        5 index + 0..4); keep: this GCN's given masks in call order."""
        keep = list(keep) if keep is not None else None
        take = (lambda: keep.pop(0)) if keep is not None else (lambda: None)
        features = self.features if self.features is not None else owner.collaborative
        temp_features = ops.linear(features, self.MLP.weight, self.MLP.bias)
        x = ops.normalize_rows(self.preference, temp_features)
        for k in range(1, min(self.num_layer, 3) + 1):
            conv, g = getattr(self, f"conv_embed_{k}"), getattr(self, f"g_layer{k}")
            h = conv(x, self.edge_index, owner, 5 * index + k - 1, take())          # Eq(4)
            x = ops.linear(h, g.weight, g.bias, act=1)                              # Eq(6); Eq(5) is never read
        mu = self.conv_embed_4(x, self.edge_index, owner, 5 * index + 3, take())
        mu = ops.linear(mu, self.g_layer4.weight, self.g_layer4.bias) + ops.linear(x, self.linear_layer4.weight, self.linear_layer4.bias, act=1)
        logvar = self.conv_embed_5(x, self.edge_index, owner, 5 * index + 4, take())
        logvar = ops.linear(logvar, self.g_layer5.weight, self.g_layer5.bias) + ops.linear(x, self.linear_layer5.weight, self.linear_layer5.bias, act=1)
        return mu, logvar


class MVGAE(nn.Module):
    fused_tail = True       # False: the reference's tail in plain torch
    fused_conv = True       # False: the reference's update() + leaky_relu in plain torch

    def __init__(self, num_user, num_item, edge_index, user_item_dict, v_feat, t_feat, dim_E, reg_weight, n_layers, device):
        super(MVGAE, self).__init__()
        self.num_user = num_user
        self.num_item = num_item
        self.user_item_dict = user_item_dict
        self.dim_E = dim_E
        self.kl_weight = reg_weight
        self.device = device
        self.n_layers = n_layers
        self.aggr_mode = 'add'
        self.concate = False
        self._fusable = int(dim_E) == ops.MVGAE_DIM

        self.register_buffer("collaborative", nn.init.xavier_normal_(torch.rand((self.num_item, self.dim_E))), persistent=False)
        self.graph = graph.basicgcn_csr(edge_index, num_user + num_item).to(device)
        self.experts = ProductOfExperts()
        self.v_feat = torch.as_tensor(v_feat).clone().detach().float().to(device)
        self.t_feat = torch.as_tensor(t_feat).clone().detach().float().to(device)
        self.v_gcn = GCN(device, self.v_feat, self.graph, num_user, num_item, dim_E, self.aggr_mode, self.concate,
                         num_layer=n_layers, dim_latent=128)
        self.t_gcn = GCN(device, self.t_feat, self.graph, num_user, num_item, dim_E, self.aggr_mode, self.concate,
                         num_layer=n_layers, dim_latent=128)
        self.c_gcn = GCN(device, None, self.graph, num_user, num_item, dim_E, self.aggr_mode, self.concate,
                         num_layer=n_layers, dim_latent=128, dim_feat=dim_E)
        self.result_embed = nn.init.xavier_normal_(torch.rand((num_user + num_item, dim_E))).to(device)
        self.to(device)

        self._state = torch.zeros(2, dtype=torch.int64, device=device)     # steps taken, the count the step in flight is keyed by
        self._row_ids = torch.arange(num_user + num_item + 1, dtype=torch.int64, device=device)
        self.seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        rowptr, col = graph.user_hist_csr(user_item_dict, num_user)
        self.hist = (rowptr.to(device), col.to(device))
        self.last = {}

    def capture_state_tensors(self):
        """Model state a captured training step updates in place (optim.GraphedTrainStep puts it back after warm-up)."""
        return [self._state]

    def _tables(self, keep=None):
        """The six [U + I, D] tables: (v_mu, v_logvar, t_mu, t_logvar, c_mu, c_logvar).  keep: 12 masks in call order."""
        if keep is not None:
            keep = [k.to(self.device) for k in keep]
            n = len(keep) // 3
            keep = [keep[:n], keep[n:2 * n], keep[2 * n:]]
        out = []
        for i, gcn in enumerate((self.v_gcn, self.t_gcn, self.c_gcn)):
            out += list(gcn(self, i, keep[i] if keep is not None else None))
        return out

    def reparametrize(self, mu, logvar, eps=None):
        """Model/MVGAE.py:270-284; eps: a given draw of logvar's shape."""
        logvar = logvar.clamp(max=MAX_LOGVAR)
        if self.training:
            if eps is None:
                eps = torch.randn_like(logvar)
            return mu + eps * 0.1 * torch.exp(logvar.mul(0.5))
        return mu

    def dot_product_decode_neg(self, z, user, neg_items, sigmoid=True):
        """Model/MVGAE.py:286-302 (not on the training path)."""
        users = torch.unsqueeze(user, 1)
        re_users = users.repeat(1, neg_items.size(0))
        neg_values = torch.sum(z[re_users] * z[neg_items + self.num_user], -1)
        max_neg_value = torch.max(neg_values, dim=-1).values
        return torch.sigmoid(max_neg_value) if sigmoid else max_neg_value

    def dot_product_decode(self, z, edge_index, sigmoid=True):
        """Model/MVGAE.py:304-313 (not on the training path)."""
        value = torch.sum(z[edge_index[0]] * z[edge_index[1] + self.num_user], dim=1)
        return torch.sigmoid(value) if sigmoid else value

    def _poe(self, tables):
        v_mu, v_logvar, t_mu, t_logvar, c_mu, c_logvar = tables
        pd_mu, pd_logvar, _ = self.experts(torch.stack([v_mu, t_mu], dim=0), torch.stack([v_logvar, t_logvar], dim=0))
        return self.experts(torch.stack([pd_mu, c_mu], dim=0), torch.stack([pd_logvar, c_logvar], dim=0))[:2]

    def forward(self, keep=None, eps=None):
        """Model/MVGAE.py:315-342 in plain torch over the six tables (loss() does not come through here when fused_tail)."""
        tables = self._tables(keep)
        pd_mu, pd_logvar = self._poe(tables)
        z = self.reparametrize(pd_mu, pd_logvar, eps)
        if self.training:
            self.result_embed = pd_mu.detach()
        return (pd_mu, pd_logvar, z, *tables)

    def recon_loss(self, z, pos_edge_index, user, neg_items):
        """Model/MVGAE.py:344-362 (not on the training path)."""
        pos_scores = self.dot_product_decode(z, pos_edge_index, sigmoid=True)
        neg_scores = self.dot_product_decode_neg(z, user, neg_items, sigmoid=True)
        return -torch.sum(torch.log2(torch.sigmoid(pos_scores - neg_scores)))

    def kl_loss(self, mu, logvar):
        """Model/MVGAE.py:364-375."""
        logvar = logvar.clamp(max=MAX_LOGVAR)
        return -0.5 * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))

    def bpr_loss(self, users, pos_items, neg_items, z):
        """Model/MVGAE.py:377-390 (LOCAL item ids)."""
        user_embeddings = z[users]
        pos_item_embeddings = z[pos_items + self.num_user]
        neg_item_embeddings = z[neg_items + self.num_user]
        pos_scores = torch.sum(user_embeddings * pos_item_embeddings, dim=1)
        neg_scores = torch.sum(user_embeddings * neg_item_embeddings, dim=1)
        return -torch.mean(torch.log(torch.sigmoid(pos_scores - neg_scores) + 1e-5))

    def _plain_tail(self, tables, users, pos, neg, eps):
        """The reference's tail (Model/MVGAE.py:398-414) -> (total, parts [8], pd_mu)."""
        pd_mu, pd_logvar = self._poe(tables)
        views = [(pd_mu, pd_logvar)] + [(tables[2 * i], tables[2 * i + 1]) for i in range(3)]
        pos, neg = pos - self.num_user, neg - self.num_user
        bpr, kl = [], []
        for x, (m, l) in enumerate(views):
            z = self.reparametrize(m, l, eps[x].to(self.device) if eps is not None else None)
            bpr.append(self.bpr_loss(users, pos, neg, z))
            kl.append(self.kl_loss(m, l))
        total = sum(b + self.kl_weight * k for b, k in zip(bpr, kl))
        return total, torch.stack(bpr + kl).detach(), pd_mu

    def loss(self, users, pos_items, neg_items, keep=None, eps=None):
        """Model/MVGAE.py:392-416 -> scalar.  pos_items / neg_items: GLOBAL ids.  keep: the 3 x (n_layers + 2) dropout masks
        [U + I, D] in call order (12 at n_layers = 2); eps: the four noise tables [4, U + I, D] in the order P, V, T, C.
        Every call advances the step counter the device draws are keyed by, and a backward redraws with the counter as it
        stands THEN: call backward() before the next loss() (an evaluation-mode one included), as every training loop
        here does -- otherwise the backward differentiates other masks and noise than its forward drew."""
        users, pos, neg = (t.to(self.device).to(torch.int64) for t in (users, pos_items, neg_items))
        ops.mvgae_tick(self._state)
        tables = self._tables(keep)
        if self.fused_tail and self._fusable:
            if eps is not None:
                eps = torch.as_tensor(eps).to(self.device).float().contiguous()
            total, parts, pd_mu = ops.mvgae_tail(*tables, users, pos, neg, self.kl_weight, self._state, self.seed,
                                                       self.training, eps, row_ids=self._row_ids)
        else:
            total, parts, pd_mu = self._plain_tail(tables, users, pos, neg, eps)
        if self.training:
            self.result_embed = pd_mu.detach()
        self.last = dict(parts=parts, pd_mu=pd_mu.detach())
        return total.reshape(())

    def gene_ranklist(self, topk=50, to_cpu=True):
        """Model/MVGAE.py:418-443: scores of result_embed, history entries = 1e-6, top-k, + num_user."""
        return ranking.gene_ranklist(self.result_embed, self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                     state=ranking.state_of(self))

    full_sort_predict = gene_ranklist
