"""LightGODE with the reference's surface (Model/LightGODE.py:33-177): matrix-factorisation training under an alignment +
uniformity loss, the graph only at evaluation as one explicit Euler step of dz/dt = A z + e.

Same constructor (plus `fused=`), parameters (`user_embedding`, `item_embedding`, xavier_normal_, created in the reference's
order: the same seed gives the same weights), `alignment`, `uniformity`, `forward(user, item)`, `get_ego_embeddings`,
`get_all_embeddings`, `loss`, `gene_ranklist`; `train_stage`, `train_strategy` ('MF_init': the raw tables while training, the ODE
in eval mode -- the reference's only setting; 'MF': never the ODE; 'GODE': the ODE in training too), `use_mf`, `t`, `gamma`,
`restore_user_e` / `restore_item_e` cached by gene_ranklist and cleared by every loss().

What changed underneath.

Training.  `loss` is ONE autograd node (ops.lightgode_loss, csrc/lightgode.hip): the 2 B rows are gathered and normalised, the
alignment mean and both uniformity terms log mean_{i<j} exp(-2 |z_i - z_j|^2) come out of one pass over the pairs on the f32
MFMA pipe together with the gradient by the gathered rows, in closed form -- no pdist vector, no [B, B] matrix -- and the
backward adds those rows into the tables in batch order, without atomics: a step is the same bits every run.

Evaluation.  odeint(f, x, [0, t], method='euler') without a step size is one step, x + t (A x + x): ops.lightgode_euler, the SpMM
kernel with its epilogue, one launch (the reference's order of operations up to rounding).  Under 'GODE' the loss
differentiates through it; A is symmetric, so the backward is the same launch.  The adjacency is graph.binary_sym_norm_csr
(degree + 1e-7, fp64, stored fp32: the reference's values), the ranking the shared ranking.gene_ranklist (mask 1e-6).

Fall-backs.  fused = False and dim_E != 64 run the reference's loss lines in plain torch (ops.lightgode_loss_plain); on a CPU
model loss, forward and get_all_embeddings run the reference's lines (gene_ranklist is the GPU ranking only).  The cache is also dropped whenever train() / eval() is called: a captured
step's replays do not run loss(), so the reference's clearing alone would leave a stale table behind them.

fused defaults to True because the measurement says so (profiles/lightgode_sports_bench.json, `fused_default`, written by
tools/bench_lightgode.py: at sports, B = 1024, D = 64 one eager training step takes 0.287 ms fused against 1.397 ms for the
reference's lines in plain torch, the node with its backward 0.095 ms against 1.257 ms, with a peak of 11.3 against 265.7 MiB
above the tables, 10.8 MiB of either being the table gradients).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import graph, ops, ranking

FUSED_WIDTH = 64


class LightGODE(nn.Module):
    def __init__(self, num_user, num_item, edge_index, user_item_dict, dim_E, gamma, t, device, fused=True):
        super(LightGODE, self).__init__()
        self.dim_E = dim_E
        self.num_user = num_user
        self.num_item = num_item
        self.gamma = gamma                                # uniformity weight
        self.train_stage = 'pretrain'
        self.train_strategy = 'MF_init'
        self.use_mf = None                                # 'MF': True, 'GODE': False, 'MF_init': follows self.training
        self.t = torch.tensor([0, t])
        self.solver = 'euler'
        self.user_item_dict = user_item_dict
        self.device = device
        self.fused = bool(fused)
        self.restore_user_e = None
        self.restore_item_e = None
        self.user_embedding = nn.Embedding(num_user, dim_E)
        self.item_embedding = nn.Embedding(num_item, dim_E)
        nn.init.xavier_normal_(self.user_embedding.weight)
        nn.init.xavier_normal_(self.item_embedding.weight)
        e = torch.as_tensor(edge_index).long()
        self.norm_adj = graph.binary_sym_norm_csr(e[:, 0], e[:, 1] - num_user, num_user, num_item).to(device)
        self.hist = ranking.history_csr(user_item_dict, num_user, device)

    @staticmethod
    def alignment(x, y, alpha=2):
        return (x - y).norm(p=2, dim=1).pow(alpha).mean()

    @staticmethod
    def uniformity(x, t=2):
        return torch.pdist(x, p=2).pow(2).mul(-t).exp().mean().log()

    def train(self, mode=True):
        self.restore_user_e, self.restore_item_e = None, None
        return super().train(mode)

    def _strategy_use_mf(self, in_forward):
        """:42-47, :106-107, :152-153: what `use_mf` is at this call."""
        if self.train_strategy == 'MF':
            return True
        if self.train_strategy == 'GODE':
            return False
        if in_forward and self.train_stage != 'pretrain':
            return self.use_mf
        return self.training

    def forward(self, user, item):
        self.use_mf = self._strategy_use_mf(True)
        user_embeddings, item_embeddings = self.get_all_embeddings()
        return F.normalize(user_embeddings[user], dim=-1), F.normalize(item_embeddings[item], dim=-1)

    def get_ego_embeddings(self):
        return torch.cat([self.user_embedding.weight, self.item_embedding.weight], dim=0)

    def euler(self, x):
        """odeint(odefunc1hop, x, [0, t], 'euler')[1]: one step of size t[1] - t[0] in the table's dtype."""
        if x.is_cuda:
            return ops.lightgode_euler(self.norm_adj, x, float((self.t[1] - self.t[0]).to(torch.float32)))
        a = self.norm_adj
        A = torch.sparse_csr_tensor(a.rowptr, a.col.long(), a.val.to(x.dtype), (a.n_rows, a.n_cols))
        t = self.t.type_as(x)
        return x + (t[1] - t[0]) * (A @ x + x)

    def get_all_embeddings(self):
        all_embeddings = self.get_ego_embeddings()
        if not self.use_mf:
            all_embeddings = self.euler(all_embeddings)
        return torch.split(all_embeddings, [self.num_user, self.num_item])

    def loss_parts(self, users, pos_items):
        """-> (loss, parts [4] = (loss, align, unif_u, unif_i)) for device ids, LOCAL item ids."""
        self.use_mf = self._strategy_use_mf(True)
        fused = self.fused and self.dim_E == FUSED_WIDTH and self.user_embedding.weight.is_cuda
        if self.use_mf:
            tab_u, tab_i, off = self.user_embedding.weight, self.item_embedding.weight, 0
        else:
            tab_u, tab_i, off = self.euler(self.get_ego_embeddings()), None, self.num_user
        return (ops.lightgode_loss if fused else ops.lightgode_loss_plain)(tab_u, tab_i, users, pos_items, self.gamma, off)

    def loss(self, users, pos_items, neg_items):
        pos_items = pos_items - self.num_user
        users, pos_items = users.to(self.device), pos_items.to(self.device)
        self.restore_user_e, self.restore_item_e = None, None
        return self.loss_parts(users, pos_items)[0]

    def gene_ranklist(self, topk=50, to_cpu=True):
        """:148-177 (mask value 1e-6; raw dot products of the tables, the ODE's in eval mode)."""
        if self.restore_user_e is None or self.restore_item_e is None:
            self.use_mf = self._strategy_use_mf(False)
            with torch.no_grad():
                self.restore_user_e, self.restore_item_e = self.get_all_embeddings()
        return ranking.gene_ranklist(self.restore_user_e.detach(), self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                      state=ranking.state_of(self), items=self.restore_item_e.detach())

    full_sort_predict = gene_ranklist
