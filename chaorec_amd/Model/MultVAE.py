"""MultVAE with the reference's surface (Model/MultVAE.py:16-195), compute on HIP kernels (csrc/multvae.hip).

Same constructor, parameters (`layers_q.0.weight [128, I]`, `layers_q.0.bias`, `layers_p.0.weight [I, 64]`,
`layers_p.0.bias`) created and initialised by the reference's own calls in its order (same torch seed -> same
weights), `loss()`, `gene_ranklist()`.  Kept as written: p_dims = [64] whatever dim_E says and no tanh anywhere (one
layer each side, :38, :83, :102); reg enters as reg_weight^2 * sum ||p||^2 over ALL parameters (:135, :158, :160);
anneal = min(0.2, update_count / 200 000) read before the increment (:145-148, :162); eps ~ N(0, 1) is drawn in eval() too
(:113), so gene_ranklist() is stochastic; history entries get the VALUE 1e-6 (:182).

What changed underneath.  The reference materialises the batch's [B, I] multi-hot rows, its logits and their
log_softmax.  Here a sample's row is a walk over hist(u_b); the encoder is a gather-sum of rows of the encoder weight,
which is therefore stored ROW-MAJOR PER ITEM, [I, 128] -- `layers_q.0.weight` is the transposed view of that buffer --,
and the likelihood is  n_b lse_b - sum_{i in hist(u_b)} logit_bi  with the logits recomputed tile by tile on the f32
MFMA pipe in the forward and in both backward passes (ops.multvae_encode / ops.multvae_decode: nothing [B, I] exists).
update_count lives in a device scalar a kernel advances, dropout mask and eps come from a counter RNG keyed by it: a
captured step draws fresh values at every replay.  `loss(..., keep=, eps=)` takes GIVEN draws (parity tests).
"""
import torch
import torch.nn as nn

from .. import graph, ops, ranking
from ..graph import CSR


class MultVAE(nn.Module):
    def __init__(self, num_user, num_item, edge_index, user_item_dict, dim_E, reg_weight, device):
        super(MultVAE, self).__init__()
        self.num_user = num_user
        self.num_item = num_item
        self.user_item_dict = user_item_dict
        self.edge_index = edge_index
        self.dim_E = dim_E
        self.reg_weight = reg_weight
        self.device = device
        self.keep_prob = 0.5
        self.total_anneal_steps = 200000
        self.anneal_cap = 0.2
        self.result = None
        p_dims = [ops.MULTVAE_LATENT]          # (Model/MultVAE.py:38: hard-wired, dim_E is not read)
        self.p_dims = p_dims + [self.num_item]
        self.q_dims = self.p_dims[::-1]
        if len(self.p_dims) != 2 or self.p_dims[0] != ops.MULTVAE_LATENT:
            raise ValueError(f"MultVAE: the kernels tile one layer each side with a latent width of {ops.MULTVAE_LATENT}")

        # Model/MultVAE.py:45-69, call for call (nn.Linear's own init consumes the generator before uniform_ does)
        self.layers_q = nn.ModuleList()
        layer = nn.Linear(self.q_dims[0], 2 * self.q_dims[1], bias=True)
        nn.init.uniform_(layer.weight)
        nn.init.uniform_(layer.bias)
        self.layers_q.append(layer)
        self.layers_p = nn.ModuleList()
        layer = nn.Linear(self.p_dims[0], self.p_dims[1], bias=True)
        nn.init.uniform_(layer.weight)
        nn.init.uniform_(layer.bias)
        self.layers_p.append(layer)
        # the encoder weight row-major per item; the Parameter keeps the reference's name, shape and values
        wq_t = self.layers_q[0].weight.detach().t().contiguous().to(device)
        self.layers_q[0].weight = nn.Parameter(wq_t.t())
        self.to(device)

        # the edges' interactions (train_csr_mat, :32-35: a repeated edge would count twice there; the data has none)
        e = torch.as_tensor(edge_index)
        rowptr, col = graph.user_hist_csr_from_edges(e.cpu().numpy() if e.is_cuda else e.numpy(), num_user)
        self.structure = ops.MultVAEStructure(rowptr, col, num_item).to(device)
        rowptr, col = graph.user_hist_csr(user_item_dict, num_user)       # gene_ranklist's mask (:180-182)
        self.hist = (rowptr.to(device), col.to(device))
        self._state = torch.zeros(2, dtype=torch.int64, device=device)     # update_count, the count the step in flight reads
        self._anneal = torch.zeros(1, dtype=torch.float32, device=device)
        self.seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self._enc_csr = None
        self.last = {}

    # -- the reference's Python float, kept on the device (a captured step cannot bake it in) -------------------
    @property
    def update_count(self):
        """Host mirror for logging (one device read)."""
        return float(self._state[0].item())

    @update_count.setter
    def update_count(self, value):
        self._state[0] = int(value)

    def capture_state_tensors(self):
        """Model state a captured training step updates in place (optim.GraphedTrainStep puts it back after warm-up)."""
        return [self._state, self._anneal]

    def _wq_t(self):
        w = self.layers_q[0].weight
        if w.stride() != (1, w.shape[0]):
            raise RuntimeError("MultVAE: layers_q.0.weight must stay the transposed view of its row-major [I, 128] buffer")
        return w.t()

    def loss(self, users, pos_items=None, neg_items=None, keep=None, eps=None):
        """Model/MultVAE.py:138-164 -> scalar.  keep (one flag per entry of the samples' history rows, sample 0's row
        first, CSR order) and eps [B, 64]: given draws; None: the counter RNG."""
        s = self.structure
        users = users.to(self.device)
        batch = s.batch(users)
        ops.multvae_tick(self._state, self._anneal, self.anneal_cap, self.total_anneal_steps)
        keep_off = None
        if keep is not None:
            keep = keep.to(self.device)
            keep_off = s.keep_offsets(batch[0])
            n_flags = int((s.rowptr[batch[0] + 1] - s.rowptr[batch[0]]).sum())      # (given draws only: one host read)
            if keep.numel() != n_flags:
                raise ValueError(f"MultVAE.loss: {keep.numel()} keep flags for {n_flags} history entries of the batch")
        if eps is not None:
            eps = eps.to(self.device).float().contiguous()
        z, kl, sq_q, h, eps_used = ops.multvae_encode(self._wq_t(), self.layers_q[0].bias, s, batch, self._state, self.seed,
                                                      self.training, self.keep_prob, keep, keep_off, eps)
        neg_ll, sq_p, lse = ops.multvae_decode(z, self.layers_p[0].weight, self.layers_p[0].bias, s, batch)
        # 2 * reg_loss = 2 * reg_weight * (reg_weight * 0.5 * sum ||p||^2)  (:135, :158, :160)
        reg2 = self.reg_weight * (self.reg_weight * 0.5 * (sq_q + sq_p)) * 2
        loss = neg_ll + self._anneal * kl + reg2
        self.last = {"z": z.detach(), "lse": lse, "h": h, "eps": eps_used, "neg_ll": neg_ll.detach(), "kl": kl.detach(),
                     "anneal": self._anneal, "sumsq": (sq_q + sq_p).detach()}
        return loss.reshape(())

    def _encoder_csr(self):
        """The normalised history rows (value 1 / sqrt(n_u), F.normalize of :78) as a fixed CSR [U, I]."""
        if self._enc_csr is None:
            s = self.structure
            n = (s.rowptr[1:] - s.rowptr[:-1]).to(torch.float32)
            val = torch.repeat_interleave(1.0 / torch.clamp(torch.sqrt(n), min=1e-12), s.rowptr[1:] - s.rowptr[:-1])
            self._enc_csr = CSR(s.rowptr, s.col, val.contiguous(), self.num_user, self.num_item)
        return self._enc_csr

    def latent(self, eps=None):
        """z for ALL users (:169-171 without the dense rows): the encoder is the existing SpMM at D = 128."""
        with torch.no_grad():
            h = ops.spmm_raw(self._encoder_csr(), self._wq_t().detach()) + self.layers_q[0].bias.detach()
            mu, logvar = h[:, :ops.MULTVAE_LATENT], h[:, ops.MULTVAE_LATENT:]
            if eps is None:
                eps = torch.randn(mu.shape, dtype=torch.float32, device=mu.device)
            return mu + eps.to(mu.device) * torch.exp(0.5 * logvar)

    def gene_ranklist(self, topk=50, to_cpu=True, eps=None):
        """Model/MultVAE.py:166-195 (mask value 1e-6).  score = z . Wp^T + bp through the bias-free scoring kernels:
        user rows [z | 1 | 0 ...], item rows [Wp | bp | 0 ...] at width 128 (the k-ascending chain gains + 1 * b, then
        + 0 * 0 terms)."""
        D = ops.MULTVAE_LATENT
        with torch.no_grad():
            z = self.latent(eps)
            ue = z.new_zeros((self.num_user, 2 * D))
            ue[:, :D] = z
            ue[:, D] = 1.0
            ie = z.new_zeros((self.num_item, 2 * D))
            ie[:, :D] = self.layers_p[0].weight.detach()
            ie[:, D] = self.layers_p[0].bias.detach()
            self.result = torch.cat((ue, ie), 0)
        return ranking.gene_ranklist(self.result, self.num_user, self.num_item, self.hist, 1e-6, topk, to_cpu=to_cpu,
                                      state=ranking.state_of(self))

    full_sort_predict = gene_ranklist
