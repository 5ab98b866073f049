"""MacridVAE with the reference's surface (Model/MacridVAE.py:14-192), compute on HIP kernels (csrc/macridvae.hip).

Same constructor, attributes and parameters (`encoder.0.weight [600, I]`, `encoder.0.bias`, `encoder.2.weight [2D, 600]`,
`encoder.2.bias`, `item_embedding.weight [I, D]`, `k_embedding.weight [10, D]`), created and initialised by the
reference's own calls in its order (same torch seed -> same weights).  Kept as written: `update` is incremented BEFORE
the anneal is read (:135-137; MultVAE reads first); the KL has no mu^2 term (:146); the multi-hot row that multiplies
log_softmax is the raw one (:150); regs = [0, 0] makes reg_loss() unreachable (:153); gene_ranklist() sets
`training = False` and leaves it (:170) and masks history entries with the VALUE 1e-6 although the scores are logs in
about [-10, 10] (:182).

What changed underneath.  The reference builds per concept a [B, I] weighted input, logits and probabilities (and the
same on [U, I] in gene_ranklist).  Here `encoder.0.weight` is the transposed view of a row-major [I, 600] buffer whose
rows are gathered once per (sample, history entry) for all K concepts (ops.macrid_encode); the likelihood recomputes its
logits tile by tile on the f32 MFMA pipe (ops.macrid_mix); ranking stages the scores of a RANGE of users under a cap and
ranks them with an exact top-k kernel.  `update` lives in a device scalar a kernel advances; dropout flags, Gumbel noise
and epsilon come from a counter RNG keyed by it, so a captured step draws fresh values at every replay.
`loss(..., keep=, gumbel=, eps=)` takes GIVEN draws (parity tests).
"""
import torch
import torch.nn as nn

from .. import graph, ops, ranking


class MacridVAE(nn.Module):
    def __init__(self, num_user, num_item, edge_index, user_item_dict, dim_E, reg_weight, device):
        super(MacridVAE, self).__init__()
        self.num_user = num_user
        self.num_item = num_item
        self.user_item_dict = user_item_dict
        self.edge_index = edge_index
        self.dim_E = dim_E
        self.device = device
        self.training = True

        self.drop_out = 0.5
        self.kfac = 10
        self.layers = [600]
        self.tau = 0.1
        self.nogb = False
        self.regs = [0.0, 0.0]
        self.std = 0.01
        self.total_anneal_steps = 200000
        self.anneal_cap = 0.2
        ops.macrid_check_shape(dim_E, self.kfac, self.layers[0])
        self._state = torch.zeros(2, dtype=torch.int64, device=device)     # update, the count the step in flight is keyed by
        self._anneal = torch.zeros(1, dtype=torch.float32, device=device)
        self.update = 0

        # Model/MacridVAE.py:38-49, call for call (each module's own init consumes the generator before xavier_normal_)
        self.encode_layer_dims = [self.num_item] + self.layers + [self.dim_E * 2]
        self.encoder = self.mlp_layers(self.encode_layer_dims)
        self.item_embedding = nn.Embedding(self.num_item, self.dim_E)
        nn.init.xavier_normal_(self.item_embedding.weight)
        self.k_embedding = nn.Embedding(self.kfac, self.dim_E)
        nn.init.xavier_normal_(self.k_embedding.weight)
        # the first layer's weight row-major per item; the Parameter keeps the reference's name, shape and values
        w1_t = self.encoder[0].weight.detach().t().contiguous().to(device)
        self.encoder[0].weight = nn.Parameter(w1_t.t())
        self.to(device)

        e = torch.as_tensor(edge_index)
        rowptr, col = graph.user_hist_csr_from_edges(e.cpu().numpy() if e.is_cuda else e.numpy(), num_user)
        self.structure = ops.MultVAEStructure(rowptr, col, num_item).to(device)      # (rating_matrix, :52-55, as a CSR)
        rowptr, col = graph.user_hist_csr(user_item_dict, num_user)                 # gene_ranklist's mask (:180-182)
        self.hist = (rowptr.to(device), col.to(torch.int64).to(device))
        self.seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self.result = None
        self.last = {}

    def mlp_layers(self, layer_dims):
        """Linear layers over consecutive widths with a Tanh between them (none after the last)."""
        linears = [nn.Linear(a, b) for a, b in zip(layer_dims, layer_dims[1:])]
        mods = [linears[0]]
        for lin in linears[1:]:
            mods += [nn.Tanh(), lin]
        return nn.Sequential(*mods)

    # -- the reference's Python int, kept on the device (a captured step cannot bake it in) ---------------------
    @property
    def update(self):
        """Host mirror for logging (one device read)."""
        return int(self._state[0].item())

    @update.setter
    def update(self, value):
        self._state[0] = int(value)

    def capture_state_tensors(self):
        """Model state a captured training step updates in place (optim.GraphedTrainStep puts it back after warm-up)."""
        return [self._state, self._anneal]

    def _w1_t(self):
        w = self.encoder[0].weight
        if w.stride() != (1, w.shape[0]):
            raise RuntimeError("MacridVAE: encoder.0.weight must stay the transposed view of its row-major [I, 600] buffer")
        return w.t()

    def reparameterize(self, mu, logvar, eps=None):
        """Model/MacridVAE.py:66-72; eps (N(0, std^2), mu's shape): a given draw, None: the counter RNG."""
        if self.training:
            std = torch.exp(0.5 * logvar)
            if eps is None:
                eps = ops.macrid_normal(mu.shape, self._state, self.seed, self.std, mu.device)
            self.last["eps"] = eps
            return mu + eps * std
        return mu

    def forward(self, users, keep=None, gumbel=None, eps=None, batch=None):
        """Model/MacridVAE.py:74-128 for the history rows of `users`, without the [B, I] logits: -> (zh [B, K, D] = the
        normalised z of every (sample, concept), mulist, logvarlist); items and cates are left in self.last, the logits
        log p_bi exist only inside ops.macrid_mix / ops.macrid_scores.  keep: one flag per entry of the samples' history
        rows (sample 0's row first, CSR order); gumbel [I, K]: the noise added to the concept logits; eps [K, B, D]."""
        s, K, D = self.structure, self.kfac, self.dim_E
        if batch is None:
            users = users.to(self.device)
            batch = (users.to(torch.int64).contiguous(), None, None)
        B = batch[0].numel()
        keep_off = None
        if keep is not None and self.training:
            keep = keep.to(self.device)
            keep_off = s.keep_offsets(batch[0])
            n_flags = int((s.rowptr[batch[0] + 1] - s.rowptr[batch[0]]).sum())      # (given draws only: one host read)
            if keep.numel() != n_flags:
                raise ValueError(f"MacridVAE: {keep.numel()} keep flags for {n_flags} history entries of the batch")
        else:
            keep = None
        if gumbel is not None:
            gumbel = gumbel.to(self.device).float().contiguous()
        items, cates = ops.macrid_concept(self.item_embedding.weight, self.k_embedding.weight, self.tau, self._state, self.seed,
                                          self.training, gumbel)
        a = ops.macrid_encode(self._w1_t(), self.encoder[0].bias, cates, s, batch, self._state, self.seed, self.training,
                              1.0 - self.drop_out, keep, keep_off)
        h = ops.linear(torch.tanh(a).view(B * K, self.layers[0]), self.encoder[2].weight, self.encoder[2].bias)
        mu, logvar = ops.macrid_split(h)
        mu = ops.normalize_rows(mu)
        if eps is not None:
            eps = eps.to(self.device).float().reshape(K, B, D).permute(1, 0, 2).reshape(B * K, D).contiguous()
        z = self.reparameterize(mu, logvar, eps)
        zh = ops.normalize_rows(z).view(B, K, D)
        self.last.update(items=items, cates=cates, logvar=logvar)
        mu3, lv3 = mu.view(B, K, D), logvar.view(B, K, D)
        return zh, [mu3[:, k] for k in range(K)], [lv3[:, k] for k in range(K)]

    def loss(self, users, pos_items=None, neg_items=None, keep=None, gumbel=None, eps=None):
        """Model/MacridVAE.py:130-156 -> scalar."""
        s = self.structure
        users = users.to(self.device)
        batch = s.batch(users)
        ops.macrid_tick(self._state, self._anneal, self.anneal_cap, self.total_anneal_steps)
        self.last = {}
        zh, _, _ = self.forward(users, keep, gumbel, eps, batch=batch)
        logvar = self.last["logvar"]
        # sum_k -0.5 mean_b sum_d (1 + logvar - exp(logvar))  (:146, no mu^2 term) = 0.5 K D mean over all elements of
        # expm1(logvar) - logvar: the same number without rounding 1 + logvar at magnitude 1
        kl = 0.5 * (self.kfac * self.dim_E) * ops.mean_all(torch.expm1(logvar) - logvar)
        ce, lse = ops.macrid_mix(zh, self.last["items"], self.last["cates"], s, batch, self.tau)
        loss = ce + kl * self._anneal
        if self.regs[0] != 0 or self.regs[1] != 0:
            loss = loss + self.reg_loss()
        self.last.update(z=zh.detach(), lse=lse, ce=ce.detach(), kl=kl.detach(), anneal=self._anneal,
                         cates=self.last["cates"].detach(), items=self.last["items"].detach())
        return loss.reshape(())

    def reg_loss(self):
        """regs[0] * (|item_embedding| + |k_embedding|) + regs[1] * sum of the encoder weights' norms (Frobenius norms, torch
        ops; unreachable from loss() while regs = [0, 0])."""
        embeddings = self.item_embedding.weight.norm(2) + self.k_embedding.weight.norm(2)
        encoder = sum(p.norm(2) for n, p in self.encoder.named_parameters() if n.endswith("weight"))
        return self.regs[0] * embeddings + self.regs[1] * encoder

    def gene_ranklist(self, topk=50, to_cpu=True):
        """Model/MacridVAE.py:168-192.  The [U, I] score matrix never exists whole: users are taken in ranges whose fp32
        staging stays under ops.MACRID_STAGING_BYTES; each range is encoded in eval mode, scored (log p_ui, history
        entries = 1e-6) and ranked by the exact top-k kernel (ties to the lowest index)."""
        self.training = False          # (:170 -- and not set back; the training loop's model.train() does that)
        U, I = self.num_user, self.num_item
        step = ops.macrid_range_users(I)
        with torch.no_grad():
            self.last = {}
            out = torch.empty((U, topk), dtype=torch.int64, device=self.device)
            staging = torch.empty((min(U, step), I), dtype=torch.float32, device=self.device)
            for u0 in range(0, U, step):
                u1 = min(U, u0 + step)
                users = torch.arange(u0, u1, dtype=torch.int64, device=self.device)
                zh, _, _ = self.forward(users)
                sc = ops.macrid_scores(zh.contiguous(), self.last["items"], self.last["cates"], self.tau, u0, self.hist, 1e-6,
                                       out=staging[:u1 - u0])
                out[u0:u1], _ = ops.rows_topk(sc, topk, id_offset=U)
        return ranking._to_host(out) if to_cpu else out

    full_sort_predict = gene_ranklist
