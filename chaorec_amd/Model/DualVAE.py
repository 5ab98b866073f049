"""DualVAE with the reference's surface (Model/DualVAE.py:26-337), compute on HIP kernels (csrc/dualvae.hip).

Same constructor, attributes and the 18 parameters in the reference's order, created by the reference's own calls in its
order (same torch seed -> same values): user_preferences, item_topics [5, 25], then the draws of theta [U, 5, 25] and
beta [I, 5, 25], user_encoder.fc0 (I -> 20), user_mu, user_std, item_encoder.fc0 (U -> 20), item_mu, item_std,
user_decoder.fc_out0, item_decoder.fc_out0 (25 -> 20).  theta, beta, mu_theta, mu_beta are plain attributes (not in
state_dict) that to() moves.  Kept as written: dim_E is stored and unused (k = 25, a = 5, hidden 20, tanh, Poisson
likelihood, EPS = 1e-10); loss() runs the item side first and overwrites beta / mu_beta before the user side reads beta;
gene_ranklist() weights by the RAW sum_k mu_beta item_topics (its softmax only goes to aspect_probability) and sets
history entries to the VALUE 1e-6 although scores can be negative.

What changed underneath.  The reference builds per aspect a dense [B, U] / [B, I] batch, decoder output and weighted
copy (and [U, I] five times in gene_ranklist).  Here a batch row is a walk over a CSR row (ops.dualvae_encode: the
encoder weight is the transposed view of a row-major [N, 20] buffer gathered once per entry for all aspects), the decoder
output is recomputed tile by tile on the f32 MFMA pipe in every pass that needs it (ops.dualvae_dense -> sum p,
sum x log(p + EPS), nei), and ranking stages a RANGE of users under a cap.  Where an id repeats in the batch the sample
at the highest position writes its table row (the reference's CPU behaviour; undefined for index_put_ on a GPU).  The
item side reads a snapshot of theta, so its backward sees the table its forward saw although the user side has written
theta[users] in between.  `loss(..., eps_item=, eps_user=)` takes GIVEN draws [5, B, 25] in the reference's draw order;
otherwise epsilon comes from a counter RNG keyed by a device step counter, so a captured step draws fresh values at
every replay.
"""
import torch
import torch.nn as nn

from .. import graph, ops, ranking

EPS = 1e-10


class DualVAE(nn.Module):
    def __init__(self, num_user, num_item, edge_index, user_item_dict, dim_E, kl_weight, ssl_reg, device):
        super(DualVAE, self).__init__()
        self.num_user = num_user
        self.num_item = num_item
        self.user_item_dict = user_item_dict
        self.dim_E = dim_E
        self.device = device
        self.kl_weight = kl_weight
        self.ssl_reg = ssl_reg

        self.k = 25
        self.a = 5
        self.act_fn = nn.Tanh()
        self.likelihood = "pois"
        encoder_structure = [20]
        decoder_structure = [20]
        ops.dualvae_check_shape(self.k, self.a, encoder_structure[0])
        self.user_encoder_structure = [num_item] + encoder_structure
        self.item_encoder_structure = [num_user] + encoder_structure
        self.user_decoder_structure = [self.k] + decoder_structure
        self.item_decoder_structure = [self.k] + decoder_structure

        # Model/DualVAE.py:56-109, call for call (the generator is consumed in this order)
        self.mu_theta = torch.zeros((num_user, self.a, self.k))
        self.mu_beta = torch.zeros((num_item, self.a, self.k))
        self.user_preferences = nn.Parameter(nn.init.kaiming_uniform_(torch.empty(self.a, self.k), a=5 ** 0.5))
        self.item_topics = nn.Parameter(nn.init.kaiming_uniform_(torch.empty(self.a, self.k), a=5 ** 0.5))
        self.theta = torch.randn(num_user, self.a, self.k) * 0.01
        self.beta = torch.randn(num_item, self.a, self.k) * 0.01
        self.user_encoder = nn.Sequential()
        self.user_encoder.add_module("fc0", nn.Linear(num_item, encoder_structure[0]))
        self.user_encoder.add_module("act0", self.act_fn)
        self.user_mu = nn.Linear(encoder_structure[0], self.k)
        self.user_std = nn.Linear(encoder_structure[0], self.k)
        self.item_encoder = nn.Sequential()
        self.item_encoder.add_module("fc0", nn.Linear(num_user, encoder_structure[0]))
        self.item_encoder.add_module("act0", self.act_fn)
        self.item_mu = nn.Linear(encoder_structure[0], self.k)
        self.item_std = nn.Linear(encoder_structure[0], self.k)
        self.user_decoder = nn.Sequential()
        self.user_decoder.add_module("fc_out0", nn.Linear(self.k, decoder_structure[0]))
        self.user_decoder.add_module("act_out0", self.act_fn)
        self.item_decoder = nn.Sequential()
        self.item_decoder.add_module("fc_out0", nn.Linear(self.k, decoder_structure[0]))
        self.item_decoder.add_module("act_out0", self.act_fn)
        self.aspect_probability = None

        # the encoders' first weights row-major per table row; the Parameters keep the reference's names, shapes and values
        for enc in (self.user_encoder, self.item_encoder):
            w_t = enc.fc0.weight.detach().t().contiguous().to(device)
            enc.fc0.weight = nn.Parameter(w_t.t())
        self._eye = torch.eye(self.a, device=device)
        self._state = torch.zeros(2, dtype=torch.int64, device=device)      # the step count, the count the step in flight is keyed by
        self.to(device)

        e = torch.as_tensor(edge_index)
        rowptr, col = graph.user_hist_csr_from_edges(e.cpu().numpy() if e.is_cuda else e.numpy(), num_user)
        # samples = users over the item table, and its transpose: samples = items over the user table
        self.user_structure = ops.MultVAEStructure(rowptr, col, num_item)
        us = self.user_structure
        self.item_structure = ops.MultVAEStructure(us.item_ptr, us.item_users, num_user)
        self.user_structure.to(device)
        self.item_structure.to(device)
        rowptr, col = graph.user_hist_csr(user_item_dict, num_user)                 # gene_ranklist's mask (:325-327)
        self.hist = (rowptr.to(device), col.to(torch.int64).to(device))
        self.seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self.last = {}

    def to(self, device=None):
        """Model/DualVAE.py:113-118: everything goes to self.device, the four tables with it."""
        self.beta = self.beta.to(device=self.device)
        self.theta = self.theta.to(device=self.device)
        self.mu_beta = self.mu_beta.to(device=self.device)
        self.mu_theta = self.mu_theta.to(device=self.device)
        return super(DualVAE, self).to(self.device)

    def capture_state_tensors(self):
        """Model state a captured training step updates in place (optim.GraphedTrainStep puts it back after warm-up)."""
        return [self._state, self.theta, self.beta, self.mu_theta, self.mu_beta]

    @staticmethod
    def _enc_t(enc):
        w = enc.fc0.weight
        if w.stride() != (1, w.shape[0]):
            raise RuntimeError("DualVAE: an encoder's fc0.weight must stay the transposed view of its row-major [N, 20] buffer")
        return w.t()

    def _encode_dense(self, enc, mu, std, x):
        h = torch.tanh(ops.gemm_raw(x, self._enc_t(enc), bias=enc.fc0.bias))
        return ops.linear(h, mu.weight, mu.bias), torch.sigmoid(ops.linear(h, std.weight, std.bias))

    def encode_user(self, x):
        """Model/DualVAE.py:120-122 for GIVEN dense rows x [n, I] (inspection only: no gradient reaches fc0 from here; the
        training path never builds x)."""
        return self._encode_dense(self.user_encoder, self.user_mu, self.user_std, x)

    def encode_item(self, x):
        """Model/DualVAE.py:124-126 for GIVEN dense rows x [n, U] (see encode_user)."""
        return self._encode_dense(self.item_encoder, self.item_mu, self.item_std, x)

    def reparameterize(self, mu, std, eps=None):
        """Model/DualVAE.py:148-150; eps (mu's shape): a given draw, None: the counter RNG."""
        if eps is None:
            eps = ops.macrid_normal(mu.shape, self._state, self.seed, 1.0, mu.device)
        return mu + eps * std

    def contrast_loss(self, x, x_):
        """Model/DualVAE.py:152-177 for x, x_ [B, 5, 25] (temperature 0.2; negatives over the aspects of one sample and over
        the samples of one aspect)."""
        B, A = x.shape[0], x.shape[1]
        x = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        x_ = x_ / x_.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        pos_score = torch.exp(torch.sum(x_ * x, dim=-1) / 0.2)
        acl_score = torch.sum(x_.unsqueeze(2) * x.unsqueeze(1), dim=-1)                 # [B, 5, 5]: x_[b, a] . x[b, a']
        acl_score = torch.sum(torch.exp(acl_score / 0.2), dim=-1)
        xt, xt_ = x.transpose(0, 1).contiguous(), x_.transpose(0, 1).contiguous()      # [5, B, 25]
        ncl_score = torch.stack([torch.sum(torch.exp(ops.linear(xt_[a], xt[a]) / 0.2), dim=-1) for a in range(A)], dim=1)
        info_nec_loss = torch.log(pos_score / (acl_score + ncl_score))
        return -float(A) * ops.mean_all(info_nec_loss)                                 # -mean_b sum_a

    def forward(self, ids, user=True, beta=None, theta=None, eps=None, batch=None, parts=False):
        """Model/DualVAE.py:179-259 for the batch rows of `ids` (LOCAL ids of users, or of items with user=False) instead of
        their dense multi-hot rows -> (z [B, 5, 25], mu [B, 5, 25], (sum_n p_bn [B], sum_{n in row} log(p_bn + EPS) [B]),
        kl, cl): the [B, N] probabilities exist only inside ops.dualvae_dense.  eps [5, B, 25]: given draws.  parts: (mu, the
        pre-sigmoid std) [B 5, 25] in place of kl (what _loss() evaluates the KL from)."""
        A, K, H = self.a, self.k, 20
        if user:
            s, table, pref = self.user_structure, (self.beta if beta is None else beta), self.item_topics
            enc, mu_l, std_l, dec_s, dec_t = self.user_encoder, self.user_mu, self.user_std, self.user_decoder, self.item_decoder
        else:
            s, table, pref = self.item_structure, (self.theta if theta is None else theta), self.user_preferences
            enc, mu_l, std_l, dec_s, dec_t = self.item_encoder, self.item_mu, self.item_std, self.item_decoder, self.user_decoder
        if batch is None:
            batch = s.batch(ids.to(self.device))
        B, N = batch[0].numel(), table.shape[0]
        # sum_k table[n, a, k] pref[a, k] as ONE product against the block-diagonal [5, 125] weight: pref's gradient is then
        # a GEMM's fixed-order sum over the N rows (a broadcast product's backward is a multi-block torch reduction, which a
        # captured step must not hold: DESIGN 3.5)
        w_blocks = (self._eye.unsqueeze(2) * pref.unsqueeze(0)).reshape(A, A * K)
        w = torch.softmax(ops.linear(table.view(N, A * K), w_blocks), dim=1).contiguous()  # [N, 5]
        pre = ops.dualvae_encode(self._enc_t(enc), enc.fc0.bias, w, s, batch)            # [B, 5, 20]
        h = torch.tanh(pre).view(B * A, H)
        mu = ops.dualvae_linear(h, mu_l.weight, mu_l.bias)
        std_pre = ops.dualvae_linear(h, std_l.weight, std_l.bias)
        std = torch.sigmoid(std_pre)
        if parts:
            kl = (mu, std_pre)      # (_loss() evaluates and sums the KL's elements in double)
        else:
            # sum_a mean_b sum_k / 5 = 25 x the mean over all B 5 25 elements
            kl = float(K) * ops.mean_all(-0.5 * (1 + 2.0 * torch.log(std) - mu.pow(2) - std.pow(2)))
        if eps is not None:
            eps = eps.to(self.device).float().reshape(A, B, K).permute(1, 0, 2).reshape(B * A, K).contiguous()
        z = self.reparameterize(mu, std, eps)
        zh = torch.tanh(ops.dualvae_linear(z, dec_s.fc_out0.weight, dec_s.fc_out0.bias))
        th = torch.tanh(ops.dualvae_linear(table.view(N * A, K), dec_t.fc_out0.weight, dec_t.fc_out0.bias))
        z3 = z.view(B, A, K)
        sum_p, xlog, nei = ops.dualvae_dense(z3, zh.view(B, A, H), th.view(N, A, H), w, table, s, batch)
        cl = self.contrast_loss(z3, nei)
        self.last["user" if user else "item"] = dict(z=z3.detach(), mu=mu.view(B, A, K).detach(), nei=nei.detach(), cl=cl.detach())
        return z3, mu.view(B, A, K), (sum_p, xlog), kl, cl

    def _loss(self, sums, kl_parts, kl_beta, cl, cl_gama):
        """Model/DualVAE.py:261-274 with the Poisson likelihood from its two row sums and the KL from (mu, pre-sigmoid std)
        -> (loss, kl, ll), each from double sums and rounded once (the gradient flows through loss)."""
        sum_p, xlog = sums
        out = ops.dualvae_loss(kl_parts[0], kl_parts[1], xlog, sum_p, cl, kl_beta, cl_gama)
        return out[0], out[1].detach(), out[2].detach()

    def loss(self, users, pos_items, neg_items=None, eps_item=None, eps_user=None):
        """Model/DualVAE.py:276-303 -> scalar."""
        users = users.to(self.device).to(torch.int64)
        pos_items = pos_items.to(self.device).to(torch.int64) - self.num_user
        ops.dualvae_tick(self._state)
        self.last = {}
        B = users.numel()
        if (eps_item is None or eps_user is None) and pos_items.numel() == B:
            drawn = ops.macrid_normal((2, self.a, B, self.k), self._state, self.seed, 1.0, self.device)
            eps_item = drawn[0] if eps_item is None else eps_item
            eps_user = drawn[1] if eps_user is None else eps_user

        ib = self.item_structure.batch(pos_items)
        theta_seen = self.theta.clone()          # the user side writes theta[users] before backward() runs
        z_i, mu_i, sums, kl, cl = self.forward(pos_items, user=False, theta=theta_seen, eps=eps_item, batch=ib, parts=True)
        item_loss, kl_i, ll_i = self._loss(sums, kl, self.kl_weight, cl, self.ssl_reg)
        ops.dualvae_writeback(ib, self.num_item, z_i.detach().contiguous(), mu_i.detach().contiguous(), self.beta, self.mu_beta)

        ub = self.user_structure.batch(users)
        z_u, mu_u, sums, kl, cl = self.forward(users, user=True, beta=self.beta, eps=eps_user, batch=ub, parts=True)
        user_loss, kl_u, ll_u = self._loss(sums, kl, self.kl_weight, cl, self.ssl_reg)
        ops.dualvae_writeback(ub, self.num_user, z_u.detach().contiguous(), mu_u.detach().contiguous(), self.theta, self.mu_theta)

        self.last["item"].update(kl=kl_i, ll=ll_i, loss=item_loss.detach())
        self.last["user"].update(kl=kl_u, ll=ll_u, loss=user_loss.detach())
        return (item_loss + user_loss).reshape(())

    def gene_ranklist(self, topk=50, to_cpu=True):
        """Model/DualVAE.py:305-337.  The [U, I] score matrix never exists whole: users are taken in ranges whose fp32
        staging stays under ops.DUALVAE_STAGING_BYTES; each range is scored (the raw aspect weight, history entries = 1e-6)
        and ranked by the exact top-k kernel (ties to the lowest index)."""
        U, I, A, K = self.num_user, self.num_item, self.a, self.k
        step = ops.dualvae_range_users(I)
        with torch.no_grad():
            aspect_prob = torch.sum(self.mu_beta * self.item_topics, dim=-1).contiguous()      # [I, 5], used BEFORE the softmax
            self.aspect_probability = torch.softmax(aspect_prob, dim=1)
            dec_u, dec_i = self.user_decoder.fc_out0, self.item_decoder.fc_out0
            th = torch.tanh(ops.linear(self.mu_beta.view(I * A, K), dec_i.weight, dec_i.bias)).view(I, A, 20)
            out = torch.empty((U, topk), dtype=torch.int64, device=self.device)
            staging = torch.empty((min(U, step), I), dtype=torch.float32, device=self.device)
            for u0 in range(0, U, step):
                u1 = min(U, u0 + step)
                zu = self.mu_theta[u0:u1].contiguous()
                zh = torch.tanh(ops.linear(zu.view((u1 - u0) * A, K), dec_u.weight, dec_u.bias)).view(u1 - u0, A, 20)
                sc = ops.dualvae_scores(zu, zh, self.mu_beta, th, aspect_prob, u0, self.hist, 1e-6, out=staging[:u1 - u0])
                out[u0:u1], _ = ops.rows_topk(sc, topk, id_offset=U)
        return ranking._to_host(out) if to_cpu else out

    full_sort_predict = gene_ranklist
