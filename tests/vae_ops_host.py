"""Per-op torch restatements of the autoencoder ops (chaorec_amd/ops_extra.py over csrc/multvae.hip, macridvae.hip,
dualvae.hip and csrc/vae_common.h), each on the DENSE form of its inputs and with its gradients taken by torch.autograd,
plus THE numpy uint64 restatement of the counter RNG (mix64 of csrc/common.h; draw_key, draw_uniform<BITS> of csrc/draws.h,
here under the names vae_key, vae_uniform): mvgae_host, dragon_host and the graph models' GPU tests import it.
A helper module, not a conftest: imported by tests/test_vae_ops_host.py, which chains the ops into one step of each model against multvae_host / macridvae_host / dualvae_host (themselves tied to the reference's goldens).
It is the oracle for comparing the kernels op by op: each op alone, any upstream gradient, any mask.
The ranking half (macrid_scores, dualvae_scores, masked) restates what gene_ranklist stages: tests/test_gpu_vae_rank_ops.py.

Every `*_fwd` function is plain torch on tensors of one dtype: run in float64 it is the oracle, run in float32 on the same
inputs it is "the reference arithmetic's own rounding" a bound is taken from.  `run()` is the numpy front: inputs in,
outputs and gradients for GIVEN upstream gradients out.  The [B, I] matrices exist here on purpose."""
import numpy as np
import torch

MULTVAE_LATENT = 64
MACRID_K, MACRID_D, MACRID_H = 10, 64, 600
DUALVAE_A, DUALVAE_K, DUALVAE_H = 5, 25, 20
DUALVAE_EPS = 1e-10
DUALVAE_LINEAR_SPLIT = 2048                     # rows per split of the small Linears' weight gradient (DV_GW_ROWS)

# the salts and bit counts of the dropout draws (csrc/multvae.hip, csrc/macridvae.hip)
MULTVAE_SALT_KEEP, MULTVAE_BITS = 0x6D756C7476616531, 24
MACRID_SALT_KEEP, MACRID_BITS = 0x6D61637269643031, 23


# ---------------------------------------------------------------------------------------------------------------
# the counter RNG, exactly: uint64 arithmetic wraps, the uniform is built in float32 as the device builds it
# ---------------------------------------------------------------------------------------------------------------
def _u64(x):
    return np.asarray(x).astype(np.uint64)


def mix64(z):
    """splitmix64's finaliser (csrc/common.h)."""
    with np.errstate(over="ignore"):
        z = _u64(z) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def vae_key(seed, step, salt):
    with np.errstate(over="ignore"):
        return mix64(mix64(_u64(seed) ^ _u64(salt)) + _u64(step))


def vae_uniform(key, a, b, bits):
    """((r >> (64 - bits)) + 0.5) / 2^bits in float32, r = mix64(key ^ mix64((a << 32) ^ b)); a, b broadcast."""
    with np.errstate(over="ignore"):
        r = mix64(_u64(key) ^ mix64((_u64(a) << np.uint64(32)) ^ _u64(b)))
    top = (r >> np.uint64(64 - bits)).astype(np.float32)
    return (top + np.float32(0.5)) * np.float32(1.0 / float(1 << bits))


def ragged_rows():
    """rowptr, col of the 40-node graph the graph models' device draws are pinned on: row 3 holds 70 entries (more than a
    wave: the whole-wave path), row 7 none, the others 0 .. 9; 40 is no multiple of the 32 rows of a workgroup nor of the 8 of
    a wave.  Columns repeat: the draws are keyed by the entry's place alone."""
    lens = np.array([(3 * n + 1) % 10 for n in range(40)])
    lens[3], lens[7] = 70, 0
    rowptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    col = np.concatenate([(n + 1 + np.arange(k)) % 40 for n, k in enumerate(lens)]).astype(np.int32)
    return rowptr, col


def ragged_structure(device):
    """ragged_rows as a graph.DropoutStructure on `device` (the launches drawn on it read no transposed entry)."""
    from chaorec_amd import graph
    rowptr, col = (torch.from_numpy(v) for v in ragged_rows())
    E = col.numel()
    entry_row = torch.repeat_interleave(torch.arange(40, dtype=torch.int32), rowptr[1:] - rowptr[:-1])
    csr = graph.CSR(rowptr, col, torch.ones(E), 40, 40, symmetric=True)
    return graph.DropoutStructure(csr, entry_row, torch.arange(E, dtype=torch.int32)).to(device)


def predict_keep(seed, step, salt, bits, keep_prob, rowptr, col, users, I):
    """The dense [B, I] mask the device-drawn forward uses: entry j of sample b's history row is kept iff
    uniform(key, b, j) < keep_prob (VaeKeep: b = the sample's place in the batch, j = the entry's place in its row)."""
    key = vae_key(seed, step, salt)
    mask = np.zeros((len(users), I), dtype=bool)
    for b, u in enumerate(np.asarray(users)):
        c = col[rowptr[u]:rowptr[u + 1]]
        u01 = vae_uniform(key, np.full(len(c), b), np.arange(len(c)), bits)
        mask[b, c] = u01 < np.float32(keep_prob)
    return mask


# ---------------------------------------------------------------------------------------------------------------
# shared pieces
# ---------------------------------------------------------------------------------------------------------------
def dense_rows(rowptr, col, ids, N):
    """[B, N] multi-hot float64 numpy rows of the samples `ids`."""
    x = np.zeros((len(ids), N), dtype=np.float64)
    for b, u in enumerate(np.asarray(ids)):
        x[b, col[rowptr[u]:rowptr[u + 1]]] = 1.0
    return x


def unit_rows(x):
    return x / torch.clamp(x.norm(dim=-1, keepdim=True), min=1e-12)


def _scaled_rows(x, mask, keep_prob, training):
    """F.normalize of the multi-hot rows, then dropout's mask / keep_prob in training (the kernels' vae_row_scale)."""
    s = 1.0 / torch.clamp(x.sum(1).sqrt(), min=1e-12)
    if training:
        s = s / keep_prob
        if mask is not None:
            x = x * mask
    return x * s[:, None]


def _touched(xs):
    """The columns some sample holds: the encoders' dense products run over these alone (every other row of the weight
    meets zeros only; indexing leaves its gradient at exactly zero)."""
    return torch.nonzero((xs != 0).any(0))[:, 0]


# ---------------------------------------------------------------------------------------------------------------
# MultVAE
# ---------------------------------------------------------------------------------------------------------------
def multvae_encode_fwd(Wq_t, bq, x, mask, eps, keep_prob=0.5, training=True):
    """Wq_t [I, 128], bq [128], x / mask [B, I], eps [B, 64] -> h [B, 128], z [B, 64], kl [], sumsq []."""
    D = MULTVAE_LATENT
    xs = _scaled_rows(x, mask, keep_prob, training)
    idx = _touched(xs)
    h = xs[:, idx] @ Wq_t[idx] + bq
    mu, lv = h[:, :D], h[:, D:]
    z = mu + eps * torch.exp(0.5 * lv)
    kl = torch.sum(0.5 * (-lv + lv.exp() + mu.pow(2) - 1), dim=1).mean()
    return {"h": h, "z": z, "kl": kl, "sumsq": (Wq_t ** 2).sum() + (bq ** 2).sum()}


def multvae_decode_fwd(z, Wp, bp, x):
    """z [B, 64], Wp [I, 64], bp [I], x [B, I] -> neg_ll [], lse [B], nll [B], sumsq []."""
    logits = z @ Wp.t() + bp
    lse = torch.logsumexp(logits, dim=-1)
    nll = x.sum(1) * lse - (logits * x).sum(1)
    return {"neg_ll": nll.mean(), "lse": lse, "nll": nll, "sumsq": (Wp ** 2).sum() + (bp ** 2).sum()}


# ---------------------------------------------------------------------------------------------------------------
# MacridVAE
# ---------------------------------------------------------------------------------------------------------------
def macrid_concept_fwd(E, Kemb, gumbel, tau=0.1):
    """E [I, D], Kemb [K, D], gumbel [I, K] (the noise added to the logits) or None -> items [I, D], cates [I, K]."""
    items, cores = unit_rows(E), unit_rows(Kemb)
    cl = items @ cores.t() / tau
    if gumbel is not None:
        cl = cl + gumbel
    return {"items": items, "cates": torch.softmax(cl, dim=1)}


def macrid_encode_fwd(W1_t, b1, cates, x, mask, keep_prob=0.5, training=True):
    """W1_t [I, 600], b1 [600], cates [I, K], x / mask [B, I] -> a [B, K, 600]."""
    xs = _scaled_rows(x, mask, keep_prob, training)
    idx = _touched(xs)
    xi, Wi, ci = xs[:, idx], W1_t[idx], cates[idx]
    a = torch.stack([xi @ (ci[:, k:k + 1] * Wi) for k in range(cates.shape[1])], 1)
    return {"a": a + b1}


def macrid_mix_fwd(zh, items, cates, x, tau=0.1):
    """zh [B, K, D], items [I, D], cates [I, K], x [B, I] -> ce [], lse [B]."""
    p = None
    for k in range(cates.shape[1]):
        pk = torch.exp(zh[:, k] @ items.t() / tau) * cates[:, k][None, :]
        p = pk if p is None else p + pk
    lse = torch.log(p.sum(1))
    ce = (x.sum(1) * lse - (torch.log(p) * x).sum(1)).mean()
    return {"ce": ce, "lse": lse}


# ---------------------------------------------------------------------------------------------------------------
# DualVAE
# ---------------------------------------------------------------------------------------------------------------
def dualvae_encode_fwd(We_t, bias, w, x):
    """We_t [N, 20], bias [20], w [N, 5], x [B, N] -> pre [B, 5, 20]."""
    idx = _touched(x)
    xi, Wi, wi = x[:, idx], We_t[idx], w[idx]
    pre = torch.stack([xi @ (wi[:, a:a + 1] * Wi) for a in range(w.shape[1])], 1)
    return {"pre": pre + bias}


def dualvae_dense_fwd(z, zh, th, w, table, x):
    """z [B, 5, 25], zh [B, 5, 20], th [N, 5, 20], w [N, 5], table [N, 5, 25], x [B, N] -> sum_p [B], xlog [B],
    nei [B, 5, 25]."""
    probs, neis = 0.0, []
    for a in range(w.shape[1]):
        pa = torch.sigmoid(z[:, a] @ table[:, a].t() + torch.tanh(zh[:, a] @ th[:, a].t())) * w[:, a]
        probs = probs + pa
        neis.append(pa @ table[:, a])
    return {"sum_p": probs.sum(1), "xlog": (x * torch.log(probs + DUALVAE_EPS)).sum(1), "nei": torch.stack(neis, 1)}


def dualvae_linear_fwd(x, weight, bias):
    return {"y": x @ weight.t() + bias}


def dualvae_loss_fwd(mu, std_pre, xlog, sum_p, cl, kl_weight, ssl_reg):
    """mu, std_pre [B * 5, 25], xlog, sum_p [B], cl [] -> out [3] = (kl_weight kl - ll + ssl_reg cl, kl, ll)."""
    B = xlog.shape[0]
    std = torch.sigmoid(std_pre)
    kl = (-0.5 * (1 + 2.0 * torch.log(std) - mu ** 2 - std ** 2)).sum() / (DUALVAE_A * B)
    ll = (xlog - sum_p).sum() / B
    return {"out": torch.stack((kl_weight * kl - ll + ssl_reg * cl, kl, ll))}


def dualvae_contrast(x, x_):
    """Model/DualVAE.py's contrast loss of z and nei [B, 5, 25] (torch glue in the model, restated for the chained step)."""
    x, x_ = unit_rows(x), unit_rows(x_)
    pos = torch.exp((x_ * x).sum(-1) / 0.2)
    acl = torch.exp(torch.einsum("bak,bck->bac", x_, x) / 0.2).sum(-1)
    ncl = torch.exp(torch.einsum("bak,cak->bac", x_, x) / 0.2).sum(-1)
    return -torch.log(pos / (acl + ncl)).sum(-1).mean()


# ---------------------------------------------------------------------------------------------------------------
# the ranking half: the scores gene_ranklist stages, and the mask over them
# ---------------------------------------------------------------------------------------------------------------
def macrid_scores(zh, items, cates, tau):
    """zh [n, K, D], items [I, D], cates [I, K] -> [n, I]: log sum_k cates[i, k] exp(<zh[u, k], items[i]> / tau)."""
    p = 0.0
    for k in range(cates.shape[1]):
        p = p + cates[:, k] * torch.exp(zh[:, k] @ items.t() / tau)
    return torch.log(p)


def dualvae_scores(z, zh, table, th, w):
    """z [n, 5, 25], zh [n, 5, 20], table [I, 5, 25], th [I, 5, 20], w [I, 5] (as given: no softmax) -> [n, I]:
    sum_a w[i, a] sigmoid(z_ua . table_ia + tanh(zh_ua . th_ia))."""
    s = 0.0
    for a in range(w.shape[1]):
        s = s + w[:, a] * torch.sigmoid(z[:, a] @ table[:, a].t() + torch.tanh(zh[:, a] @ th[:, a].t()))
    return s


def masked(scores, rowptr, col, user_begin, mask_value):
    """A copy of the numpy block scores [n, I] with row r's entries at the history columns of user user_begin + r set to
    mask_value; a column outside [0, I) is ignored."""
    out = np.array(scores)
    I = out.shape[1]
    for r in range(out.shape[0]):
        c = np.asarray(col[rowptr[user_begin + r]:rowptr[user_begin + r + 1]], dtype=np.int64)
        out[r, c[(c >= 0) & (c < I)]] = mask_value
    return out


# ---------------------------------------------------------------------------------------------------------------
# numpy front
# ---------------------------------------------------------------------------------------------------------------
def run(fwd, inputs, wrt=(), upstream=None, dtype=torch.float64, **const):
    """fwd(**inputs as tensors of `dtype`, **const) -> (outputs, gradients), both dicts of float64 numpy arrays.
    inputs: name -> array (None passes through); wrt: the input names to differentiate; upstream: output name -> the
    gradient fed into it (the loss is sum over these of <output, gradient>, so any upstream gradient can be given)."""
    t = {k: (None if v is None else torch.as_tensor(np.asarray(v)).to(dtype).clone()) for k, v in inputs.items()}
    for k in wrt:
        t[k].requires_grad_(True)
    out = fwd(**t, **const)
    grads = {}
    if wrt:
        loss = sum((out[k] * torch.as_tensor(np.asarray(g)).to(dtype)).sum() for k, g in upstream.items())
        grads = {k: g.detach().double().numpy() for k, g in zip(wrt, torch.autograd.grad(loss, [t[k] for k in wrt]))}
    return {k: v.detach().double().numpy() for k, v in out.items()}, grads


# ---------------------------------------------------------------------------------------------------------------
# the per-row measure of an op-level comparison
# ---------------------------------------------------------------------------------------------------------------
ROW_FLOOR = 1e-3
BOUND_FLOOR = 2.0 ** -22          # four fp32 roundings


def row_dev(x, ref):
    """Per output row (first index; a vector's elements are rows of one, a scalar is one row): the row's largest |error|
    over its largest |ref|, rows below ROW_FLOOR x the tensor's largest |ref| normed by that floor; the maximum over rows."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    x, ref = x.reshape(max(1, x.shape[0] if x.ndim else 1), -1), ref.reshape(max(1, ref.shape[0] if ref.ndim else 1), -1)
    top = float(np.abs(ref).max())
    if top == 0.0:
        return float(np.abs(x).max())
    norm = np.maximum(np.abs(ref).max(axis=1), ROW_FLOOR * top)
    return float((np.abs(x - ref).max(axis=1) / norm).max())


def bound_of(ref32, ref64):
    """4 x the float32 restatement's own deviation from the float64 one, at least BOUND_FLOOR."""
    return max(4.0 * row_dev(ref32, ref64), BOUND_FLOOR)
