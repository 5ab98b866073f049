"""Host side of the CF_Diff tests: the small case, the float64 restatement of CAM_AE and of the attention's backward identities,
and the keep-bit keying of csrc/cfdiff.hip restated in numpy.  Shared by tests/golden/gen_cfdiff.py, tests/test_cfdiff_host.py and
tests/test_gpu_cfdiff.py."""
import functools
import math
import os

import accept
import numpy as np
import torch
from accept import EPS32 as ULP, user_item_dict  # noqa: F401

ZERO_REF = "absolute"            # an all-zero reference compares absolutely here and in DiffRec's tests, which share this module
rel_dev = functools.partial(accept.rel_dev, zero_ref=ZERO_REF)
FIXTURE = "cfdiff_small.npz"
U, I = 12, 48                    # user 11 has no history; items 44 .. 47 have no users; item 0 is held by every user with a history
EMPTY_ITEMS = 4
STEPS, NOISE_SCALE, NOISE_MIN, NOISE_MAX = 10, 0.1, 0.0005, 0.005
DIM_INTERS, EMB = 1024, 10       # the reference hard-codes both: L = 1034
TOPK = 10
TS = np.array([0, 9, 3, 5, 0, 9, 1, 2, 7, 4, 6, 8], dtype=np.int64)      # one per user; 0 and steps - 1 twice each
STEP_USERS = np.array([3, 11], dtype=np.int64)                      # the batch of the one-step gradient check
WEIGHTS = ["emb_layer.weight", "emb_layer.bias", "forward_layers.0.weight", "forward_layers.0.bias", "forward_layers.1.weight",
           "forward_layers.1.bias", "first_hop_embedding.weight", "first_hop_embedding.bias", "first_hop_decoding.weight",
           "first_hop_decoding.bias", "second_hop_embedding.weight", "second_hop_embedding.bias", "encoder.weight", "encoder.bias",
           "decoder.weight", "decoder.bias"] + [f"self_attentions.{i}.{n}" for i in range(2)
                                                for n in ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")]


def load_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, FIXTURE), allow_pickle=False)


def small_case(seed=5):
    """edges int64 [E, 2] (user, global item id), unique, sorted."""
    rng = np.random.RandomState(seed)
    pairs = set()
    for u in range(U - 1):
        pairs.add((u, 0))
        for i in rng.choice(np.arange(1, I - EMPTY_ITEMS), rng.randint(2, 9), replace=False):
            pairs.add((u, int(i)))
    e = np.array(sorted(pairs), dtype=np.int64)
    e[:, 1] += U
    return e


def dense_rows(edges):
    x = np.zeros((U, I), dtype=np.float32)
    x[edges[:, 0], edges[:, 1] - U] = 1.0
    return x


def sec_hop_rows(edges):
    """dataload.py:238-256 restated: cnt[i] / U (fp32, as torch.sum(data, 0) / num_user) where the user holds item i."""
    x = dense_rows(edges)
    return x * (x.sum(0, dtype=np.float32) / np.float32(U))[None, :]


# ---- the float64 (or any dtype) restatement ------------------------------------------------------------------------------------
def attention(q, k, v, keep=None):
    """4 heads of width 4, scores <q, k> / 2, softmax over all keys, then the rate-1/2 dropout with given flags [B, 4, L, L]."""
    B, L, _ = q.shape

    def heads(t):
        return t.reshape(B, L, 4, 4).permute(0, 2, 1, 3)

    P = torch.softmax(heads(q) @ heads(k).transpose(2, 3) * 0.5, dim=-1)
    if keep is not None:
        P = P * (keep.to(P.dtype) * 2.0)
    return (P @ heads(v)).permute(0, 2, 1, 3).reshape(B, L, 16)


def attention_backward(q, k, v, dout, keep=None):
    """The identities csrc/cfdiff.hip's backward uses, written out per head -> (out, dq, dk, dv)."""
    B, L, _ = q.shape

    def heads(t):
        return t.reshape(B, L, 4, 4).permute(0, 2, 1, 3)

    def merge(t):
        return t.permute(0, 2, 1, 3).reshape(B, L, 16)

    qh, kh, vh, gh = heads(q), heads(k), heads(v), heads(dout)
    P = torch.softmax(qh @ kh.transpose(2, 3) * 0.5, dim=-1)
    K2 = torch.full_like(P, 1.0) if keep is None else keep.to(P.dtype) * 2.0
    out = (P * K2) @ vh
    D = (gh * out).sum(-1, keepdim=True)
    dS = P * (K2 * (gh @ vh.transpose(2, 3)) - D)
    return merge(out), merge(0.5 * dS @ kh), merge(0.5 * dS.transpose(2, 3) @ qh), merge((P * K2).transpose(2, 3) @ gh)


def time_embedding(ts, dim=EMB):
    """CAM_AE.timestep_embedding: fp32 arithmetic, as the reference's (the float64 restatement takes its fp32 values)."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    args = ts[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def cam_ae(w, x, x_sec_hop, ts, keeps=None):
    """CAM_AE.forward (Model/CF_Diff.py:75-135) over a dict of its used weights, in their dtype.  keeps None: eval mode; else the
    given flags of the four dropouts (chaorec_amd.Model.CF_Diff.CAM_AE.forward's layout)."""
    dt = w["encoder.weight"].dtype
    B = x.shape[0]

    def lin(name, t):
        return t @ w[name + ".weight"].T + w[name + ".bias"]

    e, hs = lin("encoder", x.to(dt)), lin("encoder", x_sec_hop.to(dt))
    emb = lin("emb_layer", time_embedding(ts).to(dt))
    if keeps is not None:
        e = e * (keeps["drop"].to(dt) * (1.0 / (1.0 - 0.5)))
    h = lin("first_hop_embedding", torch.cat([e, emb], -1).unsqueeze(-1))
    hs = lin("second_hop_embedding", torch.cat([hs, emb], -1).unsqueeze(-1))
    for i in range(2):
        p = f"self_attentions.{i}."
        W, b = w[p + "in_proj_weight"], w[p + "in_proj_bias"]
        q, k, v = hs @ W[:16].T + b[:16], h @ W[16:32].T + b[16:32], h @ W[32:].T + b[32:]
        a = attention(q, k, v, None if keeps is None else keeps["attn"][i]) @ w[p + "out_proj.weight"].T + w[p + "out_proj.bias"]
        if keeps is not None:
            a = a * (keeps["drop1"][i].to(dt) * (1.0 / (1.0 - 0.8)))
        h = h + a
        if keeps is not None:
            h = h * (keeps["drop2"][i].to(dt) * (1.0 / (1.0 - 0.5)))
        h = lin(f"forward_layers.{i}", h)
        if i != 1:
            h = torch.tanh(h)
    return lin("decoder", torch.tanh(lin("first_hop_decoding", h).reshape(B, -1)))


def weights_of(g, dtype=torch.float64):
    return {n: torch.from_numpy(np.asarray(g["w_" + n])).to(dtype) for n in WEIGHTS}


def load_weights(model, g):
    """The golden's CAM_AE weights into a chaorec_amd.Model.CF_Diff model (every tensor of its state_dict is one of them)."""
    sd = model.CAM_AE.state_dict()
    assert sorted(sd) == sorted(WEIGHTS), sorted(set(sd) ^ set(WEIGHTS))
    model.CAM_AE.load_state_dict({n: torch.from_numpy(np.asarray(g["w_" + n])) for n in WEIGHTS})
    return model


def schedule64():
    """The float64 tables of Model/CF_Diff.py:245-274 that the checks read."""
    betas = np.linspace(NOISE_SCALE * NOISE_MIN, NOISE_SCALE * NOISE_MAX, STEPS, dtype=np.float64)
    betas[0] = 0.00001
    ac = np.cumprod(1.0 - betas)
    prev = np.concatenate([[1.0], ac[:-1]])
    return dict(betas=betas, ac=ac, coef1=betas * np.sqrt(prev) / (1.0 - ac), coef2=(1.0 - prev) * np.sqrt(1.0 - betas) / (1.0 - ac))


def snr_weight(ts):
    """SNR(ts - 1) - SNR(ts), 1 at ts = 0 (:450-452), float64."""
    ac = schedule64()["ac"]
    snr = ac / (1.0 - ac)
    return np.where(ts == 0, 1.0, snr[ts - 1] - snr[ts])


def p_sample(w, x_start, x_sec_hop):
    """:313-342 at sampling_steps = 0 without sampling noise, in w's dtype; the coefficients are the float64 tables rounded to
    fp32, as _extract_into_tensor's .float() leaves them."""
    dt = w["encoder.weight"].dtype
    s = schedule64()
    x_t = x_start.to(dt)
    for i in range(STEPS - 1, -1, -1):
        t = torch.full((x_t.shape[0],), i, dtype=torch.int64)
        out = cam_ae(w, x_t, x_sec_hop, t)
        x_t = float(np.float32(s["coef1"][i])) * out + float(np.float32(s["coef2"][i])) * x_t
    return x_t


def masked(scores, edges):
    out = np.array(scores, dtype=np.float64, copy=True)
    out[edges[:, 0], edges[:, 1] - U] = -np.inf
    return out


def top_lists(scores):
    """(indices [U, TOPK] local, values) by descending score, ties to the lowest index."""
    idx = np.argsort(-scores, axis=1, kind="stable")[:, :TOPK]
    return idx, np.take_along_axis(scores, idx, 1)


def lt_sequence():
    """The crafted update_Lt_history calls: timestep 2 three times in the first batch; every row filled to 10; row 2 (two more per
    batch) and row 7 overflowing, row 7 by four entries in one batch while it still has room for two."""
    rng = np.random.RandomState(17)
    batches = [np.array([2, 2, 2, 0, 1, 3, 4, 5, 6, 7, 8, 9])]
    batches += [np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 2, 2]) for _ in range(7)]
    batches += [np.array([0, 1, 3, 4, 5, 6, 8, 9, 7, 7, 7, 7]), np.array([0, 1, 3, 4, 5, 6, 8, 9, 0, 1, 3, 4]),
                np.array([5, 6, 8, 9, 2, 7, 5, 5])]
    return [(b.astype(np.int64), rng.uniform(0.01, 2.0, b.size)) for b in batches]


# ---- the keep flags of the device draws (csrc/cfdiff.hip, csrc/draws.h, csrc/common.h) ------------------------------------------
M64 = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def keep_flags(B, L, seed, step, salt, b0=0):
    """uint8 [B, 4, L, L]: flag (b, head, query i, key j) is bit (j & 63) of
    mix64(key ^ mix64((((b0 + b) * 4 + head) << 32) ^ ((i << 20) | (j >> 6)))), key = mix64(mix64(seed ^ salt) + step):
    one 64-bit draw per (b, head, query, aligned word of 64 keys); a set bit is a kept entry."""
    key = mix64((mix64(seed ^ salt) + step) & M64)
    out = np.zeros((B, 4, L, L), dtype=np.uint8)
    for b in range(B):
        for h in range(4):
            a = ((b0 + b) * 4 + h) << 32
            for i in range(L):
                for w in range((L + 63) // 64):
                    r = mix64(key ^ mix64((a ^ ((i << 20) | w)) & M64))
                    n = min(64, L - 64 * w)
                    out[b, h, i, 64 * w:64 * w + n] = [(r >> jj) & 1 for jj in range(n)]
    return out
