"""Host side of the DiffRec tests: the small case (cfdiff_host's users and items), the float64 restatement of the reference's DNN,
training_losses and p_sample, the collapsed form of the chain restated, and the restatements of the two kernels' contracts.
Shared by tests/golden/gen_diffrec.py, tests/test_diffrec_host.py and tests/test_gpu_diffrec.py.  Nothing here touches the GPU."""
import math
import os

import numpy as np
import torch

import cfdiff_host as ch
from accept import ULP24 as ULP, user_item_dict  # noqa: F401

FIXTURE = "diffrec_small.npz"
U, I = ch.U, ch.I                # 12 x 48: user 11 has no history; items 44 .. 47 have no users; item 0 is held by every other user
STEPS, NOISE_SCALE, NOISE_MIN, NOISE_MAX = 5, 0.1, 0.0005, 0.005
HID, EMB = 68, 10                # dims = "[68]": one past a segment of 64, a multiple of 4
DIMS = "[68]"
TOPK = 10
SEED = 20241010
TS = np.array([0, 4, 3, 1, 0, 4, 2, 3, 1, 2, 3, 1], dtype=np.int64)       # one per user; 0 and steps - 1 twice each
NAMES = ("dnn.emb_layer.weight", "dnn.emb_layer.bias", "dnn.in_layers.0.weight", "dnn.in_layers.0.bias",
         "dnn.out_layers.0.weight", "dnn.out_layers.0.bias")

small_case, dense_rows, masked = ch.small_case, ch.dense_rows, ch.masked
rel_dev, ZERO_REF = ch.rel_dev, ch.ZERO_REF


def load_fixture(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, FIXTURE), allow_pickle=False))
    g["keep"] = np.unpackbits(g["keep_bits"])[:U * I].reshape(U, I).astype(bool)
    return g


def spread(model):
    """The reference's initialisation (std about 0.13) leaves every tanh in its linear range: widen the in-layer and the time
    path so that the hidden units saturate for some users and steps.  In place, on `model.dnn` of either implementation."""
    with torch.no_grad():
        model.dnn.in_layers[0].weight.mul_(2.5)
        model.dnn.in_layers[0].bias.normal_(0.0, 0.3)
        model.dnn.emb_layer.weight.mul_(3.0)
        model.dnn.out_layers[0].weight.mul_(2.0)
        model.dnn.out_layers[0].bias.normal_(0.0, 0.05)


def weights_of(g, dtype=torch.float64):
    return {n: torch.from_numpy(np.asarray(g["w_" + n])).to(dtype) for n in NAMES}


def load_weights(model, g):
    sd = model.state_dict()
    assert tuple(sd) == NAMES, tuple(sd)
    model.load_state_dict({n: torch.from_numpy(np.asarray(g["w_" + n])) for n in NAMES})
    return model


def new_model(device="cpu", **kw):
    from chaorec_amd.Model.DiffRec import DiffRec
    edges = small_case()
    return DiffRec(U, I, user_item_dict(edges), NOISE_SCALE, NOISE_MIN, NOISE_MAX, STEPS, DIMS, 0.001, device, **{"seed": 11, **kw})


# ---- the tables (Model/DiffRec.py:147-202), float64 ---------------------------------------------------------------------------
def schedule64():
    betas = np.linspace(NOISE_SCALE * NOISE_MIN, NOISE_SCALE * NOISE_MAX, STEPS, dtype=np.float64)
    betas[0] = 0.00001
    ac = np.cumprod(1.0 - betas)
    prev = np.concatenate([[1.0], ac[:-1]])
    return dict(betas=betas, ac=ac, sqrt_ac=np.sqrt(ac), sqrt_1mac=np.sqrt(1.0 - ac), coef1=betas * np.sqrt(prev) / (1.0 - ac),
                coef2=(1.0 - prev) * np.sqrt(1.0 - betas) / (1.0 - ac))


def snr_weight(ts):
    """SNR(ts - 1) - SNR(ts), 1 at ts = 0 (:469-471), float64; index -1 (the last step) is read and discarded."""
    ac = schedule64()["ac"]
    snr = ac / (1.0 - ac)
    ts = np.asarray(ts)
    return np.where(ts == 0, 1.0, snr[ts - 1] - snr[ts])


# ---- the denoiser (:74-114) and the losses (:425-463) in a dtype --------------------------------------------------------------
def time_embedding(ts, dim=EMB):
    """fp32 arithmetic, as the reference's (the float64 restatement takes its fp32 values)."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    args = torch.as_tensor(np.asarray(ts))[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


def hidden(w, x_in, ts):
    dt = w[NAMES[2]].dtype
    emb = time_embedding(ts).to(dt) @ w["dnn.emb_layer.weight"].T + w["dnn.emb_layer.bias"]
    return torch.tanh(torch.cat([x_in.to(dt), emb], -1) @ w["dnn.in_layers.0.weight"].T + w["dnn.in_layers.0.bias"])


def dnn(w, x_in, ts):
    return hidden(w, x_in, ts) @ w["dnn.out_layers.0.weight"].T + w["dnn.out_layers.0.bias"]


def noised_input(x0, ts, noise, keep, dtype):
    """dropout_0.5(q_sample(x0, ts, noise)) with the given flags; a, s are the float64 tables rounded to fp32 (.float())."""
    s = schedule64()
    a, b = (torch.from_numpy(s[k][np.asarray(ts)].astype(np.float32)).to(dtype)[:, None] for k in ("sqrt_ac", "sqrt_1mac"))
    x_t = a * torch.as_tensor(x0).to(dtype) + b * torch.as_tensor(noise).to(dtype)
    return x_t * (torch.as_tensor(keep).to(dtype) * 2.0)


def training_step(w, x0, ts, noise, keep, pt=None, g=1.0):
    """One training_losses call with given draws, in w's dtype -> dict(loss, reloss float64-weighted, grads by name)."""
    dt = w[NAMES[2]].dtype
    w = {n: t.detach().clone().requires_grad_(True) for n, t in w.items()}
    out = dnn(w, noised_input(x0, ts, noise, keep, dt), ts)
    reloss = torch.from_numpy(snr_weight(ts)) * ((torch.as_tensor(x0).to(dt) - out) ** 2).mean(1)
    pt = torch.ones(len(ts), dtype=torch.float64) if pt is None else torch.as_tensor(pt, dtype=torch.float64)
    loss = (reloss / pt).mean()
    (loss * g).backward()
    return dict(loss=float(loss.detach()), reloss=reloss.detach().numpy(), grads={n: t.grad.numpy() for n, t in w.items()})


def p_sample(w, x_start, s=None):
    """:263-303 at sampling_steps = 0 without sampling noise, in w's dtype; the coefficients are the float64 tables rounded to
    fp32, as _extract_into_tensor's .float() leaves them.  s: other tables than schedule64()'s."""
    dt = w[NAMES[2]].dtype
    s = s or schedule64()
    x_t = torch.as_tensor(x_start).to(dt)
    for i in range(STEPS - 1, -1, -1):
        out = dnn(w, x_t, np.full(x_t.shape[0], i, dtype=np.int64))
        x_t = float(np.float32(s["coef1"][i])) * out + float(np.float32(s["coef2"][i])) * x_t
    return x_t


def p_sample_collapsed(w, x_start, s=None):
    """The same chain in hidden space, in w's dtype -> (x^(0), beta)."""
    dt = w[NAMES[2]].dtype
    s = s or schedule64()
    c1, c2 = ([float(np.float32(v)) for v in s[k]] for k in ("coef1", "coef2"))
    W1, b1, Wo, bo = (w[n] for n in NAMES[2:])
    W1x, W1e = W1[:, :I], W1[:, I:]
    G, g0 = W1x @ Wo, W1x @ bo
    emb = time_embedding(np.arange(STEPS)).to(dt) @ w["dnn.emb_layer.weight"].T + w["dnn.emb_layer.bias"]
    e = emb @ W1e.T + b1
    x = torch.as_tensor(x_start).to(dt)
    p = x @ W1x.T
    a, prod = [], 1.0
    for t in range(STEPS):
        a.append(c1[t] * prod)
        prod *= c2[t]
    acc = torch.zeros_like(p)
    for t in range(STEPS - 1, -1, -1):
        z = torch.tanh(p + e[t])
        acc = acc + a[t] * z
        p = c1[t] * (z @ G.T + g0) + c2[t] * p
    return acc @ Wo.T + sum(a) * bo + prod * x, prod


def top_lists(scores, k=TOPK):
    idx = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(scores, idx, 1)


def lt_sequence():
    """The crafted update_Lt_history calls over 5 timesteps: timestep 2 three times in the first batch; every row filled to 10;
    row 2 (two more per batch) and row 4 overflowing, row 4 by four entries in one batch while it still has room for two."""
    rng = np.random.RandomState(23)
    batches = [np.array([2, 2, 2, 0, 1, 3, 4])]
    batches += [np.array([0, 1, 2, 3, 4, 2, 2]) for _ in range(7)]
    batches += [np.array([0, 1, 3, 4, 4, 4, 4]), np.array([0, 1, 3, 0, 1, 3]), np.array([2, 4, 3, 3, 0, 1])]
    return [(b.astype(np.int64), rng.uniform(0.01, 2.0, b.size)) for b in batches]


# ---- the kernels' contracts ----------------------------------------------------------------------------------------------------
def bit_table(x0):
    """uint32 [B, ceil(I / 32)]: bit i % 32 of word i / 32 is x0[b, i]."""
    B, n = x0.shape
    pad = np.zeros((B, (n + 31) // 32 * 32), dtype=np.uint64)
    pad[:, :n] = x0 != 0
    return (pad.reshape(B, -1, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def loss_node(h, W_out, b_out, x0, wt, pt, dtype, g=1.0):
    """The reference's lines after the in-layer, and their gradients by autograd in `dtype` -> dict of numpy arrays (loss,
    reloss_rows, d_out = the gradient by the out-layer's output, dh, dW_out, db_out), the loss multiplied by g before the
    backward.  wt, pt float64 [B]."""
    h, W_out, b_out = (torch.as_tensor(np.asarray(a)).to(dtype).requires_grad_(True) for a in (h, W_out, b_out))
    out = h @ W_out.T + b_out
    out.retain_grad()
    reloss = torch.as_tensor(wt, dtype=torch.float64) * ((torch.as_tensor(x0).to(dtype) - out) ** 2).mean(1)
    loss = (reloss / torch.as_tensor(pt, dtype=torch.float64)).mean()
    (loss * g).backward()
    return {k: v.detach().numpy() for k, v in dict(loss=loss, reloss_rows=reloss, d_out=out.grad, dh=h.grad, dW_out=W_out.grad,
                                                   db_out=b_out.grad).items()}


def chain_step(z, G, g0, p, e_next, c1, c2, dtype):
    z, G, g0, p, e_next = (torch.as_tensor(np.asarray(a)).to(dtype) for a in (z, G, g0, p, e_next))
    p_next = c1 * (z @ G.T + g0) + c2 * p
    return dict(p_next=p_next.numpy(), z_next=torch.tanh(p_next + e_next).numpy())
