"""DiffMM restated on the host (Model/DiffMM.py of the reference, train_and_evaluate.py:140-244), in torch with a dtype
argument: float64 is what the tests compare against, float32 is "the reference's own lines in fp32" whose deviation from
float64 sets each tolerance.  Weights travel as a dict under the 19 state_dict names.  Nothing here touches the GPU."""
import math
import os

import numpy as np
import torch
from accept import ULP24 as ULP, rel_dev, user_item_dict  # noqa: F401

D, H, EMB, STEPS = 64, 1000, 10, 5
NAMES = ("uEmbeds", "iEmbeds", "modal_weight", "image_trans_l.weight", "image_trans_l.bias", "text_trans_l.weight",
         "text_trans_l.bias") + tuple(
    f"denoise_model_{m}.{n}" for m in ("image", "text")
    for n in ("emb_layer.weight", "emb_layer.bias", "in_layers.0.weight", "in_layers.0.bias", "out_layers.0.weight", "out_layers.0.bias"))
HYPER = dict(reg_weight=1e-4, n_layers=1, ssl_alpha=0.01, ssl_temp=0.1, ris_lambda=0.5, e_loss=0.01, rebuild_k=1)


def small_case():
    """U 53, I 97, 400 distinct interactions (every user has one), feature widths 128 and 48 (values exact in fp16).
    The torch seed is the first of 1, 2, ... at which the untrained denoisers separate every user's top-1 item from the
    second by 3e-3 of the largest magnitude (the fixture refuses below 1e-3): the rebuild's indices then need no tolerance."""
    U, I = 53, 97
    rng = np.random.default_rng(20261019)
    pairs = {(u, int(rng.integers(0, I))) for u in range(U)}
    while len(pairs) < 400:
        pairs.add((int(rng.integers(0, U)), int(rng.integers(0, I))))
    e = np.array(sorted(pairs), dtype=np.int64)
    edges = np.stack([e[:, 0], e[:, 1] + U], 1)
    v_feat = rng.standard_normal((I, 128)).astype(np.float16).astype(np.float32)
    t_feat = rng.standard_normal((I, 48)).astype(np.float16).astype(np.float32)
    B = 16
    pick = rng.choice(len(edges), size=B, replace=False)
    return dict(U=U, I=I, edges=edges, v_feat=v_feat, t_feat=t_feat, seed=2, users=edges[pick, 0].copy(), pos=edges[pick, 1].copy(),
                neg=rng.integers(U, U + I, B).astype(np.int64), diff_users=rng.permutation(U)[:24].astype(np.int64))


def hist_csr(edges, U):
    e = np.asarray(edges, dtype=np.int64)
    key = np.unique(e[:, 0] * (1 << 32) + (e[:, 1] - U))
    u, i = key >> 32, key & 0xFFFFFFFF
    rowptr = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(np.bincount(u, minlength=U), out=rowptr[1:])
    return rowptr, i.astype(np.int32)


def dense_rows(rowptr, col, users, I):
    x = np.zeros((len(users), I), dtype=np.float32)
    for b, u in enumerate(np.asarray(users).tolist()):
        if 0 <= u < len(rowptr) - 1:
            c = col[rowptr[u]:rowptr[u + 1]]
            x[b, c[(c >= 0) & (c < I)]] = 1.0
    return x


def bit_table(x0):
    """uint32 [B, ceil(I / 32)]: bit i % 32 of word i / 32 is x0[b, i]."""
    B, I = x0.shape
    pad = np.zeros((B, (I + 31) // 32 * 32), dtype=np.uint64)
    pad[:, :I] = x0 != 0
    return (pad.reshape(B, -1, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


# ---- the diffusion tables (GaussianDiffusion.__init__ / calculate_for_diffusion), float64 -------------------------------------
def tables(noise_scale=0.1, noise_min=1e-4, noise_max=0.02, steps=STEPS):
    variance = np.linspace(noise_scale * noise_min, noise_scale * noise_max, steps, dtype=np.float64)
    alpha_bar = 1 - variance
    betas = [1 - alpha_bar[0]] + [min(1 - alpha_bar[i] / alpha_bar[i - 1], 0.999) for i in range(1, steps)]
    betas = np.array(betas, dtype=np.float64)
    betas[0] = 0.0001
    alphas = 1.0 - betas
    ac = np.cumprod(alphas)
    ac_prev = np.concatenate([[1.0], ac[:-1]])
    return dict(betas=betas, alphas_cumprod=ac, sqrt_ac=np.sqrt(ac), sqrt_1mac=np.sqrt(1.0 - ac),
                coef1=betas * np.sqrt(ac_prev) / (1.0 - ac), coef2=(1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac), snr=ac / (1 - ac))


def snr_weight(ts, T=None):
    """float64 [B]: ts == 0 ? 1 : SNR(ts - 1) - SNR(ts); index -1 (the last step) is read and discarded."""
    T = T or tables()
    ts = np.asarray(ts)
    return np.where(ts == 0, 1.0, T["snr"][ts - 1] - T["snr"][ts])


def noised_rows(x0, ts, noise, keep, T=None):
    """x_in in float32 arithmetic: fl(2 fl(fl(a x0) + fl(s n))) where kept, 0 elsewhere; a, s = float32 of the float64 tables."""
    T = T or tables()
    a, s = T["sqrt_ac"][ts].astype(np.float32)[:, None], T["sqrt_1mac"][ts].astype(np.float32)[:, None]
    xt = (a * x0.astype(np.float32)).astype(np.float32) + (s * noise.astype(np.float32)).astype(np.float32)
    return np.where(keep != 0, np.float32(2.0) * xt.astype(np.float32), np.float32(0.0)).astype(np.float32)


# ---- the denoiser and the losses, torch with a dtype ---------------------------------------------------------------------------
def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def time_emb(ts, dtype):
    freqs = torch.exp(-math.log(10000) * torch.arange(0, EMB // 2, dtype=torch.float32) / (EMB // 2))
    temp = torch.as_tensor(np.asarray(ts))[:, None].float() * freqs[None]
    return torch.cat([torch.cos(temp), torch.sin(temp)], dim=-1).to(dtype)


def hidden(w, m, x_in, ts, dtype):
    """tanh([x_in | emb] W_in^T + b_in); w: tensors of `dtype` under denoise_model_<m>.*"""
    p = f"denoise_model_{m}."
    emb = time_emb(ts, dtype) @ w[p + "emb_layer.weight"].T + w[p + "emb_layer.bias"]
    return torch.tanh(torch.cat([x_in, emb], -1) @ w[p + "in_layers.0.weight"].T + w[p + "in_layers.0.bias"])


def node(h, W_out, b_out, x0, x0E, F, wt, e_loss):
    """The reference's lines after the in-layer (Denoise.forward's out-layer, training_losses :640-658, the batch means of
    train_and_evaluate.py:166) -> (loss, diff_rows float64-weighted, gc_rows).  wt: float64 [B]."""
    out = h @ W_out.T + b_out
    mse = ((x0 - out) ** 2).mean(1)
    diff = wt * mse
    gc = ((out @ F - x0E) ** 2).mean(1)
    return diff.mean() + gc.mean() * e_loss, diff, gc


def node_all(h, W_out, b_out, x0, x0E, F, wt, e_loss, dtype, g=1.0):
    """node() and its gradients by autograd in `dtype` -> dict of numpy arrays (loss, diff_rows, gc_rows, d_out = the gradient
    by the out-layer's output, dh, dW_out, db_out), the loss multiplied by g before the backward."""
    h, W_out, b_out = (_t(a, dtype).requires_grad_(True) for a in (h, W_out, b_out))
    x0, x0E, F = _t(x0, dtype), _t(x0E, dtype), _t(F, dtype)
    out = h @ W_out.T + b_out
    out.retain_grad()
    diff = torch.as_tensor(wt, dtype=torch.float64) * ((x0 - out) ** 2).mean(1)
    gc = ((out @ F - x0E) ** 2).mean(1)
    loss = diff.mean() + gc.mean() * e_loss
    (loss * g).backward()
    return {k: v.detach().numpy() for k, v in dict(loss=loss, diff_rows=diff, gc_rows=gc, d_out=out.grad, dh=h.grad, dW_out=W_out.grad,
                                                   db_out=b_out.grad).items()}


def closed_form(h, W_out, b_out, x0, x0E, F, wt, e_loss):
    """The algebra the fused node rests on, float64 numpy: M = W_out^T F, r = h M + b_out F - x0 E,
    d_out = c_b (out - x0) + k r F^T with c_b = 2 w_b / (B I), k = 2 e_loss / (B D) -> dict(M, r, d_out, dW_out, dh, db_out)."""
    h, W_out, b_out, x0, x0E, F, wt = (np.asarray(a, dtype=np.float64) for a in (h, W_out, b_out, x0, x0E, F, wt))
    B, I = x0.shape
    M = W_out.T @ F
    r = h @ M + b_out @ F - x0E
    out = h @ W_out.T + b_out
    d_out = (2.0 * wt / (B * I))[:, None] * (out - x0) + (2.0 * e_loss / (B * F.shape[1])) * (r @ F.T)
    return dict(M=M, r=r, d_out=d_out, dW_out=d_out.T @ h, dh=d_out @ W_out, db_out=d_out.sum(0),
                gc_rows=(r * r).mean(1), diff_rows=wt * ((out - x0) ** 2).mean(1))


def cast(w, dtype):
    return {k: _t(v, dtype) for k, v in w.items()}


def feats(w, c, dtype):
    """(image_feats, text_feats): the two feature Linears."""
    return (_t(c["v_feat"], dtype) @ w["image_trans_l.weight"].T + w["image_trans_l.bias"],
            _t(c["t_feat"], dtype) @ w["text_trans_l.weight"].T + w["text_trans_l.bias"])


def diffusion_step(w, c, m, x0, ts, noise, keep, e_loss, dtype):
    """One modality's diffusion step (train_and_evaluate.py:151-173) -> dict(loss, diff_loss, gc_loss, grads {name: array})."""
    w = cast(w, dtype)
    p = f"denoise_model_{m}."
    names = [n for n in NAMES if n.startswith(p)]
    for n in names:
        w[n].requires_grad_(True)
    T = tables()
    F = feats(w, c, dtype)[0 if m == "image" else 1].detach()
    x0t = _t(x0, dtype)
    a, s = (_t(T[k][ts].astype(np.float32), dtype)[:, None] for k in ("sqrt_ac", "sqrt_1mac"))
    x_in = (a * x0t + s * _t(noise, dtype)) * (_t(keep, dtype) * 2.0)
    h = hidden(w, m, x_in, ts, dtype)
    loss, diff, gc = node(h, w[p + "out_layers.0.weight"], w[p + "out_layers.0.bias"], x0t, x0t @ w["iEmbeds"].detach(), F,
                          torch.as_tensor(snr_weight(ts, T)), e_loss)
    loss.backward()
    return dict(loss=float(loss.detach()), diff_loss=diff.detach().numpy(), gc_loss=gc.detach().numpy(),
                grads={n: w[n].grad.numpy() for n in names})


def p_sample(w, m, x0, dtype):
    """The five posterior-mean iterates of p_sample(steps = 0, no sampling noise), t = 4 .. 0 -> list of [B, I] arrays."""
    w = cast(w, dtype)
    p = f"denoise_model_{m}."
    T = tables()
    x_t, out = _t(x0, dtype), []
    with torch.no_grad():
        for i in range(STEPS - 1, -1, -1):
            ts = np.full(x0.shape[0], i, dtype=np.int64)
            mo = hidden(w, m, x_t, ts, dtype) @ w[p + "out_layers.0.weight"].T + w[p + "out_layers.0.bias"]
            c1, c2 = (_t(np.float32(T[k][i]), dtype) for k in ("coef1", "coef2"))
            x_t = c1 * mo + c2 * x_t
            out.append(x_t.numpy().copy())
    return out


# ---- the graphs ----------------------------------------------------------------------------------------------------------------
def norm_adj(edges, U, I):
    """get_norm_adj_mat, dense float64 then float32: binary A, (degree + 1e-7)^-1/2 on both sides."""
    N = U + I
    A = np.zeros((N, N))
    e = np.asarray(edges)
    A[e[:, 0], e[:, 1]] = 1.0
    A[e[:, 1], e[:, 0]] = 1.0
    d = np.power(A.sum(1) + 1e-7, -0.5)
    return (d[:, None] * A * d[None, :]).astype(np.float32)


def build_ui(u_list, i_list, U, I):
    """buildUIMatrix -> (row, col, val float32) in row-major order: the pairs in both directions, the unit diagonal,
    d_r^-1/2 d_c^-1/2 with d the row sums, in float64."""
    N = U + I
    A = np.zeros((N, N))
    A[np.asarray(u_list), U + np.asarray(i_list)] = 1.0
    A = ((A + A.T) != 0) * 1.0 + np.eye(N)
    d = np.power(A.sum(1), -0.5)
    L = d[:, None] * A * d[None, :]
    row, col = np.nonzero(L)
    return row.astype(np.int64), col.astype(np.int64), L[row, col].astype(np.float32)


def edge_drop(row, col, val, rand, keep_rate=0.5):
    mask = np.floor(np.asarray(rand, dtype=np.float32) + np.float32(keep_rate)).astype(bool)
    return row[mask], col[mask], (val[mask] / np.float32(keep_rate)).astype(np.float32)


def dense_adj(row, col, val, N, dtype):
    A = torch.zeros((N, N), dtype=dtype)
    A[torch.as_tensor(row), torch.as_tensor(col)] = _t(val, dtype)
    return A


def model_loss(w, c, image_adj, text_adj, users, pos, neg, dtype, hyper=HYPER):
    """DiffMM.loss (forward_MM, forward_cl_MM, BPR, regulariser, the modality contrast) over dense adjacencies ->
    dict(loss, usr, itm, grads).  pos / neg: GLOBAL ids."""
    w = cast(w, dtype)
    names = [n for n in NAMES if not n.startswith("denoise_model_")]
    for n in names:
        w[n].requires_grad_(True)
    U, I = c["U"], c["I"]
    adj = _t(norm_adj(c["edges"], U, I), dtype)
    nz = lambda x: torch.nn.functional.normalize(x)   # noqa: E731
    fi, ft = feats(w, c, dtype)
    uE, iE = w["uEmbeds"], w["iEmbeds"]
    weight = torch.softmax(w["modal_weight"], 0)
    ego = torch.cat([uE, iE])

    def branch(madj, f):
        e = adj @ torch.cat([uE, nz(f)])
        e = e + adj @ torch.cat([e[:U], iE])
        return e + 0.2 * (madj @ ego)
    modal = weight[0] * branch(image_adj, fi) + weight[1] * branch(text_adj, ft)
    lst = [modal]
    for _ in range(hyper["n_layers"]):
        lst.append(adj @ lst[-1])
    embeds = sum(lst) + hyper["ris_lambda"] * nz(modal)
    usr, itm = embeds[:U], embeds[U:]

    def cl_branch(madj, f):
        lst = [madj @ torch.cat([uE, nz(f)])]
        for _ in range(hyper["n_layers"]):
            lst.append(adj @ lst[-1])
        e = sum(lst)
        return e[:U], e[U:]
    u1, i1 = cl_branch(image_adj, fi)
    u2, i2 = cl_branch(text_adj, ft)
    users, pos, neg = (torch.as_tensor(np.asarray(a)) for a in (users, np.asarray(pos) - U, np.asarray(neg) - U))
    ue = usr[users]
    bpr = -torch.mean(torch.log(torch.sigmoid((ue * itm[pos]).sum(1) - (ue * itm[neg]).sum(1)) + 1e-5))
    reg = hyper["reg_weight"] * ((ue ** 2).mean() + (itm[pos] ** 2).mean() + (itm[neg] ** 2).mean())

    def contrast(e1, e2, nodes, temp):
        e1, e2 = nz(e1), nz(e2)
        p1, p2 = e1[nodes], e2[nodes]
        return -torch.log(torch.exp((p1 * p2).sum(-1) / temp) / torch.exp(p1 @ e2.T / temp).sum(-1)).mean()
    cl = (contrast(u1, u2, users, hyper["ssl_temp"]) + contrast(i1, i2, pos, hyper["ssl_temp"])) * hyper["ssl_alpha"]
    loss = bpr + reg + cl
    loss.backward()
    return dict(loss=float(loss.detach()), usr=usr.detach().numpy(), itm=itm.detach().numpy(), grads={n: w[n].grad.numpy() for n in names})


def ranklist(usr, itm, rowptr, col, U, topk):
    s = np.asarray(usr, dtype=np.float64) @ np.asarray(itm, dtype=np.float64).T
    for u in range(U):
        s[u, col[rowptr[u]:rowptr[u + 1]]] = 1e-6
    order = np.argsort(-s, axis=1, kind="stable")[:, :topk]
    return order + U, np.take_along_axis(s, order, 1)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def load_fixture(golden_dir, name="diffmm_small.npz"):
    g = dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))
    for k in ("U", "I", "seed"):
        g[k] = int(g[k])
    B, I = len(g["diff_users"]), g["I"]
    g["keep"] = np.unpackbits(g["keep_bits"]).reshape(-1)[:2 * B * I].reshape(2, B, I).astype(bool)
    return g


def build_model(c, device="cpu", hyper=HYPER):
    """chaorec_amd.Model.DiffMM on the small case from the fixture's torch seed: the constructor's draws replay the reference's."""
    from chaorec_amd.Model import DiffMM
    torch.manual_seed(c["seed"])
    return DiffMM(c["U"], c["I"], c["edges"], user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]), D,
                  hyper["reg_weight"], hyper["n_layers"], hyper["ssl_alpha"], hyper["ssl_temp"], hyper["ris_lambda"], hyper["e_loss"],
                  hyper["rebuild_k"], torch.device(device))


def weights_of(model):
    sd = model.state_dict()
    return {n: sd[n].detach().cpu().numpy().copy() for n in sd}
