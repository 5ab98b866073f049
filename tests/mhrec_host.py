"""MHRec restated on the host (Model/MHRec.py of the reference, train_and_evaluate.py:331-512), in torch with a dtype
argument: float64 is what the tests compare against, float32 is "the reference's own lines in fp32".  The hypergraph layer is
there twice: `layer` (the reference's lines, gradients by autograd) and `layer_grads` (forward AND backward written out from
the formulas, float64 numpy).  Weights travel as a dict under the 31 state_dict names.  Nothing here touches the GPU."""
import math
import os

import numpy as np
import torch
from accept import ULP24 as ULP, rel_dev, user_item_dict  # noqa: F401

D, H, EMB, STEPS, SAMPLING_STEPS = 64, 1000, 10, 20, 5
LONG_ROW = 256            # chaorec_mhrec_long_row(): the layer cases are built around it (test_gpu_mhrec asserts the library agrees)
HYPER = dict(reg_weight=1e-4, ii_topk=3, uu_topk=3, num_hypernodes=10, n_layers=2, h_layers=2, ssl_temp=0.2, ssl_alpha=0.01,
             beta1=0.5, beta2=0.5)
LR, TOPK, N_STEPS, DIFF_BATCH = 1e-3, 10, 3, 128
MAIN = ("modal_weight", "image_embedding.weight", "image_trs.weight", "image_trs.bias", "text_embedding.weight", "text_trs.weight",
        "text_trs.bias", "user_embedding.weight", "user_visual_embedding.weight", "user_textual_embedding.weight",
        "item_embedding.weight")
HYPER_A = tuple(f"hypergraphLayers{m}.{l}.a" for m in ("Visual", "Textual") for l in range(HYPER["h_layers"]))
HYPER_W = tuple(f"hypergraphLayers{m}.{l}.W.weight" for m in ("Visual", "Textual") for l in range(HYPER["h_layers"]))
DENOISE = tuple(f"denoise_model_{m}.{n}" for m in ("image", "text")
                for n in ("emb_layer.weight", "emb_layer.bias", "in_layers.0.weight", "in_layers.0.bias", "out_layers.0.weight",
                          "out_layers.0.bias"))
NAMES = MAIN + tuple(n for m in ("Visual", "Textual") for l in range(HYPER["h_layers"])
                     for n in (f"hypergraphLayers{m}.{l}.a", f"hypergraphLayers{m}.{l}.W.weight")) + DENOISE
WITH_GRAD = MAIN + HYPER_A           # what loss() reaches (the layers' W and the denoisers get no gradient from it)


def user_graph_dict(edges, U):
    """{user: [[co-occurring users], [counts]]}, by count descending, id ascending (dualgnn-gen-u-u-matrix.py's file)."""
    e = np.asarray(edges)
    A = np.zeros((U, int(e[:, 1].max()) + 1))
    A[e[:, 0], e[:, 1]] = 1.0
    C = (A @ A.T).astype(np.int64)
    np.fill_diagonal(C, 0)
    out = {}
    for u in range(U):
        ids = [v for v in np.lexsort((np.arange(U), -C[u])).tolist() if C[u, v] > 0]
        out[u] = [ids, [int(C[u, v]) for v in ids]]
    return out


def small_case(seed=1):
    """U 23, I 47 (70 nodes), 300 distinct interactions (every user has one, every user co-occurs with at least uu_topk
    others), feature widths 128 and 48 (values exact in fp16), a BPR batch of 16, the 300 input hyperedges in three diffusion
    batches of a fixed permutation.  `seed` is the torch seed of the weights: golden/gen_mhrec.py picks it."""
    U, I = 23, 47
    rng = np.random.default_rng(20261020)
    pairs = {(u, int(rng.integers(0, I))) for u in range(U)}
    while len(pairs) < 300:
        pairs.add((int(rng.integers(0, U)), int(rng.integers(0, I))))
    e = np.array(sorted(pairs), dtype=np.int64)
    edges = np.stack([e[:, 0], e[:, 1] + U], 1)
    v_feat = rng.standard_normal((I, 128)).astype(np.float16).astype(np.float32)
    t_feat = rng.standard_normal((I, 48)).astype(np.float16).astype(np.float32)
    B = 16
    pick = rng.choice(len(edges), size=B, replace=False)
    perm = rng.permutation(len(edges)).astype(np.int64)
    c = dict(U=U, I=I, edges=edges, v_feat=v_feat, t_feat=t_feat, seed=int(seed), users=edges[pick, 0].copy(), pos=edges[pick, 1].copy(),
             neg=rng.integers(U, U + I, B).astype(np.int64),
             batches=[perm[b:b + DIFF_BATCH] for b in range(0, len(perm), DIFF_BATCH)])
    c["user_graph"] = user_graph_dict(edges, U)
    assert min(len(v[0]) for v in c["user_graph"].values()) >= HYPER["uu_topk"]
    return c


def input_hyperedges(c):
    """pre_processing (Model/MHRec.py:603-636) -> (visual, textual) int64 [E, 2 + uu_topk + ii_topk]:
    [u] + the first uu_topk co-occurring users + [i] + the ii_topk most cosine-similar other items (global ids)."""
    U, e = c["U"], c["edges"]
    uu = np.array([c["user_graph"][u][0][:HYPER["uu_topk"]] for u in range(U)], dtype=np.int64)
    out = []
    for feat in (c["v_feat"], c["t_feat"]):
        f = feat.astype(np.float64)
        f = f / np.linalg.norm(f, axis=1, keepdims=True)
        sim = f @ f.T
        np.fill_diagonal(sim, -np.inf)
        knn = np.argsort(-sim, axis=1, kind="stable")[:, :HYPER["ii_topk"]]
        out.append(np.concatenate([e[:, :1], uu[e[:, 0]], e[:, 1:2], knn[e[:, 1] - U] + U], 1))
    return out[0], out[1]


def dense_rows(table, batch, N):
    """HyperDiffusionData's rows of a batch: counts (coo.toarray() sums a node named twice)."""
    x = np.zeros((len(batch), N), dtype=np.float32)
    for b, j in enumerate(np.asarray(batch).tolist()):
        np.add.at(x[b], np.asarray(table[j]), 1.0)
    return x


def draws(c, seed_offset=0):
    """Every draw of one epoch: per modality and diffusion batch ts / noise / keep, the rebuild's q_sample noise, and per BPR
    step the four layer masks [N, 64] (visual layers, then textual)."""
    rng = np.random.default_rng(77 + seed_offset)
    N = c["U"] + c["I"]
    sizes = [len(b) for b in c["batches"]]
    return dict(ts=[[rng.integers(0, STEPS, n).astype(np.int64) for n in sizes] for _ in range(2)],
                noise=[[rng.standard_normal((n, N)).astype(np.float32) for n in sizes] for _ in range(2)],
                keep=[[rng.random((n, N)) < 0.5 for n in sizes] for _ in range(2)],
                rebuild_noise=[[rng.standard_normal((n, N)).astype(np.float32) for n in sizes] for _ in range(2)],
                fwd_keep=[[rng.random((N, D)) < 0.5 for _ in range(2 * HYPER["h_layers"])] for _ in range(N_STEPS)])


# ---- the hypergraph layer ------------------------------------------------------------------------------------------------------
def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def layer(X, a, nodes):
    """HypergraphAttentionLayer.forward (Model/MHRec.py:53-89) over the ELL table nodes [E, k] (H = its incidence matrix of
    ones) -> (out, the largest |s_n + r_j|)."""
    nodes = torch.as_tensor(np.asarray(nodes)).long()
    E, k = nodes.shape
    node, hedge = nodes.reshape(-1), torch.arange(E).repeat_interleave(k)
    Ej = torch.zeros((E, X.shape[1]), dtype=X.dtype).index_add(0, hedge, X[node])
    e = torch.matmul(torch.cat([X[node], Ej[hedge]], dim=1), a).squeeze(-1)
    e_exp = torch.exp(e)
    sums = torch.zeros(X.shape[0], dtype=X.dtype).index_add(0, node, e_exp)
    alpha = e_exp / (sums[node] + 1e-16)
    out = torch.zeros_like(X).index_add(0, node, alpha.unsqueeze(-1) * Ej[hedge])
    return out, float(e.detach().abs().max())


def layer_tail(out, X, keep):
    """Model/MHRec.py:725-726: dropout_0.5(out + X) with GIVEN keep flags."""
    return (out + X) * (_t(keep, X.dtype) * 2.0)


def layer_autograd(X, a, nodes, keep, g, dtype):
    """layer + layer_tail and the gradients of <y, g> by autograd in `dtype` -> dict(out, y, dX, da)."""
    X, a = _t(X, dtype).requires_grad_(True), _t(a, dtype).reshape(-1, 1).requires_grad_(True)
    out, mx = layer(X, a, nodes)
    y = layer_tail(out, X, keep)
    (y * _t(g, dtype)).sum().backward()
    return dict(out=out.detach().numpy(), y=y.detach().numpy(), dX=X.grad.numpy(), da=a.grad.numpy().reshape(-1), max_exp=mx)


def layer_grads(X, a, nodes, keep, g):
    """The layer, its tail and its backward written out (float64 numpy):
        E_j = sum_{n in j} X_n, s_n = <X_n, a1>, r_j = <E_j, a2>, w_nj = exp(s_n + r_j), Z_n = sum_j w_nj,
        alpha_nj = w_nj / (Z_n + 1e-16), out_n = sum_j alpha_nj E_j, y_n = keep ? 2 (out_n + X_n) : 0
        gm = keep ? 2 g : 0, t_n = <gm_n, out_n>, de_nj = alpha_nj (<gm_n, E_j> - t_n)
        dE_j = sum_{n in j} alpha_nj gm_n + a2 sum_{n in j} de_nj, dX_n = gm_n + sum_j dE_j + a1 sum_j de_nj
        da2 = sum_j E_j sum_{n in j} de_nj, da1 = sum_n X_n sum_j de_nj"""
    X, a, g = (np.asarray(v, dtype=np.float64) for v in (X, a, g))
    a = a.reshape(-1)
    nodes = np.asarray(nodes, dtype=np.int64)
    E, k = nodes.shape
    N = X.shape[0]
    a1, a2 = a[:D], a[D:]
    node, hedge = nodes.reshape(-1), np.repeat(np.arange(E), k)
    Ej = X[nodes].sum(1)
    s, r = X @ a1, Ej @ a2
    w = np.exp(s[node] + r[hedge])
    Z = np.bincount(node, weights=w, minlength=N)
    alpha = w / (Z[node] + 1e-16)
    out = np.zeros_like(X)
    np.add.at(out, node, alpha[:, None] * Ej[hedge])
    mult = np.where(np.asarray(keep) != 0, 2.0, 0.0)
    y = mult * (out + X)
    gm = mult * g
    t = (gm * out).sum(1)
    de = alpha * ((gm[node] * Ej[hedge]).sum(1) - t[node])
    sde_e = np.bincount(hedge, weights=de, minlength=E)
    sde_n = np.bincount(node, weights=de, minlength=N)
    dE = np.zeros_like(Ej)
    np.add.at(dE, hedge, alpha[:, None] * gm[node])
    dE += sde_e[:, None] * a2[None]
    dX = gm + sde_n[:, None] * a1[None]
    np.add.at(dX, node, dE[hedge])
    return dict(out=out, y=y, dX=dX, da1=(X * sde_n[:, None]).sum(0), da2=(Ej * sde_e[:, None]).sum(0),
                max_exp=float(np.abs(s[node] + r[hedge]).max()), deg=np.bincount(node, minlength=N))


def layer_case(k, seed=5):
    """The kernel case: 23 + 47 = 70 nodes, E = LONG_ROW + 70 hyperedges of k distinct nodes.  Node 0 is in every hyperedge, node
    1 in exactly LONG_ROW, node 2 in LONG_ROW + 1, nodes 3 .. 6 in 64, 65, 1 and 0; the others share what is left.  E is no
    multiple of 4 (hyperedges per wave) or 16 (per workgroup).  -> dict(nodes, N, X, a, keep, g)."""
    N, E = 70, LONG_ROW + 70
    rng = np.random.default_rng(seed + k)
    want = {1: LONG_ROW, 2: LONG_ROW + 1, 3: 64, 4: 65, 5: 1}
    slots = (k - 1) * E
    fill = slots - sum(want.values())
    others = list(range(7, N))
    counts = dict(want)
    for q in range(fill):
        counts[others[q % len(others)]] = counts.get(others[q % len(others)], 0) + 1
    assert max(counts.values()) <= E and E % 4 and E % 16
    tokens = np.concatenate([np.full(cnt, n, dtype=np.int64) for n, cnt in sorted(counts.items())])
    nodes = np.concatenate([np.zeros((E, 1), dtype=np.int64), tokens.reshape(k - 1, E).T], 1)      # hyperedge j: tokens j, j + E, ...
    nodes = nodes[rng.permutation(E)]
    nodes = np.take_along_axis(nodes, np.argsort(rng.random(nodes.shape), axis=1), 1)
    assert all(len(set(row)) == k for row in nodes.tolist())
    deg = np.bincount(nodes.reshape(-1), minlength=N)
    assert deg[0] == E and deg[1] == LONG_ROW and deg[2] == LONG_ROW + 1 and tuple(deg[3:7]) == (64, 65, 1, 0)
    bound = math.sqrt(6.0 / (2 * D + 1))
    return dict(nodes=nodes, N=N, k=k, X=(0.3 * rng.standard_normal((N, D))).astype(np.float32),
                a=rng.uniform(-bound, bound, 2 * D).astype(np.float32), keep=rng.random((N, D)) < 0.5,
                g=rng.standard_normal((N, D)).astype(np.float32))


# ---- the model -----------------------------------------------------------------------------------------------------------------
def cast(w, dtype, grad=()):
    out = {k: _t(v, dtype).clone() for k, v in w.items()}          # (a copy: the steps update these in place)
    for n in grad:
        out[n].requires_grad_(True)
    return out


def norm_adj(edges, U, I):
    """get_norm_adj_mat, dense float64 then float32: binary A, (degree + 1e-7)^-1/2 on both sides."""
    N = U + I
    A = np.zeros((N, N))
    e = np.asarray(edges)
    A[e[:, 0], e[:, 1]] = 1.0
    A[e[:, 1], e[:, 0]] = 1.0
    d = np.power(A.sum(1) + 1e-7, -0.5)
    return (d[:, None] * A * d[None, :]).astype(np.float32)


def forward(w, c, Hv, Ht, keeps, hyper=HYPER):
    """MHRec.forward (Model/MHRec.py:708-779) on tensors w of one dtype -> dict.  Hv / Ht: ELL tables; keeps: the four masks."""
    dtype = w["modal_weight"].dtype
    U = c["U"]
    adj = _t(norm_adj(c["edges"], U, c["I"]), dtype)
    nz = torch.nn.functional.normalize
    v = w["image_embedding.weight"] @ w["image_trs.weight"].T + w["image_trs.bias"]
    t = w["text_embedding.weight"] @ w["text_trs.weight"].T + w["text_trs.bias"]
    weight = torch.softmax(w["modal_weight"], 0)
    hl = hyper["h_layers"]
    outs, max_exp = [], 0.0

    def gcn(first):
        lst = [first]
        for _ in range(hyper["n_layers"]):
            lst.append(adj @ lst[-1])
        return torch.stack(lst).mean(0)

    def branch(name, nodes, first, masks):
        nonlocal max_exp
        lst = [first]
        for l in range(hl):
            out, mx = layer(lst[-1], w[f"hypergraphLayers{name}.{l}.a"], nodes)
            max_exp = max(max_exp, mx)
            outs.append(out)
            lst.append(layer_tail(out, lst[-1], masks[l]))
        return torch.stack(lst).mean(0) + hyper["beta1"] * gcn(first)
    ev = branch("Visual", Hv, torch.cat([w["user_visual_embedding.weight"], nz(v)]), keeps[:hl])
    et = branch("Textual", Ht, torch.cat([w["user_textual_embedding.weight"], nz(t)]), keeps[hl:])
    modal = weight[0] * ev + weight[1] * et
    eg = gcn(torch.cat([w["user_embedding.weight"], w["item_embedding.weight"]]))
    res = eg + hyper["beta2"] * nz(modal)
    return dict(result=res, embeds_v=ev, embeds_t=et, embeds_g=eg, layer_outs=outs, max_exp=max_exp, v=v, t=t)


def model_loss(w, c, Hv, Ht, keeps, hyper=HYPER):
    """MHRec.loss (Model/MHRec.py:842-864) -> (loss tensor, forward's dict, dict of the parts)."""
    U = c["U"]
    f = forward(w, c, Hv, Ht, keeps, hyper)
    res, ev, et, eg = f["result"], f["embeds_v"], f["embeds_t"], f["embeds_g"]
    users, pos, neg = (torch.as_tensor(np.asarray(a)) for a in (c["users"], c["pos"] - U, c["neg"] - U))
    ug, ig = res[:U], res[U:]
    ue = ug[users]
    bpr = -torch.mean(torch.log(torch.sigmoid((ue * ig[pos]).sum(1) - (ue * ig[neg]).sum(1)) + 1e-5))

    def item_init(idx):
        return torch.cat([w["item_embedding.weight"][idx],
                          w["image_embedding.weight"][idx] @ w["image_trs.weight"].T + w["image_trs.bias"],
                          w["text_embedding.weight"][idx] @ w["text_trs.weight"].T + w["text_trs.bias"]], 1)
    u_init = torch.cat([w["user_embedding.weight"][users], w["user_visual_embedding.weight"][users],
                        w["user_textual_embedding.weight"][users]], 1)
    reg = hyper["reg_weight"] * ((ue ** 2).mean() + (ig[pos] ** 2).mean() + (ig[neg] ** 2).mean() + (u_init ** 2).mean()
                                 + (item_init(pos) ** 2).mean() + (item_init(neg) ** 2).mean())
    nz = torch.nn.functional.normalize

    def contrast(e1, e2, nodes):
        e1, e2 = nz(e1), nz(e2)
        p1, p2 = e1[nodes], e2[nodes]
        nume = torch.exp((p1 * p2).sum(-1) / hyper["ssl_temp"])
        deno = torch.exp(p1 @ e2.T / hyper["ssl_temp"]).sum(-1) + 1e-8
        return -torch.log(nume / deno).mean()
    ssl = (contrast(eg[:U], ev[:U], users) + contrast(eg[U:], et[U:], pos) + contrast(eg[:U], et[:U], users)
           + contrast(eg[U:], ev[U:], pos)) * hyper["ssl_alpha"]
    return bpr + reg + ssl, f, dict(bpr=float(bpr.detach()), reg=float(reg.detach()), ssl=float(ssl.detach()))


def step_losses(w, c, Hv, Ht, keeps, dtype=torch.float64):
    """loss() on FIXED weights with its gradients -> dict(loss, parts, grads, result, embeds_*, layer_outs, max_exp)."""
    wt = cast(w, dtype, WITH_GRAD)
    loss, f, parts = model_loss(wt, c, Hv, Ht, keeps)
    loss.backward()
    out = dict(loss=float(loss.detach()), parts=parts, grads={n: wt[n].grad.numpy() for n in WITH_GRAD}, max_exp=f["max_exp"],
               layer_outs=[o.detach().numpy() for o in f["layer_outs"]])
    for k in ("result", "embeds_v", "embeds_t", "embeds_g"):
        out[k] = f[k].detach().numpy()
    return out


def rank_scores(result, c):
    """gene_ranklist's score matrix in float64: history entries = 1e-6."""
    U = c["U"]
    s = np.asarray(result[:U], dtype=np.float64) @ np.asarray(result[U:], dtype=np.float64).T
    for u, i in np.asarray(c["edges"]).tolist():
        s[u, i - U] = 1e-6
    return s


# ---- the diffusion half --------------------------------------------------------------------------------------------------------
def tables(noise_scale=0.1, noise_min=1e-4, noise_max=0.02, steps=STEPS):
    variance = np.linspace(noise_scale * noise_min, noise_scale * noise_max, steps, dtype=np.float64)
    alpha_bar = 1 - variance
    betas = np.array([1 - alpha_bar[0]] + [min(1 - alpha_bar[i] / alpha_bar[i - 1], 0.999) for i in range(1, steps)], dtype=np.float64)
    betas[0] = 0.0001
    alphas = 1.0 - betas
    ac = np.cumprod(alphas)
    ac_prev = np.concatenate([[1.0], ac[:-1]])
    return dict(betas=betas, alphas_cumprod=ac, sqrt_ac=np.sqrt(ac), sqrt_1mac=np.sqrt(1.0 - ac),
                coef1=betas * np.sqrt(ac_prev) / (1.0 - ac), coef2=(1.0 - ac_prev) * np.sqrt(alphas) / (1.0 - ac), snr=ac / (1 - ac))


def snr_weight(ts, T=None):
    """float64 [B]: ts == 0 ? 1 : SNR(ts - 1) - SNR(ts)."""
    T = T or tables()
    ts = np.asarray(ts)
    return np.where(ts == 0, 1.0, T["snr"][ts - 1] - T["snr"][ts])


def time_emb(ts, dtype):
    freqs = torch.exp(-math.log(10000) * torch.arange(0, EMB // 2, dtype=torch.float32) / (EMB // 2))
    temp = torch.as_tensor(np.asarray(ts))[:, None].float() * freqs[None]
    return torch.cat([torch.cos(temp), torch.sin(temp)], dim=-1).to(dtype)


def denoise(w, m, x, ts):
    """Denoise.forward after its dropout: the in-layer over [x | emb], tanh, the out-layer."""
    p = f"denoise_model_{m}."
    dtype = x.dtype
    emb = time_emb(ts, dtype) @ w[p + "emb_layer.weight"].T + w[p + "emb_layer.bias"]
    h = torch.tanh(torch.cat([x, emb], -1) @ w[p + "in_layers.0.weight"].T + w[p + "in_layers.0.bias"])
    return h @ w[p + "out_layers.0.weight"].T + w[p + "out_layers.0.bias"]


def diffusion_loss(w, m, x0, ts, noise, keep):
    """training_losses(...).mean() (Model/MHRec.py:325-361) on tensors w; the tables' entries pass through float32 as
    _extract_into_tensor's .float() does; the SNR weight is float64."""
    dtype = w[f"denoise_model_{m}.emb_layer.bias"].dtype
    T = tables()
    x0t = _t(x0, dtype)
    a, s = (_t(T[k][ts].astype(np.float32), dtype)[:, None] for k in ("sqrt_ac", "sqrt_1mac"))
    x_t = a * x0t + s * _t(noise, dtype)
    out = denoise(w, m, x_t * (_t(keep, dtype) * 2.0), ts)
    return (torch.as_tensor(snr_weight(ts, T)) * ((x0t - out) ** 2).mean(1)).mean()


def p_sample(w, m, x0, noise):
    """p_sample(steps = 5, no sampling noise): q_sample at t = 4 with the given noise, then the 20 posterior means."""
    dtype = w[f"denoise_model_{m}.emb_layer.bias"].dtype
    T = tables()
    a, s = (_t(np.float32(T[k][SAMPLING_STEPS - 1]), dtype) for k in ("sqrt_ac", "sqrt_1mac"))
    x_t = a * _t(x0, dtype) + s * _t(noise, dtype)
    with torch.no_grad():
        for i in range(STEPS - 1, -1, -1):
            ts = np.full(x0.shape[0], i, dtype=np.int64)
            c1, c2 = (_t(np.float32(T[k][i]), dtype) for k in ("coef1", "coef2"))
            x_t = c1 * denoise(w, m, x_t, ts) + c2 * x_t
    return x_t


def topk_gap(x, k):
    """The smallest gap between a row's k-th and (k + 1)-th largest value, relative to the largest magnitude."""
    v = np.sort(np.asarray(x, dtype=np.float64), 1)[:, ::-1]
    return float((v[:, k - 1] - v[:, k]).min() / np.abs(v).max())


def rebuild(w, c, table, noises, k=HYPER["num_hypernodes"]):
    """train_and_evaluate.py:394-497 -> ([visual nodes, textual nodes] as int64 [E, k] in loader order, the smallest top-k gap).
    Both loaders read `table` (the visual hyperedges, main.py:227-228)."""
    N = c["U"] + c["I"]
    out, gap = [], np.inf
    for m, mod in enumerate(("image", "text")):
        rows = []
        for b, batch in enumerate(c["batches"]):
            x = p_sample(w, mod, dense_rows(table, batch, N), noises[m][b]).numpy()
            gap = min(gap, topk_gap(x, k))
            rows.append(np.argsort(-x, axis=1, kind="stable")[:, :k])
        out.append(np.concatenate(rows))
    return out, gap


def epoch(w, c, table, dr, dtype=torch.float64, hyper=HYPER):
    """One epoch of train_and_evaluate.py:331-512 from weights w with the draws dr: the two diffusion passes (a fresh Adam per
    denoiser), the rebuild, N_STEPS BPR steps under Adam over everything -> dict(weights, diff_losses [2][batches],
    nodes [2], gap, losses [N_STEPS])."""
    N = c["U"] + c["I"]
    wt = cast(w, dtype, NAMES)
    diff_losses = []
    for m, mod in enumerate(("image", "text")):
        names = [n for n in DENOISE if n.startswith(f"denoise_model_{mod}.")]
        opt = torch.optim.Adam([wt[n] for n in names], lr=LR, weight_decay=0)
        ls = []
        for b, batch in enumerate(c["batches"]):
            opt.zero_grad()
            loss = diffusion_loss(wt, mod, dense_rows(table, batch, N), dr["ts"][m][b], dr["noise"][m][b], dr["keep"][m][b])
            loss.backward()
            opt.step()
            ls.append(float(loss.detach()))
        diff_losses.append(ls)
    with torch.no_grad():
        nodes, gap = rebuild({k: v.detach() for k, v in wt.items()}, c, table, dr["rebuild_noise"])
    losses = bpr_steps(wt, c, nodes[0], nodes[1], dr["fwd_keep"], hyper)
    return dict(weights={n: wt[n].detach().numpy() for n in NAMES}, diff_losses=diff_losses, nodes=nodes, gap=gap, losses=losses)


def bpr_steps(wt, c, Hv, Ht, fwd_keep, hyper=HYPER):
    """N_STEPS steps of the third phase on the tensors wt (updated in place) -> the losses."""
    opt = torch.optim.Adam([wt[n] for n in NAMES], lr=LR)
    losses = []
    for s in range(len(fwd_keep)):
        opt.zero_grad()
        loss, _, _ = model_loss(wt, c, Hv, Ht, fwd_keep[s], hyper)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.array(losses)


def three_steps(w, c, Hv, Ht, fwd_keep, dtype=torch.float64):
    wt = cast(w, dtype, NAMES)
    losses = bpr_steps(wt, c, Hv, Ht, fwd_keep)
    return {n: wt[n].detach().numpy() for n in NAMES}, losses


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def load_fixture(golden_dir, name="mhrec_small.npz"):
    g = dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))
    for k in ("U", "I", "seed"):
        g[k] = int(g[k])
    return g


def build_model(c, device="cpu", hyper=HYPER):
    """chaorec_amd.Model.MHRec on the small case from the case's torch seed: the constructor's draws replay the reference's."""
    from chaorec_amd.Model import MHRec
    torch.manual_seed(c["seed"])
    return MHRec(c["U"], c["I"], c["edges"], user_item_dict(c["edges"]), torch.from_numpy(c["v_feat"]), torch.from_numpy(c["t_feat"]), D,
                 hyper["reg_weight"], hyper["ii_topk"], hyper["uu_topk"], hyper["num_hypernodes"], hyper["n_layers"], hyper["h_layers"],
                 hyper["ssl_temp"], hyper["ssl_alpha"], hyper["beta1"], hyper["beta2"], torch.device(device))


def weights_of(model):
    sd = model.state_dict()
    return {n: sd[n].detach().cpu().numpy().copy() for n in sd}


def init_weights(c):
    return weights_of(build_model(c))
