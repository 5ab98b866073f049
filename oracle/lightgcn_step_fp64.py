"""One LightGCN training step in float64 that carries a bound on the error an fp32 implementation of it may make.

TEST INFRASTRUCTURE ONLY (like oracle/torch_ref.py).  The step is the one optim.FusedLightGCNStep runs and
oracle/torch_ref.py:TorchRefLightGCN.loss + torch.optim.Adam restate: L propagates, the layer mean with weights
1 / (L + 1), the BPR term log(sigmoid(d) + 1e-5), L2 on the PROPAGATED rows of the batch, the gradient with respect to
the joined embedding table, and one Adam step (torch's arithmetic, chaorec_amd/csrc/common.h:adam_update).

The CSR passed in is taken as exact (its fp32 values are the operator), so the bound tests the arithmetic of the step and
not the normalisation of the graph.  The inputs W, m and v are exact as well (fp32 snapshots), and so are the betas:
pass the ones the implementation computes with (torch.optim.Adam: the python floats; the HIP kernels, whose interface
carries fp32 betas: those floats rounded to fp32 -- 1 - 0.999f is 1.3e-5 away from 1 - 0.999).

Every output is a pair (value, bound): |fp32 result - value| <= bound holds for any fp32 implementation that adds the same
terms in ANY order with round-to-nearest, up to first order in u = 2^-24.  The bound is a running magnitude pass next to
the value pass, with gamma(n) = n u / (1 - n u) for an element that n roundings feed:
  * propagate     E_{l+1} = |A| E_l + gamma(nnz) |A| |x_l|                   (nnz products, nnz - 1 adds)
  * layer mean    E_R = w sum E_l + gamma(L + 2) w sum |x_l|                 (L + 1 products, L adds, w itself rounded)
  * scores        E_d = sum over the dot products of gamma(D) |u . p| + |u| E_p + |p| E_u + E_u E_p, + u (|sp| + |sn|)
  * BPR term      Lipschitz constant 1 in d (d/dd log(sigmoid(d) + eps) = s (1 - s) / (s + eps) < 1), plus the rounding
                  of exp / log (each within two ulps = 4 u relative: OCML and Sleef are within one) and of the adds
  * coefficient   c = -f(s) / B with f(s) = s (1 - s) / (s + eps): Lipschitz constant 1/2 in d
                  (|df/dd| = s (1 - s) |eps (1 - 2 s) - s^2| / (s + eps)^2 <= 1/4 + 1/4), plus |f'(s)| s delta_s for the
                  rounding of s and 8 roundings on f
  * gradient rows each occurrence of a row in the batch adds one term (6 roundings each); k occurrences add k - 1 times
                  and the three gathers' gradients are joined (2 more adds): gamma(k + 8) on the sum of |terms|
  * backward      g_l = A g_{l+1} + w G:  E_l = |A| E_{l+1} + w E_G + gamma(nnz + 4) (|A| |g_{l+1}| + w |G|)
  * Adam          m' and v' are linear / quadratic in g: their propagated error is exact; the update
                  delta(g) = lr / bc1 * m'(g) / (sqrt(v'(g)) / sqrt(bc2) + eps) is taken over its exact range on
                  [g - E_g, g + E_g] (both ends and its stationary points), the roundings of m', v' and of the update
                  (10 roundings) are added to first order.  (The range is exact and costs no more than a first-order
                  term, so it is used for every element, not only where E_g is large next to |g| + eps.)
No constant here is fitted to data: each count above is the number of roundings of the expression it belongs to.
"""
import torch

U32 = 2.0 ** -24          # unit roundoff of fp32
E_TRANS = 4 * U32         # relative error of one expf / logf: within two ulps
EPS_BPR = 1e-5            # Model/LightGCN.py: log(sigmoid(d) + 1e-5)


def gamma(n):
    nu = n * U32
    return nu / (1.0 - nu)


def _csr(rowptr, col, val, n):
    rowptr = rowptr.detach().cpu().to(torch.int64)
    col = col.detach().cpu().to(torch.int64)
    val = val.detach().cpu().to(torch.float64)
    A = torch.sparse_csr_tensor(rowptr, col, val, (n, n))
    Aabs = torch.sparse_csr_tensor(rowptr, col, val.abs(), (n, n))
    nnz = (rowptr[1:] - rowptr[:-1]).to(torch.float64).unsqueeze(1)
    return A, Aabs, nnz


def torch_ref_csr(edge_index, n_nodes, dtype=torch.float64):
    """(rowptr, col, val) of the operator oracle/torch_ref.py:TorchRefLightGCN.conv applies -- y[col] += norm * x[row],
    norm = deg^-1/2[row] deg^-1/2[col] computed in `dtype` the way conv computes it -- as a CSR over destination rows."""
    row, col = edge_index.long()
    deg = torch.zeros(n_nodes, dtype=dtype).scatter_add_(0, row, torch.ones(row.numel(), dtype=dtype))
    dis = deg.pow(-0.5)
    norm = dis[row] * dis[col]
    order = torch.argsort(col * n_nodes + row)
    dst, src, norm = col[order], row[order], norm[order]
    rowptr = torch.zeros(n_nodes + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n_nodes), 0)
    return rowptr, src, norm


def _adam_delta(g, m, v, k, a, b2, c2, s2, eps):
    """the Adam update k m'(g) / (sqrt(v'(g)) / s2 + eps), m' = m + a (g - m), v' = b2 v + c2 g^2"""
    mp = m + a * (g - m)
    vp = b2 * v + c2 * g * g
    return k * mp / (vp.sqrt() / s2 + eps)


def _adam_range_error(g, Eg, m, v, k, a, b2, c2, s2, eps):
    """max |delta(g') - delta(g)| over g' in [g - Eg, g + Eg]: delta at both ends and at its stationary points.
    d delta / dg = 0  <=>  S = K g - J with S = sqrt(b2 v + c2 g^2), K = (1 - a) m c2 / (a eps s2), J = b2 v / (eps s2),
    i.e. (K^2 - c2) g^2 - 2 K J g + J^2 - b2 v = 0 (roots outside the interval are clamped into it: that only adds
    points of the interval)."""
    lo, hi = g - Eg, g + Eg
    d0 = _adam_delta(g, m, v, k, a, b2, c2, s2, eps)
    err = torch.maximum((_adam_delta(lo, m, v, k, a, b2, c2, s2, eps) - d0).abs(),
                        (_adam_delta(hi, m, v, k, a, b2, c2, s2, eps) - d0).abs())
    K = (1.0 - a) * m * c2 / (a * eps * s2)
    J = b2 * v / (eps * s2)
    A2, B2, C2 = K * K - c2, -2.0 * K * J, J * J - b2 * v
    disc = B2 * B2 - 4.0 * A2 * C2
    ok = (disc >= 0) & (Eg > 0)
    sq = torch.where(ok, disc, torch.zeros_like(disc)).sqrt()
    q = -0.5 * (B2 + torch.where(B2 >= 0, sq, -sq))
    cands = []
    with torch.no_grad():
        safe_q = torch.where(q != 0, q, torch.ones_like(q))
        safe_a = torch.where(A2 != 0, A2, torch.ones_like(A2))
        cands.append(torch.where(ok & (A2 != 0), q / safe_a, g))
        cands.append(torch.where(ok & (q != 0), C2 / safe_q, g))
    for r in cands:
        r = torch.minimum(torch.maximum(r, lo), hi)
        err = torch.maximum(err, (_adam_delta(r, m, v, k, a, b2, c2, s2, eps) - d0).abs())
    return d0, err


@torch.no_grad()
def lightgcn_step_fp64(rowptr, col, val, W, users, pos, neg, num_user, reg_weight, n_layers, m, v, t, lr,
                       betas=(0.9, 0.999), eps=1e-8):
    """One step from the joined table W [N, D] (users first), batch (users, pos, neg) with LOCAL item ids, Adam state
    (m, v [N, D]; t = the step number this step takes, 1 for the first).  -> dict of (value, bound) float64 pairs on the
    CPU: result [N, D] (the layer mean), loss (scalar), G [N, D] (d loss / d result), grad [N, D] (d loss / d W),
    m, v, W [N, D] (after the step)."""
    W = W.detach().cpu().to(torch.float64)
    N, D = W.shape
    L = int(n_layers)
    A, Aabs, nnz = _csr(rowptr, col, val, N)
    users = users.detach().cpu().long()
    pos = pos.detach().cpu().long() + num_user
    neg = neg.detach().cpu().long() + num_user
    B = users.numel()
    out = {}

    # forward: x_{l+1} = A x_l, the layer mean with weight 1 / (L + 1)
    xs, Es = [W], [torch.zeros_like(W)]
    for _ in range(L):
        x = xs[-1]
        xs.append(A @ x)
        Es.append(Aabs @ Es[-1] + gamma(nnz) * (Aabs @ x.abs()))
    w = 1.0 / (L + 1)
    R = w * sum(xs)
    ER = w * sum(Es) + gamma(L + 2) * w * sum(x.abs() for x in xs)
    out["result"] = (R, ER)

    # BPR + L2 on the propagated rows
    ru, rp, rn = R[users], R[pos], R[neg]
    eu, ep, en = ER[users], ER[pos], ER[neg]

    def dot(a, b, ea, eb):
        return (a * b).sum(1), gamma(D) * (a * b).abs().sum(1) + (a.abs() * eb + b.abs() * ea + ea * eb).sum(1)

    sp, Esp = dot(ru, rp, eu, ep)
    sn, Esn = dot(ru, rn, eu, en)
    d = sp - sn
    Ed = Esp + Esn + U32 * (sp.abs() + sn.abs() + Esp + Esn)
    s = torch.sigmoid(d)
    term = torch.log(s + EPS_BPR)
    delta_s = E_TRANS + 2 * U32                         # s = 1 / (1 + exp(-d)): exp, add, divide
    Eterm = Ed + (delta_s + 2 * U32) + E_TRANS * term.abs()     # (+ eps and its constant; log)
    bpr = -term.sum() / B
    Ebpr = (Eterm.sum() + gamma(B) * term.abs().sum()) / B + U32 * bpr.abs()
    sq = [(r * r).sum(1) for r in (ru, rp, rn)]
    Esq = [(2 * r.abs() * e + e * e).sum(1) for r, e in ((ru, eu), (rp, ep), (rn, en))]
    BD = float(B) * float(D)
    reg = reg_weight * sum(x.sum() for x in sq) / BD
    Ereg = reg_weight / BD * sum(gamma(B * D + 5) * x.sum() + e.sum() for x, e in zip(sq, Esq))
    loss = bpr + reg
    out["loss"] = (loss, Ebpr + Ereg + U32 * (bpr.abs() + reg.abs()))

    # d loss / d result: c = -f(s) / B per sample, r2 = 2 reg / (B D)
    f = s * (1 - s) / (s + EPS_BPR)
    fprime = (EPS_BPR * (1 - 2 * s) - s * s) / (s + EPS_BPR) ** 2
    c = -f / B
    Ec = (0.5 * Ed + fprime.abs() * s * delta_s + gamma(8) * f) / B
    r2 = 2.0 * reg_weight / BD
    c1 = c.unsqueeze(1)
    Ec1 = Ec.unsqueeze(1)
    val_u = c1 * (rp - rn) + r2 * ru
    val_p = c1 * ru + r2 * rp
    val_n = -c1 * ru + r2 * rn
    Eo_u = Ec1 * (rp - rn).abs() + (c1.abs() + Ec1) * (ep + en) + r2 * eu
    Eo_p = Ec1 * ru.abs() + (c1.abs() + Ec1) * eu + r2 * ep
    Eo_n = Ec1 * ru.abs() + (c1.abs() + Ec1) * eu + r2 * en
    Mo_u = c1.abs() * (rp.abs() + rn.abs()) + r2 * ru.abs()
    Mo_p = c1.abs() * ru.abs() + r2 * rp.abs()
    Mo_n = c1.abs() * ru.abs() + r2 * rn.abs()
    rows = torch.cat((users, pos, neg))
    G = torch.zeros_like(W).index_add_(0, rows, torch.cat((val_u, val_p, val_n)))
    EGp = torch.zeros_like(W).index_add_(0, rows, torch.cat((Eo_u, Eo_p, Eo_n)))
    MG = torch.zeros_like(W).index_add_(0, rows, torch.cat((Mo_u, Mo_p, Mo_n)))
    k = torch.bincount(rows, minlength=N).to(torch.float64).unsqueeze(1)
    EG = EGp + gamma(k + 8) * MG
    out["G"] = (G, EG)

    # backward: g_L = w G, g_l = A g_{l+1} + w G
    g, Eg = w * G, w * EG
    for _ in range(L):
        g_new = A @ g + w * G
        Eg = Aabs @ Eg + w * EG + gamma(nnz + 4) * (Aabs @ g.abs() + w * G.abs())
        g = g_new
    out["grad"] = (g, Eg)

    # Adam (torch.optim.Adam, weight_decay 0)
    m = m.detach().cpu().to(torch.float64)
    v = v.detach().cpu().to(torch.float64)
    b1, b2 = float(betas[0]), float(betas[1])
    a, c2 = 1.0 - b1, 1.0 - b2
    bc1 = 1.0 - b1 ** t
    s2 = (1.0 - b2 ** t) ** 0.5
    kk = lr / bc1
    gh = g.abs() + Eg
    mp = m + a * (g - m)
    vp = b2 * v + c2 * g * g
    Rm = gamma(4) * (m.abs() + a * (gh + m.abs()))
    Rv = gamma(6) * (b2 * v + c2 * gh * gh)
    out["m"] = (mp, a * Eg + Rm)
    out["v"] = (vp, c2 * (2 * g.abs() * Eg + Eg * Eg) + Rv)
    delta, Edg = _adam_range_error(g, Eg, m, v, kk, a, b2, c2, s2, eps)
    den = vp.sqrt() / s2 + eps
    root = vp.sqrt()
    dsqrt = torch.minimum(torch.where(root > 0, Rv / (2 * root.clamp_min(1e-300)), torch.full_like(Rv, float("inf"))),
                          Rv.sqrt())
    dmax = delta.abs() + Edg
    EW = Edg + kk * Rm / den + dmax * dsqrt / (s2 * den) + gamma(10) * dmax + U32 * (W.abs() + dmax)
    out["W"] = (W - delta, EW)
    return out


def excess(got, ref):
    """max over the elements of |got - value| / bound (inf where the bound is 0 and got differs); <= 1 passes."""
    value, bound = ref
    err = (got.detach().cpu().to(torch.float64) - value).abs()
    r = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                    torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0
