"""Inputs and references shared by tests/test_bpr_multi_host.py (CPU) and tests/test_gpu_bpr_multi.py (GPU): the case table of
the multi-term BPR launches (chaorec_bpr_multi_fwd_f32 / _bwd_f32 / _bwd_ordered_f32), one seeded input builder so that both
files see the same inputs, the derived error bound of a float row sum, and a second, numpy restatement of the defined order
of the ordered backward that can also produce the WRONG orders the tests must be able to tell from the right one.  Also the
guarded device buffers (`Guarded`) that tests/test_gpu_bpr_multi.py and tests/test_gpu_rowops.py let the launches write into."""
import numpy as np
from accept import ULP24 as U24  # noqa: F401  (unit roundoff of float32)

U_ROWS, I_ROWS, TABLE_ROWS = 37, 23, 40       # user table, plain item table, the longer table gathered blocks map onto
WVEC = (1.0, 1e-3, 0.0, -0.37)                # a unit, a small, a zero and a negative weight
GRAD_OUT = 0.7

# (T, B, D, variant): what each case reaches in csrc/bpr.hip is listed in tests/test_gpu_bpr_multi.py
CASES = [
    (1, 1, 4, 1),
    (2, 5, 16, 0),
    (3, 257, 64, 1),
    (4, 300, 128, 2),
    (3, 100, 192, 1),
    (2, 64, 256, 0),
    (1, 40, 260, 1),
    (3, 2049, 64, 1),
    (3, 2049, 128, 1),
    (3, 2049, 256, 1),
    (4, 4096, 64, 1),
    (4, 4097, 64, 1),
]
ORD_MAX_SLOTS, ORD_MAX_D = 16384, 256         # kOrdMaxSlots and the widest row of the ordered launch (csrc/bpr.hip)


def case_id(case):
    return "T%d-B%d-D%d-v%d" % case


def is_ordered(case):
    """The ordered launch takes the case (else: the atomic fallback).  The largest group is max(T B, 2 B) slots."""
    T, B, D, _ = case
    return max(T, 2) * B <= ORD_MAX_SLOTS and D <= ORD_MAX_D


def gathered_terms(T):
    """FREEDOM's form: term 0 reads the propagated item table, terms 1 and 2 read gathered row blocks (their gradient is also
    scattered); a fourth term is a plain table again, so an empty scatter group lies between live groups and at the end."""
    return [k in (1, 2) for k in range(T)]


def build_case(case):
    """Seeded inputs of one case.  Tables of 37 / 23 rows and 2 B-row gathered blocks whose rows map onto 40 table rows: with
    B >= 64 every destination row collects dozens of addends.  T = 2, B = 5 has ALL users equal; wherever B >= 8 every
    seventh sample of every term has pos == neg.  The gradient buffers start from non-zero values."""
    T, B, D, variant = case
    rng = np.random.default_rng([T, B, D, variant])
    f32 = lambda *shape: (rng.standard_normal(shape) * 0.3).astype(np.float32)
    inp = dict(case=case, T=T, B=B, D=D, variant=variant, tab_u=f32(U_ROWS, D), users=rng.integers(0, U_ROWS, B),
               wvec=np.asarray(WVEC[:T], np.float32), tabs=[], pos=[], neg=[], scatter_rows=[], scatter_sizes=[])
    if (T, B) == (2, 5):
        inp["users"][:] = 11
    for k, gathered in enumerate(gathered_terms(T)):
        rows = 2 * B if gathered else I_ROWS
        inp["tabs"].append(f32(rows, D))
        if gathered and k == 1:                       # FREEDOM's ids: the block is [rows of pos ; rows of neg]
            p, n = np.arange(B, dtype=np.int64), np.arange(B, dtype=np.int64) + B
        else:                                         # few distinct rows: they repeat inside the batch
            p, n = rng.integers(0, min(rows, 31), B), rng.integers(0, min(rows, 31), B)
        if B >= 8:
            n[::7] = p[::7]
        inp["pos"].append(p.astype(np.int64))
        inp["neg"].append(n.astype(np.int64))
        inp["scatter_rows"].append(rng.integers(0, TABLE_ROWS, rows) if gathered else None)
        inp["scatter_sizes"].append(TABLE_ROWS if gathered else 0)
    if not any(gathered_terms(T)):
        inp["scatter_rows"] = None
    # What the gradient buffers hold before the launch: non-zero, and about 2^-10 of ONE addend of that buffer (|coef| ~ 0.5 / B,
    # times grad_out, the term's weight and a table element ~ 0.3): enough to move the low bits of every sum, so a launch that
    # did not start from the buffer's value fails the bit comparison.  sum_bound() counts the initial value as one exact term that
    # is rounded ONCE; a value above the row's addends is instead rounded again at every addition, n times |initial| 2^-24, which
    # no bound of that form covers -- with values of the size of an addend the float oracle itself exceeded it by 1.4 x in the
    # elements whose addends happen to be small.  (A zero-weight term adds zeros: any value stays.)
    size = lambda k: 1e-4 / B * (abs(WVEC[k]) if WVEC[k] != 0 else 1.0)
    inp["init_u"] = (rng.standard_normal((U_ROWS, D)) * size(0)).astype(np.float32)
    inp["init_i"] = [(rng.standard_normal(t.shape) * size(k)).astype(np.float32) for k, t in enumerate(inp["tabs"])]
    inp["init_s"] = [(rng.standard_normal((TABLE_ROWS, D)) * size(k)).astype(np.float32) if g else None
                     for k, g in enumerate(gathered_terms(T))]
    return inp


def sum_bound(abs_sum, count, initial=None):
    """|float sum - exact sum| of one gradient element, whatever the order of the additions: (n + 4) 2^-24 S with n the number
    of addends and S the sum of their magnitudes.  An addend is  (coef * (grad_out * w)) * (p - n)  or  (coef * (grad_out * w)) * u:
    at most four roundings, 4 u S to first order; a float sum of n terms adds at most (n - 1) u S' with S' the sum of the
    rounded magnitudes; a buffer that starts from `initial` takes part in the sum as one more, exact, term: |initial| u."""
    b = (count + 4.0) * U24 * abs_sum
    return b if initial is None else b + np.abs(initial.astype(np.float64)) * U24


def _row_sums(dst, rows, addends):
    """dst[rows[j]] += addends[j], j ascending, in float32: one running sum per row."""
    for j in range(len(rows)):
        dst[rows[j]] += addends[j]


def ordered_numpy(inp, coef, grad_out, order="defined"):
    """The ordered backward in numpy float32 from zero-filled buffers: `defined` is the order of oracle_bpr_multi_bwd_ordered_f32
    (a second statement of it, independent of the C one); the others are the mistakes a repeatable kernel could make:
      neg_first     the negative slots of an item table before its positive slots
      sample_major  the user rows' addends sample by sample, the terms inside a sample
      w_after       the weight of a term applied to the row sum of the term instead of to every addend
    -> (g_u, [g_i], [scattered or None])."""
    T, B, D = inp["T"], inp["B"], inp["D"]
    f = np.float32
    coef = np.asarray(coef, f).reshape(T, B)
    go, w = f(grad_out), inp["wvec"]
    tab_u, users = inp["tab_u"], inp["users"]
    u = tab_u[users]
    late = order == "w_after"
    c = [(coef[k] * (go if late else go * w[k]))[:, None].astype(f) for k in range(T)]
    user_add = [c[k] * (inp["tabs"][k][inp["pos"][k]] - inp["tabs"][k][inp["neg"][k]]) for k in range(T)]
    g_u = np.zeros((U_ROWS, D), f)
    if late:
        for k in range(T):
            part = np.zeros_like(g_u)
            _row_sums(part, users, user_add[k])
            g_u += part * w[k]
    elif order == "sample_major":
        _row_sums(g_u, np.repeat(users, T), np.stack(user_add, 1).reshape(T * B, D))
    else:
        _row_sums(g_u, np.tile(users, T), np.concatenate(user_add))
    g_i, g_s = [], []
    for k in range(T):
        roles = [(inp["pos"][k], c[k] * u), (inp["neg"][k], (-c[k]) * u)]
        if order == "neg_first":
            roles.reverse()
        rows, add = np.concatenate([r for r, _ in roles]), np.concatenate([a for _, a in roles])
        targets = [(g_i, inp["tabs"][k].shape[0], rows)]
        if inp["scatter_rows"] is not None and inp["scatter_rows"][k] is not None:
            targets.append((g_s, TABLE_ROWS, inp["scatter_rows"][k][rows]))
        else:
            g_s.append(None)
        for out, n_rows, r in targets:
            g = np.zeros((n_rows, D), f)
            _row_sums(g, r, add)
            out.append(g * w[k] if late else g)
    return g_u, g_i, g_s


def flat(grads):
    """(g_u, [g_i], [scattered or None]) -> one float vector (for whole-result comparisons)."""
    g_u, g_i, g_s = grads
    return np.concatenate([np.ravel(g_u)] + [np.ravel(g) for g in g_i] + [np.ravel(g) for g in g_s if g is not None])


SENTINEL = 0x7FC0BEEF          # a NaN pattern no launch under test produces
GUARD = 64                     # guard words before, between and after the buffers


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


class Guarded:
    """Float buffers inside ONE allocation of sentinel words: [guard | b0 | guard | b1 | ... | guard]."""

    def __init__(self, dev, inits):
        self.shapes = [a.shape for a in inits]
        self.offs, n = [], GUARD
        for a in inits:
            self.offs.append(n)
            n += a.size + GUARD
        host = np.full(n, SENTINEL, np.int32)
        self.is_guard = np.ones(n, bool)
        for a, o in zip(inits, self.offs):
            host[o:o + a.size] = bits(a).ravel()
            self.is_guard[o:o + a.size] = False
        import torch
        self.flat = torch.from_numpy(host).to(dev)
        self.views = [self.flat[o:o + int(np.prod(s))].view(torch.float32).view(*s) for o, s in zip(self.offs, self.shapes)]

    def read(self):
        """-> the buffers as numpy arrays; asserts that no guard word changed."""
        host = self.flat.cpu().numpy()
        assert np.all(host[self.is_guard] == SENTINEL), "a launch wrote outside its buffers"
        return [host[o:o + int(np.prod(s))].view(np.float32).reshape(s).copy() for o, s in zip(self.offs, self.shapes)]
