"""The MLA prefill backward's reference, bound and rounding model (test side only; numpy, fp64; shared by tests/test_mla_bwd_cases.py on
the CPU and tests/test_gpu_mla_bwd.py on the GPU). fa_bwd_varlen_mla (include/fa_mi355.h, "Multi-head latent attention (prefill,
backward)") is, per sequence, fa_bwd_ex's operator with two head dims: q / k rows of 192 columns, v / dO / O rows of 128. The bound is
tests/backward_bound.py's per (sequence, head) -- head_exact / head_bounds / head_model take the two widths as they are -- and the bounds
of a key head's query heads add up as backward_bound._per_head adds them. No fitted factor: the test condition is
|gradient - exact| <= bound on every element. Rows without a visible key are cut before head_exact is called (tests/varlen_backward.py):
their dQ is 0 with bound 0, and so is their share of dK / dV.

The cases are the forward's own (tests/mla_prefill.py: case("seqs" | "edges", heads, dtype)); dO is drawn here, U(-1, 1) rounded to the type.

The chain (the backward on the O and LSE fa_fwd_varlen_mla wrote): tests/chain_bound.head_errors assumes one head dim, so the two terms of
its docstring are spelt out here for the MLA forward (pre-scaled query operand, fp32 row sum over unrounded probabilities):
    lse_err_i = 1e-4 + eps * scale * |q_i|_2 * max_j |k_j|_2                                    eps = 2^-9 bf16 / 2^-12 f16
    o_err_id  = u |O_id| + (u + expm1(2 max_j d_ij) + 2^-24 (visible keys_i + tiles)) * sum_j P_ij |v_jd|
and handed to head_bounds(lse_err=, o_err=).

Planted mistakes of a two-head-dim backward (BUGS), each beyond the bound on the case BUG_CASE names, in both dtypes."""
import numpy as np

import backward_bound as bb
import mla_prefill as mp
from chain_bound import PRESCALE_EPS, TILE
from varlen_backward import first_live_row

DQK, DV, DNOPE = mp.DQK, mp.DV, mp.DNOPE
SCALE = mp.SCALE
BUGS = ("delta_192", "dp_k_pitch", "dk_no_rope", "dv_nope_p", "scale_dv", "top_left", "head_mod", "dk_last_head")
# the case each planted mistake is caught on: (catalogue, heads, causal)
BUG_CASE = {"delta_192": ("seqs", (4, 4), False), "dp_k_pitch": ("seqs", (4, 4), False), "dk_no_rope": ("seqs", (4, 4), False),
            "dv_nope_p": ("seqs", (4, 4), True), "scale_dv": ("seqs", (4, 4), False), "top_left": ("seqs", (4, 4), True),
            "head_mod": ("seqs", (8, 2), False), "dk_last_head": ("seqs", (8, 2), True)}
# every GPU parity case: (catalogue, heads, dtype, causal)
PARITY = ([("seqs", h, t, c) for h in mp.HEADS for t in mp.DTYPES for c in (False, True)] +
          [("edges", (8, 2), t, c) for t in mp.DTYPES for c in (False, True)])

_DO, _SEQ = {}, {}


def _ro(x):
    x.setflags(write=False)
    return x


def d_out(c):
    """dO [total_q, Hq, 128] of a forward case: fp32 array holding values of the case's dtype; drawn once, read-only."""
    key = (c["name"], c["heads"], c["dtype"])
    if key not in _DO:
        rng = np.random.default_rng(7700 + 10 * c["heads"][0] + c["heads"][1] + (0 if c["name"] == "seqs" else 1000))
        _DO[key] = _ro(bb.rnd(rng.uniform(-1.0, 1.0, (len(c["q"]), c["heads"][0], DV)).astype(np.float32), c["dtype"]))
    return _DO[key]


def sequence(c, b):
    """(q [Hq, Lq, 192], k [Hkv, Lk, 192], v [Hkv, Lk, 128], do [Hq, Lq, 128]) of sequence b of a case."""
    q0, q1, k0, k1 = c["cu_q"][b], c["cu_q"][b + 1], c["cu_k"][b], c["cu_k"][b + 1]
    return tuple(x.transpose(1, 0, 2) for x in (c["q"][q0:q1], c["k"][k0:k1], c["v"][k0:k1], d_out(c)[q0:q1]))


def forward_errors(q, k, v, causal, scale, dtype, R):
    """(lse_err [Nq], o_err [Nq, 128]) of fa_fwd_varlen_mla for one head's live rows: the two terms of the module docstring."""
    aq, ak, av = (np.abs(np.asarray(x, np.float64)) for x in (q, k, v))
    Nq, Nk = aq.shape[0], ak.shape[0]
    u = bb.U[dtype]
    vis = np.ones((Nq, Nk), bool) if R["mask"] is None else R["mask"]
    qn, kn = np.sqrt((aq ** 2).sum(-1)), float(np.sqrt((ak ** 2).sum(-1)).max())
    lse_err = 1e-4 + PRESCALE_EPS[dtype] * scale * qn * kn
    dmax = (u * scale * np.where(vis, aq @ ak.T, 0.0)).max(1)
    rel = u + np.expm1(2.0 * dmax) + bb.U32 * (vis.sum(1) + (Nk + TILE - 1) // TILE)
    return lse_err, u * np.abs(R["o"]) + rel[:, None] * (R["p"] @ av)


class SeqBounds:
    """One sequence: ref = exact (dQ [Hq, Lq, 192], dK [Hkv, Lk, 192], dV [Hkv, Lk, 128]), bound = their bounds, o [Hq, Lq, 128] and lse
    [Hq, Lq] of the exact forward (0 and -inf on rows without a visible key). chain=True: the bound of the TRUE gradient for a backward
    fed the O and LSE of fa_fwd_varlen_mla (forward_errors). model(bug) is the kernels' rounding model, with one of BUGS planted."""

    def __init__(self, q, k, v, do, causal, scale, dtype, chain=False):
        self.q, self.k, self.v, self.do = q, k, v, do
        self.causal, self.dtype, self.scale = causal, dtype, float(scale)
        Hq, Lq, _ = q.shape
        Hkv, Lk = k.shape[0], k.shape[1]
        self.G, self.n0 = Hq // Hkv, first_live_row(Lq, Lk, causal)
        self.o, self.lse = np.zeros(do.shape), np.full((Hq, Lq), -np.inf)
        self.ref = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(v.shape))
        self.bound = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(v.shape))
        self.R = {}
        n0 = self.n0
        if n0 >= Lq:
            return
        for h in range(Hq):
            hk = h // self.G
            R = bb.head_exact(q[h, n0:], k[hk], v[hk], do[h, n0:], causal, self.scale)
            le, oe = forward_errors(q[h, n0:], k[hk], v[hk], causal, self.scale, dtype, R) if chain else (None, None)
            B = bb.head_bounds(q[h, n0:], k[hk], v[hk], do[h, n0:], self.scale, dtype, R, le, oe)
            self.R[h] = R
            self.o[h, n0:], self.lse[h, n0:] = R["o"], R["lse"]
            self.ref[0][h, n0:] = R["dq"]
            self.ref[1][hk] += R["dk"]
            self.ref[2][hk] += R["dv"]
            self.bound[0][h, n0:] = B[0]
            self.bound[1][hk] += B[1]
            self.bound[2][hk] += B[2]

    def model(self, bug=None):
        q, k, v, do, n0, dtype = self.q, self.k, self.v, self.do, self.n0, self.dtype
        Hq, Hkv = q.shape[0], k.shape[0]
        out = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(v.shape))
        for h, R in self.R.items():
            hk = h % Hkv if bug == "head_mod" else h // self.G
            if bug is None or bug == "head_mod":
                g = bb.head_model(q[h, n0:], k[hk], v[hk], do[h, n0:], self.causal, self.scale, dtype, R)
            else:
                g = _bugged_head(bug, q, k, v, do, h, hk, n0, self.causal, self.scale, dtype, R, self.R)
            out[0][h, n0:] = g[0]
            if bug == "dk_last_head":  # the group's dK is its last query head's alone
                if h % self.G == self.G - 1:
                    out[1][hk] = g[1]
            else:
                out[1][hk] += g[1]
            out[2][hk] += g[2]
        return out


def _bugged_head(bug, q, k, v, do, h, hk, n0, causal, scale, dtype, R, Rs):
    """backward_bound.head_model's arithmetic for one head with one structural mistake (its roundings, everything else exact)."""
    Hq, Hkv = q.shape[0], k.shape[0]
    qh, kh, vh, doh = (np.asarray(x, np.float32) for x in (q[h, n0:], k[hk], v[hk], do[h, n0:]))
    Lq, Lk = qh.shape[0], kh.shape[0]
    kscale = DV ** -0.5 if bug == "scale_dv" else scale
    c2 = np.float32(np.float32(kscale) * bb.LOG2E32)
    o = bb.rnd(R["o"], dtype).astype(np.float64)
    do64, v64, q64, k64 = (x.astype(np.float64) for x in (doh, vh, qh, kh))
    delta = (do64 * o).sum(-1, keepdims=True)
    if bug == "delta_192":  # rows of dO / O read 192 wide: the 64 columns behind a head's 128 are the next head's first 64
        hn = (h + 1) % Hq
        on = bb.rnd(Rs[hn]["o"], dtype).astype(np.float64)
        delta = delta + (np.asarray(do[hn, n0:], np.float64)[:, :DQK - DV] * on[:, :DQK - DV]).sum(-1, keepdims=True)
    if bug == "dp_k_pitch":  # the value tensor [Lk, Hkv, 128] walked with the key's row pitch Hkv * 192 (wrapped into the buffer)
        flat = np.ascontiguousarray(np.asarray(v, np.float64).transpose(1, 0, 2)).reshape(-1)
        j, d = np.meshgrid(np.arange(Lk), np.arange(DV), indexing="ij")
        v64 = flat[(j * Hkv * DQK + hk * DV + d) % flat.size]
    dpp = do64 @ v64.T - delta
    lse2 = (np.asarray(R["lse"]).astype(np.float32) * bb.LOG2E32).astype(np.float64)
    mask = R["mask"]
    if bug == "top_left" and causal:
        mask = np.arange(Lk)[None, :] <= (np.arange(Lq)[:, None] + n0)

    def prob(s2):
        s2 = s2 - lse2[:, None]
        return np.exp2(s2 if mask is None else np.where(mask, s2, -np.inf))

    p1 = prob(bb.rnd(qh * c2, dtype).astype(np.float64) @ k64.T)  # the dQ kernel
    dq = kscale * (bb.rnd(p1 * dpp, dtype).astype(np.float64) @ k64)
    kt = bb.rnd(kh * c2, dtype).astype(np.float64)
    p2 = prob(q64 @ kt.T)  # the dK/dV kernel
    dk = kscale * (bb.rnd(p2 * dpp, dtype).astype(np.float64).T @ q64)
    pv = prob(q64[:, :DNOPE] @ kt[:, :DNOPE].T) if bug == "dv_nope_p" else p2
    dv = bb.rnd(pv, dtype).astype(np.float64).T @ do64
    if bug == "dk_no_rope":
        dk[:, DNOPE:] = 0.0
    return dq, dk, dv


def seq_bounds(c, b, causal, chain=False):
    """SeqBounds of sequence b of a case; computed once per (case, sequence, causal, chain) and shared."""
    key = (c["name"], c["heads"], c["dtype"], b, bool(causal), bool(chain))
    if key not in _SEQ:
        _SEQ[key] = SeqBounds(*sequence(c, b), causal, SCALE, c["dtype"], chain)
    return _SEQ[key]


def worst_ratio(grads, sb):
    """Worst |g - ref| / bound over the three gradients of one sequence (a bound of exactly 0 requires the exact value); NaN / Inf
    anywhere counts as infinite."""
    if not all(np.isfinite(np.asarray(g, np.float64)).all() for g in grads):
        return float("inf")
    return max(bb.ratios(grads, sb.ref, sb.bound))


def packed(c, causal, what):
    """`what` in ("o", "lse", "ref", "bound") of every sequence, packed as the call takes / returns them: o [total_q, Hq, 128],
    lse [Hq, total_q], ref / bound = ([total_q, Hq, 192], [total_k, Hkv, 192], [total_k, Hkv, 128])."""
    sbs = [seq_bounds(c, b, causal) for b in range(len(c["lens"]))]
    if what == "o":
        return np.concatenate([s.o.transpose(1, 0, 2) for s in sbs])
    if what == "lse":
        return np.concatenate([s.lse for s in sbs], axis=1)
    return tuple(np.concatenate([getattr(s, what)[i].transpose(1, 0, 2) for s in sbs]) for i in range(3))
