"""Per-sequence reference, bound and walk model for the sliding-window varlen backward (test side only; numpy, fp64):
varlen_backward.SeqBounds under a window. The mask comes from window.visible; rows without a visible key form a prefix (i + cu < 0, or
all rows when Lk = 0) and are cut before the fp64 reference, as varlen_backward cuts them; backward_bound.head_bounds and head_model are
used unchanged -- both take their mask from R["mask"].

Also here: query_range(), the inverse of window.key_range by brute force; forward_errors(), chain_bound's lse_err / o_err of the `mfma`
route under a window's visibility (the GPU tests run the backward on the forward's own O and LSE); and walk(), a model of both kernels'
walks -- block ranges, tile loops, wave skips, two-sided masks, dead rows -- which returns the visibility each kernel effectively applies,
with one planted mistake at a time:
    "lo_edge" / "hi_edge"   either mask off by one (in both kernels)
    "dq_start_last_row"     dQ's first tile taken from the block's LAST row's lower bound
    "dkdv_end_first_key"    dK/dV's last query tile taken from the block's FIRST key
    "skip_too_much"         a wave skip that drops a sub-tile with exactly one visible pair (the test against the lower bound, strict
                            where it must not be, in both kernels)
    "dead_by_coff"          the dead-row test with coff where cu belongs"""
import numpy as np

import backward_bound as bb
import chain_bound as cb
from window import BLOCK, TILE, WAVE, visible

BUGS = ("lo_edge", "hi_edge", "dq_start_last_row", "dkdv_end_first_key", "skip_too_much", "dead_by_coff")


def first_live_row(Lq, Lk, wl, wr):
    """Query rows [0, n0) of a sequence see no key: Lk = 0, or i + coff + wr < 0 (the forward's integer test)."""
    if Lk == 0:
        return Lq
    return 0 if wr < 0 else min(Lq, max(0, -(Lk - Lq + wr)))


def query_range(Lq, Lk, wl, wr, k0, k1):
    """Brute force over the rule: (lo, hi) of the rows that see one of the keys k0 .. k1, or None when none does."""
    vis = visible(Lq, Lk, wl, wr)[:, max(k0, 0):max(k1 + 1, 0)]
    rows = np.nonzero(vis.any(1))[0] if vis.size else np.array([], int)
    return (int(rows[0]), int(rows[-1]) + 1) if len(rows) else None


def head_exact(q, k, v, do, mask, scale):
    """backward_bound.head_exact under an arbitrary mask [Nq, Nk] in which every row sees a key."""
    q, k, v, do = (np.asarray(x, np.float64) for x in (q, k, v, do))
    s = np.where(mask, (q @ k.T) * scale, -np.inf)
    m = s.max(-1, keepdims=True)
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    p /= l
    o = p @ v
    dp = do @ v.T
    delta = (do * o).sum(-1, keepdims=True)
    ds = p * (dp - delta)
    return dict(p=p, ds=ds, dp=dp, delta=delta, o=o, lse=(m + np.log(l))[:, 0], mask=mask, dq=scale * (ds @ k), dk=scale * (ds.T @ q), dv=p.T @ do)


def forward_errors(q, k, v, mask, scale, dtype, R):
    """(lse_err [Nq], o_err [Nq, D]) of tests/chain_bound.py for the `mfma` route -- the kernel the windowed forward is a mode of: a
    pre-scaled query operand, unrounded row sum, no splits -- with the visible pairs taken from `mask` (chain_bound.head_errors knows the
    causal mask only; on it the two agree, tests/test_window_bwd_cases.py)."""
    kern = cb.KERNELS["mfma"]
    assert kern.prescaled and not kern.sum_rounded and not kern.fp8pv and not kern.splits and q.shape[1] <= 128
    aq, ak, av = (np.abs(np.asarray(x, np.float64)) for x in (q, k, v))
    u = bb.U[dtype]
    nvis = mask.sum(1)
    tiles = (ak.shape[0] + cb.TILE - 1) // cb.TILE
    A = R["p"] @ av
    out_round = cb.U_OUT[dtype] * np.abs(R["o"])
    if dtype == "f16":
        out_round = np.maximum(out_round, 2.0 ** -25)
    qn, kn = np.sqrt((aq ** 2).sum(-1)), float(np.sqrt((ak ** 2).sum(-1)).max())
    dmax = (u * scale * np.where(mask, aq @ ak.T, 0.0)).max(1)
    lse_err = np.full(aq.shape[0], 1e-4) + cb.PRESCALE_EPS[dtype] * scale * qn * kn
    rel = u + np.expm1(2.0 * dmax) + bb.U32 * (nvis + tiles)
    return lse_err, out_round + rel[:, None] * A


class SeqBounds:
    """One sequence under the window (wl, wr): ref = exact (dQ, dK, dV), bound = their bounds, o [Hq, Lq, D] and lse [Hq, Lq] of the exact
    forward (0 and -inf on rows without a visible key). chain=True: the bound of the TRUE gradient for a backward fed the O and LSE of the
    `mfma` forward (forward_errors); else for one fed the exact O rounded to the type and the exact LSE. model(fn) applies a per-head
    model fn(h, q_h, k_h, v_h, do_h, R) -> (dq, dk, dv) of the LIVE rows (default: backward_bound.head_model) and assembles it like the
    reference."""

    def __init__(self, q, k, v, do, wl, wr, scale, dtype, chain=False):
        self.q, self.k, self.v, self.do = q, k, v, do
        self.wl, self.wr, self.dtype = wl, wr, dtype
        self.scale = bb.default_scale(q.shape[-1]) if scale is None else float(scale)
        Hq, Lq, D = q.shape
        Hkv, Lk = k.shape[0], k.shape[1]
        self.G, self.n0 = Hq // Hkv, first_live_row(Lq, Lk, wl, wr)
        self.vis = visible(Lq, Lk, wl, wr)
        self.unseen = ~self.vis.any(0) if Lq else np.ones(Lk, bool)
        self.o, self.lse = np.zeros(q.shape), np.full((Hq, Lq), -np.inf)
        self.ref = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        self.bound = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        self.R = {}
        n0 = self.n0
        if n0 >= Lq:
            return
        mask = self.vis[n0:]
        assert mask.any(1).all() and not self.vis[:n0].any()  # the dead rows are exactly the prefix
        for h in range(Hq):
            hk = h // self.G
            R = head_exact(q[h, n0:], k[hk], v[hk], do[h, n0:], mask, self.scale)
            le, oe = forward_errors(q[h, n0:], k[hk], v[hk], mask, self.scale, dtype, R) if chain else (None, None)
            B = bb.head_bounds(q[h, n0:], k[hk], v[hk], do[h, n0:], self.scale, dtype, R, le, oe)
            self.R[h] = R
            self.o[h, n0:], self.lse[h, n0:] = R["o"], R["lse"]
            self.ref[0][h, n0:] = R["dq"]
            self.ref[1][hk] += R["dk"]
            self.ref[2][hk] += R["dv"]
            self.bound[0][h, n0:] = B[0]
            self.bound[1][hk] += B[1]
            self.bound[2][hk] += B[2]

    def model(self, fn=None):
        q, k, v, do, n0 = self.q, self.k, self.v, self.do, self.n0
        out = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        for h, R in self.R.items():
            hk = h // self.G
            if fn is None:
                g = bb.head_model(q[h, n0:], k[hk], v[hk], do[h, n0:], True, self.scale, self.dtype, R)
            else:
                g = fn(h, q[h, n0:], k[hk], v[hk], do[h, n0:], R)
            out[0][h, n0:] = g[0]
            out[1][hk] += g[1]
            out[2][hk] += g[2]
        return out

    def walk_model(self, bug=None, max_q=None, max_k=None):
        """The three gradients as kernels that walk like walk(bug) form them: head_model under the visibility each kernel applies."""
        Lq, Lk = self.q.shape[1], self.k.shape[1]
        eff_dq, eff_kv = walk(Lq, Lk, self.wl, self.wr, bug, max_q, max_k)
        n0 = self.n0

        def fn(h, q, k, v, do, R):
            a = bb.head_model(q, k, v, do, True, self.scale, self.dtype, dict(R, mask=eff_dq[n0:]))
            b = bb.head_model(q, k, v, do, True, self.scale, self.dtype, dict(R, mask=eff_kv[n0:]))
            return a[0], b[1], b[2]
        return self.model(fn)


def walk(Lq, Lk, wl, wr, bug=None, max_q=None, max_k=None):
    """(eff_dq, eff_kv) bool [Lq, Lk]: the pairs the dQ kernel and the dK/dV kernel treat as visible (csrc/fa_bwd_dq_body.inc and
    fa_bwd_dkdv_body.inc, window mode), in Python ints. max_q / max_k: the call's max_seqlen (the host's clamp of an unbounded side)."""
    max_q, max_k = max(Lq, max_q or 0), max(Lk, max_k or 0)
    wl_ = max_k if (wl < 0 or wl > max_k) else wl
    wr_ = max_q if (wr < 0 or wr > max_q) else wr
    coff = Lk - Lq
    cl, cu = coff - wl_, coff + wr_
    e_lo, e_hi = (1 if bug == "lo_edge" else 0), (1 if bug == "hi_edge" else 0)
    skip = 1 if bug == "skip_too_much" else 0
    live = (np.arange(Lq) + (coff if bug == "dead_by_coff" else cu) >= 0) & (Lk > 0)
    eff_dq, eff_kv = np.zeros((Lq, Lk), bool), np.zeros((Lq, Lk), bool)
    # dQ: 128 query rows per block, 32 per wave, 64-key tiles of the block's key range
    for q0 in range(0, Lq, BLOCK):
        r_last = min(q0 + BLOCK - 1, Lq - 1)
        lo = min(max(0, (r_last if bug == "dq_start_last_row" else q0) + cl), Lk)
        hi = min(max(0, r_last + cu + 1), Lk)
        if lo >= hi or Lk == 0:
            continue
        for qw0 in range(q0, min(q0 + BLOCK, Lq), WAVE):
            rows = np.arange(qw0, min(qw0 + WAVE, Lq))
            for t in range(lo // TILE, (hi + TILE - 1) // TILE):
                kv0 = t * TILE
                if not kv0 < hi or kv0 > qw0 + WAVE - 1 + cu or kv0 + TILE - 1 < qw0 + cl + skip:
                    continue
                keys = np.arange(kv0, min(kv0 + TILE, Lk))
                m = np.ones((len(rows), len(keys)), bool)
                if kv0 + TILE - 1 > qw0 + cu or kv0 < qw0 + WAVE - 1 + cl or kv0 + TILE > Lk:
                    m = (keys[None, :] <= rows[:, None] + cu + e_hi) & (keys[None, :] >= rows[:, None] + cl + e_lo)
                eff_dq[np.ix_(rows, keys)] = m & live[rows][:, None]
    # dK/dV: 128 keys per block, 32 per wave, 64-query tiles of the block's query range
    for k0 in range(0, Lk, BLOCK):
        k_last = min(k0 + BLOCK - 1, Lk - 1)
        lo = min(max(0, k0 - cu), Lq)
        hi = min(max(0, (k0 if bug == "dkdv_end_first_key" else k_last) - cl + 1), Lq)
        if lo >= hi:
            continue
        for kw0 in range(k0, min(k0 + BLOCK, Lk), WAVE):
            keys = np.arange(kw0, min(kw0 + WAVE, Lk))
            for t in range(lo // TILE, (hi + TILE - 1) // TILE):
                qt0 = t * TILE
                if not qt0 < Lq or qt0 + TILE - 1 + cu < kw0 or qt0 + cl + skip > kw0 + WAVE - 1:
                    continue
                rows = np.arange(qt0, min(qt0 + TILE, Lq))
                m = np.ones((len(rows), len(keys)), bool)
                if qt0 + cu < kw0 + WAVE - 1 or qt0 + TILE - 1 + cl > kw0:
                    m = (rows[:, None] >= keys[None, :] - cu - e_hi) & (rows[:, None] <= keys[None, :] - cl - e_lo)
                eff_kv[np.ix_(rows, keys)] = m & live[rows][:, None]
    return eff_dq, eff_kv


def worst_ratio(grads, sb):
    """Worst |g - ref| / bound over the three gradients of one sequence; NaN / Inf anywhere counts as infinite."""
    if not all(np.isfinite(np.asarray(g, np.float64)).all() for g in grads):
        return float("inf")
    return max(bb.ratios(grads, sb.ref, sb.bound))
