"""Attention sinks (include/fa_mi355.h, "Attention sinks"), test side only, pure numpy: the fp64 references of the *_sink entry points, the
bars the header derives, fp32 models of the two epilogues and of the dsink reduction with one planted mistake at a time, and the
per-sequence backward bound under a sink. Shared by tests/test_sink_cases.py (CPU) and tests/test_gpu_sink*.py (GPU).

A sink is one logit per QUERY head (natural-log units, no softmax scale) in every softmax denominator; it carries no value:
    lse' = ln(exp(lse) + exp(sink)),   O' = O exp(lse - lse'),   dead rows: O' = 0, lse' = sink
with (O, lse) = window.reference, the operator without the sink. The gradient of a loss through O':
    dsink_h = -sum_i p_i delta_i,   p_i = exp(sink_h - lse'_i),   delta_i = sum_d dO_id O'_id.

The bars (derived in the header, never fitted): w = exp(lse - lse') <= 1 is the weight of the un-sinked LSE error in lse', and the fold
costs a few fp32 roundings, the conversion of the sink felt through its share 1 - w:
    lse_bar = lse_tol + 2^-22 ((1 - w) |sink| + |lse'| + 4)          o_bar_d = o_tol + |O'_d| lse_bar
    dsink, given lse and delta: 2^-24 sum_i |t_i| (|x_i| + 3 + c),  x_i = sink - lse_i, t_i = exp(x_i) delta_i,
                                c = sum_b ceil(Lq_b / 1024) + 10  (additions on the longest path of the kernel's fixed order)
    dsink, end to end: + sum_i p_i exp(lse_err_i) (|delta_i| lse_err_i + sum_d |dO_id| o_err_id)."""
import numpy as np

import backward_bound as bb
import window as wn
import window_backward as wb

LOG2E32, LN2_32 = np.float32(1.4426950408889634), np.float32(0.6931471805599453)
THREADS = 1024  # csrc/fa_sink_kernels.hip, DSINK_THREADS
WINDOWS = ((-1, 0), (-1, -1), (15, 0), (63, 0), (64, 64), (127, 5), (200, 0))
BUGS_FWD = ("scaled", "log_base", "neighbour_head", "dead_neg_inf", "no_max")
BUGS_DSINK = ("sign", "unowned", "other_block")


def sinks_for(Hq):
    """Per-head sinks that differ from head to head and straddle U(-1, 1) scores: one at -1e4 (adds exactly nothing), some within the
    scores' range, one well above every score."""
    base = np.array([-1e4, -0.5, 0.7, 8.0, 2.0, -3.0, 0.1, 1.5] * 2, np.float32)
    return base[:Hq].copy()


def fold(o, lse, sinks):
    """fp64 (O', lse') of one sequence from the un-sinked (O [Hq, Lq, D], lse [Hq, Lq]; -inf on dead rows) and sinks [Hq]."""
    s = np.asarray(sinks, np.float64)[:, None]
    lse2 = np.logaddexp(lse, s)
    return o * np.exp(lse - lse2)[..., None], lse2


def reference(q, k, v, wl, wr, sinks, scale=None):
    return fold(*wn.reference(q, k, v, wl, wr, scale), sinks)


def fold_term(lse, lse2, sinks):
    """The fp32 cost of converting and folding the sink, [Hq, Lq]."""
    s = np.abs(np.asarray(sinks, np.float64))[:, None]
    with np.errstate(invalid="ignore"):
        w = np.where(np.isneginf(lse), 0.0, np.exp(lse - lse2))
    return 2.0 ** -22 * ((1.0 - w) * s + np.abs(lse2) + 4.0)


def bars(lse_tol, o_tol, o2, lse, lse2, sinks):
    """(o_bar [Hq, Lq, D], lse_bar [Hq, Lq]) from the un-sinked route's scalar tolerances and the fp64 references."""
    lb = lse_tol + fold_term(lse, lse2, sinks)
    return o_tol + np.abs(o2) * lb[..., None], lb


# ---- fp32 models of the epilogues ----------------------------------------------------------------------------------------------------
def exp2_32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(np.asarray(x, np.float32)).astype(np.float32)


def epilogue_model(m2, l, acc, sink, scale=None, bug=None):
    """csrc/fa_mfma_kernel.hip, sink mode, rows with a visible key: m2 [n] the rows' reference (log2 units), l [n] their sums, acc [n, D]
    the unnormalised O, all fp32; sink a scalar. Returns fp32 (O [n, D], LSE [n])."""
    m2, l, acc = (np.asarray(x, np.float32) for x in (m2, l, acc))
    s = np.float32(sink) * (np.float32(scale) if bug == "scaled" else np.float32(1.0))
    s2 = s if bug == "log_base" else np.float32(s * LOG2E32)
    mm = m2 if bug == "no_max" else np.maximum(m2, s2)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ow = exp2_32(m2 - mm)
        lt = (l * ow + exp2_32(s2 - mm)).astype(np.float32)
        inv = (ow * (np.float32(1.0) / lt)).astype(np.float32)
        return (acc * inv[:, None]).astype(np.float32), (mm * LN2_32 + np.log(lt).astype(np.float32)).astype(np.float32)


def combine_model(ms, ls, accs, sink, scale=None, bug=None):
    """csrc/fa_decode_kernel.hip, decode_combine_sink_kernel: the S splits' (m [S, n], lsum [S, n], acc [S, n, D]) of n rows -- a split
    that saw no key has m = -inf, l = 0 -- reduced by their maxima, then the sink folded in. A row no split saw a key for is dead."""
    ms, ls, accs = (np.asarray(x, np.float32) for x in (ms, ls, accs))
    M = ms.max(0)
    with np.errstate(invalid="ignore"):
        f = np.where(np.isneginf(ms), np.float32(0), exp2_32(ms - M[None]))
    lsum = (ls * f).sum(0, dtype=np.float32)
    acc = (accs * f[..., None]).sum(0, dtype=np.float32)
    dead = ~(lsum > 0)
    o, lse = epilogue_model(np.where(dead, np.float32(0), M), np.where(dead, np.float32(1), lsum), acc, sink, scale, bug)
    o[dead] = 0.0
    lse[dead] = -np.inf if bug == "dead_neg_inf" else np.float32(sink)
    return o, lse


def exact_state(q, k, v, wl, wr, scale=None, splits=1):
    """What the tile loops hand the epilogue, exact: per head and LIVE row the reference m2 = max score (log2 units), l = sum 2^(s2 - m2)
    and acc = sum 2^(s2 - m2) v, rounded to fp32 once; with splits > 1 the keys are dealt to that many contiguous shares ([S, Hq, n...],
    a share without a visible key: m = -inf, l = 0). Returns (live [Lq] bool, m2, l, acc)."""
    Hq, Lq, D = q.shape
    Hkv, Lk = k.shape[0], k.shape[1]
    sc = (D ** -0.5 if scale is None else scale) * 1.4426950408889634
    vis = wn.visible(Lq, Lk, wl, wr) if Lk else np.zeros((Lq, 0), bool)
    live = vis.any(1)
    ke, ve = (np.repeat(x.astype(np.float64), Hq // Hkv, axis=0) for x in (k, v))
    s = np.where(vis[None, live], (q.astype(np.float64)[:, live] @ ke.swapaxes(-1, -2)) * sc, -np.inf)
    edges = np.linspace(0, Lk, splits + 1).astype(int)
    ms, ls, accs = [], [], []
    for a, b in zip(edges[:-1], edges[1:]):
        part = s[..., a:b]
        m = part.max(-1) if b > a else np.full(s.shape[:2], -np.inf)
        with np.errstate(invalid="ignore"):
            p = np.where(np.isneginf(m)[..., None], 0.0, np.exp2(part - np.where(np.isneginf(m), 0.0, m)[..., None]))
        ms.append(m)
        ls.append(p.sum(-1))
        accs.append(p @ ve[:, a:b])
    out = tuple(np.asarray(x, np.float32) for x in (ms, ls, accs))
    return (live,) + (tuple(x[0] for x in out) if splits == 1 else out)


def forward_model(q, k, v, wl, wr, sinks, scale=None, bug=None, splits=1):
    """fp32 (O [Hq, Lq, D], LSE [Hq, Lq]) of one sequence as the kernels' epilogues form them from an exact tile loop: the 128-row kernel
    (splits = 1) or the decode's combine. bug: one of BUGS_FWD."""
    Hq, Lq, D = q.shape
    G = Hq // k.shape[0]
    sc = D ** -0.5 if scale is None else scale
    live, m2, l, acc = exact_state(q, k, v, wl, wr, scale, splits)
    o, lse = np.zeros((Hq, Lq, D), np.float32), np.zeros((Hq, Lq), np.float32)
    for h in range(Hq):
        sink = sinks[h // G] if bug == "neighbour_head" else sinks[h]  # (the key head's index where the query head's belongs)
        if splits == 1:
            oh, lh = epilogue_model(m2[h], l[h], acc[h], sink, sc, bug)
        else:
            oh, lh = combine_model(m2[:, h], l[:, h], acc[:, h], sink, sc, bug)
        o[h, live], lse[h, live] = oh, lh
        lse[h, ~live] = -np.inf if bug == "dead_neg_inf" else np.float32(sink)
    return o, lse


# ---- the dsink reduction ---------------------------------------------------------------------------------------------------------------
def owned_rows(cu_q, total_q, max_q):
    """The token indices the kernel reads, sequence by sequence: entries clamped to [0, total_q], a non-increasing pair is length 0, a
    length stops at max_q."""
    out = []
    for b in range(len(cu_q) - 1):
        s, e = min(max(int(cu_q[b]), 0), total_q), min(max(int(cu_q[b + 1]), 0), total_q)
        out.append(np.arange(s, s + min(max(e - s, 0), max_q)))
    return out


def dsink_exact(sinks, lse, delta, cu_q, max_q):
    """fp64 dsinks [Hq] of the formula on the lse / delta [Hq, total_q] the kernel is given."""
    rows = np.concatenate(owned_rows(cu_q, lse.shape[1], max_q) + [np.array([], int)]).astype(int)
    x = np.asarray(sinks, np.float64)[:, None] - lse[:, rows].astype(np.float64)
    return -(np.exp(x) * delta[:, rows].astype(np.float64)).sum(1)


def dsink_bound(sinks, lse, delta, cu_q, max_q):
    """The header's fp32 bound of the exp and the tree sum, [Hq]."""
    per_seq = owned_rows(cu_q, lse.shape[1], max_q)
    rows = np.concatenate(per_seq + [np.array([], int)]).astype(int)
    c = sum(-(-len(r) // THREADS) for r in per_seq) + 10
    x = np.asarray(sinks, np.float64)[:, None] - lse[:, rows].astype(np.float64)
    t = np.abs(np.exp(x) * delta[:, rows].astype(np.float64))
    return 2.0 ** -24 * (t * (np.abs(x) + 3 + c)).sum(1)


def dsink_model(sinks, lse, delta, cu_q, max_q, bug=None):
    """csrc/fa_sink_kernels.hip in fp32, in its order: thread t adds rows t, t + 1024, ... of every sequence, then a binary tree."""
    Hq, total_q = lse.shape
    lse, delta = np.asarray(lse, np.float32), np.asarray(delta, np.float32)
    per_seq = [np.arange(total_q)] if bug == "unowned" else owned_rows(cu_q, total_q, max_q)
    out = np.zeros(Hq, np.float32)
    for h in range(Hq):
        part = np.zeros(THREADS, np.float32)
        for rows in per_seq:
            for a in range(0, len(rows), THREADS):
                r = rows[a:a + THREADS]
                lr = lse[h, np.roll(rows, 128)[a:a + THREADS]] if bug == "other_block" else lse[h, r]
                with np.errstate(over="ignore", invalid="ignore"):
                    term = (np.exp((np.float32(sinks[h]) - lr).astype(np.float32)).astype(np.float32) * delta[h, r]).astype(np.float32)
                part[:len(r)] = (part[:len(r)] + term).astype(np.float32)
        w = THREADS // 2
        while w >= 1:
            part[:w] = (part[:w] + part[w:2 * w]).astype(np.float32)
            w //= 2
        out[h] = part[0] if bug == "sign" else -part[0]
    return out


# ---- the backward under a sink -----------------------------------------------------------------------------------------------------------
def head_exact(q, k, v, do, mask, scale, sink):
    """window_backward.head_exact with the sink in the denominator: p's rows add up to 1 - p_sink; dsink = -sum_i p_sink_i delta_i."""
    q, k, v, do = (np.asarray(x, np.float64) for x in (q, k, v, do))
    s = np.where(mask, (q @ k.T) * scale, -np.inf)
    lse = np.logaddexp(np.log(np.exp(s - s.max(-1, keepdims=True)).sum(-1)) + s.max(-1), sink)
    p = np.exp(s - lse[:, None])
    o = p @ v
    dp = do @ v.T
    delta = (do * o).sum(-1, keepdims=True)
    ds = p * (dp - delta)
    ps = np.exp(sink - lse)
    return dict(p=p, ds=ds, dp=dp, delta=delta, o=o, lse=lse, mask=mask, dq=scale * (ds @ k), dk=scale * (ds.T @ q), dv=p.T @ do, ps=ps,
                dsink=-(ps * delta[:, 0]).sum())


class SeqBounds:
    """window_backward.SeqBounds(chain=True) for one sequence under (wl, wr) and sinks [Hq]: ref / bound of (dQ, dK, dV) through
    backward_bound.head_bounds on the sink-including P and dS, with window_backward.forward_errors plus the fold's terms as the forward's
    lse_err / o_err; o, lse = the exact forward (dead rows: 0 and the sink); dsink_ref [Hq] and the chain bound dsink_chain [Hq] =
    sum_i p_i exp(lse_err_i) (|delta_i| lse_err_i + sum_d |dO_id| o_err_id) of this sequence's rows."""

    def __init__(self, q, k, v, do, wl, wr, sinks, scale, dtype):
        self.scale = bb.default_scale(q.shape[-1]) if scale is None else float(scale)
        Hq, Lq, D = q.shape
        Hkv, Lk = k.shape[0], k.shape[1]
        G = Hq // Hkv
        self.n0 = n0 = wb.first_live_row(Lq, Lk, wl, wr)
        self.vis = wn.visible(Lq, Lk, wl, wr)
        self.unseen = ~self.vis.any(0) if Lq else np.ones(Lk, bool)
        self.o = np.zeros(q.shape)
        self.lse = np.repeat(np.asarray(sinks, np.float64)[:, None], Lq, axis=1)
        self.ref = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        self.bound = (np.zeros(q.shape), np.zeros(k.shape), np.zeros(k.shape))
        self.dsink_ref, self.dsink_chain = np.zeros(Hq), np.zeros(Hq)
        if n0 >= Lq:
            return
        mask = self.vis[n0:]
        assert mask.any(1).all() and not self.vis[:n0].any()
        for h in range(Hq):
            hk = h // G
            R = head_exact(q[h, n0:], k[hk], v[hk], do[h, n0:], mask, self.scale, float(sinks[h]))
            le, oe = wb.forward_errors(q[h, n0:], k[hk], v[hk], mask, self.scale, dtype, R)
            # (the sink's share 1 - w of the row's sum is ps)
            le = le + 2.0 ** -22 * (R["ps"] * abs(float(sinks[h])) + np.abs(R["lse"]) + 4.0)
            oe = oe + np.abs(R["o"]) * le[:, None]
            B = bb.head_bounds(q[h, n0:], k[hk], v[hk], do[h, n0:], self.scale, dtype, R, le, oe)
            self.o[h, n0:], self.lse[h, n0:] = R["o"], R["lse"]
            self.ref[0][h, n0:] = R["dq"]
            self.ref[1][hk] += R["dk"]
            self.ref[2][hk] += R["dv"]
            self.bound[0][h, n0:] = B[0]
            self.bound[1][hk] += B[1]
            self.bound[2][hk] += B[2]
            self.dsink_ref[h] = R["dsink"]
            ado = np.abs(np.asarray(do[h, n0:], np.float64))
            self.dsink_chain[h] = (R["ps"] * np.exp(le) * (np.abs(R["delta"][:, 0]) * le + (ado * oe).sum(-1))).sum()
