"""The key split of the paged prefill (include/fa_mi355.h, "Key split in the paged prefill"), test side only, pure numpy: the split rule,
a brute-force "which split owns key j of block qb", an fp32 model of the partial state and of the combine (with and without a sink,
one planted mistake at a time) and the bars. Shared by tests/test_ksplit_cases.py (CPU) and tests/test_gpu_ksplit.py (GPU).

The rule: a 128-row block walks tiles [tb, nT) of 64 keys, the tiles of the keys its rows see together (window.key_range), n = nT - tb.
Split s of S takes tiles tb + floor(s n / S) .. tb + floor((s + 1) n / S) - 1. Per owned row a split leaves o_s = acc / l (fp32) and
lse2_s = m + log2 l (log2 units; -inf without a visible key), and the combine forms, over s in order,
    M = max lse2_s,  w_s = 2^(lse2_s - M),  W = sum w_s,  O = (sum w_s o_s) / W,  LSE = (M + log2 W) ln 2
skipping every split with lse2_s = -inf; M = -inf: O = 0, LSE = -inf (with a sink: sinks[h]). A sink is folded once, behind the reduction.

The bars (derived, never fitted): the un-split route's (util.o_tol / lse_tol; with sinks sink.bars on them) plus, on O, the header's term for
merged key splits, 2 (S + 3) 2^-24 sum_j P_ij |v_jd| (and 6 2^-24 |LSE| sum_j P_ij |v_jd| for the resolution of lse2_s, merge_o_term()),
and on LSE the fp32 roundings of the merge, merge_lse_term() below."""
import numpy as np

import sink as sk
import window as wn

TILE, BLOCK = wn.TILE, wn.BLOCK
SPLITS = (2, 3, 5, 16)
MAX_SPLITS, MIN_TILES = 64, 4  # FA_VARLEN_PAGED_MAX_SPLITS, FA_KSPLIT_MIN_TILES
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
SABOTAGES = ("empty_split_weighs_1", "weights_not_applied", "reference_of_split_0", "tile_in_two_splits", "last_tile_skipped",
             "sink_in_every_split", "log_base")


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
def block_tiles(Lq, Lk, wl, wr, qb):
    """(tb, nT) of block qb, or None when its rows see no key (brute force over the visibility rule)."""
    kr = wn.key_range(Lq, Lk, wl, wr, qb * BLOCK, min(qb * BLOCK + BLOCK, Lq) - 1) if Lk and qb * BLOCK < Lq else None
    return None if kr is None else (kr[0] // TILE, (kr[1] + TILE - 1) // TILE)


def split_tiles(tb, nT, s, S):
    n = nT - tb
    return tb + (s * n) // S, tb + ((s + 1) * n) // S


def owner_of_key(Lq, Lk, wl, wr, qb, S):
    """int [Lk]: for every key the splits whose tile range holds it, as a count and the last such split: (count [Lk], split [Lk]); keys
    outside the block's tiles have count 0. Brute force: every split's range is scanned."""
    count, split = np.zeros(Lk, int), np.full(Lk, -1)
    bt = block_tiles(Lq, Lk, wl, wr, qb)
    if bt is None:
        return count, split
    for s in range(S):
        t0, t1 = split_tiles(*bt, s, S)
        for j in range(t0 * TILE, min(t1 * TILE, Lk)):
            count[j] += 1
            split[j] = s
    return count, split


def num_splits(B, Hq, max_q, D, P, max_pages):
    """fa_fwd_varlen_paged_num_splits, restated."""
    blocks = B * Hq * ((max_q + BLOCK - 1) // BLOCK)
    slots = 512  # FA_KSPLIT_SLOTS: 256 CUs x 2 at both head dims (768 at head_dim 64 was measured slower)
    S = (slots + blocks - 1) // blocks
    S = min(S, max(1, ((P * max_pages + TILE - 1) // TILE) // MIN_TILES))
    return max(1, min(S, MAX_SPLITS))


def workspace_bytes(S, Hq, total_q, D):
    return 0 if S < 2 else (S * Hq * total_q * (D + 1) * 4 + 15) // 16 * 16


# ---- the bars --------------------------------------------------------------------------------------------------------------------------
def merge_o_term(S, absum, lse=None):
    """The header's term for S merged key splits on O: 2 (S + 3) 2^-24 sum_j P_ij |v_jd| (absum [.., D]). With lse [..] (natural-log
    units), plus what the ONE fp32 number lse2_s costs: its sum m + log2 l and its logarithm round at the magnitude of lse2_s, 1.5 ulp =
    1.5 2^-24 |L2| each, so a weight 2^(lse2_s - M) is off by a factor within 3 2^-24 |L2| ln 2 = 3 2^-24 |LSE|, and numerator and
    denominator together move O by at most 6 2^-24 |LSE| sum_j P_ij |v_jd|. Invisible at |LSE| of a few units; it is what bounds a
    cancelling element when the scores reach hundreds."""
    extra = 0.0 if lse is None else 6.0 * np.abs(np.where(np.isfinite(lse), lse, 0.0))[..., None]
    return (2.0 * (S + 3) + extra) * 2.0 ** -24 * absum


def merge_lse_term(S, lse):
    """fp32 roundings between the splits' exact (m, l) and LSE, in natural-log units, with u = 2^-24:
      - lse2_s = fl(m + fl(log2 l)): the hardware logarithm (1 ulp) and the sum, <= 3 u |lse2_s|; a split d = M - lse2_s below the
        maximum carries weight 2^-d, and 2^-d (|M| + d) <= |M| + 0.54: in all 3 u (|L2| + 1) with |L2| <= |LSE| / ln 2 + log2 S;
      - d_s = fl(lse2_s - M) moves w_s by a factor within u d_s ln 2, and 2^-d d <= 0.54: u per split against W >= 1, <= S u in all;
      - the exponentials (1 ulp each) and W's S - 1 additions: (S + 1) u relative on W, i.e. (S + 1) u / ln 2 on log2 W;
      - log2 W (1 ulp of a value <= log2 S <= 6), the sum M + log2 W and the product by ln 2: 2 u 6 + 2 u |L2|.
    Times ln 2 and rounded up: 2^-24 (5 |LSE| + 2 S + 5 log2 S + 16) <= 2^-22 (2 |LSE| + S + 6)."""
    return 2.0 ** -22 * (2.0 * np.abs(np.where(np.isfinite(lse), lse, 0.0)) + S + 6.0)


def absum_reference(q, k, v, wl, wr, scale=None):
    """fp64 sum_j P_ij |v_jd| [Hq, Lq, D] of one sequence (0 on dead rows): the operator on |V|."""
    return wn.reference(q, k, np.abs(v), wl, wr, scale)[0]


def bars(S, lse_tol, o_tol, o64, l64, absum, sinks=None):
    """(o_bar [Hq, Lq, D], lse_bar [Hq, Lq], O reference, LSE reference) of one sequence from the un-split route's scalar tolerances, the
    sink-free fp64 references and sum_j P |v|. With sinks: sink.bars on top (the references become the folded ones; the merge term on O
    shrinks with the fold's factor <= 1 and is kept as it is)."""
    tl = lse_tol + merge_lse_term(S, l64)
    if sinks is None:
        return o_tol + merge_o_term(S, absum, l64), tl, o64, l64
    o2, l2 = sk.fold(o64, l64, sinks)
    lb = tl + sk.fold_term(l64, l2, sinks) + merge_lse_term(S, l2)
    return o_tol + merge_o_term(S, absum, l64) + np.abs(o2) * lb[..., None], lb, o2, l2


# ---- an fp32 model of the two kernels ----------------------------------------------------------------------------------------------------
def partial_state(q, k, v, wl, wr, S, scale=None, bug=None):
    """What the S partial launches leave for one sequence, from an exact (fp64) tile loop rounded to fp32 once:
    o_s [S, Hq, Lq, D] and lse2_s [S, Hq, Lq] (-inf: no visible key in the split). q [Hq, Lq, D], k / v [Hkv, Lk, D]."""
    Hq, Lq, D = q.shape
    Hkv, Lk = k.shape[0], k.shape[1]
    c2 = (D ** -0.5 if scale is None else scale) * LOG2E
    o_s, lse2 = np.zeros((S, Hq, Lq, D), np.float32), np.full((S, Hq, Lq), -np.inf, np.float32)
    if Lq == 0 or Lk == 0:
        return o_s, lse2
    vis = wn.visible(Lq, Lk, wl, wr)
    ke, ve = (np.repeat(x.astype(np.float64), Hq // Hkv, axis=0) for x in (k, v))
    s_all = np.where(vis[None], (q.astype(np.float64) @ ke.swapaxes(-1, -2)) * c2, -np.inf)
    for qb in range((Lq + BLOCK - 1) // BLOCK):
        bt = block_tiles(Lq, Lk, wl, wr, qb)
        if bt is None:
            continue
        rows = slice(qb * BLOCK, min(qb * BLOCK + BLOCK, Lq))
        for s in range(S):
            t0, t1 = split_tiles(*bt, s, S)
            if bug == "tile_in_two_splits" and s + 1 < S:
                t1 = min(t1 + 1, bt[1])
            if bug == "last_tile_skipped" and s == S - 1:
                t1 -= 1
            if t0 >= t1:
                continue
            keys = slice(t0 * TILE, min(t1 * TILE, Lk))
            sc = s_all[:, rows, keys]
            m = sc.max(-1)
            some = np.isfinite(m)
            p = np.where(some[..., None], np.exp2(sc - np.where(some, m, 0.0)[..., None]), 0.0)
            l = p.sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                o_s[s, :, rows] = np.where(some[..., None], (p @ ve[:, keys]) / l[..., None], 0.0)
                lse2[s, :, rows] = np.where(some, m + np.log2(l), -np.inf)
    return o_s, lse2


def combine_model(o_s, lse2, sinks=None, bug=None):
    """csrc/fa_mfma_kernel.hip, ksplit_combine_kernel, in fp32 and in its order. o_s [S, Hq, Lq, D], lse2 [S, Hq, Lq]; sinks [Hq] or None.
    Returns fp32 (O [Hq, Lq, D], LSE [Hq, Lq])."""
    o_s, lse2 = np.asarray(o_s, np.float32), np.asarray(lse2, np.float32)
    S = o_s.shape[0]
    empty = np.isneginf(lse2)
    M = lse2[0] if bug == "reference_of_split_0" else lse2.max(0)
    W = np.zeros(M.shape, np.float32)
    acc = np.zeros(o_s.shape[1:], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(S):
            w = sk.exp2_32(lse2[s] - M)
            if bug == "weights_not_applied":
                w = np.ones_like(w)
            take = ~empty[s] | (bug == "empty_split_weighs_1")
            w = np.where(empty[s], np.float32(1.0), w)
            W = np.where(take, (W + w).astype(np.float32), W)
            acc = np.where(take[..., None], (acc + (w[..., None] * np.where(empty[s][..., None], np.float32(0), o_s[s])).astype(np.float32))
                           .astype(np.float32), acc)
        dead = empty.all(0)
        unit = np.float32(1.0) if bug == "log_base" else sk.LN2_32
        if sinks is None:
            inv = np.where(dead, np.float32(0), np.float32(1.0) / np.where(dead, np.float32(1), W)).astype(np.float32)
            lse = np.where(dead, -np.inf, (M + np.log2(np.where(dead, np.float32(1), W)).astype(np.float32)).astype(np.float32) * unit)
        else:
            s2 = (np.asarray(sinks, np.float32) * sk.LOG2E32).astype(np.float32)[:, None]
            Mm = np.where(dead, s2, np.maximum(M, s2))
            ow = np.where(dead, np.float32(0), sk.exp2_32(np.where(dead, np.float32(0), M) - Mm))
            n_sink = np.float32(S if bug == "sink_in_every_split" else 1)
            Wt = (np.where(dead, np.float32(0), W * ow) + n_sink * sk.exp2_32(s2 - Mm)).astype(np.float32)
            inv = (ow * (np.float32(1.0) / Wt)).astype(np.float32)
            lse = np.where(dead, np.asarray(sinks, np.float32)[:, None], (Mm + np.log2(Wt).astype(np.float32)).astype(np.float32) * unit)
        o = np.where(dead[..., None], np.float32(0), (acc * inv[..., None]).astype(np.float32))
    return o.astype(np.float32), lse.astype(np.float32)


def forward_model(q, k, v, wl, wr, S, sinks=None, scale=None, bug=None):
    """fp32 (O, LSE) of one sequence as the pair of kernels forms them from an exact tile loop; bug: one of SABOTAGES."""
    o_s, lse2 = partial_state(q, k, v, wl, wr, S, scale, bug)
    return combine_model(o_s, lse2, sinks, bug)


# ---- ramped inputs with teeth ------------------------------------------------------------------------------------------------------------
# On U(-1, 1) inputs the splits' LSEs nearly agree, and a merge without weights would pass. The ramped half of the parity cases is built
# here on exact_forward.build_window's plan (key j carries -1 on coordinate j mod (D - 6), queries are 0 / 1 masks there and hold 1 on the
# six last coordinates, V on its grid, scale = fp32(ln 2) 2^k: every score an exact integer in log2 units) with a ramp that FALLS BY
# RAMP_STEP = 16 PER KEY: s_ij = 16 (Lk - 1 - j) - (0 | 1). A row's visible keys are contiguous, so each of its non-empty splits has its
# maximum at its first visible key and a sum below 1 + 2^-14: two non-empty splits lie at least 16 - 1 - 0.01 units apart wherever the
# split's edge falls, under every window, bounded on the left or not. (build_window's own slopes step 1 or 3 per key: a first split of
# one key then sits one to three units above the next, which is why they cannot serve.) Multiples of 16 up to 16 * 256 are exact in bf16
# and in f16, and six coordinates of at most 16 * 167 carry 16 * 999: ONE set of values serves both types. The window does not enter the
# values: a case is a sequence, viewed under a window.
RAMP_STEP = 16
RAMP_SPAN = 8.0   # what the issue asks of the per-split LSEs of every row with two or more non-empty splits
RAMP_LEFT_OUT = ()  # (window, sequence, S) that cannot meet it, as window.LEFT_OUT lists its own: none -- at most a quarter may be
_RAMPED = {}


def ramp_case(seq, D, heads, dtype, window=None):
    """The ramped case of one window.SEQS sequence (an exact_forward case, family "B": ef.reference_head / ef.bars / ef.ratios take it)."""
    from types import SimpleNamespace

    from exact_forward import VBITS, _spread, exact_scale

    key = (tuple(seq), D, tuple(heads))
    if key not in _RAMPED:
        (Lq, Lk), (Hq, Hkv), kexp, vb, Dc = seq, heads, wn.KEXP[D], VBITS["bf16"], D - 6
        assert VBITS["f16"] == vb
        rng = np.random.default_rng(2216 + 7 * wn.SEQS.index(tuple(seq)) + D + heads[0])
        k = np.zeros((1, Hkv, Lk, D), np.float32)
        j = np.arange(Lk)
        k[:, :, j, j % Dc] = -1.0
        for coord, part in zip(range(Dc, D), _spread(Lk - 1 - j, 6, 256) if Lk else ()):
            k[..., coord] = RAMP_STEP * part
        q = np.zeros((1, Hq, Lq, D), np.float32)
        q[..., :Dc] = rng.integers(0, 2, (1, Hq, Lq, Dc))
        q[..., Dc:] = 1.0
        q *= np.float32(2.0 ** -kexp)
        v = (rng.integers(-(1 << vb), (1 << vb) + 1, (1, Hkv, Lk, D)) / float(1 << vb)).astype(np.float32)
        _RAMPED[key] = dict(family="B", q=q, k=k, v=v, causal=False, kexp=kexp, scale=exact_scale(kexp), span=0, vbits=vb, lens=None, ramp="fall",
                            slope="step16", every=1)
    return SimpleNamespace(dtype=dtype, window=None if window is None else tuple(window), **_RAMPED[key])


def split_lse_span(q, k, wl, wr, S, scale=None):
    """Per row with two or more non-empty splits, max - min of the splits' exact lse2_s (log2 units); NaN elsewhere. [Hq, Lq]."""
    _, lse2 = partial_state(q, k, np.zeros_like(k), wl, wr, S, scale)
    lse2 = lse2.astype(np.float64)
    live = np.isfinite(lse2)
    hi = np.where(live, lse2, -np.inf).max(0)
    lo = np.where(live, lse2, np.inf).min(0)
    with np.errstate(invalid="ignore"):
        return np.where(live.sum(0) >= 2, hi - lo, np.nan)
