"""Forward inputs on which every intermediate the kernels round is exactly representable (pure numpy, shared by
tests/test_exact_forward_cases.py on the CPU and tests/test_gpu_exact_forward.py on the GPU).

The construction
  scale   scale = fp32(ln 2) * 2^k: c2 = fp32(scale) * fp32(log2 e) is exactly 2^k in fp32 (c2_of, asserted by the CPU tests), so the
          pre-scaled operand round(c2 * q) is 2^k q bit for bit and the kernels that scale the scores in fp32 multiply by a power of two.
  Q, K    2^k q_i . k_j is an INTEGER for every pair. Key j carries -c_j (c_j in 1 .. span; key 0 is the zero vector) on coordinate
          j mod Dc; query i is a random 0/1 mask (times 2^-k) over those Dc coordinates: the score is -c_j or 0. Every probability,
          against the true row maximum or any reference an integer away from it, is a power of two: exact in bf16, in f16 (down to
          2^-24) and in e4m3 (2^-9 .. 2^8); every rescale factor and split-merge weight is a power of two; every row sum is a sum of
          powers of two, exact in fp32.
  V       multiples of 2^-vbits in [-1, 1] (6 bits for f16 / bf16, 3 for e4m3: representable in each).
  family A ("maximum first"): key 0 scores 0 and nothing scores higher, every row sees key 0: the reference is final after the first
          tile. Every term of the PV sum is a multiple of 2^-(span + vbits); where sum_j p_ij |v_jd| < 2^(24 - span - vbits) every
          partial sum in ANY order is exact in fp32 (criterion(): it PROVES a row). Kernels that give each key split a maximum of its
          own multiply a split's sums by 2^(m_s - M) >= 2^-span in the merge: the criterion then takes 2 * span.
  family B ("rising maximum"): Dc = D - 6; three more coordinates carry a ramp every row sees and three a ramp only one row in 32
          sees (a single row of a wave), both rising along the keys in integer steps -- by 1 for a stretch (below every deferral
          threshold), then by 9 .. 12 (past it) at a tile start, inside a tile, and two keys before the end (the ragged last tile);
          never by more than 15 inside one tile, which keeps every probability above f16's 2^-24 (ramps()).
          P stays exact; fp32 partial sums may round, so the bar adds the textbook n * 2^-24 * sum_j p_ij |v_jd|.

The bars, per element (no fitted factor; units of 2^-24 = one fp32 rounding, a hardware rcp / exp2 / log2 counts 2 = one ulp):
  O    u_out |O|                                   rounding of O to its type (2^-11 f16, 2^-8 bf16; f16 subnormal: 2^-25 absolute)
     + EPI_O * 2^-24 |O|                           the epilogue: reciprocal or division of l (<= 2), its product with the accumulator
                                                   (1), one ulp on l in case the hardware exp2 of an integer is not the exact power of
                                                   two (2), the cross-lane addition of the row-sum halves (1): 6 covers every kernel
                                                   (flash_attention_metal_amd/csrc/fa_mfma_kernel.hip:800-834, fa_mfma16_kernel.hip:648-668, fa_fp8_kernel.hip:325-343,
                                                   fa_fwd_splitkv_kernel.hip:266-290, fa_decode_kernel.hip:508-511)
     + merge: 2 (S + 3) * 2^-24 sum_j p |v|        kernels that merge S key splits: a weight exp2(m_s - M) within one ulp (2), its
                                                   product (1) and S additions, once for the numerator and once for l
                                                   (fa_mfma_kernel.hip:784-792, fa_fwd_splitkv_kernel.hip:253-278, fa_decode_kernel.hip:468-507)
     + family B / unproven rows: n * 2^-24 sum_j p |v|,  n = visible keys + tiles  (one addition per key, one rescale per tile)
  LSE  EPI_L * 2^-23 (|m'| ln 2 + |ln l'| + |LSE|) + the relative error of l from the terms above, where m' / l' are the reference and
       the row sum as the kernel holds them (m + shift, l / 2^shift: shift = BIAS 7 / 3 of fa_mfma16_kernel.hip:230-234, -SHIFT = -3 of
       fa_fp8_kernel.hip:13-15, else 0) and EPI_L = 4: log, product with ln 2 or with scale, the sum, fp32(ln 2) itself
       (fa_mfma_kernel.hip:819, fa_mfma16_kernel.hip:658, fa_fp8_kernel.hip:331, fa_fwd_splitkv_kernel.hip:267, fa_decode_kernel.hip:512).
"""
from types import SimpleNamespace

import numpy as np

LN2_F32 = np.float32(0.6931471805599453)
LOG2E_F32 = np.float32(1.4426950408889634)
LN2 = 0.6931471805599453
U_OUT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "fp8": 2.0 ** -8}  # e4m3 inputs: O is bf16
VBITS = {"f16": 6, "bf16": 6, "fp8": 3}
EPI_O, EPI_L = 6, 4
TILE = 64
RESERVED = 6  # family B: coordinates D-1, D-3, D-4 carry the ramp all rows see, D-2, D-5, D-6 the ramp of the solo rows
ALL_COORDS, SOLO_COORDS = (-1, -3, -4), (-2, -5, -6)
SOLO_EVERY, SOLO_AT = 32, 5  # rows i with i % 32 == 5: one row of every 32-row wave


def exact_scale(kexp):
    """fp32(ln 2) * 2^k as a Python float (exactly an fp32 value)."""
    return float(LN2_F32 * np.float32(2.0 ** kexp))


def c2_of(scale):
    """The kernels' score factor: fp32(scale) * fp32(log2 e), one fp32 product."""
    return np.float32(np.float32(scale) * LOG2E_F32)


def reference_shift(variant, dtype):
    """How far the kernel's reference sits from the row maximum it was set from (log2 units), per the kernel headers."""
    if variant == "mfma16":
        return 3.0 if dtype == "f16" else 7.0  # fa_mfma16_kernel.hip:230-234 (BIAS)
    if variant == "mfma_fp8pv":
        return -3.0  # fa_fp8_kernel.hip:13-15 (SHIFT)
    return 0.0


def span_for(dtype, split, nk):
    """Largest score depth of family A that keeps the criterion provable at this length (the criterion is still checked per row).
    Single-maximum kernels: 2^(24 - span - vbits) must exceed sum p |v| ~ 0.35 Nk -- 7 up to 4096 keys, 4 beyond (bf16 / f16, 6-bit V).
    e4m3 probabilities (fa_fp8_kernel.hip:13-15: P' = 8 P, exact down to 2^-9) allow 12; 4 keeps every P' a NORMAL e4m3 (>= 2^-6 with
    the factor 8 ... 2^-1). Kernels with a maximum per key split need 2 * span: 3 up to 8192 keys (2^12 > 0.35 Nk), 2 beyond
    (2^14 at 16384 keys)."""
    if split:
        return 3 if nk <= 8192 else 2
    if dtype == "fp8":
        return 4
    return 7 if nk <= 4096 else 4


TILE_RISE = 15     # family B: a row's scores rise by at most this much inside one 64-key tile (both ramps together)
TILE_RISE_E4M3 = 6  # ... for the kernel with e4m3 probabilities (variant mfma_fp8pv)


def ramps(nk, rise=TILE_RISE):
    """The two integer ramps of family B over the keys (non-decreasing, 0 at key 0). A probability is formed against a reference that
    is at least the largest score of its own tile (plus BIAS = 3 in the f16 16x16x32 kernel, fa_mfma16_kernel.hip:230-234), and f16
    holds powers of two down to 2^-24 only: rise inside a tile (<= 15) + depth (3) + BIAS (3) stays below 24, so every P is exact in
    every type. The kernel with e4m3 probabilities forms P' = 8 P against its reference (fa_fp8_kernel.hip:13-15); e4m3 is normal down to
    2^-6, so its cases take rise <= 6: rise + depth (3) <= 9 keeps every P' a normal e4m3 power of two, and a step of 6 still sends
    P' to 2^9 > 448, the renewal of the reference (fa_fp8_kernel.hip:15-18). Steps that would pass the budget of their tile are cut
    down to it."""
    mid = (nk // 2) // TILE * TILE
    events = [(p, s, 0) for p, s in [(5, 1), (20, 1), (40, 1), (70, 1), (100, 1), (128, 10), (150, 1), (170, 1), (mid + 37, 12), (nk - 2, 9)]]
    events += [(p, s, 1) for p, s in [(10, 1), (30, 1), (65, 11), (90, 1), (3 * nk // 4, 10)]]
    out = np.zeros((2, nk), np.int64)
    used = {}
    for pos, step, which in sorted(events):
        if not 0 < pos < nk:
            continue
        step = min(step, rise - used.get(pos // TILE, 0))
        if step > 0:
            used[pos // TILE] = used.get(pos // TILE, 0) + step
            out[which, pos:] += step
    return out[0], out[1]


def _spread(r, ncoord=3, cap=16):
    """An integer 0 .. 48 as three near-equal integers 0 .. 16 (each representable in e4m3, whose integers are exact up to 16; all three
    coordinates carry weight as soon as the ramp reaches 3)."""
    out = [r // ncoord + (i < r % ncoord) for i in range(ncoord)]
    assert sum(out).tolist() == r.tolist() and max(int(x.max()) for x in out) <= cap
    return out


def build(family, B, Hq, Hkv, Nq, Nk, D, dtype, causal, kexp=0, span=7, seed=0, lens=None, rise=TILE_RISE):
    """One case: q [B,Hq,Nq,D], k / v [B,Hkv,Nk,D] as fp32 arrays holding values of `dtype`; `lens` (per-sequence key counts, paged
    cache) only enters the reference. Call the kernels with scale = case.scale."""
    assert family in "AB" and Hq % Hkv == 0 and (not causal or Nk >= Nq or lens is not None)
    rng = np.random.default_rng(seed)
    vb = VBITS[dtype]
    Dc = D if family == "A" else D - RESERVED
    c = rng.integers(1, span + 1, (B, Hkv, Nk))  # at least 1: every key but key 0 tells a masked-in coordinate from a masked-out one
    c[:, :, 0] = 0
    k = np.zeros((B, Hkv, Nk, D), np.float32)
    j = np.arange(Nk)
    k[:, :, j, j % Dc] = -c
    q = np.zeros((B, Hq, Nq, D), np.float32)
    q[..., :Dc] = rng.integers(0, 2, (B, Hq, Nq, Dc))
    if family == "B":
        ramp_all, ramp_solo = ramps(Nk, rise)
        for coord, part in zip(ALL_COORDS, _spread(ramp_all)):
            k[..., coord] = part
            q[..., coord] = 1.0
        solo = (np.arange(Nq) % SOLO_EVERY == SOLO_AT).astype(np.float32)
        for coord, part in zip(SOLO_COORDS, _spread(ramp_solo)):
            k[..., coord] = part
            q[..., coord] = solo[None, None, :]
    q *= np.float32(2.0 ** -kexp)
    v = (rng.integers(-(1 << vb), (1 << vb) + 1, (B, Hkv, Nk, D)) / float(1 << vb)).astype(np.float32)
    return SimpleNamespace(family=family, q=q, k=k, v=v, dtype=dtype, causal=bool(causal), kexp=kexp, scale=exact_scale(kexp),
                           span=span, rise=rise, vbits=vb, lens=None if lens is None else [int(x) for x in lens], c=c)


# ---- sliding-window cases (tests/window.py holds their catalogue) -------------------------------------------------------------------
WINDOW_CSPAN = 1      # c_j = 1: the ramp, not c, spreads the scores, and a small c-span leaves the ramp the depth a proven row can have
WINDOW_RESERVED = 6   # the last six coordinates carry the ramp; every query holds 1 there
WINDOW_BUDGET = 21    # (largest - smallest visible score) + c-span of a shallow row: every probability >= 2^-24 with three units to spare
WINDOW_STEP = {"shallow": 1, "steep": 1, "cliff": 3}  # the ramp's step (shallow: once per `every` keys; else per key)
INT_CAP = {"bf16": 256, "f16": 2048, "fp8": 16}  # integers up to here are exact in the type


def window_ramp(ramp, nk, every):
    """The monotone integer ramp along the keys, one step per `every` keys: "fall" from key 0 down to 0 at the last key (keys in front
    of a row's lower bound score above everything it sees), "rise" from 0 at key 0 (keys past its upper bound do)."""
    j = np.arange(nk)
    return (nk - 1 - j) // every if ramp == "fall" else j // every


def _window_every(ramp, Lq, Lk, window, cap_total, cspan):
    """The smallest step length at which, for every live row, the ramp over the keys it sees spans no more than
    WINDOW_BUDGET - 2 * cspan (the scores add at most the c-span to that), a rising ramp climbs by no more than WINDOW_BUDGET - cspan
    inside a 64-key tile, and the ramp's largest value fits the reserved coordinates."""
    case = SimpleNamespace(q=np.zeros((1, 1, Lq, 1)), k=np.zeros((1, 1, Lk, 1)), lens=None, causal=False, window=window)
    vis = visible(case, 0, np.arange(Lq))
    live = vis.any(1)
    first, last = vis.argmax(1)[live], (Lk - 1 - vis[:, ::-1].argmax(1))[live]
    room = WINDOW_BUDGET - 2 * cspan
    every = 1
    while True:
        r = window_ramp(ramp, Lk, every)
        tile_rise = max(int(abs(r[min(t + TILE, Lk) - 1] - r[t])) for t in range(0, Lk, TILE))
        tile_ok = ramp == "fall" or tile_rise <= WINDOW_BUDGET - cspan
        if (not live.any() or int(np.abs(r[last] - r[first]).max()) <= room) and tile_ok and int(r.max()) <= cap_total:
            return every
        every += 1


def build_window(ramp, slope, Hq, Hkv, Lq, Lk, D, dtype, window, kexp=0, seed=0, prove=None, cspan=WINDOW_CSPAN):
    """One sequence under a sliding window (B = 1; case.window = (wl, wr) enters visible()): the construction of build() -- key j carries
    -c_j (1 .. cspan) on coordinate j mod Dc, queries are 0/1 masks, V on its grid, scale = fp32(ln 2) 2^k -- plus a monotone
    integer ramp along the keys (window_ramp) on the WINDOW_RESERVED last coordinates, which every query holds a 1 on.
      slope "shallow": one step per `every` keys, `every` the smallest at which every row's visible depth plus the c-span stays within
              WINDOW_BUDGET (_window_every) and -- with `prove`, the default -- criterion() proves every live row of every head: family
              "A", case.span = the largest visible depth of the case.
      slope "steep": one step per key (bf16: powers of two stay exact far below 2^-24); partial sums may round: family "B".
      slope "cliff": three steps per key (bf16, narrow windows): a key 45 places in front of a row's bound -- every wave has such rows --
              scores 135 above everything the row sees, which no bf16 probability survives. Family "B"."""
    assert ramp in ("fall", "rise") and slope in WINDOW_STEP and Hq % Hkv == 0 and (slope == "shallow" or dtype == "bf16")
    prove = (slope == "shallow") if prove is None else prove
    vb = VBITS[dtype]
    Dc = D - WINDOW_RESERVED
    rng = np.random.default_rng(seed)
    c = rng.integers(1, cspan + 1, (1, Hkv, Lk))
    k = np.zeros((1, Hkv, Lk, D), np.float32)
    j = np.arange(Lk)
    k[:, :, j, j % Dc] = -c
    q = np.zeros((1, Hq, Lq, D), np.float32)
    q[..., :Dc] = rng.integers(0, 2, (1, Hq, Lq, Dc))
    q[..., Dc:] = 1.0
    q *= np.float32(2.0 ** -kexp)
    v = (rng.integers(-(1 << vb), (1 << vb) + 1, (1, Hkv, Lk, D)) / float(1 << vb)).astype(np.float32)
    case = SimpleNamespace(family="A" if slope == "shallow" else "B", q=q, k=k, v=v, dtype=dtype, causal=False, window=tuple(window), kexp=kexp,
                           scale=exact_scale(kexp), span=0, vbits=vb, lens=None, c=c, ramp=ramp, slope=slope, every=1)
    every = 1 if slope != "shallow" else _window_every(ramp, Lq, Lk, window, WINDOW_RESERVED * INT_CAP[dtype], cspan)
    rows = np.arange(Lq)
    vis = visible(case, 0, rows)
    while True:
        r = window_ramp(ramp, Lk, every) * WINDOW_STEP[slope]
        for coord, part in zip(range(Dc, D), _spread(r, WINDOW_RESERVED, INT_CAP[dtype])):
            k[..., coord] = part
        depth = 0
        for h in range(Hq):
            s = scores(case, 0, h, rows)
            live = vis.any(1)
            if live.any():
                depth = max(depth, int((np.where(vis, s, -np.inf).max(1)[live] - np.where(vis, s, np.inf).min(1)[live]).max()))
        case.span, case.every = depth, every
        if not prove or all(criterion(case, reference_head(case, 0, h), False)[vis.any(1)].all() for h in range(Hq)):
            return case
        every += max(1, every // 8)


# ---- representability --------------------------------------------------------------------------------------------------------
def round_bf16(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def round_e4m3(x):
    """RNE to OCP e4m3fn (4 significant bits, smallest normal 2^-6, subnormal step 2^-9), saturating at 448."""
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    step = 2.0 ** (np.maximum(e, -6.0) - 3.0)
    return (np.sign(x) * np.minimum(np.round(ax / step) * step, 448.0)).astype(np.float32)


def round_to(x, dtype):
    x = np.asarray(x, np.float32)
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    if dtype == "bf16":
        return round_bf16(x)
    if dtype == "fp8":
        return round_e4m3(x)
    return x


def representable(x, dtype):
    return bool(np.array_equal(round_to(x, dtype), np.asarray(x, np.float32)))


# ---- the fp64 reference ------------------------------------------------------------------------------------------------------
def visible(case, b, rows):
    """[len(rows), Nk] mask of the keys row i of sequence b sees (bottom-right causal alignment on the sequence's own length; a case
    with `window = (wl, wr)` -- build_window() -- takes the sliding-window rule instead)."""
    Nq, Nk = case.q.shape[2], case.k.shape[2]
    L = Nk if case.lens is None else min(case.lens[b], Nk)
    jj = np.arange(Nk)[None, :]
    vis = np.broadcast_to(jj < L, (len(rows), Nk))
    window = getattr(case, "window", None)
    if window is not None:  # the rule of tests/window.py visible(): the same offset, a negative side is unbounded
        wl, wr = window
        ii = np.asarray(rows, np.int64)[:, None] + (L - Nq)
        return vis & ((jj >= ii - wl) if wl >= 0 else True) & ((jj <= ii + wr) if wr >= 0 else True)
    if case.causal:
        vis = vis & (jj <= np.asarray(rows)[:, None] + (L - Nq))
    return vis


def scores(case, b, h, rows, key_head=None):
    """2^k q_i . k_j in fp64 (exact: integers) for the given rows of head (b, h)."""
    G = case.q.shape[1] // case.k.shape[1]
    hk = h // G if key_head is None else key_head
    return (case.q[b, h, rows].astype(np.float64) @ case.k[b, hk].astype(np.float64).T) * 2.0 ** case.kexp


def reference_head(case, b, h, rows=None, block=512, damage=None):
    """fp64 O [R, D], LSE [R], sum_j p |v| [R, D] (normalised like O), the row maximum m (log2 units), the row sum l (against m) and
    the number of visible keys, for the rows of one head. `damage(ctx)` (sabotage table) may edit the pieces before they are combined."""
    Nq, D = case.q.shape[2], case.q.shape[3]
    rows = np.arange(Nq) if rows is None else np.asarray(rows)
    G = case.q.shape[1] // case.k.shape[1]
    R = len(rows)
    out = SimpleNamespace(o=np.zeros((R, D)), lse=np.full(R, -np.inf), absum=np.zeros((R, D)), m=np.zeros(R), l=np.zeros(R), nvis=np.zeros(R, np.int64), rows=rows)
    for r0 in range(0, R, block):
        rr = rows[r0:r0 + block]
        ctx = SimpleNamespace(case=case, b=b, h=h, rows=rr, hk=h // G)
        if damage is not None:
            damage(ctx, "head")
        s = scores(case, b, h, rr, ctx.hk)
        ctx.vis = visible(case, b, rr)
        if damage is not None:
            damage(ctx, "mask")
        s = np.where(ctx.vis, s, -np.inf)
        nv = ctx.vis.sum(1)
        some = nv > 0
        m = np.where(some, s.max(1, initial=-np.inf), 0.0)
        ctx.p = np.where(ctx.vis, np.exp2(s - m[:, None]), 0.0)  # the weights of the row sum ...
        ctx.p_pv = ctx.p.copy()                                # ... and of the PV product
        ctx.v = case.v[b, ctx.hk].astype(np.float64)
        ctx.s, ctx.m = s, m
        if damage is not None:
            damage(ctx, "weights")
        l = ctx.p.sum(1)
        ls = np.where(some, l, 1.0)
        sl = slice(r0, r0 + len(rr))
        out.o[sl] = (ctx.p_pv @ ctx.v) / ls[:, None]
        out.absum[sl] = (np.abs(ctx.p_pv) @ np.abs(ctx.v)) / ls[:, None]
        out.lse[sl] = np.where(some, LN2 * (m + np.log2(ls)), -np.inf)
        out.m[sl], out.l[sl], out.nvis[sl] = m, l, nv
    return out


# ---- the criterion and the bars ----------------------------------------------------------------------------------------------
def criterion(case, ref, split):
    """Per row: is every fp32 partial sum of the PV product and of the row sum exact, in any order? Family A only, and proven from the
    inputs: V on its grid (every term a multiple of 2^-(span_eff + vbits)), and the magnitude sum_j p |v| -- against the row maximum,
    i.e. un-normalised -- below 2^(24 - span_eff - vbits) on every element of the row; the row sum itself below 2^(24 - span_eff).
    span_eff = span, or 2 * span where every key split has a maximum of its own."""
    R = len(ref.rows)
    if case.family != "A":
        return np.zeros(R, bool)
    grid = float(1 << case.vbits)
    assert np.array_equal(case.v * grid, np.round(case.v * grid)) and np.abs(case.v).max() <= 1.0
    se = case.span * (2 if split else 1)
    mag = (ref.absum * ref.l[:, None]).max(1)
    return (mag < 2.0 ** (24 - se - case.vbits)) & (ref.l < 2.0 ** (24 - se))


def tiles_of(case):
    return (case.k.shape[2] + TILE - 1) // TILE


def bars(case, ref, split=0, shift=0.0):
    """(bar_O [R, D], bar_LSE [R], proven [R]) for one head's reference; split = number of key splits the kernel merges (0: none)."""
    ok = criterion(case, ref, split > 0)
    u = U_OUT[case.dtype]
    a = np.abs(ref.o)
    b_o = u * a
    if case.dtype == "f16":
        b_o = np.maximum(b_o, 2.0 ** -25)  # half the subnormal spacing
    n_sum = np.where(ok, 0, ref.nvis + tiles_of(case)) + (2 * (split + 3) if split else 0)
    b_o = b_o + 2.0 ** -24 * (EPI_O * a + n_sum[:, None] * ref.absum)
    some = ref.nvis > 0
    lse = np.where(some, ref.lse, 0.0)
    lnl = np.log(np.where(some, ref.l, 1.0))
    mag = np.maximum(np.abs(ref.m) * LN2 + np.abs(lnl), np.abs(ref.m + shift) * LN2 + np.abs(lnl - shift * LN2)) + np.abs(lse)
    rel_l = 2.0 ** -24 * (2 + np.where(ok, 0, ref.nvis + tiles_of(case)) + ((split + 3) if split else 0))
    b_l = EPI_L * 2.0 ** -23 * mag + rel_l
    return b_o, b_l, ok


def ratios(case, ref, o, lse, split=0, shift=0.0):
    """Worst error / bar of one head: dict(o=, lse=, proven=fraction of rows under bar A, at=(row, column) of the worst O element).
    Rows without a visible key must hold exactly O = 0 and LSE = -inf (ratio inf otherwise)."""
    b_o, b_l, ok = bars(case, ref, split, shift)
    o, lse = np.asarray(o, np.float64), np.asarray(lse, np.float64)
    some = ref.nvis > 0
    err_o = np.abs(o - ref.o)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_o = np.where(err_o == 0, 0.0, err_o / b_o)
        err_l = np.where(some, np.abs(lse - np.where(some, ref.lse, 0.0)), np.where(np.isneginf(lse), 0.0, np.inf))
        r_l = np.where(err_l == 0, 0.0, err_l / b_l)
    r_o = np.where(np.isfinite(o), r_o, np.inf)
    r_o[~some] = np.where(o[~some] == 0, 0.0, np.inf)
    at = np.unravel_index(np.argmax(r_o), r_o.shape) if r_o.size else (0, 0)
    return dict(o=float(r_o.max(initial=0.0)), lse=float(r_l.max(initial=0.0)), proven=float(ok.mean()) if ok.size else 1.0,
                at=(int(ref.rows[at[0]]) if r_o.size else 0, int(at[1])))


# ---- an fp32 model of the kernels' online softmax (CPU tests) ----------------------------------------------------------------
def model_arrays(q, k, v, vis, c2, in_dtype, p_dtype, out_dtype, thr=8.0, splits=1, interleave=True, shift=0.0, rng=None, prescaled=True,
                 sum_rounded=None):
    """One head through an fp32 online softmax as the kernels run it, on plain arrays: q [Nq, D], k / v [Nk, D] (fp32 values of
    `in_dtype`), vis [Nq, Nk] bool, c2 = c2_of(scale). 64-key tiles; a reference that is renewed only when a score passes it by more than
    `thr` (and sits `shift` from the maximum it was set from); P rounded to `p_dtype` for the PV product; the row sum adds the fp32 P, or
    the rounded ones (`sum_rounded`; default: with e4m3 probabilities); `splits` partial results over interleaved (even / odd) or
    contiguous tile sets, merged by their references; keys of a tile added in a shuffled order; the query operand pre-scaled by c2 and
    rounded to `in_dtype` once (`prescaled`), or every score scaled in fp32. Returns (O rounded to out_dtype, LSE) in fp32."""
    f32 = np.float32
    Nq, D = q.shape
    Nk = k.shape[0]
    if sum_rounded is None:
        sum_rounded = p_dtype == "fp8"
    qs = round_to((q * c2).astype(f32), in_dtype) if prescaled else np.asarray(q, f32)
    nt = (Nk + TILE - 1) // TILE
    owner = (np.arange(nt) % splits) if interleave else (np.arange(nt) * splits // nt)
    parts = []
    for sp in range(splits):
        mref = np.full(Nq, -np.inf, f32)
        l = np.zeros(Nq, f32)
        acc = np.zeros((Nq, D), f32)
        for t in np.flatnonzero(owner == sp):
            keys = np.arange(t * TILE, min(Nk, (t + 1) * TILE))
            if rng is not None:
                keys = rng.permutation(keys)
            s = (qs @ k[keys].T).astype(f32)
            if not prescaled:
                s = (s * c2).astype(f32)
            s = np.where(vis[:, keys], s, f32(-np.inf))
            mx = s.max(1)
            renew = np.isfinite(mx) & (np.isneginf(mref) | (mx > mref - f32(shift) + f32(thr)))
            m_new = np.where(renew, np.maximum(mref, mx + f32(shift)), mref).astype(f32)
            with np.errstate(invalid="ignore"):
                alpha = np.where(np.isneginf(mref), f32(0), np.exp2(mref - m_new)).astype(f32)
            acc = (acc * alpha[:, None]).astype(f32)
            l = (l * alpha).astype(f32)
            mref = m_new
            with np.errstate(invalid="ignore"):
                p = np.where(np.isfinite(s), np.exp2(s - mref[:, None]), 0).astype(f32)
            pr = round_to(p, p_dtype)
            l = (l + (pr if sum_rounded else p).sum(1, dtype=f32)).astype(f32)
            acc = (acc + (pr @ v[keys]).astype(f32)).astype(f32)
        parts.append((mref, l, acc))
    M = np.max([p[0] for p in parts], axis=0)
    lt = np.zeros(Nq, f32)
    at = np.zeros((Nq, D), f32)
    for mref, l, acc in parts:
        with np.errstate(invalid="ignore"):
            w = np.where(np.isneginf(mref), f32(0), np.exp2(mref - M)).astype(f32)
        lt = (lt + l * w).astype(f32)
        at = (at + acc * w[:, None]).astype(f32)
    some = lt > 0
    inv = np.where(some, f32(1) / np.where(some, lt, f32(1)), f32(0)).astype(f32)
    o = round_to((at * inv[:, None]).astype(f32), out_dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = np.where(some, ((M + np.log2(lt).astype(f32)) * LN2_F32), f32(-np.inf)).astype(f32)
    return o, lse


def model_head(case, b, h, p_dtype, out_dtype, thr=8.0, splits=1, interleave=True, shift=0.0, rng=None):
    """All rows of one head of a case through model_arrays (the pre-scaled operand; the row sum adds the fp32 P, or the rounded ones with
    e4m3). Returns (O rounded to out_dtype, LSE) in fp32."""
    hk = h // (case.q.shape[1] // case.k.shape[1])
    vis = visible(case, b, np.arange(case.q.shape[2]))
    return model_arrays(case.q[b, h], case.k[b, hk], case.v[b, hk], vis, c2_of(case.scale), {"fp8": "fp8"}.get(case.dtype, case.dtype), p_dtype,
                        out_dtype, thr, splits, interleave, shift, rng)


# ---- the catalogue: every case the GPU tests run, and the CPU tests check (one list, no copy) --------------------------------------
from collections import namedtuple  # noqa: E402

Spec = namedtuple("Spec", "group family B Hq Hkv Nq Nk D dtype causal kexp seed lens heads rows")
GRID_N = (1, 63, 64, 65, 129, 255, 257, 576, 1000)
GRID_D = (32, 64, 96, 128, 256, 40, 72, 104)
FULL = [  # name, B, H, N, D, dtype, causal, variant, heads, resolved variant (None: by name), kernel-name suffix
    ("config3", 4, 16, 4096, 64, "bf16", True, "auto", [(0, 0), (3, 15)], "mfma16", "64, true, 8, false, 1>"),           # eight-wave 16x16x32
    ("config3_noncausal", 4, 16, 2304, 64, "bf16", False, "auto", [(1, 7), (3, 0)], "mfma16", "64, false, 8, false, 1>"),
    ("config4_shard", 1, 32, 16384, 128, "bf16", True, "auto", [(0, 0), (0, 31)], "mfma16", "128, true, 4, false, 1>"),
    ("config5_fp8pv", 4, 16, 8192, 64, "fp8", True, "mfma_fp8pv", [(0, 0), (3, 15)], None, None),
    ("config5_exact", 4, 16, 8192, 64, "fp8", True, "mfma_exact", [(0, 0), (3, 15)], None, None)]
ROUTES = [  # one shape per kernel AUTO can pick: B, H, N, D, dtype, causal, the variant it resolves to
    (1, 8, 1024, 64, "f16", False, "mfma_splitkv"), (1, 8, 1040, 64, "bf16", True, "mfma_h64s2"), (1, 65, 512, 64, "bf16", False, "mfma"),
    (1, 32, 2048, 64, "bf16", True, "mfma_split2"), (1, 80, 2048, 64, "f16", True, "mfma16"), (1, 80, 1024, 64, "fp8", True, "mfma_fp8pv"),
    (1, 64, 1024, 128, "f16", False, "mfma16"), (1, 32, 2048, 128, "fp8", True, "mfma_fp8pv"), (1, 40, 512, 64, "fp8", True, "mfma_split2")]
GENERALISED = [  # B, Hq, Hkv, Nq, Nk, D, causal: the cases of test_generalised_forward_gqa_and_rectangular
    (2, 8, 2, 200, 200, 64, True), (1, 8, 1, 130, 130, 64, False), (2, 4, 4, 64, 300, 64, True),
    (1, 6, 3, 1, 257, 64, True), (1, 4, 2, 100, 37, 64, False), (1, 8, 2, 129, 512, 128, True),
    (1, 2, 1, 77, 77, 128, True), (1, 16, 4, 33, 1000, 64, True), (1, 4, 2, 70, 150, 32, True),
    (1, 4, 1, 65, 65, 96, False), (1, 2, 2, 40, 300, 256, True),
    (2, 32, 8, 1, 1000, 128, True), (1, 8, 8, 1, 65, 64, False), (4, 32, 8, 16, 700, 64, True),
    (3, 32, 4, 130, 260, 64, True), (1, 72, 8, 128, 128, 128, True)]
DECODE = [  # B, Hq, Hkv, Nq, Nk, D, causal (tests/test_gpu_decode.py CASES)
    (1, 32, 8, 1, 1000, 64, True), (2, 32, 8, 1, 4096, 128, True), (1, 8, 8, 1, 65, 64, False), (4, 32, 8, 4, 700, 64, True),
    (1, 8, 1, 4, 513, 64, True), (1, 16, 2, 1, 2049, 128, False), (1, 4, 4, 16, 300, 64, True), (1, 8, 4, 16, 300, 128, True),
    (1, 2, 2, 32, 129, 64, True), (1, 64, 8, 1, 8192, 64, True), (1, 6, 3, 5, 77, 64, True), (3, 4, 2, 3, 1, 64, False),
    (1, 8, 2, 7, 7, 128, True), (1, 32, 4, 1, 16384, 128, True), (2, 16, 16, 2, 640, 64, False)]
PAGED = [(16, 4, 1, 64, True), (8, 1, 4, 128, True), (4, 4, 2, 64, False), (8, 4, 7, 128, True)]  # Hq, Hkv, Nq, D, causal
PAGE_SIZES = (16, 256)


def _some_heads(B, Hq):
    return None if B * Hq <= 16 else [(0, 0), (B - 1, Hq - 1), (0, Hq // 2), (B - 1, 1)]


def decode_splits(nk):
    """An upper estimate of the work items the decode kernels merge: at most one per 64-key tile, at most 256
    (flash_attention_metal_amd/csrc/fa_decode_kernel.hip:449; the kernel picks S from the chip's item slots, never more)."""
    return min(256, (nk + TILE - 1) // TILE)


def grid_specs(dtype, D, causal):
    """fa_fwd, B = 1, H = 2: N on both sides of every tile / wave / block edge; k = 0 and one k != 0; family B from 129 keys on."""
    for n_i, N in enumerate(GRID_N):
        runs = [("A", 0)] + ([("A", -3)] if N in (65, 1000) else []) + ([("A", 2)] if N in (255, 576) else [])
        runs += [("B", 0 if N != 257 else 1)] if N >= 129 else []
        for family, kexp in runs:
            yield Spec("grid", family, 1, 2, 2, N, N, D, dtype, causal, kexp, 1000 * n_i + D + kexp, None, None, None)


def full_spec(B, H, N, D, dtype, causal, heads):
    rows = None
    if N > 8192:  # the rows the parity tests' _full_size samples, plus every 64th
        rows = np.unique(np.concatenate([[0, 1, 31, 32, 63, 64, 127, 128, N - 129, N - 128, N - 65, N - 64, N - 1],
                                         np.random.default_rng(7).integers(0, N, 48), np.arange(0, N, 64)]))
    return Spec("full", "A", B, H, H, N, N, D, dtype, causal, 0, N + D, None, heads, rows)


def padded_specs(group, dtype="bf16"):
    if group == "fa_fwd":
        return [Spec("padded", f, 3, 5, 5, 320, 320, 64, dtype, True, 0, 5, None, None, None) for f in "AB"]
    if group == "fa_fwd_exv":
        return [Spec("padded", "B", 2, 8, 2, 130, 300, 64, dtype, True, 0, 9, None, None, None)]
    return [Spec("padded", "B", 2, 8, 2, 4, 700, 64, dtype, True, 0, 77, None, None, None)]  # the decode entry points


def generalised_specs(dtype, seed0=0, kexp=None, cases=GENERALISED):
    for ci, (B, Hq, Hkv, Nq, Nk, D, causal) in enumerate(cases):
        for family in (("A", "B") if Nk >= 129 else ("A",)):
            k = (-1 if ci % 3 == 0 else 0) if kexp is None else kexp
            yield Spec("generalised", family, B, Hq, Hkv, Nq, Nk, D, dtype, causal, k, seed0 + ci, None, _some_heads(B, Hq), None)


def decode_specs(dtype):
    """dtype "kv8": bf16 queries on an e4m3 cache (the values are e4m3 either way)."""
    for ci, (B, Hq, Hkv, Nq, Nk, D, causal) in enumerate(DECODE):
        if dtype in ("fp8", "kv8") and Nk * D % 16:
            continue
        for family in (("A", "B") if Nk >= 129 else ("A",)):
            yield Spec("decode", family, B, Hq, Hkv, Nq, Nk, D, "fp8" if dtype == "kv8" else dtype, causal, (0, -2, 1)[ci % 3], 50 + ci, None,
                       _some_heads(B, Hq), None)


def paged_specs(dtype, P):
    """Mixed lengths incl. 0 and lengths that are not a multiple of the page, in a shuffled order per shape."""
    rng = np.random.default_rng(300 + P)
    lens = [0, 1, 63, 64, 65, P - 1, P, P + 1, 1000, 4097]
    for si, (Hq, Hkv, Nq, D, causal) in enumerate(PAGED):
        ls = tuple(int(x) for x in rng.permutation(lens))
        for family in "AB":
            yield Spec("paged", family, len(ls), Hq, Hkv, Nq, max(ls), D, "fp8" if dtype == "kv8" else dtype, causal, (0, -1)[si % 2], 90 + si, ls,
                       [(b, h) for b in range(len(ls)) for h in (0, Hq // 2, Hq - 1)], None)


def make(spec, split, e4m3_p=False):
    """The case of a spec for a kernel class: `split` -- the kernel (or one AUTO may pick) gives every key split a maximum of its own;
    `e4m3_p` -- its probabilities are e4m3 (variant mfma_fp8pv)."""
    span = span_for(spec.dtype, split, spec.Nk) if spec.family == "A" else 3
    return build(spec.family, spec.B, spec.Hq, spec.Hkv, spec.Nq, spec.Nk, spec.D, spec.dtype, spec.causal, kexp=spec.kexp, span=span,
                 seed=spec.seed, lens=spec.lens, rise=TILE_RISE_E4M3 if e4m3_p else TILE_RISE)


def heads_of(spec):
    return spec.heads if spec.heads is not None else [(b, h) for b in range(spec.B) for h in range(spec.Hq)]


def catalogue():
    """(spec, split, e4m3_p) for every case of tests/test_gpu_exact_forward.py, in every kernel class it can be run with there."""
    for dtype in ("f16", "bf16", "fp8"):
        for D in GRID_D:
            for causal in (False, True):
                for spec in grid_specs(dtype, D, causal):
                    yield spec, False, False
                    if spec.family == "A":  # (family B has one depth, 3: the split kernels' cases are the same arrays)
                        yield spec, True, False
                    if dtype == "fp8" and D in (64, 128):
                        yield spec, False, True
    for (_, B, H, N, D, dtype, causal, variant, heads, _, _) in FULL:
        yield full_spec(B, H, N, D, dtype, causal, heads), False, variant == "mfma_fp8pv"
    for (B, H, N, D, dtype, causal, want) in ROUTES:
        yield full_spec(B, H, N, D, dtype, causal, [(0, 0), (0, H - 1)]), want in ("mfma_splitkv", "mfma_split2", "mfma_h64s2"), want == "mfma_fp8pv"
    for dtype in ("f16", "bf16"):
        for spec in list(padded_specs("fa_fwd", dtype)) + list(generalised_specs(dtype)) + list(generalised_specs(dtype, 200, 1, GENERALISED[:11])):
            yield spec, False, False
            if spec.family == "A":
                yield spec, True, False
    for spec in padded_specs("fa_fwd_exv"):
        yield spec, False, False
    for dtype in ("f16", "bf16", "fp8"):
        for spec in list(decode_specs(dtype)) + [s for P in PAGE_SIZES for s in paged_specs(dtype, P)]:
            yield spec, True, False
    for dtype in ("bf16", "fp8"):
        for spec in padded_specs("decode", dtype):
            yield spec, True, False
