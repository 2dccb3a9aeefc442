"""The sliding-window cases (pure numpy; shared by tests/test_window_cases.py on the CPU, which checks that every case is what it claims
to be, and tests/test_gpu_window.py on the GPU): the visibility rule of include/fa_mi355.h ("Sliding window"), an fp64 reference built on
it, the catalogue the GPU tests draw from, and a numpy model of the kernels' online softmax with tile skipping.

Key j is visible to query i iff i + coff - wl <= j <= i + coff + wr and 0 <= j < Lk, coff = Lk - Lq; a negative side is unbounded.

At the end: the catalogue of exact-arithmetic cases whose scores ramp along the keys (exact_forward.build_window), for
tests/test_window_exact_cases.py (CPU) and tests/test_gpu_window_exact.py (GPU)."""
import numpy as np

from exact_forward import LN2, build_window, c2_of, round_to, scores, span_for, visible as case_visible

INT_MAX = 2 ** 31 - 1
TILE, BLOCK, WAVE = 64, 128, 32
# (Lq, Lk): the sequences a call is drawn from
SEQS = ((1, 1), (70, 70), (129, 1), (64, 0), (200, 130), (130, 257), (257, 513), (100, 1000))
WL = (0, 1, 31, 63, 64, 65, 127, 200, INT_MAX)
WR = (0, 5, 64, -1)
HEADS = ((4, 4), (8, 2))  # (Hq, Hkv)
# decode: (Nq, L) against a capacity of 4096 keys, a group of 4 query heads per key head
DECODE_NQ = (1, 4)
DECODE_L = (1, 63, 200, 1000)
# the shift identity: (Lq, Lk, wl) and the keys dropped in front (block 0 starts at tile 10); decode: L, Nq, wl, dropped
SHIFT = (100, 1000, 200, 640)
SHIFT_DECODE = (1000, 1, 199, 768)


def visible(Lq, Lk, wl, wr):
    """[Lq, Lk] bool: the rule, in Python ints / int64 (no wrap at INT_MAX)."""
    i = np.arange(Lq, dtype=np.int64)[:, None]
    j = np.arange(Lk, dtype=np.int64)[None, :]
    coff = Lk - Lq
    lo = np.full_like(i, -1) if wl < 0 else i + coff - wl
    hi = np.full_like(i, Lk) if wr < 0 else i + coff + wr
    return (j >= lo) & (j <= hi)


def dead_rows(Lq, Lk, wl, wr):
    """bool [Lq]: rows with no visible key."""
    return ~visible(Lq, Lk, wl, wr).any(1) if Lk else np.ones(Lq, bool)


def unseen_keys(Lq, Lk, wl, wr):
    """bool [Lk]: keys no query of the sequence sees."""
    return ~visible(Lq, Lk, wl, wr).any(0) if Lq else np.ones(Lk, bool)


def identity_claimed(Lq, Lk):
    """(INT_MAX, 0) == causal and (INT_MAX, INT_MAX) == full, bit for bit: the precondition of the header."""
    return Lk >= Lq >= 1


def key_range(Lq, Lk, wl, wr, r0, r1):
    """Brute force over the rule: (lo, hi) of the keys rows r0 .. r1 see together, or None when they see none."""
    vis = visible(Lq, Lk, wl, wr)[max(r0, 0):max(r1 + 1, 0)]
    cols = np.nonzero(vis.any(0))[0] if vis.size else np.array([], int)
    return (int(cols[0]), int(cols[-1]) + 1) if len(cols) else None


def reference(q, k, v, wl, wr, scale=None):
    """fp64 O [Hq, Lq, D] and LSE [Hq, Lq] of one sequence: q [Hq, Lq, D], k / v [Hkv, Lk, D]. Dead rows: O = 0, LSE = -inf."""
    Hq, Lq, D = q.shape
    Hkv, Lk = k.shape[0], k.shape[1]
    sc = D ** -0.5 if scale is None else scale
    o, lse = np.zeros((Hq, Lq, D)), np.full((Hq, Lq), -np.inf)
    if Lq == 0 or Lk == 0:
        return o, lse
    vis = visible(Lq, Lk, wl, wr)
    live = vis.any(1)
    ke, ve = (np.repeat(x.astype(np.float64), Hq // Hkv, axis=0) for x in (k, v))
    s = np.where(vis[None], (q.astype(np.float64) @ ke.swapaxes(-1, -2)) * sc, -np.inf)
    m = np.where(live, s.max(-1), 0.0)
    p = np.exp(s - m[..., None])
    l = p.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where(live[None, :, None], (p @ ve) / l[..., None], 0.0)
        lse = np.where(live[None], m + np.log(l), -np.inf)
    return o, lse


# ---- a model of the 128-row kernel's walk (csrc/fa_mfma_kernel.hip, window mode): per 128-row block the tiles [t_lo, nT) of the block's
# key range, per 32-row wave the skip of tiles wholly outside its rows' bounds, per score the two-sided mask, an online softmax in fp64
# whose reference maximum starts at the wave's first active tile with a finite floor. `bug` plants one mistake:
#   "lo_edge" / "hi_edge": the lower / upper mask off by one; "start_last_row": the block's first tile taken from its LAST row's bound;
#   "no_lower_in_recompute": the lower mask missing on tiles that take the exact path after the first; "ignore_wr": the upper offset
#   without wr.
#   "max_over_hidden": the reference maximum of a tile taken before the mask is applied.
# p_dtype ("f16" / "bf16"; None: fp64): every probability is rounded to that type before it enters the PV sum, as in the kernels (the
# row sum adds the unrounded ones): a reference that sits too high flushes probabilities to zero, which fp64 alone would not show.
# base2: scores in log2 units (times exact_forward.c2_of(scale), a power of two on exact-arithmetic inputs) and exp2, as the kernels run
# it: every probability of such inputs is then the exact power of two (exp(n ln 2) in fp64 is not).
def model(q, k, v, wl, wr, scale=None, bug=None, p_dtype=None, base2=False):
    Hq, Lq, D = q.shape
    Hkv, Lk = k.shape[0], k.shape[1]
    sc = D ** -0.5 if scale is None else scale
    ex, unit = np.exp, 1.0
    if base2:
        sc, ex, unit = float(c2_of(sc)), np.exp2, LN2
    o, lse = np.zeros((Hq, Lq, D)), np.full((Hq, Lq), -np.inf)
    if Lq == 0 or Lk == 0:
        return o, lse
    wl_ = Lk if (wl < 0 or wl > Lk) else wl       # the host's clamp
    wr_ = Lq if (wr < 0 or wr > Lq) else wr
    coff = Lk - Lq
    cl, cu = coff - wl_, coff + (0 if bug == "ignore_wr" else wr_)
    FLOOR = -3.4028234663852886e38
    ke, ve = (np.repeat(x.astype(np.float64), Hq // Hkv, axis=0) for x in (k, v))
    q64 = q.astype(np.float64)
    for q0 in range(0, Lq, BLOCK):
        r_last = min(q0 + BLOCK - 1, Lq - 1)
        lo = max(0, (r_last if bug == "start_last_row" else q0) + cl)
        hi = min(Lk, r_last + cu + 1)
        if lo >= hi:
            continue
        t_lo, nT = lo // TILE, (hi + TILE - 1) // TILE
        for qw0 in range(q0, min(q0 + BLOCK, Lq), WAVE):
            rows = np.arange(qw0, min(qw0 + WAVE, Lq))
            m = np.full((Hq, len(rows)), -np.inf)
            l = np.zeros((Hq, len(rows)))
            acc = np.zeros((Hq, len(rows), D))
            first = True
            for t in range(t_lo, nT):
                kv0 = t * TILE
                if kv0 > qw0 + WAVE - 1 + cu or kv0 + TILE - 1 < qw0 + cl:
                    continue
                keys = np.arange(kv0, min(kv0 + TILE, Lk))
                s = (q64[:, rows] @ ke[:, keys].swapaxes(-1, -2)) * sc
                up = keys[None, :] <= rows[:, None] + cu + (1 if bug == "hi_edge" else 0)
                dn = keys[None, :] >= rows[:, None] + cl + (1 if bug == "lo_edge" else 0)
                if bug == "no_lower_in_recompute" and not first:
                    dn = np.ones_like(dn)
                raw = s
                s = np.where((up & dn)[None], s, -np.inf)
                m_new = np.maximum(np.maximum(m, (raw if bug == "max_over_hidden" else s).max(-1)), FLOOR)
                alpha = ex(np.maximum(m, FLOOR) - m_new) if not first else np.zeros_like(m)
                p = ex(s - m_new[..., None])
                l = l * alpha + p.sum(-1)
                acc = acc * alpha[..., None] + (p if p_dtype is None else round_to(p, p_dtype).astype(np.float64)) @ ve[:, keys]
                m, first = m_new, False
            live = (rows + cu >= 0) & (l > 0).all(0)
            with np.errstate(divide="ignore", invalid="ignore"):
                o[:, rows] = np.where(live[None, :, None], acc / l[..., None], 0.0)
                lse[:, rows] = np.where(live[None], unit * (m + (np.log2(l) if base2 else np.log(l))), -np.inf)
    return o, lse


def draw(round_to, rng, dtype, *shape):
    return round_to(rng.uniform(-1.0, 1.0, shape).astype(np.float32), dtype)


def draw_seqs(round_to, rng, Hq, Hkv, D, dtype, lens):
    return [(draw(round_to, rng, dtype, Hq, Lq, D), draw(round_to, rng, dtype, Hkv, Lk, D), draw(round_to, rng, dtype, Hkv, Lk, D)) for Lq, Lk in lens]


# the GPU catalogue: (name, sequences, wl, wr). Every wl and every wr of the issue appears, every sequence appears under a small and a
# large window, and the calls stay few: one launch per case and (dtype, D, heads).
CASES = (
    ("point", SEQS, 0, 0),                 # the known answer: O = V[i + coff]
    ("w1", SEQS, 1, 0),
    ("w31_r5", SEQS, 31, 5),
    ("w63", SEQS, 63, 0),
    ("w64_r64", SEQS, 64, 64),             # a symmetric band
    ("w65_unbounded_right", SEQS, 65, -1),
    ("w127_r5", SEQS, 127, 5),
    ("w200", SEQS, 200, 0),
    ("left_unbounded_r5", SEQS, -1, 5),    # the windowed kernels with no lower bound that binds
    ("intmax_causal", SEQS, INT_MAX, 0),
    ("intmax_full", SEQS, INT_MAX, INT_MAX),
)


# ---- exact-arithmetic inputs with per-row score ranges (exact_forward.build_window): the catalogue of tests/test_gpu_window_exact.py,
# walked on the CPU by tests/test_window_exact_cases.py. One sequence per case; a call packs the sequences of one (window, ramp, slope).
EXACT_SEQS = ((70, 70), (200, 130), (130, 257), (257, 513), (100, 1000))  # (200, 130): dead rows; (130, 257): coff = 127
EXACT_WINDOWS = ((15, 0), (63, 0), (64, 64), (127, 5), (200, 0), (65, -1), (-1, 5))
STEEP_WINDOWS = ((15, 0), (63, 0), (127, 5))
CLIFF_WINDOWS = ((15, 0),)  # (wider ones would flush a row's own deepest probabilities)
CLIFF_SEQS = EXACT_SEQS[:4]  # 3 (Lk - 1) within six bf16-exact coordinates
RAMPS = ("fall", "rise")
EXACT_MATRIX = tuple((D, heads) for D in (64, 128) for heads in HEADS)
KEXP = {64: 0, 128: -1}  # one per head dim
FLUSH = {"f16": 24, "bf16": 133}  # a probability more than this far below the reference is zero in the type
EXACT_DECODE_L = (63, 200, 1000)
EXACT_DECODE_WINDOWS = ((0, 0), (31, 0), (64, 5), (200, -1))
EXACT_DECODE_HEADS = (8, 2)
# The claim that gives a case its teeth (hidden_margin(), at least half of the live rows) fails on these: left out, per the rule that
# a (window, ramp) pair stays only where every one of its cases meets the claim. slope, dtype, ramp, window, sequences.
LEFT_OUT = (
    ("shallow", "f16", "rise", (15, 0), None),  # a rising ramp may climb 20 per tile: one step per 4 keys at the least, too flat for this window
    ("shallow", "f16", "fall", (63, 0), ((70, 70), (200, 130), (100, 1000))),  # (blocks with few rows behind their first row's bound)
    ("shallow", "f16", "rise", (63, 0), ((70, 70), (200, 130), (100, 1000))),
    ("shallow", "f16", "fall", (64, 64), None), ("shallow", "f16", "rise", (64, 64), None),  # 129 and more visible keys: a row that is
    ("shallow", "f16", "fall", (127, 5), None), ("shallow", "f16", "rise", (127, 5), None),  # proven exact has a ramp too flat to put a
    ("shallow", "f16", "fall", (200, 0), None), ("shallow", "f16", "rise", (200, 0), None),  # block-mate's key 24 above its smallest score
    ("shallow", "f16", "fall", (65, -1), None), ("shallow", "f16", "rise", (-1, 5), None),
    ("steep", "bf16", "fall", (15, 0), None), ("steep", "bf16", "rise", (15, 0), None),      # 127 steps inside a block + a depth of 16 / 64
    ("steep", "bf16", "fall", (63, 0), None), ("steep", "bf16", "rise", (63, 0), None),      # reach 133 on too few rows
    ("steep", "bf16", "fall", (127, 5), ((70, 70), (200, 130))), ("steep", "bf16", "rise", (127, 5), ((70, 70), (200, 130))),
    ("cliff", "bf16", "fall", (15, 0), ((70, 70), (200, 130))),
)


def bound_binds(ramp, wl, wr):
    """The ramp puts keys a row does not see ABOVE what it sees only past a bounded side: in front of the lower bound when it falls,
    past the upper bound when it rises."""
    return wl >= 0 if ramp == "fall" else wr >= 0


def left_out(slope, dtype, ramp, window, seq):
    return any(e[:4] == (slope, dtype, ramp, tuple(window)) and (e[4] is None or tuple(seq) in e[4]) for e in LEFT_OUT)


def exact_specs(dtype, slope):
    """(ramp, window, [sequences]) of every packed call of one value type and slope."""
    assert slope == "shallow" or dtype == "bf16"
    for window in {"shallow": EXACT_WINDOWS, "steep": STEEP_WINDOWS, "cliff": CLIFF_WINDOWS}[slope]:
        for ramp in RAMPS:
            seqs = [s for s in (CLIFF_SEQS if slope == "cliff" else EXACT_SEQS) if not left_out(slope, dtype, ramp, window, s)]
            if seqs:
                yield ramp, window, seqs


_CASES = {}


def exact_case(ramp, slope, window, seq, D, heads, dtype):
    """The case of one sequence (built once per process; f16 and bf16 shallow cases hold the same values)."""
    key = (ramp, slope, tuple(window), tuple(seq), D, tuple(heads))
    if key not in _CASES:
        seed = 9000 + 7 * EXACT_SEQS.index(tuple(seq)) + 100 * (EXACT_WINDOWS.index(tuple(window)) + 1) + D + heads[0] + (1 if ramp == "rise" else 0)
        _CASES[key] = build_window(ramp, slope, heads[0], heads[1], seq[0], seq[1], D, "bf16", window, kexp=KEXP[D], seed=seed)
    case = _CASES[key]
    return case if dtype == "bf16" else type(case)(**{**vars(case), "dtype": dtype})


def decode_case(ramp, window, Nq, L, D, dtype):
    """A decode step's case: Nq rows against L keys, the shallow ramp within the exact integers and the V grid of `dtype` ("fp8": an
    e4m3 cache), c_j in 1 .. span_for(dtype, True, L). Every key split has a maximum of its own, so no row is asked to be proven
    (bars(..., split=S) decides per row)."""
    key = ("decode", ramp, tuple(window), Nq, L, D, dtype)
    if key not in _CASES:
        Hq, Hkv = EXACT_DECODE_HEADS
        seed = 9500 + L + 10 * Nq + D + EXACT_DECODE_WINDOWS.index(tuple(window)) + (1 if ramp == "rise" else 0)
        _CASES[key] = build_window(ramp, "shallow", Hq, Hkv, Nq, L, D, dtype, window, kexp=KEXP[D], seed=seed, prove=False, cspan=span_for(dtype, True, L))
    return _CASES[key]


def hidden_margin(case, flush):
    """Per head, the fraction of live rows with a key they do NOT see, that another row of the same 128-row block DOES see, and whose
    score lies more than `flush` above the row's smallest visible score -- above its maximum by more than flush - visible depth: a
    reference set from that key sends at least one of the row's probabilities to zero in the type. Returns the smallest fraction."""
    Lq, Hq = case.q.shape[2], case.q.shape[1]
    rows = np.arange(Lq)
    vis = case_visible(case, 0, rows)
    live = vis.any(1)
    block_sees = np.zeros_like(vis)
    for q0 in range(0, Lq, BLOCK):
        block_sees[q0:q0 + BLOCK] = vis[q0:q0 + BLOCK].any(0)[None]
    out = 1.0
    for h in range(Hq):
        s = scores(case, 0, h, rows)
        best_hidden = np.where(block_sees & ~vis, s, -np.inf).max(1)
        smallest = np.where(vis, s, np.inf).min(1)
        out = min(out, float((best_hidden[live] - smallest[live] > flush).mean()) if live.any() else 1.0)
    return out
