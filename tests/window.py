"""The sliding-window cases (pure numpy; shared by tests/test_window_cases.py on the CPU, which checks that every case is what it claims
to be, and tests/test_gpu_window.py on the GPU): the visibility rule of include/fa_mi355.h ("Sliding window"), an fp64 reference built on
it, the catalogue the GPU tests draw from, and a numpy model of the kernels' online softmax with tile skipping.

Key j is visible to query i iff i + coff - wl <= j <= i + coff + wr and 0 <= j < Lk, coff = Lk - Lq; a negative side is unbounded."""
import numpy as np

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
def model(q, k, v, wl, wr, scale=None, bug=None):
    Hq, Lq, D = q.shape
    Hkv, Lk = k.shape[0], k.shape[1]
    sc = D ** -0.5 if scale is None else scale
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
                s = np.where((up & dn)[None], s, -np.inf)
                m_new = np.maximum(np.maximum(m, s.max(-1)), FLOOR)
                alpha = np.exp(np.maximum(m, FLOOR) - m_new) if not first else np.zeros_like(m)
                p = np.exp(s - m_new[..., None])
                l = l * alpha + p.sum(-1)
                acc = acc * alpha[..., None] + p @ ve[:, keys]
                m, first = m_new, False
            live = (rows + cu >= 0) & (l > 0).all(0)
            with np.errstate(divide="ignore", invalid="ignore"):
                o[:, rows] = np.where(live[None, :, None], acc / l[..., None], 0.0)
                lse[:, rows] = np.where(live[None], m + np.log(l), -np.inf)
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
