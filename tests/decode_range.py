"""Decode inputs with many key splits and with scores far from zero, and a numpy model of the decode kernels' arithmetic (test side
only; pure numpy, so the CPU test of the cases and the GPU test share them).

flash_attention_metal_amd/csrc/fa_decode_kernel.hip packs the R = (Hq / Hkv) * Nq rows of a key head into one block (row r = gi * Nq + iq), gives split s of S the
64-key tiles [s * nT / S, (s + 1) * nT / S), runs an online softmax per tile inside a split and merges the S partial results by their
maxima, lane l of the combine taking splits l, l + 64, l + 128, l + 192. The cases reach what ordinary U(-1,1) data at up to 64
splits cannot: S = 65 ... 256, uneven partitions under the cap, splits / tiles / rows of one block at very different depths, spikes.
Scores are in log2 units on Q~ = round(scale * log2(e) * Q) ("depth"), the construction is tests/score_range.py's: q = alpha * u + noise,
k = -beta * u + noise with |u| = 1. Every builder takes the oracle's round_to and a dtype ("f16", "bf16", "fp8": the e4m3 values serve
both the all-e4m3 mode and bf16 queries on an e4m3 cache) and returns Cases of exactly representable values with what they claim:
  S          the split count the case was written for (asserted against the library by the GPU test: splits_of)
  top_key    int [B, Hq, Nq]: the key that holds the row maximum; -1: no claim; -2: the head's spike is masked for this row, whose
             maximum stays a log2 unit and more below the spike's score (seeing the spike would at least double its row sum)
  top_split  int [B, Hq, Nq]: the split (of S) that holds the row maximum; -1: no claim
  depth      float [B, Hq, Nq] (nan: no claim): the row maximum lies within span(depth) = 0.5 + 0.06 |depth| of it
tests/test_decode_range_cases.py checks the claims from fp64 scores and runs model() -- and its sabotaged forms -- against the bars of
tests/test_gpu_decode_range.py, which runs the kernels.
"""
from collections import namedtuple

import numpy as np

from score_range import LOG2E, _noise, log2_scores, product_for, unit  # noqa: F401  (log2_scores: what scores() computes)

Case = namedtuple("Case", "name q k v causal S top_key top_split depth")
TILE = 64
LN2 = 0.6931471805599453
MODES = ("f16", "bf16", "fp8", "kv8")  # queries / cache: f16, bf16, e4m3 / e4m3, bf16 / e4m3
BUILD = {"f16": "f16", "bf16": "bf16", "fp8": "fp8", "kv8": "fp8"}  # the values a mode runs on
ARITH = {"f16": "f16", "bf16": "bf16", "fp8": "bf16", "kv8": "bf16"}  # e4m3 inputs are widened exactly: the arithmetic is bf16
ALPHA = {"f16": 2.0, "bf16": 2.0, "fp8": 8.0}  # e4m3 ends at 448: a larger alpha keeps beta = product / alpha inside it
# Many-split shapes, B = 1 and Hkv = 2: S = min(nT / 4, 256) for both head dims and all four modes
S_OF_NK = {16704: 65, 20000: 78, 33000: 129, 49500: 193, 65536: 256, 70001: 256, 1100: 4}
# e4m3 heads are 16-byte aligned (Nk * D % 16 == 0): (family, case name) pairs the e4m3 modes leave out. Every case here has D = 64 or
# 128, so none does; tests/test_decode_range_cases.py checks the list against the shapes.
E4M3_LEFT_OUT = ()


def span(depth):
    return 0.5 + 0.06 * np.abs(depth)


def tiles(Nk):
    return (Nk + TILE - 1) // TILE


def split_tiles(Nk, S):
    """(t0, t1) [S] each: split s streams tiles [t0, t1) (fa_decode_kernel.hip: t0 = s * nT / S)."""
    s = np.arange(S + 1, dtype=np.int64) * tiles(Nk) // S
    return s[:-1], s[1:]


def split_of_key(Nk, S):
    """[Nk]: the split that streams key j."""
    t0, _ = split_tiles(Nk, S)
    return np.searchsorted(t0, np.arange(Nk) // TILE, side="right") - 1


def splits_of(fa, B, Hq, Hkv, Nq, Nk, D):
    """S as the library sizes its workspace: bytes / (B * Hkv * 16 * QT * (D + 2) * 4). The workspace serves every dtype, so this is the
    larger of the 16-bit and the e4m3 split count; on the shapes of S_OF_NK the two agree."""
    QT = ((Hq // Hkv) * Nq + 15) // 16
    per = B * Hkv * 16 * QT * (D + 2) * 4
    n = fa.decode_workspace_bytes(B, Hq, Hkv, Nq, Nk, D)
    assert n % per == 0
    return n // per


def paged_splits_of(fa, B, Hq, Hkv, Nq, D, P, max_pages):
    QT = ((Hq // Hkv) * Nq + 15) // 16
    per = B * Hkv * 16 * QT * (D + 2) * 4
    n = fa.decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, P, max_pages)
    assert n % per == 0
    return n // per


def _uniform(round_to, dtype, rng, shape):
    return round_to(rng.uniform(-1, 1, shape).astype(np.float32), dtype)


def _none(B, Hq, Nq):
    return np.full((B, Hq, Nq), -1), np.full((B, Hq, Nq), -1), np.full((B, Hq, Nq), np.nan)


# ---- L: many splits, ordinary data ------------------------------------------------------------------------------------------------
def ordinary(round_to, dtype, Hq, Hkv, Nq, Nk, D, seed=1):
    rng = np.random.default_rng(seed + Nk + D)
    q, k, v = (_uniform(round_to, dtype, rng, s) for s in ((1, Hq, Nq, D), (1, Hkv, Nk, D), (1, Hkv, Nk, D)))
    return Case(f"ordinary Hq={Hq} Nq={Nq} Nk={Nk} D={D}", q, k, v, Nq > 1, S_OF_NK[Nk], *_none(1, Hq, Nq))


# ---- S, T, U: every row at a depth that depends on the key (its split, its tile) or on the batch entry -----------------------------------
def by_key(round_to, dtype, name, key_depth, B, Hq, Hkv, Nq, Nk, D, S, seed=2):
    """key_depth [Nk] or [B, Nk] (<= 0): the depth of every row's score against key j. The noise of q is orthogonal to u (no row-wide
    shift of a depth); that of k spreads a row's scores by alpha * 0.05 * scale * log2(e) < 0.1 log2 units."""
    rng, u, alpha = np.random.default_rng(seed + D), unit(D), ALPHA[dtype]
    kd = np.broadcast_to(np.asarray(key_depth, np.float64), (B, Nk))
    beta = (product_for(kd, D) / alpha).astype(np.float32)[:, None, :, None]
    nq = _noise(rng, (B, Hq, Nq, D))
    nq -= (nq @ u)[..., None] * u
    q = round_to(np.float32(alpha) * u + nq, dtype)
    k = round_to(-beta * u + _noise(rng, (B, Hkv, Nk, D)), dtype)
    causal = Nq > 1
    top = np.empty((B, Hq, Nq))
    where = np.empty((B, Hq, Nq), np.int64)
    sk = split_of_key(Nk, S)
    for iq in range(Nq):  # the deepest visible level decides (causal: the last Nq - 1 - iq keys are masked)
        vis = Nk - (Nq - 1 - iq) if causal else Nk
        top[:, :, iq] = kd[:, :vis].max(1)[:, None]
        for b in range(B):  # (levels that several splits share claim no split)
            at = np.unique(sk[:vis][kd[b, :vis] == kd[b, :vis].max()])
            where[b, :, iq] = at[0] if len(at) == 1 else -1
    return Case(name, q, k, _uniform(round_to, dtype, rng, k.shape), causal, S, np.full((B, Hq, Nq), -1), where, top)


def split_levels(round_to, dtype, Nk, D, kind, at=None, Hq=8, Hkv=2, Nq=1):
    """(S) one depth per key split. 'up' / 'down': a step per split of 3 log2 units at S = 65 and 1 at S = 256 (the far end weighs
    2^-190 and less); 'one': split `at` 40 above all others."""
    S = S_OF_NK[Nk]
    step = 3.0 if S <= 65 else 1.0
    s = split_of_key(Nk, S)
    d = {"up": -step * (S - 1 - s), "down": -step * s, "one": np.where(s == at, 0.0, -40.0)}[kind]
    return by_key(round_to, dtype, f"splits {kind}{'' if at is None else ' at %d' % at} S={S} D={D}", d, 1, Hq, Hkv, Nq, Nk, D, S, seed=3)


def tile_climb(round_to, dtype, D, start, step, Nk=1100):
    """(T) every 64-key tile `step` above (below) the one before, inside the 4 - 5 tiles of a split and across the splits."""
    d = start + step * (np.arange(Nk) // TILE)
    assert d.max() <= 0.0
    return by_key(round_to, dtype, f"tiles from {start:g} by {step:+g} D={D}", d, 1, 8, 2, 4, Nk, D, S_OF_NK[Nk], seed=4)


DEPTHS_U = (-6.0, -14.0, -22.0, -30.0, -60.0, -75.0)


def uniform_depth(round_to, dtype, Nk, D):
    """(U) batch entry b has every row at DEPTHS_U[b]. B * Hkv = 12: S = min(ceil(256 * per_cu / 12), nT / 4) is 4 at 1100 keys and, at head
    dim 64, 65 at 16704 for every mode (at head dim 128 the 16-bit modes would run 43 items: not used there)."""
    assert D == 64 or Nk == 1100
    B = len(DEPTHS_U)
    d = np.repeat(np.asarray(DEPTHS_U)[:, None], Nk, 1)
    return by_key(round_to, dtype, f"uniform depth Nk={Nk} D={D}", d, B, 8, 2, 1, Nk, D, S_OF_NK[Nk], seed=5)


# ---- R: the rows of one packed block at different depths -------------------------------------------------------------------------------
def row_ramp(round_to, dtype, Hq, Hkv, Nq, Nk, D, deepest, seed=6):
    """(R) packed row r = gi * Nq + iq of a key head at depth deepest * r / (R - 1): the ramp is in alpha, beta is small (20; 40 for the
    e4m3 values at head dim 128, whose alpha would pass 448), as score_range.ramp."""
    rng, u = np.random.default_rng(seed + D + Nk), unit(D)
    G = Hq // Hkv
    R = G * Nq
    beta = 40.0 if (dtype == "fp8" and D == 128) else 20.0
    d = deepest * np.arange(R) / (R - 1.0)
    alpha = (product_for(d, D) / beta).astype(np.float32).reshape(G, Nq)
    nq = _noise(rng, (1, Hq, Nq, D))
    nq -= (nq @ u)[..., None] * u
    q = round_to(np.tile(alpha, (Hkv, 1))[None, :, :, None] * u + nq, dtype)
    k = round_to(-np.float32(beta) * u + _noise(rng, (1, Hkv, Nk, D)), dtype)
    depth = np.tile(d.reshape(G, Nq), (Hkv, 1))[None]
    return Case(f"rows 0 to {deepest:g} R={R} Hkv={Hkv} Nk={Nk} D={D}", q, k, _uniform(round_to, dtype, rng, k.shape), Nq > 1, S_OF_NK[Nk],
                np.full((1, Hq, Nq), -1), np.full((1, Hq, Nq), -1), depth)


# ---- K: spikes ----------------------------------------------------------------------------------------------------------------------------
SPIKES = (30.0, 400.0, 900.0, 1200.0, 2000.0, 3000.0)


def _orthogonal(rng, n, D):
    """n mutually orthogonal rows of U(-1,1)-sized entries (Gram-Schmidt on U(-1,1) draws; rounding to the type leaves q_i . q_j / |q_i|^2
    of a few 1e-3 in bf16 and 1e-2 in e4m3: a spike of score c for one row moves the others by that fraction of c)."""
    x = rng.uniform(-1, 1, (n, D))
    for i in range(n):
        for j in range(i):
            x[i] -= (x[i] @ x[j]) / (x[j] @ x[j]) * x[j]
    return x.astype(np.float32)


def spike_positions(Nk, S):
    """Key 0; the last key of tile 0 and the first of tile 1; the last key of a split and the first of the next; inside the ragged
    last tile; the last key."""
    t0, t1 = split_tiles(Nk, S)
    edge = int(t1[S // 2]) * TILE
    ragged = (tiles(Nk) - 1) * TILE + (Nk - (tiles(Nk) - 1) * TILE) // 2
    pos = [0, TILE - 1, TILE, edge - 1, edge, ragged, Nk - 1]
    assert len(set(pos)) == 7 and split_of_key(Nk, S)[edge - 1] + 1 == split_of_key(Nk, S)[edge]
    return pos


def spikes(round_to, dtype, Nk, D, seed=7):
    """(K) B = 3, 14 query heads on 2 key heads, one query: the 7 rows of a key head are mutually orthogonal, row r has the key
    c * q_r / |q_r|^2 (score c for that row alone) at spike_positions()[r], and c is SPIKES[2 b + hkv]: every position with every size."""
    rng = np.random.default_rng(seed + Nk + D)
    B, Hq, Hkv, G, S = 3, 14, 2, 7, S_OF_NK[Nk]
    pos = spike_positions(Nk, S)
    q = np.stack([np.concatenate([_orthogonal(rng, G, D) for _ in range(Hkv)]) for _ in range(B)])[:, :, None, :]
    q = round_to(q, dtype)
    k = rng.uniform(-1, 1, (B, Hkv, Nk, D)).astype(np.float32)
    top = np.empty((B, Hq, 1), np.int64)
    for b in range(B):
        for h in range(Hkv):
            for r in range(G):
                qi = q[b, h * G + r, 0].astype(np.float64)
                k[b, h, pos[r]] = SPIKES[2 * b + h] * qi / (qi @ qi)
                top[b, h * G + r, 0] = pos[r]
    k = round_to(k, dtype)
    return Case(f"spikes Nk={Nk} D={D}", q, k, _uniform(round_to, dtype, rng, k.shape), False, S, top, split_of_key(Nk, S)[top],
                np.full((B, Hq, 1), np.nan))


def causal_spikes(round_to, dtype, Nk, D, seed=8):
    """(K, causal) B = 3, 8 query heads on 2 key heads, Nq = 4: the four queries of a head are one vector, the 4 heads of a key head are
    mutually orthogonal, and head gi = 0, 1, 2 has its spike at key Nk - 1, Nk - 2, Nk - 4 -- visible to query 3 only, to queries 2 and
    3, to all four (bottom-right aligned mask); head 3 has none. c is SPIKES[2 b + hkv]."""
    rng = np.random.default_rng(seed + Nk + D)
    B, Hq, Hkv, G, Nq, S = 3, 8, 2, 4, 4, S_OF_NK[Nk]
    q = np.stack([np.concatenate([_orthogonal(rng, G, D) for _ in range(Hkv)]) for _ in range(B)])
    q = round_to(np.repeat(q[:, :, None, :], Nq, 2), dtype)
    k = rng.uniform(-1, 1, (B, Hkv, Nk, D)).astype(np.float32)
    top = np.full((B, Hq, Nq), -1, np.int64)
    for b in range(B):
        for h in range(Hkv):
            for gi, back in enumerate((1, 2, 4)):
                qi = q[b, h * G + gi, 0].astype(np.float64)
                k[b, h, Nk - back] = SPIKES[2 * b + h] * qi / (qi @ qi)
                for iq in range(Nq):
                    top[b, h * G + gi, iq] = Nk - back if Nk - back <= iq + Nk - Nq else -2
    k = round_to(k, dtype)
    return Case(f"causal spikes Nk={Nk} D={D}", q, k, _uniform(round_to, dtype, rng, k.shape), True, S, top,
                np.where(top >= 0, split_of_key(Nk, S)[np.maximum(top, 0)], -1), np.full((B, Hq, Nq), np.nan))


# ---- the families of tests/test_gpu_decode_range.py: name -> [build(round_to, dtype) -> Case] ----------------------------------------------
NK_L = (16704, 20000, 33000, 49500, 65536, 70001, 1100)
DOMINANT_AT = (63, 64, 127, 128, 191, 192, 255)
RAMPS = (-30.0, -200.0, -1400.0)
SHAPES_R = ((16, 2, 4), (32, 1, 1), (8, 2, 4))  # Hq, Hkv, Nq: R = 32 (causal), R = 32, R = 16 (causal)


def _case(builder, *args, **kw):
    """A case not yet built: call it with (round_to, dtype). (The large ones take a second to draw: they are built one at a time.)"""
    def build(round_to, dtype):
        return builder(round_to, dtype, *args, **kw)
    build.label = builder.__name__ + "".join(f"-{x:g}" if isinstance(x, (int, float)) else f"-{x}" for x in list(args) + list(kw.values()))
    return build


def family_L():
    out = [_case(ordinary, 8, 2, 1, Nk, D) for D in (64, 128) for Nk in NK_L]
    return out + [_case(ordinary, Hq, 2, 4, Nk, D) for D in (64, 128) for Hq in (8, 16) for Nk in (16704, 70001)]


def family_S():
    out = [_case(split_levels, Nk, D, kind) for (Nk, D) in ((16704, 64), (65536, 128)) for kind in ("up", "down")]
    out += [_case(split_levels, 16704, 128, "one", at=40), _case(split_levels, 1100, 64, "one", at=2)]
    return out + [_case(split_levels, 65536, 64 if i % 2 else 128, "one", at=at, Hq=16, Nq=4) for i, at in enumerate(DOMINANT_AT)]


def family_T():
    return [_case(tile_climb, D, start, step) for D in (64, 128) for (start, step) in ((-40.0, 2.0), (-204.0, 12.0), (0.0, -12.0))]


def family_R():
    out = [_case(row_ramp, Hq, Hkv, Nq, 1100, D, deep) for (Hq, Hkv, Nq) in SHAPES_R for D in (64, 128) for deep in RAMPS]
    return out + [_case(row_ramp, Hq, Hkv, Nq, 16704, D, deep) for (Hq, Hkv, Nq, D) in ((16, 2, 4, 64), (32, 1, 1, 128)) for deep in RAMPS]


def family_U():
    return [_case(uniform_depth, 1100, 64), _case(uniform_depth, 1100, 128), _case(uniform_depth, 16704, 64)]


def family_K():
    return [_case(f, Nk, D) for f in (spikes, causal_spikes) for (Nk, D) in ((1100, 64), (1100, 128), (16704, 64), (16704, 128))]


FAMILIES = {"L": family_L(), "S": family_S(), "T": family_T(), "R": family_R(), "U": family_U(), "K": family_K()}
PAGED_FAMILIES = ("L", "S", "R", "K")


# ---- the bars (tests/test_gpu_decode_range.py says where they come from) -------------------------------------------------------------------
def bars(mode, lse_ref):
    """(bar on |O - oracle on Q~|, bar on |LSE - oracle on Q~| per row): twice the parity bars, plus four fp32 roundings of the LSE itself."""
    from util import TOL_LSE, TOL_O

    a = ARITH[mode]
    return 2.0 * TOL_O[a], 2.0 * TOL_LSE[a] + 4.0 * 2.0 ** -23 * np.abs(lse_ref)


def q_tilde(round_to, q, mode):
    """util.effective_q for a mode: e4m3 queries are widened to bf16 before the product (scale LN2 goes with it)."""
    c2 = np.float32(np.float32(q.shape[-1] ** -0.5) * np.float32(1.4426950408889634))
    return round_to((q.astype(np.float32) * c2).astype(np.float32), ARITH[mode])


def scores(round_to, c, mode):
    """score_range.log2_scores of a case -- fp64 scores of Q~ in log2 units, [B, Hq, Nq, Nk], masked entries -inf -- without its copy of K
    per query head (these K have up to 70001 rows)."""
    B, Hq, Nq, D = c.q.shape
    Hkv, Nk = c.k.shape[1], c.k.shape[2]
    qt = q_tilde(round_to, c.q, mode).astype(np.float64).reshape(B, Hkv, (Hq // Hkv) * Nq, D)
    s = np.matmul(qt, c.k.astype(np.float64).transpose(0, 1, 3, 2)).reshape(B, Hq, Nq, Nk)
    if c.causal:
        s = np.where(np.arange(Nk)[None, :] > np.arange(Nq)[:, None] + (Nk - Nq), -np.inf, s)
    return s


# ---- the model: the kernels' arithmetic in numpy ---------------------------------------------------------------------------------------------
SABOTAGES = ("combine_first_64", "combine_m_of_split_0", "shared_tile_max", "o_not_rescaled", "l_not_rescaled", "empty_split_weighs_1",
             "last_tile_skipped")


def model(round_to, c, mode, S=None, sabotage=None):
    """(O [B, Hq, Nq, D], LSE [B, Hq, Nq]) as fa_decode_kernel.hip computes them, in fp32: Q~ rounded to the type, fp32 scores, per split
    an online softmax over its 64-key tiles (maximum per row and tile, alpha = 2^(m - m'), l and O rescaled, l adds the fp32
    probabilities, the PV product multiplies them rounded to the type -- f16 with gradual underflow), the merge by maxima with weight 0
    for a split that saw nothing, O rounded to the type. `sabotage`: one of SABOTAGES, the same arithmetic with one thing wrong."""
    assert sabotage is None or sabotage in SABOTAGES
    f32, a = np.float32, ARITH[mode]
    S = c.S if S is None else S
    B, Hq, Nq, D = c.q.shape
    Hkv, Nk = c.k.shape[1], c.k.shape[2]
    G, nT = Hq // Hkv, tiles(Nk)
    R = G * Nq
    qt = q_tilde(round_to, c.q, mode)
    t0, t1 = split_tiles(Nk, S)
    if sabotage == "last_tile_skipped" and nT % S:
        t1 = np.where(t1 - t0 > nT // S, t1 - 1, t1)
    o = np.zeros((B, Hq, Nq, D), f32)
    lse = np.zeros((B, Hq, Nq), f32)
    iq = np.tile(np.arange(Nq), G)
    lim = (iq + Nk - Nq) if c.causal else np.full(R, Nk - 1)
    pad = nT * TILE - Nk
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        for b in range(B):
            for h in range(Hkv):
                qb = qt[b, h * G:(h + 1) * G].reshape(R, D).astype(np.float64)
                sc = (qb @ c.k[b, h].astype(np.float64).T).astype(f32)
                sc = np.where(np.arange(Nk)[None, :] > lim[:, None], f32(-np.inf), sc)
                sc = np.pad(sc, ((0, 0), (0, pad)), constant_values=-np.inf).reshape(R, nT, TILE)
                vt = np.pad(c.v[b, h], ((0, pad), (0, 0))).reshape(nT, TILE, D)
                m = np.full((R, S), -np.inf, f32)
                l = np.zeros((R, S), f32)
                acc = np.zeros((R, S, D), f32)
                for j in range(int((t1 - t0).max())):
                    t = t0 + j
                    act = t < t1
                    tc = np.minimum(t, nT - 1)
                    st = np.where(act[None, :, None], sc[:, tc], f32(-np.inf))
                    mx = st.max(-1)
                    if sabotage == "shared_tile_max":  # (the padding rows of the block hold q = 0: their scores are 0 wherever a key is in range)
                        mx = np.broadcast_to(np.maximum(mx.max(0), np.where(act & (R % 16 != 0), f32(0), f32(-np.inf))), mx.shape)
                    m_new = np.maximum(m, mx)
                    m_use = np.where(np.isneginf(m_new), f32(0), m_new)
                    alpha = np.exp2(m - m_use).astype(f32)
                    p = np.exp2(st - m_use[..., None]).astype(f32)
                    l = ((l if sabotage == "l_not_rescaled" else l * alpha) + p.sum(-1, dtype=f32)).astype(f32)
                    pv = np.matmul(round_to(p, a).reshape(p.shape).transpose(1, 0, 2), vt[tc]).transpose(1, 0, 2).astype(f32)
                    acc = ((acc if sabotage == "o_not_rescaled" else acc * alpha[..., None]) + pv).astype(f32)
                    m = m_new
                ms, ls, oc = m, l, acc
                if sabotage == "combine_first_64":
                    ms, ls, oc = m[:, :64], l[:, :64], acc[:, :64]
                M = ms[:, 0] if sabotage == "combine_m_of_split_0" else ms.max(1)
                w = np.where(np.isneginf(ms), f32(1 if sabotage == "empty_split_weighs_1" else 0), np.exp2(ms - M[:, None])).astype(f32)
                lsum = (ls * w).sum(1, dtype=f32)
                ob = ((oc * w[..., None]).sum(1, dtype=f32) * (f32(1) / lsum)[:, None]).astype(f32)
                o[b, h * G:(h + 1) * G] = round_to(ob, a).reshape(G, Nq, D)
                lse[b, h * G:(h + 1) * G] = ((M + np.log2(lsum).astype(f32)) * f32(LN2)).reshape(G, Nq)
    return o, lse
