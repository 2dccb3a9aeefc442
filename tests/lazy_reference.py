"""Inputs whose rows RISE above the reference the bf16 16x16x32 forward kernel holds (test side only; pure numpy, shared by the CPU test
of the cases and the GPU test), and a numpy model of that kernel's lazy arithmetic.

The kernel (csrc/fa_mfma16_kernel.hip, LAZY: bf16 at head_dim 64) forms bf16 probabilities against whatever reference a row has -- an assumed maximum of 0
plus BIAS on the first tile, the first tile's true maximum plus BIAS if a first-tile row sum of the wave vanished -- and looks at the row
sums one tile later: a sum of 2^e.f >= THR is renormalised by 2^-e exactly, a sum at or above POISON (inf, NaN) sends the whole workgroup
through a second, exact run. Construction as in tests/score_range.py: q = alpha*u + noise, k = -beta*u + noise with |u| = 1 puts a score
at about -alpha*beta*scale*log2(e) log2 units; every builder returns a Case of fp32 arrays of exactly representable values plus what
the case claims. tests/test_lazy_reference_cases.py checks the claims from the fp64 scores of Q~ and runs lazy_model() on the cases.
"""
from collections import namedtuple

import numpy as np

from score_range import LOG2E, _noise, _v, log2_scores, product_for, unit  # noqa: F401

BIAS, THR, POISON, FLOOR = 7.0, 2.0 ** 20, 2.0 ** 64, 2.0 ** -64  # csrc/fa_mfma16_kernel.hip, bf16
START, TOP, STEP = -66.0, -6.0, 6.0
# Case.claim: dict of what the case says about itself (checked on the CPU); Case.spikes: [(b, h, row, key)]
Case = namedtuple("Case", "name q k v claim spikes")


def wave_ramp(N):
    """0 ... 1 ... 0 over the rows of every 32-row group (= one wave), up in even groups and down in odd ones."""
    j, g = np.arange(N) % 32, np.arange(N) // 32
    return np.where(g % 2 == 0, j, 31 - j) / 31.0


def stairs(N, phase):
    """Key depths of a full-weight row: the first 64 + phase keys at START (a whole first tile: its sum against the assumed reference
    vanishes and the wave starts over on the true maxima), then STEP up per stair of `width` keys to TOP. width is 64 where N has room
    for ten such stairs (phase 0: every step on a tile border; phase 32: in the middle of a tile); a shorter sequence gets narrower
    stairs, so that its rows still make the whole climb."""
    first = 64 + phase
    width = 64 if N >= first + 640 else max((N - first) // 10, 1)
    j = np.arange(N)
    return np.minimum(START + STEP * np.where(j < first, 0, 1 + (j - first) // width), TOP), width, first


def climb(round_to, dtype, N, D=64, H=2, alpha=8.0, seed=11):
    """(1) batch entry 0 steps on multiples of the stair width, entry 1 half a stair later; row i of every wave carries the weight
    wave_ramp(i): its scores are that fraction of the full climb (weight 0: ordinary scores that never renormalise)."""
    rng, u = np.random.default_rng(seed), unit(D)
    w = wave_ramp(N).astype(np.float32).reshape(1, 1, N, 1)
    q = round_to(np.float32(alpha) * w * u + _noise(rng, (2, H, N, D)), dtype)
    k = np.empty((2, H, N, D), np.float32)
    for b, phase in enumerate((0, 32)):
        d, width, _ = stairs(N, phase)
        beta = (product_for(d, D) / alpha).astype(np.float32).reshape(1, N, 1)
        k[b] = -beta * u + _noise(rng, (H, N, D))
    k = round_to(k, dtype)
    return Case(f"climb N={N} D={D}", q, k, _v(round_to, dtype, rng, k.shape), {"width": width}, [])


def spike(round_to, dtype, Nq, places, D=64, Hq=2, Hkv=None, Nk=None, height=150.0, alpha=8.0, seed=12):
    """(2) ordinary U(-1,1) data; batch entry b has ONE key, places[b] = (row, key), at +height for that one row of query head 0 (key
    head 0): the row is alpha*u + noise, the key +beta*u, every other query is orthogonal to u."""
    rng, u, B = np.random.default_rng(seed), unit(D), len(places)
    Hkv, Nk = Hkv or Hq, Nk or Nq
    q = rng.uniform(-1, 1, (B, Hq, Nq, D)).astype(np.float32)
    q -= (q @ u)[..., None] * u
    k = rng.uniform(-1, 1, (B, Hkv, Nk, D)).astype(np.float32)
    beta = np.float32(product_for(-height, D) / alpha)
    for b, (row, key) in enumerate(places):
        q[b, 0, row] = np.float32(alpha) * u + _noise(rng, (D,))
        k[b, 0, key] = beta * u
    spikes = [(b, 0, row, key) for b, (row, key) in enumerate(places)]
    return Case(f"spike Nq={Nq} Nk={Nk} D={D}", round_to(q, dtype), round_to(k, dtype), _v(round_to, dtype, rng, k.shape), {"height": height}, spikes)


def spike_places(N, rows_per_block=128):
    """(row, key): in a middle tile; in the last tile of the row's workgroup (seen by the test behind the tile loop); on the row's own
    diagonal tile, in the FIRST wave of a workgroup (the diagonal tile is then not the workgroup's last). key <= row: the same inputs
    serve the causal and the full run."""
    last_block = ((N - 1) // rows_per_block) * rows_per_block
    return [(N - 7, (N // 2) // 64 * 64 + 21), (N - 2, N - 3), (last_block + 5, last_block + 5)]


def deep_first_tile(round_to, dtype, N, D=64, H=2, depth=-140.0, alpha=8.0, seed=13):
    """(3) keys 0..63 at `depth` for every row (the first tile starts over on the true maxima), every later key ordinary."""
    rng, u = np.random.default_rng(seed), unit(D)
    q = round_to(np.float32(alpha) * u + _noise(rng, (1, H, N, D)), dtype)
    k = rng.uniform(-1, 1, (1, H, N, D)).astype(np.float32)
    k[:, :, :64] = -np.float32(product_for(depth, D) / alpha) * u + _noise(rng, (1, H, 64, D))
    k = round_to(k, dtype)
    return Case(f"deep first tile N={N} D={D}", q, k, _v(round_to, dtype, rng, k.shape), {"depth": depth}, [])


def non_finite(round_to, dtype, N, D=64, seed=14):
    """(4) ordinary data, causal: the LAST key of head 0 has one +inf element, of head 1 one NaN element, and the last query a positive
    value there -- under the mask only row N - 1 of each head sees its key. Returns the case and k with those elements zeroed."""
    rng = np.random.default_rng(seed)
    q, k, v = (round_to(rng.uniform(-1, 1, (1, 2, N, D)).astype(np.float32), dtype) for _ in range(3))
    q[:, :, N - 1, 5] = 0.5
    clean = k.copy()
    clean[:, :, N - 1, 5] = 0.0
    k[0, 0, N - 1, 5], k[0, 1, N - 1, 5] = np.inf, np.nan
    return Case(f"non-finite N={N} D={D}", q, k, v, {}, [(0, 0, N - 1, N - 1), (0, 1, N - 1, N - 1)]), clean


def to_bf16(x):
    """fp32 -> bf16 -> fp32, round to nearest even; inf stays inf, values past the largest bf16 become inf, NaN stays NaN."""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), np.float32(np.nan), r)


def lazy_model(s, v, rows_per_block=128, thr=THR):
    """The kernel's arithmetic on fp32 scores s [B, H, Nq, Nk] (log2 units, masked entries -inf) and v [B, H, Nk, D]: returns
    (O [.., D] rounded to bf16, LSE in log2 units, info). P' = bf16(exp2(s - m)) in fp32, fp32 row sums of the rounded P', fp32 O.
    First tile: m = BIAS; a 32-row wave with a row sum below FLOOR starts over from the true maxima + BIAS. Later tiles: a row whose sum
    so far is in [thr, POISON) first takes 2^-e; at or above POISON (or NaN) its workgroup is poisoned. Poisoned workgroups are computed
    again in slow mode: in front of every tile m_new = max(m, tile maximum + BIAS), exact rescale. info: per-row count of
    renormalisations, rows that ran in slow mode, waves that started over."""
    s = np.asarray(s, np.float32)
    B, H, N, Nk = s.shape
    v = np.asarray(v, np.float32)
    f32 = np.float32
    wave, block = np.arange(N) // 32, np.arange(N) // rows_per_block
    group_any = lambda x, idx: np.stack([x[..., idx == g].any(-1) for g in range(idx.max() + 1)], -1)[..., idx]  # noqa: E731

    def run(slow):
        m = np.full((B, H, N), BIAS, f32) if not slow else np.full((B, H, N), -np.inf, f32)
        l, o = np.zeros((B, H, N), f32), np.zeros((B, H, N, v.shape[-1]), f32)
        renorms, poisoned, restarted = np.zeros((B, H, N), int), np.zeros((B, H, N), bool), np.zeros((B, H, N), bool)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for t in range(0, Nk, 64):
                st, vt = s[..., t:t + 64], v[:, :, t:t + 64]
                active = group_any(~np.isneginf(st).all(-1), wave)  # (a wave skips the tiles past its diagonal)
                if slow:
                    m_new = np.maximum(m, st.max(-1) + f32(BIAS))
                    a = np.where(np.isneginf(m), f32(0), np.exp2(m - m_new)).astype(f32)  # (first tile: nothing to rescale)
                    l, o, m = l * a, o * a[..., None], m_new
                elif t > 0:
                    bad = active & ~(l < f32(POISON))
                    big = active & ~bad & (l >= f32(thr))
                    e = np.where(big, np.floor(np.log2(np.where(big, l, f32(1)))), 0).astype(f32)
                    l, o, m = l * np.exp2(-e), o * np.exp2(-e)[..., None], m + e
                    renorms += big
                    poisoned |= bad
                p = to_bf16(np.exp2(st - m[..., None]).astype(f32))
                l1, o1 = l + p.sum(-1, dtype=f32), o + np.einsum("bhqk,bhkd->bhqd", p, vt).astype(f32)
                if t == 0 and not slow:
                    again = group_any(l1 < f32(FLOOR), wave)
                    restarted |= again
                    m = np.where(again, st.max(-1) + f32(BIAS), m)
                    p = to_bf16(np.exp2(st - m[..., None]).astype(f32))
                    l1, o1 = np.where(again, p.sum(-1, dtype=f32), l1), np.where(again[..., None], np.einsum("bhqk,bhkd->bhqd", p, vt).astype(f32), o1)
                l, o = l1, o1
            poisoned |= ~(l < f32(POISON))
            out = to_bf16((o / l[..., None]).astype(f32))
            lse = np.log2(l) + m
        return out, lse, renorms, poisoned, restarted

    o, lse, renorms, poisoned, restarted = run(False)
    rerun = group_any(poisoned, block)
    if rerun.any():
        o2, lse2, *_ = run(True)
        o, lse = np.where(rerun[..., None], o2, o), np.where(rerun, lse2, lse)
    return o, lse, {"renorms": renorms, "slow": rerun, "restarted": restarted}
