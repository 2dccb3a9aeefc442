"""Inputs for the POSITION of the look at the row sums in the bf16 16x16x32 forward kernel (test side only; pure numpy, shared by the CPU
test of the cases and the GPU test), and a numpy model of the kernel's arithmetic with that position and its lag.

The kernel (csrc/fa_mfma16_kernel.hip, LAZY with FA16_LOOK = 1) looks at the row sums of the tiles BEFORE tile t inside tile t's PV
product -- one ballot per 32-row wave: "some row of mine has summed to THR or more" -- and acts on a non-zero ballot behind that
product's last MFMA, from the sums as they stand then (tile t included): a row in [THR, POISON) takes its exact power of two, a row at or
above POISON (inf, NaN) poisons the workgroup, which runs again in slow mode. The first tile has no look; the sums behind the last tile
are tested against POISON only. So a rise in tile t is repaired behind tile t + 1, one tile later than with the look in front of the
tile, and a rise in the last tile a wave visits stays pending into the epilogue (LSE = reference + log2(sum): consistent either way).

Construction as in tests/lazy_reference.py (spike): ordinary U(-1,1) data whose queries are orthogonal to a unit vector u; the chosen
rows get w.alpha.u on top, the chosen keys ARE beta.u, so that row's score against that key is w.height log2 units and every other score
stays ordinary. A height is given as the RISE above the reference a row holds from its first tile (BIAS above an assumed maximum of 0):
a rise of r makes P' = 2^r.
"""
from collections import namedtuple

import numpy as np

from lazy_reference import BIAS, FLOOR, POISON, THR, to_bf16, wave_ramp
from score_range import _v, log2_scores, product_for, unit  # noqa: F401

RISE, RISE2, OUT = 24.0, 30.0, 150.0  # P' = 2^24: repaired; two of 2^30: legal with either lag; 150 above a rise: out of fp32's range
ALPHA = 8.0
# Case.events: [(b, h, rows, weights, key, rise)]
Case = namedtuple("Case", "name q k v events")


def last_tile(N):
    return (N - 1) // 64


def build(round_to, dtype, shape, events, seed=31, name=""):
    """shape = (B, H, N, D); events = [(b, h, rows, weights, key, rise)]: query rows `rows` of head (b, h) carry weights.ALPHA.u, key
    `key` of that head is beta.u with ALPHA.beta.scale.log2(e) = BIAS + rise (weight 1: P' = 2^rise against the assumed reference)."""
    B, H, N, D = shape
    rng, u = np.random.default_rng(seed), unit(D)
    q = rng.uniform(-1, 1, shape).astype(np.float32)
    k = rng.uniform(-1, 1, shape).astype(np.float32)
    heads = {(b, h) for (b, h, *_) in events}
    for (b, h) in heads:
        q[b, h] -= (q[b, h] @ u)[..., None] * u
    done = set()
    for (b, h, rows, weights, key, rise) in events:
        rows, weights = np.asarray(rows), np.asarray(weights, np.float32)
        new = [r for r in rows.tolist() if (b, h, r) not in done]
        if new:  # (a row named by two events keeps one weight)
            sel = np.isin(rows, new)
            q[b, h, rows[sel]] += (np.float32(ALPHA) * weights[sel])[:, None] * u
            done |= {(b, h, r) for r in new}
        k[b, h, key] = np.float32(product_for(-(BIAS + rise), D) / ALPHA) * u
    return Case(name, round_to(q, dtype), round_to(k, dtype), _v(round_to, dtype, rng, shape), list(events))


def wave_rows(N):
    """The last wave of the last 128-row workgroup that is whole: it sees every tile under the mask."""
    top = N // 32 * 32
    return np.arange(top - 32, top)


def one_rise(round_to, dtype, N, D, t, B=2, H=2):
    """(1) a rise of RISE at tile t, in head 0: batch entry 0 in ONE row of a wave, entry 1 in all 32 rows of a wave on wave_ramp weights
    (the rows of one wave repair by different exponents, or not at all). Head 1: ordinary."""
    rows = wave_rows(N)
    key = 64 * t + 3
    ev = [(0, 0, rows[[27]], [1.0], key, RISE), (1, 0, rows, wave_ramp(32), key, RISE)]
    return build(round_to, dtype, (B, H, N, D), ev, name=f"one rise N={N} D={D} t={t}")


def rise_then_out(round_to, dtype, N, D, t, B=2, H=2):
    """(2) the rise of (1) at tile t and, in tile t + 1, a key OUT units higher in the same row(s): the sum leaves the trusted range
    while a repair is pending."""
    rows = wave_rows(N)
    k1, k2 = 64 * t + 3, 64 * (t + 1) + 5
    ev = [(0, 0, rows[[27]], [1.0], k1, RISE), (0, 0, rows[[27]], [1.0], k2, RISE + OUT),
          (1, 0, rows[[4, 27]], [1.0, 1.0], k1, RISE), (1, 0, rows[[4, 27]], [1.0, 1.0], k2, RISE + OUT)]
    return build(round_to, dtype, (B, H, N, D), ev, name=f"rise then out N={N} D={D} t={t}")


def two_rises(round_to, dtype, N, D, t, B=2, H=2):
    """(3) a rise of RISE2 at tile t and RISE2 more at tile t + 1 (one row in entry 0, a ramp in entry 1)."""
    rows = wave_rows(N)
    k1, k2 = 64 * t + 3, 64 * (t + 1) + 5
    w = wave_ramp(32)
    ev = [(0, 0, rows[[27]], [1.0], k1, RISE2), (0, 0, rows[[27]], [1.0], k2, 2 * RISE2),
          (1, 0, rows, w, k1, RISE2), (1, 0, rows, w, k2, 2 * RISE2)]
    return build(round_to, dtype, (B, H, N, D), ev, name=f"two rises N={N} D={D} t={t}")


def diagonal_and_skipped(round_to, dtype, N, D, B=2, H=2):
    """(4) entry 0: the rise on the wave's OWN diagonal tile, under the mask (row 170 of wave 1 of workgroup 1, key 165 in tile 2).
    Entry 1: the rise in a tile that the lower waves of the workgroup skip under the mask (row 250, wave 3 of workgroup 1; key 200 in
    tile 3, which waves 0 and 1 -- rows 128 ... 191 -- never visit). N >= 256."""
    ev = [(0, 0, [170], [1.0], 165, RISE), (1, 0, [250], [1.0], 200, RISE)]
    return build(round_to, dtype, (B, H, N, D), ev, name=f"diagonal / skipped N={N} D={D}")


def look_model(s, v, rows_per_block=128, thr=THR):
    """The kernel's arithmetic with the look inside the PV product, on fp32 scores s [B, H, Nq, Nk] (log2 units, masked entries -inf)
    and v [B, H, Nk, D]: returns (O rounded to bf16, LSE in log2 units, info). P' = bf16(exp2(s - m)) in fp32, fp32 row sums of the
    rounded P', fp32 O. First tile: m = BIAS, no look; a 32-row wave with a row sum below FLOOR starts over from the true maxima + BIAS.
    Tile t > 0: the wave's ballot is taken on the sums of the tiles before t; tile t is added; in a wave whose ballot was non-zero every
    row whose sum NOW is in [thr, POISON) takes 2^-e, and a row at or above POISON (or NaN) poisons its workgroup. Behind the last tile:
    POISON only. Poisoned workgroups are computed again in slow mode (true maxima in front of every tile).
    info: repairs [B, H, N, T] (the exponent taken behind tile t, 0 = none), pending_poison (rows poisoned by a repair, i.e. behind a
    look), slow (rows of workgroups that ran again), active [B, H, N, T] (the wave visits the tile), restarted."""
    s, v, f32 = np.asarray(s, np.float32), np.asarray(v, np.float32), np.float32
    B, H, N, Nk = s.shape
    T = (Nk + 63) // 64
    wave, block = np.arange(N) // 32, np.arange(N) // rows_per_block
    group_any = lambda x, idx: np.stack([x[..., idx == g].any(-1) for g in range(idx.max() + 1)], -1)[..., idx]  # noqa: E731

    def run(slow):
        m = np.full((B, H, N), -np.inf if slow else BIAS, f32)
        l, o = np.zeros((B, H, N), f32), np.zeros((B, H, N, v.shape[-1]), f32)
        repairs, active_at = np.zeros((B, H, N, T), int), np.zeros((B, H, N, T), bool)
        poisoned, pending, restarted = np.zeros((B, H, N), bool), np.zeros((B, H, N), bool), np.zeros((B, H, N), bool)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for ti, t in enumerate(range(0, Nk, 64)):
                st, vt = s[..., t:t + 64], v[:, :, t:t + 64]
                active = group_any(~np.isneginf(st).all(-1), wave)  # (a wave skips the tiles past its diagonal)
                active_at[..., ti] = active
                ballot = np.zeros((B, H, N), bool)
                if slow:
                    m_new = np.maximum(m, st.max(-1) + f32(BIAS))
                    a = np.where(np.isneginf(m), f32(0), np.exp2(m - m_new)).astype(f32)
                    l, o, m = l * a, o * a[..., None], m_new
                elif t > 0:
                    ballot = group_any(active & ~(l < f32(thr)), wave) & active
                p = to_bf16(np.exp2(st - m[..., None]).astype(f32))
                l1, o1 = l + p.sum(-1, dtype=f32), o + np.einsum("bhqk,bhkd->bhqd", p, vt).astype(f32)
                if t == 0 and not slow:
                    again = group_any(l1 < f32(FLOOR), wave)
                    restarted |= again
                    m = np.where(again, st.max(-1) + f32(BIAS), m)
                    p = to_bf16(np.exp2(st - m[..., None]).astype(f32))
                    l1, o1 = np.where(again, p.sum(-1, dtype=f32), l1), np.where(again[..., None], np.einsum("bhqk,bhkd->bhqd", p, vt).astype(f32), o1)
                l, o = np.where(active, l1, l), np.where(active[..., None], o1, o)
                bad = ballot & ~(l < f32(POISON))
                big = ballot & ~bad & (l >= f32(thr))
                e = np.where(big, np.floor(np.log2(np.where(big, l, f32(1)))), 0).astype(f32)
                l, o, m = l * np.exp2(-e), o * np.exp2(-e)[..., None], m + e
                repairs[..., ti] = e
                pending |= bad
            poisoned = pending | ~(l < f32(POISON))
            out = to_bf16((o / l[..., None]).astype(f32))
            lse = np.log2(l) + m
        return out, lse, repairs, poisoned, pending, restarted, active_at

    o, lse, repairs, poisoned, pending, restarted, active_at = run(False)
    rerun = group_any(poisoned, block)
    if rerun.any():
        o2, lse2, *_ = run(True)
        o, lse = np.where(rerun[..., None], o2, o), np.where(rerun, lse2, lse)
    return o, lse, {"repairs": repairs, "pending_poison": pending, "slow": rerun, "active": active_at, "restarted": restarted}
