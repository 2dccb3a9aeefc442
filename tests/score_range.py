"""Inputs whose scores sit far below zero (test side only; pure numpy, so the CPU test of the cases and the GPU test share them).

Construction as in test_strongly_negative_scores_from_the_first_tile_on: q = alpha*u + noise, k = -beta*u + noise with |u| = 1, so a
score is about -alpha*beta*scale*log2(e) log2 units ("depth"; the kernels work in log2 units on Q~ = round(scale*log2(e)*Q)).
Every builder takes the oracle's round_to and returns a Case: q, k, v (fp32 arrays of exactly representable values) plus what the
case claims -- `window`: bool [B, Hq, Nq], the rows meant to sit at a depth; `depth`: float [B], the depth of batch entry b's window
rows; `span`: (below, above), the whole-row maximum of a window row lies in [depth - below, depth + above].
tests/test_score_range_cases.py checks those claims from the fp64 scores; tests/test_gpu_score_range.py runs the kernels on them.
"""
from collections import namedtuple

import numpy as np

LOG2E = 1.4426950408889634
Case = namedtuple("Case", "name q k v window depth span")


def unit(D, seed=77):
    u = np.random.default_rng(seed).standard_normal(D).astype(np.float32)
    return u / np.sqrt((u ** 2).sum())


def product_for(depth, D):
    """alpha*beta that puts a score at `depth` log2 units (depth < 0) for head dim D and the default scale."""
    return -np.asarray(depth, np.float64) * np.sqrt(D) / LOG2E


def log2_scores(oracle, q, k, dtype, causal):
    """fp64 scores of Q~ (util.effective_q) in log2 units, [B, Hq, Nq, Nk], masked entries -inf (bottom-right aligned mask)."""
    from util import effective_q

    g = q.shape[1] // k.shape[1]
    s = np.einsum("bhqd,bhkd->bhqk", effective_q(oracle, q, dtype).astype(np.float64), np.repeat(k, g, 1).astype(np.float64))
    if causal:
        nq, nk = s.shape[-2:]
        s = np.where(np.arange(nk)[None, :] > np.arange(nq)[:, None] + (nk - nq), -np.inf, s)
    return s


def _v(round_to, dtype, rng, shape):
    return round_to(rng.uniform(-1, 1, shape).astype(np.float32), dtype)


def _noise(rng, shape, sigma=0.05):
    return sigma * rng.standard_normal(shape).astype(np.float32)


def uniform(round_to, dtype, N, depths, D=64, H=3, alpha=2.0, seed=1):
    """(a), (h): batch entry b has every row at depths[b]."""
    rng, u, B = np.random.default_rng(seed), unit(D), len(depths)
    beta = (product_for(depths, D) / alpha).astype(np.float32).reshape(B, 1, 1, 1)
    q = round_to(alpha * u + _noise(rng, (B, H, N, D)), dtype)
    k = round_to(-beta * u + _noise(rng, (B, H, N, D)), dtype)
    sd = 0.05 * LOG2E / np.sqrt(D) * float(beta.max())  # the row-wide shift -beta * (u . noise_q), log2 units
    return Case(f"uniform N={N}", q, k, _v(round_to, dtype, rng, k.shape), np.ones((B, H, N), bool), np.asarray(depths, float), (5 * sd + 0.2, 5 * sd + 0.2))


def ramp_depths(N, deepest):
    """Row i of every 32 rows: from 0 down to `deepest` in even groups, back up in odd ones."""
    j, g = np.arange(N) % 32, np.arange(N) // 32
    return deepest * np.where(g % 2 == 0, j, 31 - j) / 31.0


def ramp(round_to, dtype, N, deepest, D=64, B=1, H=3, beta=20.0, seed=2):
    """(b): every 32-row group (= one wave of the 16x16x32 kernel) holds rows from depth 0 to `deepest`. beta is small and the ramp is
    in alpha so that the row-wide shift of a depth, beta * (u . noise_q), stays near 0.2 log2 units: no row strays a whole unit."""
    rng, u = np.random.default_rng(seed), unit(D)
    d = ramp_depths(N, deepest)
    alpha = (product_for(d, D) / beta).astype(np.float32).reshape(1, 1, N, 1)
    q = round_to(alpha * u + _noise(rng, (B, H, N, D)), dtype)
    k = round_to(-np.float32(beta) * u + _noise(rng, (B, H, N, D)), dtype)
    window = np.broadcast_to((d <= -11) & (d >= -21), (B, H, N)).copy()
    return Case(f"ramp to {deepest} N={N} D={D}", q, k, _v(round_to, dtype, rng, k.shape), window, np.full(B, float(deepest)), None)


def some_rows(round_to, dtype, Nq, cases, D=64, Hq=2, Hkv=None, Nk=None, alpha=2.0, seed=3):
    """(c), (e): ordinary U(-1,1) data except the query rows cases[b] = (depth, rows) of batch entry b. Every key carries -beta*u, the
    ordinary queries are orthogonal to u (their scores stay ordinary), the placed rows are alpha*u + noise."""
    rng, u, B = np.random.default_rng(seed), unit(D), len(cases)
    Hkv, Nk = Hkv or Hq, Nk or Nq
    depths = np.array([c[0] for c in cases], float)
    beta = (product_for(depths, D) / alpha).astype(np.float32).reshape(B, 1, 1, 1)
    q = rng.uniform(-1, 1, (B, Hq, Nq, D)).astype(np.float32)
    q -= (q @ u)[..., None] * u
    window = np.zeros((B, Hq, Nq), bool)
    for b, (_, rows) in enumerate(cases):
        rows = np.asarray(rows)
        window[b, :, rows] = True
        q[b, :, rows] = alpha * u + _noise(rng, (len(rows), Hq, D))
    k = round_to(-beta * u + rng.uniform(-1, 1, (B, Hkv, Nk, D)).astype(np.float32), dtype)
    # a placed row's scores spread by alpha * (u . U(-1,1)^D): 0.21 log2 units at alpha = 2, D = 64
    return Case(f"rows Nq={Nq} Nk={Nk}", round_to(q, dtype), k, _v(round_to, dtype, rng, k.shape), window, depths, (2.0, 2.0))


def identical_keys(round_to, dtype, N, depths, first_only, D=64, H=3, alpha=2.0, seed=4):
    """(d): the first 64 keys (or all) are one and the same vector -beta*u: every P' of a row rounds the same way."""
    c = uniform(round_to, dtype, N, depths, D, H, alpha, seed)
    B = len(depths)
    beta = (product_for(depths, D) / alpha).astype(np.float32).reshape(B, 1, 1, 1)
    same = round_to(np.broadcast_to(-beta * unit(D), c.k.shape), dtype)
    k = c.k.copy()
    k[:, :, :64 if first_only else N] = same[:, :, :64 if first_only else N]
    return c._replace(name=f"identical keys ({'first 64' if first_only else 'all'}) N={N}", k=k)


def first_tile(round_to, dtype, N, depths, rest, D=64, H=3, alpha=2.0, seed=5):
    """(f): keys 0..63 at depths[b]; the later keys `rest`: 'ordinary' (U(-1,1): scores near 0), 'climb' (every 64 keys 2 log2 units
    higher than the 64 before, never above -3), 'lower' (10 log2 units below the first 64), 'tail' (8 below the first 64, and the first 64
    shallow: a first tile that is NOT started over, followed by a thousand keys whose P' against the assumed reference are subnormal)."""
    rng, u, B = np.random.default_rng(seed), unit(D), len(depths)
    q = round_to(alpha * u + _noise(rng, (B, H, N, D)), dtype)
    tile_no = (np.arange(N) // 64).astype(np.float64)
    step = {"ordinary": 0.0, "climb": 2.0, "lower": 0.0, "tail": 0.0}[rest]
    d = np.asarray(depths, float)[:, None] + step * tile_no[None, :] - {"lower": 10.0, "tail": 8.0}.get(rest, 0.0) * (tile_no > 0)
    assert d.max() <= -2.0
    beta = (product_for(d, D) / alpha).astype(np.float32).reshape(B, 1, N, 1)
    k = -beta * u + _noise(rng, (B, H, N, D))
    if rest == "ordinary":
        k[:, :, 64:] = rng.uniform(-1, 1, (B, H, N - 64, D)).astype(np.float32)
    sd = 0.05 * LOG2E / np.sqrt(D) * float(beta.max())
    # `depth` is that of the first 64 keys; only with rest 'lower' is it the whole-row maximum too (`span`)
    return Case(f"first tile, rest {rest} N={N}", q, round_to(k, dtype), _v(round_to, dtype, rng, k.shape), np.ones((B, H, N), bool),
                np.asarray(depths, float), (5 * sd + 0.2, 5 * sd + 0.2) if rest in ("lower", "tail") else None)


# ---- the cases of tests/test_gpu_score_range.py, by kind: name -> (builder(round_to, dtype) -> [Case], causal settings) ---------------
DEPTHS_A = list(range(-6, -31, -1))
DEPTHS_C = (-12, -15, -18, -21)
DEPTHS_D = (-8, -10, -11, -12, -13, -15, -18, -21)
DEPTHS_F = (-13, -17, -20)
DEPTHS_TAIL = (-2, -3, -4, -5, -6, -7, -8, -9, -10)
DEPTHS_H = list(range(-55, -77, -2))
ROWS_C = (0, 17, 31, 32, 127, 128, 299)
ROWS_E = (0, 1, 2, 3, 128, 129, 130, 131)
BOTH, CAUSAL = (False, True), (True,)
KINDS = {
    "a": (lambda r, t: [uniform(r, t, N, DEPTHS_A) for N in (64, 300, 1100)], BOTH),
    "b1": (lambda r, t: [ramp(r, t, N, -20.0) for N in (64, 300, 1100)], BOTH),
    "b2": (lambda r, t: [ramp(r, t, N, -30.0) for N in (64, 300, 1100)], BOTH),
    "c": (lambda r, t: [some_rows(r, t, 300, [(d, [row]) for d in DEPTHS_C for row in ROWS_C])], BOTH),
    "d": (lambda r, t: [identical_keys(r, t, N, DEPTHS_D, first) for N in (64, 300) for first in (True, False)], BOTH),
    "e": (lambda r, t: [some_rows(r, t, 300, [(d, ROWS_E) for d in DEPTHS_C], seed=6)], CAUSAL),
    "f-i": (lambda r, t: [first_tile(r, t, 300, DEPTHS_F, "ordinary")], BOTH),
    "f-ii": (lambda r, t: [first_tile(r, t, 300, DEPTHS_F, "climb")], BOTH),
    "f-iii": (lambda r, t: [first_tile(r, t, 300, DEPTHS_F, "lower")], BOTH),
    "f-iv": (lambda r, t: [first_tile(r, t, 1100, DEPTHS_TAIL, "tail")], BOTH),
    "g-D128": (lambda r, t: [ramp(r, t, 300, -20.0, D=128)], BOTH),
    "g-D40": (lambda r, t: [ramp(r, t, 300, -20.0, D=40)], BOTH),
    "g-D104": (lambda r, t: [ramp(r, t, 300, -20.0, D=104)], BOTH),
    "h": (lambda r, t: [uniform(r, t, N, DEPTHS_H, alpha=4.0) for N in (64, 300)] + [ramp(r, t, 300, -75.0)], BOTH),
}
# (e) through fa_fwd_ex: 200 queries on 300 keys (bottom-right aligned mask), 8 query heads on 2 key heads
E_EX = lambda r, t: some_rows(r, t, 200, [(d, ROWS_E) for d in DEPTHS_C], Hq=8, Hkv=2, Nk=300, seed=7)  # noqa: E731
