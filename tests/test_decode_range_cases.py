"""The inputs of tests/test_gpu_decode_range.py are what they claim, the decode kernels' arithmetic holds that test's bars on them, and
the same arithmetic with one thing wrong does not -- shown without a GPU, on the values rounded to each type the GPU test uses.

(a) claims: from the fp64 scores of Q~, every row's maximum is at the key / in the split / at the depth tests/decode_range.py says.
(b) decode_range.model() restates fa_decode_kernel.hip in numpy (fp32 sums, P rounded to the type, the merge by maxima) at the split
    count the case asserts -- and, for the paged regime, at S = 256 on 1100 keys, where 238 of the 256 splits are empty. It holds the bars.
(c) each sabotage of SABOTAGES misses a bar on the case named in SHARP. One cannot: a split that saw no visible key has l = 0 and O = 0
    exactly, so the weight it is merged with -- 0 or 1 -- never reaches the result; test_the_weight_of_an_empty_split_is_inert pins
    that instead (the kernel's guard is about inf - inf for a row that no split saw, which the `lsum > 0` test of the paged combine
    catches either way).
"""
import numpy as np
import pytest

import decode_range as dr
from util import LN2

DTYPES = ("f16", "bf16", "fp8")  # the values; "fp8" serves the modes fp8 and kv8 (same Q~: e4m3 queries are widened to bf16)


def worst(oracle, c, mode, o, lse):
    """(worst |O err| / bar, worst |LSE err| / bar) against the fp64 oracle on Q~; inf where something is not finite."""
    o64, l64 = oracle.attn_fwd_ex_f64(dr.q_tilde(oracle.round_to, c.q, mode), c.k, c.v, c.causal, LN2)
    bar_o, bar_l = dr.bars(mode, l64)
    if not (np.isfinite(o).all() and np.isfinite(lse).all()):
        return np.inf, np.inf
    return float(np.abs(o - o64).max() / bar_o), float((np.abs(lse - l64) / bar_l).max())


def claims_hold(oracle, family, c, dtype):
    B, Hq, Nq, D = c.q.shape
    Nk = c.k.shape[2]
    assert c.S == min(max(1, dr.tiles(Nk) // 4), 256), c.name  # the rule where nT / 4 or the cap binds
    assert (Nk * D % 16 == 0) != ((family, c.name) in dr.E4M3_LEFT_OUT), c.name
    keys = np.unique(np.concatenate([np.arange(0, Nk, 17), np.arange(max(0, Nk - 130), Nk)]))  # (every builder ends in round_to: a sample of K, V)
    for x in (c.q, c.k[:, :, keys], c.v[:, :, keys]):
        assert np.array_equal(oracle.round_to(x, dtype), x), c.name
    if not ((c.top_key != -1).any() or (c.top_split != -1).any() or (~np.isnan(c.depth)).any()):
        return  # ordinary data claims its shape and split count only
    s = dr.scores(oracle.round_to, c, dtype)
    top, arg = s.max(-1), s.argmax(-1)
    claimed = c.top_key >= 0
    assert np.array_equal(arg[claimed], c.top_key[claimed]), (c.name, np.argwhere(claimed & (arg != c.top_key))[:4])
    masked = c.top_key == -2
    if masked.any():  # rows of a head whose spike they cannot see stay a log2 unit below what the rows that see it reach
        spike = np.where(claimed, top, np.inf).min(-1, keepdims=True)
        assert (top < spike - 1.0)[masked].all() and np.isfinite(spike[masked.any(-1)]).all(), c.name
    if family == "K":  # every spike scores close to its c (e4m3 keys: 3 mantissa bits)
        assert (top[claimed] > 0.8 * dr.SPIKES[0] * D ** -0.5 * dr.LOG2E).all(), c.name
    claimed = c.top_split >= 0
    assert np.array_equal(dr.split_of_key(Nk, c.S)[arg][claimed], c.top_split[claimed]), c.name
    claimed = ~np.isnan(c.depth)
    dev = np.abs(top - c.depth)[claimed]
    assert (dev <= dr.span(c.depth[claimed])).all(), (c.name, dev.max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family", list(dr.FAMILIES))
def test_claims_hold_and_the_model_holds_the_bars(oracle_mod, family, dtype):
    """(a) and (b), case by case (a case is built once)."""
    for build in dr.FAMILIES[family]:
        c = build(oracle_mod.round_to, dtype)
        claims_hold(oracle_mod, family, c, dtype)
        ro, rl = worst(oracle_mod, c, dtype, *dr.model(oracle_mod.round_to, c, dtype))
        print(f"{family} {c.name} {dtype} S={c.S}: model worst O err / bar {ro:.3f} LSE err / bar {rl:.3f}")
        assert ro < 1.0 and rl < 1.0, (c.name, ro, rl)


def test_split_staircases_reach_the_far_end_and_every_lane_boundary(oracle_mod):
    up = [b(oracle_mod.round_to, "bf16") for b in dr.FAMILIES["S"] if b.label.endswith("-up")]
    assert {c.S for c in up} == {65, 256}
    for c in up:
        s = dr.scores(oracle_mod.round_to, c, "bf16")
        first = s[..., :dr.TILE * 4].max(-1) - s.max(-1)  # split 0 against the row maximum
        assert (first < -185.0).all(), (c.name, first.max())
    at = sorted(int(b.label.split("-")[-3]) for b in dr.FAMILIES["S"] if "-65536-" in b.label and "-one-" in b.label)
    assert at == list(dr.DOMINANT_AT), at
    c = dr.tile_climb(oracle_mod.round_to, "f16", 64, -40.0, 2.0)  # scores() is score_range.log2_scores
    assert np.array_equal(dr.scores(oracle_mod.round_to, c, "f16"), dr.log2_scores(oracle_mod, c.q, c.k, "f16", c.causal))


def test_many_split_shapes_cover_every_lane_slot_and_the_uneven_partition():
    assert sorted(set(dr.S_OF_NK.values())) == [4, 65, 78, 129, 193, 256]
    assert 78 % 8 == 6  # the combine's tail loop
    t0, t1 = dr.split_tiles(70001, 256)
    assert dr.tiles(70001) == 1094 and set((t1 - t0).tolist()) == {4, 5} and 70001 % 64 != 0
    t0, t1 = dr.split_tiles(65536, 256)
    assert set((t1 - t0).tolist()) == {4}


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_holds_the_bars_where_most_splits_are_empty(oracle_mod, dtype):
    # the paged regime: S from a capacity of 65536 keys, tiles from 1100 (and 37) keys
    mode = dtype
    for c in (dr.ordinary(oracle_mod.round_to, dtype, 8, 2, 4, 1100, 64), dr.row_ramp(oracle_mod.round_to, dtype, 16, 2, 4, 1100, 128, -200.0)):
        for S in (256, 128):
            ro, rl = worst(oracle_mod, c, mode, *dr.model(oracle_mod.round_to, c, mode, S=S))
            assert ro < 1.0 and rl < 1.0, (c.name, S, ro, rl)


# sabotage -> (builder, dtype, what misses): the cases on which the wrong arithmetic misses a bar
SHARP = {
    "combine_first_64": [(lambda r, t: dr.split_levels(r, t, 65536, 64, "one", at=64, Hq=16, Nq=4), "bf16", "o"),
                         (lambda r, t: dr.ordinary(r, t, 8, 2, 1, 16704, 64), "bf16", "lse")],
    "combine_m_of_split_0": [(lambda r, t: dr.split_levels(r, t, 16704, 64, "up"), "bf16", "o"),
                             (lambda r, t: dr.split_levels(r, t, 65536, 128, "up"), "f16", "o")],
    "shared_tile_max": [(lambda r, t: dr.row_ramp(r, t, 16, 2, 4, 1100, 64, -200.0), "bf16", "o"),
                        (lambda r, t: dr.row_ramp(r, t, 32, 1, 1, 1100, 64, -30.0), "f16", "o")],
    "o_not_rescaled": [(lambda r, t: dr.tile_climb(r, t, 64, -40.0, 2.0), "bf16", "o"), (lambda r, t: dr.tile_climb(r, t, 128, -204.0, 12.0), "f16", "o")],
    "l_not_rescaled": [(lambda r, t: dr.tile_climb(r, t, 64, -40.0, 2.0), "bf16", "lse")],
    "last_tile_skipped": [(lambda r, t: dr.ordinary(r, t, 8, 2, 1, 70001, 64), "bf16", "lse"), (lambda r, t: dr.ordinary(r, t, 8, 2, 1, 20000, 128), "f16", "lse")],
}


@pytest.mark.parametrize("sabotage", list(SHARP))
def test_each_sabotage_misses_a_bar_on_a_named_case(oracle_mod, sabotage):
    for build, dtype, what in SHARP[sabotage]:
        c = build(oracle_mod.round_to, dtype)
        ro, rl = worst(oracle_mod, c, dtype, *dr.model(oracle_mod.round_to, c, dtype))
        assert ro < 1.0 and rl < 1.0, (c.name, ro, rl)
        so, sl = worst(oracle_mod, c, dtype, *dr.model(oracle_mod.round_to, c, dtype, sabotage=sabotage))
        print(f"{sabotage} on {c.name} {dtype}: O err / bar {so:.3g} (sound {ro:.3f}) LSE err / bar {sl:.3g} (sound {rl:.3f})")
        assert (so if what == "o" else sl) >= 1.0, (sabotage, c.name, dtype, so, sl)


def test_the_weight_of_an_empty_split_is_inert(oracle_mod):
    """A split that saw no visible key leaves m = -inf, l = 0 and O = 0: merged with weight 1 instead of 0 it adds exact zeros. The
    results are the same bit for bit -- this sabotage of the list cannot miss a bar, on any input."""
    assert set(dr.SABOTAGES) == set(SHARP) | {"empty_split_weighs_1"}
    for c in (dr.ordinary(oracle_mod.round_to, "bf16", 8, 2, 4, 1100, 64), dr.causal_spikes(oracle_mod.round_to, "f16", 1100, 64)):
        a = dr.model(oracle_mod.round_to, c, "bf16", S=256)
        b = dr.model(oracle_mod.round_to, c, "bf16", S=256, sabotage="empty_split_weighs_1")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
