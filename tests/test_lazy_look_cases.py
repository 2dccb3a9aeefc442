"""The inputs of tests/test_gpu_lazy_look.py are what they claim, and the kernel's scheme -- the look at the row sums inside the PV
product, the repair one tile later -- holds the bars on them, without a GPU.

Premise: from the fp64 scores of Q~ (util.effective_q) the chosen rows rise by what tests/lazy_look.py says, in the tile it says, and
nothing else does. Scheme: lazy_look.look_model restates the bf16 arithmetic of csrc/fa_mfma16_kernel.hip in numpy with the look's
position and lag (a wave-wide ballot on the sums of the tiles before t, the repair behind tile t from the sums that include it) and
meets the bars the GPU test applies (check(tol_scale=2) against the oracle on Q~). It also says which rows repair, behind which tile,
and which workgroups run again -- asserted here per case.
"""
import numpy as np
import pytest

import lazy_look as ll
from util import LN2, ROWSUM_EPS, TOL_LSE, TOL_O, effective_q

DT = "bf16"
BAR_O, BAR_LSE = 2.0 * TOL_O[DT], 2.0 * TOL_LSE[DT] + ROWSUM_EPS[DT]
NS, DS = (192, 256, 320), (64, 40)


def model(oracle, c, causal):
    s = ll.log2_scores(oracle, c.q, c.k, DT, causal)
    o, lse, info = ll.look_model(s.astype(np.float32), c.v)
    o64, l64 = oracle.attn_fwd_f64(effective_q(oracle, c.q, DT), c.k, c.v, causal, LN2)
    eo, el = np.abs(o - o64).max(-1), np.abs(lse * LN2 - l64)
    assert eo.max() < BAR_O and el.max() < BAR_LSE, (c.name, causal, eo.max(), el.max())
    return s, info


def premise(c, s):
    """Every event's row scores its key at weight.(BIAS + rise) within half a unit; every score that is no event's stays ordinary."""
    rest = np.where(np.isfinite(s), s, 0.0)
    for (b, h, rows, w, key, rise) in c.events:
        rows, w = np.asarray(rows), np.asarray(w, float)
        got = s[b, h, rows, key]
        assert np.isfinite(got).all(), (c.name, "the event is visible to its rows, masked or not")
        assert np.abs(got - w * (ll.BIAS + rise)).max() < 0.5 + 0.01 * rise, (c.name, b, key, got, w * (ll.BIAS + rise))
        rest[b, h, :, key] = 0.0  # (other rows against an event's key: below, with the row's weight 0 they are ordinary too)
        others = np.setdiff1d(np.arange(s.shape[2]), rows)
        assert np.abs(np.where(np.isfinite(s[b, h, others, key]), s[b, h, others, key], 0.0)).max() < 4.0
    assert np.abs(rest).max() < 8.0, (c.name, np.abs(rest).max())


def cases_t(last_offset):
    return [(N, D, t) for N in NS for D in DS for t in range(ll.last_tile(N) + 1 - last_offset)]


@pytest.mark.parametrize("N,D,t", cases_t(0))
def test_one_rise_is_repaired_behind_the_next_tile_or_stays_pending(oracle_mod, N, D, t):
    c = ll.one_rise(oracle_mod.round_to, DT, N, D, t)
    rows, last = ll.wave_rows(N), ll.last_tile(N)
    for causal in (False, True):
        s, info = model(oracle_mod, c, causal)
        premise(c, s)
        r = info["repairs"]
        assert not info["slow"].any() and not info["restarted"][..., 32:].any()
        want = np.zeros_like(r, bool)
        if t < last:  # behind tile t + 1; a rise in the last tile stays pending into the epilogue
            want[0, 0, rows[27], t + 1] = True
            assert abs(r[0, 0, rows[27], t + 1] - ll.RISE) <= 1
            e = r[1, 0, rows, t + 1]
            w = ll.wave_ramp(32)
            # rows of ONE wave: P' = 2^(31 w - 7) -- 2^20 and more from w = 27 / 31 on; different exponents, most rows none
            assert (e[w * (ll.BIAS + ll.RISE) - ll.BIAS >= 20.5] >= 20).all() and (e[w * (ll.BIAS + ll.RISE) - ll.BIAS < 19.5] == 0).all()
            assert len(np.unique(e[e > 0])) >= 3 and (e == 0).sum() >= 20
            want[1, 0, rows, t + 1] = e > 0
        assert np.array_equal(r > 0, want), (c.name, causal, np.argwhere((r > 0) != want)[:5])


@pytest.mark.parametrize("N,D,t", cases_t(1))
def test_rise_then_a_key_out_of_range_poisons_behind_the_look(oracle_mod, N, D, t):
    c = ll.rise_then_out(oracle_mod.round_to, DT, N, D, t)
    rows = ll.wave_rows(N)
    blk = slice(rows[0] // 128 * 128, min(rows[0] // 128 * 128 + 128, N))
    for causal in (False, True):
        s, info = model(oracle_mod, c, causal)
        premise(c, s)
        want = np.zeros(info["slow"].shape, bool)
        want[:, 0, blk] = True  # the rows' workgroup in head 0 of both batch entries, and no other workgroup
        assert np.array_equal(info["slow"], want)
        # the sum left the trusted range while the repair was pending: found by the repair behind tile t + 1, not by the tail test
        assert info["pending_poison"][0, 0, rows[27]] and info["pending_poison"][1, 0, rows[[4, 27]]].all()
        assert info["pending_poison"].sum() == 3 and not (info["repairs"][..., : t + 1] > 0).any()


@pytest.mark.parametrize("N,D,t", cases_t(1))
def test_two_rises_in_consecutive_tiles_take_one_repair(oracle_mod, N, D, t):
    c = ll.two_rises(oracle_mod.round_to, DT, N, D, t)
    rows = ll.wave_rows(N)
    for causal in (False, True):
        s, info = model(oracle_mod, c, causal)
        premise(c, s)
        r = info["repairs"]
        assert not info["slow"].any()
        assert abs(r[0, 0, rows[27], t + 1] - 2 * ll.RISE2) <= 1 and (r[0, 0, rows[27]] > 0).sum() == 1  # 2^60 < POISON: one repair
        assert (r[..., : t + 1] == 0).all() and (r[1, 0, rows, t + 1] > 0).sum() >= 5


@pytest.mark.parametrize("N", [256, 320])
@pytest.mark.parametrize("D", DS)
def test_rise_on_the_diagonal_tile_and_in_a_tile_the_lower_waves_skip(oracle_mod, N, D):
    c = ll.diagonal_and_skipped(oracle_mod.round_to, DT, N, D)
    last = ll.last_tile(N)
    for causal in (False, True):
        s, info = model(oracle_mod, c, causal)
        premise(c, s)
        r, act = info["repairs"], info["active"]
        assert not info["slow"].any()
        if causal:
            assert act[0, 0, 170, 2] and not act[0, 0, 170, 3] and np.isneginf(s[0, 0, 170, 171:192]).all()  # its own diagonal tile, its last
            assert not act[1, 0, 128:192, 3].any() and act[1, 0, 192:256, 3].all()  # waves 0 and 1 of the workgroup skip tile 3
            assert not (r[0] > 0).any()  # pending into the epilogue
            assert not (r[1] > 0).any()  # (tile 3 is the diagonal tile of row 250's wave: pending, too)
        else:
            assert r[0, 0, 170, 3] > 0 and (r[0] > 0).sum() == 1
            assert (r[1] > 0).sum() == (1 if last >= 4 else 0) and (last < 4 or r[1, 0, 250, 4] > 0)
