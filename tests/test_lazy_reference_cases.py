"""The inputs of tests/test_gpu_lazy_reference.py are what they claim, and the lazy reference itself holds the bars -- without a GPU.

Premise: from the fp64 scores of Q~ (util.effective_q), rows rise above the reference the kernel will hold by what tests/lazy_reference.py
says, in the tiles it says. Scheme: lazy_reference.lazy_model restates the bf16 arithmetic of csrc/fa_mfma16_kernel.hip in numpy -- fp32
scores against a stale reference, P' rounded to bf16, fp32 sums of the rounded P', exact 2^-e renormalisation at THR, a second exact run of
a poisoned workgroup -- and meets the bars the GPU test applies (check(tol_scale=2) against the oracle on Q~). That the implementation
follows the scheme is the GPU test's part; that the scheme is within tolerance is shown here.
"""
import numpy as np
import pytest

import lazy_reference as lz
from util import LN2, ROWSUM_EPS, TOL_LSE, TOL_O, effective_q

DT = "bf16"
BAR_O, BAR_LSE = 2.0 * TOL_O[DT], 2.0 * TOL_LSE[DT] + ROWSUM_EPS[DT]


def model_errors(oracle, c, causal, **kw):
    s = lz.log2_scores(oracle, c.q, c.k, DT, causal).astype(np.float32)
    g = c.q.shape[1] // c.k.shape[1]
    o, lse, info = lz.lazy_model(s, np.repeat(c.v, g, 1), **kw)
    o64, l64 = oracle.attn_fwd_ex_f64(effective_q(oracle, c.q, DT), c.k, c.v, causal, LN2)
    return np.abs(o - o64).max(-1), np.abs(lse * LN2 - l64), info


def held_reference(s):
    """The reference a row holds after its first tile (log2 units): BIAS above an assumed maximum of 0, or above the first tile's true
    maximum where a first-tile row sum of its 32-row wave vanished."""
    first = np.exp2(s[..., :64] - lz.BIAS).sum(-1)
    N = s.shape[2]
    wave = np.arange(N) // 32
    again = np.stack([(first < lz.FLOOR)[..., wave == w].any(-1) for w in range(wave.max() + 1)], -1)[..., wave]
    return np.where(again, s[..., :64].max(-1) + lz.BIAS, lz.BIAS), again


@pytest.mark.parametrize("D", [64, 128, 40])
@pytest.mark.parametrize("N", [300, 1100])
def test_climb_renormalises_some_rows_of_every_wave_several_times(oracle_mod, N, D):
    c = lz.climb(oracle_mod.round_to, DT, N, D=D)
    w = lz.wave_ramp(N)
    whole = N // 32 * 32
    for causal in (False, True):
        s = lz.log2_scores(oracle_mod, c.q, c.k, DT, causal)
        at_top = 0
        for b, phase in enumerate((0, 32)):
            d, width, first = lz.stairs(N, phase)
            at_top = max(at_top, first + 10 * width)
            full = s[b][:, w == 1.0]  # the full-weight rows follow the stairs within two units (row-wide shift of the noise)
            vis = np.isfinite(full)
            assert np.abs(full - d)[vis].max() < 2.0, (N, D, causal, b, np.abs(full - d)[vis].max())
            steps = np.flatnonzero(np.diff(d) > 0) + 1
            assert len(steps) == 10 and d[0] == lz.START and d[-1] == lz.TOP
            if N == 1100:  # phase 0: every step on a tile border; phase 32: every step in the middle of a tile
                assert (steps % 64 == (0 if phase == 0 else 32)).all(), (phase, steps)
        ref, again = held_reference(s)
        assert again[..., :whole].all()  # every whole wave holds a full-weight row at -66: its first-tile sum against the assumed reference vanishes
        eo, el, info = model_errors(oracle_mod, c, causal)
        assert np.array_equal(info["restarted"], again)
        r = info["renorms"]
        for g0 in range(0, whole, 32):
            if causal and g0 < at_top:
                continue  # (under the mask the early waves see only the foot of the stairs)
            rg = r[..., g0:g0 + 32].reshape(-1, 32)
            rise = (s.max(-1) - ref)[..., g0:g0 + 32].reshape(-1, 32)
            # the full-weight row ends 60 above the reference it held, the weight-0 row stays under it; in between rows renormalise at
            # different tiles, some more than once, some never
            assert (rise.max(-1) > 50.0).all() and (rise.min(-1) < 0.0).all(), (N, D, causal, g0)
            # (N = 300 makes the climb in under four tiles: one renormalisation takes 2^-40 at once; N = 1100, 6 per tile: two or three)
            need = 2 if N == 1100 else 1
            assert (rg.max(-1) >= need).all() and (rg.min(-1) == 0).all() and all(len(np.unique(x)) > need for x in rg), (N, D, causal, g0, rg[0])
        assert not info["slow"].any()
        assert eo.max() < BAR_O and el.max() < BAR_LSE, (N, D, causal, eo.max(), el.max())
        print(f"climb N={N} D={D} causal={causal}: model max|O err| {eo.max():.2e} max|LSE err| {el.max():.2e}, renormalisations per row up to {r.max()}")


@pytest.mark.parametrize("N", [300, 1100])
def test_spike_poisons_its_workgroup_only(oracle_mod, N):
    c = lz.spike(oracle_mod.round_to, DT, N, lz.spike_places(N))
    for causal in (False, True):
        s = lz.log2_scores(oracle_mod, c.q, c.k, DT, causal)
        for (b, h, row, key) in c.spikes:
            others = np.delete(s[b, h, row], key)
            assert s[b, h, row, key] - others[np.isfinite(others)].max() >= 140.0, (b, row, key)
            rest = np.delete(s[b], row, axis=1) if h == 0 else s[b]
            assert np.abs(np.delete(s[b, h], row, axis=0))[np.isfinite(np.delete(s[b, h], row, axis=0))].max() < 4.0  # every other row: ordinary
            del rest
        eo, el, info = model_errors(oracle_mod, c, causal)
        for (b, h, row, key) in c.spikes:
            blk = slice(row // 128 * 128, row // 128 * 128 + 128)
            assert info["slow"][b, h, blk].all()
        assert info["slow"].sum() == sum(min(128, N - row // 128 * 128) for (_, _, row, _) in c.spikes)  # and no other workgroup
        assert eo.max() < BAR_O and el.max() < BAR_LSE, (N, causal, eo.max(), el.max())
    places = lz.spike_places(N)
    assert places[0][1] // 64 not in (0, (N - 1) // 64) and places[1][1] // 64 == (N - 1) // 64 and places[2][0] == places[2][1] and places[2][0] % 128 < 32


def test_spike_through_grouped_heads_on_a_rectangle(oracle_mod):
    c = lz.spike(oracle_mod.round_to, DT, 200, [(150, 170), (199, 298)], Hq=8, Hkv=2, Nk=300)
    s = lz.log2_scores(oracle_mod, c.q, c.k, DT, True)
    for (b, h, row, key) in c.spikes:
        assert np.isfinite(s[b, h, row, key]) and s[b, h, row, key] - np.delete(s[b, h, row], key)[np.isfinite(np.delete(s[b, h, row], key))].max() >= 140.0
    eo, el, info = model_errors(oracle_mod, c, True)
    assert info["slow"].any() and eo.max() < BAR_O and el.max() < BAR_LSE, (eo.max(), el.max())


@pytest.mark.parametrize("N", [300, 1100])
def test_deep_first_tile_then_ordinary_keys(oracle_mod, N):
    c = lz.deep_first_tile(oracle_mod.round_to, DT, N)
    for causal in (False, True):
        s = lz.log2_scores(oracle_mod, c.q, c.k, DT, causal)
        assert s[..., :64].max() < -130.0 and np.abs(s[..., 64:][np.isfinite(s[..., 64:])]).max() < 6.0
        ref, again = held_reference(s)
        assert again.all()  # the first tile starts over on the true maxima ...
        rise = s[..., 64:, :].max(-1) - ref[..., 64:]
        assert rise.min() > 120.0  # ... and the next tile stands more than 120 log2 units above that reference: inf, poison, second run
        eo, el, info = model_errors(oracle_mod, c, causal)
        assert info["restarted"].all() and info["slow"].all()
        assert eo.max() < BAR_O and el.max() < BAR_LSE, (N, causal, eo.max(), el.max())


def test_ordinary_data_never_leaves_the_common_path_and_a_low_threshold_changes_nothing_beyond_rounding(oracle_mod):
    from util import make_qkv

    q, k, v = make_qkv(oracle_mod, 1, 2, 300, 64, DT)
    c = lz.Case("ordinary", q, k, v, {}, [])
    eo, el, info = model_errors(oracle_mod, c, True)
    assert info["renorms"].sum() == 0 and not info["slow"].any() and not info["restarted"][..., 32:].any()
    assert eo.max() < BAR_O and el.max() < BAR_LSE
    eo2, el2, info2 = model_errors(oracle_mod, c, True, thr=2.0 ** -3)  # every row renormalises: exact powers of two, same bars
    assert info2["renorms"].sum() > 0 and eo2.max() < BAR_O and el2.max() < BAR_LSE


def test_non_finite_case_touches_one_row_per_head(oracle_mod):
    c, clean = lz.non_finite(oracle_mod.round_to, DT, 300)
    s = lz.log2_scores(oracle_mod, c.q, c.k, DT, True)
    bad = ~np.isfinite(s) & ~np.isneginf(s)
    assert bad[0, 0].sum() == 1 and bad[0, 0, 299, 299] and s[0, 0, 299, 299] == np.inf
    assert bad[0, 1].sum() == 1 and np.isnan(s[0, 1, 299, 299])
    assert np.array_equal(np.isfinite(clean), np.ones_like(clean, bool))
