"""The inputs of tests/test_gpu_score_range.py are what they claim, and its f16 cases are sharp -- shown without a GPU.

Premise: from the fp64 scores of Q~, the targeted rows' whole-row maxima lie where tests/score_range.py says.
Sharpness: assumed_reference() below restates in numpy the arithmetic of a 16x16x32 forward kernel whose first tile forms the
probabilities against an ASSUMED row maximum of 0 and starts over only if a first-tile row sum is below `floor` (2^-64: the guard
before the f16 floor of csrc/fa_mfma16_kernel.hip). On the f16 cases of kinds (a), (b1), (d), (e), (f-iii) whose window rows are at -15
or deeper, and of kind (c) at -18 or deeper, it misses the strict f16 bar on O or on LSE, and it holds the bar where every row is above
-9: the GPU tests fail on a kernel with that guard, and not for another reason. (Two exceptions, both the wave-wide ballot at work:
uniform depths below -20 flush some row of nearly every wave completely, which starts the wave over; (c) at -15 spreads 300 keys
over 0.2 log2 units, their roundings average out.) With the f16 floor of the kernel the same arithmetic holds the bar on every case;
with a floor of 2^-7 -- one power of two above where the first tile alone stops missing -- it does not (kind f-iv).
The emulation ASSUMES gradual underflow of P' (subnormal f16 probabilities taken as they are by the matrix core). Measured on MI355X:
that is what the hardware does ("first tile"; profiles/r06/parent_score_range.log follows this model to two digits).
"""
import numpy as np
import pytest

import score_range as sr
from util import LN2, ROWSUM_EPS, TOL_LSE, TOL_O, effective_q

BAR_O, BAR_LSE = 2.0 * TOL_O["f16"], 2.0 * TOL_LSE["f16"] + ROWSUM_EPS["f16"]  # check(tol_scale=2) against the oracle on Q~
F16_FLOOR = 1.0  # FIRST_SUM_FLOOR of csrc/fa_mfma16_kernel.hip for f16


def assumed_reference(oracle, c, causal, floor, bias=3.0):
    """(|O - exact|, |LSE - exact|) per row, [B, H, N], of the f16 16x16x32 kernel's arithmetic in numpy: Q~ rounded to f16, fp32 scores,
    P' = 2^(s - reference) rounded to f16 WITH gradual underflow, row sums over the rounded P', O rounded to f16. The reference of a row is
    bias above an assumed maximum of 0 until some P' of its 32-row wave reaches 2 (then: the true maxima so far + bias). After the first
    64 keys a wave with a row sum below `floor` starts over from the true maxima (the wave-wide ballot)."""
    s = sr.log2_scores(oracle, c.q, c.k, "f16", causal).astype(np.float32).astype(np.float64)
    v = np.repeat(c.v, c.q.shape[1] // c.k.shape[1], 1).astype(np.float64)
    B, H, N, Nk = s.shape
    wave = np.arange(N) // 32
    m = np.full((B, H, N), bias)
    l, o = np.zeros((B, H, N)), np.zeros((B, H, N, v.shape[-1]))
    pad = (-N) % 32
    any_in_wave = lambda x: np.pad(x, ((0, 0), (0, 0), (0, pad))).reshape(B, H, -1, 32).any(-1)[..., wave]  # noqa: E731
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(0, Nk, 64):
            st, vt = s[..., t:t + 64], v[:, :, t:t + 64]
            p = lambda: np.exp2(st - m[..., None]).astype(np.float16).astype(np.float64)  # noqa: E731
            renew = any_in_wave(~(p() < 2.0).all(-1))
            for first_tile_guard in (False, True):
                m_new = np.where(renew, np.maximum(m if t else -np.inf, st.max(-1) + bias), m)
                m_new = np.where(np.isfinite(m_new), m_new, m)  # a row with no visible key in this tile keeps its reference
                l, o, m = l * np.exp2(m - m_new), o * np.exp2(m - m_new)[..., None], m_new
                if first_tile_guard:
                    break
                l1, o1 = l + p().sum(-1), o + p() @ vt
                renew = any_in_wave(l1 < floor) & ~renew if t == 0 else np.zeros_like(renew)
                if not renew.any():
                    break
                l, o = np.where(renew, 0.0, l), np.where(renew[..., None], 0.0, o)
                l1 = o1 = None
            if l1 is None:
                l1, o1 = l + p().sum(-1), o + p() @ vt
            l, o = l1, o1
    o = (o / l[..., None]).astype(np.float16).astype(np.float64)
    lse = (np.log2(l) + m) * LN2
    o64, l64 = oracle.attn_fwd_ex_f64(effective_q(oracle, c.q, "f16"), c.k, c.v, causal, LN2)
    return np.abs(o - o64).max(-1), np.abs(lse - l64)


def _row_max(oracle, c, dtype, causal, keys=None):
    return sr.log2_scores(oracle, c.q, c.k, dtype, causal)[..., :keys].max(-1)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["a", "c", "d", "e", "f-iii", "f-iv", "h"])
def test_window_rows_sit_where_the_case_says(oracle_mod, kind, dtype):
    build, causals = sr.KINDS[kind]
    cases = build(oracle_mod.round_to, dtype) + ([sr.E_EX(oracle_mod.round_to, dtype)] if kind == "e" else [])
    for c in cases:
        if c.span is None:
            continue  # the ramp of (h): next test
        for causal in causals:
            dev = (_row_max(oracle_mod, c, dtype, causal) - c.depth[:, None, None])[c.window]
            assert -c.span[0] <= dev.min() and dev.max() <= c.span[1], (c.name, causal, dev.min(), dev.max())
    if kind == "a":  # alpha = 2, beta = 30 ... 58 (depths -11 ... -21) puts every row's maximum inside [-10, -22]
        inside = [b for b, d in enumerate(cases[1].depth) if -21 <= d <= -11]
        m = _row_max(oracle_mod, cases[1], dtype, False)[inside]
        assert m.max() <= -9.0 and m.min() >= -24.0, (m.min(), m.max())  # (the row-wide shift of a depth has a standard deviation of up to 0.52)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["b1", "b2", "g-D128", "g-D40", "g-D104"])
def test_ramps_mix_depths_inside_every_wave(oracle_mod, kind, dtype):
    build, causals = sr.KINDS[kind]
    for c in build(oracle_mod.round_to, dtype):
        for causal in causals:
            m = _row_max(oracle_mod, c, dtype, causal)
            N = m.shape[-1]
            for g0 in range(0, N - 31, 32):  # every whole 32-row group
                g = m[..., g0:g0 + 32]
                assert (((g <= -11) & (g >= -21)).sum(-1) >= 8).all() and ((g > -8).sum(-1) >= 2).all(), (c.name, causal, g0)
                if kind == "b2":
                    assert ((g < -26).sum(-1) >= 2).all(), (c.name, causal, g0)
            if kind != "b2":
                assert m.min() > -21.5, (c.name, causal, m.min())  # no first-tile row sum is zero: 64 * 2^(-21.5 - 3) rounds to 2^-24 at least


@pytest.mark.parametrize("rest", ["ordinary", "climb", "lower"])
def test_first_tile_cases(oracle_mod, rest):
    for dtype in ("f16", "bf16"):
        (c,), _ = sr.KINDS[{"ordinary": "f-i", "climb": "f-ii", "lower": "f-iii"}[rest]][0](oracle_mod.round_to, dtype), None
        s = sr.log2_scores(oracle_mod, c.q, c.k, dtype, False)
        first = s[..., :64].max(-1) - np.asarray(sr.DEPTHS_F, float)[:, None, None]
        assert np.abs(first).max() < 2.0, first
        if rest == "ordinary":  # the reference has to climb by 4 at least
            assert (s[..., 64:].max(-1) > s[..., :64].max(-1) + 4.0).all() and s.max() < 4.0
        if rest == "climb":  # every 64 keys 1 ... 3 above the 64 before, and no score ever reaches the assumed maximum + 1: no P' >= 2
            tops = np.stack([s[..., t:t + 64].max(-1) for t in range(0, 300, 64)], -1)
            step = np.diff(tops, axis=-1)
            assert (step > 1.0).all() and (step < 3.0).all() and s.max() < 0.0, (step.min(), step.max(), s.max())
        if rest == "lower":
            assert (s[..., 64:].max(-1) < s[..., :64].max(-1) - 7.0).all()


def test_a_floor_next_to_the_first_tile_boundary_is_not_enough(oracle_mod):
    # (f-iv) the first 64 keys at -2 ... -10, a thousand keys 8 lower: with a floor of 2^-7 the first tile at -9 (row sums of about 2^-6)
    # is kept, the tail's P' of 2^-20 have five bits and the LSE misses the bar; with the kernel's floor every depth holds it
    (c,) = sr.KINDS["f-iv"][0](oracle_mod.round_to, "f16")
    s = sr.log2_scores(oracle_mod, c.q, c.k, "f16", False)
    gap = s[..., :64].max(-1) - s[..., 64:].max(-1)
    assert gap.min() > 6.0 and gap.max() < 10.0, (gap.min(), gap.max())
    for causal in (False, True):
        _, el = assumed_reference(oracle_mod, c, causal, 2.0 ** -7)
        assert el[list(sr.DEPTHS_TAIL).index(-9)].max() >= BAR_LSE, el.max((1, 2))
        fo, fl = assumed_reference(oracle_mod, c, causal, F16_FLOOR)
        assert fo.max() < BAR_O and fl.max() < BAR_LSE, (fo.max(), fl.max())


SHARP = ["a", "b1", "c", "d", "e", "f-iii"]


@pytest.mark.parametrize("kind", SHARP)
def test_f16_cases_are_sharp_against_the_assumed_reference(oracle_mod, kind):
    build, causals = sr.KINDS[kind]
    for c in build(oracle_mod.round_to, "f16"):
        if c.q.shape[2] > 300:
            continue  # (the longest sequences add nothing here: the first 64 keys decide)
        for causal in causals:
            eo, el = assumed_reference(oracle_mod, c, causal, 2.0 ** -64)
            fo, fl = assumed_reference(oracle_mod, c, causal, F16_FLOOR)
            assert fo.max() < BAR_O and fl.max() < BAR_LSE, (c.name, causal, fo.max(), fl.max())  # with the floor: within the bar
            top = sr.log2_scores(oracle_mod, c.q, c.k, "f16", causal).max(-1)
            for b, d in enumerate(c.depth):
                missed = eo[b].max() >= BAR_O or el[b].max() >= BAR_LSE
                # uniform depths below -20: some row of nearly every wave has all its P' zero and the old guard fires for the wave.
                # (c) at -15: 300 keys spread over 0.2 log2 units round independently and average out (model: 2.0e-4 ... 6.3e-4 on O and
                # LSE, under the bar; causal rows 0 ... 32 miss it) -- sharp from -18 on.
                deep = {"a": -20 <= d <= -15, "d": -20 <= d <= -15, "c": d <= -18}.get(kind, d <= -15)
                if deep:
                    assert missed, (c.name, causal, d, eo[b].max(), el[b].max())
                if top[b].max() > -9 and c.window[b].all():
                    assert not missed, (c.name, causal, d, eo[b].max(), el[b].max())
