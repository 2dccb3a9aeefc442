"""The exact-arithmetic sliding-window catalogue of tests/window.py (exact_forward.build_window) is what it claims to be (no GPU):
scores are integers, inputs are representable, every live row stays within the depth budget and -- shallow cases -- is proven exact by
exact_forward.criterion; dead rows are those of window.dead_rows; the cases with a binding bound put, for at least half of their live
rows, a key of a block-mate far enough above the row's own scores to flush a probability (the cases that cannot are listed in
window.LEFT_OUT, and shown here not to); the model of the kernels' walk with probabilities rounded to the type stays within
exact_forward.bars on every case, and each planted mistake exceeds them on a named one."""
import numpy as np
import pytest

import exact_forward as ef
import window as wn

KINDS = (("f16", "shallow"), ("bf16", "shallow"), ("bf16", "steep"), ("bf16", "cliff"))


def all_cases(dtype, slope, D, heads):
    for ramp, window, seqs in wn.exact_specs(dtype, slope):
        for seq in seqs:
            yield ramp, window, seq, wn.exact_case(ramp, slope, window, seq, D, heads, dtype)


def model_ratios(case, bug=None):
    """Worst error / bar over the heads of window.model on a case (natural-log LSE, O rounded to the case's type as the kernels do)."""
    o, lse = wn.model(case.q[0], case.k[0], case.v[0], *case.window, scale=case.scale, bug=bug, p_dtype=case.dtype, base2=True)
    worst = dict(o=0.0, lse=0.0, proven=1.0)
    for h in range(case.q.shape[1]):
        r = ef.ratios(case, ef.reference_head(case, 0, h), ef.round_to(o[h], case.dtype), lse[h], 0, 0.0)
        worst = dict(o=max(worst["o"], r["o"]), lse=max(worst["lse"], r["lse"]), proven=min(worst["proven"], r["proven"]))
    return worst


def test_the_catalogue_covers_the_issue():
    assert wn.EXACT_SEQS == ((70, 70), (200, 130), (130, 257), (257, 513), (100, 1000))
    assert wn.EXACT_WINDOWS == ((15, 0), (63, 0), (64, 64), (127, 5), (200, 0), (65, -1), (-1, 5)) and wn.STEEP_WINDOWS == ((15, 0), (63, 0), (127, 5))
    # bf16 shallow cases carry no claim about hidden keys: nothing of theirs is left out
    assert len(list(wn.exact_specs("bf16", "shallow"))) == 14 and all(len(s) == 5 for _, _, s in wn.exact_specs("bf16", "shallow"))
    assert {w for _, w, _ in wn.exact_specs("f16", "shallow")} == {(15, 0), (63, 0), (65, -1), (-1, 5)}
    assert {(r, w) for r, w, _ in wn.exact_specs("bf16", "steep")} == {("fall", (127, 5)), ("rise", (127, 5))}
    assert {(r, w, tuple(s)) for r, w, s in wn.exact_specs("bf16", "cliff")} == {("fall", (15, 0), wn.EXACT_SEQS[2:4]), ("rise", (15, 0), wn.EXACT_SEQS[:4])}
    assert ef.c2_of(ef.exact_scale(0)) == 1.0 and ef.c2_of(ef.exact_scale(-1)) == 0.5
    assert wn.EXACT_DECODE_L == (63, 200, 1000) and wn.EXACT_DECODE_WINDOWS == ((0, 0), (31, 0), (64, 5), (200, -1))


def test_visible_takes_the_window_rule():
    for Lq, Lk in wn.EXACT_SEQS + ((4, 63), (1, 1000)):
        for wl, wr in wn.EXACT_WINDOWS + wn.EXACT_DECODE_WINDOWS + ((wn.INT_MAX, 0), (wn.INT_MAX, wn.INT_MAX), (-1, -1)):
            case = ef.SimpleNamespace(q=np.zeros((1, 1, Lq, 1)), k=np.zeros((1, 1, Lk, 1)), lens=None, causal=False, window=(wl, wr))
            assert np.array_equal(ef.visible(case, 0, np.arange(Lq)), wn.visible(Lq, Lk, wl, wr)), (Lq, Lk, wl, wr)
    # absent: the causal / full rule as before; with lens: the offset of the sequence's own length
    plain = ef.build("A", 1, 1, 1, 5, 9, 64, "bf16", True)
    assert np.array_equal(ef.visible(plain, 0, np.arange(5)), wn.visible(5, 9, -1, 0))
    case = ef.SimpleNamespace(q=np.zeros((1, 1, 4, 1)), k=np.zeros((1, 1, 300, 1)), lens=[200], causal=False, window=(31, 0))
    assert np.array_equal(ef.visible(case, 0, np.arange(4))[:, :200], wn.visible(4, 200, 31, 0)) and not ef.visible(case, 0, np.arange(4))[:, 200:].any()


def check_claims(case, ramp, window, seq, cspan, need_proof, split=False):
    Lq, Lk = seq
    dtype = case.dtype
    assert ef.representable(case.q, dtype) and ef.representable(case.k, dtype) and ef.representable(case.v, dtype), (ramp, window, seq)
    assert case.window == tuple(window) and case.q.shape[2] == Lq and case.k.shape[2] == Lk
    rows = np.arange(Lq)
    vis = ef.visible(case, 0, rows)
    live = vis.any(1)
    assert np.array_equal(~live, wn.dead_rows(Lq, Lk, *window)), (window, seq)
    r = ef.window_ramp(ramp, Lk, case.every) * ef.WINDOW_STEP[case.slope]
    assert np.array_equal(case.k[0, :, :, -ef.WINDOW_RESERVED:].sum(-1), np.broadcast_to(r, case.k.shape[1:3])) and (np.diff(r) * (1 if ramp == "rise" else -1) >= 0).all()
    if ramp == "rise" and case.slope == "shallow":
        assert max(r[min(t + 64, Lk) - 1] - r[t] for t in range(0, Lk, 64)) + cspan <= ef.WINDOW_BUDGET
    depth = 0
    for h in range(case.q.shape[1]):
        s = ef.scores(case, 0, h, rows)
        assert np.array_equal(s, np.round(s)), "scores are integers"
        if live.any():
            d = (np.where(vis, s, -np.inf).max(1) - np.where(vis, s, np.inf).min(1))[live]
            depth = max(depth, int(d.max()))
            if case.slope == "shallow":
                assert d.max() + cspan <= ef.WINDOW_BUDGET, (ramp, window, seq, d.max())  # every probability >= 2^-24 with room to spare
            else:
                assert d.max() <= 133  # bf16: powers of two are exact down to 2^-133
        proven = ef.criterion(case, ef.reference_head(case, 0, h), split)
        assert not need_proof or proven[live].all(), (ramp, window, seq, h, "a live row of a shallow case is not proven")
        assert case.slope == "shallow" or not proven.any()  # steep: the wider bar, never the narrow one
    assert case.span == depth


@pytest.mark.parametrize("D,heads", wn.EXACT_MATRIX)
def test_every_case_is_what_it_claims(D, heads):
    for dtype, slope in KINDS:
        for ramp, window, seq, case in all_cases(dtype, slope, D, heads):
            assert case.scale == ef.exact_scale(wn.KEXP[D]) and case.family == ("A" if slope == "shallow" else "B")
            check_claims(case, ramp, window, seq, ef.WINDOW_CSPAN, slope == "shallow")
            assert slope != "shallow" or max(v.sum() for v in ef.visible(case, 0, np.arange(seq[0]))) <= 1000


@pytest.mark.parametrize("D", (64, 128))
def test_every_decode_case_is_what_it_claims(D):
    for dtype in ("f16", "bf16", "fp8"):
        for ramp in wn.RAMPS:
            for window in wn.EXACT_DECODE_WINDOWS:
                for Nq in wn.DECODE_NQ:
                    for L in wn.EXACT_DECODE_L:
                        case = wn.decode_case(ramp, window, Nq, L, D, dtype)
                        assert case.vbits == ef.VBITS[dtype] and np.abs(case.k).max() <= (16 if dtype == "fp8" else 256)
                        check_claims(case, ramp, window, (Nq, L), ef.span_for(dtype, True, L), False, split=True)


@pytest.mark.parametrize("D,heads", wn.EXACT_MATRIX)
def test_a_block_mates_key_would_flush_a_probability_of_half_the_rows(D, heads):
    for dtype, slope in (("f16", "shallow"), ("bf16", "steep"), ("bf16", "cliff")):
        bound = 0
        for ramp, window, seq, case in all_cases(dtype, slope, D, heads):
            if wn.bound_binds(ramp, *window):
                bound += 1
                assert wn.hidden_margin(case, wn.FLUSH[dtype]) >= 0.5, (dtype, slope, ramp, window, seq)
        assert bound >= 6, (dtype, slope)


def test_what_is_left_out_cannot_meet_the_claim():
    """Each entry of LEFT_OUT names cases with a binding bound that miss the half on at least one (head dim, heads) of the matrix."""
    for slope, dtype, ramp, window, seqs in wn.LEFT_OUT:
        assert wn.bound_binds(ramp, *window)
        for seq in (seqs or wn.EXACT_SEQS):
            worst = min(wn.hidden_margin(wn.exact_case(ramp, slope, window, seq, D, heads, dtype), wn.FLUSH[dtype]) for D, heads in wn.EXACT_MATRIX)
            assert worst < 0.5, (slope, dtype, ramp, window, seq, worst)


@pytest.mark.parametrize("D,heads", wn.EXACT_MATRIX)
def test_the_model_of_the_kernels_walk_reaches_the_bars(D, heads):
    for dtype, slope in KINDS:
        for ramp, window, seq, case in all_cases(dtype, slope, D, heads):
            r = model_ratios(case)
            assert r["o"] <= 1.0 and r["lse"] <= 1.0, (dtype, slope, ramp, window, seq, r)
            assert slope != "shallow" or r["proven"] == 1.0


SHARP = [  # bug, dtype, slope, ramp, window, sequence
    ("lo_edge", "bf16", "shallow", "fall", (200, 0), (257, 513)),   # the widest windows, in bf16
    ("hi_edge", "bf16", "shallow", "rise", (127, 5), (130, 257)),
    ("lo_edge", "f16", "shallow", "fall", (15, 0), (70, 70)),
    ("hi_edge", "bf16", "steep", "rise", (127, 5), (100, 1000)),
    ("start_last_row", "bf16", "shallow", "fall", (200, 0), (257, 513)),
    ("no_lower_in_recompute", "f16", "shallow", "fall", (15, 0), (130, 257)),     # bounds 112 .. 143 of wave 0 cross the tile edge at 128
    ("no_lower_in_recompute", "bf16", "steep", "fall", (127, 5), (100, 1000)),    # bounds 805 .. 836 of wave 1 cross 832
    ("ignore_wr", "bf16", "shallow", "rise", (64, 64), (100, 1000)),
    ("max_over_hidden", "f16", "shallow", "fall", (15, 0), (130, 257)),
    ("max_over_hidden", "f16", "shallow", "fall", (63, 0), (257, 513)),
    ("max_over_hidden", "bf16", "cliff", "fall", (15, 0), (257, 513)),
    ("max_over_hidden", "bf16", "cliff", "rise", (15, 0), (70, 70)),
]


@pytest.mark.parametrize("bug,dtype,slope,ramp,window,seq", SHARP)
def test_each_mistake_exceeds_a_bar(bug, dtype, slope, ramp, window, seq):
    assert not wn.left_out(slope, dtype, ramp, window, seq)
    for D, heads in ((64, (4, 4)), (128, (8, 2))):
        r = model_ratios(wn.exact_case(ramp, slope, window, seq, D, heads, dtype), bug)
        print(f"{bug} {dtype} {slope} {ramp} {window} {seq} D={D}: O {r['o']:.3g} LSE {r['lse']:.3g} of bar")
        assert r["o"] > 1.0 or r["lse"] > 1.0, (bug, D, r)
