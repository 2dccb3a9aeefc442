"""The key split of the paged prefill on the CPU (tests/ksplit.py; no GPU): on window.SEQS under sink.WINDOWS and S in {2, 3, 5, 16}
  1. the splits of every block partition its tile range: each key the block's rows see lies in exactly one split;
  2. the fp32 model of the partial state and of the combine stays inside the bars, with and without a sink, on U(-1, 1) inputs, on the ramped
     exact-arithmetic inputs of ksplit.ramp_case (the GPU parity test's other half) and on those of window.exact_case;
  3. each planted mistake of ksplit.SABOTAGES exceeds a bar on a named case, in both dtypes;
  4. what gives the ramped parity inputs their teeth: the per-split LSEs of every row with two non-empty splits lie 8 log2 units apart,
     so a merge without weights cannot pass.
These tests hold the numpy model of tests/ksplit.py and the inputs to the header's words; most of them pass without the kernels. What ties
the model to the kernels is the GPU parity test alone (tests/test_gpu_ksplit.py), which checks the kernels against the same references
at the same bars."""
import numpy as np
import pytest

import exact_forward as ef
import ksplit as ks
import sink as sk
import window as wn
from util import TOL_O, lse_tol, o_tol

HQ, HKV, D = 2, 1, 64
DTYPES = ("f16", "bf16")
# window.exact_case's own ramps (one or three units per key) as further inputs of the model: exact bars, no claim about the splits' LSEs
RAMPED = (("bf16", "steep"), ("f16", "shallow"), ("bf16", "shallow"))


def seqs_of(dtype, seed=0):
    rng = np.random.default_rng(2200 + seed + (1 if dtype == "f16" else 0))
    return wn.draw_seqs(ef.round_to, rng, HQ, HKV, D, dtype, wn.SEQS)


def test_the_splits_of_every_block_partition_its_tile_range():
    checked = 0
    for Lq, Lk in wn.SEQS:
        for wl, wr in sk.WINDOWS:
            vis = wn.visible(Lq, Lk, wl, wr) if Lk else np.zeros((Lq, 0), bool)
            for qb in range((Lq + ks.BLOCK - 1) // ks.BLOCK):
                seen = vis[qb * ks.BLOCK:(qb + 1) * ks.BLOCK].any(0)
                bt = ks.block_tiles(Lq, Lk, wl, wr, qb)
                assert (bt is None) == (not seen.any())
                for S in ks.SPLITS:
                    count, split = ks.owner_of_key(Lq, Lk, wl, wr, qb, S)
                    assert (count[seen] == 1).all(), ((Lq, Lk), (wl, wr), qb, S, "a visible key in no split, or in two")
                    if bt is None:
                        assert not count.any()
                        continue
                    inside = np.zeros(Lk, bool)
                    inside[bt[0] * ks.TILE:bt[1] * ks.TILE] = True
                    assert np.array_equal(count == 1, inside) and (np.diff(split[inside]) >= 0).all()  # exactly the tile range, in order
                    ranges = [ks.split_tiles(*bt, s, S) for s in range(S)]
                    assert ranges[0][0] == bt[0] and ranges[-1][1] == bt[1] and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
                    assert sum(t1 == t0 for t0, t1 in ranges) == max(0, S - (bt[1] - bt[0]))  # empty exactly when n < S
                    checked += 1
    assert checked > 300


def ratios(dtype, q, k, v, wl, wr, S, sinks, o, lse):
    """Worst error / bar (O, LSE) of one sequence's fp32 model output against the fp64 reference; inf where a value is not finite."""
    Lq, Lk = q.shape[1], k.shape[1]
    o64, l64 = wn.reference(q, k, v, wl, wr)
    dead = wn.dead_rows(Lq, Lk, wl, wr)
    bar_o, bar_l, o_ref, l_ref = ks.bars(S, lse_tol(dtype, 1, q, k) if Lk else 1e-4, o_tol(dtype, 1, q, k, v, None, TOL_O[dtype]) if Lk else 1e-3, o64, l64,
                                         ks.absum_reference(q, k, v, wl, wr), sinks)
    o = ef.round_to(o, dtype).astype(np.float64)
    if not np.isfinite(o).all():
        return np.inf, np.inf
    want_dead = np.full((q.shape[0], int(dead.sum())), -np.inf, np.float32) if sinks is None else np.repeat(np.asarray(sinks, np.float32)[:, None], dead.sum(), 1)
    if o[:, dead].any() or not np.array_equal(lse[:, dead].view(np.int32), want_dead.view(np.int32)):
        return np.inf, np.inf
    live = ~dead
    if not live.any():
        return 0.0, 0.0
    with np.errstate(invalid="ignore"):
        rl = np.abs(lse.astype(np.float64) - l_ref)[:, live] / bar_l[:, live]
    rl = np.where(np.isfinite(lse[:, live]), rl, np.inf)
    return float((np.abs(o - o_ref) / bar_o)[:, live].max()), float(rl.max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_fp32_model_stays_inside_the_bars(dtype):
    worst = [0.0, 0.0]
    sinks = sk.sinks_for(HQ)[::-1].copy()  # (0.7 within the scores and -0.5; sinks_for's -1e4 comes in the GPU tests)
    for (q, k, v) in seqs_of(dtype):
        for wl, wr in sk.WINDOWS:
            for S in ks.SPLITS:
                for s in (None, sinks):
                    o, lse = ks.forward_model(q, k, v, wl, wr, S, s)
                    ro, rl = ratios(dtype, q, k, v, wl, wr, S, s, o, lse)
                    assert ro <= 1.0 and rl <= 1.0, (dtype, q.shape, k.shape, (wl, wr), S, s is not None, ro, rl)
                    worst = [max(worst[0], ro), max(worst[1], rl)]
    assert worst[0] > 0.01, worst  # the rounding of O to the type alone fills a part of the bar


def ramped_case(dtype, slope, ramp, window, seq):
    return wn.exact_case(ramp, slope, window, seq, D, (4, 4), dtype)


def ramped_ratios(case, S, sinks=None, bug=None):
    """Worst error / bar (O, LSE) over the heads of a ramped case: the model against exact_forward.bars(split=S), on O plus the
    resolution term of lse2_s (ksplit.merge_o_term: these scores reach hundreds of log2 units)."""
    q, k, v = case.q[0], case.k[0], case.v[0]
    o, lse = ks.forward_model(q, k, v, *case.window, S, sinks, scale=case.scale, bug=bug)
    o = ef.round_to(o, case.dtype).astype(np.float64)
    worst = [0.0, 0.0]
    for h in range(q.shape[0]):
        ref = ef.reference_head(case, 0, h)
        b_o, b_l, _ = ef.bars(case, ref, S, 0.0)
        b_o = b_o + ks.merge_o_term(0, ref.absum, ref.lse) - ks.merge_o_term(0, ref.absum)
        some = ref.nvis > 0
        if not np.isfinite(o[h]).all() or not np.isfinite(lse[h][some]).all() or o[h][~some].any() or not np.isneginf(lse[h][~some]).all():
            return [np.inf, np.inf]
        err = np.abs(o[h] - ref.o)
        worst = [max(worst[0], float(np.where(err == 0, 0.0, err / np.where(b_o > 0, b_o, 1e-300)).max())),
                 max(worst[1], float((np.abs(lse[h][some] - ref.lse[some]) / b_l[some]).max(initial=0.0)))]
    return worst


@pytest.mark.parametrize("dtype,slope", RAMPED)
def test_the_model_on_ramped_inputs_stays_inside_the_exact_bars(dtype, slope):
    for ramp, window, seqs in list(wn.exact_specs(dtype, slope))[:3]:
        for seq in seqs[-2:]:
            for S in (2, 5, 16):
                ro, rl = ramped_ratios(ramped_case(dtype, slope, ramp, window, seq), S)
                assert ro <= 1.0 and rl <= 1.0, (dtype, slope, ramp, window, seq, S, ro, rl)


# sabotage -> (kind, what the named case is): "uniform" cases are window.SEQS entries under U(-1, 1), "ramped" ones ksplit.ramp_case
NAMED = {
    "empty_split_weighs_1": ("uniform", (70, 70), (-1, 0), 16, False),     # 2 tiles under 16 splits: 14 empty ones weigh 1 each
    "weights_not_applied": ("ramped", (257, 513), (63, 0), 3, False),      # a row's 64 keys straddle two splits whose maxima differ
    "reference_of_split_0": ("uniform", (257, 513), (15, 0), 2, False),    # rows behind the first tile have no key in split 0: 2^(x + inf)
    "tile_in_two_splits": ("uniform", (70, 70), (-1, 0), 2, False),        # keys 64 .. 69 counted twice
    "last_tile_skipped": ("uniform", (70, 70), (-1, 0), 2, False),         # ... or not at all
    "sink_in_every_split": ("uniform", (130, 257), (127, 5), 16, True),
    "log_base": ("uniform", (100, 1000), (-1, -1), 5, False),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bug", ks.SABOTAGES)
def test_each_planted_mistake_exceeds_a_bar_on_its_named_case(bug, dtype):
    kind, seq, (wl, wr), S, with_sink = NAMED[bug]
    sinks = sk.sinks_for(HQ)[::-1].copy() if with_sink else None
    if kind == "uniform":
        q, k, v = seqs_of(dtype)[wn.SEQS.index(seq)]
        clean = ratios(dtype, q, k, v, wl, wr, S, sinks, *ks.forward_model(q, k, v, wl, wr, S, sinks))
        broken = ratios(dtype, q, k, v, wl, wr, S, sinks, *ks.forward_model(q, k, v, wl, wr, S, sinks, bug=bug))
    else:
        case = ks.ramp_case(seq, D, (4, 4), dtype, (wl, wr))
        clean, broken = ramped_ratios(case, S, sinks), ramped_ratios(case, S, sinks, bug=bug)
    assert max(clean) <= 1.0, (bug, dtype, clean)
    assert max(broken) > 1.0, (bug, dtype, broken, "the planted mistake stays inside both bars on its named case")


# the configurations whose ramped cases the GPU parity test runs (tests/test_gpu_ksplit.py, MATRIX): f16 and bf16 hold the same values
GPU_CONFIGS = ((64, (4, 4)), (128, (8, 2)))


def test_the_ramped_parity_inputs_have_teeth():
    """From the fp64 reference, for every configuration, window.SEQS sequence, sink.WINDOWS window and S of the GPU parity test: the
    per-split LSEs of EVERY row with two or more non-empty splits span at least 8 log2 units (ksplit.RAMP_SPAN; in fact 15: a step of 16
    per key less the 0 / 1 of the query masks). A condition on the inputs. Nothing is left out (ksplit.RAMP_LEFT_OUT; a quarter may be),
    and the ramped cases are half of the parity cases: the same sequences, windows and S as the U(-1, 1) half."""
    cases, rows = 0, 0
    for Dh, heads in GPU_CONFIGS:
        for seq in wn.SEQS:
            case = ks.ramp_case(seq, Dh, heads, "bf16")
            for dtype in DTYPES:
                assert ef.representable(case.q, dtype) and ef.representable(case.k, dtype) and ef.representable(case.v, dtype), (seq, dtype)
            for window in sk.WINDOWS:
                for S in ks.SPLITS:
                    cases += 1
                    if (tuple(window), tuple(seq), S) in ks.RAMP_LEFT_OUT:
                        continue
                    span = ks.split_lse_span(case.q[0], case.k[0], *window, S, scale=case.scale)
                    many = np.isfinite(span)
                    assert (span[many] >= ks.RAMP_SPAN).all(), (Dh, heads, window, seq, S, float(span[many].min()))
                    rows += int(many.sum())
    assert 4 * len(ks.RAMP_LEFT_OUT) * len(GPU_CONFIGS) <= cases and rows > 100000


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", ks.SPLITS)
def test_the_model_on_the_ramped_cases_and_a_merge_without_weights(S, dtype):
    for n, window in enumerate(sk.WINDOWS):
        for seq in wn.SEQS[4 + n % 2::2]:
            case = ks.ramp_case(seq, D, (4, 4), dtype, window)
            ro, rl = ramped_ratios(case, S)
            assert ro <= 1.0 and rl <= 1.0, (window, seq, S, ro, rl)
            assert max(ramped_ratios(case, S, bug="weights_not_applied")) > 1.0, (window, seq, S)


def test_sabotages_are_the_issues_list():
    assert set(NAMED) == set(ks.SABOTAGES) and len(ks.SABOTAGES) == 7
