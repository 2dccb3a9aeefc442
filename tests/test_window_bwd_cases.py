"""The catalogue of the sliding-window backward's GPU tests (window.CASES x window.SEQS), judged on the CPU (numpy only):
  * the walk model of tests/window_backward.py -- block ranges, tile loops, wave skips, masks, dead rows as the two kernels form them --
    applies exactly the rule's visibility on every case;
  * backward_bound.head_model -- the kernels' roundings -- under the window masks stays inside the per-sequence bound (ratio <= 1);
  * each planted mistake of the walk exceeds the bound on a NAMED case, in both dtypes: a catalogue on which a mistake does not show is no
    evidence that the kernels do not make it."""
import numpy as np
import pytest

import backward_bound as bb
import chain_bound as cb
import window as W
import window_backward as wb


def draw(seed, Hq, Hkv, Lq, Lk, D, dtype):
    rng = np.random.default_rng(seed)

    def one(*shape):
        return bb.rnd(rng.uniform(-1.0, 1.0, shape).astype(np.float32), dtype)
    return one(Hq, Lq, D), one(Hkv, Lk, D), one(Hkv, Lk, D), one(Hq, Lq, D)


def test_the_walks_apply_exactly_the_rule_on_every_case():
    max_q, max_k = max(s[0] for s in W.SEQS), max(s[1] for s in W.SEQS)
    for name, seqs, wl, wr in W.CASES:
        for Lq, Lk in seqs:
            vis = W.visible(Lq, Lk, wl, wr)
            for mq, mk in ((None, None), (max_q, max_k)):
                eff_dq, eff_kv = wb.walk(Lq, Lk, wl, wr, None, mq, mk)
                assert (eff_dq == vis).all() and (eff_kv == vis).all(), (name, Lq, Lk)
            n0 = wb.first_live_row(Lq, Lk, wl, wr)
            assert (W.dead_rows(Lq, Lk, wl, wr) == (np.arange(Lq) < n0)).all(), (name, Lq, Lk)


def test_forward_errors_agree_with_chain_bound_on_the_causal_mask():
    q, k, v, do = draw(5, 1, 1, 70, 130, 64, "bf16")
    mask = W.visible(70, 130, -1, 0)
    R = bb.head_exact(q[0], k[0], v[0], do[0], True, 0.125)
    assert (R["mask"] == mask).all()
    want = cb.head_errors(q[0], k[0], v[0], True, 0.125, "bf16", ["mfma"], R)
    got = wb.forward_errors(q[0], k[0], v[0], mask, 0.125, "bf16", R)
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("D", [64, 128])
def test_rounding_model_stays_inside_the_bound_on_every_case(dtype, D):
    worst = 0.0
    for ci, (name, seqs, wl, wr) in enumerate(W.CASES):
        for si, (Lq, Lk) in enumerate(seqs):
            sb = wb.SeqBounds(*draw(100 * ci + si + D, 2, 1, Lq, Lk, D, dtype), wl, wr, None, dtype)
            r = wb.worst_ratio(sb.model(), sb)
            assert r <= 1.0, (name, (Lq, Lk), r)
            worst = max(worst, r)
            n0 = sb.n0  # rows without a visible key, keys no query sees: zero gradient, zero bound
            assert not sb.ref[0][:, :n0].any() and not sb.bound[0][:, :n0].any()
            assert not sb.ref[1][:, sb.unseen].any() and not sb.bound[2][:, sb.unseen].any()
    print(f"worst model error / bound {dtype} D={D}: {worst:.3f}")
    assert worst > 0.01  # the bound is not vacuous


# (mistake, case name, (Lq, Lk)): where each planted mistake must show
NAMED = {
    "lo_edge": ("w63", (130, 257)),
    "hi_edge": ("w127_r5", (130, 257)),
    "dq_start_last_row": ("w63", (257, 513)),
    "dkdv_end_first_key": ("w63", (257, 513)),
    "skip_too_much": ("point", (130, 257)),  # cl = 127: the pair (row 0, key 127) is alone in its sub-tile for both kernels' first wave
    "dead_by_coff": ("w127_r5", (200, 130)),
}


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("bug", wb.BUGS)
def test_each_planted_mistake_exceeds_the_bound_on_its_named_case(bug, dtype):
    name, (Lq, Lk) = NAMED[bug]
    _, seqs, wl, wr = next(c for c in W.CASES if c[0] == name)
    assert (Lq, Lk) in seqs
    sb = wb.SeqBounds(*draw(7, 2, 1, Lq, Lk, 64, dtype), wl, wr, None, dtype)
    assert wb.worst_ratio(sb.walk_model(None), sb) <= 1.0
    r = wb.worst_ratio(sb.walk_model(bug), sb)
    print(bug, dtype, name, (Lq, Lk), "error / bound", r)
    assert not r <= 1.0, (bug, r)
