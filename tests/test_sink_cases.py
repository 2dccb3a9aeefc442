"""CPU: the bars of tests/sink.py hold an fp32 model of both sink epilogues and of the dsink reduction, and each planted mistake exceeds
one of them on a named case -- so the GPU tests (tests/test_gpu_sink.py, test_gpu_sink_bwd.py), which use the same bars, can tell a
kernel that makes it. The models' tile loops are exact (one rounding of m, l and the accumulators to fp32): what is judged here is the
fold, with lse_tol = o_tol = 0 for the un-sinked route -- stricter than any GPU test."""
import numpy as np
import pytest

import backward_bound as bb
import sink as sk
import window as wn

D, HEADS = 64, (8, 2)
SEQS = {"dead_rows": (200, 130), "coff_127": (130, 257), "square": (70, 70)}
SINKS = sk.sinks_for(HEADS[0])
# what one rounding of the exact (m, l, acc) to fp32 costs: the models' own input error, in place of the route's tolerances
IN_LSE, IN_O = 2.0 ** -22 * 8, 2.0 ** -22


def seq(name, seed=0):
    rng = np.random.default_rng(1800 + seed + sum(SEQS[name]))
    Lq, Lk = SEQS[name]
    return wn.draw_seqs(bb.rnd, rng, HEADS[0], HEADS[1], D, "bf16", [(Lq, Lk)])[0]


def worst_forward(name, window, sinks, bug=None, splits=1):
    """Worst error / bar of the forward model on one case (inf: a NaN / Inf, or a dead row that is not exactly O = 0, LSE = sink)."""
    q, k, v = seq(name)
    o, lse = wn.reference(q, k, v, *window)
    o2, lse2 = sk.fold(o, lse, sinks)
    ob, lb = sk.bars(IN_LSE, IN_O, o2, lse, lse2, sinks)
    om, lm = sk.forward_model(q, k, v, *window, sinks, bug=bug, splits=splits)
    dead = wn.dead_rows(*SEQS[name], *window)
    if not (np.isfinite(om).all() and np.isfinite(lm).all()):
        return np.inf
    if om[:, dead].any() or not np.array_equal(lm[:, dead], np.repeat(np.float32(sinks)[:, None], dead.sum(), axis=1)):
        return np.inf
    return max(float((np.abs(om - o2) / ob).max()), float((np.abs(lm - lse2) / lb).max()))


CASES = [(n, w) for n in SEQS for w in sk.WINDOWS]


def test_the_models_stay_inside_every_forward_bar():
    worst = 0.0
    for name, window in CASES:
        for splits in (1, 5):
            for sinks in (SINKS, np.full(8, 60, np.float32), np.full(8, -60, np.float32), np.full(8, 100, np.float32), np.full(8, -1e4, np.float32)):
                r = worst_forward(name, window, sinks, splits=splits)
                assert r <= 1.0, (name, window, splits, sinks[:4], r)
                worst = max(worst, r)
    print(f"SINK forward model: worst error / bar {worst:.3f}")
    assert worst > 0.01  # the bars are not vacuous


def test_a_sink_that_underflows_changes_no_bit_of_the_model():
    for name, window in (("coff_127", (63, 0)), ("dead_rows", (-1, 0))):
        q, k, v = seq(name)
        live, m2, l, acc = sk.exact_state(q, k, v, *window)
        for h in range(2):
            o, lse = sk.epilogue_model(m2[h], l[h], acc[h], -1e4)
            want_o = (acc[h] * (np.float32(1) / l[h])[:, None]).astype(np.float32)
            want_l = (m2[h] * sk.LN2_32 + np.log(l[h]).astype(np.float32)).astype(np.float32)
            assert np.array_equal(o.view(np.int32), want_o.view(np.int32)) and np.array_equal(lse.view(np.int32), want_l.view(np.int32))


# each planted mistake, and the case that exposes it
@pytest.mark.parametrize("bug,name,window,sinks", [
    ("scaled", "square", (-1, 0), SINKS),                     # the sink times the softmax scale: head 3's 8.0 becomes 1.0
    ("log_base", "coff_127", (63, 0), SINKS),                 # natural-log units taken for log2 units
    ("neighbour_head", "coff_127", (127, 5), SINKS),          # sinks[h / G]: head 1 reads head 0's -1e4
    ("dead_neg_inf", "dead_rows", (-1, 0), SINKS),            # rows 0 .. 69 of (200, 130) see no key
    ("no_max", "square", (15, 0), np.full(8, 100, np.float32)),  # 2^(s2 - m) overflows fp32 from s2 - m = 128 on
])
def test_every_planted_forward_mistake_exceeds_a_bar(bug, name, window, sinks):
    assert worst_forward(name, window, sinks) <= 1.0
    assert worst_forward(name, window, sinks, bug=bug) > 1.0, bug
    if bug != "neighbour_head":  # (the combine's model takes its sink from the caller)
        assert worst_forward(name, window, sinks, bug=bug, splits=5) > 1.0, (bug, "combine")


# ---- dsink ---------------------------------------------------------------------------------------------------------------------------
def dsink_case(seed=0, nan_unowned=True):
    """A packed batch of lse / delta [Hq, total_q] as the backward hands them to the reduction: three sequences of which the second is
    clamped by max_seqlen_q, 37 tokens nobody owns at the end; what the kernel must not read holds NaN."""
    rng = np.random.default_rng(1890 + seed)
    Hq, total_q, max_q = 8, 2600, 1500
    cu_q = np.array([0, 300, 2000, 2563], np.int32)  # lengths 300, 1700 (clamped to 1500), 563
    sinks = sk.sinks_for(Hq)
    lse = np.logaddexp(rng.uniform(2.0, 6.0, (Hq, total_q)), sinks[:, None].astype(np.float64)).astype(np.float32)
    delta = rng.uniform(-1.0, 1.0, (Hq, total_q)).astype(np.float32)
    owned = np.zeros(total_q, bool)
    owned[np.concatenate(sk.owned_rows(cu_q, total_q, max_q))] = True
    assert owned.sum() == 300 + 1500 + 563
    if nan_unowned:
        delta[:, ~owned] = np.nan
    return sinks, lse, delta, cu_q, max_q


def dsink_ratio(bug=None, **kw):
    sinks, lse, delta, cu_q, max_q = dsink_case(**kw)
    got = sk.dsink_model(sinks, lse, delta, cu_q, max_q, bug)
    if not np.isfinite(got).all():
        return np.inf
    want, bound = sk.dsink_exact(sinks, lse, delta, cu_q, max_q), sk.dsink_bound(sinks, lse, delta, cu_q, max_q)
    assert (bound[1:] > 0).all() and bound[0] == 0 and want[0] == 0  # head 0's sink at -1e4: exactly nothing
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, np.abs(got - want) / bound, np.where(got != want, np.inf, 0.0))
    return float(r.max())


def test_the_dsink_model_stays_inside_its_bound_and_is_reproducible():
    worst = max(dsink_ratio(seed=s) for s in range(4))
    print(f"SINK dsink model: worst error / bound {worst:.3f}")
    assert 0.001 < worst <= 1.0
    a, b = (sk.dsink_model(*dsink_case()) for _ in range(2))
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("bug", sk.BUGS_DSINK)
def test_every_planted_dsink_mistake_exceeds_the_bound(bug):
    assert dsink_ratio(bug) > 1.0, bug
    if bug == "unowned":  # finite garbage where nobody owns a token is caught as well
        assert dsink_ratio(bug, nan_unowned=False) > 1.0


def test_dead_rows_add_nothing_and_the_reference_matches_autodiff_by_differences():
    # (200, 130) under the mask: rows 0 .. 69 are dead -- lse = sink, O = 0, delta = 0 -- and the end-to-end dsink of sink.SeqBounds is
    # the derivative of sum(dO o O') with respect to the sink, checked by central differences in fp64
    q, k, v = seq("dead_rows")
    do = bb.rnd(np.random.default_rng(7).uniform(-1, 1, q.shape).astype(np.float32), "bf16")
    sinks = SINKS.astype(np.float64)
    sb = sk.SeqBounds(q, k, v, do, -1, 0, sinks, None, "bf16")
    assert sb.n0 == 70 and not sb.o[:, :70].any() and np.array_equal(sb.lse[:, :70], np.repeat(sinks[:, None], 70, axis=1))

    def loss(s):
        return (do.astype(np.float64) * sk.reference(q, k, v, -1, 0, s, bb.default_scale(D))[0]).sum((1, 2))
    for h in (1, 3, 5):
        e = np.zeros(8)
        e[h] = 1e-5
        fd = (loss(sinks + e)[h] - loss(sinks - e)[h]) / 2e-5
        assert abs(fd - sb.dsink_ref[h]) < 1e-6 * max(1.0, abs(fd)), (h, fd, sb.dsink_ref[h])
    assert sb.dsink_chain[0] == 0 and (sb.dsink_chain[1:] > 0).all() and np.isfinite(sb.dsink_chain).all()  # (head 0: the sink at -1e4)
