"""The sliding-window catalogue of tests/window.py is what it claims to be (fp64, no GPU): which rows are dead, which keys nobody sees,
which identities hold; the numpy model of the kernels' walk (tile range per block, per-wave skip, two-sided mask, a reference maximum
that starts at the wave's first active tile) stays within the GPU bars on every case; and each mistake the GPU tests exist to catch
exceeds a bar on a named case."""
import numpy as np
import pytest

import window as wn
from util import TOL_O, lse_tol, o_tol

INT_MAX = wn.INT_MAX
DTYPE, D, HEADS = "bf16", 64, (4, 2)


@pytest.fixture(scope="module")
def seqs(oracle_mod):
    return wn.draw_seqs(oracle_mod.round_to, np.random.default_rng(14), HEADS[0], HEADS[1], D, DTYPE, wn.SEQS)


def test_the_catalogue_covers_the_issue():
    assert {c[2] for c in wn.CASES} >= set(wn.WL) and {c[3] for c in wn.CASES} >= set(wn.WR)
    assert all(c[1] == wn.SEQS for c in wn.CASES) and len({c[0] for c in wn.CASES}) == len(wn.CASES)
    assert wn.SEQS == ((1, 1), (70, 70), (129, 1), (64, 0), (200, 130), (130, 257), (257, 513), (100, 1000))
    assert wn.DECODE_NQ == (1, 4) and wn.DECODE_L == (1, 63, 200, 1000)


def test_dead_rows_and_unseen_keys():
    for _, lens, wl, wr in wn.CASES:
        for Lq, Lk in lens:
            dead = wn.dead_rows(Lq, Lk, wl, wr)
            # dead only through the upper bound or without keys
            want = np.ones(Lq, bool) if Lk == 0 else np.zeros(Lq, bool) if wr < 0 else (np.arange(Lq) + Lk - Lq + wr < 0)
            assert np.array_equal(dead, want), (Lq, Lk, wl, wr)
            un = wn.unseen_keys(Lq, Lk, wl, wr)
            rng = wn.key_range(Lq, Lk, wl, wr, 0, Lq - 1)
            seen = np.zeros(Lk, bool)
            if rng:
                seen[rng[0]:rng[1]] = True  # what a sequence sees is one interval
            assert np.array_equal(~un, seen), (Lq, Lk, wl, wr)
    # the cases the GPU tests lean on
    assert wn.dead_rows(129, 1, 0, 0)[:128].all() and not wn.dead_rows(129, 1, 0, 0)[128]
    assert wn.dead_rows(200, 130, 31, 5)[:65].all() and not wn.dead_rows(200, 130, 31, 5)[65:].any()
    assert wn.dead_rows(64, 0, 5, 5).all() and not wn.dead_rows(100, 1000, 0, 0).any()
    assert wn.unseen_keys(100, 1000, 200, 0)[:700].all() and not wn.unseen_keys(100, 1000, 200, 0)[700:].any()
    for wl, wr in ((0, 0), (63, 0), (64, 64), (200, 0), (31, 5)):  # test 5 of the GPU file hides something in each
        assert sum(int(wn.unseen_keys(Lq, Lk, wl, wr).sum()) for Lq, Lk in wn.SEQS) > 0


def test_identities_claimed():
    for Lq, Lk in wn.SEQS:
        i, j = np.arange(Lq)[:, None], np.arange(Lk)[None, :]
        causal = j <= i + Lk - Lq
        assert np.array_equal(wn.visible(Lq, Lk, INT_MAX, 0), causal) and np.array_equal(wn.visible(Lq, Lk, -1, 0), causal)
        assert wn.visible(Lq, Lk, INT_MAX, INT_MAX).all() and wn.visible(Lq, Lk, -1, -1).all()
    assert sum(wn.identity_claimed(*s) for s in wn.SEQS) == 5
    # a causal window of W keys is (W - 1, 0)
    assert (wn.visible(50, 90, 7, 0).sum(1) == 8).all()
    # the shift identity: block 0 of the sequence starts at tile 10, and the shifted problem is the same rule on the remaining keys
    Lq, Lk, wl, drop = wn.SHIFT
    assert (wn.key_range(Lq, Lk, wl, 0, 0, 127)[0] // wn.TILE) * wn.TILE == drop == 640
    assert np.array_equal(wn.visible(Lq, Lk, wl, 0)[:, drop:], wn.visible(Lq, Lk - drop, wl, 0)) and not wn.visible(Lq, Lk, wl, 0)[:, :drop].any()
    L, Nq, wl, drop = wn.SHIFT_DECODE
    assert (wn.key_range(Nq, L, wl, 0, 0, Nq - 1)[0] // wn.TILE) * wn.TILE == drop == 768
    assert np.array_equal(wn.visible(Nq, L, wl, 0)[:, drop:], wn.visible(Nq, L - drop, wl, 0))


def test_known_answer_of_a_one_key_window(seqs):
    for (Lq, Lk), (q, k, v) in zip(wn.SEQS, seqs):
        o, lse = wn.reference(q, k, v, 0, 0)
        rows = np.nonzero(~wn.dead_rows(Lq, Lk, 0, 0))[0]
        ve, ke = np.repeat(v, 2, axis=0), np.repeat(k, 2, axis=0)
        assert np.array_equal(o[:, rows], ve[:, rows + Lk - Lq].astype(np.float64))
        assert np.allclose(lse[:, rows], (q[:, rows].astype(np.float64) * ke[:, rows + Lk - Lq]).sum(-1) * D ** -0.5, rtol=0, atol=1e-12)


def errors(a, b, dead):
    live = ~dead
    eo = np.abs(a[0] - b[0]).max(initial=0.0)
    both = np.isneginf(a[1]) == np.isneginf(b[1])
    el = np.inf if not both.all() else np.abs(a[1][:, live] - b[1][:, live]).max(initial=0.0)
    return eo, el


def test_the_model_of_the_kernels_walk_stays_within_the_gpu_bars(seqs):
    for name, lens, wl, wr in wn.CASES:
        for (Lq, Lk), (q, k, v) in zip(lens, seqs):
            if Lk == 0:
                continue
            eo, el = errors(wn.model(q, k, v, wl, wr), wn.reference(q, k, v, wl, wr), wn.dead_rows(Lq, Lk, wl, wr))
            assert eo < o_tol(DTYPE, 1, q, k, v, None, TOL_O[DTYPE]) and el < lse_tol(DTYPE, 1, q, k), (name, Lq, Lk, eo, el)
            assert eo < 1e-9 and el < 1e-9  # fp64 throughout: the walk is the rule


@pytest.mark.parametrize("bug,case,seq", [("lo_edge", "point", (70, 70)), ("hi_edge", "point", (70, 70)), ("lo_edge", "w64_r64", (257, 513)),
                                          ("hi_edge", "w127_r5", (130, 257)), ("start_last_row", "w200", (257, 513)),
                                          ("no_lower_in_recompute", "w1", (257, 513)), ("ignore_wr", "w31_r5", (70, 70)),
                                          ("ignore_wr", "w64_r64", (100, 1000))])
def test_each_mistake_exceeds_a_bar(seqs, bug, case, seq):
    _, lens, wl, wr = next(c for c in wn.CASES if c[0] == case)
    b = lens.index(seq)
    q, k, v = seqs[b]
    eo, el = errors(wn.model(q, k, v, wl, wr, bug=bug), wn.reference(q, k, v, wl, wr), wn.dead_rows(*seq, wl, wr))
    assert eo > o_tol(DTYPE, 1, q, k, v, None, TOL_O[DTYPE]) or el > lse_tol(DTYPE, 1, q, k), (bug, case, seq, eo, el)
