"""The soft-capping cases on the CPU (no GPU; tests/softcap.py): the inputs of the GPU parity tests have teeth -- over every case's visible
pairs at least a tenth saturate (|x| > 1.5) and a tenth stay linear (|x| < 0.25); the fp32 model of the kernels' arithmetic stays inside the
bars on them; tanh32 stays inside tanh_err; and each planted mistake exceeds a bar on a named case, in both dtypes."""
import numpy as np
import pytest

import backward_bound as bb
import oracle
import softcap as sc
import window as wn
from util import TOL_O, lse_tol, o_tol

DTYPES = ("f16", "bf16")
_SEQS = {}


def seqs(dtype, D, heads):
    """The sequences of tests/test_gpu_window.py::data (the GPU tests' inputs), drawn the same way."""
    key = (dtype, D, heads)
    if key not in _SEQS:
        rng = np.random.default_rng(14000 + D + 10 * heads[0] + heads[1] + (1 if dtype == "f16" else 0))
        _SEQS[key] = wn.draw_seqs(oracle.round_to, rng, heads[0], heads[1], D, dtype, wn.SEQS)
    return _SEQS[key]


def test_tanh_model_stays_inside_tanh_err():
    x = np.concatenate([np.linspace(-12, 12, 200001), np.array([0.0, 1e-8, -1e-8, 40.0, -40.0, 100.0, -100.0])])
    y = (2.0 * x * 1.4426950408889634).astype(np.float32)
    exact = np.tanh(y.astype(np.float64) / (2.0 * 1.4426950408889634))
    err = np.abs(sc.tanh32(y).astype(np.float64) - exact).max()
    assert err <= sc.TANH_ERR_ROUNDED < sc.TANH_ERR, (err, sc.TANH_ERR_ROUNDED)
    assert err > 1e-7  # the bound is not vacuous: within a factor of four of what the formula really loses
    assert sc.tanh32(np.float32(0)) == 0 and sc.tanh32(np.float32(np.inf)) == 1 and sc.tanh32(np.float32(-np.inf)) == -1
    assert sc.tanh32(np.float32(300.0)) == 1 and sc.tanh32(np.float32(-300.0)) == -1  # 2^y = inf and 2^y = 0: finite at both ends


@pytest.mark.parametrize("D", (64, 128))
def test_the_inputs_have_teeth(D):
    """Every parity case: over its visible pairs at least 10 % saturate and at least 10 % stay linear."""
    for dtype in DTYPES:
        for heads in wn.HEADS:
            for name, cap, rs in sc.REGIMES:
                scale = sc.scale_of(rs, D)
                for wl, wr in sc.WINDOWS:
                    sat = lin = n = 0.0
                    for (q, k, v) in seqs(dtype, D, heads):
                        th = sc.teeth(q, k, wl, wr, cap, scale)
                        if th is None:
                            continue
                        w = float(wn.visible(q.shape[1], k.shape[1], wl, wr).sum())
                        sat, lin, n = sat + th[0] * w, lin + th[1] * w, n + w
                    assert sat / n >= 0.10 and lin / n >= 0.10, (dtype, D, heads, name, (wl, wr), sat / n, lin / n)
    # and the regime that proves nothing: softcap = 50 at the default scale never leaves the linear range
    q, k, _ = seqs("bf16", D, (4, 4))[6]
    assert sc.teeth(q, k, -1, 0, 50.0, bb.default_scale(D))[0] == 0.0


def forward_ratio(o, lse, q, k, v, wl, wr, cap, scale, dtype):
    o64, l64 = sc.reference(q, k, v, wl, wr, cap, scale)
    bar_o, bar_l = sc.bars(lse_tol(dtype, 1, q, k, scale), o_tol(dtype, 1, q, k, v, scale, TOL_O[dtype]), o64, cap)
    live = ~wn.dead_rows(q.shape[1], k.shape[1], wl, wr)
    if not np.isfinite(o).all() or not np.isfinite(lse[:, live]).all():
        return float("inf"), float("inf")
    return float((np.abs(o - o64) / bar_o).max()), float(np.abs(lse[:, live] - l64[:, live]).max() / bar_l)


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_model_stays_inside_the_bars(dtype):
    worst = [0.0, 0.0]
    for D, heads in ((64, (4, 4)), (128, (8, 2))):
        for name, cap, rs in sc.REGIMES:
            scale = sc.scale_of(rs, D)
            for wl, wr in sc.WINDOWS:
                for (q, k, v) in seqs(dtype, D, heads):
                    if k.shape[1] == 0:
                        continue
                    o, lse = sc.forward_model(q, k, v, wl, wr, cap, scale, dtype)
                    ro, rl = forward_ratio(o, lse, q, k, v, wl, wr, cap, scale, dtype)
                    assert ro <= 1.0 and rl <= 1.0, (dtype, D, name, (wl, wr), q.shape, k.shape, ro, rl)
                    worst = [max(worst[0], ro), max(worst[1], rl)]
    print(f"SOFTCAP forward model {dtype}: worst error / bar O {worst[0]:.3f} LSE {worst[1]:.3f}")
    assert worst[1] > 0.01


# the named case of each forward mistake: (sequence index in window.SEQS, window, regime index). (257, 513) under (63, 0) hides most keys
# of every row; the small cap makes exp(-softcap) a weight of 0.78 and C = softcap log2e differ from softcap by 0.11 per unit of t.
FWD_CASES = {
    "mask_before_cap": (6, (63, 0), 0),
    "scale_after_tanh": (6, (63, 0), 0),
    "no_multiply_back": (6, (63, 0), 0),
    "cap_not_log2": (6, (63, 0), 0),
    "recompute_uncapped": (6, (63, 0), 0),
}


@pytest.mark.parametrize("bug", sc.BUGS_FWD)
@pytest.mark.parametrize("dtype", DTYPES)
def test_each_forward_mistake_exceeds_a_bar(dtype, bug):
    b, (wl, wr), r = FWD_CASES[bug]
    for D, heads in ((64, (4, 4)), (128, (8, 2))):
        name, cap, rs = sc.REGIMES[r]
        scale = sc.scale_of(rs, D)
        q, k, v = seqs(dtype, D, heads)[b]
        good = forward_ratio(*sc.forward_model(q, k, v, wl, wr, cap, scale, dtype), q, k, v, wl, wr, cap, scale, dtype)
        bad = forward_ratio(*sc.forward_model(q, k, v, wl, wr, cap, scale, dtype, bug=bug), q, k, v, wl, wr, cap, scale, dtype)
        assert max(good) <= 1.0 < max(bad), (bug, dtype, D, good, bad)


def draw_do(q, dtype, seed):
    return oracle.round_to(np.random.default_rng(seed).uniform(-1.0, 1.0, q.shape).astype(np.float32), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_model_stays_inside_the_bound(dtype):
    worst = 0.0
    for D, heads in ((64, (4, 4)), (128, (8, 2))):
        for name, cap, rs in sc.REGIMES:
            scale = sc.scale_of(rs, D)
            for wl, wr in sc.BWD_WINDOWS:
                for b in (1, 4, 5):  # (70, 70), (200, 130) with dead rows, (130, 257)
                    q, k, v = seqs(dtype, D, heads)[b]
                    sb = sc.SeqBounds(q, k, v, draw_do(q, dtype, 77 + b), wl, wr, cap, scale, dtype)
                    r = max(bb.ratios(sb.model(), sb.ref, sb.bound))
                    assert r <= 1.0, (dtype, D, name, (wl, wr), b, r)
                    worst = max(worst, r)
    print(f"SOFTCAP backward model {dtype}: worst error / bound {worst:.3f}")
    assert worst > 0.01


@pytest.mark.parametrize("bug", sc.BUGS_BWD)
@pytest.mark.parametrize("dtype", DTYPES)
def test_each_backward_mistake_exceeds_the_bound(dtype, bug):
    """The named case: (130, 257) under (63, 0) with the small cap (saturating and linear pairs in every row)."""
    for D, heads in ((64, (4, 4)), (128, (8, 2))):
        name, cap, rs = sc.REGIMES[0]
        scale = sc.scale_of(rs, D)
        q, k, v = seqs(dtype, D, heads)[5]
        sb = sc.SeqBounds(q, k, v, draw_do(q, dtype, 82), 63, 0, cap, scale, dtype)
        good, bad = max(bb.ratios(sb.model(), sb.ref, sb.bound)), max(bb.ratios(sb.model(bug), sb.ref, sb.bound))
        assert good <= 1.0 < bad, (bug, dtype, D, good, bad)
