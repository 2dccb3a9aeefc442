"""The backward's componentwise bound (tests/backward_bound.py) on the CPU: no GPU, no kernel.

(a) a numpy model of the kernels' documented roundings stays within 1.0 x bound on the input families tests/test_gpu_backward_rows.py
    feeds the kernels (at reduced sizes), so the GPU test does not fail a correct kernel;
(b) each gradient of a fixed list of sabotages exceeds 1.0 x bound, while the whole-tensor measure of tests/test_gpu_backward.py,
    rel() = max|g - ref| / max|ref| at 2e-2 (bf16), lets at least the first of them through -- so the GPU test is sharper than that.
Measured (printed by the tests): model worst err / bound 0.59 (bf16) / 0.55 (f16) / 0.40 (e4m3 inputs) over the families; the sabotages
score 7.7 ... 48 in bf16 and 61 ... 379 in f16, the zeroed 16-key tail 46 / 48 (dK / dV, bf16) at rel() = 1.8e-2 / 9.1e-3 < 2e-2.
"""
import numpy as np
import pytest

import backward_bound as bb
from util import make_qkv, rect_reference

TOL = {"f16": 4e-3, "bf16": 2e-2}  # the bars of tests/test_gpu_backward.py


def rel(a, ref):
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-4)


def inputs(oracle, dtype, B, Hq, Hkv, Nq, Nk, D, amp=1.0, do_mul=1.0):
    """The GPU test's inputs: the suite's generator (seeds 42 / 43 / 44, dO 45), rounded to the type."""
    q, _, _ = make_qkv(oracle, B, Hq, Nq, D, dtype, amp=amp)
    _, k, v = make_qkv(oracle, B, Hkv, Nk, D, dtype, amp=amp)
    if amp != 1.0 and dtype != "fp8":  # larger logits: Q and K only
        v = make_qkv(oracle, B, Hkv, Nk, D, dtype)[2]
    do_t = "bf16" if dtype == "fp8" else dtype
    do = oracle.round_to(oracle.init_random(B * Hq * Nq * D, 45).reshape(B, Hq, Nq, D) * np.float32(do_mul), do_t)
    return q, k, v, do


FAMILIES = [  # (name, B, Hq, Hkv, Nq, Nk, D, causal, scale, amp, do_mul)
    ("square causal D=64", 1, 2, 2, 200, 200, 64, True, None, 1.0, 1.0),
    ("square causal N=520", 1, 1, 1, 520, 520, 64, True, None, 1.0, 1.0),
    ("square full D=128", 1, 1, 1, 520, 520, 128, False, None, 1.0, 1.0),
    ("D=256 causal", 1, 1, 1, 129, 129, 256, True, None, 1.0, 1.0),
    ("padded head dim 8", 1, 2, 2, 65, 65, 8, True, None, 1.0, 1.0),
    ("padded head dim 40, scale 1.0", 1, 1, 1, 200, 200, 40, False, 1.0, 1.0, 1.0),
    ("padded head dim 120", 1, 1, 1, 129, 129, 120, True, None, 1.0, 1.0),
    ("scale 0.05", 1, 1, 1, 203, 203, 32, True, 0.05, 1.0, 1.0),
    ("scale 0.3", 1, 1, 1, 300, 300, 64, False, 0.3, 1.0, 1.0),
    ("scale 1.0, D=64", 1, 1, 1, 200, 200, 64, True, 1.0, 1.0, 1.0),
    ("grouped G=4", 1, 4, 1, 129, 129, 64, True, None, 1.0, 1.0),
    ("Nq != Nk causal, coff 160", 1, 2, 1, 100, 260, 64, True, None, 1.0, 1.0),
    ("Nq > Nk full", 1, 2, 2, 260, 100, 64, False, None, 1.0, 1.0),
    ("inputs x3", 1, 1, 1, 300, 300, 64, True, None, 3.0, 1.0),
    ("small dO", 1, 1, 1, 300, 300, 64, True, None, 1.0, 2.0 ** -8),
    ("one key", 1, 1, 1, 1, 1, 64, True, None, 1.0, 1.0),
    ("long causal", 1, 1, 1, 1000, 1000, 64, True, None, 1.0, 1.0),
]


@pytest.mark.parametrize("dtype", ["bf16", "f16", "fp8"])
def test_rounding_model_stays_within_the_bound(oracle_mod, dtype):
    worst = 0.0
    for (name, B, Hq, Hkv, Nq, Nk, D, causal, scale, amp, do_mul) in FAMILIES:
        if dtype == "fp8":
            if D % 16 or amp != 1.0 or do_mul != 1.0:
                continue
            amp = 2.0  # the e4m3 family of the suite
        q, k, v, do = inputs(oracle_mod, dtype, B, Hq, Hkv, Nq, Nk, D, amp, do_mul)
        X = bb.Bounds(q, k, v, do, causal, scale, dtype, model=True)
        # the module's own fp64 gradients are the suite's references
        for a, b in zip(X.ref, rect_reference(q, k, v, do, causal, bb.default_scale(D) if scale is None else scale)):
            assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-30)
        if Nq == Nk and Hq == Hkv:
            for a, b in zip(X.ref, oracle_mod.attn_bwd_f64(q, k, v, do, causal, scale)):
                assert np.abs(a - b).max() <= 1e-6 * max(np.abs(b).max(), 1e-30)  # (the oracle takes the scale as an fp32)
        r = bb.ratios(X.model, X.ref, X.bound)
        print(f"model err/bound {dtype:4s} {name:32s} dq {r[0]:.3f} dk {r[1]:.3f} dv {r[2]:.3f}")
        assert max(r) <= 1.0, (dtype, name, r)
        worst = max(worst, *r)
    print(f"model err/bound {dtype}: worst {worst:.3f}")


def _sabotages(q, k, v, do, causal, scale, X):
    """(name, (dq, dk, dv), tensors it damages) on the model's gradients of ONE batch entry with G query heads on one key head."""
    G, N, D = q.shape[1], q.shape[2], q.shape[3]
    R = [bb.head_exact(q[0, h], k[0, 0], v[0, 0], do[0, h], causal, scale) for h in range(G)]
    base = [x.copy() for x in X.model]
    out = []

    def case(name, damaged):
        g = [x.copy() for x in base]
        out.append((name, g, damaged))
        return g

    g = case("dK and dV of the last 16 keys zero (a key-block tail never stored)", (1, 2))
    g[1][0, 0, -16:] = 0
    g[2][0, 0, -16:] = 0
    g = case("diagonal dropped in dK, dV (mask j < i)", (1, 2))
    for h in range(G):
        g[1][0, 0] -= scale * np.diag(R[h]["ds"])[:, None] * q[0, h]
        g[2][0, 0] -= np.diag(R[h]["p"])[:, None] * do[0, h]
    g = case("one 32-query half left out of one key block's dK, dV", (1, 2))
    i0, j0 = 384, 256  # queries 384..415 never reach keys 256..383
    for h in range(G):
        g[1][0, 0, j0:j0 + 128] -= scale * R[h]["ds"][i0:i0 + 32, j0:j0 + 128].T @ q[0, h, i0:i0 + 32].astype(np.float64)
        g[2][0, 0, j0:j0 + 128] -= R[h]["p"][i0:i0 + 32, j0:j0 + 128].T @ do[0, h, i0:i0 + 32].astype(np.float64)
    g = case("rows 1..7 of dQ off by 50 %", (0,))
    g[0][0, :, 1:8] *= 1.5
    g = case("scale taken as 1/sqrt(D) on the finished dK", (1,))
    g[1] *= D ** -0.5 / scale
    g = case("one query head missing from the group sum of dK", (1,))
    g[1][0, 0] -= scale * R[G - 1]["ds"].T @ q[0, G - 1].astype(np.float64)
    return out


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_sabotaged_gradients_exceed_the_bound(oracle_mod, dtype):
    N, D, G, causal, scale = 520, 64, 2, True, 0.3  # (a scale other than 1/sqrt(D) = 0.125: one sabotage confuses the two)
    q, k, v, do = inputs(oracle_mod, dtype, 1, G, 1, N, N, D)
    X = bb.Bounds(q, k, v, do, causal, scale, dtype, model=True)
    r0 = bb.ratios(X.model, X.ref, X.bound)
    assert max(r0) <= 1.0, r0
    assert all(rel(g, r) < TOL[dtype] for g, r in zip(X.model, X.ref))
    print(f"undamaged {dtype}: err/bound dq {r0[0]:.3f} dk {r0[1]:.3f} dv {r0[2]:.3f}")
    passed_rel = []
    for name, g, damaged in _sabotages(q, k, v, do, causal, scale, X):
        r = bb.ratios(g, X.ref, X.bound)
        rl = [rel(a, b) for a, b in zip(g, X.ref)]
        print(f"sabotage {dtype} {name}: err/bound " + " ".join(f"{'dq dk dv'.split()[t]} {r[t]:.1f}" for t in damaged)
              + "; rel() " + " ".join(f"{rl[t]:.1e}" for t in damaged) + f" (bar {TOL[dtype]:g})")
        for t in damaged:
            assert r[t] > 1.0, (dtype, name, t, r[t])
        passed_rel.append(all(x < TOL[dtype] for x in rl))
    if dtype == "bf16":
        assert passed_rel[0], "the whole-tensor measure was expected to let the zeroed key-block tail through"


def test_sabotage_table_of_the_issue(oracle_mod):
    """The square single-head bf16 point (D = 64, N = 520, causal, default scale): zeroed tails of dK / dV pass rel() at 2e-2 and
    exceed the bound by far."""
    q, k, v, do = inputs(oracle_mod, "bf16", 1, 1, 1, 520, 520, 64)
    X = bb.Bounds(q, k, v, do, True, None, "bf16", model=True)
    for tail in (16, 64):
        g = [x.copy() for x in X.model]
        g[2][0, 0, -tail:] = 0
        if tail == 16:
            g[1][0, 0, -tail:] = 0
        r, rl = bb.ratios(g, X.ref, X.bound), [rel(a, b) for a, b in zip(g, X.ref)]
        print(f"last {tail} keys zero: rel dk {rl[1]:.1e} dv {rl[2]:.1e}; err/bound dk {r[1]:.1f} dv {r[2]:.1f}")
        assert max(rl) < TOL["bf16"] and r[2] > 1.0 and (tail != 16 or r[1] > 1.0)


def test_zero_bound_means_exact():
    z = np.zeros((1, 1, 2, 8))
    b = np.zeros_like(z)
    b[..., 0, :] = 1.0
    g = z.copy()
    assert bb.ratios([g], [z], [b]) == [0.0]
    g[0, 0, 1, 3] = 1e-30
    assert bb.ratios([g], [z], [b]) == [np.inf]
