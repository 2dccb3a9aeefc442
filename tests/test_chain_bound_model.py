"""The chain bound (tests/chain_bound.py into tests/backward_bound.py) on the CPU: no GPU, no kernel.

A forward MODEL (exact_forward.model_arrays: fp32 online softmax in 64-key tiles, lagging reference, P rounded to the type, row sum over
fp32 or rounded P, 1 / 2 / 8 key splits, O rounded to the type, query operand pre-scaled or not) writes O and LSE; the backward model of
backward_bound.head_model consumes them. Over dtype x D (64, 128, 40, 256) x causal / full x MHA N = 203 / grouped rectangular
(Hq 4, Hkv 2, Nq 130, Nk 200) x default scale / 0.3 and five forward variants:
(a) the model's O and LSE lie within chain_bound's o_err / lse_err, element by element / row by row;
(b) the backward model's gradients lie within 1.0 x the given-input bound of the given-input reference AND within 1.0 x the
    true-gradient bound (lse_err, o_err) of the fp64 gradient, on every element;
(c) six sabotaged O / LSE handed to the backward model exceed the true-gradient bound on at least one element.
    They run on a square causal shape of 198 rows (B 2, Hq 4, Hkv 2, D 64) through all five variants; "lse + 4 lse_err" runs where
    lse_err is not dwarfed by u (mfma, mfma16, mfma_split2; with the 1e-4 of mfma_exact / mfma_splitkv it lies inside u by
    construction -- such an LSE is as good as the documented one). In this shape the last row is one of the rows i % 32 == 5 and its
    last key is seen by that row alone, so dV of that key is ONE product and the row's factor exp(-4 lse_err) shows undiluted
    (1.5 ... 2.0 x bound). The mask leak is put on row 1, where the leaked key carries a third of the row.
WHAT THE TRUE-GRADIENT BOUND DOES NOT SEE. It is a worst-case bound, loose wherever many comparable terms add: where the damaged rows
share every key with undamaged ones (N = 203) "lse + 4 lse_err" on one row in 32 stays INSIDE it (0.8), and a mask leak on row 37
(one key in 39) moves bf16 gradients by 0.14 x bound, indistinguishable from rounding. So the per-element bound does not in general
detect one LSE row in 32 that is off by a few lse_err, nor a leak of a key that carries a few percent of its row; it detects LSE and O
faults of the order of the quantities themselves (wrong base, wrong row, wrong head, wrong batch entry: 3 ... 650 x bound) and small
ones only where an element is one product. The given-input ratio of tests/test_gpu_chain.py is the tight one (a function of the
backward's inputs alone); the true ratio there is small on dQ / dK for the same reason (see that file's table).
Measured (printed by the tests), worst over the grid, f16 / bf16: forward model |lse - exact| / lse_err 0.27 / 0.21, |O - exact| / o_err
0.73 / 0.77; gradients / given-input bound 0.34 / 0.36, / true-gradient bound 0.29 / 0.36. No term had to be added to the derivation
the issue states; chain_bound.py spells out two the header documents (f16 subnormal O, low probabilities of f16 mfma16).
The blind spot. rel() < TOL of tests/test_gpu_backward.py (4e-3 f16 / 2e-2 bf16) on the same sabotaged gradients: it CATCHES LSE times
log2(e) (rel 0.4-0.6), rows shifted by one (0.5-1.2), the other head's LSE (0.3-0.6), the other batch entry's O (2.3-2.7 on dQ, dK) and
the mask leak on row 1 (0.13-0.26) -- at these sizes such faults reach the largest gradients --, and LETS THROUGH "lse + 4 lse_err on
the rows i % 32 == 5" in every variant and type (rel 1e-3 ... 2.0e-2 against 2.0 ... 1.5 x bound): one wrong row in 32.
"""
import numpy as np
import pytest

import backward_bound as bb
import chain_bound as cb
import exact_forward as ef
from test_backward_bound_model import TOL, inputs, rel

# forward model variants: name -> (chain_bound kernel, model_arrays keywords); the mfma16 form takes shift 3 (f16) / 7 (bf16)
VARIANTS = {
    "mfma": ("mfma", dict(thr=8.0, splits=1)),
    "mfma_exact": ("mfma_exact", dict(thr=8.0, splits=1)),
    "mfma16": ("mfma16", dict(thr=4.0, splits=1, sum_rounded=True)),
    "mfma_split2": ("mfma_split2", dict(thr=8.0, splits=2, interleave=True)),
    "mfma_splitkv": ("mfma_splitkv", dict(thr=8.0, splits=8, interleave=False)),
}
SHAPES = [(1, 2, 2, 203, 203), (1, 4, 2, 130, 200)]  # B, Hq, Hkv, Nq, Nk


def forward_model(q, k, v, causal, scale, dtype, variant, damage=None):
    """O [B,Hq,Nq,D] (values of the type) and LSE [B,Hq,Nq] (fp32) of a forward model variant. damage(b, h, vis) may edit a head's mask."""
    kern, kw = VARIANTS[variant]
    kw = dict(kw)
    if variant == "mfma16":
        kw["shift"] = 3.0 if dtype == "f16" else 7.0
    B, Hq, Nq, D = q.shape
    G = Hq // k.shape[1]
    pre = cb._prescaled(cb.KERNELS[kern], dtype, D)
    o, lse = np.zeros(q.shape, np.float32), np.zeros(q.shape[:3], np.float32)
    rng = np.random.default_rng(11)
    for b in range(B):
        for h in range(Hq):
            _, vis = cb.log2_scores(q[b, h], k[b, h // G], causal, scale)
            if damage is not None:
                vis = damage(b, h, vis.copy())
            o[b, h], lse[b, h] = ef.model_arrays(q[b, h], k[b, h // G], v[b, h // G], vis, ef.c2_of(scale), dtype, dtype, dtype, rng=rng,
                                                 prescaled=pre, **kw)
    return o, lse


def chain(q, k, v, do, causal, scale, dtype, variant, o=None, lse=None):
    """Bounds of one problem with the variant's lse_err / o_err, the backward model run on (o, lse) (default: the forward model's)."""
    if o is None:
        o, lse = forward_model(q, k, v, causal, scale, dtype, variant)
    le, oe = cb.errors(q, k, v, causal, scale, dtype, cb.kernels_of(VARIANTS[variant][0], dtype))
    X = bb.Bounds(q, k, v, do, causal, scale, dtype, model=True, lse_err=le, o_err=oe, o_in=o.astype(np.float64), lse_in=lse.astype(np.float64))
    return X, le, oe, o, lse


@pytest.mark.parametrize("D", [64, 128, 40, 256])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_forward_and_backward_models_stay_within_the_chain_bound(oracle_mod, dtype, D):
    worst = dict(lse=0.0, o=0.0, given=0.0, true=0.0)
    for (B, Hq, Hkv, Nq, Nk) in SHAPES:
        q, k, v, do = inputs(oracle_mod, dtype, B, Hq, Hkv, Nq, Nk, D)
        for causal in (False, True):
            for scale in (bb.default_scale(D), 0.3):
                for variant in VARIANTS:
                    if variant in ("mfma16", "mfma_split2") and D == 256:
                        continue  # (no such kernel: the 16x16x32 and the two-split forms end at head_dim 128)
                    X, le, oe, o, lse = chain(q, k, v, do, causal, scale, dtype, variant)
                    r_l = float((np.abs(lse - X.lse) / le).max())
                    r_o = float((np.abs(o - X.o) / oe).max())
                    r_g = bb.ratios(X.model, X.given_ref, X.given_bound)
                    r_t = bb.ratios(X.model, X.ref, X.bound)
                    print(f"chain model {dtype} D{D} Hq{Hq} Hkv{Hkv} Nq{Nq} Nk{Nk} causal={int(causal)} scale={scale:.4f} {variant:12s} | fwd lse {r_l:.3f} "
                          f"o {r_o:.3f} | given dq {r_g[0]:.3f} dk {r_g[1]:.3f} dv {r_g[2]:.3f} | true dq {r_t[0]:.3f} dk {r_t[1]:.3f} dv {r_t[2]:.3f}")
                    tag = (dtype, D, (B, Hq, Hkv, Nq, Nk), causal, scale, variant)
                    assert r_l <= 1.0 and r_o <= 1.0, (tag, r_l, r_o)
                    assert max(r_g) <= 1.0, (tag, "given", r_g)
                    assert max(r_t) <= 1.0, (tag, "true", r_t)
                    for key, val in (("lse", r_l), ("o", r_o), ("given", max(r_g)), ("true", max(r_t))):
                        worst[key] = max(worst[key], val)
    print(f"chain model {dtype} D{D}: worst fwd lse {worst['lse']:.3f} o {worst['o']:.3f} given {worst['given']:.3f} true {worst['true']:.3f}")


def test_default_arguments_reproduce_the_former_bound(oracle_mod):
    """lse_err = 0 and o_err = u |O| is the bound without the arguments (to rounding; the defaults themselves are bit for bit the former)."""
    q, k, v, do = inputs(oracle_mod, "bf16", 1, 4, 2, 130, 200, 64)
    X = bb.Bounds(q, k, v, do, True, None, "bf16")
    Y = bb.Bounds(q, k, v, do, True, None, "bf16", lse_err=np.zeros(q.shape[:3]), o_err=bb.U["bf16"] * np.abs(X.o))
    for a, b in zip(X.bound, Y.bound):
        assert np.allclose(a, b, rtol=1e-12, atol=0)
    # the given-input reference on the exact O and LSE is the exact gradient
    Z = bb.Bounds(q, k, v, do, True, None, "bf16", o_in=X.o, lse_in=X.lse)
    for a, b in zip(Z.given_ref, X.ref):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()


SABOTAGE_SHAPE = (2, 4, 2, 198, 198, 64)  # B, Hq, Hkv, Nq, Nk, D
MASK_ROW = 1


def _sabotages(q, k, v, causal, scale, dtype, variant, o, lse, le):
    Nq, Nk = q.shape[2], k.shape[2]
    out = [("LSE times log2(e)", o, lse * np.float32(cb.LOG2E)),
           ("LSE rows shifted by one", o, np.roll(lse, 1, axis=2)),
           ("LSE of the other query head of the group", o, lse[:, [1, 0, 3, 2]]),
           ("O of the other batch entry", o[::-1].copy(), lse)]
    l5 = lse.astype(np.float64).copy()
    l5[:, :, 5::32] += 4.0 * le[:, :, 5::32]
    out.append(("lse + 4 lse_err on the rows i % 32 == 5", o, l5.astype(np.float32)))

    def damage(b, h, vis):
        vis[MASK_ROW, MASK_ROW + (Nk - Nq) + 1] = True
        return vis

    out.append((f"forward mask lets row {MASK_ROW} see key i + coff + 1", *forward_model(q, k, v, causal, scale, dtype, variant, damage)))
    return out


LSE_ERR_INSIDE_U = ("mfma_exact", "mfma_splitkv")  # lse_err = 1e-4: "lse + 4 lse_err" is as good an LSE as the documented one


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_sabotaged_forward_outputs_exceed_the_chain_bound(oracle_mod, dtype, variant):
    B, Hq, Hkv, Nq, Nk, D = SABOTAGE_SHAPE
    causal, scale = True, bb.default_scale(D)
    q, k, v, do = inputs(oracle_mod, dtype, B, Hq, Hkv, Nq, Nk, D)
    X, le, oe, o, lse = chain(q, k, v, do, causal, scale, dtype, variant)
    assert max(bb.ratios(X.model, X.ref, X.bound)) <= 1.0
    assert all(rel(g, r) < TOL[dtype] for g, r in zip(X.model, X.ref))
    for name, o_s, lse_s in _sabotages(q, k, v, causal, scale, dtype, variant, o, lse, le):
        if variant in LSE_ERR_INSIDE_U and name.startswith("lse + 4 lse_err"):
            continue
        Y = bb.Bounds(q, k, v, do, causal, scale, dtype, model=True, lse_err=le, o_err=oe, o_in=o_s.astype(np.float64), lse_in=lse_s.astype(np.float64))
        r = bb.ratios(Y.model, X.ref, X.bound)
        rg = bb.ratios(Y.model, Y.given_ref, Y.given_bound)
        rl = [rel(a, b) for a, b in zip(Y.model, X.ref)]
        through = all(x < TOL[dtype] for x in rl)
        print(f"chain sabotage {dtype} {variant:10s} {name}: true dq {r[0]:.2f} dk {r[1]:.2f} dv {r[2]:.2f} | given {max(rg):.2f} | rel() "
              + " ".join(f"{x:.1e}" for x in rl) + f" (bar {TOL[dtype]:g}): {'PASSES rel()' if through else 'caught by rel()'}")
        assert max(rg) <= 1.0, (name, "the backward model on its own inputs", rg)
        assert max(r) > 1.0, (dtype, variant, name, r)
