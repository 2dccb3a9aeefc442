"""CPU side of the exact-arithmetic forward tests (tests/exact_forward.py; the GPU side is tests/test_gpu_exact_forward.py):
the cases are what they claim, no input coordinate is idle, an fp32 model of the kernels' online softmax stays inside the bar, and a
table of structural mistakes -- each applied to the fp64 reference -- exceeds it. For the mistakes that touch the PV product only,
the same damage on the suite's U(-1,1) inputs at full length stays INSIDE the flat bar the parity tests use (util.TOL_O) with the LSE
unchanged: that is the gap these tests close."""
from types import SimpleNamespace

import numpy as np
import pytest

import exact_forward as ef
from util import TOL_O, effective_q, make_qkv

def test_scale_makes_the_score_factor_a_power_of_two():
    for kexp in range(-4, 3):
        assert ef.c2_of(ef.exact_scale(kexp)) == np.float32(2.0 ** kexp)
        assert np.float32(ef.exact_scale(kexp)) == np.float32(ef.exact_scale(kexp))  # the C entry points take it as an fp32 value
    # ... so c2 * q is 2^k q bit for bit over ALL finite f16 values
    allf16 = np.arange(1 << 16, dtype=np.uint16).view(np.float16).astype(np.float32)
    allf16 = allf16[np.isfinite(allf16)]
    for kexp in (-3, 1):
        prod = (allf16 * ef.c2_of(ef.exact_scale(kexp))).astype(np.float32)
        assert np.array_equal(prod, allf16 * np.float32(2.0 ** kexp))


def test_rounding_helpers_agree_with_the_oracle(oracle_mod):
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(20000) * np.exp2(rng.integers(-12, 8, 20000))).astype(np.float32)
    for dtype in ("f16", "bf16", "fp8"):
        assert np.array_equal(ef.round_to(x, dtype), oracle_mod.round_to(x, dtype)), dtype


def test_every_gpu_case_is_what_it_claims(oracle_mod):
    """Walks ef.catalogue(): the very specs tests/test_gpu_exact_forward.py runs, in every kernel class it runs them with."""
    n = 0
    for spec, split, e4m3_p in ef.catalogue():
        case = ef.make(spec, split, e4m3_p)
        what = (tuple(spec[:12]), split, e4m3_p, case.span)
        for x in (case.q, case.k, case.v):
            assert ef.representable(x, spec.dtype), what
        if spec.dtype != "fp8" and case.q.size <= 1 << 20:  # the pre-scaled operand is 2^k q, unchanged by its rounding
            assert np.array_equal(effective_q(oracle_mod, case.q, spec.dtype, case.scale), case.q * np.float32(2.0 ** spec.kexp)), what
        grid = float(1 << case.vbits)
        assert np.array_equal(case.v * grid, np.round(case.v * grid)) and np.abs(case.v).max() <= 1.0, what
        heads = ef.heads_of(spec)
        for (b, h) in (heads if spec.group in ("full", "decode", "paged") else [heads[0], heads[-1]]):
            rr = np.arange(spec.Nq) if spec.rows is None else spec.rows
            s = ef.scores(case, b, h, rr)
            assert np.array_equal(s, np.round(s)), what
            if spec.family == "A":
                assert s.min() >= -case.span and s.max() <= 0 and (s[:, 0] == 0).all(), what
            else:  # the stated climb: the two ramps, minus a depth of at most `span`
                ra, rs = ef.ramps(spec.Nk, case.rise)
                solo = (rr % ef.SOLO_EVERY == ef.SOLO_AT)[:, None]
                d = s - ra[None, :] - solo * rs[None, :]
                assert d.min() >= -case.span and d.max() <= 0, what
            ref = ef.reference_head(case, b, h, spec.rows)
            ok = ef.criterion(case, ref, split)
            assert ok.all() if spec.family == "A" else not ok.any(), (what, (b, h), "bar A must apply to every row of a family-A case")
        n += 1
    assert n > 1500


SENSITIVITY = [("A", 1, 2, 1, 200, 200, 64, "bf16", True, 7), ("A", 1, 1, 1, 129, 300, 32, "f16", True, 3), ("A", 1, 1, 1, 300, 300, 128, "fp8", False, 4),
               ("B", 1, 1, 1, 200, 200, 64, "bf16", False, 3), ("A", 1, 1, 1, 130, 130, 40, "bf16", True, 7)]


@pytest.mark.parametrize("spec", SENSITIVITY)
def test_no_input_coordinate_is_idle(spec):
    """Zeroing any single coordinate of Q, of K, or any single column of V moves the reference beyond the bar somewhere."""
    family, B, Hq, Hkv, Nq, Nk, D, dtype, causal, span = spec
    case = ef.build(family, B, Hq, Hkv, Nq, Nk, D, dtype, causal, span=span, seed=3)
    b, h = 0, Hq - 1
    ref = ef.reference_head(case, b, h)
    for which in "qkv":
        for d in range(D):
            x = getattr(case, which)
            saved = x[..., d].copy()
            x[..., d] = 0
            moved = ef.reference_head(case, b, h)
            x[..., d] = saved
            r = ef.ratios(case, ref, moved.o, moved.lse)
            assert max(r["o"], r["lse"]) > 1.0, (spec, which, d, r)


def test_family_b_ramps_rise_past_every_threshold_but_stay_inside_f16():
    import itertools

    # (e4m3 probabilities: a step of 6 takes P' = 8 P to 2^9 > 448, which renews the reference)
    for nk, (rise, jump) in itertools.product((129, 255, 257, 300, 512, 576, 700, 1000, 2049, 4097, 16384), ((ef.TILE_RISE, 9), (ef.TILE_RISE_E4M3, 6))):
        ra, rs = ef.ramps(nk, rise)
        tot = ra + rs
        assert ra[0] == 0 and rs[0] == 0 and (np.diff(ra) >= 0).all() and (np.diff(rs) >= 0).all()
        assert np.diff(ra).max() >= jump and np.diff(rs).max() >= jump  # past THR = 8 (and the f16 16x16x32 kernel's 4) in one step
        assert (np.diff(ra) == 1).sum() >= 3                       # ... and a stretch of steps below it
        for t in range(0, nk, ef.TILE):  # rise inside a tile + depth 3 + BIAS 3 < 24: every P a power of two f16 holds
            assert tot[min(nk, t + ef.TILE) - 1] - tot[t] <= rise
        assert ra.max() <= 48 and rs.max() <= 48  # three coordinates of at most 16 each (e4m3 integers)


MODELS = [  # dtype, probabilities, threshold, splits, interleaved, shift : the kernels' forms
    ("bf16", "bf16", 8.0, 1, True, 0.0), ("f16", "f16", 8.0, 1, True, 0.0), ("bf16", "bf16", 0.0, 1, True, 0.0),  # deferred / exact reference
    ("bf16", "bf16", 8.0, 1, True, 7.0), ("f16", "f16", 4.0, 1, True, 3.0),                                    # the 16x16x32 kernel's BIAS
    ("fp8", "bf16", 8.0, 1, True, 0.0), ("fp8", "fp8", 5.8, 1, True, -3.0),                                    # e4m3 inputs; e4m3 probabilities
    ("bf16", "bf16", 8.0, 2, True, 0.0), ("f16", "f16", 8.0, 2, True, 0.0), ("bf16", "bf16", 0.0, 8, False, 0.0), ("f16", "f16", 0.0, 5, False, 0.0)]


@pytest.mark.parametrize("dtype,p_dtype,thr,splits,interleave,shift", MODELS)
def test_fp32_model_of_the_online_softmax_stays_inside_the_bar(dtype, p_dtype, thr, splits, interleave, shift):
    rng = np.random.default_rng(5)
    worst = {}
    for family in "AB":
        for (Nq, Nk, D, causal) in ((1000, 1000, 64, True), (576, 576, 128, False), (130, 700, 64, True), (2048, 2048, 64, False), (129, 129, 64, True), (257, 257, 96, True)):
            span = ef.span_for(dtype, splits > 1, Nk) if family == "A" else 3
            case = ef.build(family, 1, 2, 1, Nq, Nk, D, dtype, causal, kexp=-1, span=span, seed=Nk, rise=ef.TILE_RISE_E4M3 if p_dtype == "fp8" else ef.TILE_RISE)
            ref = ef.reference_head(case, 0, 1)
            o, lse = ef.model_head(case, 0, 1, p_dtype, "bf16" if dtype == "fp8" else dtype, thr=thr, splits=splits, interleave=interleave, shift=shift, rng=rng)
            r = ef.ratios(case, ref, o, lse, split=splits if splits > 1 else 0, shift=shift)
            assert r["o"] <= 1.0 and r["lse"] <= 1.0, (family, Nq, Nk, D, causal, r)
            if family == "A":
                assert r["proven"] == 1.0
            worst[family] = max(worst.get(family, 0.0), r["o"])
    print("model worst error / bar:", worst)


# ---- the sabotage table --------------------------------------------------------------------------------------------------------
def pv_damage(kind, Nk):
    """The PV-side mistakes: the row sum (LSE) never sees them."""
    j = (Nk // 2) // 64 * 64 + 21  # a key inside a tile in the middle

    def damage(ctx, stage):
        if stage != "weights":
            return
        if kind == "key dropped":
            ctx.p_pv[:, j] = 0
        elif kind == "key counted twice":
            ctx.p_pv[:, j] *= 2
        elif kind == "two V rows swapped inside a 16-key group":
            ctx.v = ctx.v.copy()
            ctx.v[[j, j + 1]] = ctx.v[[j + 1, j]]
        elif kind == "V columns d and d^1 swapped in every row":
            ctx.v = ctx.v.copy()
            ctx.v[:, [4, 5]] = ctx.v[:, [5, 4]]
        elif kind == "V columns d and d^1 swapped in one tile":
            ctx.v = ctx.v.copy()
            ctx.v[j - 21:j - 21 + 64, [4, 5]] = ctx.v[j - 21:j - 21 + 64, [5, 4]]
        elif kind == "16-key group missing":
            ctx.p_pv[:, j - 21 + 48:j - 21 + 64] = 0
        elif kind == "64-key tile missing":
            ctx.p_pv[:, j - 21:j - 21 + 64] = 0
        else:
            raise KeyError(kind)
    return damage


PV_KINDS = ["key dropped", "key counted twice", "two V rows swapped inside a 16-key group", "V columns d and d^1 swapped in one tile",
            "16-key group missing", "64-key tile missing", "V columns d and d^1 swapped in every row"]


def other_damage(kind):
    def damage(ctx, stage):
        case = ctx.case
        Nq, Nk = case.q.shape[2], case.k.shape[2]
        if kind == "one rescale of the accumulator skipped on one row" and stage == "weights":
            ra, _ = ef.ramps(Nk)
            jump = int(ra[Nk - 2] - ra[Nk - 3])  # the last step of the ramp every row sees, two keys before the end
            assert jump >= 9
            ctx.p_pv[np.flatnonzero(ctx.rows == Nq - 1), :Nk - 2] *= 2.0 ** jump  # what the accumulator held was not scaled down
        elif kind == "a split merged with the wrong weight" and stage == "weights":
            odd = (np.arange(Nk) // 64) % 2 == 1
            ctx.p[:, odd] *= 2
            ctx.p_pv[:, odd] *= 2
        elif kind == "causal limit off by one at a tile edge" and stage == "mask":
            lim = ctx.rows + (Nk - Nq) + 1
            hit = (lim % 64 == 0) & (lim < Nk)
            ctx.vis = ctx.vis.copy()
            ctx.vis[np.flatnonzero(hit), lim[hit]] = True
        elif kind == "grouped heads read key head h % Hkv" and stage == "head":
            ctx.hk = ctx.h % case.k.shape[1]
        elif kind == "keys >= Nk of the ragged last tile counted" and stage == "weights":
            ctx.p[:, 0] += (-Nk % 64) * np.exp2(-ctx.m)  # zero-filled rows of the tile: score 0, V = 0
    return damage


OTHER_KINDS = ["one rescale of the accumulator skipped on one row", "a split merged with the wrong weight", "causal limit off by one at a tile edge",
               "grouped heads read key head h % Hkv", "keys >= Nk of the ragged last tile counted"]


@pytest.mark.parametrize("kind", PV_KINDS + OTHER_KINDS)
def test_sabotage_exceeds_the_new_bar(kind):
    family = "B" if kind.startswith("one rescale") else "A"
    # (the last two: decode steps under the decode kernels' bar -- S = decode_splits(Nk) merged splits, the depth span_for gives them)
    for (dtype, Nq, Nk, D, span, S) in (("bf16", 1000, 1000, 64, 7, 0), ("f16", 300, 1000, 64, 3, 0), ("bf16", 2000, 2000, 128, 7, 0), ("fp8", 1000, 1000, 64, 4, 0),
                                        ("bf16", 4, 16386, 128, ef.span_for("bf16", True, 16386), ef.decode_splits(16386)),
                                        ("f16", 4, 1026, 64, ef.span_for("f16", True, 1026), ef.decode_splits(1026))):
        if "split" in kind:  # the merge of key splits: the depth a kernel with a maximum per split takes
            span = ef.span_for(dtype, True, Nk)
        case = ef.build(family, 1, 4, 2, Nq, Nk, D, dtype, True, span=span if family == "A" else 3, seed=11)
        dmg = pv_damage(kind, Nk) if kind in PV_KINDS else other_damage(kind)
        b, h = 0, 1  # (h % Hkv = 1, h // G = 0)
        ref, bad = ef.reference_head(case, b, h), ef.reference_head(case, b, h, damage=dmg)
        split = S or (2 if "split" in kind else 0)
        assert family == "B" or ef.criterion(case, ref, split > 0).all()  # the bar these mistakes must exceed is bar A
        r = ef.ratios(case, ref, bad.o, bad.lse, split=split)
        assert max(r["o"], r["lse"]) > 1.0, (kind, dtype, r)
        if kind in PV_KINDS:
            assert r["lse"] == 0.0 and r["o"] > 1.0  # the row sum is untouched: only O's own bar can notice
        print(f"sabotage {kind!r} {dtype} Nq={Nq} Nk={Nk} D={D}: {r['o']:.0f} x the O bar, {r['lse']:.0f} x the LSE bar")


@pytest.mark.parametrize("kind", PV_KINDS[:-1])
def test_pv_sabotage_passes_the_old_flat_bar(oracle_mod, kind):
    """The gap: on U(-1,1) inputs, scale 1/sqrt(D), the same PV-side damage moves no sampled element of O by as much as
    TOL_O["bf16"] and leaves the LSE as it is. N = 4096, head_dim 64 (config 3's length). (Two V columns swapped in EVERY row is not
    in this list: it moves O by 1.2e-2 here, twice the flat bar, and by 1.0e-2 at N = 16384, head_dim 128 on the rows sampled below --
    the flat bar does see that one; the swap inside one tile, which the transposed LDS read of one fragment would give, it does not.)"""
    N, D = 4096, 64
    q, k, v = make_qkv(oracle_mod, 1, 1, N, D, "bf16")
    plain = SimpleNamespace(q=q, k=k, v=v, causal=False, lens=None, kexp=float(np.log2(D ** -0.5 * 1.4426950408889634)), dtype="bf16", family="B", vbits=6, span=0)
    rows = np.random.default_rng(1).choice(N, 64, replace=False)
    ref = ef.reference_head(plain, 0, 0, rows)
    bad = ef.reference_head(plain, 0, 0, rows, damage=pv_damage(kind, N))
    change = np.abs(bad.o - ref.o).max()
    print(f"{kind!r} at N={N} D={D}: largest change of an O element {change:.2e} (largest |O| {np.abs(ref.o).max():.2e}); flat bar {TOL_O['bf16']:.1e}")
    assert 0 < change < TOL_O["bf16"] and np.array_equal(bad.lse, ref.lse)
