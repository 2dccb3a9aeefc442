"""GPU: the three sliding-window entry points on exact-arithmetic inputs whose scores ramp along the keys (exact_forward.build_window;
the catalogue lives in tests/window.py and is walked on the CPU by tests/test_window_exact_cases.py). The keys a row does not see score
far above (or below) the keys it sees, so a reference maximum, a mask edge or a first tile taken from the wrong keys moves O and LSE
by far more than the bars. EVERY element of O and LSE is held to exact_forward.bars -- the bars of tests/test_gpu_exact_forward.py,
nothing fitted -- against the fp64 reference of the same rule:
  1. fa_fwd_varlen_window: the sequences of a (window, ramp, slope) packed into one call, with trailing tokens nobody owns. Shallow
     cases: every live row proven exact (bar A), or the test fails; steep and cliff cases (bf16): bar B. Dead rows exactly 0 / -inf.
  2. fa_fwd_varlen_paged_window: the same cases through shuffled pools (P = 16 HND, P = 256 NHD; NaN in unreferenced pages and in
     slots past the length), the same bars, and bit for bit the varlen windowed call for every sequence with Lk >= Lq >= 1.
  3. (INT_MAX, 0) / (INT_MAX, INT_MAX) through the windowed kernels on such scores: bit for bit the causal / full call.
  4. fa_fwd_decode_paged_window: Nq 1 and 4, L 63 / 200 / 1000 in a cache of 4096, four dtype pairs, split = the call's own split count.
Each test prints its worst error / bar ("EXACT ..." lines, "EXACT-SUMMARY ..." at the end of the module; above 1 fails)."""
import numpy as np
import pytest

import decode_range as dr
import exact_forward as ef
import varlen_paged as vp
import window as wn
from test_gpu_decode_paged import to_layout
from util import to_dev

pytestmark = pytest.mark.gpu
INT_MAX = wn.INT_MAX
CAP = 4096
WORST = {}
_REFS = {}


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    yield fa
    for (entry, dtype, slope), w in sorted(WORST.items()):
        print(f"EXACT-SUMMARY {entry} {dtype} {slope}: worst O error / bar {w['o']:.3f}, worst LSE error / bar {w['lse']:.3f}")


def i32(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def bits(t):
    import torch

    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def references(case, key):
    """The fp64 reference of every head of a case, once per process (f16 and bf16 cases hold the same values)."""
    if key not in _REFS:
        _REFS[key] = [ef.reference_head(case, 0, h) for h in range(case.q.shape[1])]
    return _REFS[key]


def hold(case, key, o, lse, entry, what, split=0):
    """o [Hq, Lq, D], lse [Hq, Lq] (numpy) of one sequence against the bars, element by element. Shallow prefill cases: every live row
    proven, or it fails."""
    worst = dict(o=0.0, lse=0.0, proven=1.0)
    for h, ref in enumerate(references(case, key)):
        r = ef.ratios(case, ref, o[h], lse[h], split, 0.0)
        if r["o"] > 1.0 or r["lse"] > 1.0:
            print(f"EXACT {entry} {case.dtype} {case.slope} {what} head {h}: O {r['o']:.3f} (at {r['at']}) LSE {r['lse']:.3f} of bar: ABOVE")
        assert r["o"] <= 1.0 and r["lse"] <= 1.0, (entry, what, h, r)
        if case.family == "A" and split == 0:
            assert ef.criterion(case, ref, False)[ref.nvis > 0].all(), (entry, what, h, "a live row of a shallow case is not proven exact")
        worst = dict(o=max(worst["o"], r["o"]), lse=max(worst["lse"], r["lse"]), proven=min(worst["proven"], r["proven"]))
    print(f"EXACT {entry} {case.dtype} {case.slope} {what}: O {worst['o']:.3f} LSE {worst['lse']:.3f} of bar (rows proven exact: {worst['proven']:.2f})")
    w = WORST.setdefault((entry, case.dtype, case.slope), dict(o=0.0, lse=0.0))
    w["o"], w["lse"] = max(w["o"], worst["o"]), max(w["lse"], worst["lse"])


def pack(cases, dtype):
    """The cases' sequences back to back: q with three trailing tokens nobody owns, k / v with one."""
    qn, cu_q = vp.pack_rows([c.q[0] for c in cases], tail=3)
    kn, cu_k = vp.pack_rows([c.k[0] for c in cases], tail=1)
    vn, _ = vp.pack_rows([c.v[0] for c in cases], tail=1)
    return dict(q=to_dev(qn, dtype), k=to_dev(kn, dtype), v=to_dev(vn, dtype), cu_q=cu_q, cu_k=cu_k, max_q=max(c.q.shape[2] for c in cases),
                max_k=max(c.k.shape[2] for c in cases), scale=cases[0].scale, dtype=dtype, cases=cases)


def varlen(fa, d, window=None, causal=False):
    import torch

    o, lse = fa.flash_attention_varlen(d["q"], d["k"], d["v"], i32(d["cu_q"]), i32(d["cu_k"]), d["max_q"], d["max_k"], is_causal=causal, window=window,
                                       scale=d["scale"])
    torch.cuda.synchronize()
    return o, lse


def paged(fa, d, P, layout, window=None, causal=False):
    import torch

    pool = vp.build_pool([c.k[0] for c in d["cases"]], [c.v[0] for c in d["cases"]], P, rng=np.random.default_rng(P + len(d["cases"])), spare=2)
    o, lse = fa.flash_attention_varlen_paged(d["q"], to_layout(pool["k"], d["dtype"], layout), to_layout(pool["v"], d["dtype"], layout), i32(d["cu_q"]),
                                             i32(pool["table"]), i32([c.k.shape[2] for c in d["cases"]]), d["max_q"], is_causal=causal, layout=layout,
                                             window=window, scale=d["scale"])
    torch.cuda.synchronize()
    return o, lse


def piece(r, cu_q, b):
    s, e = int(cu_q[b]), int(cu_q[b + 1])
    return r[0][s:e].transpose(0, 1), r[1][:, s:e]


KINDS = [("f16", "shallow"), ("bf16", "shallow"), ("bf16", "steep"), ("bf16", "cliff")]
PREFILL = [(t, s, D, heads) for t, s in KINDS for D, heads in wn.EXACT_MATRIX]


# ---- 1, 2. the packed and the paged prefill ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,slope,D,heads", PREFILL, ids=[f"{t}-{s}-{D}-{h[0]}x{h[1]}" for t, s, D, h in PREFILL])
def test_prefill_window_exact(fa, dtype, slope, D, heads):
    import torch

    for ramp, window, seqs in wn.exact_specs(dtype, slope):
        keys = [(ramp, slope, window, seq, D, heads) for seq in seqs]
        cases = [wn.exact_case(ramp, slope, window, seq, D, heads, dtype) for seq in seqs]
        for c in cases:
            assert ef.representable(c.q, dtype) and ef.representable(c.k, dtype) and ef.representable(c.v, dtype)
        d = pack(cases, dtype)
        dense = varlen(fa, d, window)
        runs = [("fa_fwd_varlen_window", "", dense)] + [("fa_fwd_varlen_paged_window", f" P={P} {layout}", paged(fa, d, P, layout, window))
                                                        for P, layout in ((16, "HND"), (256, "NHD"))]
        for entry, how, r in runs:
            for b, (seq, case, key) in enumerate(zip(seqs, cases, keys)):
                ob, lb = piece(r, d["cu_q"], b)
                hold(case, key, ob.float().cpu().numpy(), lb.cpu().numpy(), entry, f"D={D} {heads} {ramp} {window} {seq}{how}")
                if entry != "fa_fwd_varlen_window" and wn.identity_claimed(*seq):
                    od, ld = piece(dense, d["cu_q"], b)
                    assert torch.equal(bits(ob), bits(od)) and torch.equal(bits(lb), bits(ld)), (how, ramp, window, seq, "differs from the varlen windowed call")


# ---- 3. an unbinding window on deep scores ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [(t, D) for t in ("f16", "bf16") for D in (64, 128)])
def test_an_unbinding_window_on_deep_scores_is_the_unwindowed_call_bit_for_bit(fa, dtype, D):
    import torch

    heads = (8, 2)
    picks = [("shallow", "fall", (63, 0)), ("shallow", "rise", (63, 0))] + ([("steep", "rise", (127, 5)), ("steep", "fall", (127, 5))] if dtype == "bf16" else [])
    for slope, ramp, window in picks:
        seqs = [s for s in wn.EXACT_SEQS if not wn.left_out(slope, dtype, ramp, window, s) and wn.identity_claimed(*s)]
        assert len(seqs) >= 2
        d = pack([wn.exact_case(ramp, slope, window, seq, D, heads, dtype) for seq in seqs], dtype)
        n = int(d["cu_q"][-1])
        for causal, win in ((True, (INT_MAX, 0)), (False, (INT_MAX, INT_MAX))):
            for call in (lambda **kw: varlen(fa, d, **kw), lambda **kw: paged(fa, d, 16, "HND", **kw), lambda **kw: paged(fa, d, 256, "NHD", **kw)):
                new, old = call(window=win), call(causal=causal)
                assert torch.equal(bits(new[0][:n]), bits(old[0][:n])) and torch.equal(bits(new[1][:, :n]), bits(old[1][:, :n])), (slope, ramp, causal)
                assert bool(torch.isfinite(old[0][:n].float()).all()) and bool(torch.isfinite(old[1][:, :n]).all())


# ---- 4. the paged decode ---------------------------------------------------------------------------------------------------------------
DECODE_PAIRS = (("f16", "f16"), ("bf16", "bf16"), ("fp8", "fp8"), ("bf16", "fp8"))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("qdt,kvdt", DECODE_PAIRS)
def test_decode_paged_window_exact(fa, qdt, kvdt, D):
    import torch

    Hq, Hkv = wn.EXACT_DECODE_HEADS
    assert Hq // Hkv == 4
    dtype = "fp8" if kvdt == "fp8" else qdt
    entry = "fa_fwd_decode_paged_window" + ("(kv8)" if qdt != kvdt else "")
    n = 0
    for Nq in wn.DECODE_NQ:
        for window in wn.EXACT_DECODE_WINDOWS:
            for ramp in wn.RAMPS:
                P, layout = ((16, "HND"), (256, "NHD"), (16, "NHD"), (256, "HND"))[n % 4]
                n += 1
                lens = list(wn.EXACT_DECODE_L)
                cases = [wn.decode_case(ramp, window, Nq, L, D, dtype) for L in lens]
                for c in cases:
                    assert ef.representable(c.q, qdt) and ef.representable(c.k, dtype) and ef.representable(c.v, dtype)
                pool = vp.build_pool([c.k[0] for c in cases], [c.v[0] for c in cases], P, rng=np.random.default_rng(P + n), spare=2, max_pages=CAP // P)
                S = dr.paged_splits_of(fa, len(lens), Hq, Hkv, Nq, D, P, CAP // P)
                assert S == min(CAP // 64 // 4, 256)  # from the capacity, not from the lengths
                q = np.concatenate([c.q for c in cases])
                o, lse = fa.flash_attention_decode_paged(to_dev(q, qdt), to_layout(pool["k"], kvdt, layout), to_layout(pool["v"], kvdt, layout),
                                                         i32(pool["table"]), i32(lens), layout=layout, window=window, scale=cases[0].scale)
                torch.cuda.synchronize()
                on, ln = o.float().cpu().numpy(), lse.cpu().numpy()
                for b, (L, case) in enumerate(zip(lens, cases)):
                    hold(case, ("decode", ramp, window, Nq, L, D, dtype), on[b], ln[b], entry, f"D={D} Nq={Nq} L={L} {ramp} {window} P={P} {layout} S={S}", split=S)
