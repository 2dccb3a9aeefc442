"""GPU: the attention-sink forwards fa_fwd_varlen_sink, fa_fwd_varlen_paged_sink and fa_fwd_decode_paged_sink (sinks= of
flash_attention_varlen / _varlen_paged / _decode_paged). References and bars live in tests/sink.py (held against an fp32 model of the
epilogues, and shown to expose the planted mistakes, by tests/test_sink_cases.py on the CPU):
  1. parity with the fp64 reference element by element, per-head sinks that straddle the scores (-1e4, within the range, +8), at
     lse_bar = lse_tol + fold term, o_bar = o_tol + |O'| lse_bar (include/fa_mi355.h, "Attention sinks"); dead rows exactly O = 0 and
     LSE = sinks[h]; the paged prefill bit for bit the packed call;
  2. sinks = -1e4 everywhere: bit for bit the *_window call;
  3. known answers: K = 0, n visible keys, sinks[h] = k fp32(ln 2): LSE = ln(n + 2^k), O = sum v / (n + 2^k);
  4. range: sinks of +-60 and +-100, finite and inside the bars;
  5. the decode: Nq 1 / 4, L 0 / 1 / 63 / 200 / 1000, both layouts, four dtype pairs, NaN in unused slots, empty splits, both loops of
     the combine (16 and 5 splits).

Worst error / bar measured on an MI355X (printed by the parity tests): O 0.11, LSE 0.33; decode O 0.10, LSE 0.34."""
import numpy as np
import pytest

import chain_bound as cb
import sink as sk
import varlen_paged as vp
import window as wn
from test_gpu_decode_paged import to_layout
from test_gpu_window import data, decode, decode_batch, paged, paged_config, piece, refs, same_bits, varlen
from util import TOL_O, lse_tol, o_tol, to_dev

pytestmark = pytest.mark.gpu
INT_MAX = wn.INT_MAX
MATRIX = [(t, d) for t in ("f16", "bf16") for d in (64, 128)]


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


def dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def ratio(err, bar):
    return float((err / bar).max()) if err.size else 0.0


def check_parity(d, r, wl, wr, sinks, what):
    """Every sequence of the batch against the fp64 reference, element by element. Returns the worst error / bar (O, LSE)."""
    dtype, worst = d["dtype"], [0.0, 0.0]
    for b, (Lq, Lk) in enumerate(d["lens"]):
        q, k, v = d["seqs"][b]
        ob, lb = piece(r, d["cu_q"], b)
        on, ln = ob.float().cpu().numpy(), lb.cpu().numpy()
        o64, l64 = refs(d, wl, wr)[b]
        o2, l2 = sk.fold(o64, l64, sinks)
        dead = wn.dead_rows(Lq, Lk, wl, wr)
        assert not on[:, dead].any() and np.array_equal(ln[:, dead].view(np.int32), np.repeat(sinks[:, None], dead.sum(), 1).view(np.int32)), \
            (what, b, "dead rows: O = 0 and LSE = sinks[h], bit for bit")
        assert np.isfinite(on).all() and np.isfinite(ln).all(), (what, b)
        if Lk == 0:
            continue
        bar_o, bar_l = sk.bars(lse_tol(dtype, 1, q, k), o_tol(dtype, 1, q, k, v, None, TOL_O[dtype]), o2, l64, l2, sinks)
        ro, rl = ratio(np.abs(on - o2), bar_o), ratio(np.abs(ln - l2), bar_l)
        assert ro <= 1.0 and rl <= 1.0, (what, b, (Lq, Lk), "error / bar", ro, rl)
        worst = [max(worst[0], ro), max(worst[1], rl)]
    return worst


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", MATRIX)
def test_parity_with_the_fp64_reference(fa, oracle_mod, dtype, D):
    worst = [0.0, 0.0]
    for heads in wn.HEADS:
        d = data(oracle_mod, dtype, D, heads)
        sinks = sk.sinks_for(heads[0])
        for n, (wl, wr) in enumerate(sk.WINDOWS):
            a = varlen(fa, d, (wl, wr), sinks=dev(sinks))
            w1 = check_parity(d, a, wl, wr, sinks, ("varlen", dtype, D, heads, (wl, wr)))
            P, layout = paged_config(n)
            p = paged(fa, d, P, layout, (wl, wr), sinks=dev(sinks))
            w2 = check_parity(d, p, wl, wr, sinks, ("paged", P, layout, dtype, D, heads, (wl, wr)))
            worst = [max(worst[0], w1[0], w2[0]), max(worst[1], w1[1], w2[1])]
            for b, (Lq, Lk) in enumerate(d["lens"]):  # the paged prefill is the packed call, bit for bit
                if Lk >= Lq >= 1:
                    assert same_bits(piece(p, d["cu_q"], b), piece(a, d["cu_q"], b)), ("paged != packed", heads, (wl, wr), b)
    print(f"SINK parity {dtype} D={D}: worst error / bar O {worst[0]:.3f} LSE {worst[1]:.3f}")
    assert worst[0] > 0.01  # the bars are not vacuous


def test_window_none_and_the_wrapper(fa, oracle_mod):
    d = data(oracle_mod, "bf16", 64, (8, 2))
    s = dev(sk.sinks_for(8))
    for call in (lambda **kw: varlen(fa, d, **kw), lambda **kw: paged(fa, d, 16, "HND", **kw)):
        assert same_bits(call(window=None, causal=True, sinks=s), call(window=(-1, 0), sinks=s))
        assert same_bits(call(window=None, sinks=s), call(window=(-1, -1), sinks=s))
        assert same_bits(call(window=(63, -1), causal=True, sinks=s), call(window=(63, 0), sinks=s))
        assert same_bits(call(window=(63, 0), sinks=s.double()), call(window=(63, 0), sinks=s))  # any float dtype: cast to fp32
        nol = call(window=(63, 0), sinks=s, return_lse=False)
        assert nol[1] is None and same_bits((nol[0], None), call(window=(63, 0), sinks=s))
        with pytest.raises(ValueError):
            call(window=(63, 0), sinks=s[:4])


# ---- 2. a sink that adds nothing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", MATRIX)
def test_sinks_far_below_every_score_change_no_bit(fa, oracle_mod, dtype, D):
    for heads in wn.HEADS:
        d = data(oracle_mod, dtype, D, heads)
        s = dev(np.full(heads[0], -1e4, np.float32))
        for n, (wl, wr) in enumerate(sk.WINDOWS):
            # the same kernels' window mode under the same host clamp: an unbounded side of the sink call is the never-binding width
            twin = (INT_MAX if wl < 0 else wl, INT_MAX if wr < 0 else wr)
            P, layout = paged_config(n)
            for new, old, route in ((varlen(fa, d, (wl, wr), sinks=s), varlen(fa, d, twin), "varlen"),
                                    (paged(fa, d, P, layout, (wl, wr), sinks=s), paged(fa, d, P, layout, twin), "paged")):
                for b, (Lq, Lk) in enumerate(d["lens"]):
                    (on, ln), (oo, lo) = piece(new, d["cu_q"], b), piece(old, d["cu_q"], b)
                    live = ~wn.dead_rows(Lq, Lk, wl, wr)
                    assert same_bits((on[:, live], ln[:, live]), (oo[:, live], lo[:, live])), (route, heads, (wl, wr), b)
                    assert not bool(on[:, ~live].any()) and bool((ln[:, ~live] == -1e4).all()), (route, heads, (wl, wr), b, "dead rows")


# ---- 3. known answers ----------------------------------------------------------------------------------------------------------------
KNOWN_SEQS = ((130, 257), (200, 130), (64, 0))
KNOWN_WINDOWS = ((-1, 0), (-1, -1), (15, 0), (64, 64), (127, 5), (200, 0))


@pytest.mark.parametrize("dtype,D", MATRIX)
def test_known_answers_with_zero_keys_and_power_of_two_sinks(fa, oracle_mod, dtype, D):
    Hq, Hkv = 8, 2
    d = data(oracle_mod, dtype, D, (Hq, Hkv), lens=KNOWN_SEQS, seed=3)
    kz = to_dev(np.zeros_like(d["kn"]), dtype)
    ks = np.arange(Hq) - 2  # 2^k = 1/4 .. 32
    sinks = (ks * np.float32(np.log(2.0))).astype(np.float32)
    for wl, wr in KNOWN_WINDOWS:
        for r, what in ((varlen(fa, d, (wl, wr), k=kz, sinks=dev(sinks)), "varlen"),
                        (paged(fa, d, 16, "NHD", (wl, wr), sinks=dev(sinks),
                               pool=_zero_k_pool(d, 16, "NHD")), "paged")):
            for b, (Lq, Lk) in enumerate(KNOWN_SEQS):
                on, ln = (x.float().cpu().numpy() for x in piece(r, d["cu_q"], b))
                vis = wn.visible(Lq, Lk, wl, wr) if Lk else np.zeros((Lq, 0), bool)
                n = vis.sum(1).astype(np.float64)
                dead = n == 0
                assert not on[:, dead].any() and np.array_equal(ln[:, dead].view(np.int32), np.repeat(sinks[:, None], dead.sum(), 1).view(np.int32)), \
                    (what, (wl, wr), b, "dead rows")
                if Lk == 0:
                    continue
                v = np.repeat(d["seqs"][b][2].astype(np.float64), Hq // Hkv, axis=0)  # [Hq, Lk, D]
                den = n[None, :] + 2.0 ** ks[:, None]
                o2 = np.einsum("ij,hjd->hid", vis.astype(np.float64), v) / den[..., None]
                A = np.einsum("ij,hjd->hid", vis.astype(np.float64), np.abs(v)) / den[..., None]
                with np.errstate(divide="ignore"):
                    l64, l2 = np.broadcast_to(np.log(n)[None], den.shape), np.log(den)
                l2 = np.where(dead[None], sinks[:, None].astype(np.float64), l2)
                # every score is 0: m = 0 and l = n exactly, every probability is 1 in the type. What is left is the fold, the fp32 sums over
                # the n values (one addition per key, one pass per tile) and the rounding of O to the type
                bar_l = sk.fold_term(l64, l2, sinks)
                out_round = np.maximum(cb.U_OUT[dtype] * np.abs(o2), 2.0 ** -25 if dtype == "f16" else 0.0)
                bar_o = out_round + 2.0 ** -24 * (n[None, :, None] + 8) * A + np.abs(o2) * bar_l[..., None]
                live = ~dead
                ro, rl = float((np.abs(on - o2)[:, live] / bar_o[:, live]).max()), float((np.abs(ln - l2)[:, live] / bar_l[:, live]).max())
                assert ro <= 1.0 and rl <= 1.0, (what, (wl, wr), (Lq, Lk), "error / bar", ro, rl)


def _zero_k_pool(d, P, layout):
    ks = [np.zeros_like(s[1]) for s in d["seqs"]]
    pool = vp.build_pool(ks, [s[2] for s in d["seqs"]], P, rng=np.random.default_rng(P), spare=2, fill=0.0)
    return to_layout(pool["k"], d["dtype"], layout), to_layout(pool["v"], d["dtype"], layout), pool["table"]


# ---- 4. range --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_sinks_far_above_and_below_stay_finite_and_inside_the_bars(fa, oracle_mod, dtype, D):
    d = data(oracle_mod, dtype, D, (8, 2))
    for value in (60.0, -60.0, 100.0, -100.0):
        sinks = np.full(8, value, np.float32)
        for wl, wr in ((-1, 0), (127, 5)):
            check_parity(d, varlen(fa, d, (wl, wr), sinks=dev(sinks)), wl, wr, sinks, ("range varlen", value, (wl, wr)))
            check_parity(d, paged(fa, d, 256, "NHD", (wl, wr), sinks=dev(sinks)), wl, wr, sinks, ("range paged", value, (wl, wr)))


# ---- 5. decode ---------------------------------------------------------------------------------------------------------------------------
DECODE_L = (0, 1, 63, 200, 1000)
DECODE_WINDOWS = ((-1, 0), (-1, -1), (63, 0), (200, 5))
DECODE_CASES = [  # qdt, kvdt, D, Hq, Hkv, Nq, P, layout, capacity: 16 splits at 4096 keys (the combine's unrolled loop), 5 at 1280 (its tail)
    ("f16", "f16", 64, 8, 2, 1, 16, "HND", 4096), ("bf16", "bf16", 128, 8, 2, 4, 256, "NHD", 4096), ("fp8", "fp8", 64, 8, 2, 4, 16, "HND", 1280),
    ("bf16", "fp8", 128, 8, 2, 1, 256, "NHD", 1280), ("bf16", "bf16", 64, 8, 1, 4, 16, "HND", 1280), ("f16", "f16", 128, 16, 2, 4, 256, "NHD", 4096),
]


def nan_pool(ks, vs, kvdt, P, layout, cap):
    """Pages in random order, NaN in every slot no key occupies (the tail of a last page, the spare pages)."""
    pool = vp.build_pool(ks, vs, P, rng=np.random.default_rng(P + cap), spare=2, fill=np.nan, max_pages=cap // P)
    return to_layout(pool["k"], kvdt, layout), to_layout(pool["v"], kvdt, layout), pool["table"]


@pytest.mark.parametrize("qdt,kvdt,D,Hq,Hkv,Nq,P,layout,cap", DECODE_CASES)
def test_decode_parity_dead_rows_and_the_window_calls_bits(fa, oracle_mod, qdt, kvdt, D, Hq, Hkv, Nq, P, layout, cap):
    lens = list(DECODE_L)
    q, ks, vs = decode_batch(oracle_mod, qdt, kvdt, D, Hq, Hkv, Nq, P, layout, lens=DECODE_L, seed=18)
    pool = nan_pool(ks, vs, kvdt, P, layout, cap)
    # the workspace is sized for the call's split count: 16 at a capacity of 4096 keys, 5 at 1280 (csrc/fa_decode_kernel.hip, decode_splits)
    S = fa.decode_paged_workspace_bytes(len(lens), Hq, Hkv, Nq, D, P, cap // P) // (len(lens) * Hkv * (32 if (Hq // Hkv) * Nq > 16 else 16) * (D + 2) * 4)
    assert S == (16 if cap == 4096 else 5)
    bar = "bf16" if "fp8" in (qdt, kvdt) else qdt
    base_o = (2 if kvdt == "fp8" else 1) * TOL_O[bar]  # (an e4m3 cache at twice the amplitude, as tests/test_gpu_window.py)
    sinks = sk.sinks_for(Hq)
    worst = [0.0, 0.0]
    for wl, wr in DECODE_WINDOWS:
        o, lse = decode(fa, q, qdt, pool, lens, layout, (wl, wr), sinks=dev(sinks))
        on, ln = o.float().cpu().numpy(), lse.cpu().numpy()
        assert np.isfinite(on).all() and np.isfinite(ln).all(), (wl, wr)
        for b, L in enumerate(lens):
            o64, l64 = wn.reference(q[b], ks[b], vs[b], wl, wr)
            o2, l2 = sk.fold(o64, l64, sinks)
            dead = wn.dead_rows(Nq, L, wl, wr)
            assert not on[b][:, dead].any() and np.array_equal(ln[b][:, dead].view(np.int32), np.repeat(sinks[:, None], dead.sum(), 1).view(np.int32)), \
                ((wl, wr), L, "dead rows")
            if L == 0:
                continue
            bar_o, bar_l = sk.bars(lse_tol(bar, 1, q[b], ks[b]), o_tol(bar, 1, q[b], ks[b], vs[b], None, base_o), o2, l64, l2, sinks)
            ro, rl = ratio(np.abs(on[b] - o2), bar_o), ratio(np.abs(ln[b] - l2), bar_l)
            assert ro <= 1.0 and rl <= 1.0, ((wl, wr), L, "error / bar", ro, rl)
            worst = [max(worst[0], ro), max(worst[1], rl)]
        # sinks at -1e4: the windowed call's bits on every row with a visible key (the same partial kernels, the sink combine)
        low = dev(np.full(Hq, -1e4, np.float32))
        twin = (INT_MAX if wl < 0 else wl, INT_MAX if wr < 0 else wr)
        new, old = decode(fa, q, qdt, pool, lens, layout, (wl, wr), sinks=low), decode(fa, q, qdt, pool, lens, layout, twin)
        for b, L in enumerate(lens):
            live = ~wn.dead_rows(Nq, L, wl, wr)
            assert same_bits((new[0][b][:, live], new[1][b][:, live]), (old[0][b][:, live], old[1][b][:, live])), ((wl, wr), L)
            assert not bool(new[0][b][:, ~live].any()) and bool((new[1][b][:, ~live] == -1e4).all()), ((wl, wr), L)
    print(f"SINK decode {qdt}/{kvdt} D={D} Nq={Nq} P={P} {layout} cap={cap} ({S} splits): worst error / bar O {worst[0]:.3f} LSE {worst[1]:.3f}")
    # the wrapper: window=None is (-1, 0) under is_causal, else (-1, -1)
    s = dev(sinks)
    assert same_bits(decode(fa, q, qdt, pool, lens, layout, None, causal=True, sinks=s), decode(fa, q, qdt, pool, lens, layout, (-1, 0), sinks=s))
    assert same_bits(decode(fa, q, qdt, pool, lens, layout, None, sinks=s), decode(fa, q, qdt, pool, lens, layout, (-1, -1), sinks=s))
