"""GPU: fa_fwd_varlen_mla (the MLA prefill forward, head dims 192 / 128; include/fa_mi355.h) -- every element of O and LSE against the
fp64 references of tests/mla_prefill.py on the cases tests/test_mla_prefill_cases.py holds the bars on; the four tensors under strides of
their own inside sentinel- and NaN-filled buffers; bit-identity with fa_fwd_varlen at D = 128 when the rotary columns are zero; the
separation of the rotary columns; known answers; corrupt tables, lse=None and reproducibility; the chunked-context chain of
INTEGRATION.md against one causal call; a captured graph replayed after the tables and the data changed in place.
Worst error / bar measured on an MI355X over the 16 parity calls (printed by the tests): strict O 3.0e-3 / 6e-3 (bf16), 3.8e-4 / 1.5e-3
(f16); strict LSE 1.1e-6 / 1e-4 (both); the chain: merged against fp64 O 2.7e-3 / 3.9e-2, LSE 9.9e-4 / 1.1e-2 (bf16); see README.md,
round 25."""
import numpy as np
import pytest

import mla_prefill as mp
from util import TORCH_DTYPE

pytestmark = pytest.mark.gpu

DQK, DV, SCALE = mp.DQK, mp.DV, mp.SCALE


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


def _dev(x, dtype):
    import torch

    return torch.from_numpy(np.array(x, copy=True)).to(getattr(torch, TORCH_DTYPE[dtype])).cuda()  # (a copy: the shared cases are read-only)


def _i32(x):
    import torch

    return torch.from_numpy(np.array(x, dtype=np.int32)).cuda()


def _np(o, lse):
    return o.float().cpu().numpy().astype(np.float64), (None if lse is None else lse.cpu().numpy().astype(np.float64))


def _bits(t):
    import torch

    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def run(fa, c, causal, q=None, k=None, v=None, **kw):
    """one packed call on a case's tables; q / k / v: device tensors that take the case's place"""
    import torch

    d = c["dtype"]
    q, k, v = (_dev(c[n], d) if t is None else t for n, t in (("q", q), ("k", k), ("v", v)))
    o, lse = fa.flash_attention_varlen_mla(q, k, v, _i32(c["cu_q"]), _i32(c["cu_k"]), c["max_q"], c["max_k"], is_causal=causal, scale=SCALE, **kw)
    torch.cuda.synchronize()
    return o, lse


# ---- parity: every element of O and LSE, all eight sequences of window.SEQS in one packed call ----------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", mp.DTYPES)
@pytest.mark.parametrize("heads", mp.HEADS)
def test_parity_against_fp64(fa, heads, dtype, causal):
    c = mp.case("seqs", heads, dtype)
    mp.check(*_np(*run(fa, c, causal)), c, causal, ("gpu seqs", heads, dtype, causal))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_parity_at_the_tile_edges(fa, dtype, causal):
    c = mp.case("edges", (8, 2), dtype)
    mp.check(*_np(*run(fa, c, causal)), c, causal, ("gpu edges", dtype, causal))


# ---- layouts: four stride pairs, NaN where nobody may read, sentinels where nobody may write -----------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_strided_views_and_the_write_footprint(fa, dtype, causal):
    import torch

    c = mp.case("seqs", (8, 2), dtype)
    Hq, Hkv = c["heads"]
    tq, tk, extra = len(c["q"]), len(c["k"]), 5  # five more query tokens than the tables own
    tdt = getattr(torch, TORCH_DTYPE[dtype])
    # q: a slice of a wider projection (padded row stride); its unowned tail rows hold NaN
    qbuf = torch.full((tq + extra, Hq * DQK + 64), float("nan"), dtype=tdt, device="cuda")
    q = qbuf[:, :Hq * DQK].view(tq + extra, Hq, DQK)
    q[:tq] = _dev(c["q"], dtype)
    k = _dev(c["k"], dtype)
    # v: the upper 128 columns of the [total_k, Hkv, 256] output of the kv up-projection; the lower 128 hold NaN
    kvbuf = torch.full((tk, Hkv, 256), float("nan"), dtype=tdt, device="cuda")
    v = kvbuf[:, :, 128:]
    v.copy_(_dev(c["v"], dtype))
    assert v.stride() == (Hkv * 256, 256, 1) and q.stride() == (Hq * DQK + 64, DQK, 1)
    # o: inside a wider sentinel-filled buffer (gaps between heads, between rows, and whole rows behind the last token)
    obuf = torch.full((tq + extra + 2, Hq, 160), 77.0, dtype=tdt, device="cuda")
    out = obuf[:tq + extra, :, :DV]
    lse = torch.full((Hq, tq + extra), 55.0, dtype=torch.float32, device="cuda")
    o, l = fa.flash_attention_varlen_mla(q, k, v, _i32(c["cu_q"]), _i32(c["cu_k"]), c["max_q"], c["max_k"], is_causal=causal, scale=SCALE,
                                         out=out, lse=lse)
    torch.cuda.synchronize()
    assert o.data_ptr() == out.data_ptr()
    assert (obuf[:, :, DV:] == 77.0).all() and (obuf[tq:] == 77.0).all() and (lse[:, tq:] == 55.0).all()
    assert torch.isfinite(obuf).all()
    mp.check(*_np(o[:tq], l[:, :tq]), c, causal, ("gpu views", dtype, causal))
    plain = run(fa, c, causal)
    assert _same_bits(o[:tq], plain[0]) and _same_bits(l[:, :tq], plain[1])  # the strides change no bit


# ---- bit-identity with fa_fwd_varlen at D = 128: zero rotary columns add exact zeros behind the eight nope k-steps ---------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_zero_rotary_columns_give_the_bits_of_fa_fwd_varlen(fa, dtype, causal):
    import torch

    c = mp.case("seqs", (8, 2), dtype)
    q, k, v = (_dev(c[n], dtype) for n in "qkv")
    q[:, :, mp.DNOPE:] = 0
    k[:, :, mp.DNOPE:] = 0
    o, lse = run(fa, c, causal, q, k, v)
    o128, lse128 = fa.flash_attention_varlen(q[:, :, :mp.DNOPE].contiguous(), k[:, :, :mp.DNOPE].contiguous(), v, _i32(c["cu_q"]), _i32(c["cu_k"]),
                                             c["max_q"], c["max_k"], is_causal=causal, scale=SCALE)
    torch.cuda.synchronize()
    assert _same_bits(o, o128) and _same_bits(lse, lse128)  # every sequence, dead rows included


@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_the_rotary_columns_of_k_meet_the_rotary_columns_of_q_only(fa, dtype):
    c = mp.case("seqs", (4, 4), dtype)
    q, k = _dev(c["q"], dtype), _dev(c["k"], dtype)
    q[:, :, mp.DNOPE:] = 0
    a = run(fa, c, True, q, k)
    k[:, :, mp.DNOPE:] = 1e4
    b = run(fa, c, True, q, k)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_zero_keys_give_the_mean_of_the_visible_values(fa, dtype, causal):
    import torch

    from util import TOL_LSE, TOL_O

    c = mp.case("seqs", (8, 2), dtype)
    k = torch.zeros((len(c["k"]), 2, DQK), dtype=getattr(torch, TORCH_DTYPE[dtype]), device="cuda")
    o, lse = _np(*run(fa, c, causal, k=k))
    G = c["heads"][0] // c["heads"][1]
    worst_o = worst_l = 0.0
    for b, (Lq, Lk) in enumerate(c["lens"]):
        q0, k0 = c["cu_q"][b], c["cu_k"][b]
        vis = mp.visible(Lq, Lk, causal)
        cnt = vis.sum(1)
        for i in range(Lq):
            if cnt[i] == 0:
                assert (o[q0 + i] == 0).all() and np.isneginf(lse[:, q0 + i]).all()
                continue
            mean = np.repeat(c["v"][k0:k0 + Lk][vis[i]].astype(np.float64).mean(0), G, axis=0)  # [Hq, 128]
            worst_o = max(worst_o, float(np.abs(o[q0 + i] - mean).max()))
            worst_l = max(worst_l, float(np.abs(lse[:, q0 + i] - np.log(cnt[i])).max()))
    print(f"mla_prefill K = 0 ({dtype}, causal={causal}): O {worst_o:.3e} / {TOL_O[dtype]:.3e}  LSE {worst_l:.3e} / {TOL_LSE[dtype]:.3e}")
    assert worst_o < TOL_O[dtype] and worst_l < TOL_LSE[dtype]


@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_a_row_with_one_visible_key_returns_that_value_row(fa, dtype):
    c = mp.case("seqs", (8, 2), dtype)
    v = _dev(c["v"], dtype)
    o, lse = run(fa, c, True, v=v)
    G, seen = c["heads"][0] // c["heads"][1], 0
    for b, (Lq, Lk) in enumerate(c["lens"]):
        if Lq == Lk:  # row 0 of a causal Lq = Lk sequence sees key 0 alone
            want = v[int(c["cu_k"][b])].repeat_interleave(G, dim=0)
            assert _same_bits(o[int(c["cu_q"][b])], want), (b, Lq)
            seen += 1
    assert seen >= 2


# ---- robustness, no side effects --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_corrupt_tables_touch_nothing_they_do_not_own(fa, dtype):
    import torch

    c = mp.case("seqs", (8, 2), dtype)
    Hq, Hkv = c["heads"]
    tq, tk, G, max_q, max_k = len(c["q"]), len(c["k"]), 4, 200, 400
    tdt = getattr(torch, TORCH_DTYPE[dtype])
    # entries of -5 and total + 7 and a decreasing pair: sequences own [0, 50), [50, 250) (300 clamped by max_seqlen_q), [300, total), nothing
    cu_q = [-5, 50, 300, tq + 7, 10]
    cu_k = [-5, 90, 700, tk + 7, 3]
    owned = np.zeros(tq, bool)
    for b in range(4):
        s, e = (min(max(x, 0), tq) for x in cu_q[b:b + 2])
        owned[s:s + min(max(e - s, 0), max_q)] = True
    assert owned[:50].all() and owned[50:250].all() and not owned[250:300].any() and owned[300:500].all() and not owned[500:].any()
    obuf = torch.full((G + tq + G, Hq, DV), 77.0, dtype=tdt, device="cuda")
    lse = torch.full((Hq, tq), 55.0, dtype=torch.float32, device="cuda")
    q, k, v = (_dev(c[n], dtype) for n in "qkv")
    for causal in (False, True):
        fa.flash_attention_varlen_mla(q, k, v, _i32(cu_q), _i32(cu_k), max_q, max_k, is_causal=causal, scale=SCALE, out=obuf[G:G + tq], lse=lse)
        torch.cuda.synchronize()
        assert (obuf[:G] == 77.0).all() and (obuf[G + tq:] == 77.0).all()
        un = torch.from_numpy(~owned).cuda()
        assert (obuf[G:G + tq][un] == 77.0).all() and (lse[:, un] == 55.0).all()
        assert torch.isfinite(obuf).all() and not torch.isnan(lse).any()
        assert not (lse[:, ~un] == 55.0).any()  # every owned token got its LSE


@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_lse_none_and_two_runs_are_bit_identical(fa, dtype):
    c = mp.case("seqs", (4, 4), dtype)
    a, b = run(fa, c, True), run(fa, c, True)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    o, none = run(fa, c, True, return_lse=False)
    assert none is None and _same_bits(o, a[0])


# ---- the chunked-context chain of INTEGRATION.md -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_chunked_context_merges_to_the_single_causal_call(fa, dtype):
    import torch

    from exact_forward import round_to
    from util import TOL_LSE, TOL_O, lse_tol, o_tol

    Hq, Hkv = 8, 2
    rng = np.random.default_rng(2525)
    lens = [(Ln, Lc + Ln) for Ln, Lc in mp.CHAIN]
    tq, tk = sum(a for a, _ in lens), sum(b for _, b in lens)
    q, k, v = (round_to(rng.uniform(-1.0, 1.0, s).astype(np.float32), dtype) for s in ((tq, Hq, DQK), (tk, Hkv, DQK), (tk, Hkv, DV)))
    cu = lambda xs: np.concatenate([[0], np.cumsum(xs)]).astype(np.int32)
    cu_q, cu_k = cu([a for a, _ in lens]), cu([b for _, b in lens])
    # the cached context and the new keys of every sequence, packed apart
    ctx = np.concatenate([np.arange(cu_k[b], cu_k[b] + Lc) for b, (_, Lc) in enumerate(mp.CHAIN)]).astype(np.int64)
    new = np.concatenate([np.arange(cu_k[b] + Lc, cu_k[b + 1]) for b, (_, Lc) in enumerate(mp.CHAIN)]).astype(np.int64)
    cu_c, cu_n = cu([Lc for _, Lc in mp.CHAIN]), cu([Ln for Ln, _ in mp.CHAIN])
    qd, kd, vd = _dev(q, dtype), _dev(k, dtype), _dev(v, dtype)
    mq, mk, mc = max(a for a, _ in lens), max(b for _, b in lens), max(Lc for _, Lc in mp.CHAIN)
    one = fa.flash_attention_varlen_mla(qd, kd, vd, _i32(cu_q), _i32(cu_k), mq, mk, is_causal=True, scale=SCALE)
    a = fa.flash_attention_varlen_mla(qd, _dev(k[ctx], dtype), _dev(v[ctx], dtype), _i32(cu_q), _i32(cu_c), mq, mc, is_causal=False, scale=SCALE)
    b = fa.flash_attention_varlen_mla(qd, _dev(k[new], dtype), _dev(v[new], dtype), _i32(cu_q), _i32(cu_n), mq, mq, is_causal=True, scale=SCALE)
    torch.cuda.synchronize()
    (o1, l1), (oa, la), (ob, lb) = _np(*one), _np(*a), _np(*b)
    om, lm = mp.merge(oa, la, ob, lb)
    # every call's bars against the exact operator on the true Q (util.o_tol / lse_tol on the call's own keys), through the merge formula
    eO = lambda kk, vv: o_tol(dtype, 1, q, kk, vv, SCALE, TOL_O[dtype])
    eL = lambda kk: lse_tol(dtype, 1, q, kk, SCALE, TOL_LSE[dtype])
    bar_o, bar_l = mp.merge_bars(eO(k[ctx], v[ctx]), eL(k[ctx]), eO(k[new], v[new]), eL(k[new]), float(np.abs(v).max()))
    c = dict(name="chain", heads=(Hq, Hkv), dtype=dtype, lens=lens, cu_q=cu_q, cu_k=cu_k, q=q, k=k, v=v)
    ref_o, ref_l = mp.per_sequence(c, lambda qq, kk, vv: mp.reference(qq, kk, vv, True, SCALE))
    e_ref = (float(np.abs(om - ref_o).max()), float(np.abs(lm - ref_l).max()))
    e_one = (float(np.abs(om - o1).max()), float(np.abs(lm - l1).max()))
    print(f"mla_prefill chain ({dtype}): merged vs fp64 O {e_ref[0]:.3e} / {bar_o:.3e} LSE {e_ref[1]:.3e} / {bar_l:.3e}; "
          f"merged vs one call O {e_one[0]:.3e} / {bar_o + eO(k, v):.3e} LSE {e_one[1]:.3e} / {bar_l + eL(k):.3e}")
    assert np.isfinite(om).all() and np.isfinite(lm).all()
    assert e_ref[0] < bar_o and e_ref[1] < bar_l
    assert e_one[0] < bar_o + eO(k, v) and e_one[1] < bar_l + eL(k)  # two approximations of one value: the single call's bars on top


# ---- one captured graph, replayed after both tables and the data changed in place ---------------------------------------------------------
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_graph_replay_after_tables_and_data_change(fa, dtype):
    import torch

    ca, cb = mp.case("edges", (8, 2), dtype), mp.case("edges", (8, 2), dtype)
    lens_b = tuple(reversed(ca["lens"]))  # the same totals and maxima under other tables
    cu = lambda xs: np.concatenate([[0], np.cumsum(xs)]).astype(np.int32)
    q, k, v = (_dev(ca[n], dtype) for n in "qkv")
    cu_q, cu_k = _i32(ca["cu_q"]), _i32(ca["cu_k"])
    o = torch.empty((len(ca["q"]), 8, DV), dtype=q.dtype, device="cuda")
    lse = torch.empty((8, len(ca["q"])), dtype=torch.float32, device="cuda")
    call = lambda: fa.flash_attention_varlen_mla(q, k, v, cu_q, cu_k, ca["max_q"], ca["max_k"], is_causal=True, scale=SCALE, out=o, lse=lse)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    rng = np.random.default_rng(99)
    from exact_forward import round_to

    for lens in (lens_b, ca["lens"]):
        c = dict(cb, lens=lens, cu_q=cu([a for a, _ in lens]), cu_k=cu([b for _, b in lens]),
                 q=round_to(rng.uniform(-1, 1, ca["q"].shape).astype(np.float32), dtype),
                 k=round_to(rng.uniform(-1, 1, ca["k"].shape).astype(np.float32), dtype),
                 v=round_to(rng.uniform(-1, 1, ca["v"].shape).astype(np.float32), dtype))
        cu_q.copy_(_i32(c["cu_q"]))
        cu_k.copy_(_i32(c["cu_k"]))
        for dst, n in ((q, "q"), (k, "k"), (v, "v")):
            dst.copy_(_dev(c[n], dtype))
        o.fill_(float("nan"))
        lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        ref_o, ref_l = mp.per_sequence(c, lambda qq, kk, vv: mp.reference(qq, kk, vv, True, SCALE))
        go, gl = _np(o, lse)
        bo, bl = mp.bars(c)[2:]
        assert np.abs(go - ref_o).max() < bo and np.abs(gl - ref_l).max() < bl, lens
