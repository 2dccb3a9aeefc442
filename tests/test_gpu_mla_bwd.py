"""GPU: fa_bwd_varlen_mla (flash_attention_varlen_mla_backward; include/fa_mi355.h, "Multi-head latent attention (prefill, backward)")
on the forward's own small cases (tests/mla_prefill.py), through tests/mla_bwd.py:
  * parity: every element of dq / dk / dv inside the derived bound (no fitted factor), on the oracle's O and LSE rounded to the type --
    all eight sequences of mla_prefill.SEQS in one call (dead rows, Lk = 0, Lq > Lk, 1000 keys), and the tile-edge lengths;
  * bit-identity with fa_bwd_varlen at D = 128 under zero rotary columns, the rotary gradient columns exactly zero;
  * the four stride pairs at once, NaN where nobody may read and sentinels where nobody may write, bit-equal to the contiguous call;
  * exact probes: one visible key per row, dO = 0, the separation of the rotary columns;
  * robustness: a NaN workspace and NaN in unowned tokens, corrupt tables, max_seqlen above the true lengths, two runs;
  * a captured graph replayed after tables and data changed in place; the chain behind fa_fwd_varlen_mla; autograd through the op."""
import numpy as np
import pytest

import mla_bwd as mb
import mla_prefill as mp
from util import TORCH_DTYPE

pytestmark = pytest.mark.gpu

DQK, DV, DNOPE, SCALE = mp.DQK, mp.DV, mp.DNOPE, mp.SCALE


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


def _dev(x, dtype):
    import torch

    return torch.from_numpy(np.array(x, copy=True, order="C")).to(getattr(torch, TORCH_DTYPE[dtype])).cuda()  # (a contiguous copy: the shared cases are read-only)


def _f32(x):
    import torch

    return torch.from_numpy(np.array(x, dtype=np.float32, order="C")).cuda()


def _i32(x):
    import torch

    return torch.from_numpy(np.array(x, dtype=np.int32)).cuda()


def _same_bits(a, b):
    import torch

    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def inputs(c, causal):
    """device q, k, v, o, do, lse of a case: O and LSE the oracle's, O rounded to the type (dead rows: 0 and -inf)"""
    d = c["dtype"]
    q, k, v, do = _dev(c["q"], d), _dev(c["k"], d), _dev(c["v"], d), _dev(mb.d_out(c), d)
    return q, k, v, _dev(mb.packed(c, causal, "o"), d), do, _f32(mb.packed(c, causal, "lse"))


def backward(fa, c, causal, t, **kw):
    import torch

    q, k, v, o, do, lse = t
    g = fa.flash_attention_varlen_mla_backward(q, k, v, o, do, lse, _i32(kw.pop("cu_q", c["cu_q"])), _i32(kw.pop("cu_k", c["cu_k"])),
                                               kw.pop("max_q", c["max_q"]), kw.pop("max_k", c["max_k"]), is_causal=causal, scale=SCALE, **kw)
    torch.cuda.synchronize()
    return g


def check(g, c, causal, where, chain=False):
    """every sequence: finite, inside the bound element by element (a bound of 0 asks for the exact value); prints the worst ratio"""
    worst = 0.0
    for b in range(len(c["lens"])):
        sb = mb.seq_bounds(c, b, causal, chain)
        q0, q1, k0, k1 = c["cu_q"][b], c["cu_q"][b + 1], c["cu_k"][b], c["cu_k"][b + 1]
        got = [x.cpu().numpy().astype(np.float64).transpose(1, 0, 2) for x in (g[0][q0:q1], g[1][k0:k1], g[2][k0:k1])]
        r = mb.worst_ratio(got, sb)
        worst = max(worst, r)
        assert r <= 1.0, (where, b, c["lens"][b], "error / bound", r)
        assert not got[0][:, :sb.n0].any(), (where, b, "dQ of a row without a visible key must be 0 exactly")
        if sb.n0 >= c["lens"][b][0]:
            assert not got[1].any() and not got[2].any(), (where, b, "dK / dV of keys no query sees must be 0 exactly")
    print(f"mla_bwd {where}: worst error / bound {worst:.3f}")
    return worst


# ---- parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,heads,dtype,causal", mb.PARITY)
def test_parity_against_fp64_inside_the_bound(fa, name, heads, dtype, causal):
    c = mp.case(name, heads, dtype)
    check(backward(fa, c, causal, inputs(c, causal)), c, causal, ("gpu", name, heads, dtype, causal))


# ---- bit-identity with fa_bwd_varlen at D = 128 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_zero_rotary_columns_give_the_bits_of_fa_bwd_varlen(fa, dtype, causal):
    import torch

    c = mp.case("seqs", (8, 2), dtype)
    q, k, v, o, do, lse = inputs(c, causal)
    q[:, :, DNOPE:] = 0
    k[:, :, DNOPE:] = 0
    dq, dk, dv = backward(fa, c, causal, (q, k, v, o, do, lse))
    r = fa.flash_attention_varlen_backward(q[:, :, :DNOPE].contiguous(), k[:, :, :DNOPE].contiguous(), v, o, do, lse, _i32(c["cu_q"]), _i32(c["cu_k"]),
                                           c["max_q"], c["max_k"], is_causal=causal, scale=SCALE)
    torch.cuda.synchronize()
    for b, (Lq, Lk) in enumerate(c["lens"]):  # per sequence; only owned tokens are written by either call, and every token is owned here
        q0, q1, k0, k1 = c["cu_q"][b], c["cu_q"][b + 1], c["cu_k"][b], c["cu_k"][b + 1]
        assert _same_bits(dq[q0:q1, :, :DNOPE], r[0][q0:q1]), (b, "dQ")
        assert _same_bits(dk[k0:k1, :, :DNOPE], r[1][k0:k1]), (b, "dK")
        assert _same_bits(dv[k0:k1], r[2][k0:k1]), (b, "dV")
    assert not bool(dq[:, :, DNOPE:].any()) and not bool(dk[:, :, DNOPE:].any())  # the rotary gradient columns are exactly zero


# ---- strides ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_strided_views_and_the_write_footprint(fa, dtype, causal):
    import torch

    c = mp.case("seqs", (8, 2), dtype)
    Hq, Hkv = c["heads"]
    tq, tk, extra = len(c["q"]), len(c["k"]), 5  # five more tokens than the tables own, on both sides
    tdt = getattr(torch, TORCH_DTYPE[dtype])
    nan, S = float("nan"), 77.0
    t = inputs(c, causal)
    plain = backward(fa, c, causal, t)
    # q: a slice of a wider projection; v: the upper half of a NaN-filled [total_k, Hkv, 256] buffer; o / d_o inside wider buffers
    qbuf = torch.full((tq + extra, Hq * DQK + 64), nan, dtype=tdt, device="cuda")
    q = qbuf[:, :Hq * DQK].view(tq + extra, Hq, DQK)
    q[:tq] = t[0]
    kbuf = torch.full((tk + extra, Hkv, DQK + 8), nan, dtype=tdt, device="cuda")
    k = kbuf[:, :, :DQK]
    k[:tk] = t[1]
    kvbuf = torch.full((tk + extra, Hkv, 256), nan, dtype=tdt, device="cuda")
    v = kvbuf[:, :, 128:]
    v[:tk] = t[2]
    obuf, dobuf = (torch.full((tq + extra, Hq, 160), nan, dtype=tdt, device="cuda") for _ in range(2))
    o, do = obuf[:, :, :DV], dobuf[:, :, :DV]
    o[:tq], do[:tq] = t[3], t[4]
    lse = torch.full((Hq, tq + extra), nan, dtype=torch.float32, device="cuda")
    lse[:, :tq] = t[5]
    # the gradients into sentinel-filled fp32 buffers of those shapes
    gq, gk, gv = (torch.full(x.shape, S, dtype=torch.float32, device="cuda") for x in (qbuf, kbuf, kvbuf))
    dq, dk, dv = gq[:, :Hq * DQK].view(tq + extra, Hq, DQK), gk[:, :, :DQK], gv[:, :, 128:]
    assert dq.stride() == q.stride() and dk.stride() == k.stride() and dv.stride() == v.stride() == (Hkv * 256, 256, 1)
    ws = torch.full((fa.varlen_backward_workspace_bytes(Hq, tq + extra),), 0xFF, dtype=torch.uint8, device="cuda")
    out = backward(fa, c, causal, (q, k, v, o, do, lse), dq=dq, dk=dk, dv=dv, workspace=ws)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, (dq, dk, dv)))
    assert _same_bits(dq[:tq], plain[0]) and _same_bits(dk[:tk], plain[1]) and _same_bits(dv[:tk], plain[2])  # the strides change no bit
    # every byte outside the owned elements is untouched
    assert bool((gq[:, Hq * DQK:] == S).all()) and bool((gq[tq:] == S).all())
    assert bool((gk[:, :, DQK:] == S).all()) and bool((gk[tk:] == S).all())
    assert bool((gv[:, :, :128] == S).all()) and bool((gv[tk:] == S).all())


# ---- exact probes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_one_visible_key_per_row(fa, dtype, causal):
    # every sequence has ONE key: P = 1 on the rows that see it, O = v, and with dO in quarters and v in eighths dP - delta is exactly 0
    # in any order of summation: dQ = dK = 0 exactly, and the key's dV row is the exact sum of the dO rows that see it (all rows
    # without the mask, the last row under it) over the key head's group. q is nonzero in 8 columns and at most 1/2, so that exp2 of the
    # operand rounding stays below half an ulp of the type around 1.
    import torch

    Hq, Hkv, lens = 8, 2, ((5, 1), (129, 1), (1, 1), (64, 1))
    rng = np.random.default_rng(91)
    tq, tk = sum(a for a, _ in lens), len(lens)
    q = np.zeros((tq, Hq, DQK), np.float32)
    q[:, :, [3, 40, 77, 127, 128, 150, 171, 191]] = rng.integers(-4, 5, (tq, Hq, 8)) / 8.0
    k = rng.integers(-8, 9, (tk, Hkv, DQK)) / 8.0
    v = rng.integers(-8, 9, (tk, Hkv, DV)) / 8.0
    do = rng.integers(-16, 17, (tq, Hq, DV)) / 4.0
    cu_q, cu_k = np.cumsum([0] + [a for a, _ in lens]), np.arange(tk + 1)
    G = Hq // Hkv
    sees = np.zeros(tq, bool)
    for b, (Lq, _) in enumerate(lens):
        sees[(cu_q[b + 1] - 1 if causal else cu_q[b]):cu_q[b + 1]] = True
    kb = np.repeat(np.arange(tk), [a for a, _ in lens])  # the key of a token
    lse = np.where(sees[None], SCALE * np.einsum("thd,thd->ht", q.astype(np.float64), np.repeat(k, G, axis=1)[kb]), -np.inf)
    o = np.where(sees[:, None, None], np.repeat(v, G, axis=1)[kb], 0.0)
    want_dv = np.zeros((tk, Hkv, DV))
    for t_ in np.nonzero(sees)[0]:
        want_dv[kb[t_]] += do[t_].reshape(Hkv, G, DV).sum(1)
    dq, dk, dv = fa.flash_attention_varlen_mla_backward(*(_dev(x, dtype) for x in (q, k, v, o, do)), _f32(lse), _i32(cu_q), _i32(cu_k), 129, 1,
                                                        is_causal=causal, scale=SCALE)
    torch.cuda.synchronize()
    assert not bool(dq.any()) and not bool(dk.any())
    assert np.array_equal(dv.cpu().numpy().astype(np.float64), want_dv)


@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_zero_d_out_gives_three_zero_gradients(fa, dtype):
    c = mp.case("seqs", (8, 2), dtype)
    t = list(inputs(c, True))
    t[4] = t[4] * 0
    assert all(not bool(g.any()) for g in backward(fa, c, True, t))


@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_the_rotary_columns_of_k_meet_the_rotary_columns_of_q_only(fa, dtype):
    c = mp.case("seqs", (4, 4), dtype)
    t = list(inputs(c, True))
    t[0][:, :, DNOPE:] = 0
    a = backward(fa, c, True, t)
    t[1] = t[1].clone()
    t[1][:, :, DNOPE:] = 1e4
    b = backward(fa, c, True, t)
    assert _same_bits(a[0][:, :, :DNOPE], b[0][:, :, :DNOPE]) and _same_bits(a[1][:, :, :DNOPE], b[1][:, :, :DNOPE]) and _same_bits(a[2], b[2])


# ---- robustness -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,causal", [("bf16", True), ("f16", False)])
def test_nan_workspace_and_nan_in_unowned_tokens_change_nothing(fa, dtype, causal):
    import torch

    c = mp.case("seqs", (8, 2), dtype)
    Hq = c["heads"][0]
    tq, tk = len(c["q"]), len(c["k"])
    t = inputs(c, causal)
    plain = backward(fa, c, causal, t)

    def tail(x, n, dim=0):  # n tokens behind the last sequence, owned by nobody, filled with NaN
        shape = list(x.shape)
        shape[dim] = n
        return torch.cat([x, torch.full(shape, float("nan"), dtype=x.dtype, device="cuda")], dim=dim).contiguous()

    t2 = (tail(t[0], 40), tail(t[1], 70), tail(t[2], 70), tail(t[3], 40), tail(t[4], 40), tail(t[5], 40, 1))
    ws = torch.full((fa.varlen_backward_workspace_bytes(Hq, tq + 40),), 0xFF, dtype=torch.uint8, device="cuda")
    grads = tuple(torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda") for x in t2[:3])
    backward(fa, c, causal, t2, dq=grads[0], dk=grads[1], dv=grads[2], workspace=ws)
    for g, p, n in zip(grads, plain, (tq, tk, tk)):
        assert bool(torch.isfinite(g[:n]).all()) and _same_bits(g[:n], p)
        assert bool(torch.isnan(g[n:]).all())  # not written


@pytest.mark.parametrize("dtype,causal", [("bf16", True), ("f16", False)])
def test_corrupt_tables_write_nothing_they_do_not_own(fa, dtype, causal):
    import torch

    # -5 and total + 7 are clamped to [0, total]; the decreasing pair (total + 7 -> 300) is an empty sequence: the call is the one on the
    # tables [0, 100, total, total], and the ten tokens behind `total` (inside the buffers, outside total_q / total_k) keep their sentinel
    c = mp.case("seqs", (4, 4), dtype)
    tq, tk = len(c["q"]), len(c["k"])
    q, k, v, o, do, lse = inputs(c, causal)
    o, lse = o * 0, lse * 0 + 1.0  # (any finite O / LSE: the tables below are not the oracle's)
    clean = backward(fa, c, causal, (q, k, v, o, do, lse), cu_q=[0, 100, tq, tq], cu_k=[0, 100, tk, tk], max_q=tq, max_k=tk)
    S = 77.0
    bufs = tuple(torch.full((n + 10,) + tuple(x.shape[1:]), S, dtype=torch.float32, device="cuda") for n, x in ((tq, q), (tk, k), (tk, v)))
    lib = fa.load_library()
    cu_q, cu_k = _i32([-5, 100, tq + 7, 300]), _i32([-5, 100, tk + 7, 300])
    ws = torch.zeros(fa.varlen_backward_workspace_bytes(4, tq), dtype=torch.uint8, device="cuda")
    st = lib.fa_bwd_varlen_mla(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), bufs[0].data_ptr(),
                               bufs[1].data_ptr(), bufs[2].data_ptr(), ws.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), 3, 4, 4, tq, tk, tq, tk,
                               DQK, DV, SCALE, *q.stride()[:2], *k.stride()[:2], *v.stride()[:2], *o.stride()[:2], int(causal),
                               {"f16": 1, "bf16": 2}[dtype], None)
    torch.cuda.synchronize()
    assert st == 0, lib.fa_last_error()
    for buf, ref, n in zip(bufs, clean, (tq, tk, tk)):
        assert bool((buf[n:] == S).all()) and _same_bits(buf[:n], ref)


@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_max_seqlen_above_the_true_lengths_and_a_second_run_change_no_bit(fa, dtype):
    c = mp.case("seqs", (8, 2), dtype)
    t = inputs(c, True)
    a = backward(fa, c, True, t)
    b = backward(fa, c, True, t, max_q=len(c["q"]), max_k=len(c["k"]))  # more blocks, all of which own nothing
    a2 = backward(fa, c, True, t)
    assert all(_same_bits(x, y) and _same_bits(x, z) for x, y, z in zip(a, b, a2))


# ---- one captured graph, replayed after the tables and the data changed in place -----------------------------------------------------------
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_graph_replay_after_tables_and_data_change(fa, dtype):
    import torch

    c = mp.case("seqs", (8, 2), dtype)
    Hq, Hkv = c["heads"]
    tq, tk = len(c["q"]), len(c["k"])
    q, k, v, do = _dev(c["q"], dtype), _dev(c["k"], dtype), _dev(c["v"], dtype), _dev(mb.d_out(c), dtype)
    splits = [(list(c["cu_q"]), list(c["cu_k"])), ([0, 300, 300, 310, 400, 500, 600, 700, tq], [0, 500, 600, 600, 900, 1000, 1500, 1600, tk])]
    cu_q, cu_k = _i32(splits[0][0]), _i32(splits[0][1])
    o = torch.zeros(tq, Hq, DV, dtype=q.dtype, device="cuda")
    lse = torch.empty(Hq, tq, dtype=torch.float32, device="cuda")
    dq, dk, dv = (torch.empty(x.shape, dtype=torch.float32, device="cuda") for x in (q, k, v))
    ws = torch.empty(fa.varlen_backward_workspace_bytes(Hq, tq), dtype=torch.uint8, device="cuda")

    def step():  # forward and backward, nothing allocated, no device value read
        fa.flash_attention_varlen_mla(q, k, v, cu_q, cu_k, tq, tk, is_causal=True, scale=SCALE, out=o, lse=lse)
        fa.flash_attention_varlen_mla_backward(q, k, v, o, do, lse, cu_q, cu_k, tq, tk, is_causal=True, scale=SCALE, dq=dq, dk=dk, dv=dv, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for i, (sq, sk) in enumerate((splits[1], splits[0], splits[1])):
        cu_q.copy_(_i32(sq))
        cu_k.copy_(_i32(sk))
        q.copy_(q.flip(0))  # the data changes in place as well
        do.copy_(do.flip(1))
        for t in (dq, dk, dv):
            t.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        o2, lse2 = fa.flash_attention_varlen_mla(q, k, v, cu_q, cu_k, tq, tk, is_causal=True, scale=SCALE)
        want = fa.flash_attention_varlen_mla_backward(q, k, v, o2, do, lse2, cu_q, cu_k, tq, tk, is_causal=True, scale=SCALE)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(g).all()) and _same_bits(g, w) for g, w in zip((dq, dk, dv), want)), (i, sq)  # (every token is owned)


# ---- the chain: the backward on the forward's own O and LSE ---------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtype", mp.DTYPES)
def test_chain_behind_the_forward_inside_the_bound(fa, dtype, causal):
    import torch

    c = mp.case("seqs", (8, 2), dtype)
    q, k, v, do = _dev(c["q"], dtype), _dev(c["k"], dtype), _dev(c["v"], dtype), _dev(mb.d_out(c), dtype)
    o, lse = fa.flash_attention_varlen_mla(q, k, v, _i32(c["cu_q"]), _i32(c["cu_k"]), c["max_q"], c["max_k"], is_causal=causal, scale=SCALE)
    torch.cuda.synchronize()
    check(backward(fa, c, causal, (q, k, v, o, do, lse)), c, causal, ("gpu chain", dtype, causal), chain=True)


# ---- autograd through the op ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,causal", [("bf16", True), ("f16", False)])
def test_autograd_through_the_op(fa, dtype, causal):
    import torch

    from flash_attention_metal_amd import torch_op

    c = mp.case("seqs", (8, 2), dtype)
    Hq, Hkv = c["heads"]
    tq, tk = len(c["q"]), len(c["k"])

    def tail(x, n):  # n tokens owned by nobody
        return torch.cat([x, torch.ones((n,) + tuple(x.shape[1:]), dtype=x.dtype, device="cuda")]).contiguous()

    q, k, v, do = tail(_dev(c["q"], dtype), 20), tail(_dev(c["k"], dtype), 30), tail(_dev(c["v"], dtype), 30), tail(_dev(mb.d_out(c), dtype), 20)
    cu_q, cu_k = _i32(c["cu_q"]), _i32(c["cu_k"])
    qg, kg, vg = (t.detach().requires_grad_(True) for t in (q, k, v))
    o, lse = torch_op.attention_varlen_mla(qg, kg, vg, cu_q, cu_k, c["max_q"], c["max_k"], causal, 0.0)  # scale 0.0: 192 ** -0.5
    assert o.shape == (tq + 20, Hq, DV) and lse.shape == (Hq, tq + 20)
    assert not bool(o[tq:].any()) and bool(torch.isneginf(lse[:, tq:]).all())
    gq, gk, gv = torch.autograd.grad(o, (qg, kg, vg), do.transpose(0, 1).contiguous().transpose(0, 1))  # (restrided to o's strides by the op)
    torch.cuda.synchronize()
    o2, lse2 = fa.flash_attention_varlen_mla(q, k, v, cu_q, cu_k, c["max_q"], c["max_k"], is_causal=causal, scale=SCALE)
    assert torch.equal(o2[:tq], o[:tq])
    want = fa.flash_attention_varlen_mla_backward(q, k, v, o.detach(), do, lse.detach(), cu_q, cu_k, c["max_q"], c["max_k"], is_causal=causal, scale=SCALE)
    torch.cuda.synchronize()
    for g, w, x, n in ((gq, want[0], q, tq), (gk, want[1], k, tk), (gv, want[2], v, tk)):
        assert g.dtype == x.dtype and g.shape == x.shape
        assert torch.equal(g[:n], w[:n].to(x.dtype))  # the wrapper's result, bit for bit after the cast
        assert not bool(g[n:].any()), "tokens owned by nobody get a zero gradient"
    o3, lse3 = torch_op.attention_varlen_mla(qg, kg, vg, cu_q, cu_k, c["max_q"], c["max_k"], causal, 0.0)
    with pytest.raises(Exception, match="LSE"):  # no gradient through the LSE output
        lse3[:, :tq].nan_to_num(neginf=0.0).sum().backward()
