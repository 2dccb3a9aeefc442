"""GPU: fa_bwd_varlen_sink (flash_attention_varlen_backward(sinks=...)) on the O / LSE that flash_attention_varlen(sinks=...) wrote, and
the op fa_mi355::attention_varlen_sink. One launch packs all of window.SEQS. Bounds: tests/sink.py (CPU side: tests/test_sink_cases.py).

  * dQ, dK, dV: bit for bit fa_bwd_varlen_window on the same six tensors; every element inside sink.SeqBounds (backward_bound.py on the
    sink-including P and dS, the forward's lse_err / o_err of include/fa_mi355.h "Attention sinks"); dead rows' dQ exactly 0;
  * dsinks: against the fp64 formula on the lse and the workspace's delta it was given (the fp32 bound of the exp and the tree sum), and
    against the fp64 end-to-end gradient (plus the chain bound); sentinels around it; bitwise reproducible; dsinks = NULL changes nothing;
  * NaN in the workspace at unowned tokens and beyond the max_seqlen_q clamp does not reach dsinks;
  * one captured graph of forward and backward, replayed after sinks and tables changed in place;
  * autograd of the op: four gradients, the sinks' in the parameter's dtype; the wrappers' dispatch.

Worst error / bound measured on an MI355X (printed by the tests): dQ / dK / dV 0.42, dsinks 0.065 against the given-input formula and 0.002
end to end; the op's gradients 0.28 (bf16) / 0.77 (f16, after the cast)."""
import math

import numpy as np
import pytest

import backward_bound as bb
import sink as sk
import window as W
import window_backward as wb
from test_gpu_varlen import cu_dev
from test_gpu_varlen_bwd import pack4, seq_piece
from test_gpu_window_bwd import draw_seqs, maxes
from util import to_dev
from varlen_backward import draw_seq

pytestmark = pytest.mark.gpu


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


def fwd_bwd(fa, tensors, grads, cu_q, cu_k, max_q, max_k, window, sinks, dsinks=None, workspace=None, scale=None):
    """Forward and backward with sinks; returns (o, lse, dsinks, workspace as fp32 [Hq, total_q])."""
    import torch

    q, k, v, do = tensors
    s = dev(sinks)
    o, lse = fa.flash_attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), int(max_q), int(max_k), scale=scale, window=window, sinks=s)
    if workspace is None:
        workspace = torch.empty(fa.varlen_backward_workspace_bytes(q.shape[1], q.shape[0]), dtype=torch.uint8, device="cuda")
    out = fa.flash_attention_varlen_backward(q, k, v, o, do, lse, cu_dev(cu_q), cu_dev(cu_k), int(max_q), int(max_k), scale=scale, dq=grads[0],
                                             dk=grads[1], dv=grads[2], workspace=workspace, window=window, sinks=s, dsinks=dsinks)
    torch.cuda.synchronize()
    assert len(out) == 4 and all(a.data_ptr() == b.data_ptr() for a, b in zip(out, grads))
    return o, lse, out[3], workspace.view(torch.float32).view(q.shape[1], q.shape[0])


def check_sequences(seqs, grads, dsinks, lse, delta, cu_q, cu_k, max_q, dtype, wl, wr, sinks, scale, what, cast_to=None, sinks_cast=None):
    """Every sequence inside sink.SeqBounds element by element; dsinks against the given-input formula (lse, delta: what the kernel read;
    None skips it) and against the end-to-end reference. Returns the worst error / bound of (dQ/dK/dV, dsinks given, dsinks end to end)."""
    import torch

    worst, ds_ref, ds_chain = 0.0, np.zeros(len(sinks)), np.zeros(len(sinks))
    for b, seq in enumerate(seqs):
        g = [seq_piece(t, cu, b).float() for t, cu in zip(grads, (cu_q, cu_k, cu_k))]
        assert all(bool(torch.isfinite(x).all()) for x in g), (what, b, "NaN / Inf in a gradient")
        sb = sk.SeqBounds(*seq, wl, wr, sinks, scale, dtype)
        if cast_to is not None:
            # (an f16 value below 2^-14 is subnormal and rounded absolutely, to a multiple of 2^-24: under a sink of +8 the probabilities,
            # and with them many gradient elements, are that small)
            # (where the bound is 0 the gradient is exactly 0 before and after the cast)
            sb.bound = tuple(bd + np.where(bd > 0, np.maximum(bb.U[cast_to] * (np.abs(r) + bd), bb.TINY[cast_to]), 0.0) for r, bd in zip(sb.ref, sb.bound))
        r = wb.worst_ratio([x.cpu().numpy() for x in g], sb)
        assert r <= 1.0, (what, b, (seq[0].shape[1], seq[1].shape[1]), "error / bound", r)
        worst = max(worst, r)
        assert not bool(g[0][:, :sb.n0].any()), (what, b, "dQ of a row without a visible key must be 0 exactly")
        ds_ref += sb.dsink_ref
        ds_chain += sb.dsink_chain
    got = dsinks.double().cpu().numpy()
    assert np.isfinite(got).all(), (what, "dsinks")
    given = 0.0
    fp32 = np.zeros(len(sinks))
    if lse is not None:
        ln, dn = lse.cpu().numpy(), delta.cpu().numpy()
        want, fp32 = sk.dsink_exact(sinks, ln, dn, cu_q, max_q), sk.dsink_bound(sinks, ln, dn, cu_q, max_q)
        with np.errstate(divide="ignore", invalid="ignore"):
            rg = np.where(fp32 > 0, np.abs(got - want) / fp32, np.where(got != want, np.inf, 0.0))
        given = float(rg.max())
        assert given <= 1.0, (what, "dsinks against the fp64 formula on the given lse / delta", rg)
    total = fp32 + ds_chain
    if sinks_cast is not None:
        total = total + sinks_cast * (np.abs(ds_ref) + total)
    with np.errstate(divide="ignore", invalid="ignore"):
        re = np.where(total > 0, np.abs(got - ds_ref) / total, np.where(got != ds_ref, np.inf, 0.0))
    assert float(re.max()) <= 1.0, (what, "dsinks against the end-to-end gradient", re, got, ds_ref)
    return worst, given, float(re.max())


@pytest.mark.parametrize("heads", W.HEADS, ids=lambda h: f"h{h[0]}_{h[1]}")
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_chain_inside_the_bounds_and_bit_identical_to_the_window_backward(fa, dtype, D, heads):
    import torch

    Hq, Hkv = heads
    sinks = sk.sinks_for(Hq)
    worst = [0.0, 0.0, 0.0]
    for ci, (wl, wr) in enumerate(sk.WINDOWS):
        seqs = draw_seqs(1800 + 90 * ci + D + Hq, Hq, Hkv, D, dtype, W.SEQS)
        tensors, grads, cu_q, cu_k = pack4(seqs, dtype, "THD", 5, 3, 0.0)  # trailing tokens nobody owns
        buf = torch.full((Hq + 2,), 777.0, dtype=torch.float32, device="cuda")  # sentinels around dsinks
        o, lse, dsinks, delta = fwd_bwd(fa, tensors, grads, cu_q, cu_k, *maxes(W.SEQS), (wl, wr), sinks, dsinks=buf[1:-1])
        assert float(buf[0]) == 777.0 and float(buf[-1]) == 777.0 and dsinks.data_ptr() == buf[1:].data_ptr()
        # the same six tensors through fa_bwd_varlen_window: the same bits
        _, g2, _, _ = pack4(seqs, dtype, "THD", 5, 3, 0.0)
        q, k, v, do = tensors
        fa.flash_attention_varlen_backward(q, k, v, o, do, lse, cu_dev(cu_q), cu_dev(cu_k), *maxes(W.SEQS), dq=g2[0], dk=g2[1], dv=g2[2], window=(wl, wr))
        torch.cuda.synchronize()
        nq, nk = int(cu_q[-1]), int(cu_k[-1])
        for a, c, n in zip(grads, g2, (nq, nk, nk)):
            assert torch.equal(a[:n], c[:n]) and bool(torch.isnan(a[n:]).all()), (wl, wr)
        # reproducible, and written rather than accumulated: a second call into the same buffer
        first = dsinks.clone()
        fwd_bwd(fa, tensors, grads, cu_q, cu_k, *maxes(W.SEQS), (wl, wr), sinks, dsinks=buf[1:-1])
        assert torch.equal(first.view(torch.int32), buf[1:-1].view(torch.int32))
        w = check_sequences(seqs, grads, dsinks, lse, delta, cu_q, cu_k, maxes(W.SEQS)[0], dtype, wl, wr, sinks, None, (dtype, D, heads, (wl, wr)))
        worst = [max(a, c) for a, c in zip(worst, w)]
    print(f"SINK BWD worst error / bound {dtype} D={D} heads={heads}: dQ/dK/dV {worst[0]:.3f} dsinks given {worst[1]:.3f} end to end {worst[2]:.3f}")
    assert worst[0] > 0.01  # the bound is not vacuous


@pytest.mark.parametrize("dtype,D,window", [("bf16", 64, (63, 0)), ("f16", 128, (-1, 0))])
def test_null_dsinks_leaves_the_three_gradients_unchanged(fa, dtype, D, window):
    import torch

    Hq, Hkv = 8, 2
    sinks = sk.sinks_for(Hq)
    seqs = draw_seqs(1861 + D, Hq, Hkv, D, dtype, W.SEQS)
    tensors, g1, cu_q, cu_k = pack4(seqs, dtype, "THD")
    _, g2, _, _ = pack4(seqs, dtype, "THD")
    o, lse, _, _ = fwd_bwd(fa, tensors, g1, cu_q, cu_k, *maxes(W.SEQS), window, sinks)
    q, k, v, do = tensors
    lib, s, cq, ck = fa.load_library(), dev(sinks), cu_dev(cu_q), cu_dev(cu_k)
    ws = torch.empty(fa.varlen_backward_workspace_bytes(Hq, q.shape[0]), dtype=torch.uint8, device="cuda")
    st = lib.fa_bwd_varlen_sink(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), g2[0].data_ptr(),
                                g2[1].data_ptr(), g2[2].data_ptr(), ws.data_ptr(), cq.data_ptr(), ck.data_ptr(), len(W.SEQS), Hq, Hkv, q.shape[0],
                                k.shape[0], *maxes(W.SEQS), D, 1.0 / math.sqrt(D), q.stride(0), q.stride(1), k.stride(0), k.stride(1), *window,
                                s.data_ptr(), None, fa.DTYPES[dtype], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == 0, lib.fa_last_error()
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


@pytest.mark.parametrize("dtype,D,window", [("bf16", 128, (127, 5)), ("f16", 64, (-1, 0))])
def test_nan_in_the_workspace_where_nobody_owns_a_token_does_not_reach_dsinks(fa, dtype, D, window):
    import torch

    # sequence 1 holds 300 rows under max_seqlen_q = 200: its rows 200 .. 299 lie beyond the clamp; 40 trailing tokens belong to nobody
    Hq, Hkv, lens, max_q, max_k = 4, 2, [(70, 70), (300, 300), (130, 257)], 200, 300
    sinks = sk.sinks_for(Hq)
    seqs = draw_seqs(1873 + D, Hq, Hkv, D, dtype, lens)
    tensors, grads, cu_q, cu_k = pack4(seqs, dtype, "THD", 40, 70, float("nan"))
    total_q = tensors[0].shape[0]
    ws = torch.full((fa.varlen_backward_workspace_bytes(Hq, total_q),), 0xFF, dtype=torch.uint8, device="cuda")  # every float a NaN
    o, lse, dsinks, delta = fwd_bwd(fa, tensors, grads, cu_q, cu_k, max_q, max_k, window, sinks, workspace=ws)
    owned = np.zeros(total_q, bool)
    owned[np.concatenate(sk.owned_rows(cu_q, total_q, max_q))] = True
    assert owned.sum() == 70 + 200 + 130
    dn, ln = delta.cpu().numpy(), lse.cpu().numpy()
    assert np.isnan(dn[:, ~owned]).all() and np.isfinite(dn[:, owned]).all(), "delta is written for the owned rows only"
    got = dsinks.double().cpu().numpy()
    assert np.isfinite(got).all()
    ln = np.where(owned[None], ln, np.nan)  # (lse of rows nobody owns is whatever torch.empty held: not read either)
    want, bound = sk.dsink_exact(sinks, ln, dn, cu_q, max_q), sk.dsink_bound(sinks, ln, dn, cu_q, max_q)
    assert (np.abs(got - want) <= bound).all() and (bound[1:] > 0).all(), (got, want, bound)


@pytest.mark.parametrize("dtype,D,window", [("bf16", 64, (127, 0)), ("f16", 128, (-1, 0))])
def test_graph_replay_after_sinks_and_tables_change(fa, dtype, D, window):
    import torch

    Hq, Hkv, total_q, total_k, max_q, max_k = 8, 2, 700, 900, 400, 500
    qn, kn, vn, don = draw_seq(np.random.default_rng(1847 + D), Hq, Hkv, total_q, total_k, D, dtype)
    q, k, v, do = (to_dev(x.transpose(1, 0, 2), dtype) for x in (qn, kn, vn, don))
    splits = [([0, 100, 450, 700], [0, 300, 650, 900]), ([0, 390, 400, 700], [0, 400, 900, 900])]  # (the second: one sequence without keys)
    sink_sets = [sk.sinks_for(Hq), sk.sinks_for(Hq)[::-1].copy()]
    cu_q, cu_k, s = cu_dev(splits[0][0]), cu_dev(splits[0][1]), dev(sink_sets[0])
    o = torch.empty_like(q)
    lse = torch.empty(Hq, total_q, dtype=torch.float32, device="cuda")
    dq, dk, dv = (torch.empty(x.shape, dtype=torch.float32, device="cuda") for x in (q, k, k))
    dsinks = torch.empty(Hq, dtype=torch.float32, device="cuda")
    ws = torch.empty(fa.varlen_backward_workspace_bytes(Hq, total_q), dtype=torch.uint8, device="cuda")

    def step():  # forward and backward, nothing allocated, no device value read
        fa.flash_attention_varlen(q, k, v, cu_q, cu_k, max_q, max_k, out=o, lse=lse, window=window, sinks=s)
        fa.flash_attention_varlen_backward(q, k, v, o, do, lse, cu_q, cu_k, max_q, max_k, dq=dq, dk=dk, dv=dv, workspace=ws, window=window,
                                           sinks=s, dsinks=dsinks)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for (sq, sk_), sinks in ((splits[1], sink_sets[1]), (splits[0], sink_sets[1]), (splits[1], sink_sets[0])):
        cu_q.copy_(cu_dev(sq))
        cu_k.copy_(cu_dev(sk_))
        s.copy_(dev(sinks))
        for t in (o, lse, dq, dk, dv, dsinks):
            t.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        seqs = [tuple(np.ascontiguousarray(x) for x in (qn[:, sq[b]:sq[b + 1]], kn[:, sk_[b]:sk_[b + 1]], vn[:, sk_[b]:sk_[b + 1]], don[:, sq[b]:sq[b + 1]]))
                for b in range(3)]
        delta = ws.view(torch.float32).view(Hq, total_q)
        check_sequences(seqs, (dq, dk, dv), dsinks, lse, delta, np.array(sq), np.array(sk_), max_q, dtype, *window, sinks, None, ("graph", sq))
        # the replayed forward is the operator with the sinks now in the buffer: dead rows carry them bit for bit
        b_dead = [b for b in range(3) if sk_[b + 1] == sk_[b] and sq[b + 1] > sq[b]]
        for b in b_dead:
            rows = lse[:, sq[b]:sq[b + 1]]
            assert torch.equal(rows, s[:, None].expand_as(rows)) and not bool(o[sq[b]:sq[b + 1]].any())


# ---- the torch op ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,sdt", [("bf16", 64, "bf16"), ("f16", 128, "f32")])
def test_autograd_of_the_sink_op_inside_the_bounds(fa, dtype, D, sdt):
    import torch

    from flash_attention_metal_amd import torch_op

    Hq, Hkv, lens, window = 8, 2, [(70, 70), (130, 130), (257, 257)], (63, 0)
    seqs = draw_seqs(1853 + D, Hq, Hkv, D, dtype, lens)
    (q, k, v, do), _, cu_q, cu_k = pack4(seqs, dtype, "QKV")  # three views of one packed projection
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    tdt = torch.bfloat16 if sdt == "bf16" else torch.float32
    sinks = np.array([-2.0, -0.5, 0.75, 8.0, 2.0, -3.0, 0.125, 1.5], np.float32)  # exact in bf16: the parameter holds these very values
    s = dev(sinks).to(tdt).requires_grad_(True)
    o, lse = torch_op.attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), 257, 257, window=window, sinks=s)
    assert lse.shape == (Hq, q.shape[0]) and o.stride() == q.stride()
    o.backward(do)
    torch.cuda.synchronize()
    for g, x in ((q.grad, q), (k.grad, k), (v.grad, v), (s.grad, s)):
        assert g is not None and g.dtype == x.dtype and g.shape == x.shape
    # the op rounds the fp32 gradients to the inputs' types: |round(g) - ref| <= bound + max(u (|ref| + bound), 2^-25 for f16)
    w = check_sequences(seqs, (q.grad, k.grad, v.grad), s.grad, None, None, cu_q, cu_k, 257, dtype, *window, sinks, None, "autograd", cast_to=dtype,
                        sinks_cast=(bb.U["bf16"] if sdt == "bf16" else 0.0))
    print(f"SINK BWD autograd worst error / bound {dtype} D={D}: dQ/dK/dV {w[0]:.3f} dsinks {w[2]:.3f}")
    o2, lse2 = torch_op.attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), 257, 257, window=window, sinks=s)
    with pytest.raises(Exception, match="LSE"):  # no gradient through the LSE output
        lse2.sum().backward()


def test_wrapper_dispatch_with_and_without_sinks(fa):
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode

    from flash_attention_metal_amd import torch_op

    seen = []

    class Record(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(str(func))
            return func(*args, **(kwargs or {}))

    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(10, 2, 64, dtype=torch.bfloat16, device="cuda")
    cu = cu_dev([0, 4, 10])
    s = torch.zeros(4, device="cuda")
    with Record():
        torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, True)
        torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, True, window=(2, -1))
        a = torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, True, sinks=s)
        b = torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, True, window=(2, -1), sinks=s)
        c = torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, False, sinks=s)
    torch.cuda.synchronize()
    ops = [x for x in seen if "fa_mi355" in x]
    assert ops == ["fa_mi355.attention_varlen.default", "fa_mi355.attention_varlen_window.default"] + ["fa_mi355.attention_varlen_sink.default"] * 3, ops
    # K = 0 and a sink of 0: LSE = ln(visible keys + 1), whichever window the dispatch chose
    for (o, lse), wl, wr in ((a, -1, 0), (b, 2, 0), (c, -1, -1)):
        for st, n in ((0, 4), (4, 6)):
            want = torch.from_numpy(np.log(W.visible(n, n, wl, wr).sum(1) + 1.0)).float().cuda()
            assert torch.allclose(lse[:, st:st + n], want[None].expand(4, n), atol=1e-5, rtol=0), (wl, wr)
