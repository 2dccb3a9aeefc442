"""GPU: fa_bwd_varlen_softcap (flash_attention_varlen_backward(softcap=...)) on the O / LSE that flash_attention_varlen(softcap=...) wrote,
and the op fa_mi355::attention_varlen_softcap. One launch packs all of window.SEQS. Bounds: tests/softcap.py (CPU side:
tests/test_softcap_cases.py).

  * dQ, dK, dV: every element inside softcap.SeqBounds (backward_bound's per-element bound scaled by 1 - t^2, plus the factor's own term,
    with the forward's lse_err / o_err of include/fa_mi355.h "Logit soft-capping") on windows (-1, 0), (63, 0), (127, 5), both regimes,
    both dtypes, both head dims, both head pairs; dead rows' dQ and unseen keys' dK / dV exactly 0;
  * the visibility probe of tests/test_gpu_window_bwd.py: K = 0 (every t = 0, the factor 1) and one dO row;
  * rows whose every visible score saturates get dQ = 0 to the bound, and their keys no dK from them;
  * NaN in the workspace and in unowned tokens changes nothing; write sentinels under a clamped table;
  * one captured graph of forward and backward, replayed after the tables changed in place;
  * autograd of the op against torch's fp64 autograd of the formula on the CPU, at the bound after the cast.

Worst error / bound measured on an MI355X (printed by the tests): dQ / dK / dV 0.72 (f16, head_dim 64, heads (4, 4)), 0.20 for bf16; the
op's gradients after the cast 0.19."""
import numpy as np
import pytest

import backward_bound as bb
import softcap as sc
import window as W
from test_gpu_varlen import cu_dev
from test_gpu_varlen_bwd import pack4, seq_piece
from test_gpu_window_bwd import CANARY16, CANARY32, draw_seqs, maxes
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


def backward(fa, tensors, grads, o, lse, cu_q, cu_k, max_q, max_k, window, cap, scale=None, workspace=None):
    import torch

    q, k, v, do = tensors
    out = fa.flash_attention_varlen_backward(q, k, v, o, do, lse, cu_dev(cu_q), cu_dev(cu_k), int(max_q), int(max_k), scale=scale, dq=grads[0],
                                             dk=grads[1], dv=grads[2], workspace=workspace, window=window, softcap=cap)
    torch.cuda.synchronize()
    assert len(out) == 3 and all(a.data_ptr() == b.data_ptr() for a, b in zip(out, grads))


def fwd_bwd(fa, tensors, grads, cu_q, cu_k, max_q, max_k, window, cap, scale=None, workspace=None):
    q, k, v, _ = tensors
    o, lse = fa.flash_attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), int(max_q), int(max_k), scale=scale, window=window, softcap=cap)
    backward(fa, tensors, grads, o, lse, cu_q, cu_k, max_q, max_k, window, cap, scale, workspace)
    return o, lse


def check_sequences(seqs, grads, cu_q, cu_k, dtype, wl, wr, cap, scale, what, cast_to=None):
    """Every sequence: finite, inside the bound element by element, exact zeros where required. cast_to: the gradients were rounded to
    that type after the kernels (the torch op), which adds u (|ref| + bound) -- for f16 at least 2^-25 -- to the bound."""
    import torch

    worst = 0.0
    for b, seq in enumerate(seqs):
        Lq, Lk = seq[0].shape[1], seq[1].shape[1]
        g = [seq_piece(t, cu, b).float() for t, cu in zip(grads, (cu_q, cu_k, cu_k))]
        assert all(bool(torch.isfinite(x).all()) for x in g), (what, b, "NaN / Inf in a gradient")
        sb = sc.SeqBounds(*seq, wl, wr, cap, scale, dtype)
        if cast_to is not None:
            sb.bound = tuple(bd + np.where(bd > 0, np.maximum(bb.U[cast_to] * (np.abs(r) + bd), bb.TINY[cast_to]), 0.0) for r, bd in zip(sb.ref, sb.bound))
        r = bb.ratios([x.cpu().numpy() for x in g], sb.ref, sb.bound)
        print(f"SOFTCAP BWD {what} seq {b} {(Lq, Lk)}: error / bound dQ {r[0]:.3f} dK {r[1]:.3f} dV {r[2]:.3f}")
        assert max(r) <= 1.0, (what, b, (Lq, Lk), "error / bound", r)
        worst = max(worst, max(r))
        assert not bool(g[0][:, :sb.n0].any()), (what, b, "dQ of a row without a visible key must be 0 exactly")
        unseen = torch.from_numpy(sb.unseen).cuda()
        assert not bool(g[1][:, unseen].any()) and not bool(g[2][:, unseen].any()), (what, b, "dK / dV of keys no query sees must be 0 exactly")
    return worst


@pytest.mark.parametrize("heads", W.HEADS, ids=lambda h: f"h{h[0]}_{h[1]}")
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_every_element_inside_the_bound_on_the_forwards_own_o_and_lse(fa, dtype, D, heads):
    Hq, Hkv = heads
    worst = 0.0
    for ri, (name, cap, rs) in enumerate(sc.REGIMES):
        scale = sc.scale_of(rs, D)
        for ci, (wl, wr) in enumerate(sc.BWD_WINDOWS):
            seqs = draw_seqs(2000 + 90 * ci + 7 * ri + D + Hq, Hq, Hkv, D, dtype, W.SEQS)
            tensors, grads, cu_q, cu_k = pack4(seqs, dtype, "THD", 5, 3, 0.0)  # trailing tokens nobody owns
            fwd_bwd(fa, tensors, grads, cu_q, cu_k, *maxes(W.SEQS), (wl, wr), cap, scale)
            worst = max(worst, check_sequences(seqs, grads, cu_q, cu_k, dtype, wl, wr, cap, scale, (dtype, D, heads, name, (wl, wr))))
    print(f"SOFTCAP BWD worst error / bound {dtype} D={D} heads={heads}: {worst:.3f}")
    assert worst > 0.01  # the bound is not vacuous


PROBE_SEQS = ((130, 257), (200, 130))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_dv_rows_are_nonzero_exactly_where_the_probed_row_sees_the_key(fa, dtype, D):
    import torch

    Hq, Hkv = 2, 1
    for Lq, Lk in PROBE_SEQS:
        probes = sorted({0, 31, 32, 127, 128, Lq - 1})
        for wl, wr in sc.BWD_WINDOWS:
            vis = W.visible(Lq, Lk, wl, wr)
            nvis = vis.sum(1)
            rng = np.random.default_rng(Lq + wl + D)
            seqs = []
            for i in probes:
                q = bb.rnd(rng.uniform(-1, 1, (Hq, Lq, D)).astype(np.float32), dtype)
                do = np.zeros((Hq, Lq, D), np.float32)
                do[:, i] = 1.0
                seqs.append((q, np.zeros((Hkv, Lk, D), np.float32), np.ones((Hkv, Lk, D), np.float32), do))
            tensors, grads, cu_q, cu_k = pack4(seqs, dtype, "THD")
            with np.errstate(divide="ignore"):
                lse_row = np.log(nvis.astype(np.float64)).astype(np.float32)  # K = 0: every capped score is 0; -inf on dead rows
            lse = torch.from_numpy(np.tile(lse_row, (Hq, len(probes)))).cuda().contiguous()
            o = to_dev(np.tile((nvis > 0).astype(np.float32)[:, None, None], (len(probes), Hq, D)), dtype)  # O = mean of the visible V = 1
            backward(fa, tensors, grads, o, lse, cu_q, cu_k, Lq, Lk, (wl, wr), 50.0)
            for b, i in enumerate(probes):
                dq, dk, dv = (seq_piece(t, cu, b) for t, cu in zip(grads, (cu_q, cu_k, cu_k)))
                assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(dk).all()) and bool(torch.isfinite(dv).all())
                assert not bool(dq.any()), ((Lq, Lk), (wl, wr), i, "dQ = scale dS K with K = 0")
                seen = torch.from_numpy(vis[i]).cuda()
                got = (dv != 0).any(-1).any(0)
                assert torch.equal(got, seen), ((Lq, Lk), (wl, wr), i, "dV rows", torch.nonzero(got != seen).flatten().tolist()[:8])
                assert bool((dv[:, seen] != 0).all()), ((Lq, Lk), (wl, wr), i)


@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_rows_whose_every_score_saturates_get_no_dq_and_give_no_dk(fa, dtype, D):
    """softcap = 2, scale = 1: the first 40 rows of each sequence have q = 8 e_0 and every key k_0 = +-16, so scale s = +-128 and t = +-1
    exactly: 1 - t^2 = 0. Their dQ is 0 to the bound (the factor's own term); with ONLY such rows a key's dK is 0 too. The other rows are
    ordinary and keep the bound honest."""
    import torch

    Hq, Hkv, cap, scale, lens = 4, 2, 2.0, 1.0, [(70, 70), (130, 257)]
    seqs = []
    for q, k, v, do in draw_seqs(2100 + D, Hq, Hkv, D, dtype, lens):
        q, k = q.copy() / 8, k.copy()
        k[..., 0] = np.where(k[..., 0] > 0, 16.0, -16.0)
        q[:, :40] = 0.0
        q[:, :40, 0] = 8.0
        q[:, 40:, 0] = 0.0  # (ordinary rows: the saturating coordinate off, scores of the other D - 1 coordinates / 8)
        seqs.append((bb.rnd(q, dtype), bb.rnd(k, dtype), v, do))
    for wl, wr in ((-1, 0), (63, 0)):
        tensors, grads, cu_q, cu_k = pack4(seqs, dtype, "THD")
        fwd_bwd(fa, tensors, grads, cu_q, cu_k, *maxes(lens), (wl, wr), cap, scale)
        check_sequences(seqs, grads, cu_q, cu_k, dtype, wl, wr, cap, scale, ("saturated", (wl, wr)))
        for b in range(len(lens)):
            dq = seq_piece(grads[0], cu_q, b)
            sb = sc.SeqBounds(*seqs[b], wl, wr, cap, scale, dtype)
            assert float(np.abs(sb.ref[0][:, :40]).max()) < 1e-40  # the exact gradient: (1 - tanh(64)^2) is below 1e-55
            assert bool((dq[:, :40].abs().cpu().numpy() <= sb.bound[0][:, :40]).all())
    # only saturated rows: the keys get no dK at all (dV they do get)
    only = [(s[0][:, :40], s[1], s[2], s[3][:, :40]) for s in seqs]
    tensors, grads, cu_q, cu_k = pack4(only, dtype, "THD")
    fwd_bwd(fa, tensors, grads, cu_q, cu_k, 40, 257, (-1, -1), cap, scale)
    n = int(cu_k[-1])
    bound = np.concatenate([sc.SeqBounds(*s, -1, -1, cap, scale, dtype).bound[1].transpose(1, 0, 2) for s in only])
    assert bool((grads[1][:n].abs().cpu().numpy() <= bound).all()) and float(grads[1][:n].abs().max()) < 1e-4 and bool(grads[2][:n].any())


LENS = [(70, 70), (200, 130), (130, 257)]


@pytest.mark.parametrize("dtype,D,window", [("bf16", 128, (127, 5)), ("f16", 64, (63, 0))])
def test_nan_workspace_and_nan_in_unowned_tokens_change_nothing(fa, dtype, D, window):
    import torch

    seqs = draw_seqs(2137 + D, 4, 2, D, dtype, LENS)
    t1, g1, cu_q, cu_k = pack4(seqs, dtype, "THD", 40, 70, 0.0)
    t2, g2, _, _ = pack4(seqs, dtype, "THD", 40, 70, float("nan"))
    need = fa.varlen_backward_workspace_bytes(4, t1[0].shape[0])
    fwd_bwd(fa, t1, g1, cu_q, cu_k, *maxes(LENS), window, 0.25, workspace=torch.zeros(need, dtype=torch.uint8, device="cuda"))
    fwd_bwd(fa, t2, g2, cu_q, cu_k, *maxes(LENS), window, 0.25, workspace=torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda"))
    for a, b, cu in zip(g1, g2, (cu_q, cu_k, cu_k)):
        n = int(cu[-1])
        assert bool(torch.isfinite(a[:n]).all()) and torch.equal(a[:n], b[:n])
        assert bool(torch.isnan(a[n:]).all()) and bool(torch.isnan(b[n:]).all())  # (pack4 fills the gradients with NaN: not written)


@pytest.mark.parametrize("dtype,D,window", [("bf16", 64, (63, 0)), ("f16", 128, (127, 5))])
def test_write_footprint_under_a_clamped_table(fa, dtype, D, window):
    # as tests/test_gpu_window_bwd.py: sentinels around all three gradients and around the workspace; table entries below 0 and above the
    # totals; tokens owned by nobody; sequence 1 has 300 rows under max_seqlen_q = 200. Exactly the owners' rows are written, with the bits
    # a call on the owner's slice alone gives.
    import torch

    Hq, Hkv, total_q, total_k, max_q, max_k, cap = 4, 2, 487, 731, 200, 350, 0.25
    cu_q, cu_k = [-7, 100, 400, 450], [-1, 150, 500, 2 ** 31 - 1]
    owners = [(0, 100, 0, 150), (100, 200, 150, 350), (400, 50, 500, 231)]
    qn, kn, vn, don = draw_seq(np.random.default_rng(2143 + D), Hq, Hkv, total_q, total_k, D, dtype)
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16

    def gapped(x, H):
        buf = torch.full((x.shape[1] + 3, H + 1, 2 * D), CANARY16[dtype], dtype=torch.int16, device="cuda").view(tdt)
        view = buf[:x.shape[1], :H, :D]
        view.copy_(to_dev(x.transpose(1, 0, 2), dtype))
        return view

    def gapped_grad(total, H):
        buf = torch.full((total + 3, H + 1, 2 * D), CANARY32, dtype=torch.int32, device="cuda")
        return buf, buf.view(torch.float32)[:total, :H, :D]

    q, k, v, do = gapped(qn, Hq), gapped(kn, Hkv), gapped(vn, Hkv), gapped(don, Hq)
    (bq, dq), (bk, dk), (bv, dv) = gapped_grad(total_q, Hq), gapped_grad(total_k, Hkv), gapped_grad(total_k, Hkv)
    need = fa.varlen_backward_workspace_bytes(Hq, total_q)
    wsbuf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device="cuda")
    o, lse = fwd_bwd(fa, (q, k, v, do), (dq, dk, dv), cu_q, cu_k, max_q, max_k, window, cap, workspace=wsbuf[256:256 + need])
    assert bool((wsbuf[:256] == 0xA5).all()) and bool((wsbuf[256 + need:] == 0xA5).all()), "written outside the workspace"
    for name, buf, H, rows in (("dQ", bq, Hq, [(s, n) for s, n, _, _ in owners]), ("dK", bk, Hkv, [(ks, nk) for _, _, ks, nk in owners]),
                               ("dV", bv, Hkv, [(ks, nk) for _, _, ks, nk in owners])):
        written = torch.zeros_like(buf, dtype=torch.bool)
        for s, n in rows:
            written[s:s + n, :H, :D] = True
        assert bool((buf[~written] == CANARY32).all()), name + " was written outside the specified rows"
        assert bool(torch.isfinite(buf.view(torch.float32)[written]).all()), name + ": a specified row was not written"
    for (s, n, ks, nk) in owners:
        seq = tuple(np.ascontiguousarray(x) for x in (qn[:, s:s + n], kn[:, ks:ks + nk], vn[:, ks:ks + nk], don[:, s:s + n]))
        alone, g, cq, ck = pack4([seq], dtype, "THD")
        backward(fa, alone, g, o[s:s + n].contiguous(), lse[:, s:s + n].contiguous(), cq, ck, n, nk, window, cap)
        assert torch.equal(g[0], dq[s:s + n]) and torch.equal(g[1], dk[ks:ks + nk]) and torch.equal(g[2], dv[ks:ks + nk]), (s, n, ks, nk)


@pytest.mark.parametrize("dtype,D,window", [("bf16", 64, (63, 0)), ("f16", 128, (-1, 0))])
def test_graph_replay_after_the_tables_change(fa, dtype, D, window):
    import torch

    Hq, Hkv, total_q, total_k, max_q, max_k, cap = 8, 2, 700, 900, 400, 500, 0.25
    qn, kn, vn, don = draw_seq(np.random.default_rng(2147 + D), Hq, Hkv, total_q, total_k, D, dtype)
    q, k, v, do = (to_dev(x.transpose(1, 0, 2), dtype) for x in (qn, kn, vn, don))
    splits = [([0, 100, 450, 700], [0, 300, 650, 900]), ([0, 390, 400, 700], [0, 400, 900, 900])]  # (the second: one sequence without keys)
    cu_q, cu_k = cu_dev(splits[0][0]), cu_dev(splits[0][1])
    o = torch.empty_like(q)
    lse = torch.empty(Hq, total_q, dtype=torch.float32, device="cuda")
    dq, dk, dv = (torch.empty(x.shape, dtype=torch.float32, device="cuda") for x in (q, k, k))
    ws = torch.empty(fa.varlen_backward_workspace_bytes(Hq, total_q), dtype=torch.uint8, device="cuda")

    def step():  # forward and backward, nothing allocated, no device value read
        fa.flash_attention_varlen(q, k, v, cu_q, cu_k, max_q, max_k, out=o, lse=lse, window=window, softcap=cap)
        fa.flash_attention_varlen_backward(q, k, v, o, do, lse, cu_q, cu_k, max_q, max_k, dq=dq, dk=dk, dv=dv, workspace=ws, window=window, softcap=cap)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for sq, sk in (splits[1], splits[0]):
        cu_q.copy_(cu_dev(sq))
        cu_k.copy_(cu_dev(sk))
        for t in (o, lse, dq, dk, dv):
            t.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        seqs = [tuple(np.ascontiguousarray(x) for x in (qn[:, sq[b]:sq[b + 1]], kn[:, sk[b]:sk[b + 1]], vn[:, sk[b]:sk[b + 1]], don[:, sq[b]:sq[b + 1]]))
                for b in range(3)]
        check_sequences(seqs, (dq, dk, dv), np.array(sq), np.array(sk), dtype, *window, cap, None, ("graph", sq))


# ---- the torch op ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_autograd_of_the_op_against_torch_fp64_autograd_of_the_formula(fa, dtype, D):
    import torch

    from flash_attention_metal_amd import torch_op

    Hq, Hkv, lens, window, cap = 8, 2, [(70, 70), (130, 130), (257, 257)], (63, 0), 0.25
    scale = bb.default_scale(D)
    seqs = draw_seqs(2153 + D, Hq, Hkv, D, dtype, lens)
    (q, k, v, do), _, cu_q, cu_k = pack4(seqs, dtype, "QKV")  # three views of one packed projection
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    o, lse = torch_op.attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), 257, 257, window=window, softcap=cap)
    assert lse.shape == (Hq, q.shape[0]) and o.stride() == q.stride()
    o.backward(do)
    torch.cuda.synchronize()
    for g, x in ((q.grad, q), (k.grad, k), (v.grad, v)):
        assert g is not None and g.dtype == x.dtype and g.shape == x.shape
    worst = 0.0
    for b, (qs, ks, vs, dos) in enumerate(seqs):  # torch's fp64 autograd of the formula, on the CPU
        q64, k64, v64 = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (qs, ks, vs))
        ke, ve = k64.repeat_interleave(Hq // Hkv, 0), v64.repeat_interleave(Hq // Hkv, 0)
        s = cap * torch.tanh((q64 @ ke.transpose(-1, -2)) * (scale / cap))
        vis = torch.from_numpy(W.visible(qs.shape[1], ks.shape[1], *window))
        p = torch.softmax(s.masked_fill(~vis[None], float("-inf")), -1)
        ((p @ ve) * torch.tensor(dos, dtype=torch.float64)).sum().backward()
        sb = sc.SeqBounds(qs, ks, vs, dos, *window, cap, scale, dtype)
        for mine, auto in zip(sb.ref, (q64.grad, k64.grad, v64.grad)):  # the reference the bound is built around is that gradient
            assert np.allclose(mine, auto.numpy(), rtol=1e-9, atol=1e-12)
        bound = tuple(bd + np.where(bd > 0, np.maximum(bb.U[dtype] * (np.abs(r) + bd), bb.TINY[dtype]), 0.0) for r, bd in zip(sb.ref, sb.bound))
        g = [seq_piece(t, cu, b).float().cpu().numpy() for t, cu in zip((q.grad, k.grad, v.grad), (cu_q, cu_k, cu_k))]
        r = bb.ratios(g, [a.numpy() for a in (q64.grad, k64.grad, v64.grad)], bound)
        assert max(r) <= 1.0, (b, "error / bound after the cast", r)
        worst = max(worst, max(r))
    print(f"SOFTCAP BWD autograd worst error / bound {dtype} D={D}: {worst:.3f}")
    o2, lse2 = torch_op.attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), 257, 257, window=window, softcap=cap)
    with pytest.raises(Exception, match="LSE"):  # no gradient through the LSE output
        lse2.sum().backward()


def test_wrapper_dispatch_with_and_without_a_cap(fa):
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
    with Record():
        torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, True)
        torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, True, softcap=0.0)
        a = torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, True, softcap=50.0)
        b = torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, True, window=(2, -1), softcap=50.0)
        c = torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, False, softcap=50.0)
    torch.cuda.synchronize()
    ops = [x for x in seen if "fa_mi355" in x]
    assert ops == ["fa_mi355.attention_varlen.default"] * 2 + ["fa_mi355.attention_varlen_softcap.default"] * 3, ops
    # K = 0: LSE = ln(visible keys), whichever window the dispatch chose
    for (o, lse), wl, wr in ((a, -1, 0), (b, 2, 0), (c, -1, -1)):
        for st, n in ((0, 4), (4, 6)):
            want = torch.from_numpy(np.log(W.visible(n, n, wl, wr).sum(1).astype(np.float64))).float().cuda()
            assert torch.allclose(lse[:, st:st + n], want[None].expand(4, n), atol=1e-5, rtol=0), (wl, wr)
