"""GPU: fa_bwd_varlen_window (flash_attention_varlen_backward(window=...)), the backward under a sliding window, fed the O / LSE that
flash_attention_varlen(window=...) wrote. One launch packs all of window.SEQS.

  * bound: every element of dQ / dK / dV finite and inside the per-sequence bound of tests/window_backward.py (backward_bound.py under
    the window's visibility, with the lse_err / o_err tests/chain_bound.py derives for the `mfma` forward route); dead rows' dQ and unseen
    keys' dK / dV exactly 0. The catalogue window.CASES is shown on the CPU to expose the planted mistakes (test_window_bwd_cases.py);
  * visibility, bit for bit: K = 0, LSE = ln(visible keys), dO zero but for one row i: the dV row of key j is non-zero iff visible[i, j];
  * identities: sign routing, (INT_MAX, 0) / (INT_MAX, INT_MAX) through the windowed kernels, dropped keys in front of every block;
  * the varlen backward's properties under a window: max_seqlen, NaN workspace / unowned tokens, write footprint, graph replay;
  * autograd of fa_mi355::attention_varlen_window.

Worst error / bound measured on an MI355X (printed by the bound tests): f16 D=64 0.37, D=128 0.24; bf16 D=64 0.41, D=128 0.26."""
import numpy as np
import pytest

import backward_bound as bb
import window as W
import window_backward as wb
from test_gpu_varlen import cu_dev
from test_gpu_varlen_bwd import pack4, seq_piece
from util import to_dev
from varlen_backward import draw_seq

pytestmark = pytest.mark.gpu
INT_MAX = W.INT_MAX


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


def forward(fa, tensors, cu_q, cu_k, max_q, max_k, window, scale=None, causal=False):
    q, k, v, _ = tensors
    return fa.flash_attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), int(max_q), int(max_k), is_causal=causal, scale=scale, window=window)


def backward(fa, tensors, grads, o, lse, cu_q, cu_k, max_q, max_k, window, scale=None, causal=False, workspace=None):
    import torch

    q, k, v, do = tensors
    out = fa.flash_attention_varlen_backward(q, k, v, o, do, lse, cu_dev(cu_q), cu_dev(cu_k), int(max_q), int(max_k), is_causal=causal,
                                             scale=scale, dq=grads[0], dk=grads[1], dv=grads[2], workspace=workspace, window=window)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, grads))


def fwd_bwd(fa, tensors, grads, cu_q, cu_k, max_q, max_k, window, scale=None, workspace=None):
    o, lse = forward(fa, tensors, cu_q, cu_k, max_q, max_k, window, scale)
    backward(fa, tensors, grads, o, lse, cu_q, cu_k, max_q, max_k, window, scale, workspace=workspace)
    return o, lse


def maxes(lens):
    return max(l[0] for l in lens), max(max(l[1] for l in lens), 1)


def check_sequences(seqs, grads, cu_q, cu_k, dtype, wl, wr, scale, what, cast_to=None):
    """Every sequence: finite, inside the bound element by element, exact zeros where required. cast_to: the gradients were rounded to
    that type after the kernels (the torch op), which adds u (|ref| + bound) to the bound. Returns the worst error / bound."""
    import torch

    worst = 0.0
    for b, seq in enumerate(seqs):
        Lq, Lk = seq[0].shape[1], seq[1].shape[1]
        g = [seq_piece(t, cu, b).float() for t, cu in zip(grads, (cu_q, cu_k, cu_k))]
        assert all(bool(torch.isfinite(x).all()) for x in g), (what, b, "NaN / Inf in a gradient")
        sb = wb.SeqBounds(*seq, wl, wr, scale, dtype, chain=True)
        if cast_to is not None:
            sb.bound = tuple(bd + bb.U[cast_to] * (np.abs(r) + bd) for r, bd in zip(sb.ref, sb.bound))
        r = wb.worst_ratio([x.cpu().numpy() for x in g], sb)
        assert r <= 1.0, (what, b, (Lq, Lk), "error / bound", r)
        worst = max(worst, r)
        assert not bool(g[0][:, :sb.n0].any()), (what, b, "dQ of a row without a visible key must be 0 exactly")
        unseen = torch.from_numpy(sb.unseen).cuda()
        assert not bool(g[1][:, unseen].any()) and not bool(g[2][:, unseen].any()), (what, b, "dK / dV of keys no query sees must be 0 exactly")
    return worst


def draw_seqs(seed, Hq, Hkv, D, dtype, lens):
    rng = np.random.default_rng(seed)
    return [draw_seq(rng, Hq, Hkv, Lq, Lk, D, dtype) for Lq, Lk in lens]


# ---- the bound, per element ------------------------------------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("heads", W.HEADS, ids=lambda h: f"h{h[0]}_{h[1]}")
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_every_element_inside_the_bound_on_the_catalogue(fa, dtype, D, heads):
    Hq, Hkv = heads
    worst = 0.0
    for ci, (name, lens, wl, wr) in enumerate(W.CASES):
        seqs = draw_seqs(900 * ci + D + Hq, Hq, Hkv, D, dtype, lens)
        scale = 0.05 if name == "w63" else None  # one case under a custom scale
        tensors, grads, cu_q, cu_k = pack4(seqs, dtype, "THD")
        fwd_bwd(fa, tensors, grads, cu_q, cu_k, *maxes(lens), (wl, wr), scale)
        worst = max(worst, check_sequences(seqs, grads, cu_q, cu_k, dtype, wl, wr, scale, name))
    WORST[(dtype, D)] = max(WORST.get((dtype, D), 0.0), worst)
    print(f"WINDOW BWD worst error / bound {dtype} D={D} heads={heads}: {worst:.3f}")
    assert worst > 0.01  # the bound is not vacuous


# ---- visibility, bit for bit -------------------------------------------------------------------------------------------------------
PROBE_SEQS = ((130, 257), (200, 130))
PROBE_WINDOWS = ((0, 0), (63, 0), (64, 64), (127, 5), (65, -1), (-1, 5))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_dv_rows_are_nonzero_exactly_where_the_probed_row_sees_the_key(fa, dtype, D):
    import torch

    Hq, Hkv = 2, 1
    for Lq, Lk in PROBE_SEQS:
        probes = sorted({0, 31, 32, 127, 128, Lq - 1})
        lens = [(Lq, Lk)] * len(probes)
        for wl, wr in PROBE_WINDOWS:
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
                lse_row = np.log(nvis.astype(np.float64)).astype(np.float32)  # -inf on dead rows
            lse = torch.from_numpy(np.tile(lse_row, (Hq, len(probes)))).cuda().contiguous()
            o = to_dev(np.tile((nvis > 0).astype(np.float32)[:, None, None], (len(probes), Hq, D)), dtype)  # O = mean of the visible V = 1
            backward(fa, tensors, grads, o, lse, cu_q, cu_k, Lq, Lk, (wl, wr))
            for b, i in enumerate(probes):
                dq, dk, dv = (seq_piece(t, cu, b) for t, cu in zip(grads, (cu_q, cu_k, cu_k)))
                assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(dk).all()) and bool(torch.isfinite(dv).all())
                rows = torch.arange(Lq, device="cuda") != i
                assert not bool(dq[:, rows].any()), ((Lq, Lk), (wl, wr), i, "dQ of a row without dO")
                seen = torch.from_numpy(vis[i]).cuda()
                got = (dv != 0).any(-1).any(0)
                assert torch.equal(got, seen), ((Lq, Lk), (wl, wr), i, "dV rows", torch.nonzero(got != seen).flatten().tolist()[:8])
                assert bool((dv[:, seen] != 0).all()), ((Lq, Lk), (wl, wr), i)


# ---- identities ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_sign_routing_is_bit_identical_to_the_unwindowed_call(fa, dtype, D):
    import torch

    seqs = draw_seqs(3 + D, 8, 2, D, dtype, W.SEQS)
    for causal, window in ((False, (-1, -1)), (True, (-1, 0)), (True, (-5, 0))):
        tensors, g1, cu_q, cu_k = pack4(seqs, dtype, "THD")
        _, g2, _, _ = pack4(seqs, dtype, "THD")
        o, lse = forward(fa, tensors, cu_q, cu_k, *maxes(W.SEQS), None, causal=causal)
        backward(fa, tensors, g1, o, lse, cu_q, cu_k, *maxes(W.SEQS), None, causal=causal)
        backward(fa, tensors, g2, o, lse, cu_q, cu_k, *maxes(W.SEQS), window)
        assert all(torch.equal(a, b) for a, b in zip(g1, g2)), window


@pytest.mark.parametrize("dtype,D,heads", [("bf16", 64, (8, 2)), ("f16", 128, (4, 4)), ("bf16", 128, (8, 2)), ("f16", 64, (4, 4))])
def test_never_binding_bounds_through_the_window_kernels_give_the_varlen_bits(fa, dtype, D, heads):
    import torch

    seqs = draw_seqs(13 + D, heads[0], heads[1], D, dtype, W.SEQS)
    for causal, window in ((True, (INT_MAX, 0)), (False, (INT_MAX, INT_MAX))):
        tensors, g1, cu_q, cu_k = pack4(seqs, dtype, "THD")
        _, g2, _, _ = pack4(seqs, dtype, "THD")
        o, lse = forward(fa, tensors, cu_q, cu_k, *maxes(W.SEQS), None, causal=causal)
        backward(fa, tensors, g1, o, lse, cu_q, cu_k, *maxes(W.SEQS), None, causal=causal)
        backward(fa, tensors, g2, o, lse, cu_q, cu_k, *maxes(W.SEQS), window)
        claimed = 0
        for b, (Lq, Lk) in enumerate(W.SEQS):
            if W.identity_claimed(Lq, Lk):
                claimed += 1
                for name, a, c, cu in zip(("dQ", "dK", "dV"), g1, g2, (cu_q, cu_k, cu_k)):
                    assert torch.equal(seq_piece(a, cu, b), seq_piece(c, cu, b)), (window, (Lq, Lk), name)
        assert claimed >= 5


@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_dropping_keys_no_block_can_see_changes_nothing(fa, dtype, D):
    import torch

    Lq, Lk, wl, drop = W.SHIFT
    assert drop % W.TILE == 0 and wb.query_range(Lq, Lk, wl, 0, 0, drop - 1) is None
    (q, k, v, do), = draw_seqs(23 + D, 8, 2, D, dtype, [(Lq, Lk)])
    full, g1, cu_q, cu_k = pack4([(q, k, v, do)], dtype, "THD")
    cut, g2, cu_q2, cu_k2 = pack4([(q, np.ascontiguousarray(k[:, drop:]), np.ascontiguousarray(v[:, drop:]), do)], dtype, "THD")
    o, lse = fwd_bwd(fa, full, g1, cu_q, cu_k, Lq, Lk, (wl, 0))
    backward(fa, cut, g2, o, lse, cu_q2, cu_k2, Lq, Lk - drop, (wl, 0))
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1][drop:], g2[1]) and torch.equal(g1[2][drop:], g2[2])
    assert not bool(g1[1][:drop].any()) and not bool(g1[2][:drop].any())


# ---- the varlen backward's properties under a window ----------------------------------------------------------------------------------
LENS = [(70, 70), (200, 130), (130, 257), (129, 1), (257, 513)]


@pytest.mark.parametrize("dtype,D,window", [("bf16", 64, (63, 0)), ("f16", 128, (65, -1))])
def test_max_seqlen_above_the_true_lengths_changes_nothing(fa, dtype, D, window):
    import torch

    seqs = draw_seqs(31 + D, 4, 2, D, dtype, LENS)
    tensors, g1, cu_q, cu_k = pack4(seqs, dtype, "THD")
    _, g2, _, _ = pack4(seqs, dtype, "THD")
    o, lse = fwd_bwd(fa, tensors, g1, cu_q, cu_k, *maxes(LENS), window)
    backward(fa, tensors, g2, o, lse, cu_q, cu_k, int(cu_q[-1]), int(cu_k[-1]), window)  # more blocks, and another clamp of the open side
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


@pytest.mark.parametrize("dtype,D,window", [("bf16", 128, (127, 5)), ("f16", 64, (63, 0))])
def test_nan_workspace_and_nan_in_unowned_tokens_change_nothing(fa, dtype, D, window):
    import torch

    seqs = draw_seqs(37 + D, 4, 2, D, dtype, LENS)
    t1, g1, cu_q, cu_k = pack4(seqs, dtype, "THD", 40, 70, 0.0)
    t2, g2, _, _ = pack4(seqs, dtype, "THD", 40, 70, float("nan"))
    need = fa.varlen_backward_workspace_bytes(4, t1[0].shape[0])
    fwd_bwd(fa, t1, g1, cu_q, cu_k, *maxes(LENS), window, workspace=torch.zeros(need, dtype=torch.uint8, device="cuda"))
    fwd_bwd(fa, t2, g2, cu_q, cu_k, *maxes(LENS), window, workspace=torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda"))
    for a, b, cu in zip(g1, g2, (cu_q, cu_k, cu_k)):
        n = int(cu[-1])
        assert bool(torch.isfinite(a[:n]).all()) and torch.equal(a[:n], b[:n])
        assert bool(torch.isnan(a[n:]).all()) and bool(torch.isnan(b[n:]).all())  # (pack4 fills the gradients with NaN: not written)


CANARY16 = {"bf16": 0x7FC1, "f16": 0x7E01}  # NaNs with a payload (positive as int16)
CANARY32 = 0x7FC00001


@pytest.mark.parametrize("dtype,D,window", [("bf16", 64, (63, 0)), ("f16", 128, (127, 5))])
def test_write_footprint_under_a_clamped_table(fa, dtype, D, window):
    # sentinels around all three gradients (a spare head per row, a head pitch of 2 D, three spare rows) and around the workspace;
    # table entries below 0 and above the totals; 37 / 31 tokens owned by nobody; sequence 1 has 300 rows under max_seqlen_q = 200.
    # Exactly the owners' rows are written, with the bits a call on the owner's slice alone gives.
    import torch

    Hq, Hkv, total_q, total_k, max_q, max_k = 4, 2, 487, 731, 200, 350
    cu_q, cu_k = [-7, 100, 400, 450], [-1, 150, 500, 2 ** 31 - 1]
    owners = [(0, 100, 0, 150), (100, 200, 150, 350), (400, 50, 500, 231)]
    qn, kn, vn, don = draw_seq(np.random.default_rng(43 + D), Hq, Hkv, total_q, total_k, D, dtype)
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
    o, lse = fwd_bwd(fa, (q, k, v, do), (dq, dk, dv), cu_q, cu_k, max_q, max_k, window, workspace=wsbuf[256:256 + need])
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
        backward(fa, alone, g, o[s:s + n].contiguous(), lse[:, s:s + n].contiguous(), cq, ck, n, nk, window)
        assert torch.equal(g[0], dq[s:s + n]) and torch.equal(g[1], dk[ks:ks + nk]) and torch.equal(g[2], dv[ks:ks + nk]), (s, n, ks, nk)


@pytest.mark.parametrize("dtype,D,window", [("bf16", 64, (63, 0)), ("f16", 128, (64, 64))])
def test_graph_replay_after_the_tables_change(fa, dtype, D, window):
    import torch

    Hq, Hkv, total_q, total_k, max_q, max_k = 8, 2, 700, 900, 400, 500
    qn, kn, vn, don = draw_seq(np.random.default_rng(47 + D), Hq, Hkv, total_q, total_k, D, dtype)
    q, k, v, do = (to_dev(x.transpose(1, 0, 2), dtype) for x in (qn, kn, vn, don))
    splits = [([0, 100, 450, 700], [0, 300, 650, 900]), ([0, 390, 400, 700], [0, 400, 900, 900])]  # (the second: one sequence without keys)
    cu_q, cu_k = cu_dev(splits[0][0]), cu_dev(splits[0][1])
    o = torch.empty_like(q)
    lse = torch.empty(Hq, total_q, dtype=torch.float32, device="cuda")
    dq, dk, dv = (torch.empty(x.shape, dtype=torch.float32, device="cuda") for x in (q, k, k))
    ws = torch.empty(fa.varlen_backward_workspace_bytes(Hq, total_q), dtype=torch.uint8, device="cuda")

    def step():  # forward and backward, nothing allocated, no device value read
        fa.flash_attention_varlen(q, k, v, cu_q, cu_k, max_q, max_k, out=o, lse=lse, window=window)
        fa.flash_attention_varlen_backward(q, k, v, o, do, lse, cu_q, cu_k, max_q, max_k, dq=dq, dk=dk, dv=dv, workspace=ws, window=window)

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
        check_sequences(seqs, (dq, dk, dv), np.array(sq), np.array(sk), dtype, *window, None, ("graph", sq))


# ---- the torch op ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_autograd_of_the_window_op_inside_the_bound(fa, dtype, D):
    import torch

    from flash_attention_metal_amd import torch_op

    Hq, Hkv, lens, window = 8, 2, [(70, 70), (130, 130), (257, 257)], (63, 0)
    seqs = draw_seqs(53 + D, Hq, Hkv, D, dtype, lens)
    (q, k, v, do), _, cu_q, cu_k = pack4(seqs, dtype, "QKV")  # three views of one packed projection
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    o, lse = torch_op.attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), 257, 257, window=window)
    assert lse.shape == (Hq, q.shape[0]) and o.stride() == q.stride()
    o.backward(do)
    torch.cuda.synchronize()
    for g, x in ((q.grad, q), (k.grad, k), (v.grad, v)):
        assert g.dtype == x.dtype and g.shape == x.shape
    # the op rounds the fp32 gradients to the input type: |round(g) - ref| <= bound + u (|ref| + bound)
    worst = check_sequences(seqs, (q.grad, k.grad, v.grad), cu_q, cu_k, dtype, *window, None, "autograd", cast_to=dtype)
    print(f"WINDOW BWD autograd worst error / bound {dtype} D={D}: {worst:.3f}")
    o2, lse2 = torch_op.attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), 257, 257, window=window)
    with pytest.raises(Exception, match="LSE"):  # no gradient through the LSE output
        lse2.sum().backward()


def test_meta_shapes_and_window_none_reaches_the_old_op(fa):
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode

    from flash_attention_metal_amd import torch_op

    qm = torch.empty(10, 8, 128, dtype=torch.float16, device="meta")
    km = torch.empty(12, 2, 128, dtype=torch.float16, device="meta")
    cum = torch.empty(3, dtype=torch.int32, device="meta")
    om, lm = torch.ops.fa_mi355.attention_varlen_window(qm, km, km, cum, cum, 10, 12, 3, 0, 0.0)
    assert om.shape == qm.shape and om.dtype == qm.dtype and lm.shape == (8, 10) and lm.dtype == torch.float32

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
        torch_op.attention_varlen(q, k, k, cu, cu, 6, 6, True, window=(2, -1))
    torch.cuda.synchronize()
    ops = [s for s in seen if "fa_mi355" in s]
    assert ops == ["fa_mi355.attention_varlen.default", "fa_mi355.attention_varlen_window.default"], ops
