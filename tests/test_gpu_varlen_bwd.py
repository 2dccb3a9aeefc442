"""GPU: fa_bwd_varlen (flash_attention_varlen_backward), the backward over packed variable-length sequences, fed the O / LSE that
flash_attention_varlen wrote.

Per sequence the operator is fa_bwd_ex on that sequence, so every check is made sequence by sequence:
  * every element of dQ / dK / dV inside the derived bound of tests/backward_bound.py (through tests/varlen_backward.py; the catalogue is
    shown on the CPU to expose the structural mistakes, tests/test_varlen_bwd_cases.py);
  * bit for bit against fa_bwd_ex on the sequence alone (torch.equal) wherever Lk >= Lq >= 1 (without the mask: Lq, Lk >= 1), whatever
    the layout, the other sequences or max_seqlen_*;
  * rows without a visible key: dQ = 0 exactly, nothing added to dK / dV, no NaN / Inf anywhere; Lq = 0: dK = dV = 0 exactly;
  * a NaN-filled workspace and NaN in tokens owned by nobody change nothing;
  * the write footprint in canary-filled buffers, also under corrupt tables and a max_seqlen below a true length;
  * one captured graph replayed after both tables changed in place; the torch op's autograd."""
import numpy as np
import pytest

from test_gpu_varlen import cu_dev
from util import to_dev
from varlen_backward import CASES, SeqBounds, draw_seq, worst_ratio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def pack4(seqs, dtype, layout, tail_q=0, tail_k=0, tail_value=0.0):
    """(q, k, v, do) of every sequence back to back as device tensors q, do [total_q, Hq, D] and k, v [total_k, Hkv, D] in one of the
    layouts the header names, the fp32 gradient tensors dq, dk, dv under the same element strides (QKV: three views of ONE buffer),
    and the cu_seqlens (numpy int32). tail_*: tokens behind the last sequence that belong to nobody, filled with tail_value."""
    import torch

    Hq, _, D = seqs[0][0].shape
    Hkv = seqs[0][1].shape[0]

    def cat(i, H, tail):
        return np.concatenate([s[i].transpose(1, 0, 2) for s in seqs] + [np.full((tail, H, D), tail_value, np.float32)])
    qn, kn, vn, don = cat(0, Hq, tail_q), cat(1, Hkv, tail_k), cat(2, Hkv, tail_k), cat(3, Hq, tail_q)
    cu_q = np.cumsum([0] + [s[0].shape[1] for s in seqs]).astype(np.int32)
    cu_k = np.cumsum([0] + [s[1].shape[1] for s in seqs]).astype(np.int32)
    if layout == "THD":
        q, k, v, do = (to_dev(x, dtype) for x in (qn, kn, vn, don))
        dq, dk, dv = (torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda") for x in (q, k, v))
    elif layout == "HTD":
        q, k, v, do = (to_dev(x.transpose(1, 0, 2), dtype).transpose(0, 1) for x in (qn, kn, vn, don))
        dq, dk, dv = (torch.full((x.shape[1], x.shape[0], D), float("nan"), dtype=torch.float32, device="cuda").transpose(0, 1) for x in (q, k, v))
    else:  # "QKV": three views of one packed [total, Hq + 2 Hkv, D] projection; its gradient is ONE fp32 buffer of that shape
        assert layout == "QKV" and qn.shape[0] == kn.shape[0]
        buf = to_dev(np.concatenate([qn, kn, vn], axis=1), dtype)
        q, k, v = buf[:, :Hq], buf[:, Hq:Hq + Hkv], buf[:, Hq + Hkv:]
        do = to_dev(np.concatenate([don, kn, vn], axis=1), dtype)[:, :Hq]
        g = torch.full(buf.shape, float("nan"), dtype=torch.float32, device="cuda")
        dq, dk, dv = g[:, :Hq], g[:, Hq:Hq + Hkv], g[:, Hq + Hkv:]
    return (q, k, v, do), (dq, dk, dv), cu_q, cu_k


def fwd_bwd(fa, tensors, grads, cu_q, cu_k, max_q, max_k, causal, scale=None, workspace=None):
    import torch

    q, k, v, do = tensors
    cq, ck = cu_dev(cu_q), cu_dev(cu_k)
    o, lse = fa.flash_attention_varlen(q, k, v, cq, ck, int(max_q), int(max_k), is_causal=causal, scale=scale)
    out = fa.flash_attention_varlen_backward(q, k, v, o, do, lse, cq, ck, int(max_q), int(max_k), is_causal=causal, scale=scale,
                                             dq=grads[0], dk=grads[1], dv=grads[2], workspace=workspace)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, grads))
    return o, lse


def seq_piece(t, cu, b):
    """Sequence b of a packed [total, H, D] tensor as [H, L, D]."""
    return t[int(cu[b]):int(cu[b + 1])].transpose(0, 1)


def dense_bwd(fa, seq, o_b, lse_b, dtype, causal, scale=None):
    """fa_bwd_ex on one sequence alone (contiguous [1, H, L, D]), fed the same O / LSE: (dQ, dK, dV) as [H, L, D] device tensors."""
    import torch

    q, k, v, do = (to_dev(x[None], dtype) for x in seq)
    o4 = torch.empty_like(q).copy_(o_b[None])  # (not .contiguous(): a one-row sequence's view already counts as contiguous under its own strides)
    dq, dk, dv = fa.flash_attention_backward(q, k, v, o4, do, lse_b[None].contiguous(), is_causal=causal, scale=scale)
    torch.cuda.synchronize()
    return dq[0], dk[0], dv[0]


def qualifies(Lq, Lk, causal):
    return Lq >= 1 and Lk >= 1 and (Lk >= Lq or not causal)


def check_sequences(fa, seqs, grads, o, lse, cu_q, cu_k, dtype, causal, scale, what, bits=True):
    """Every sequence: finite, inside the bound element by element, exact zeros where required, the dense kernels' bits where they apply.
    Returns the worst error / bound."""
    import torch

    worst = 0.0
    for b, seq in enumerate(seqs):
        Lq, Lk = seq[0].shape[1], seq[1].shape[1]
        g = [seq_piece(t, cu, b) for t, cu in zip(grads, (cu_q, cu_k, cu_k))]
        assert all(bool(torch.isfinite(x).all()) for x in g), (what, b, "NaN / Inf in a gradient")
        sb = SeqBounds(*seq, causal, scale, dtype)
        r = worst_ratio([x.cpu().numpy() for x in g], sb)
        assert r <= 1.0, (what, b, (Lq, Lk), "error / bound", r)
        worst = max(worst, r)
        assert not bool(g[0][:, :sb.n0].any()), (what, b, "dQ of a row without a visible key must be 0 exactly")
        if sb.n0 >= Lq:
            assert not bool(g[1].any()) and not bool(g[2].any()), (what, b, "dK / dV of keys no query sees must be 0 exactly")
        if bits and qualifies(Lq, Lk, causal):
            ob, lb = seq_piece(o, cu_q, b), lse[:, int(cu_q[b]):int(cu_q[b + 1])]
            for name, x, y in zip(("dQ", "dK", "dV"), g, dense_bwd(fa, seq, ob, lb, dtype, causal, scale)):
                assert torch.equal(x, y), (what, b, (Lq, Lk), name + " differs from fa_bwd_ex on the sequence alone", float((x - y).abs().max()))
    return worst


GRID = [(t, d, c) for t in ("f16", "bf16") for d in (64, 128) for c in (False, True)]
WORST = {}


def draw_case(ci, dtype, D, causal):
    Hq, Hkv, layout, lens = CASES[ci]
    rng = np.random.default_rng(500 * ci + D + (11 if causal else 0))
    return layout, lens, [draw_seq(rng, Hq, Hkv, Lq, Lk, D, dtype) for Lq, Lk in lens]


# ---- the bound and the dense kernels' bits, per sequence ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,causal", GRID)
def test_bound_and_dense_bits_per_sequence(fa, dtype, D, causal):
    # the catalogue: Hq / Hkv of 1, 4 and 8; 1 - 9 sequences; lengths on both sides of 64, 128 and 256; the three layouts (QKV: one fp32
    # gradient buffer); the last case holds Lk < Lq, Lk = 0 and Lq = 0. Case 1 runs under a custom scale.
    worst = 0.0
    for ci in range(len(CASES)):
        layout, lens, seqs = draw_case(ci, dtype, D, causal)
        scale = 0.05 if ci == 1 else None
        tensors, grads, cu_q, cu_k = pack4(seqs, dtype, layout)
        o, lse = fwd_bwd(fa, tensors, grads, cu_q, cu_k, max(l[0] for l in lens), max(max(l[1] for l in lens), 1), causal, scale)
        worst = max(worst, check_sequences(fa, seqs, grads, o, lse, cu_q, cu_k, dtype, causal, scale, (ci, layout)))
    WORST[(dtype, D, causal)] = worst
    print(f"worst error / bound {dtype} D={D} causal={causal}: {worst:.3f}")


@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_max_seqlen_above_the_true_lengths_changes_nothing(fa, dtype, D):
    import torch

    layout, lens, seqs = draw_case(1, dtype, D, True)
    tensors, g1, cu_q, cu_k = pack4(seqs, dtype, layout)
    _, g2, _, _ = pack4(seqs, dtype, layout)
    fwd_bwd(fa, tensors, g1, cu_q, cu_k, 128, 257, True)
    fwd_bwd(fa, tensors, g2, cu_q, cu_k, int(cu_q[-1]), int(cu_k[-1]), True)  # more blocks, all of which own nothing
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


# ---- the workspace's contents and tokens owned by nobody ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,causal", [("bf16", 64, True), ("f16", 128, False), ("bf16", 128, True)])
def test_nan_workspace_and_nan_in_unowned_tokens_change_nothing(fa, dtype, D, causal):
    import torch

    layout, lens, seqs = draw_case(4, dtype, D, causal)
    Hq = seqs[0][0].shape[0]
    max_q, max_k = max(l[0] for l in lens), max(l[1] for l in lens)
    t1, g1, cu_q, cu_k = pack4(seqs, dtype, layout, 40, 70, 0.0)
    t2, g2, _, _ = pack4(seqs, dtype, layout, 40, 70, float("nan"))
    need = fa.varlen_backward_workspace_bytes(Hq, t1[0].shape[0])
    fwd_bwd(fa, t1, g1, cu_q, cu_k, max_q, max_k, causal, workspace=torch.zeros(need, dtype=torch.uint8, device="cuda"))
    fwd_bwd(fa, t2, g2, cu_q, cu_k, max_q, max_k, causal, workspace=torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda"))
    for a, b, cu in zip(g1, g2, (cu_q, cu_k, cu_k)):
        n = int(cu[-1])
        assert bool(torch.isfinite(a[:n]).all()) and torch.equal(a[:n], b[:n])
        assert bool(torch.isnan(a[n:]).all()) and bool(torch.isnan(b[n:]).all())  # (pack4 fills the gradients with NaN: not written)


# ---- write footprint ------------------------------------------------------------------------------------------------------------
CANARY16 = {"bf16": 0x7FC1, "f16": 0x7E01}  # NaNs with a payload (positive as int16)
CANARY32 = 0x7FC00001


def _footprint(fa, dtype, D, causal, cu_q, cu_k, max_q, max_k, total_q, total_k, owners, seed):
    """One forward + backward on canary-filled, gapped buffers (a spare head per row and a head pitch of 2 D: wide strides). owners:
    [(first q token, rows, first key, keys)] per sequence as the documented clamps define it: exactly their dQ / dK / dV rows must be
    written, bit for bit what fa_bwd_ex gives on the owner's slice; every other byte of the three buffers keeps its canary."""
    import torch

    Hq, Hkv = 4, 2
    rng = np.random.default_rng(seed)
    qn, kn, vn, don = draw_seq(rng, Hq, Hkv, total_q, total_k, D, dtype)
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
    assert dq.stride() == q.stride() and dk.stride() == k.stride()
    o, lse = fwd_bwd(fa, (q, k, v, do), (dq, dk, dv), cu_q, cu_k, max_q, max_k, causal,
                     workspace=torch.full((fa.varlen_backward_workspace_bytes(Hq, total_q),), 0xFF, dtype=torch.uint8, device="cuda"))
    for name, buf, H, rows in (("dQ", bq, Hq, [(s, n) for s, n, _, _ in owners]), ("dK", bk, Hkv, [(ks, nk) for _, _, ks, nk in owners]),
                               ("dV", bv, Hkv, [(ks, nk) for _, _, ks, nk in owners])):
        written = torch.zeros_like(buf, dtype=torch.bool)
        for s, n in rows:
            written[s:s + n, :H, :D] = True
        assert bool((buf[~written] == CANARY32).all()), name + " was written outside the specified rows"
        assert bool(torch.isfinite(buf.view(torch.float32)[written]).all()), name + ": a specified row was not written"
    for (s, n, ks, nk) in owners:
        assert nk >= n >= 1
        seq = tuple(np.ascontiguousarray(x) for x in (qn[:, s:s + n], kn[:, ks:ks + nk], vn[:, ks:ks + nk], don[:, s:s + n]))
        ref = dense_bwd(fa, seq, o[s:s + n].transpose(0, 1), lse[:, s:s + n], dtype, causal)
        got = (dq[s:s + n].transpose(0, 1), dk[ks:ks + nk].transpose(0, 1), dv[ks:ks + nk].transpose(0, 1))
        assert all(torch.equal(a, b) for a, b in zip(got, ref)), (s, n, ks, nk)


@pytest.mark.parametrize("dtype,D,causal", [("bf16", 64, True), ("f16", 128, True), ("bf16", 128, False), ("f16", 64, False)])
def test_write_footprint_with_unowned_tokens_and_a_clamped_sequence(fa, dtype, D, causal):
    # 37 query tokens and 31 keys behind cu[B] belong to nobody; sequence 1 has 300 rows but max_seqlen_q = 200: its rows 200 .. 299 are
    # not written and its first 200 rows are those of a sequence of 200 queries; its keys 350 .. of 350 are all inside max_seqlen_k
    _footprint(fa, dtype, D, causal, [0, 100, 400, 450], [0, 150, 500, 700], 200, 350, 487, 731,
               [(0, 100, 0, 150), (100, 200, 150, 350), (400, 50, 500, 200)], 31)


@pytest.mark.parametrize("dtype,D,causal", [("bf16", 128, True), ("f16", 64, False)])
def test_write_footprint_with_max_seqlen_k_below_a_true_length(fa, dtype, D, causal):
    # sequence 1 has 350 keys but max_seqlen_k = 250: its keys 250 .. 349 get no dK / dV and take no part (a sequence of 250 keys)
    _footprint(fa, dtype, D, causal, [0, 100, 300, 450], [0, 150, 500, 700], 200, 250, 487, 731,
               [(0, 100, 0, 150), (100, 200, 150, 250), (300, 150, 500, 200)], 32)


@pytest.mark.parametrize("dtype,D,causal", [("bf16", 64, True), ("f16", 128, False)])
def test_out_of_range_table_entries_are_clamped(fa, dtype, D, causal):
    # entries below 0 and above total: clamped to [0, total] -- sequence 0 starts at token 0, sequence 2 ends with the last token / key
    _footprint(fa, dtype, D, causal, [-7, 100, 400, 10000], [-1, 150, 500, 2 ** 31 - 1], 300, 350, 487, 731,
               [(0, 100, 0, 150), (100, 300, 150, 350), (400, 87, 500, 231)], 33)


@pytest.mark.parametrize("dtype,D,causal", [("bf16", 128, True), ("f16", 64, False)])
def test_a_decreasing_table_entry_gives_an_empty_sequence(fa, dtype, D, causal):
    # (200, 100) and (400, 150) decrease: sequence 0 has neither rows nor keys and writes nothing; the others are untouched by it
    _footprint(fa, dtype, D, causal, [200, 100, 300, 487], [400, 150, 500, 731], 300, 350, 487, 731,
               [(100, 200, 150, 350), (300, 187, 500, 231)], 34)


# ---- one captured graph, replayed after both tables changed in place -----------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_graph_replay_after_the_tables_change(fa, dtype, D):
    import torch

    Hq, Hkv, total_q, total_k, max_q, max_k = 8, 2, 700, 900, 400, 500
    rng = np.random.default_rng(41 + D)
    qn, kn, vn, don = draw_seq(rng, Hq, Hkv, total_q, total_k, D, dtype)
    q, k, v, do = (to_dev(x.transpose(1, 0, 2), dtype) for x in (qn, kn, vn, don))
    splits = [([0, 100, 450, 700], [0, 300, 650, 900]), ([0, 390, 400, 700], [0, 400, 900, 900])]  # (the second: one sequence without keys)
    cu_q, cu_k = cu_dev(splits[0][0]), cu_dev(splits[0][1])
    o = torch.empty_like(q)
    lse = torch.empty(Hq, total_q, dtype=torch.float32, device="cuda")
    dq, dk, dv = torch.empty(q.shape, dtype=torch.float32, device="cuda"), torch.empty(k.shape, dtype=torch.float32, device="cuda"), torch.empty(k.shape, dtype=torch.float32, device="cuda")
    ws = torch.empty(fa.varlen_backward_workspace_bytes(Hq, total_q), dtype=torch.uint8, device="cuda")

    def step():  # forward and backward, nothing allocated, no device value read
        fa.flash_attention_varlen(q, k, v, cu_q, cu_k, max_q, max_k, is_causal=True, out=o, lse=lse)
        fa.flash_attention_varlen_backward(q, k, v, o, do, lse, cu_q, cu_k, max_q, max_k, is_causal=True, dq=dq, dk=dk, dv=dv, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for sq, sk in (splits[1], splits[0], splits[1]):
        cu_q.copy_(cu_dev(sq))
        cu_k.copy_(cu_dev(sk))
        for t in (o, lse, dq, dk, dv):
            t.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        seqs = [tuple(np.ascontiguousarray(x) for x in (qn[:, sq[b]:sq[b + 1]], kn[:, sk[b]:sk[b + 1]], vn[:, sk[b]:sk[b + 1]], don[:, sq[b]:sq[b + 1]]))
                for b in range(3)]
        check_sequences(fa, seqs, (dq, dk, dv), o, lse, np.array(sq), np.array(sk), dtype, True, None, ("graph", sq))


# ---- the torch op ----------------------------------------------------------------------------------------------------------------
# (shapes on which the dense op's forward routes to the kernel the varlen forward is the mode of -- at head_dim 64 that takes more than 64
# blocks of 128 rows per sequence --, so that O, LSE and with them the gradients can be compared bit for bit)
@pytest.mark.parametrize("dtype,D,causal,Hq,Hkv,lens", [("bf16", 64, True, 32, 8, [(257, 257), (300, 400), (260, 300)]),
                                                        ("f16", 128, False, 8, 2, [(100, 100), (64, 200), (129, 257)]),
                                                        ("bf16", 128, True, 8, 1, [(100, 100), (64, 200), (129, 257)])])
def test_autograd_of_the_op_matches_the_dense_op_per_sequence(fa, dtype, D, causal, Hq, Hkv, lens):
    import torch

    from flash_attention_metal_amd import torch_op

    max_q, max_k = max(l[0] for l in lens), max(l[1] for l in lens)
    rng = np.random.default_rng(51 + D)
    seqs = [draw_seq(rng, Hq, Hkv, Lq, Lk, D, dtype) for Lq, Lk in lens]
    (q, k, v, do), _, cu_q, cu_k = pack4(seqs, dtype, "THD", 20, 30)  # 20 / 30 tokens owned by nobody
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    o, lse = torch_op.attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), max_q, max_k, causal, 0.0)
    assert lse.shape == (Hq, q.shape[0]) and not bool(o[int(cu_q[-1]):].any())
    o.backward(do.transpose(0, 1).contiguous().transpose(0, 1))  # a gradient under other strides is restrided to q's
    torch.cuda.synchronize()
    for g, x, cu in ((q.grad, q, cu_q), (k.grad, k, cu_k), (v.grad, v, cu_k)):
        assert g.dtype == x.dtype and g.shape == x.shape
        assert not bool(g[int(cu[-1]):].any()), "tokens owned by nobody get a zero gradient"
    for b, seq in enumerate(seqs):
        qb, kb, vb, dob = (to_dev(x[None], dtype) for x in seq)
        qb, kb, vb = (t.requires_grad_(True) for t in (qb, kb, vb))
        ob, _ = torch_op.attention_forward(qb, kb, vb, causal, 0.0)
        assert torch.equal(ob[0], seq_piece(o, cu_q, b))
        ob.backward(dob)
        torch.cuda.synchronize()
        for name, g, ref, cu in (("dQ", q.grad, qb.grad, cu_q), ("dK", k.grad, kb.grad, cu_k), ("dV", v.grad, vb.grad, cu_k)):
            assert torch.equal(seq_piece(g, cu, b), ref[0]), (b, name)
    o2, lse2 = torch_op.attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), max_q, max_k, causal, 0.0)
    with pytest.raises(Exception, match="LSE"):  # no gradient through the LSE output
        lse2[:, :int(cu_q[-1])].sum().backward()


def test_wrapper_refuses_a_short_workspace_and_foreign_outputs(fa):
    import torch

    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16, device="cuda")
    k = torch.zeros(12, 2, 64, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(4, 10, device="cuda")
    cu = cu_dev([0, 4, 10])
    bw = fa.flash_attention_varlen_backward
    with pytest.raises(ValueError, match="workspace of 100 bytes"):
        bw(q, k, k, q, q, lse, cu, cu, 10, 12, workspace=torch.zeros(100, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="dq must be an fp32 device tensor"):
        bw(q, k, k, q, q, lse, cu, cu, 10, 12, dq=torch.zeros(10, 4, 64, device="cuda").half())
    with pytest.raises(ValueError, match="dk must be an fp32 device tensor"):
        bw(q, k, k, q, q, lse, cu, cu, 10, 12, dk=torch.zeros(2, 12, 64, device="cuda").transpose(0, 1))
