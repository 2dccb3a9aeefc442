"""GPU: fa_mla_sparse_head_probs and fa_mla_indexer_loss_sparse -- every written element inside the derived bounds of
tests/mla_indexer_loss.py (fp64 references on gathered rows), footprints under NaN-filled surroundings, exact probes, and the chain
forward -> head probabilities -> loss through the autograd op and one captured graph."""
import numpy as np
import pytest

import backward_bound as bb
import mla_indexer_loss as il
import mla_sparse
from test_gpu_mla_decode import _dev, _i32, _pool_view, _same_bits, fa  # noqa: F401  (fa: the fixture)

pytestmark = pytest.mark.gpu
SCALE, WILD = mla_sparse.SCALE, np.array([2 ** 31 - 1, -1, 12345678, -(2 ** 31)], np.int32)


def wild_tails(indices, lens, pitch):
    """the lists with entries no pool holds behind every n_t"""
    out = np.resize(WILD, (len(lens), pitch))
    for t, n in enumerate(lens):
        out[t, :n] = indices[t, :n]
    return _i32(out)


def named_only(view, indices, lens, P):
    """the pool with NaN in every row that no list names"""
    import torch

    named = np.zeros(view.shape[0] * P, bool)
    for t, n in enumerate(lens):
        x = indices[t, :n].astype(np.int64)
        named[x[(x >= 0) & (x < named.size)]] = True
    return torch.where(torch.from_numpy(named.reshape(-1, P, 1)).cuda(), view, torch.full_like(view, float("nan")))


@pytest.mark.parametrize("idx,dtype", [(i, d) for i in (0, 1, 2, 3, 5, 6, 8) for d in ("bf16", "f16")])
def test_head_probs_per_element_footprint_and_row_sum(fa, idx, dtype):
    """tests/mla_sparse.py's cases (Hq 1 .. 128, topk 1 .. 320, P 16 / 64 / 256, counts 0 / 1 / mid / topk and NULL, a pitch above topk,
    duplicates, entries outside the pool) on the forward's own LSE, NaN in unnamed rows and wild list tails, a canary behind n_t"""
    import torch

    c = mla_sparse.case(idx, dtype)
    T, topk, lens = c["T"], c["topk"], c["lens"]
    q, view = _dev(c["q"], dtype), named_only(_pool_view(c["pool"], dtype, c["P"])[1], c["indices"], lens, c["P"])
    lists, cnt = wild_tails(c["indices"], lens, c["indices"].shape[1])[:, :topk], None if c["counts"] is None else _i32(c["counts"])
    _, lse = fa.flash_attention_mla_decode_sparse(q, view, lists, SCALE, index_counts=cnt)
    probs = fa.mla_sparse_head_probs(q, view, lse, lists, cnt, SCALE).cpu().numpy()
    # the C call into a wider canary buffer: the same bits in front of n_t, the canary's behind it
    buf = torch.full((T, topk + 5), -77.0, dtype=torch.float32, device="cuda")
    lib = fa.load_library()
    st = lib.fa_mla_sparse_head_probs(q.data_ptr(), view.data_ptr(), lse.data_ptr(), buf.data_ptr(), lists.data_ptr(), None if cnt is None else cnt.data_ptr(),
                                      T, c["Hq"], 576, 512, topk, c["P"], view.shape[0], SCALE, q.stride(0), q.stride(1), view.stride(0), view.stride(1),
                                      lists.stride(0), topk + 5, fa.ops.DTYPES[dtype], None)
    torch.cuda.synchronize()
    assert st == 0, lib.fa_last_error()
    buf, worst = buf.cpu().numpy(), 0.0
    ref, bound = il.probs_reference(c["q"], c["kvs"], lens, lse.cpu().numpy(), SCALE, dtype)
    for t, n in enumerate(lens):
        assert (buf[t, n:] == -77.0).all() and not probs[t, n:].any() and np.array_equal(buf[t, :n], probs[t, :n])
        if n:
            err = np.abs(probs[t, :n].astype(np.float64) - ref[t])
            worst = max(worst, (err / bound[t]).max())
            assert abs(probs[t, :n].astype(np.float64).sum() - c["Hq"]) <= 2 * bound[t].sum() + (n + 64) * bb.U32 * c["Hq"], t
            x = c["indices"][t, :n]
            for j in range(1, n):  # a slot named twice: the same value in both places
                assert x[j] != x[0] or probs[t, j] == probs[t, 0]
    print(mla_sparse.CASES[idx], dtype, "head probs worst error / bound %.3g" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("dtype,Hq,topk", [("bf16", 128, 130), ("f16", 33, 65), ("bf16", 16, 64)])
def test_head_probs_exact_probe(fa, dtype, Hq, topk):
    """scale = ln 2 (scale . log2 e = 1 in fp32), sparse q and rows in {-1, 0, 1}, lse = 0: every P is 2^s, s an integer in [-6, 6], and
    every fp32 sum of at most 128 of them is exact: probs equals the reference bit for bit"""
    import torch

    rng, T, P = np.random.default_rng(9000 + Hq), 3, 16
    sparse = lambda *shape: (rng.integers(-1, 2, shape) * (rng.uniform(0, 1, shape) < 0.02)).astype(np.float32)
    qn, pool = sparse(T, Hq, 576), sparse(64, P, 576)
    qn[:, :, 6:], pool[:, :, 6:] = 0.0, 0.0  # six columns: |s| <= 6
    qn[:, :, :6] = rng.integers(-1, 2, (T, Hq, 6))
    pool[:, :, :6] = rng.integers(-1, 2, (64, P, 6))
    idxs = np.stack([rng.permutation(64 * P)[:(topk + 3) // 4 * 4] for _ in range(T)]).astype(np.int32)  # (a pitch that is a multiple of 4)
    s = np.einsum("thd,tjd->thj", qn.astype(np.float64), pool.reshape(-1, 576)[idxs[:, :topk]].astype(np.float64))
    scale = float(np.float32(np.log(2.0)))
    assert np.float32(scale) * np.float32(1.4426950408889634) == np.float32(1.0)
    out = fa.mla_sparse_head_probs(_dev(qn, dtype), _dev(pool, dtype), torch.zeros((T, Hq), device="cuda"), _i32(idxs)[:, :topk], None, scale)
    assert np.array_equal(out.cpu().numpy(), np.exp2(s).sum(1).astype(np.float32))


def loss_inputs(c, dtype):
    """device [q_idx, w, pool view (NaN in unnamed rows), lists with wild tails, counts, target with NaN behind n_t, loss_grad]"""
    import torch

    P, topk = c["P"], c["topk"]
    pool = named_only(_dev(c["pool"].reshape(-1, P, il.DI), dtype), c["indices"], c["lens"], P)
    tgt = np.array(c["target"], copy=True)
    for t, n in enumerate(c["lens"]):
        tgt[t, n:] = np.nan
    cnt = None if c["counts"] is None else _i32(c["counts"])
    return [_dev(c["q"], dtype), torch.from_numpy(np.array(c["w"])).cuda(), pool, wild_tails(c["indices"], c["lens"], c["indices"].shape[1])[:, :topk], cnt,
            torch.from_numpy(tgt).cuda(), torch.from_numpy(np.array(c["u"])).cuda()]


@pytest.mark.parametrize("idx,dtype", [(i, d) for i in range(len(il.LOSS_CASES)) for d in ("bf16", "f16")])
def test_indexer_loss_per_element(fa, idx, dtype):
    """Hi 32 / 64 x topk 1 / 65 / 320, counts 0 / 1 / mid / topk and NULL, a duplicate, an entry outside the pool, a zero target row, a
    per-token loss_grad: loss, dq, dw and dk inside their bounds, unnamed dk rows untouched, the loss-only call's bits the full call's"""
    import torch

    c = il.loss_case(idx, dtype)
    a, r = loss_inputs(c, dtype), c["ref"]
    loss, dq, dw, dk = fa.mla_indexer_loss_sparse(*a[:6], loss_grad=a[6])
    only = fa.mla_indexer_loss_sparse(*a[:6], need_grads=False)
    torch.cuda.synchronize()
    assert only[1:] == (None, None, None) and _same_bits(only[0], loss)
    dk = dk.cpu().numpy().reshape(-1, il.DI)
    got = [x.cpu().numpy().astype(np.float64) for x in (loss, dq, dw)] + [dk.astype(np.float64)]
    out = bb.ratios(got, (r["loss"], r["dq"], r["dw"], r["dk"]), (r["loss_b"], r["dq_b"], r["dw_b"], r["dk_b"]))
    print(il.LOSS_CASES[idx], dtype, "worst error / bound: loss %.3g dq %.3g dw %.3g dk %.3g" % tuple(out))
    assert max(out) <= 1.0 and not dk[~r["named"]].any() and (np.signbit(dk[~r["named"]]) == 0).all()
    for t, n in enumerate(c["lens"]):
        if n == 0 or not c["target"][t, :n].any():  # no loss: zeros exactly
            assert got[0][t] == 0 and not got[1][t].any() and not got[2][t].any()


def test_chain_autograd_and_graph_replay(fa):
    """forward -> head probabilities -> loss: the autograd op's gradients of (loss . u).sum() are the direct call's (dq, dw bit for bit, dk
    inside twice its bound: two atomic orders), and one captured graph of the three launches follows lists and counts changed in place"""
    import torch
    from flash_attention_metal_amd import torch_op

    dtype, c, lc = "bf16", mla_sparse.case(4, "bf16"), il.loss_case(5, "bf16")  # Hq 64, topk 320, P 64; Hi 64 on the same page size
    T, topk = 3, c["topk"]
    q, view = _dev(c["q"][:T], dtype), _pool_view(c["pool"], dtype, c["P"])[1]
    lists, cnt = _i32(np.array(c["indices"][:T] % il.NSLOTS)), _i32(np.array([topk, 129, 65]))
    qi, w, kpool, u = _dev(lc["q"], dtype), torch.from_numpy(np.array(lc["w"])).cuda(), _dev(lc["pool"].reshape(-1, 64, il.DI), dtype), torch.from_numpy(np.array(lc["u"])).cuda()

    def chain():
        _, lse = fa.flash_attention_mla_decode_sparse(q, view, lists, SCALE, index_counts=cnt)
        return fa.mla_sparse_head_probs(q, view, lse, lists, cnt, SCALE)

    target = chain()
    loss, dq, dw, dk = fa.mla_indexer_loss_sparse(qi, w, kpool, lists, cnt, target, loss_grad=u)
    leaves = [t.clone().requires_grad_() for t in (qi, w, kpool)]
    op_loss = torch_op.mla_indexer_kl_loss(*leaves, lists, cnt, target)
    gq, gw, gk = torch.autograd.grad((op_loss * u).sum(), leaves)
    assert _same_bits(op_loss, loss) and _same_bits(gq, dq.to(qi.dtype)) and _same_bits(gw, dw) and gk.shape == kpool.shape and gk.dtype == kpool.dtype
    assert torch.allclose(gk.float(), dk, rtol=2.0 ** -8, atol=1e-6)  # (the pool's dtype: one rounding to bf16, half an ulp of 2^-8; two atomic orders)
    # one graph over the three launches, replayed after lists and counts change in place
    ws = torch.empty(fa.mla_decode_sparse_workspace_bytes(T, c["Hq"], 512, topk), dtype=torch.uint8, device="cuda")
    o, lse = fa.flash_attention_mla_decode_sparse(q, view, lists, SCALE, index_counts=cnt, workspace=ws)
    probs, g_loss = torch.zeros((T, topk), device="cuda"), torch.empty(T, device="cuda")
    lib, DT = fa.load_library(), fa.ops.DTYPES[dtype]

    def launches(stream):
        fa.flash_attention_mla_decode_sparse(q, view, lists, SCALE, index_counts=cnt, out=o, lse=lse, workspace=ws, stream=stream)
        assert lib.fa_mla_sparse_head_probs(q.data_ptr(), view.data_ptr(), lse.data_ptr(), probs.data_ptr(), lists.data_ptr(), cnt.data_ptr(), T, c["Hq"], 576,
                                            512, topk, c["P"], view.shape[0], SCALE, q.stride(0), q.stride(1), view.stride(0), view.stride(1),
                                            lists.stride(0), topk, DT, stream) == 0
        assert lib.fa_mla_indexer_loss_sparse(qi.data_ptr(), w.data_ptr(), kpool.data_ptr(), lists.data_ptr(), cnt.data_ptr(), probs.data_ptr(), None,
                                              g_loss.data_ptr(), None, None, None, T, 64, il.DI, topk, 64, kpool.shape[0], qi.stride(0), qi.stride(1),
                                              w.stride(0), kpool.stride(0), kpool.stride(1), 0, 0, lists.stride(0), topk, DT, stream) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launches(side.cuda_stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            launches(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    for shift in (0, 7, 19):
        lists.copy_(_i32(np.array((c["indices"][:T] + shift) % il.NSLOTS)))
        cnt.copy_(_i32(np.array([topk - shift, 129 + shift, 65])))
        graph.replay()
        eager = fa.mla_indexer_loss_sparse(qi, w, kpool, lists, cnt, chain(), need_grads=False)[0]
        torch.cuda.synchronize()
        assert _same_bits(g_loss, eager), shift
