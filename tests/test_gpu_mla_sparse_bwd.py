"""GPU: fa_bwd_mla_sparse -- every element of dq and dkv inside the derived bound of tests/mla_sparse_bwd.py on tests/mla_sparse.py's cases
(reference O / LSE, and the forward's own); footprint and strides; exact probes; poisoned workspace, graph replay; autograd through the op."""
import numpy as np
import pytest

import backward_bound as bb
import mla_sparse
import mla_sparse_bwd as sb
from test_gpu_mla_decode import _dev, _i32, _pool_view, _same_bits, fa  # noqa: F401  (fa: the fixture)

pytestmark = pytest.mark.gpu
DQK, DV, SCALE = sb.DQK, sb.DV, sb.SCALE


def inputs(c, r, dtype, o=None, lse=None):
    # device [q, pool view, o, d_o, lse, indices, counts]; o / lse default to the reference's (O rounded to the type)
    import torch

    o = _dev(bb.rnd(r["o"].astype(np.float32), dtype), dtype) if o is None else o
    lse = torch.from_numpy(r["lse"].astype(np.float32)).cuda() if lse is None else lse
    cnt = None if c["counts"] is None else _i32(c["counts"])
    return [_dev(c["q"], dtype), _pool_view(c["pool"], dtype, c["P"])[1], o, _dev(r["do"], dtype), lse, _i32(c["indices"])[:, :c["topk"]], cnt]


def call(fa, a, **kw):
    import torch

    dq, dkv = fa.flash_attention_mla_sparse_backward(*a[:6], a[6], scale=SCALE, **kw)
    torch.cuda.synchronize()
    return dq, dkv


def host(dq, dkv):
    return dq.cpu().numpy().astype(np.float64), dkv.cpu().numpy().astype(np.float64).reshape(-1, DQK)


@pytest.mark.parametrize("idx,dtype,chain", [(i, d, False) for i in range(len(mla_sparse.CASES)) for d in ("bf16", "f16")] + [(3, "bf16", True), (4, "f16", True)])
def test_parity_per_element(fa, idx, dtype, chain):
    c, r = mla_sparse.case(idx, dtype), sb.problem(idx, dtype, chain)
    a = inputs(c, r, dtype)
    if chain:  # the O and LSE that the forward itself wrote, against the bound of the true gradient
        a[2], a[4] = fa.flash_attention_mla_decode_sparse(a[0], a[1], a[5], SCALE, index_counts=a[6])
    dq, dkv = host(*call(fa, a))
    assert max(sb.worst(r, dq, dkv, what=(mla_sparse.CASES[idx], dtype, chain))) <= 1.0 and not dkv[~r["named"]].any()


@pytest.mark.parametrize("idx,dtype", [(1, "bf16"), (5, "f16"), (8, "bf16")])
def test_footprint_and_strides(fa, idx, dtype):
    """wide NaN-filled q / o / d_o, sentinel-filled dq / dkv, NaN in unnamed pool rows, wild entries behind n_t: dq's bits, nothing else moved"""
    import torch

    c, r = mla_sparse.case(idx, dtype), sb.problem(idx, dtype)
    a = inputs(c, r, dtype)
    dq0, _ = call(fa, a)
    T, Hq, P = c["T"], c["Hq"], c["P"]
    named = torch.from_numpy(r["named"].reshape(-1, P)).cuda()
    w = list(a)
    for i, D in ((0, DQK), (2, DV), (3, DV)):
        buf = torch.full((T, Hq + 1, 640), float("nan"), dtype=a[i].dtype, device="cuda")
        buf[:, :Hq, :D] = a[i]
        w[i] = buf[:, :Hq, :D]
    w[1] = torch.where(named[:, :, None], a[1], torch.full_like(a[1], float("nan")))
    wild = np.resize(np.array([2 ** 31 - 1, -1, 12345678, -(2 ** 31)], np.int32), (T, (c["topk"] + 11) // 4 * 4))
    for t, n in enumerate(c["lens"]):
        wild[t, :n] = c["indices"][t, :n]
    w[5] = _i32(wild)[:, :c["topk"]]
    dq_buf = torch.full((T, Hq + 1, 640), 77.0, dtype=torch.float32, device="cuda")
    dkv_buf = torch.full((named.shape[0], P + 1, 648), 77.0, dtype=torch.float32, device="cuda")
    dkv_buf[:, :P, :DQK] = torch.where(named[:, :, None], 0.0, 77.0)
    dq, dkv = call(fa, w, dq=dq_buf[:, :Hq, :DQK], dkv=dkv_buf[:, :P, :DQK])
    assert _same_bits(dq, dq0) and (dq_buf[:, :Hq, DQK:] == 77.0).all() and (dq_buf[:, Hq:] == 77.0).all()
    assert (dkv_buf[:, :P, DQK:] == 77.0).all() and (dkv_buf[:, P:] == 77.0).all() and (dkv[~named] == 77.0).all()
    dkv_h = np.where(r["named"][:, None], dkv.cpu().numpy().astype(np.float64).reshape(-1, DQK), 0.0)
    assert max(sb.worst(r, dq.cpu().numpy().astype(np.float64), dkv_h, what=("wide", mla_sparse.CASES[idx], dtype))) <= 1.0


def test_exact_probes(fa):
    """d_o = 0: dq = 0, dkv keeps its content; two calls into one buffer: twice the gradient. n_t = 0: dq = 0, nothing touched. One entry
    under q = 0: P = 1, dS = 0, dq = 0, the row's value side the exact head sum of dO (quarters: every fp32 sum is exact)"""
    import torch

    c, r = mla_sparse.case(3, "bf16"), sb.problem(3, "bf16")
    a = inputs(c, r, "bf16")
    prior = torch.randn((c["pool"].shape[0], c["P"], DQK), dtype=torch.float32, device="cuda")
    dq, dkv = call(fa, a[:3] + [torch.zeros_like(a[3])] + a[4:], dkv=prior.clone())
    assert not dq.any() and torch.equal(dkv, prior)
    _, dkv = call(fa, a)
    dq2, dkv2 = call(fa, a, dkv=dkv)
    assert max(sb.worst(r, 2.0 * dq2.cpu().numpy().astype(np.float64), host(dq2, dkv2)[1], 2.0, "accumulated twice")) <= 1.0
    rng = np.random.default_rng(8899)
    T, Hq, P, pages, x = 2, 33, 16, 4, 37
    do = _dev(rng.integers(-4, 5, (T, Hq, DV)) / 4.0, "bf16")
    pool = _dev(rng.integers(-4, 5, (pages, P, DQK)) / 4.0, "bf16")
    o = pool.reshape(-1, DQK)[x, :DV].expand(T, Hq, DV).contiguous()
    lse = torch.tensor([[float("nan")] * Hq, [0.0] * Hq], dtype=torch.float32, device="cuda")  # (n_t = 0 is known by the integer)
    idx = _i32(np.array([[x, 5, 6, 7], [x, -1, 2 ** 31 - 1, 9]]))
    dq, dkv = call(fa, [torch.zeros((T, Hq, DQK), dtype=torch.bfloat16, device="cuda"), pool, o, do, lse, idx, _i32(np.array([0, 1]))])
    want = torch.zeros_like(dkv).reshape(-1, DQK)
    want[x, :DV] = do[1].float().sum(0)
    assert not dq.any() and torch.equal(dkv.reshape(-1, DQK), want)


def test_poisoned_workspace_two_runs_and_a_replayed_graph(fa):
    import torch

    c, r = mla_sparse.case(7, "bf16"), sb.problem(7, "bf16")
    a = inputs(c, r, "bf16")
    dq0, dkv0 = call(fa, a)
    ws = torch.full((fa.mla_sparse_backward_workspace_bytes(c["T"], c["Hq"]),), 0xFF, dtype=torch.uint8, device="cuda")
    dq1, dkv1 = call(fa, a, workspace=ws)
    assert _same_bits(dq0, dq1) and max(sb.worst(r, *host(dq1, dkv1), what="0xFF workspace")) <= 1.0
    # the graph is captured on other data: q = 0, lists reversed, counts 0; the case's data then arrive in place
    g = [torch.zeros_like(a[0]), a[1].contiguous(), torch.zeros_like(a[2]), torch.zeros_like(a[3]), torch.zeros_like(a[4]),
         a[5].flip(1).contiguous(), torch.zeros_like(a[6])]
    dq, dkv = torch.empty_like(dq0), torch.zeros_like(dkv0)
    call(fa, g, dq=dq, dkv=dkv, workspace=ws)  # (warm-up: the kernel's attributes are set outside the capture)
    graph, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=s):
        fa.flash_attention_mla_sparse_backward(*g[:6], g[6], scale=SCALE, dq=dq, dkv=dkv, workspace=ws, stream=s.cuda_stream)
    graph.replay()
    torch.cuda.synchronize()
    assert not dq.any() and not dkv.any()
    for dst, src in zip(g, a):
        dst.copy_(src)
    for _ in range(2):
        dkv.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(dq, dq0) and max(sb.worst(r, *host(dq, dkv), what="graph replay")) <= 1.0


def test_autograd_through_the_op(fa):
    import torch

    from flash_attention_metal_amd import torch_op

    idx, dtype = 2, "bf16"  # 17 heads, a list that names seven slots again and again
    c, r = mla_sparse.case(idx, dtype), sb.problem(idx, dtype, True)
    a = inputs(c, r, dtype)
    q, pool = a[0].requires_grad_(), a[1].contiguous().requires_grad_()
    o, lse = torch_op.attention_mla_sparse(q, pool, a[5], a[6], SCALE)
    (o.float() * a[3].float()).sum().backward()
    dq, _ = call(fa, [q.detach(), pool.detach(), o.detach(), a[3], lse.detach(), a[5], a[6]])
    assert _same_bits(q.grad, dq.to(q.dtype)) and pool.grad.dtype == pool.dtype and pool.grad.shape == pool.shape
    gkv = pool.grad.float().cpu().numpy().astype(np.float64).reshape(-1, DQK)
    wide = r["dkv_bound"] + bb.U[dtype] * (np.abs(r["dkv"]) + r["dkv_bound"])  # one rounding to the type
    assert bb.ratios((gkv,), (r["dkv"],), (wide,))[0] <= 1.0 and not gkv[~r["named"]].any()
    with pytest.raises(NotImplementedError, match="LSE"):
        o2, lse2 = torch_op.attention_mla_sparse(q, pool, a[5], a[6], SCALE)
        lse2.sum().backward()
