"""GPU: fa_fwd_mla_decode_sparse (absorbed MLA decode over a list of slots per query token; include/fa_mi355.h) -- every element of O and
LSE against the fp64 reference on the cases tests/test_mla_sparse_cases.py holds the bars on (tests/mla.py's bars, unchanged), and
BIT-IDENTITY with fa_fwd_mla_decode_paged_wide on the twin pool into which the listed rows were copied in list order (the test with
teeth for the gather: a wrong slot address, a wrong list, a wrong count or a race in the shared tile shows as different bits); the split
cases at topk = 2048; entries outside the pool as zero rows; what stands behind the count, in unlisted slots and in the workspace has no
influence; exact answers; the write footprint; two runs alike; a graph replayed after lists, counts and rows changed in place.
Worst error / bar measured on an MI355X over the 18 parity cases (printed by the tests): strict O 2.7e-3 / 6e-3 (bf16), 4.0e-4 / 1.5e-3
(f16); strict LSE 8.0e-7 / 1e-4 (both); every case bit-identical to its twin; see README.md, round 30."""
import numpy as np
import pytest

import mla
import mla_sparse
from test_gpu_mla_decode import _dev, _i32, _np, _pool_view, _same_bits, fa  # noqa: F401  (fa: the fixture)

pytestmark = pytest.mark.gpu

DQK, DV, SCALE = mla.DQK, mla.DV, mla.SCALE


def run(fa, q, view, indices, counts, dtype, padded_q=False, wide_o=False, **kw):
    """q fp32 numpy [T,Hq,576], indices numpy [T, pitch] (the call takes its first topk = kw.pop("topk") columns), counts numpy or None ->
    (O, LSE) device tensors; padded_q: q rows of 640 with a spare head behind every token; wide_o: O rows of 640 inside a sentinel-filled
    buffer whose write footprint is asserted"""
    import torch

    topk = kw.pop("topk", indices.shape[1])
    T, Hq, _ = q.shape
    qd = _dev(q, dtype)
    if padded_q:
        qbuf = torch.full((T, Hq + 1, 640), float("nan"), dtype=qd.dtype, device="cuda")
        qbuf[:, :Hq, :DQK] = qd
        qd = qbuf[:, :Hq, :DQK]
    out = None
    if wide_o:
        buf = torch.full((T, Hq + 1, 640), 77.0, dtype=qd.dtype, device="cuda")
        out = buf[:, :Hq, :DV]
    idx = indices if isinstance(indices, torch.Tensor) else _i32(indices)
    cnt = counts if counts is None or isinstance(counts, torch.Tensor) else _i32(counts)
    o, lse = fa.flash_attention_mla_decode_sparse(qd, view, idx[:, :topk], SCALE, index_counts=cnt, out=out, **kw)
    torch.cuda.synchronize()
    if wide_o:  # the write footprint: nothing behind column 511 of a row, nothing between the tokens
        assert (buf[:, :Hq, DV:] == 77.0).all() and (buf[:, Hq:] == 77.0).all()
    return o, lse


def twin_run(fa, c, dtype, seed):
    """fa_fwd_mla_decode_paged_wide(B = T, Nq = 1, P = 64, cap / 64 pages, not causal, seqlens_k = n) on the twin of case-like dict c"""
    import torch

    pool, table, lens = mla_sparse.twin(c, np.random.default_rng(seed))
    o, lse = fa.flash_attention_mla_decode_paged(_dev(mla_sparse.q4(c["q"]), dtype), _dev(pool, dtype), _i32(table), _i32(lens), SCALE,
                                                 is_causal=False, wide=True)
    torch.cuda.synchronize()
    return o[:, :, 0], lse[:, :, 0]


def both(fa, oracle_mod, c, dtype, what, **kw):
    """the sparse call on c, held to the four bars and to the bits of the wide call on the twin"""
    view = _pool_view(c["pool"], dtype, c["P"])[1]
    o, lse = run(fa, c["q"], view, c["indices"], c["counts"], dtype, topk=c["topk"], **kw)
    ot, lt = twin_run(fa, c, dtype, 7)
    on, ln = _np(o, lse)
    mla.check(oracle_mod, on[:, :, None], ln[:, :, None], mla_sparse.q4(c["q"]), c["kvs"], c["lens"], False, dtype, what)
    assert _same_bits(o, ot) and _same_bits(lse, lt), what
    return o, lse


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("idx", range(len(mla_sparse.CASES)))
def test_parity_against_fp64_and_the_bits_of_the_wide_call_on_the_twin(fa, oracle_mod, idx, dtype):
    c = mla_sparse.case(idx, dtype)
    both(fa, oracle_mod, c, dtype, ("gpu sparse", mla_sparse.CASES[idx], dtype), padded_q=idx % 2 == 1, wide_o=idx % 3 == 1)


def _big(oracle_mod, rng, T, Hq, counts, dtype="bf16", topk=2048, P=64, nslots=8192):
    c = {"Hq": Hq, "topk": topk, "P": P, "dtype": dtype, "T": T, "kind": "perm",
         "q": oracle_mod.round_to(rng.uniform(-1.0, 1.0, (T, Hq, DQK)).astype(np.float32), dtype),
         "pool": mla_sparse.make_pool(oracle_mod, rng, P, nslots, dtype),
         "indices": mla_sparse.make_lists(rng, T, topk, topk, nslots, "perm"),
         "counts": None if counts is None else np.array(counts, np.int32)}
    c["kvs"], c["lens"] = mla_sparse.gather(c)
    return c


@pytest.mark.parametrize("T,Hq,counts", [(1, 16, None), (1, 16, [65]), (2, 128, [2048, 1000])])
def test_split_cases(fa, oracle_mod, T, Hq, counts):
    """topk = 2048: 32 tiles in eight splits of four (tests/test_mla_sparse_cases.py); with a count of 65 all splits but two are empty --
    their workgroups meet one barrier, stage nothing and write (0, -inf, 0)"""
    assert fa.mla_decode_sparse_workspace_bytes(T, Hq, DV, 2048) == T * 8 * -(-Hq // 16) * 16 * 514 * 4  # S = 8
    c = _big(oracle_mod, np.random.default_rng(3100 + T + Hq), T, Hq, counts)
    both(fa, oracle_mod, c, "bf16", ("sparse splits", T, Hq, counts))


def test_what_nobody_names_has_no_influence(fa, oracle_mod):
    """arbitrary values behind the count, NaN in every slot no list names, a NaN-filled workspace with a canary behind it, lse = None,
    a second run: the same bits"""
    import torch

    dtype = "bf16"
    c = dict(mla_sparse.case(3, dtype))  # 33 heads, topk = 65 at a pitch of 72, counts 0 .. 65
    T, Hq, topk, P = c["T"], c["Hq"], c["topk"], c["P"]
    view = _pool_view(c["pool"], dtype, P)[1]
    o1, l1 = run(fa, c["q"], view, c["indices"], c["counts"], dtype, topk=topk)
    # (a) entries behind n_t: negative, huge, outside the pool
    idx = c["indices"].copy()
    rng = np.random.default_rng(3201)
    for t in range(T):
        n = c["lens"][t]
        idx[t, n:] = rng.choice(np.array([-1, -(2 ** 31), 2 ** 31 - 1, 2 ** 30, P * view.shape[0], 12345678], np.int64), idx.shape[1] - n).astype(np.int32)
    o2, l2 = run(fa, c["q"], view, idx, c["counts"], dtype, topk=topk)
    assert _same_bits(o1, o2) and _same_bits(l1, l2)
    # (b) NaN in every slot that no counted entry names
    named = np.zeros(view.shape[0] * P, bool)
    for t in range(T):
        named[c["indices"][t, :c["lens"][t]]] = True
    pool = c["pool"].copy()
    pool[:, :P][~named.reshape(-1, P)] = np.nan
    assert np.isnan(pool[:, :P, 0]).sum() == (~named).sum() > 0
    o3, l3 = run(fa, c["q"], _pool_view(pool, dtype, P)[1], idx, c["counts"], dtype, topk=topk)
    assert _same_bits(o1, o3) and _same_bits(l1, l3) and torch.isfinite(o3).all()
    # (c) the workspace: NaN-filled, a canary behind it (three 16-row slots per item: the fourth wave has none); lse = None
    need = fa.mla_decode_sparse_workspace_bytes(T, Hq, DV, topk)
    assert need % (3 * 16 * 514 * 4) == 0
    buf = torch.full((need + 16 * 514 * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    o4, l4 = run(fa, c["q"], view, c["indices"], c["counts"], dtype, topk=topk, workspace=buf[:need], return_lse=False)
    assert l4 is None and _same_bits(o1, o4) and (buf[need:] == 0xFF).all()
    # (d) the token with no entry: O = 0 exactly, LSE = -inf
    dead = c["lens"].index(0)
    assert (o1[dead] == 0).all() and torch.isneginf(l1[dead]).all()
    live = [t for t in range(T) if c["lens"][t] > 0]
    assert torch.isfinite(l1[live]).all()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_exact_answers(fa, oracle_mod, dtype):
    import torch

    rng = np.random.default_rng(3301)
    P, nslots = 16, 1024
    # (a) one listed key returns its first 512 elements bit for bit, at 33 heads and at 128, at one split (topk = 1) and at eight (2048)
    pool = mla_sparse.make_pool(oracle_mod, rng, P, nslots, dtype, 640, True)
    view = _pool_view(pool, dtype, P)[1]
    for Hq in (33, 128):
        for topk in (1, 2048):
            q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (2, Hq, DQK)).astype(np.float32), dtype)
            idx = mla_sparse.make_lists(rng, 2, topk, -(-topk // 4) * 4, nslots, "perm")
            o, lse = run(fa, q, view, idx, np.array([1, 1], np.int32), dtype, topk=topk)
            for t in range(2):
                x = int(idx[t, 0])
                want = _dev(np.broadcast_to(pool[x // P, x % P, :DV], (Hq, DV)), dtype)
                assert _same_bits(o[t], want), (dtype, Hq, topk, t)
    # (b) q = 0: LSE = ln n, O = the mean of integer-valued latent rows (exact sums), duplicates counted as often as they are named
    Hq, topk = 16, 200
    ipool = np.full((nslots // P, P, DQK), np.nan, np.float32)
    ipool[:] = rng.integers(-4, 5, ipool.shape).astype(np.float32)
    idx = mla_sparse.make_lists(rng, 4, topk, topk, nslots, "perm")
    idx[3, :topk] = rng.choice(idx[3, :5], topk)  # a list of five slots named 200 times
    counts = [1, 37, 64, 200]
    o, lse = run(fa, np.zeros((4, Hq, DQK), np.float32), _dev(ipool, dtype), idx, np.array(counts, np.int32), dtype)
    on, ln = _np(o, lse)
    for t, n in enumerate(counts):
        assert np.abs(ln[t] - np.log(n)).max() < 1e-6 * max(1.0, np.log(n)) + 1e-6, (t, n)
        mean = ipool.reshape(-1, DQK)[idx[t, :n], :DV].astype(np.float64).mean(0)
        rounded = _dev(mean.astype(np.float32), dtype).float().cpu().numpy()
        # the sums are exact in fp32 and the probabilities all equal 1: what is left is sum * (1 / n) in fp32 and one rounding to the
        # output type, which may fall on the other side of a tie: one ulp of the output type (2^-7 / 2^-10 of the value)
        ulp = 2.0 ** -7 if dtype == "bf16" else 2.0 ** -10
        assert (np.abs(on[t] - rounded[None]) <= np.abs(rounded)[None] * ulp + 1e-30).all(), (t, n)
    assert torch.isfinite(o).all()


def test_graph_replay_after_lists_counts_and_rows_changed_in_place(fa, oracle_mod):
    import torch

    dtype = "bf16"
    rng = np.random.default_rng(3401)
    a = _big(oracle_mod, rng, 3, 16, [100, 320, 64], topk=320, nslots=2048)
    b = _big(oracle_mod, rng, 3, 16, [320, 3, 129], topk=320, nslots=2048)
    b["q"] = a["q"]
    qd, pd, idx, cnt = _dev(a["q"], dtype), _dev(a["pool"], dtype), _i32(a["indices"]), _i32(a["counts"])
    out = torch.empty((3, 16, DV), dtype=qd.dtype, device="cuda")
    lse = torch.empty((3, 16), dtype=torch.float32, device="cuda")
    ws = torch.empty(fa.mla_decode_sparse_workspace_bytes(3, 16, DV, 320), dtype=torch.uint8, device="cuda")
    call = lambda: fa.flash_attention_mla_decode_sparse(qd, pd, idx, SCALE, index_counts=cnt, out=out, lse=lse, workspace=ws)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # a warm-up call outside the capture (the first call sets the kernel's LDS attribute)
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    g.replay()
    torch.cuda.synchronize()
    on, ln = _np(out, lse)
    mla.check(oracle_mod, on[:, :, None], ln[:, :, None], mla_sparse.q4(a["q"]), a["kvs"], a["lens"], False, dtype, "sparse graph, first replay")
    pd.copy_(_dev(b["pool"], dtype))
    idx.copy_(_i32(b["indices"]))
    cnt.copy_(_i32(b["counts"]))
    g.replay()
    torch.cuda.synchronize()
    on, ln = _np(out, lse)
    mla.check(oracle_mod, on[:, :, None], ln[:, :, None], mla_sparse.q4(b["q"]), b["kvs"], b["lens"], False, dtype, "sparse graph, replay after the change")


def test_the_wrapper_refuses_what_it_cannot_pass_on(fa, oracle_mod):
    import torch

    c = mla_sparse.case(1, "bf16")
    view = _pool_view(c["pool"], "bf16", c["P"])[1]
    qd, idx = _dev(c["q"], "bf16"), _i32(c["indices"])
    with pytest.raises(ValueError, match="needs the model's scale"):
        fa.flash_attention_mla_decode_sparse(qd, view, idx, None)
    with pytest.raises(ValueError, match="no CPU path"):
        fa.flash_attention_mla_decode_sparse(qd, view, idx.cpu(), SCALE)
    with pytest.raises(ValueError, match="int32 \\[T, topk\\]"):
        fa.flash_attention_mla_decode_sparse(qd, view, idx.long(), SCALE)
    with pytest.raises(ValueError, match="index_counts"):
        fa.flash_attention_mla_decode_sparse(qd, view, idx, SCALE, index_counts=torch.zeros(c["T"] + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(fa.FaError, match="indices_stride=63 must be a multiple of 4"):
        fa.flash_attention_mla_decode_sparse(qd, view, idx[:, :63].contiguous(), SCALE)
    with pytest.raises(fa.FaError, match="Hq <= 128 heads"):
        fa.flash_attention_mla_decode_sparse(torch.zeros((1, 129, DQK), dtype=qd.dtype, device="cuda"), view, idx[:1], SCALE)
