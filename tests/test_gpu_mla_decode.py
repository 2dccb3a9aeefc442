"""GPU: fa_fwd_mla_decode_paged (absorbed MLA decode over a paged latent cache; include/fa_mi355.h) -- every element of O and LSE against
the fp64 reference of tests/mla.py on the cases tests/test_mla_cases.py holds the bars on, exact answers, the separation of the score's
576 columns from the value's 512, the write footprint, robustness against what the pool, the tables and the workspace hold where nobody
may look, the chain behind fa_kv_append_paged on the aliased pool, and a graph replayed after everything changed in place.
Worst error / bar measured on an MI355X over the 36 parity cases (printed by the tests): strict O 2.7e-3 / 6e-3 (bf16), 3.1e-4 / 1.5e-3
(f16); strict LSE 1.3e-6 / 1e-4 (both); see README.md, round 24."""
import numpy as np
import pytest

import mla
from util import TORCH_DTYPE

pytestmark = pytest.mark.gpu

DQK, DV, SCALE = mla.DQK, mla.DV, mla.SCALE


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

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def _pool_view(pool, dtype, P):
    """the device pool with its padding rows and columns, and the [num_pages, P, 576] view the call takes"""
    full = _dev(pool, dtype)
    return full, full[:, :P, :DQK]


def _np(o, lse):
    return o.float().cpu().numpy().astype(np.float64), (None if lse is None else lse.cpu().numpy().astype(np.float64))


def _bits(t):
    import torch

    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def run(fa, q, view, table, lens, causal, dtype, token_major=False, wide_o=False, **kw):
    """q fp32 numpy [B,Hq,Nq,576] -> (O, LSE) device tensors; token_major: q lives as [B,Nq,Hq,576]; wide_o: O rows of 640 inside a
    sentinel-filled buffer, returned with that buffer"""
    import torch

    qd = _dev(q, dtype)
    if token_major:
        qd = qd.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    out = None
    if wide_o:
        B, Hq, Nq, _ = q.shape
        buf = torch.full((B, Hq, Nq + 1, 640), 77.0, dtype=qd.dtype, device="cuda")
        out = buf[:, :, :Nq, :DV]
    o, lse = fa.flash_attention_mla_decode_paged(qd, view, _i32(table), _i32(lens), SCALE, is_causal=causal, out=out, **kw)
    torch.cuda.synchronize()
    if wide_o:  # the write footprint: nothing behind column 511 of a row, nothing between the rows
        assert (buf[:, :, :Nq, DV:] == 77.0).all() and (buf[:, :, Nq:] == 77.0).all()
    return o, lse


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("P", mla.PAGES)
@pytest.mark.parametrize("idx", range(len(mla.SHAPES)))
def test_parity_against_fp64(fa, oracle_mod, idx, P, dtype):
    c = mla.case(P, dtype, idx)
    _, view = _pool_view(c["pool"], dtype, P)
    o, lse = run(fa, c["q"], view, c["table"], c["lens"], c["causal"], dtype, c["token_major"], c["wide_o"])
    mla.check(oracle_mod, *_np(o, lse), c["q"], c["kvs"], c["lens"], c["causal"], dtype, ("gpu", mla.SHAPES[idx], P, dtype))


@pytest.mark.parametrize("L", [16384, 100])
def test_many_splits_on_one_sequence(fa, oracle_mod, L):
    """B = 1 at a capacity of 65536 keys: 256 splits; with 16384 keys every split has a tile, with 100 keys all but two are empty"""
    dtype, P = "bf16", 64
    rng = np.random.default_rng(7 + L)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (1, 16, 2, DQK)).astype(np.float32), dtype)
    pool, table, kvs = mla.make_pool(oracle_mod, rng, P, [L], dtype, max_pages=65536 // P)
    assert fa.mla_decode_paged_workspace_bytes(1, 16, 2, DV, P, 65536 // P) == 128 * 32 * 514 * 4  # S = 128 per row block pair
    o, lse = run(fa, q, _pool_view(pool, dtype, P)[1], table, [L], True, dtype)
    mla.check(oracle_mod, *_np(o, lse), q, kvs, [L], True, dtype, ("splits", L))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_exact_answers(fa, oracle_mod, dtype):
    import torch

    P, Hq, Nq = 16, 8, 4
    rng = np.random.default_rng(11)
    # (a) causal row 0 with L_b = Nq sees exactly key 0: its first 512 elements, bit for bit -- at one split and at many (a large capacity)
    for max_pages in (1, 4096):
        lens = [Nq, Nq]
        q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (2, Hq, Nq, DQK)).astype(np.float32), dtype)
        pool, table, kvs = mla.make_pool(oracle_mod, rng, P, lens, dtype, max_pages=max_pages)
        o, lse = run(fa, q, _pool_view(pool, dtype, P)[1], table, lens, True, dtype)
        for b in range(2):
            want = _dev(np.broadcast_to(kvs[b][0, :DV], (Hq, DV)), dtype)
            assert _same_bits(o[b, :, 0], want), (dtype, max_pages, b)
    # (b) q = 0: LSE = ln(visible keys), O = the mean of integer-valued latent rows (exact sums; the bars are the parity test's)
    lens = [1, 37, 64, 200]
    pool, table, kvs = mla.make_pool(oracle_mod, rng, P, lens, dtype, integer=True)
    q = np.zeros((4, Hq, Nq, DQK), np.float32)
    o, lse = run(fa, q, _pool_view(pool, dtype, P)[1], table, lens, False, dtype)
    on, ln = _np(o, lse)
    for b, L in enumerate(lens):
        assert np.abs(ln[b] - np.log(L)).max() < 1e-6 * max(1.0, np.log(L)) + 1e-6, (b, L)
        mean = kvs[b][:, :DV].astype(np.float64).mean(0)
        rounded = _dev(mean.astype(np.float32), dtype).float().cpu().numpy()
        # the sums are exact in fp32 and the probabilities all equal 1 (exact in every type): what is left is sum * (1 / L) in fp32 and one
        # rounding to the output type, which may fall on the other side of a tie: one ulp of the output type (2^-7 / 2^-10 of the value)
        ulp = 2.0 ** -7 if dtype == "bf16" else 2.0 ** -10
        assert (np.abs(on[b] - rounded[None, None]) <= np.abs(rounded)[None, None] * ulp + 1e-30).all(), (b, L)
    assert torch.isfinite(o).all()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_column_separation(fa, oracle_mod, dtype):
    P, Hq, Nq = 64, 16, 2
    rng = np.random.default_rng(13)
    lens = [1, 65, 130, 700]
    pool, table, kvs = mla.make_pool(oracle_mod, rng, P, lens, dtype)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (4, Hq, Nq, DQK)).astype(np.float32), dtype)
    # q without a rotary part: the pool's columns 512..575 must not matter, 1e4 in them included
    q0 = q.copy()
    q0[..., DV:] = 0.0
    other = pool.copy()
    other[:, :, DV:DQK] = np.where(np.isnan(other[:, :, DV:DQK]), np.nan, 1e4)
    o1, l1 = run(fa, q0, _pool_view(pool, dtype, P)[1], table, lens, True, dtype)
    o2, l2 = run(fa, q0, _pool_view(other, dtype, P)[1], table, lens, True, dtype)
    assert _same_bits(o1, o2) and _same_bits(l1, l2)
    # q with a rotary part only: parity at the bars
    q1 = q.copy()
    q1[..., :DV] = 0.0
    o, lse = run(fa, q1, _pool_view(pool, dtype, P)[1], table, lens, True, dtype)
    mla.check(oracle_mod, *_np(o, lse), q1, kvs, lens, True, dtype, ("rotary only", dtype))


def test_robustness(fa, oracle_mod):
    import torch

    dtype, P, Hq, Nq = "bf16", 16, 16, 2
    rng = np.random.default_rng(17)
    lens = [0, 1, 40, 300, 1000]  # L = 0 and (causal, Nq = 2) L = 1: dead rows
    B = len(lens)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (B, Hq, Nq, DQK)).astype(np.float32), dtype)
    pool, table, kvs = mla.make_pool(oracle_mod, rng, P, lens, dtype, max_pages=80)
    full, view = _pool_view(pool, dtype, P)
    qd, td, ld = _dev(q, dtype), _i32(table), _i32(lens)
    need = fa.mla_decode_paged_workspace_bytes(B, Hq, Nq, DV, P, 80)
    # a NaN-filled workspace with a canary behind it; two runs bit-equal
    buf = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    o1, l1 = fa.flash_attention_mla_decode_paged(qd, view, td, ld, SCALE, is_causal=True, workspace=buf[:need])
    o2, l2 = fa.flash_attention_mla_decode_paged(qd, view, td, ld, SCALE, is_causal=True)
    torch.cuda.synchronize()
    assert (buf[need:] == 0xFF).all() and _same_bits(o1, o2) and _same_bits(l1, l2)
    e = mla.check(oracle_mod, *_np(o1, l1), q, kvs, lens, True, dtype, "robustness")
    on, ln = _np(o1, l1)
    assert np.isneginf(ln[0]).all() and (on[0] == 0).all() and np.isneginf(ln[1, :, 0]).all() and np.isfinite(ln[1, :, 1]).all() and e
    # lse = None
    o3, l3 = fa.flash_attention_mla_decode_paged(qd, view, td, ld, SCALE, is_causal=True, return_lse=False)
    torch.cuda.synchronize()
    assert l3 is None and _same_bits(o1, o3)
    # entries past ceil(L_b / P) have no influence
    t2 = table.copy()
    for b, L in enumerate(lens):
        t2[b, (L + P - 1) // P:] = rng.integers(-5, pool.shape[0] + 5, 80 - (L + P - 1) // P)
    o4, l4 = fa.flash_attention_mla_decode_paged(qd, view, _i32(t2), ld, SCALE, is_causal=True)
    torch.cuda.synchronize()
    assert _same_bits(o1, o4) and _same_bits(l1, l4)
    # a table entry of -1 and one of num_pages: the bits of a pool whose page is zeros
    t3, zp = table.copy(), pool.copy()
    zp[table[3, 2]] = 0.0
    zp[table[4, 5]] = 0.0
    t3[3, 2], t3[4, 5] = -1, pool.shape[0]
    o5, l5 = fa.flash_attention_mla_decode_paged(qd, view, _i32(t3), ld, SCALE, is_causal=True)
    o6, l6 = fa.flash_attention_mla_decode_paged(qd, _pool_view(zp, dtype, P)[1], td, ld, SCALE, is_causal=True)
    torch.cuda.synchronize()
    assert _same_bits(o5, o6) and _same_bits(l5, l6) and not _same_bits(o5, o1)
    assert full.shape[0] == pool.shape[0]


def test_chain_behind_the_append_on_the_aliased_pool(fa, oracle_mod):
    import torch

    dtype, P, Hq, Nq = "bf16", 16, 16, 1
    rng = np.random.default_rng(19)
    before, new = [0, 5, 16, 100], [1, 3, 16, 40]
    lens = [a + n for a, n in zip(before, new)]
    pool, table, kvs = mla.make_pool(oracle_mod, rng, P, lens, dtype)
    direct = _dev(pool, dtype)  # the pool as it should look; untouched slots are NaN
    # the pool before the append: the new slots hold a sentinel, as does everything the direct pool holds NaN in
    start = pool.copy()
    rows = []
    for b in range(len(lens)):
        for j in range(before[b], lens[b]):
            start[table[b, j // P], j % P, :DQK] = np.nan
        rows.append(kvs[b][before[b]:])
    work = _dev(np.where(np.isnan(start), 123.0, start), dtype)
    knew = _dev(np.concatenate(rows), dtype).view(-1, 1, DQK)  # [total_new, 1, 576]
    cu = _i32(np.concatenate([[0], np.cumsum(new)]))
    view4 = work.view(work.shape[0], P, 1, DQK)  # [num_pages, P, 1, 576]: NHD with one latent head
    fa.kv_append_paged(knew, knew, view4, view4, cu, _i32(table), _i32(lens), max(new), layout="NHD")
    torch.cuda.synchronize()
    want = torch.where(torch.isnan(direct), torch.full_like(direct, 123.0), direct)
    assert _same_bits(work, want)  # the appended slots, and nothing else, changed
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (len(lens), Hq, Nq, DQK)).astype(np.float32), dtype)
    o1, l1 = run(fa, q, view4, table, lens, False, dtype)
    o2, l2 = run(fa, q, direct, table, lens, False, dtype)
    assert _same_bits(o1, o2) and _same_bits(l1, l2)
    mla.check(oracle_mod, *_np(o1, l1), q, kvs, lens, False, dtype, "chain")


def test_graph_replay_after_everything_changed_in_place(fa, oracle_mod):
    import torch

    dtype, P, Hq, Nq, mp = "bf16", 64, 16, 2, 16
    rng = np.random.default_rng(23)
    lens_a, lens_b = [100, 1000, 64], [700, 3, 129]
    pool_a, table_a, kvs_a = mla.make_pool(oracle_mod, rng, P, lens_a, dtype, max_pages=mp, spare=20)
    pool_b, table_b, kvs_b = mla.make_pool(oracle_mod, rng, P, lens_b, dtype, max_pages=mp, spare=20 + sum((a + P - 1) // P for a in lens_a) - sum((b + P - 1) // P for b in lens_b))
    assert pool_a.shape == pool_b.shape
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (3, Hq, Nq, DQK)).astype(np.float32), dtype)
    qd, pd, td, ld = _dev(q, dtype), _dev(pool_a, dtype), _i32(table_a), _i32(lens_a)
    out = torch.empty((3, Hq, Nq, DV), dtype=qd.dtype, device="cuda")
    lse = torch.empty((3, Hq, Nq), dtype=torch.float32, device="cuda")
    ws = torch.empty(fa.mla_decode_paged_workspace_bytes(3, Hq, Nq, DV, P, mp), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # a warm-up call outside the capture (the first call sets the kernel's LDS attribute)
        fa.flash_attention_mla_decode_paged(qd, pd, td, ld, SCALE, is_causal=True, out=out, lse=lse, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fa.flash_attention_mla_decode_paged(qd, pd, td, ld, SCALE, is_causal=True, out=out, lse=lse, workspace=ws)
    g.replay()
    torch.cuda.synchronize()
    mla.check(oracle_mod, *_np(out, lse), q, kvs_a, lens_a, True, dtype, "graph, first replay")
    pd.copy_(_dev(pool_b, dtype))
    td.copy_(_i32(table_b))
    ld.copy_(_i32(lens_b))
    g.replay()
    torch.cuda.synchronize()
    mla.check(oracle_mod, *_np(out, lse), q, kvs_b, lens_b, True, dtype, "graph, replay after the change")
