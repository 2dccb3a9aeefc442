"""GPU: fa_fwd_mla_decode_paged_wide (absorbed MLA decode for up to 128 packed rows, workgroups of two or four waves over one shared
tile; include/fa_mi355.h) -- every element of O and LSE against the fp64 reference on the cases tests/test_mla_wide_cases.py holds the
bars on (tests/mla.py's bars, unchanged), BIT-IDENTITY with the one-wave call wherever both split the keys alike (the test with teeth
for the shared tile: a race or a wrong piece owner shows as different bits over 65 tiles), many splits with most of them empty, exact
answers, the write footprint and the workspace slot that does not exist, robustness against what the pool, the tables and the workspace
hold where nobody may look, a graph replayed after everything changed in place, and the Python wrapper's routing.
Worst error / bar measured on an MI355X over the 60 parity cases (printed by the tests): strict O 3.0e-3 / 6e-3 (bf16), 3.6e-4 / 1.5e-3
(f16); strict LSE 1.5e-6 / 1e-4 (both); see README.md, round 26."""
import numpy as np
import pytest

import mla
import mla_wide
from test_gpu_mla_decode import _dev, _i32, _np, _pool_view, _same_bits, fa, run  # noqa: F401  (fa: the fixture)

pytestmark = pytest.mark.gpu

DQK, DV, SCALE = mla.DQK, mla.DV, mla.SCALE


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("P", mla_wide.PAGES)
@pytest.mark.parametrize("idx", range(len(mla_wide.SHAPES)))
def test_parity_against_fp64(fa, oracle_mod, idx, P, dtype):
    c = mla_wide.case(P, dtype, idx)
    _, view = _pool_view(c["pool"], dtype, P)
    o, lse = run(fa, c["q"], view, c["table"], c["lens"], c["causal"], dtype, c["token_major"], c["wide_o"], wide=True)
    mla.check(oracle_mod, *_np(o, lse), c["q"], c["kvs"], c["lens"], c["causal"], dtype, ("gpu wide", mla_wide.SHAPES[idx], P, dtype))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("i", range(len(mla_wide.BITID)))
def test_bits_of_the_one_wave_call(fa, oracle_mod, i, dtype):
    """heads [k * heads, (k + 1) * heads) of the wide call == the one-wave call on that slice of q, bit for bit in O and LSE: both split the
    keys alike (asserted on the CPU, tests/test_mla_wide_cases.py) and every wave runs the one-wave item's text on the shared tile"""
    import torch

    (Hq, Nq, causal), heads = mla_wide.BITID[i]
    lens, mp = mla_wide.bitid_capacity(i)
    P = mla_wide.BITID_P
    rng = np.random.default_rng(2650 + i)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (len(lens), Hq, Nq, DQK)).astype(np.float32), dtype)
    pool, table, kvs = mla.make_pool(oracle_mod, rng, P, lens, dtype, max_pages=mp)
    view = _pool_view(pool, dtype, P)[1]
    qd, td, ld = _dev(q, dtype), _i32(table), _i32(lens)
    o, lse = fa.flash_attention_mla_decode_paged(qd, view, td, ld, SCALE, is_causal=causal, wide=True)
    for k in range(Hq // heads):
        part = slice(k * heads, (k + 1) * heads)
        o1, l1 = fa.flash_attention_mla_decode_paged(qd[:, part], view, td, ld, SCALE, is_causal=causal, wide=False)
        torch.cuda.synchronize()
        assert _same_bits(o[:, part], o1) and _same_bits(lse[:, part], l1), (mla_wide.BITID[i], dtype, k)
    mla.check(oracle_mod, *_np(o, lse), q, kvs, lens, causal, dtype, ("bits", mla_wide.BITID[i], dtype))


@pytest.mark.parametrize("L", [16384, 100])
def test_many_splits_on_one_sequence(fa, oracle_mod, L):
    """B = 1 at a capacity of 65536 keys, one block of 64 rows: 256 splits; with 16384 keys every split has a tile, with 100 keys all but two
    are empty -- their workgroups meet one barrier, stage nothing and write (0, -inf, 0)"""
    dtype, P = "bf16", 64
    rng = np.random.default_rng(2607 + L)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (1, 16, 4, DQK)).astype(np.float32), dtype)
    pool, table, kvs = mla.make_pool(oracle_mod, rng, P, [L], dtype, max_pages=65536 // P)
    assert fa.mla_decode_paged_wide_workspace_bytes(1, 16, 4, DV, P, 65536 // P) == 256 * 64 * 514 * 4  # S = 256
    o, lse = run(fa, q, _pool_view(pool, dtype, P)[1], table, [L], True, dtype, wide=True)
    mla.check(oracle_mod, *_np(o, lse), q, kvs, [L], True, dtype, ("wide splits", L))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_exact_answers(fa, oracle_mod, dtype):
    import torch

    P = 16
    rng = np.random.default_rng(2611)
    # (a) one visible key returns its first 512 elements bit for bit, at 33 rows (a lone row in the third wave) and at 128 (two blocks):
    # L_b = 1 and Nq = 1 -- at one split and at many (a large capacity)
    for Hq in (33, 128):
        for max_pages in (1, 4096):
            lens = [1, 1]
            q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (2, Hq, 1, DQK)).astype(np.float32), dtype)
            pool, table, kvs = mla.make_pool(oracle_mod, rng, P, lens, dtype, max_pages=max_pages)
            o, lse = run(fa, q, _pool_view(pool, dtype, P)[1], table, lens, True, dtype, wide=True)
            for b in range(2):
                want = _dev(np.broadcast_to(kvs[b][0, :DV], (Hq, DV)), dtype)
                assert _same_bits(o[b, :, 0], want), (dtype, Hq, max_pages, b)
    # (b) q = 0: LSE = ln(visible keys), O = the mean of integer-valued latent rows (exact sums), at 16 x 3 = 48 rows
    Hq, Nq = 16, 3
    lens = [1, 37, 64, 200]
    pool, table, kvs = mla.make_pool(oracle_mod, rng, P, lens, dtype, integer=True)
    q = np.zeros((4, Hq, Nq, DQK), np.float32)
    o, lse = run(fa, q, _pool_view(pool, dtype, P)[1], table, lens, False, dtype, wide=True)
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


def test_robustness_at_33_rows(fa, oracle_mod):
    """33 rows: three 16-row workspace slots, and a fourth wave that has none"""
    import torch

    dtype, P, Hq, Nq = "bf16", 16, 11, 3
    rng = np.random.default_rng(2617)
    lens = [0, 1, 2, 40, 300, 1000]  # L = 0, and causal with Nq = 3: L = 1 leaves tokens 0 and 1 dead, L = 2 token 0
    B = len(lens)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (B, Hq, Nq, DQK)).astype(np.float32), dtype)
    pool, table, kvs = mla.make_pool(oracle_mod, rng, P, lens, dtype, max_pages=80)  # (NaN in the slots >= L_b and in the spare pages)
    full, view = _pool_view(pool, dtype, P)
    qd, td, ld = _dev(q, dtype), _i32(table), _i32(lens)
    call = lambda *a, **kw: fa.flash_attention_mla_decode_paged(*a, is_causal=True, wide=True, **kw)  # noqa: E731
    need = fa.mla_decode_paged_wide_workspace_bytes(B, Hq, Nq, DV, P, 80)
    assert need % (3 * 16 * 514 * 4) == 0
    # a NaN-filled workspace with a canary behind it (where a fourth slot would begin); two runs bit-equal
    buf = torch.full((need + 16 * 514 * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    o1, l1 = call(qd, view, td, ld, SCALE, workspace=buf[:need])
    o2, l2 = call(qd, view, td, ld, SCALE)
    torch.cuda.synchronize()
    assert (buf[need:] == 0xFF).all() and _same_bits(o1, o2) and _same_bits(l1, l2)
    mla.check(oracle_mod, *_np(o1, l1), q, kvs, lens, True, dtype, "wide robustness")
    on, ln = _np(o1, l1)
    assert np.isneginf(ln[0]).all() and (on[0] == 0).all()
    assert np.isneginf(ln[1, :, :2]).all() and np.isfinite(ln[1, :, 2]).all() and np.isneginf(ln[2, :, 0]).all() and np.isfinite(ln[2, :, 1:]).all()
    # lse = None
    o3, l3 = call(qd, view, td, ld, SCALE, return_lse=False)
    torch.cuda.synchronize()
    assert l3 is None and _same_bits(o1, o3)
    # entries past ceil(L_b / P) have no influence
    t2 = table.copy()
    for b, L in enumerate(lens):
        t2[b, (L + P - 1) // P:] = rng.integers(-5, pool.shape[0] + 5, 80 - (L + P - 1) // P)
    o4, l4 = call(qd, view, _i32(t2), ld, SCALE)
    torch.cuda.synchronize()
    assert _same_bits(o1, o4) and _same_bits(l1, l4)
    # a table entry of -1 and one of num_pages: the bits of a pool whose page is zeros
    t3, zp = table.copy(), pool.copy()
    zp[table[4, 2]] = 0.0
    zp[table[5, 5]] = 0.0
    t3[4, 2], t3[5, 5] = -1, pool.shape[0]
    o5, l5 = call(qd, view, _i32(t3), ld, SCALE)
    o6, l6 = call(qd, _pool_view(zp, dtype, P)[1], td, ld, SCALE)
    torch.cuda.synchronize()
    assert _same_bits(o5, o6) and _same_bits(l5, l6) and not _same_bits(o5, o1)
    # o under wide strides inside a sentinel buffer: only the 512 columns of the 33 real rows change (asserted in run)
    o7, l7 = run(fa, q, view, table, lens, True, dtype, wide_o=True, wide=True)
    assert _same_bits(o7, o1) and _same_bits(l7, l1)
    assert full.shape[0] == pool.shape[0]


def test_graph_replay_after_everything_changed_in_place(fa, oracle_mod):
    import torch

    dtype, P, Hq, Nq, mp = "bf16", 64, 16, 3, 16
    rng = np.random.default_rng(2623)
    lens_a, lens_b = [100, 1000, 64], [700, 3, 129]
    pool_a, table_a, kvs_a = mla.make_pool(oracle_mod, rng, P, lens_a, dtype, max_pages=mp, spare=20)
    pool_b, table_b, kvs_b = mla.make_pool(oracle_mod, rng, P, lens_b, dtype, max_pages=mp,
                                           spare=20 + sum((a + P - 1) // P for a in lens_a) - sum((b + P - 1) // P for b in lens_b))
    assert pool_a.shape == pool_b.shape
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (3, Hq, Nq, DQK)).astype(np.float32), dtype)
    qd, pd, td, ld = _dev(q, dtype), _dev(pool_a, dtype), _i32(table_a), _i32(lens_a)
    out = torch.empty((3, Hq, Nq, DV), dtype=qd.dtype, device="cuda")
    lse = torch.empty((3, Hq, Nq), dtype=torch.float32, device="cuda")
    ws = torch.empty(fa.mla_decode_paged_wide_workspace_bytes(3, Hq, Nq, DV, P, mp), dtype=torch.uint8, device="cuda")
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
    mla.check(oracle_mod, *_np(out, lse), q, kvs_a, lens_a, True, dtype, "wide graph, first replay")
    pd.copy_(_dev(pool_b, dtype))
    td.copy_(_i32(table_b))
    ld.copy_(_i32(lens_b))
    g.replay()
    torch.cuda.synchronize()
    mla.check(oracle_mod, *_np(out, lse), q, kvs_b, lens_b, True, dtype, "wide graph, replay after the change")


def test_default_routing(fa, oracle_mod):
    """wide=None: 48 rows go to the wide call (and succeed); 16 rows go where they went, bit for bit"""
    import torch

    dtype, P = "bf16", 64
    rng = np.random.default_rng(2629)
    lens = [200, 1, 777]
    pool, table, kvs = mla.make_pool(oracle_mod, rng, P, lens, dtype)
    view, td, ld = _pool_view(pool, dtype, P)[1], _i32(table), _i32(lens)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (3, 16, 3, DQK)).astype(np.float32), dtype)
    qd = _dev(q, dtype)
    o, lse = fa.flash_attention_mla_decode_paged(qd, view, td, ld, SCALE, is_causal=True)
    ow, lw = fa.flash_attention_mla_decode_paged(qd, view, td, ld, SCALE, is_causal=True, wide=True)
    torch.cuda.synchronize()
    assert _same_bits(o, ow) and _same_bits(lse, lw)
    mla.check(oracle_mod, *_np(o, lse), q, kvs, lens, True, dtype, "routing, 48 rows")
    with pytest.raises(fa.FaError, match="Hq \\* Nq <= 32"):
        fa.flash_attention_mla_decode_paged(qd, view, td, ld, SCALE, is_causal=True, wide=False)
    q16 = qd[:, :, :1]
    o, lse = fa.flash_attention_mla_decode_paged(q16, view, td, ld, SCALE)
    oo, lo = fa.flash_attention_mla_decode_paged(q16, view, td, ld, SCALE, wide=False)
    ow, lw = fa.flash_attention_mla_decode_paged(q16, view, td, ld, SCALE, wide=True)
    torch.cuda.synchronize()
    assert _same_bits(o, oo) and _same_bits(lse, lo)
    mla.check(oracle_mod, *_np(ow, lw), q[:, :, :1], kvs, lens, False, dtype, "wide=True at 16 rows")
