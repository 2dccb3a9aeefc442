"""GPU: fa_fwd_mla_decode_paged_kv8 (absorbed MLA decode, bf16 queries on an e4m3 latent pool, four waves that stage every tile through
registers and widen it into the wide call's image; include/fa_mi355.h). The contract is the wide call on the exactly widened pool, so on
every case O and LSE must be BIT-IDENTICAL to fa_fwd_mla_decode_paged_wide (bf16) on the twin pool of tests/mla_kv8.py -- the same page
order, strides in elements and unreadable slots (0x7F / 0xFF here, NaN there) -- and inside tests/mla.py's four bars against fp64 on the
widened values (tests/test_mla_kv8_cases.py holds the reference to them on the CPU). Then exact answers over all 254 finite codes, many
splits with most of them empty, robustness against what the pool, the tables and the workspace hold where nobody may look, the chain
behind fa_kv_append_paged_quant on the aliased pool, a graph replayed after everything changed in place, and the Python routing.
Worst error / bar measured on an MI355X over the 30 parity cases (printed by the tests): strict O 2.6e-3 / 6e-3; strict LSE 1.4e-6 / 1e-4;
O and LSE against the true Q 2.7e-3 / 6.7e-2 and 3.2e-3 / 3.1e-2; see README.md, round 27."""
import numpy as np
import pytest

import kv8
import mla
import mla_kv8
from test_gpu_mla_decode import _bits, _dev, _i32, _np, _same_bits, fa, run  # noqa: F401  (fa: the fixture)

pytestmark = pytest.mark.gpu

DQK, DV, SCALE, DTYPE = mla.DQK, mla.DV, mla.SCALE, mla_kv8.DTYPE


def _pool8(codes, P):
    """the device pool of bytes with its padding rows and columns, and the [num_pages, P, 576] e4m3 view the call takes"""
    import torch

    full = torch.from_numpy(np.array(codes, copy=True)).cuda()
    return full, full.view(kv8.E4M3)[:, :P, :DQK]


def _pool16(twin, P):
    return _dev(twin, DTYPE)[:, :P, :DQK]


def both(fa, q, codes, twin, table, lens, causal, P, token_major=False, wide_o=False, **kw):
    """(O, LSE) of the e4m3 call and of the wide call on the twin, asserted bit-identical in every element"""
    o8, l8 = run(fa, q, _pool8(codes, P)[1], table, lens, causal, DTYPE, token_major, wide_o, **kw)
    o16, l16 = run(fa, q, _pool16(twin, P), table, lens, causal, DTYPE, token_major, wide_o, wide=True, **kw)
    assert _same_bits(o8, o16), "O differs from the wide call on the widened pool"
    assert (l8 is None and l16 is None) or _same_bits(l8, l16), "LSE differs from the wide call on the widened pool"
    return o8, l8


@pytest.mark.parametrize("P", mla_kv8.PAGES)
@pytest.mark.parametrize("idx", range(len(mla_kv8.SHAPES)))
def test_bits_of_the_wide_call_and_parity_against_fp64(fa, oracle_mod, idx, P):
    c = mla_kv8.case(P, idx)
    o, lse = both(fa, c["q"], c["codes"], c["twin"], c["table"], c["lens"], c["causal"], P, c["token_major"], c["wide_o"])
    mla.check(oracle_mod, *_np(o, lse), c["q"], c["kvs"], c["lens"], c["causal"], DTYPE, ("gpu kv8", mla_kv8.SHAPES[idx], P))


@pytest.mark.parametrize("Hq", [1, 128])
def test_one_visible_key_returns_its_widened_row_over_all_finite_codes(fa, oracle_mod, Hq):
    """L_b = 1: O is the key's first 512 values, bit for bit. Eight sequences whose rows together hold each of the 254 finite codes
    (subnormals and both zeros included) -- at one split and at many"""
    P, B = 16, 8
    rng = np.random.default_rng(2711 + Hq)
    rows = np.resize(kv8.FINITE_CODES, B * DQK)
    rng.shuffle(rows)
    rows = rows.reshape(B, DQK)
    assert set(rows[:, :DV].reshape(-1).tolist()) == set(kv8.FINITE_CODES.tolist())
    vals = kv8.widen(rows)
    for max_pages in (1, 4096):
        it = iter(range(B))
        codes, twin, table, kvs = mla_kv8.make_twins(rng, P, [1] * B, max_pages=max_pages, draw=lambda L: vals[next(it)][None])
        q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (B, Hq, 1, DQK)).astype(np.float32), DTYPE)
        o, lse = both(fa, q, codes, twin, table, [1] * B, True, P)
        for b in range(B):
            want = _bits(_dev(np.broadcast_to(kvs[b][0, :DV], (Hq, DV)), DTYPE))
            got = _bits(o[b, :, 0])
            # bit for bit, but for the code 0x80: the accumulator starts at +0 and +0 + (-0 * 1) = +0 in the matrix core, in this call as in
            # the wide call on a pool that holds -0 (a conversion that turned -0 into anything but a zero still shows)
            minus0 = want == np.int16(-32768)
            assert np.array_equal(np.where(minus0, 0, want), got), (Hq, max_pages, b)
        assert any((_bits(_dev(kv[0, :DV], DTYPE)) == np.int16(-32768)).any() for kv in kvs)


def test_zero_query_gives_the_exact_mean_and_the_log_of_the_count(fa, oracle_mod):
    P, Hq, Nq = 16, 16, 3
    rng = np.random.default_rng(2713)
    lens = [1, 37, 64, 200]
    codes, twin, table, kvs = mla_kv8.make_twins(rng, P, lens, integer=True)
    o, lse = both(fa, np.zeros((4, Hq, Nq, DQK), np.float32), codes, twin, table, lens, False, P)
    on, ln = _np(o, lse)
    for b, L in enumerate(lens):
        assert np.abs(ln[b] - np.log(L)).max() < 1e-6 * max(1.0, np.log(L)) + 1e-6, (b, L)
        rounded = _dev(kvs[b][:, :DV].astype(np.float64).mean(0).astype(np.float32), DTYPE).float().cpu().numpy()
        # exact sums, probabilities all 1: what is left is sum * (1 / L) in fp32 and one rounding to bf16 (tests/test_gpu_mla_decode_wide.py)
        assert (np.abs(on[b] - rounded[None, None]) <= np.abs(rounded)[None, None] * 2.0 ** -7 + 1e-30).all(), (b, L)


@pytest.mark.parametrize("L", [16384, 100])
def test_many_splits_on_one_sequence(fa, oracle_mod, L):
    """B = 1 at a capacity of 65536 keys, one block of 64 rows: 256 splits; with 100 keys all but two are empty"""
    P = 64
    rng = np.random.default_rng(2707 + L)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (1, 16, 4, DQK)).astype(np.float32), DTYPE)
    codes, twin, table, kvs = mla_kv8.make_twins(rng, P, [L], max_pages=65536 // P)
    assert fa.mla_decode_paged_kv8_workspace_bytes(1, 16, 4, DV, P, 65536 // P) == 256 * 64 * 514 * 4  # S = 256
    o, lse = both(fa, q, codes, twin, table, [L], True, P)
    mla.check(oracle_mod, *_np(o, lse), q, kvs, [L], True, DTYPE, ("kv8 splits", L))


def test_robustness_at_33_rows(fa, oracle_mod):
    """33 rows: three 16-row workspace slots, and a fourth wave that has none"""
    import torch

    P, Hq, Nq = 16, 11, 3
    rng = np.random.default_rng(2717)
    lens = [0, 1, 2, 40, 300, 1000]
    B = len(lens)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (B, Hq, Nq, DQK)).astype(np.float32), DTYPE)
    codes, twin, table, kvs = mla_kv8.make_twins(rng, P, lens, max_pages=80)
    view = _pool8(codes, P)[1]
    qd, td, ld = _dev(q, DTYPE), _i32(table), _i32(lens)
    call = lambda *a, **kw: fa.flash_attention_mla_decode_paged(*a, is_causal=True, **kw)  # noqa: E731
    need = fa.mla_decode_paged_kv8_workspace_bytes(B, Hq, Nq, DV, P, 80)
    assert need % (3 * 16 * 514 * 4) == 0 and need == fa.mla_decode_paged_wide_workspace_bytes(B, Hq, Nq, DV, P, 80)
    # a NaN-filled workspace with a canary behind it (where a fourth slot would begin); two runs bit-equal
    buf = torch.full((need + 16 * 514 * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    o1, l1 = call(qd, view, td, ld, SCALE, workspace=buf[:need])
    o2, l2 = call(qd, view, td, ld, SCALE)
    torch.cuda.synchronize()
    assert (buf[need:] == 0xFF).all() and _same_bits(o1, o2) and _same_bits(l1, l2)
    mla.check(oracle_mod, *_np(o1, l1), q, kvs, lens, True, DTYPE, "kv8 robustness")
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
        t2[b, (L + P - 1) // P:] = rng.integers(-5, codes.shape[0] + 5, 80 - (L + P - 1) // P)
    o4, l4 = call(qd, view, _i32(t2), ld, SCALE)
    torch.cuda.synchronize()
    assert _same_bits(o1, o4) and _same_bits(l1, l4)
    # a table entry of -1 and one of num_pages: the bits of a pool whose page is zeros
    t3, zc = table.copy(), codes.copy()
    zc[table[4, 2]] = 0
    zc[table[5, 5]] = 0
    t3[4, 2], t3[5, 5] = -1, codes.shape[0]
    o5, l5 = call(qd, view, _i32(t3), ld, SCALE)
    o6, l6 = call(qd, _pool8(zc, P)[1], td, ld, SCALE)
    torch.cuda.synchronize()
    assert _same_bits(o5, o6) and _same_bits(l5, l6) and not _same_bits(o5, o1)
    # o under wide strides inside a sentinel buffer: only the 512 columns of the 33 real rows change (asserted in run)
    o7, l7 = run(fa, q, view, table, lens, True, DTYPE, wide_o=True)
    assert _same_bits(o7, o1) and _same_bits(l7, l1)


@pytest.mark.parametrize("new_dtype", ["f16", "bf16"])
def test_chain_behind_the_quantising_append_on_the_aliased_pool(fa, oracle_mod, new_dtype):
    """fa_kv_append_paged_quant with Hkv = 1, D = 576, k_pages == v_pages, k_new == v_new, k_mul = v_mul = 0.5 into a 0x7F-filled pool: the
    bytes are kv8.quant_reference's, and the decode on them is, bit for bit, the decode on a pool written on the host"""
    import torch

    from util import TORCH_DTYPE

    P, Hq, Nq, mp = 16, 16, 2, 8
    rng = np.random.default_rng(2719)
    before, new = [0, 17, 100], [1, 40, 21]
    after = [a + n for a, n in zip(before, new)]
    B, total = len(new), sum(new)
    num_pages = sum(-(-a // P) for a in after) + 2
    table = np.full((B, mp), num_pages - 1, np.int32)
    perm, used = rng.permutation(num_pages - 1), 0
    for b, a in enumerate(after):
        n = -(-a // P)
        table[b, :n] = perm[used:used + n]
        used += n
    tdt = getattr(torch, TORCH_DTYPE[new_dtype])
    rows = torch.from_numpy(rng.uniform(-2.5, 2.5, (total, 1, DQK)).astype(np.float32)).to(tdt)
    want_codes = kv8.quant_reference(rows, 0.5)  # [total, 1, 576]
    pool = torch.full((num_pages, P, 1, DQK), 0x7F, dtype=torch.uint8, device="cuda")
    p8 = pool.view(kv8.E4M3)
    cu = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    rd = rows.cuda()
    fa.kv_append_paged(rd, rd, p8, p8, _i32(cu), _i32(table), _i32(after), max(new), layout="NHD", k_mul=0.5, v_mul=0.5)
    torch.cuda.synchronize()
    host = np.full((num_pages, P, 1, DQK), 0x7F, np.uint8)
    for b in range(B):
        for i in range(new[b]):
            pos = before[b] + i
            host[table[b, pos // P], pos % P, 0] = want_codes[cu[b] + i, 0]
    assert np.array_equal(pool.cpu().numpy(), host), "the appended bytes"
    # the decode sees only the appended keys of each sequence where the rest is NaN: give every sequence its new rows alone
    lens = new
    t2 = np.full((B, mp), num_pages - 1, np.int32)
    pool2 = np.full((num_pages, P, DQK), 0x7F, np.uint8)
    kvs = []
    used = 0
    for b in range(B):
        codes_b = want_codes[cu[b]:cu[b + 1], 0]
        n = -(-new[b] // P)
        t2[b, :n] = perm[used:used + n]
        for j in range(n):
            pool2[perm[used + j], :min(P, new[b] - j * P)] = codes_b[j * P:(j + 1) * P]
        used += n
        kvs.append(kv8.widen(codes_b))
    # the same rows appended by the library into a second 0x7F-filled pool at positions 0 .. n_b - 1
    pool3 = torch.full((num_pages, P, 1, DQK), 0x7F, dtype=torch.uint8, device="cuda")
    fa.kv_append_paged(rd, rd, pool3.view(kv8.E4M3), pool3.view(kv8.E4M3), _i32(cu), _i32(t2), _i32(lens), max(new), layout="NHD", k_mul=0.5, v_mul=0.5)
    torch.cuda.synchronize()
    assert np.array_equal(pool3.cpu().numpy()[:, :, 0], pool2)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (B, Hq, Nq, DQK)).astype(np.float32), DTYPE)
    qd = _dev(q, DTYPE)
    oa, la = fa.flash_attention_mla_decode_paged(qd, pool3.view(kv8.E4M3), _i32(t2), _i32(lens), SCALE, is_causal=True)
    ob, lb = fa.flash_attention_mla_decode_paged(qd, torch.from_numpy(pool2).cuda().view(kv8.E4M3), _i32(t2), _i32(lens), SCALE, is_causal=True)
    torch.cuda.synchronize()
    assert _same_bits(oa, ob) and _same_bits(la, lb)
    mla.check(oracle_mod, *_np(oa, la), q, kvs, lens, True, DTYPE, ("kv8 chain", new_dtype))


def test_graph_replay_after_everything_changed_in_place(fa, oracle_mod):
    import torch

    P, Hq, Nq, mp = 64, 16, 3, 16
    rng = np.random.default_rng(2723)
    lens_a, lens_b = [100, 1000, 64], [700, 3, 129]
    codes_a, _, table_a, kvs_a = mla_kv8.make_twins(rng, P, lens_a, max_pages=mp, spare=20)
    codes_b, _, table_b, kvs_b = mla_kv8.make_twins(rng, P, lens_b, max_pages=mp,
                                                    spare=20 + sum((a + P - 1) // P for a in lens_a) - sum((b + P - 1) // P for b in lens_b))
    assert codes_a.shape == codes_b.shape
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (3, Hq, Nq, DQK)).astype(np.float32), DTYPE)
    qd, td, ld = _dev(q, DTYPE), _i32(table_a), _i32(lens_a)
    raw = torch.from_numpy(codes_a.copy()).cuda()
    pd = raw.view(kv8.E4M3)
    out = torch.empty((3, Hq, Nq, DV), dtype=qd.dtype, device="cuda")
    lse = torch.empty((3, Hq, Nq), dtype=torch.float32, device="cuda")
    ws = torch.empty(fa.mla_decode_paged_kv8_workspace_bytes(3, Hq, Nq, DV, P, mp), dtype=torch.uint8, device="cuda")
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
    mla.check(oracle_mod, *_np(out, lse), q, kvs_a, lens_a, True, DTYPE, "kv8 graph, first replay")
    raw.copy_(torch.from_numpy(codes_b.copy()))
    td.copy_(_i32(table_b))
    ld.copy_(_i32(lens_b))
    g.replay()
    torch.cuda.synchronize()
    mla.check(oracle_mod, *_np(out, lse), q, kvs_b, lens_b, True, DTYPE, "kv8 graph, replay after the change")


def test_python_routing(fa, oracle_mod):
    """an e4m3 pool under bf16 q goes to the new call for 16 and for 48 rows, whatever `wide` says but False; the bf16 routes are where they were"""
    import torch

    P = 64
    rng = np.random.default_rng(2729)
    lens = [200, 1, 777]
    codes, twin, table, kvs = mla_kv8.make_twins(rng, P, lens)
    v8, v16, td, ld = _pool8(codes, P)[1], _pool16(twin, P), _i32(table), _i32(lens)
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (3, 16, 3, DQK)).astype(np.float32), DTYPE)
    for qd in (_dev(q, DTYPE), _dev(q, DTYPE)[:, :, :1]):
        o, lse = fa.flash_attention_mla_decode_paged(qd, v8, td, ld, SCALE, is_causal=True)
        ot, lt = fa.flash_attention_mla_decode_paged(qd, v8, td, ld, SCALE, is_causal=True, wide=True)
        ow, lw = fa.flash_attention_mla_decode_paged(qd, v16, td, ld, SCALE, is_causal=True, wide=True)
        torch.cuda.synchronize()
        assert o.dtype == torch.bfloat16 and _same_bits(o, ot) and _same_bits(lse, lt) and _same_bits(o, ow) and _same_bits(lse, lw)
        with pytest.raises(ValueError, match="wide=False"):
            fa.flash_attention_mla_decode_paged(qd, v8, td, ld, SCALE, wide=False)
        with pytest.raises(ValueError, match="bf16 queries only"):
            fa.flash_attention_mla_decode_paged(qd.to(torch.float16), v8, td, ld, SCALE)
    mla.check(oracle_mod, *_np(o, lse), q[:, :, :1], kvs, lens, True, DTYPE, "kv8 routing, 16 rows")
    # the raw call refuses every other pair
    assert fa.mla_decode_paged_kv8_supported("bf16", "fp8_e4m3", DQK, DV, 16, 3, P)
    assert not fa.mla_decode_paged_kv8_supported("f16", "fp8_e4m3", DQK, DV, 16, 3, P)
