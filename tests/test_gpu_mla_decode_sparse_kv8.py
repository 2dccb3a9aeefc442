"""GPU: fa_fwd_mla_decode_sparse_kv8 (absorbed MLA decode over a list of slots per query token of an e4m3 latent pool; include/fa_mi355.h).
The contract is two bit-identities, so on every case O and LSE must be BIT-IDENTICAL to (1) fa_fwd_mla_decode_sparse (bf16) on the pool
widened element by element -- the same lists, counts, strides in elements and page size; 0x7F / 0xFF here is NaN there -- and to (2)
fa_fwd_mla_decode_paged_kv8 on the e4m3 pool of 64-row pages into which the listed rows were copied in list order; and inside
tests/mla.py's four bars against fp64 on the widened values (tests/test_mla_sparse_kv8_cases.py holds the reference to them on the
CPU). Then the split cases at topk = 2048, what nobody names has no influence, exact answers over all 254 finite codes, the chain
behind fa_kv_append_paged_quant on the aliased pool, a graph replayed after lists, counts and pool bytes changed in place, and the
Python routing.
Worst error / bar measured on an MI355X over the nine parity cases (printed by the tests): strict O 2.6e-3 / 6e-3; strict LSE 9.0e-7 / 1e-4;
O and LSE against the true Q 2.7e-3 / 6.5e-2 and 3.7e-3 / 3.1e-2; every case bit-identical to both twins; see README.md, round 31."""
import numpy as np
import pytest

import kv8
import mla
import mla_sparse
import mla_sparse_kv8 as msk
from test_gpu_mla_decode import _bits, _dev, _i32, _np, _same_bits, fa  # noqa: F401  (fa: the fixture)
from test_gpu_mla_decode_kv8 import _pool8, _pool16
from test_gpu_mla_decode_sparse import run

pytestmark = pytest.mark.gpu

DQK, DV, SCALE, DTYPE = mla.DQK, mla.DV, mla.SCALE, msk.DTYPE


def gathered_run(fa, c, seed):
    """identity 2: fa_fwd_mla_decode_paged_kv8(B = T, Nq = 1, P = 64, cap / 64 pages, not causal, seqlens_k = n) on the gathered e4m3 twin"""
    import torch

    codes, table, lens = msk.twin8(c, np.random.default_rng(seed))
    o, lse = fa.flash_attention_mla_decode_paged(_dev(mla_sparse.q4(c["q"]), DTYPE), _pool8(codes, 64)[1], _i32(table), _i32(lens), SCALE,
                                                 is_causal=False)
    torch.cuda.synchronize()
    return o[:, :, 0], lse[:, :, 0]


def both(fa, oracle_mod, c, what, **kw):
    """the call on c, held to the four bars and to the bits of both twins; returns (O, LSE, the four figures)"""
    P = c["P"]
    o, lse = run(fa, c["q"], _pool8(c["codes"], P)[1], c["indices"], c["counts"], DTYPE, topk=c["topk"], **kw)
    o1, l1 = run(fa, c["q"], _pool16(c["pool"], P), c["indices"], c["counts"], DTYPE, topk=c["topk"], **kw)
    o2, l2 = gathered_run(fa, c, 7)
    on, ln = _np(o, lse)
    e = mla.check(oracle_mod, on[:, :, None], ln[:, :, None], mla_sparse.q4(c["q"]), c["kvs"], c["lens"], False, DTYPE, what)
    assert _same_bits(o, o1) and _same_bits(lse, l1), ("differs from the sparse call on the widened pool", what)
    assert _same_bits(o, o2) and _same_bits(lse, l2), ("differs from the dense e4m3 call on the gathered pool", what)
    return o, lse, e


@pytest.mark.parametrize("idx", range(len(msk.CASES)))
def test_parity_against_fp64_and_the_bits_of_both_twins(fa, oracle_mod, idx):
    c = msk.case(idx)
    both(fa, oracle_mod, c, ("gpu sparse kv8", msk.CASES[idx]), padded_q=idx % 2 == 1, wide_o=idx % 3 == 1)


def _big(oracle_mod, rng, T, Hq, counts, topk=2048, P=64, nslots=8192, kind="perm", integer=False):
    indices = mla_sparse.make_lists(rng, T, topk, -(-topk // 4) * 4, nslots, kind)
    counts = None if counts is None else np.array(counts, np.int32)
    draw = (lambda *shape: rng.integers(-4, 5, shape).astype(np.float32)) if integer else None
    codes, twin = msk.make_pools(rng, P, nslots, indices, counts, topk, draw=draw)
    c = {"Hq": Hq, "topk": topk, "P": P, "dtype": DTYPE, "T": T, "kind": kind, "codes": codes, "pool": twin, "indices": indices, "counts": counts,
         "q": oracle_mod.round_to(rng.uniform(-1.0, 1.0, (T, Hq, DQK)).astype(np.float32), DTYPE)}
    c["kvs"], c["lens"] = mla_sparse.gather(c)
    return c


@pytest.mark.parametrize("T,Hq,counts", [(1, 16, None), (3, 128, None), (3, 16, [65, 2048, 1000])])
def test_split_cases(fa, oracle_mod, T, Hq, counts):
    """topk = 2048 on a pool of 8192 slots: 32 tiles in eight splits of four; with a count of 65 all splits but two are empty -- their
    workgroups meet no barrier, stage nothing and write (0, -inf, 0)"""
    assert fa.mla_decode_sparse_kv8_workspace_bytes(T, Hq, DV, 2048) == T * 8 * -(-Hq // 16) * 16 * 514 * 4  # S = 8
    c = _big(oracle_mod, np.random.default_rng(3150 + T + Hq), T, Hq, counts)
    both(fa, oracle_mod, c, ("sparse kv8 splits", T, Hq, counts))


def test_what_nobody_names_has_no_influence(fa, oracle_mod):
    """arbitrary values behind the count, other bytes -- finite codes, the two NaN codes exchanged -- in every slot no list names, a
    NaN-filled workspace with a canary behind it, lse = None, a second run: the same bits"""
    import torch

    c = msk.case(3)  # 33 heads, topk = 65 at a pitch of 72, counts 0 .. 65, P = 16, rows of 640 bytes
    T, Hq, topk, P = c["T"], c["Hq"], c["topk"], c["P"]
    view = _pool8(c["codes"], P)[1]
    o1, l1 = run(fa, c["q"], view, c["indices"], c["counts"], DTYPE, topk=topk)
    o1b, l1b = run(fa, c["q"], view, c["indices"], c["counts"], DTYPE, topk=topk)
    assert _same_bits(o1, o1b) and _same_bits(l1, l1b)  # two runs alike
    # (a) entries behind n_t: negative, huge, outside the pool
    idx = c["indices"].copy()
    rng = np.random.default_rng(3251)
    for t in range(T):
        n = c["lens"][t]
        idx[t, n:] = rng.choice(np.array([-1, -(2 ** 31), 2 ** 31 - 1, 2 ** 30, P * view.shape[0], 12345678], np.int64), idx.shape[1] - n).astype(np.int32)
    o2, l2 = run(fa, c["q"], view, idx, c["counts"], DTYPE, topk=topk)
    assert _same_bits(o1, o2) and _same_bits(l1, l2)
    # (b) every byte that no counted entry names: 0x7F / 0xFF as the case holds them, then exchanged, then random finite codes
    unread = np.isin(c["codes"], kv8.NAN_CODES)
    assert unread[:, :P, :DQK].any() and unread[:, :, DQK:].all()
    for other in (np.where(unread, c["codes"] ^ 0x80, c["codes"]), np.where(unread, rng.choice(kv8.FINITE_CODES, c["codes"].shape), c["codes"])):
        assert (other != c["codes"])[unread].all() and np.array_equal(other[~unread], c["codes"][~unread])
        o3, l3 = run(fa, c["q"], _pool8(other.astype(np.uint8), P)[1], idx, c["counts"], DTYPE, topk=topk)
        assert _same_bits(o1, o3) and _same_bits(l1, l3) and torch.isfinite(o3).all()
    # (c) the workspace: NaN-filled, a canary behind it (three 16-row slots per item: the fourth wave has none); lse = None
    need = fa.mla_decode_sparse_kv8_workspace_bytes(T, Hq, DV, topk)
    assert need % (3 * 16 * 514 * 4) == 0
    buf = torch.full((need + 16 * 514 * 4,), 0xFF, dtype=torch.uint8, device="cuda")
    o4, l4 = run(fa, c["q"], view, c["indices"], c["counts"], DTYPE, topk=topk, workspace=buf[:need], return_lse=False)
    assert l4 is None and _same_bits(o1, o4) and (buf[need:] == 0xFF).all()
    # (d) the token with no entry: O = 0 exactly, LSE = -inf
    dead = c["lens"].index(0)
    assert (o1[dead] == 0).all() and torch.isneginf(l1[dead]).all()
    live = [t for t in range(T) if c["lens"][t] > 0]
    assert torch.isfinite(l1[live]).all() and torch.isfinite(o1).all()


@pytest.mark.parametrize("Hq", [1, 128])
def test_one_listed_key_returns_its_widened_row_over_all_finite_codes(fa, oracle_mod, Hq):
    """n_t = 1: O is the key's first 512 values, bit for bit. Eight tokens whose rows together hold each of the 254 finite codes
    (subnormals and both zeros included), in rows of 640 bytes with a padding row per page -- at one split (topk = 1) and at eight (2048)"""
    P, T, nslots = 16, 8, 1024
    rng = np.random.default_rng(3311 + Hq)
    rows = np.resize(kv8.FINITE_CODES, T * DQK)
    rng.shuffle(rows)
    rows = rows.reshape(T, DQK)
    assert set(rows[:, :DV].reshape(-1).tolist()) == set(kv8.FINITE_CODES.tolist())
    codes = np.full((nslots // P, P + 1, 640), 0x7F, np.uint8)
    slots = rng.permutation(nslots)[:T]
    for t, x in enumerate(slots):
        codes[x // P, x % P, :DQK] = rows[t]
    twin = kv8.widen(codes)
    for topk in (1, 2048):
        idx = mla_sparse.make_lists(rng, T, topk, -(-topk // 4) * 4, nslots, "perm")
        idx[:, 0] = slots
        q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (T, Hq, DQK)).astype(np.float32), DTYPE)
        ones = np.ones(T, np.int32)
        o, lse = run(fa, q, _pool8(codes, P)[1], idx, ones, DTYPE, topk=topk)
        o16, l16 = run(fa, q, _pool16(twin, P), idx, ones, DTYPE, topk=topk)
        assert _same_bits(o, o16) and _same_bits(lse, l16), (Hq, topk)
        for t in range(T):
            want = _bits(_dev(np.broadcast_to(kv8.widen(rows[t, :DV]), (Hq, DV)), DTYPE))
            # bit for bit, but for the code 0x80: the accumulator starts at +0 and +0 + (-0 * 1) = +0 in the matrix core, in this call as in
            # both twins (tests/test_gpu_mla_decode_kv8.py; a conversion that turned -0 into anything but a zero still shows)
            minus0 = want == np.int16(-32768)
            assert np.array_equal(np.where(minus0, 0, want), _bits(o[t])), (Hq, topk, t)
    assert (rows[:, :DV] == 0x80).any()


def test_zero_query_gives_the_exact_mean_and_the_log_of_the_count(fa, oracle_mod):
    rng = np.random.default_rng(3313)
    Hq, topk, counts = 16, 200, [1, 37, 64, 200]
    c = _big(oracle_mod, rng, 4, Hq, counts, topk=topk, P=16, nslots=1024, integer=True)
    idx = c["indices"].copy()
    idx[3, :topk] = rng.choice(idx[3, :5], topk)  # a list of five slots named 200 times (named already: the pool stays what it is)
    c["indices"] = idx
    c["kvs"], c["lens"] = mla_sparse.gather(c)
    o, lse = run(fa, np.zeros((4, Hq, DQK), np.float32), _pool8(c["codes"], 16)[1], idx, c["counts"], DTYPE, topk=topk)
    on, ln = _np(o, lse)
    for t, n in enumerate(counts):
        assert np.abs(ln[t] - np.log(n)).max() < 1e-6 * max(1.0, np.log(n)) + 1e-6, (t, n)
        rounded = _dev(c["kvs"][t][:, :DV].astype(np.float64).mean(0).astype(np.float32), DTYPE).float().cpu().numpy()
        # exact sums, probabilities all 1: what is left is sum * (1 / n) in fp32 and one rounding to bf16 (tests/test_gpu_mla_decode_sparse.py)
        assert (np.abs(on[t] - rounded[None]) <= np.abs(rounded)[None] * 2.0 ** -7 + 1e-30).all(), (t, n)


@pytest.mark.parametrize("new_dtype", ["f16", "bf16"])
def test_chain_behind_the_quantising_append_on_the_aliased_pool(fa, oracle_mod, new_dtype):
    """fa_kv_append_paged_quant with Hkv = 1, D = 576, k_pages == v_pages, k_new == v_new, k_mul = v_mul = 0.5 into a 0x7F-filled pool, then
    the sparse call over the SLOTS of the rows just written, in shuffled order: bit for bit the call on a pool written on the host"""
    import torch

    from util import TORCH_DTYPE

    P, Hq, mp = 16, 16, 8
    rng = np.random.default_rng(3319)
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
    rows = torch.from_numpy(rng.uniform(-2.5, 2.5, (total, 1, DQK)).astype(np.float32)).to(getattr(torch, TORCH_DTYPE[new_dtype]))
    want_codes = kv8.quant_reference(rows, 0.5)  # [total, 1, 576]
    pool = torch.full((num_pages, P, 1, DQK), 0x7F, dtype=torch.uint8, device="cuda")
    p8 = pool.view(kv8.E4M3)
    cu = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    rd = rows.cuda()
    fa.kv_append_paged(rd, rd, p8, p8, _i32(cu), _i32(table), _i32(after), max(new), layout="NHD", k_mul=0.5, v_mul=0.5)
    torch.cuda.synchronize()
    host = np.full((num_pages, P, DQK), 0x7F, np.uint8)
    topk = 40
    idx = np.full((B, topk), -7, np.int32)
    kvs = []
    for b in range(B):
        order = rng.permutation(new[b])
        pos = before[b] + order
        idx[b, :new[b]] = table[b, pos // P] * P + pos % P
        for i in range(new[b]):
            host[table[b, (before[b] + i) // P], (before[b] + i) % P] = want_codes[cu[b] + i, 0]
        kvs.append(kv8.widen(want_codes[cu[b]:cu[b + 1], 0][order]))
    assert np.array_equal(pool.cpu().numpy()[:, :, 0], host), "the appended bytes"
    q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (B, Hq, DQK)).astype(np.float32), DTYPE)
    oa, la = run(fa, q, p8[:, :, 0], idx, np.array(new, np.int32), DTYPE)
    ob, lb = run(fa, q, _pool8(host, P)[1], idx, np.array(new, np.int32), DTYPE)
    assert _same_bits(oa, ob) and _same_bits(la, lb)
    on, ln = _np(oa, la)
    mla.check(oracle_mod, on[:, :, None], ln[:, :, None], mla_sparse.q4(q), kvs, new, False, DTYPE, ("sparse kv8 chain", new_dtype))


def test_graph_replay_after_lists_counts_and_pool_bytes_changed_in_place(fa, oracle_mod):
    import torch

    rng = np.random.default_rng(3401)
    a = _big(oracle_mod, rng, 3, 16, [100, 320, 64], topk=320, nslots=2048)
    b = _big(oracle_mod, rng, 3, 16, [320, 3, 129], topk=320, nslots=2048)
    b["q"] = a["q"]
    qd, idx, cnt = _dev(a["q"], DTYPE), _i32(a["indices"]), _i32(a["counts"])
    raw = torch.from_numpy(a["codes"].copy()).cuda()
    pd = raw.view(kv8.E4M3)
    out = torch.empty((3, 16, DV), dtype=qd.dtype, device="cuda")
    lse = torch.empty((3, 16), dtype=torch.float32, device="cuda")
    ws = torch.empty(fa.mla_decode_sparse_kv8_workspace_bytes(3, 16, DV, 320), dtype=torch.uint8, device="cuda")
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
    mla.check(oracle_mod, on[:, :, None], ln[:, :, None], mla_sparse.q4(a["q"]), a["kvs"], a["lens"], False, DTYPE, "sparse kv8 graph, first replay")
    raw.copy_(torch.from_numpy(b["codes"].copy()))
    idx.copy_(_i32(b["indices"]))
    cnt.copy_(_i32(b["counts"]))
    g.replay()
    torch.cuda.synchronize()
    on, ln = _np(out, lse)
    mla.check(oracle_mod, on[:, :, None], ln[:, :, None], mla_sparse.q4(b["q"]), b["kvs"], b["lens"], False, DTYPE,
              "sparse kv8 graph, replay after the change")


def test_python_routing(fa, oracle_mod):
    """an e4m3 pool under bf16 q goes to the new call; f16 q on it is refused before the library; the bf16 route is where it was"""
    import torch

    c = msk.case(1)
    P = c["P"]
    v8, v16 = _pool8(c["codes"], P)[1], _pool16(c["pool"], P)
    qd, idx, cnt = _dev(c["q"], DTYPE), _i32(c["indices"]), _i32(c["counts"])
    o, lse = fa.flash_attention_mla_decode_sparse(qd, v8, idx[:, :c["topk"]], SCALE, index_counts=cnt)
    o4, l4 = fa.flash_attention_mla_decode_sparse(qd, v8[:, :, None], idx[:, :c["topk"]], SCALE, index_counts=cnt)  # [num_pages, P, 1, 576]
    ow, lw = fa.flash_attention_mla_decode_sparse(qd, v16, idx[:, :c["topk"]], SCALE, index_counts=cnt)
    torch.cuda.synchronize()
    assert o.dtype == torch.bfloat16 and _same_bits(o, ow) and _same_bits(lse, lw) and _same_bits(o, o4) and _same_bits(lse, l4)
    with pytest.raises(ValueError, match="bf16 queries only"):
        fa.flash_attention_mla_decode_sparse(qd.to(torch.float16), v8, idx, SCALE)
    with pytest.raises(ValueError, match="needs the model's scale"):
        fa.flash_attention_mla_decode_sparse(qd, v8, idx, None)
    with pytest.raises(ValueError, match="no CPU path"):
        fa.flash_attention_mla_decode_sparse(qd, v8, idx.cpu(), SCALE)
    with pytest.raises(ValueError, match="int32 \\[T, topk\\]"):
        fa.flash_attention_mla_decode_sparse(qd, v8, idx.long(), SCALE)
    with pytest.raises(ValueError, match="index_counts"):
        fa.flash_attention_mla_decode_sparse(qd, v8, idx, SCALE, index_counts=torch.zeros(c["T"] + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(fa.FaError, match="fa_fwd_mla_decode_sparse_kv8: indices_stride=63 must be a multiple of 4"):
        fa.flash_attention_mla_decode_sparse(qd, v8, idx[:, :63].contiguous(), SCALE)
    with pytest.raises(fa.FaError, match="fa_fwd_mla_decode_sparse_kv8: .*Hq <= 128 heads"):
        fa.flash_attention_mla_decode_sparse(torch.zeros((1, 129, DQK), dtype=qd.dtype, device="cuda"), v8, idx[:1], SCALE)
    assert fa.mla_decode_sparse_kv8_supported("bf16", "fp8_e4m3", DQK, DV, c["Hq"], P)
    assert not fa.mla_decode_sparse_kv8_supported("f16", "fp8_e4m3", DQK, DV, c["Hq"], P)
