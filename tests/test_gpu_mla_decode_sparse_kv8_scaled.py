"""GPU: fa_fwd_mla_decode_sparse_kv8_scaled (absorbed MLA decode over a list of slots per token of a pool of 656-byte rows: e4m3 latent,
a fp32 scale per 128 latent elements, bf16 rotary) and fa_mla_kv_append_paged_scaled, the append that writes those rows
(include/fa_mi355.h). On every case O and LSE must be BIT-IDENTICAL to fa_fwd_mla_decode_sparse (bf16) on the twin pool dequantised by
the stated rule, and inside tests/mla.py's four bars against fp64 on the twin's values. The append must write the bytes of the numpy
reference, scales included, and nothing else."""
import numpy as np
import pytest

import mla
import mla_sparse
import mla_sparse_kv8_scaled as mss
from test_gpu_mla_decode import _dev, _i32, _np, _same_bits, fa  # noqa: F401  (fa: the fixture)
from test_gpu_mla_decode_sparse import run

pytestmark = pytest.mark.gpu

DQK, DV, SCALE, DTYPE, ROW = mla.DQK, mla.DV, mla.SCALE, mss.DTYPE, mss.ROW


def _view(pool, P):
    """the device pool of bytes with its padding rows and columns, as the [num_pages, P, 656] uint8 view the call takes"""
    import torch

    return torch.from_numpy(np.array(pool, copy=True)).cuda()[:, :P, :ROW]


def both(fa, oracle_mod, c, what, pool=None, **kw):
    """the call on c's pool of bytes (or `pool`), held to the bits of the sparse call on the dequantised twin and to the four bars"""
    P = c["P"]
    o, lse = run(fa, c["q"], _view(c["bytes"] if pool is None else pool, P), c["indices"], c["counts"], DTYPE, topk=c["topk"], **kw)
    o1, l1 = run(fa, c["q"], _dev(c["pool"], DTYPE), c["indices"], c["counts"], DTYPE, topk=c["topk"])
    assert _same_bits(o, o1) and (lse is None or _same_bits(lse, l1)), ("differs from the sparse call on the dequantised pool", what)
    on, ln = _np(o, l1)
    mla.check(oracle_mod, on[:, :, None], ln[:, :, None], mla_sparse.q4(c["q"]), c["kvs"], c["lens"], False, DTYPE, what)
    return o, lse


@pytest.mark.parametrize("idx", range(len(mss.CASES)))
def test_bits_of_the_sparse_call_on_the_dequantised_twin_and_parity_against_fp64(fa, oracle_mod, idx):
    c = mss.case(idx)
    if c["topk"] == 2048:
        assert fa.mla_decode_sparse_kv8_scaled_workspace_bytes(c["T"], c["Hq"], DV, 2048) == c["T"] * 8 * 16 * 514 * 4  # S = 8
    both(fa, oracle_mod, c, ("gpu sparse kv8 scaled", mss.CASES[idx]), padded_q=idx % 2 == 1, wide_o=idx % 3 == 1)


def test_what_nobody_names_has_no_influence(fa, oracle_mod):
    """every unnamed slot, padding row and byte between rows exchanged (0xFF codes, scales and rotary bits <-> 0x7F codes and the other
    NaN), then a NaN-filled workspace with a canary behind it and lse = None: the same bits; the token without entries: O = 0, LSE = -inf"""
    import torch

    c = mss.case(1)  # 16 heads, topk = 63 at a pitch of 64, counts 0 .. 63, P = 256, rows of 720 bytes, a padding row per page
    o1, l1 = both(fa, oracle_mod, c, "sparse kv8 scaled, 0xFF fill")
    other = mss.refill(c["bytes"], c["named"], c["P"])
    assert (other != c["bytes"]).any(axis=2)[:, :c["P"]][~c["named"].reshape(-1, c["P"])].all() and (other[:, :, ROW:] != c["bytes"][:, :, ROW:]).all()
    o2, l2 = both(fa, oracle_mod, c, "sparse kv8 scaled, the fills exchanged", pool=other)
    assert _same_bits(o1, o2) and _same_bits(l1, l2)
    need = fa.mla_decode_sparse_kv8_scaled_workspace_bytes(c["T"], c["Hq"], DV, c["topk"])
    buf = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    o3, l3 = both(fa, oracle_mod, c, "sparse kv8 scaled, NaN workspace", workspace=buf[:need], return_lse=False)
    assert l3 is None and _same_bits(o1, o3) and (buf[need:] == 0xFF).all()
    dead = c["lens"].index(0)
    assert (o1[dead] == 0).all() and torch.isneginf(l1[dead]).all() and torch.isfinite(o1).all()


def test_named_rows_at_both_ends_of_a_pool_above_4_gib(fa, oracle_mod):
    """25600 pages of 256 rows of 656 bytes: 4.0 GiB and a little. The lists name rows of the first page and of the last, whose byte
    offsets need more than 32 bits; every other byte is 0xFF. The bits must be those of the same rows in a compact two-page pool"""
    import torch

    P, T, Hq, topk, num_pages = 256, 3, 17, 130, 25600
    assert num_pages * P * ROW > (1 << 32) + P * ROW and num_pages * P < (1 << 30)
    rng = np.random.default_rng(3471)
    indices = mla_sparse.make_lists(rng, T, topk, 132, 2 * P, "perm")
    indices[0, :2] = [0, 2 * P - 1]  # the pool's first and last slot
    counts = np.array([130, 65, 1], np.int32)
    pool, named, twin = mss.make_pool(oracle_mod, rng, P, 2 * P, indices, counts, topk)
    c = {"Hq": Hq, "topk": topk, "P": P, "T": T, "bytes": pool, "pool": twin, "indices": indices, "counts": counts,
         "q": oracle_mod.round_to(rng.uniform(-1.0, 1.0, (T, Hq, DQK)).astype(np.float32), DTYPE)}
    c["kvs"], c["lens"] = mla_sparse.gather(c)
    o_c, l_c = both(fa, oracle_mod, c, "sparse kv8 scaled, compact")
    big = torch.full((num_pages, P, ROW), 0xFF, dtype=torch.uint8, device="cuda")
    try:
        big[0], big[-1] = _view(pool, P)[0], _view(pool, P)[1]
        far_idx = np.where(indices >= P, indices + (num_pages - 2) * P, indices)
        o_f, l_f = run(fa, c["q"], big, far_idx, counts, DTYPE, topk=topk)
        assert _same_bits(o_f, o_c) and _same_bits(l_f, l_c), "the far pool differs from the compact one"
    finally:
        del big
        torch.cuda.empty_cache()


def _append_case(oracle_mod, rng, P=16, mp=4, row_stride=720):
    """five sequences appended at once into a canary-filled pool of wide rows: positions below 0 (the last sequence), past the capacity
    (the third) and on a table entry outside the pool (the fourth, its third page) are skipped. Returns the new rows, the tables, the
    pool as the numpy reference leaves it, and per sequence the slots of the rows that were written, in order"""
    before, new = [0, 17, 60, 30, -2], [5, 40, 9, 7, 5]
    after = [a + n for a, n in zip(before, new)]
    B, total, num_pages = len(new), sum(new), 5 * mp + 2
    table = rng.permutation(num_pages - 1)[:B * mp].reshape(B, mp).astype(np.int32)
    table[3, 2] = num_pages + 3
    x = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (total, DQK)).astype(np.float32) * np.exp2(rng.integers(-6, 1, (total, 1))).astype(np.float32),
                            DTYPE)
    x[0, :128] = 0.0                                 # an all-zero group: e = -32
    x[1, 128:256] = np.clip(x[1, 128:256], -1, 1)
    x[1, 130] = -448.0 * 2.0 ** -3                   # amax exactly 448 * 2^e
    x[2, 256:384] = np.clip(x[2, 256:384], -1, 1)
    x[2, 300] = 450.0 * 2.0 ** -3                    # the next bf16 value above it: e + 1
    x[3, 384:512] *= np.float32(2.0 ** 40)           # too large for e = 32: saturates through the clamp
    want = mss.quantise(x)
    host = np.full((num_pages, P + 1, row_stride), 0xA5, np.uint8)
    cu = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    slots = []
    for b in range(B):
        pos = np.arange(before[b], after[b])
        ok = (pos >= 0) & (pos < P * mp) & (table[b, np.clip(pos // P, 0, mp - 1)] < num_pages)
        slots.append((table[b, pos[ok] // P] * P + pos[ok] % P).astype(np.int32))
        host[slots[b] // P, slots[b] % P, :ROW] = want[cu[b]:cu[b + 1]][ok]
    assert [len(s) for s in slots] == [5, 40, 4, 2, 3]
    return x, cu, table, np.array(after, np.int32), max(new), host, slots


def test_append_writes_the_reference_bytes_and_nothing_else_and_the_chain(fa, oracle_mod):
    import torch

    P, Hq = 16, 16
    rng = np.random.default_rng(3481)
    x, cu, table, after, max_new, host, slots = _append_case(oracle_mod, rng)
    pool = torch.full(host.shape, 0xA5, dtype=torch.uint8, device="cuda")
    xd = torch.full((x.shape[0], 640), float("nan"), dtype=torch.bfloat16, device="cuda")  # (a row stride above 576)
    xd[:, :DQK] = _dev(x, DTYPE)
    fa.mla_kv_append_paged_scaled(xd[:, :DQK], pool[:, :P, :ROW], _i32(cu), _i32(table), _i32(after), max_new)
    torch.cuda.synchronize()
    got = pool.cpu().numpy()
    assert np.array_equal(got[:, :P, :ROW], host[:, :P, :ROW]), "the written rows, scales included, and the slots nobody wrote"
    assert np.array_equal(got, host), "the canaries between rows and in the padding rows"
    # the chain: attention over the slots just written, in shuffled order, on the appended pool = on the reference's dequantised rows
    # (but for the first sequence's four edge rows, whose magnitudes are no attention input: the bytes above are their check)
    topk = 40
    slots[0] = slots[0][4:]
    idx = np.full((len(slots), topk), -7, np.int32)
    for b, s in enumerate(slots):
        idx[b, :len(s)] = rng.permutation(s)
    counts = np.array([len(s) for s in slots], np.int32)
    twin = mss.dequant(oracle_mod, host[:, :P, :ROW].reshape(-1, ROW)).reshape(-1, P, DQK)
    c = {"Hq": Hq, "topk": topk, "P": P, "T": len(slots), "bytes": got, "pool": twin, "indices": idx, "counts": counts,
         "q": oracle_mod.round_to(rng.uniform(-1.0, 1.0, (len(slots), Hq, DQK)).astype(np.float32), DTYPE)}
    c["kvs"], c["lens"] = mla_sparse.gather(c)
    both(fa, oracle_mod, c, "append, then sparse kv8 scaled")


def test_graph_of_append_and_attention_replayed_after_rows_and_lists_changed_in_place(fa, oracle_mod):
    import torch

    P, Hq, topk = 16, 16, 40
    rng = np.random.default_rng(3491)
    x, cu, table, after, max_new, host, slots = _append_case(oracle_mod, rng)
    xd, cud, td, ad = _dev(x, DTYPE), _i32(cu), _i32(table), _i32(after)
    qd = _dev(rng.uniform(-1.0, 1.0, (len(slots), Hq, DQK)).astype(np.float32), DTYPE)
    idx = torch.full((len(slots), topk), -7, dtype=torch.int32, device="cuda")
    cnt = _i32([len(s) for s in slots])
    pool = torch.full(host.shape, 0xA5, dtype=torch.uint8, device="cuda")
    out, lse = torch.empty((len(slots), Hq, DV), dtype=qd.dtype, device="cuda"), torch.empty((len(slots), Hq), dtype=torch.float32, device="cuda")
    ws = torch.empty(fa.mla_decode_sparse_kv8_scaled_workspace_bytes(len(slots), Hq, DV, topk), dtype=torch.uint8, device="cuda")

    def call(pool, out, lse):
        fa.mla_kv_append_paged_scaled(xd, pool[:, :P, :ROW], cud, td, ad, max_new)
        fa.flash_attention_mla_decode_sparse(qd, pool[:, :P, :ROW], idx, SCALE, index_counts=cnt, out=out, lse=lse, workspace=ws)

    def fill(seed):  # new rows and newly shuffled lists, in place
        r = np.random.default_rng(seed)
        xd.copy_(_dev(oracle_mod.round_to(r.uniform(-3.0, 3.0, x.shape).astype(np.float32), DTYPE), DTYPE))
        for b, s in enumerate(slots):
            idx[b, :len(s)] = _i32(r.permutation(s))

    fill(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # a warm-up call outside the capture (the first call sets the kernel's LDS attribute)
        call(pool, out, lse)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(pool, out, lse)
    for seed in (1, 2, 3):
        fill(seed)
        g.replay()
        torch.cuda.synchronize()
        pool2, o2, l2 = torch.full_like(pool, 0xA5), torch.empty_like(out), torch.empty_like(lse)
        call(pool2, o2, l2)
        torch.cuda.synchronize()
        assert torch.equal(pool, pool2) and _same_bits(out, o2) and _same_bits(lse, l2) and torch.isfinite(out).all(), seed
