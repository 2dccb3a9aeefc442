"""GPU: the e4m3 indexer's input stage (include/fa_mi355.h, "The MLA indexer's input stage") -- fa_mla_indexer_k_append_paged_quant and
fa_mla_indexer_q_quant against a numpy fp32 model of the row rule, BIT FOR BIT (the arithmetic is specified, so there is no tolerance):
whole pools, scales and paddings over sentinels, and the chain into fa_mla_indexer_logits_paged_kv8 on inputs the stage keeps exactly."""
import numpy as np
import pytest

import kv8
from test_gpu_mla_indexer import TORCH, fa  # noqa: F401  (fa: fixture)

pytestmark = pytest.mark.gpu


def row_rule(x, rotate):
    """x fp32 [n, 128] -> (codes uint8 [n, 128], e int32 [n]): every step one fp32 operation, in the header's order"""
    y = np.array(x, np.float32)
    if rotate:
        i = np.arange(128)
        for s in range(7):
            lo = i[(i >> s) & 1 == 0]
            y[:, lo], y[:, lo + (1 << s)] = y[:, lo] + y[:, lo + (1 << s)], y[:, lo] - y[:, lo + (1 << s)]
        y = y * np.float32(128 ** -0.5)
    amax = np.abs(y).max(1)
    m, k = np.frexp(amax)  # amax = m * 2^k, 0.5 <= m < 1, and 448 = 0.875 * 2^9
    e = np.clip(np.where(amax == 0, -32, k - 9 + (m > 0.875)), -32, 32).astype(np.int32)
    return kv8.to_e4m3_bytes(np.clip(y * np.ldexp(np.float32(1), -e).astype(np.float32)[:, None], -448.0, 448.0)), e


def draw_rows(rng, n, dtype):
    """(fp32 numpy, device tensor) of n rows of `dtype` values, a different magnitude per row; rows 1 .. 8 are special: zeros (two of them
    -0), amax exactly 448 * 2^-3 and one step above it, a row that saturates (bf16; f16 has no such value) and a tiny one, and rows
    whose butterfly sums cancel (constant, alternating, one element)"""
    import torch

    x = rng.standard_normal((n, 128)) * np.ldexp(1.0, rng.integers(-6, 7, (n, 1)))
    x[1] = 0.0
    x[1, [5, 70]] = -0.0
    x[2], x[3] = rng.uniform(-50, 50, 128), rng.uniform(-50, 50, 128)
    x[2, 77], x[3, 3] = -56.0, 56.25
    x[4, 9] = 2.0 ** 50 if dtype == "bf16" else 60000.0
    x[5] = rng.standard_normal(128) * (2.0 ** -38 if dtype == "bf16" else 2.0 ** -12)  # (bf16: e clamps at -32)
    x[6], x[7], x[8] = 3.0, 3.0 * (-1.0) ** np.arange(128), 0.0
    x[8, 37] = -1.5
    t = torch.from_numpy(x).to(getattr(torch, TORCH[dtype]))
    return t.float().numpy(), t.cuda()


@pytest.mark.parametrize("P", [16, 64])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("rotate", [0, 1])
def test_the_append_writes_numpys_image_and_nothing_else(fa, rotate, dtype, packed, P):
    import torch

    rng, mp, num_pages = np.random.default_rng(3600 + P), 3, 11
    n = [P + 5, 0, 6]     # sequence 0 crosses two page boundaries; sequence 1 appends nothing
    sk = [2 * P + 2, 7, 3 * P + 1]  # sequence 2's last token lies past the capacity
    bt = rng.permutation(num_pages)[:9].reshape(3, mp).astype(np.int32)
    bt[0, 2], bt[1, 0] = num_pages + 2, -1  # sequence 0's last two tokens: a table entry outside the pool
    cu = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    x, dx = draw_rows(rng, cu[-1] + 2, dtype)  # (two rows nobody owns)
    codes, e = row_rule(x, rotate)
    if packed:  # pages of 128 P code bytes followed by 4 P scale bytes
        pool = np.full((num_pages, 132 * P), 0xA5, np.uint8)
        kv = lambda a: a[:, :128 * P].reshape(num_pages, P, 128) if isinstance(a, np.ndarray) else a[:, :128 * P].unflatten(1, (P, 128))
        sv = lambda a, _: a[:, 128 * P:].view(np.float32 if isinstance(a, np.ndarray) else torch.float32)
        scales = pool
    else:  # a pool with bytes between rows and a padding row per page, scales with padding columns
        pool, scales = np.full((num_pages, P + 1, 144), 0xA5, np.uint8), np.full((num_pages, P + 3), -7.25, np.float32)
        kv = lambda a: a[:, :P, :128]
        sv = lambda _, s: s[:, :P]
    dpool, dscales = torch.from_numpy(pool.copy()).cuda(), (None if packed else torch.from_numpy(scales.copy()).cuda())
    for b in range(3):
        for i in range(n[b]):
            pos = sk[b] - n[b] + i
            if 0 <= pos < mp * P and 0 <= bt[b, pos // P] < num_pages:
                kv(pool)[bt[b, pos // P], pos % P] = codes[cu[b] + i]
                sv(pool, scales)[bt[b, pos // P], pos % P] = np.ldexp(np.float32(1), e[cu[b] + i])
    assert len(set(e[:cu[-1]])) > 4  # (the rows' exponents differ)
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.int32)).cuda()
    fa.mla_indexer_k_append_quant(dx, kv(dpool), sv(dpool, dscales), i32(cu), i32(bt), i32(sk), max(n), rotate=bool(rotate))
    assert np.array_equal(dpool.cpu().numpy(), pool)
    assert packed or np.array_equal(dscales.cpu().numpy().view(np.uint32), scales.view(np.uint32))


@pytest.mark.parametrize("Hi", [32, 64])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("rotate", [0, 1])
def test_the_query_call_writes_numpys_codes_and_weights(fa, rotate, dtype, Hi):
    import torch

    rng, T, w_mul, alias = np.random.default_rng(3610 + Hi), 5, 0.17, (Hi == 32 and dtype == "bf16")
    x, dx = draw_rows(rng, T * Hi, dtype)
    codes, e = row_rule(x, rotate)
    q = torch.zeros((T, Hi + 1, 160), dtype=getattr(torch, TORCH[dtype]), device="cuda")  # wide strides, in and out
    q[:, :Hi, :128] = dx.view(T, Hi, 128)
    hw = rng.uniform(0.1, 3.0, (T, Hi + 3)).astype(np.float32)
    want_q, want_w = np.full((T, Hi + 2, 144), 0x5A, np.uint8), (hw.copy() if alias else np.full((T, Hi + 3), -7.25, np.float32))
    dq, dhw = torch.from_numpy(want_q.copy()).cuda(), torch.from_numpy(hw).cuda()
    dw = dhw if alias else torch.from_numpy(want_w.copy()).cuda()  # (alias: w_out is head_w itself, in place)
    want_q[:, :Hi, :128] = codes.reshape(T, Hi, 128)
    want_w[:, :Hi] = (hw[:, :Hi] * np.float32(w_mul)) * np.ldexp(np.float32(1), e).astype(np.float32).reshape(T, Hi)
    q8, w = fa.mla_indexer_q_quant(q[:, :Hi, :128], dhw[:, :Hi], w_mul=w_mul, rotate=bool(rotate), q_out=dq[:, :Hi, :128], w_out=dw[:, :Hi])
    assert q8.data_ptr() == dq.data_ptr() and w.data_ptr() == dw.data_ptr()
    assert np.array_equal(dq.cpu().numpy(), want_q)
    assert np.array_equal(dw.cpu().numpy().view(np.uint32), want_w.view(np.uint32))


def test_the_library_written_cache_and_query_give_the_16_bit_logits(fa):
    """rotate = 0 on integer rows in [-8, 8] that each hold an 8: every e is -5 and every code exact, so the e4m3 logits on what the two
    calls wrote and the bf16 logits on the unquantised inputs are both exact (the header's exact-inputs clause) and must be equal bits"""
    import torch

    rng = np.random.default_rng(3620)
    Hi, P, L, Lq = 32, 16, 100, 3
    mp, num_pages = -(-L // P), 9

    def ints(n):
        a = rng.integers(-8, 9, (n, 128)).astype(np.float32)
        a[np.arange(n), rng.integers(0, 128, n)] = 8.0
        return a

    k, q, hw = ints(L), ints(Lq * Hi), rng.integers(1, 5, (Lq, Hi)).astype(np.float32)
    for a in (k, q):  # the numpy model keeps these inputs exactly, so both sides see the same numbers
        codes, e = row_rule(a, 0)
        assert (e == -5).all() and np.array_equal(kv8.widen(codes) * np.float32(2.0 ** -5), a)
    i32 = lambda a: torch.from_numpy(np.asarray(a, np.int32)).cuda()
    bt, cu_new, cu_q, sk = i32(rng.permutation(num_pages)[:mp].reshape(1, mp)), i32([0, L]), i32([0, Lq]), i32([L])
    k16, q16 = torch.from_numpy(k).bfloat16().cuda(), torch.from_numpy(q).bfloat16().cuda().view(Lq, Hi, 128)
    pool16 = torch.zeros((num_pages, P, 128), dtype=torch.bfloat16, device="cuda")
    pool16.view(-1, 128)[(bt[0].long()[:, None] * P + torch.arange(P, device="cuda")).flatten()[:L]] = k16
    pool8 = torch.zeros((num_pages, P, 128), dtype=torch.float8_e4m3fn, device="cuda")
    ks = torch.zeros((num_pages, P), device="cuda")
    fa.mla_indexer_k_append_quant(k16, pool8, ks, cu_new, bt, sk, L, rotate=False)
    q8, w8 = fa.mla_indexer_q_quant(q16, torch.from_numpy(hw).cuda(), rotate=False)
    got = fa.mla_indexer_logits(q8, w8, pool8, cu_q, bt, sk, Lq, k_scale_pages=ks)
    want = fa.mla_indexer_logits(q16, torch.from_numpy(hw).cuda(), pool16, cu_q, bt, sk, Lq)
    for t in range(Lq):
        v = L - Lq + t + 1
        assert torch.equal(got[t, :v].view(torch.int32), want[t, :v].view(torch.int32)) and float(want[t, :v].abs().max()) > 0, t
