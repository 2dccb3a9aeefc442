"""GPU parity of fa_fwd_decode_paged (a decode step against a paged KV cache with a length per sequence; include/fa_mi355.h) against
the fp64 oracle of the generalised operator on each sequence's gathered keys, and bit for bit against fa_fwd_decode on the gathered
dense cache when every sequence is full. Page tables are shuffled over a pool larger than needed; every page nobody references and
every slot past a sequence's length holds NaN. Not in the reference: unpinned by it, like the rest of scope row f3."""
import numpy as np
import pytest

from util import LN2, TORCH_DTYPE, effective_q, lse_tol

pytestmark = pytest.mark.gpu

TOL_O = {"f16": 1.5e-3, "bf16": 6e-3}


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


def _dev(x, dtype):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).to(getattr(torch, TORCH_DTYPE[dtype])).cuda()


def _i32(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def make_cache(oracle, rng, Hkv, D, P, lens, dtype, layout="HND", spare=3, max_pages=None, amp=1.0):
    """Pools (device, `layout`), block table, per-sequence K / V [Hkv, L_b, D] (fp32 holding `dtype` values). Pages are a random
    permutation of the pool; unused table entries name a NaN-filled spare page; slots past L_b in a last page are NaN."""
    npb = [(L + P - 1) // P for L in lens]
    mp = max_pages or max(max(npb), 1)
    num_pages = sum(npb) + spare
    perm = rng.permutation(num_pages)
    kpool = np.full((num_pages, Hkv, P, D), np.nan, np.float32)
    vpool = np.full((num_pages, Hkv, P, D), np.nan, np.float32)
    table = np.full((len(lens), mp), perm[-1], np.int32)
    ks, vs, used = [], [], 0
    for b, L in enumerate(lens):
        pages = perm[used:used + npb[b]]
        used += npb[b]
        table[b, :npb[b]] = pages
        k = oracle.round_to(amp * rng.uniform(-1.0, 1.0, (Hkv, L, D)).astype(np.float32), dtype)
        v = oracle.round_to(amp * rng.uniform(-1.0, 1.0, (Hkv, L, D)).astype(np.float32), dtype)
        for j, pg in enumerate(pages):
            n = min(P, L - j * P)
            kpool[pg, :, :n] = k[:, j * P:j * P + n]
            vpool[pg, :, :n] = v[:, j * P:j * P + n]
        ks.append(k)
        vs.append(v)
    return to_layout(kpool, dtype, layout), to_layout(vpool, dtype, layout), table, ks, vs


def to_layout(pool, dtype, layout):
    return _dev(pool if layout == "HND" else pool.transpose(0, 2, 1, 3), dtype)


def expected(oracle, q, ks, vs, lens, causal, scale=None):
    """fp64 (O, LSE) per sequence on its own keys; rows with no visible key: O = 0, LSE = -inf."""
    B, Hq, Nq, D = q.shape
    o = np.zeros(q.shape, np.float64)
    lse = np.full((B, Hq, Nq), -np.inf)
    for b, L in enumerate(lens):
        if L == 0:
            continue
        if not causal or L >= Nq:
            o[b:b + 1], lse[b:b + 1] = oracle.attn_fwd_ex_f64(q[b:b + 1], ks[b][None], vs[b][None], causal, scale)
            continue
        for i in range(Nq):  # causal with fewer keys than queries: row i sees keys [0, i + L - Nq]
            vis = i + L - Nq + 1
            if vis > 0:
                oi, li = oracle.attn_fwd_ex_f64(np.ascontiguousarray(q[b:b + 1, :, i:i + 1]), np.ascontiguousarray(ks[b][None, :, :vis]),
                                                np.ascontiguousarray(vs[b][None, :, :vis]), False, scale)
                o[b, :, i], lse[b, :, i] = oi[0, :, 0], li[0, :, 0]
    return o, lse


def check(oracle, o, lse, q, ks, vs, lens, causal, dtype, what, tol_o=None, strict=True):
    on, ln = o.float().cpu().numpy(), lse.cpu().numpy()
    o64, l64 = expected(oracle, q, ks, vs, lens, causal)
    empty = np.isneginf(l64)
    assert np.array_equal(on[empty], np.zeros_like(on[empty])) and np.isneginf(ln[empty]).all(), what  # exactly 0 and -inf
    full = ~empty
    assert np.isfinite(on).all() and np.isfinite(ln[full]).all(), what
    kk = np.concatenate([k.reshape(-1, k.shape[-1]) for k in ks if k.size] or [np.zeros((1, q.shape[-1]), np.float32)])
    tol_o = TOL_O[dtype] if tol_o is None else tol_o
    assert np.abs(on - o64).max() < tol_o, (what, np.abs(on - o64).max())
    assert np.abs(ln[full] - l64[full]).max(initial=0.0) < lse_tol("bf16" if dtype == "fp8" else dtype, 1, q, kk), what
    if strict:  # the exact operator on the pre-scaled operand the kernel multiplies
        o64q, l64q = expected(oracle, effective_q(oracle, q, dtype), ks, vs, lens, causal, LN2)
        assert np.abs(on - o64q).max() < tol_o and np.abs(ln[full] - l64q[full]).max(initial=0.0) < 1e-4, what


SHAPES = [  # Hq, Hkv, Nq, D, causal: grouped heads and several causal queries, as the dense decode's CASES
    (32, 8, 1, 64, True), (16, 2, 4, 128, True), (8, 8, 2, 64, False), (8, 4, 7, 128, True),
]


@pytest.mark.parametrize("P", [16, 64, 256])
@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_paged_vs_oracle(fa, oracle_mod, P, layout, dtype):
    import torch

    rng = np.random.default_rng(100 + P)
    lens = [0, 1, 63, 64, 65, P - 1, P, P + 1, 1000, 4097, 16384]
    for (Hq, Hkv, Nq, D, causal) in SHAPES:
        ls = [int(x) for x in rng.permutation(lens)]
        B = len(ls)
        q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (B, Hq, Nq, D)).astype(np.float32), dtype)
        kp, vp, table, ks, vs = make_cache(oracle_mod, rng, Hkv, D, P, ls, dtype, layout)
        o, lse = fa.flash_attention_decode_paged(_dev(q, dtype), kp, vp, _i32(table), _i32(ls), is_causal=causal, layout=layout)
        torch.cuda.synchronize()
        check(oracle_mod, o, lse, q, ks, vs, ls, causal, dtype, (P, layout, dtype, Hq, Hkv, Nq, D, causal))


@pytest.mark.parametrize("layout", ["HND", "NHD"])
def test_paged_full_cache_is_bit_identical_to_dense_decode(fa, oracle_mod, layout):
    import torch

    fp8 = torch.float8_e4m3fn
    rng = np.random.default_rng(7)
    for (qdt, kvdt) in (("f16", "f16"), ("bf16", "bf16"), ("fp8", "fp8"), ("bf16", "fp8")):
        for (B, Hq, Hkv, Nq, D, causal, P, mp) in ((3, 16, 4, 2, 128, True, 16, 64), (2, 32, 8, 1, 64, False, 64, 40),
                                                    (2, 8, 2, 4, 64, True, 256, 5),
                                                    # 65536 keys on B * Hkv = 2: 256 key splits (tests/decode_range.py S_OF_NK)
                                                    (1, 8, 2, 1, 64, False, 16, 4096), (1, 8, 2, 4, 128, True, 256, 256)):
            cap = P * mp
            amp = 2.0 if kvdt == "fp8" else 1.0
            q = oracle_mod.round_to(amp * rng.uniform(-1.0, 1.0, (B, Hq, Nq, D)).astype(np.float32), qdt)
            kp, vp, table, ks, vs = make_cache(oracle_mod, rng, Hkv, D, P, [cap] * B, kvdt, layout, amp=amp)
            qd = _dev(q, qdt)
            o, lse = fa.flash_attention_decode_paged(qd, kp, vp, _i32(table), _i32([cap] * B), is_causal=causal, layout=layout)
            kd, vd = (_dev(np.stack(x), kvdt) for x in (ks, vs))  # the gathered dense cache [B, Hkv, cap, D]
            o2, lse2 = fa.flash_attention_decode(qd, kd, vd, is_causal=causal)
            torch.cuda.synchronize()
            what = (qdt, kvdt, layout, B, Hq, Hkv, Nq, D, causal, P)
            assert o.dtype == o2.dtype == (torch.bfloat16 if kd.dtype == fp8 else qd.dtype), what
            assert torch.equal(o, o2) and torch.equal(lse, lse2), what


def test_paged_e4m3(fa, oracle_mod):
    """An e4m3 pool under e4m3 or bf16 queries: widened exactly to bf16 on the way into LDS, so the result is the bf16 paged path's on the
    widened pool (other key splits: close, not equal) and holds the bars of test_gpu_decode.py::test_decode_e4m3_inputs."""
    import torch

    rng = np.random.default_rng(8)
    for (qdt, Hq, Hkv, Nq, D, causal, P, layout) in (("fp8", 32, 8, 1, 128, True, 64, "HND"), ("bf16", 16, 4, 2, 64, True, 16, "NHD"),
                                                      ("bf16", 32, 8, 1, 128, False, 256, "NHD"), ("fp8", 8, 8, 4, 64, True, 32, "HND")):
        ls = [int(x) for x in rng.permutation([0, 1, 65, P - 1, P + 1, 1000, 4097])]
        B = len(ls)
        amp = 2.0 if qdt == "fp8" else 1.0
        q = oracle_mod.round_to(amp * rng.uniform(-1.0, 1.0, (B, Hq, Nq, D)).astype(np.float32), qdt)
        kp, vp, table, ks, vs = make_cache(oracle_mod, rng, Hkv, D, P, ls, "fp8", layout, amp=2.0)
        bt, sl = _i32(table), _i32(ls)
        o8, l8 = fa.flash_attention_decode_paged(_dev(q, qdt), kp, vp, bt, sl, is_causal=causal, layout=layout)
        ob, lb = fa.flash_attention_decode_paged(_dev(q, "bf16"), kp.to(torch.bfloat16), vp.to(torch.bfloat16), bt, sl, is_causal=causal,
                                                 layout=layout)
        torch.cuda.synchronize()
        what = (qdt, Hq, Hkv, Nq, D, causal, P, layout)
        assert o8.dtype == torch.bfloat16 and (o8.float() - ob.float()).abs().max().item() < TOL_O["bf16"], what
        fin = torch.isfinite(lb)
        assert torch.equal(fin, torch.isfinite(l8)) and (l8[fin] - lb[fin]).abs().max().item() < 2e-5, what
        check(oracle_mod, o8, l8, q, ks, vs, ls, causal, "fp8", what, tol_o=2 * TOL_O["bf16"], strict=False)


def test_paged_empty_rows(fa, oracle_mod):
    """L_b = 0, and causal rows with i + L_b < Nq: exactly 0 and -inf; the other rows as the oracle says."""
    import torch

    rng = np.random.default_rng(9)
    Hq, Hkv, Nq, D, P = 8, 2, 8, 64, 16
    for causal in (True, False):
        ls = [0, 3, 0, 7, 8, 9, 700]
        q = oracle_mod.round_to(rng.uniform(-1.0, 1.0, (len(ls), Hq, Nq, D)).astype(np.float32), "bf16")
        kp, vp, table, ks, vs = make_cache(oracle_mod, rng, Hkv, D, P, ls, "bf16")
        o, lse = fa.flash_attention_decode_paged(_dev(q, "bf16"), kp, vp, _i32(table), _i32(ls), is_causal=causal)
        torch.cuda.synchronize()
        ln = lse.cpu().numpy()
        assert np.isneginf(ln[0]).all() and np.isneginf(ln[2]).all() and np.isfinite(ln[4:]).all()
        if causal:  # L = 3: rows 0..4 see nothing; L = 7: row 0 sees nothing
            assert np.isneginf(ln[1, :, :5]).all() and np.isfinite(ln[1, :, 5:]).all() and np.isneginf(ln[3, :, 0]).all()
        check(oracle_mod, o, lse, q, ks, vs, ls, causal, "bf16", ("empty rows", causal))


def test_paged_known_answers_across_page_tile_and_split_edges(fa):
    """Q = 0 -> uniform softmax over the visible keys; V[j, 0] = delta(j, t) through a shuffled table: O[i, 0] = 1 / visible(i) if t is
    visible, EXACTLY 0 else; t at page (16), tile (64) and split edges of both sequences."""
    import torch

    B, Hq, Hkv, Nq, D, P = 2, 8, 2, 4, 64, 16
    lens = [1000, 701]
    mp = 64
    rng = np.random.default_rng(10)
    num_pages = 110
    perm = rng.permutation(num_pages)
    table = np.full((B, mp), perm[-1], np.int32)
    table[0, :63], table[1, :44] = perm[:63], perm[63:107]
    bt, sl = _i32(table), _i32(lens)
    q = torch.zeros(B, Hq, Nq, D, dtype=torch.bfloat16, device="cuda")
    kp = torch.randn(num_pages, Hkv, P, D, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(fa.decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, P, mp), dtype=torch.uint8, device="cuda")
    edges = sorted({e + d for e in range(0, 1000, 16) for d in (-1, 0)} | {e + 1 for e in range(0, 1000, 64)} | {698, 699, 700, 995, 996, 999})
    for t in [e for e in edges if 0 <= e < 1000]:
        vp = torch.zeros(num_pages, Hkv, P, D, dtype=torch.bfloat16, device="cuda")
        for b, L in enumerate(lens):
            vp[int(perm[-1])] = float("nan")  # the spare page nobody's valid keys live in
            last = int(table[b, (L - 1) // P])
            vp[last, :, (L - 1) % P + 1:] = float("nan")  # the tail of the last page
            if t < L:
                vp[int(table[b, t // P]), :, t % P, 0] = 1.0
        ws.fill_(0xFF)
        o, lse = fa.flash_attention_decode_paged(q, kp, vp, bt, sl, is_causal=True, workspace=ws)
        torch.cuda.synchronize()
        on, ln = o.float().cpu().numpy(), lse.cpu().numpy()
        for b, L in enumerate(lens):
            for iq in range(Nq):
                vis = L - Nq + iq + 1
                col = on[b, :, iq, 0]
                if t < vis:
                    want = float(torch.tensor(1.0 / vis, dtype=torch.bfloat16).float())
                    assert np.all(np.abs(col - want) <= 8e-3 * want), (t, b, iq, col, want)
                else:
                    assert np.array_equal(col, np.zeros(Hq, np.float32)), (t, b, iq)
                assert np.abs(ln[b, :, iq] - np.log(vis)).max() < 1e-5, (t, b, iq)
        assert np.count_nonzero(on[..., 1:]) == 0, t


def test_paged_pool_over_4gib(fa, oracle_mod):
    """A bf16 pool of 4.5 GiB with every used page past byte offset 2^32 gives the bits the same data gives in low pages."""
    import torch

    Hq, Hkv, Nq, D, P = 32, 8, 1, 128, 256
    page_bytes = Hkv * P * D * 2
    num_pages = (9 << 29) // page_bytes  # 4.5 GiB
    lens = [5000, 12345]
    rng = np.random.default_rng(11)
    kp_lo, vp_lo, table, ks, vs = make_cache(oracle_mod, rng, Hkv, D, P, lens, "bf16", spare=1)
    used = int(table.max()) + 1
    first_hi = (1 << 32) // page_bytes + 3
    assert first_hi + used <= num_pages
    q = _dev(oracle_mod.round_to(rng.uniform(-1.0, 1.0, (2, Hq, Nq, D)).astype(np.float32), "bf16"), "bf16")
    sl = _i32(lens)
    o_lo, l_lo = fa.flash_attention_decode_paged(q, kp_lo, vp_lo, _i32(table), sl, is_causal=True)
    kp = torch.empty(num_pages, Hkv, P, D, dtype=torch.bfloat16, device="cuda")
    vp = torch.empty_like(kp)
    kp[first_hi:first_hi + used] = kp_lo[:used]
    vp[first_hi:first_hi + used] = vp_lo[:used]
    o_hi, l_hi = fa.flash_attention_decode_paged(q, kp, vp, _i32(table + first_hi), sl, is_causal=True)
    torch.cuda.synchronize()
    assert torch.equal(o_hi, o_lo) and torch.equal(l_hi, l_lo)
    del kp, vp
    check(oracle_mod, o_lo, l_lo, q.float().cpu().numpy(), ks, vs, lens, True, "bf16", "4 GiB", strict=False)


def test_paged_graph_capture_and_replay_with_new_tables(fa, oracle_mod):
    """One captured call (one stream, two kernels in sequence): rewriting seqlens_k and block_table in place between replays changes
    the lengths and pages it reads; every replay equals an eager call."""
    import torch

    Hq, Hkv, Nq, D, P, mp = 16, 4, 2, 128, 64, 40
    rng = np.random.default_rng(12)
    B = 3
    kp, vp, table0, _, _ = make_cache(oracle_mod, rng, Hkv, D, P, [P * mp] * B, "bf16", spare=0, max_pages=mp)
    num_pages = kp.shape[0]
    q = torch.randn(B, Hq, Nq, D, dtype=torch.bfloat16, device="cuda")
    bt, sl = _i32(table0), _i32([100, 2000, 1])
    ws = torch.empty(fa.decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, P, mp), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(q)
    lse = torch.empty(B, Hq, Nq, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm up outside the capture
        fa.flash_attention_decode_paged(q, kp, vp, bt, sl, is_causal=True, out=out, lse=lse, workspace=ws)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fa.flash_attention_decode_paged(q, kp, vp, bt, sl, is_causal=True, out=out, lse=lse, workspace=ws)
    for step in range(4):
        lens = [int(x) for x in rng.integers(0, P * mp + 1, B)]
        if step == 0:
            lens = [P * mp, 0, 65]
        tbl = np.stack([rng.permutation(num_pages)[:mp] for _ in range(B)]).astype(np.int32)
        sl.copy_(_i32(lens))
        bt.copy_(_i32(tbl))
        g.replay()
        torch.cuda.synchronize()
        o_g, l_g = out.clone(), lse.clone()
        o_e, l_e = fa.flash_attention_decode_paged(q, kp, vp, _i32(tbl), _i32(lens), is_causal=True)
        torch.cuda.synchronize()
        assert torch.equal(o_g, o_e) and torch.equal(l_g, l_e), (step, lens)


def test_paged_workspace_contents_and_wrapper_errors(fa, oracle_mod):
    import torch

    Hq, Hkv, Nq, D, P = 8, 2, 2, 64, 32
    rng = np.random.default_rng(13)
    ls = [900, 0, 33]
    kp, vp, table, _, _ = make_cache(oracle_mod, rng, Hkv, D, P, ls, "bf16")
    q = torch.randn(len(ls), Hq, Nq, D, dtype=torch.bfloat16, device="cuda")
    bt, sl = _i32(table), _i32(ls)
    ws = torch.empty(fa.decode_paged_workspace_bytes(len(ls), Hq, Hkv, Nq, D, P, table.shape[1]), dtype=torch.uint8, device="cuda")
    ws.zero_()
    o1, l1 = fa.flash_attention_decode_paged(q, kp, vp, bt, sl, is_causal=True, workspace=ws)
    ws.fill_(0xFF)
    o2, l2 = fa.flash_attention_decode_paged(q, kp, vp, bt, sl, is_causal=True, workspace=ws)
    o3, l3 = fa.flash_attention_decode_paged(q, kp, vp, bt, sl, is_causal=True)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and torch.equal(o1, o3) and torch.equal(l1, l3)
    with pytest.raises(ValueError):
        fa.flash_attention_decode_paged(q, kp, vp, bt.long(), sl)  # int64 table
    with pytest.raises(ValueError):
        fa.flash_attention_decode_paged(q, kp, vp, bt, sl.cpu())  # a table on the host
    with pytest.raises(ValueError):
        fa.flash_attention_decode_paged(q, kp, vp, bt.cpu(), sl)
    with pytest.raises(ValueError):
        fa.flash_attention_decode_paged(q, kp, vp[:-1], bt, sl)  # pools of different shapes
    with pytest.raises(ValueError):
        fa.flash_attention_decode_paged(q.half(), kp, vp, bt, sl)  # mixed dtypes
    with pytest.raises(ValueError):
        fa.flash_attention_decode_paged(q, kp, vp.half(), bt, sl)
    with pytest.raises(ValueError):
        fa.flash_attention_decode_paged(q, kp, vp, bt, sl, layout="NDH")
    with pytest.raises(fa.FaError) as e:
        fa.flash_attention_decode_paged(q, kp, vp, bt, sl, workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
    assert e.value.status == -1 and "workspace" in str(e.value)
