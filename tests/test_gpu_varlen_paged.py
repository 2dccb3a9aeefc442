"""GPU: fa_fwd_varlen_paged (flash_attention_varlen_paged), packed queries against a paged KV cache, and fa_kv_append_paged.

Per sequence the operator is fa_fwd_ex on the sequence's gathered keys, so every check is made sequence by sequence:
  * against the fp64 oracle on the effective (pre-scaled) Q at the bars of tests/test_gpu_varlen.py (util.TOL_O, util.lse_tol); rows
    without a visible key give exactly 0 and -inf;
  * bit for bit against fa_fwd_varlen on the gathered dense cache (every sequence the header's identity covers), across page sizes,
    layouts and page orders, and with NaN / spare / out-of-range storage that nobody may read;
  * the write footprint in canary-filled buffers, also under the table corruptions the contract clamps;
  * chunked prefill through fa_kv_append_paged against one call on the full cache, and a last token against fa_fwd_decode_paged;
  * the append byte for byte; the exact-arithmetic inputs of tests/exact_forward.py; a captured graph replayed after the tables
    changed in place; a pool above 4 GiB; return_lse=False.
The cases live in tests/varlen_paged.py (checked on the CPU by tests/test_varlen_paged_cases.py)."""
import numpy as np
import pytest

import exact_forward as ef
import varlen_paged as vp
from test_gpu_decode_paged import to_layout
from util import LN2, TOL_O, effective_q, lse_tol, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


# ---- helpers -------------------------------------------------------------------------------------------------------------------
def i32(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def paged(fa, q, kp, vpool, cu_q, table, lens_k, max_q, causal, layout, **kw):
    import torch

    o, lse = fa.flash_attention_varlen_paged(q, kp, vpool, i32(cu_q), i32(table), i32(lens_k), int(max_q), is_causal=causal, layout=layout, **kw)
    torch.cuda.synchronize()
    return o, lse


def dense_varlen(fa, q, ks, vs, cu_q, max_q, causal, dtype, scale=None):
    """fa_fwd_varlen on the gathered dense cache: the sequences' keys back to back, a cu_seqlens_k built from the lengths."""
    import torch

    kn, cu_k = vp.pack_rows(ks, tail=1)  # (one spare token: the call wants total_k >= 1 even if no sequence has keys)
    vn, _ = vp.pack_rows(vs, tail=1)
    max_k = max(max(k.shape[1] for k in ks), 1)
    o, lse = fa.flash_attention_varlen(q, to_dev(kn, dtype), to_dev(vn, dtype), i32(cu_q), i32(cu_k), int(max_q), max_k, is_causal=causal,
                                       scale=scale)
    torch.cuda.synchronize()
    return o, lse


def oracle_seq(oracle, q, k, v, causal, dtype):
    """fp64 (O [Hq, Lq, D], LSE [Hq, Lq]) of one sequence on the pre-scaled operand; rows without a visible key: 0 and -inf."""
    Hq, Lq, D = q.shape
    L = k.shape[1]
    k, v = np.ascontiguousarray(k), np.ascontiguousarray(v)
    o, lse = np.zeros((Hq, Lq, D)), np.full((Hq, Lq), -np.inf)
    dead = vp.dead_rows(Lq, L, causal)
    if dead < Lq:  # rows dead .. Lq-1 against all keys (under the mask: the bottom-right aligned problem of those rows)
        qs = np.ascontiguousarray(q[:, dead:])
        o64, l64 = oracle.attn_fwd_ex_f64(effective_q(oracle, qs, dtype)[None], k[None], v[None], causal, LN2)
        o[:, dead:], lse[:, dead:] = o64[0], l64[0]
    return o, lse


def piece(o, lse, cu_q, b):
    s, e = int(cu_q[b]), int(cu_q[b + 1])
    return o[s:e].transpose(0, 1), lse[:, s:e]


_DATA, _RUNS, _DENSE, _ORACLE = {}, {}, {}, {}


def data(oracle, dtype, D, heads):
    """The base batch for one (dtype, head_dim, heads): numpy sequences and the packed q on the device. Drawn once."""
    key = (dtype, D, heads)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * D + 10 * heads[0] + heads[1] + (1 if dtype == "f16" else 0))
        seqs = vp.draw_seqs(oracle.round_to, rng, heads[0], heads[1], D, dtype, vp.BASE)
        qn, cu_q = vp.pack_rows([s[0] for s in seqs])
        _DATA[key] = (seqs, to_dev(qn, dtype), cu_q)
    return _DATA[key]


def storage_order(P, layout):
    return "table" if (P == 256 and layout == "NHD") else "random"


def run(fa, oracle, dtype, D, heads, P, layout, causal):
    """The base batch through the paged call under one storage. Cached: parity, identity and the storage comparison share the runs."""
    key = (dtype, D, heads, P, layout, causal)
    if key not in _RUNS:
        seqs, q, cu_q = data(oracle, dtype, D, heads)
        order = storage_order(P, layout)
        pool = vp.build_pool([s[1] for s in seqs], [s[2] for s in seqs], P, rng=np.random.default_rng(P + D) if order == "random" else None, spare=3)
        kp, vpool = to_layout(pool["k"], dtype, layout), to_layout(pool["v"], dtype, layout)
        _RUNS[key] = paged(fa, q, kp, vpool, cu_q, pool["table"], [L for _, L in vp.BASE], max(lq for lq, _ in vp.BASE), causal, layout)
    return _RUNS[key]


def dense(fa, oracle, dtype, D, heads, causal):
    key = (dtype, D, heads, causal)
    if key not in _DENSE:
        seqs, q, cu_q = data(oracle, dtype, D, heads)
        _DENSE[key] = dense_varlen(fa, q, [s[1] for s in seqs], [s[2] for s in seqs], cu_q, max(lq for lq, _ in vp.BASE), causal, dtype)
    return _DENSE[key]


def reference(oracle, dtype, D, heads, causal):
    key = (dtype, D, heads, causal)
    if key not in _ORACLE:
        seqs, _, _ = data(oracle, dtype, D, heads)
        _ORACLE[key] = [oracle_seq(oracle, *s, causal, dtype) for s in seqs]
    return _ORACLE[key]


MATRIX = [(t, d, p, lay, c) for t in ("f16", "bf16") for d in (64, 128) for p in vp.PAGE_SIZES for lay in ("HND", "NHD") for c in (True, False)]


# ---- 1. oracle parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,P,layout,causal", MATRIX)
def test_oracle_parity_per_sequence(fa, oracle_mod, dtype, D, P, layout, causal):
    for heads in vp.HEADS:
        seqs, _, cu_q = data(oracle_mod, dtype, D, heads)
        o, lse = run(fa, oracle_mod, dtype, D, heads, P, layout, causal)
        refs = reference(oracle_mod, dtype, D, heads, causal)
        for b, (Lq, L) in enumerate(vp.BASE):
            if Lq == 0:
                continue
            ob, lb = piece(o, lse, cu_q, b)
            on, ln = ob.float().cpu().numpy(), lb.cpu().numpy()
            o64, l64 = refs[b]
            dead = vp.dead_rows(Lq, L, causal)
            assert np.array_equal(on[:, :dead], np.zeros_like(on[:, :dead])) and np.isneginf(ln[:, :dead]).all(), (heads, b, "rows without a key")
            if dead == Lq:
                continue
            assert np.isfinite(on).all() and np.isfinite(ln[:, dead:]).all(), (heads, b)
            err_o, err_l = np.abs(on - o64).max(), np.abs(ln[:, dead:] - l64[:, dead:]).max()
            tol_l = lse_tol(dtype, 1, seqs[b][0][:, dead:], seqs[b][1])
            print(f"VARLEN-PAGED parity {dtype} D={D} P={P} {layout} causal={causal} Hq/Hkv={heads} seq {b} {(Lq, L)}: O {err_o:.2e} "
                  f"(bar {TOL_O[dtype]:.1e}) LSE {err_l:.2e} (bar {tol_l:.2e})")
            assert err_o < TOL_O[dtype], (heads, b, err_o)
            assert err_l < tol_l, (heads, b, err_l)


# ---- 2. bit-identity to fa_fwd_varlen on the gathered dense cache --------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,P,layout,causal", MATRIX)
def test_bit_identical_to_varlen_on_the_gathered_cache(fa, oracle_mod, dtype, D, P, layout, causal):
    import torch

    for heads in vp.HEADS:
        _, _, cu_q = data(oracle_mod, dtype, D, heads)
        o, lse = run(fa, oracle_mod, dtype, D, heads, P, layout, causal)
        od, ld = dense(fa, oracle_mod, dtype, D, heads, causal)
        claimed = 0
        for b, (Lq, L) in enumerate(vp.BASE):
            if not vp.identity_claimed(Lq, L, causal):
                continue
            claimed += 1
            (ob, lb), (odb, ldb) = piece(o, lse, cu_q, b), piece(od, ld, cu_q, b)
            assert torch.equal(ob.view(torch.int16), odb.view(torch.int16)), (heads, b, "O differs from fa_fwd_varlen on the gathered cache")
            assert torch.equal(lb.view(torch.int32), ldb.view(torch.int32)), (heads, b, "LSE differs from fa_fwd_varlen on the gathered cache")
        assert claimed == (6 if causal else 7)


# ---- 3. bit-identity across storage --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,causal", [(t, d, c) for t in ("f16", "bf16") for d in (64, 128) for c in (True, False)])
def test_bit_identical_across_storage(fa, oracle_mod, dtype, D, causal):
    import torch

    assert storage_order(16, "HND") == "random" and storage_order(256, "NHD") == "table"
    for heads in vp.HEADS:
        _, _, cu_q = data(oracle_mod, dtype, D, heads)
        a = run(fa, oracle_mod, dtype, D, heads, 16, "HND", causal)
        b = run(fa, oracle_mod, dtype, D, heads, 256, "NHD", causal)
        n = int(cu_q[-1])  # every row, the rows without a visible key included
        assert torch.equal(a[0][:n].view(torch.int16), b[0][:n].view(torch.int16)), heads
        assert torch.equal(a[1][:, :n].view(torch.int32), b[1][:, :n].view(torch.int32)), heads
    # and reproducible: the same call again gives the same bits
    seqs, q, cu_q = data(oracle_mod, dtype, D, (8, 2))
    pool = vp.build_pool([s[1] for s in seqs], [s[2] for s in seqs], 16, rng=np.random.default_rng(16 + D), spare=3)
    again = paged(fa, q, to_layout(pool["k"], dtype, "HND"), to_layout(pool["v"], dtype, "HND"), cu_q, pool["table"], [L for _, L in vp.BASE],
                  130, causal, "HND")
    first = run(fa, oracle_mod, dtype, D, (8, 2), 16, "HND", causal)
    assert torch.equal(again[0].view(torch.int16), first[0].view(torch.int16)) and torch.equal(again[1].view(torch.int32), first[1].view(torch.int32))


# ---- 4. unused storage has no influence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,P,layout", [("bf16", 64, 16, "HND"), ("f16", 128, 16, "NHD"), ("bf16", 128, 64, "HND"), ("f16", 64, 256, "NHD")])
def test_unused_storage_has_no_influence(fa, oracle_mod, dtype, D, P, layout):
    import torch

    heads = (8, 2)
    seqs, q, cu_q = data(oracle_mod, dtype, D, heads)
    ks, vs, lens = [s[1] for s in seqs], [s[2] for s in seqs], [L for _, L in vp.BASE]
    mp = vp.pages_of(1024, P) + 2  # two entries past the longest sequence's last page too

    def go(causal, **kw):
        pool = vp.build_pool(ks, vs, P, rng=np.random.default_rng(5), spare=3, max_pages=mp, **kw)
        return paged(fa, q, to_layout(pool["k"], dtype, layout), to_layout(pool["v"], dtype, layout), cu_q, pool["table"], lens, 130, causal, layout)

    for causal in (True, False):
        clean = go(causal, fill=0.0, unused="zero")
        for how in ("spare", "minus1", "beyond"):  # NaN in slots >= L_b and in the spare pages; entries past ceil(L_b / P) of each kind
            dirty = go(causal, fill=np.nan, unused=how)
            assert torch.equal(dirty[0].view(torch.int16), clean[0].view(torch.int16)), (causal, how, "O")
            assert torch.equal(dirty[1].view(torch.int32), clean[1].view(torch.int32)), (causal, how, "LSE")


@pytest.mark.parametrize("dtype,D,causal", [("bf16", 64, False), ("f16", 128, True), ("bf16", 128, False), ("f16", 64, True)])
def test_an_out_of_range_page_inside_the_used_range_reads_as_zeros(fa, oracle_mod, dtype, D, causal):
    # a known answer: V is all ones except on the page the table misnames, whose keys and values read as zeros, so every element of a
    # row of O equals the softmax weight that is NOT on that page (its keys score 0)
    Hq, Hkv, Lq, L, P = 4, 2, 40, 100, 16
    rng = np.random.default_rng(D + causal)
    q = vp.draw(oracle_mod.round_to, rng, dtype, Hq, Lq, D)
    k = vp.draw(oracle_mod.round_to, rng, dtype, Hkv, L, D)
    v = np.ones((Hkv, L, D), np.float32)
    for bad in (-1, None):  # below 0; num_pages
        pool = vp.build_pool([k], [v], P, rng=np.random.default_rng(3), spare=2, fill=np.nan)
        pool["table"][0, 2] = pool["num_pages"] if bad is None else bad  # keys 32 .. 47
        o, lse = paged(fa, to_dev(q.transpose(1, 0, 2), dtype), to_layout(pool["k"], dtype, "HND"), to_layout(pool["v"], dtype, "HND"),
                       [0, Lq], pool["table"], [L], Lq, causal, "HND")
        kz = k.astype(np.float64).copy()
        kz[:, 32:48] = 0.0
        s = np.einsum("hid,hjd->hij", effective_q(oracle_mod, q, dtype).astype(np.float64), np.repeat(kz, Hq // Hkv, axis=0)) * LN2
        if causal:
            i, j = np.arange(Lq)[:, None], np.arange(L)[None, :]
            s = np.where(j <= i + L - Lq, s, -np.inf)
        m = s.max(-1, keepdims=True)
        p = np.exp(s - m)
        want_lse = (m + np.log(p.sum(-1, keepdims=True)))[..., 0]
        p /= p.sum(-1, keepdims=True)
        want = p[:, :, :32].sum(-1) + p[:, :, 48:].sum(-1)
        on, ln = o.transpose(0, 1).float().cpu().numpy(), lse.cpu().numpy()
        assert np.abs(on - want[..., None]).max() < TOL_O[dtype], (bad, np.abs(on - want[..., None]).max())
        assert np.abs(ln - want_lse).max() < lse_tol(dtype, 1, q, k), bad
        assert want.max() < 0.95  # the zero page carries real weight: the answer is not the trivial 1


# ---- 5. write footprint ----------------------------------------------------------------------------------------------------------
CANARY16 = {"bf16": 0x7FC1, "f16": 0x7E01}  # NaNs with a payload (positive as int16)
CANARY32 = 0x7FC00001


def _owners(cu, total, max_q):
    """(first token, rows) per sequence under the documented clamps."""
    out = []
    for b in range(len(cu) - 1):
        s, e = min(max(int(cu[b]), 0), total), min(max(int(cu[b + 1]), 0), total)
        out.append((s, min(max(e - s, 0), max_q)))
    return out


@pytest.mark.parametrize("dtype,D,causal", [("bf16", 64, True), ("f16", 128, True), ("bf16", 128, False), ("f16", 64, False)])
@pytest.mark.parametrize("table", ["unowned tail and a clamped sequence", "negative and above total", "decreasing"])
def test_write_footprint(fa, oracle_mod, dtype, D, causal, table):
    import torch

    Hq, Hkv, P, total_q = 4, 2, 16, 487
    cu, max_q = {"unowned tail and a clamped sequence": ([0, 100, 400, 450], 200),  # 37 tokens behind cu[B]; 300 rows clamped to 200
                 "negative and above total": ([-7, 100, 400, 10000], 300),
                 "decreasing": ([200, 100, 300, 487], 300)}[table]
    lens_k = [150, 350, 33]
    rng = np.random.default_rng(len(table) + D)
    qn = vp.draw(oracle_mod.round_to, rng, dtype, total_q, Hq, D)
    ks = [vp.draw(oracle_mod.round_to, rng, dtype, Hkv, L, D) for L in lens_k]
    vs = [vp.draw(oracle_mod.round_to, rng, dtype, Hkv, L, D) for L in lens_k]
    pool = vp.build_pool(ks, vs, P, rng=rng, spare=2)
    kp, vpool = to_layout(pool["k"], dtype, "HND"), to_layout(pool["v"], dtype, "HND")
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    # q and o: [total, H, D] views with a spare head per row (row gap) and a head pitch of 2 D (head gap), canaries in the gaps
    qbuf = torch.full((total_q + 3, Hq + 1, 2 * D), CANARY16[dtype], dtype=torch.int16, device="cuda").view(tdt)
    q = qbuf[:total_q, :Hq, :D]
    q.copy_(to_dev(qn, dtype))
    obuf = torch.full((total_q + 3, Hq + 1, 2 * D), CANARY16[dtype], dtype=torch.int16, device="cuda")
    o = obuf.view(tdt)[:total_q, :Hq, :D]
    lbuf = torch.full((Hq * total_q + 64,), CANARY32, dtype=torch.int32, device="cuda")
    lse = lbuf.view(torch.float32)[32:32 + Hq * total_q].view(Hq, total_q)
    paged(fa, q, kp, vpool, cu, pool["table"], lens_k, max_q, causal, "HND", out=o, lse=lse)
    owners = _owners(cu, total_q, max_q)
    written_o = torch.zeros_like(obuf, dtype=torch.bool)
    written_l = torch.zeros_like(lbuf, dtype=torch.bool)
    for s, n in owners:
        written_o[s:s + n, :Hq, :D] = True
        written_l[32:32 + Hq * total_q].view(Hq, total_q)[:, s:s + n] = True
    assert int(written_o.sum()) == sum(n for _, n in owners) * Hq * D  # the owners do not overlap: the inputs are ones the contract calls safe
    assert bool((obuf[~written_o] == CANARY16[dtype]).all()), "O was written outside the specified rows"
    assert bool((lbuf[~written_l] == CANARY32).all()), "LSE was written outside the specified rows"
    # what was written: the bits of a plain call whose clean table says what the clamps make of this one
    keep = [(s, n, b) for b, (s, n) in enumerate(owners) if n > 0]
    q2 = to_dev(np.concatenate([qn[s:s + n] for s, n, _ in keep]), dtype)
    cu2 = np.cumsum([0] + [n for _, n, _ in keep])
    o2, l2 = paged(fa, q2, kp, vpool, cu2, pool["table"][[b for _, _, b in keep]], [lens_k[b] for _, _, b in keep], max_q, causal, "HND")
    for i, (s, n, b) in enumerate(keep):
        assert torch.equal(o[s:s + n].view(torch.int16), o2[cu2[i]:cu2[i + 1]].view(torch.int16)), (b, "O")
        assert torch.equal(lse[:, s:s + n].view(torch.int32), l2[:, cu2[i]:cu2[i + 1]].view(torch.int32)), (b, "LSE")
        assert not bool((o[s:s + n].view(torch.int16) == CANARY16[dtype]).any()), (b, "a specified row was not written")


# ---- 6. chunked prefill ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128), ("bf16", 128), ("f16", 64)])
def test_chunked_prefill_matches_one_call_on_the_full_cache(fa, oracle_mod, dtype, D):
    import torch

    Hq, Hkv, P, N, CH = 8, 2, 16, 300, 48
    rng = np.random.default_rng(60 + D)
    q = vp.draw(oracle_mod.round_to, rng, dtype, Hq, N + 1, D)   # one more token: the decode step at the end
    k = vp.draw(oracle_mod.round_to, rng, dtype, Hkv, N + 1, D)
    v = vp.draw(oracle_mod.round_to, rng, dtype, Hkv, N + 1, D)
    qd, kd, vd = (to_dev(x.transpose(1, 0, 2), dtype) for x in (q, k, v))  # [N + 1, H, D]
    # one causal call on the full cache
    full = vp.build_pool([k[:, :N]], [v[:, :N]], P, rng=np.random.default_rng(1), spare=2)
    o_full, l_full = paged(fa, qd[:N], to_layout(full["k"], dtype, "HND"), to_layout(full["v"], dtype, "HND"), [0, N], full["table"], [N], N,
                           True, "HND")
    # the same prompt 48 tokens at a time into an empty pool: append, then a causal call, seqlens_k advanced in place
    mp = vp.pages_of(N + 1, P)
    table = i32(np.random.default_rng(2).permutation(mp + 3)[:mp][None])
    kp = torch.full((mp + 3, Hkv, P, D), float("nan"), dtype=qd.dtype, device="cuda")
    vpool = torch.full_like(kp, float("nan"))
    sl = i32([0])
    o_ch = torch.empty_like(o_full)
    l_ch = torch.empty_like(l_full)
    for s, n in vp.chunks(N, CH):
        sl.fill_(s + n)
        cu = i32([0, n])
        fa.kv_append_paged(kd[s:s + n], vd[s:s + n], kp, vpool, cu, table, sl, n)
        oc, lc = fa.flash_attention_varlen_paged(qd[s:s + n], kp, vpool, cu, table, sl, n, is_causal=True)
        o_ch[s:s + n], l_ch[:, s:s + n] = oc, lc
    torch.cuda.synchronize()
    tol_l = lse_tol(dtype, 1, q, k)
    err_o = float((o_ch.float() - o_full.float()).abs().max())
    err_l = float((l_ch - l_full).abs().max())
    print(f"VARLEN-PAGED chunked {dtype} D={D}: O {err_o:.2e} (bar {2 * TOL_O[dtype]:.1e}) LSE {err_l:.2e} (bar {2 * tol_l:.2e})")
    assert err_o < 2 * TOL_O[dtype] and err_l < 2 * tol_l
    # both sides are within one bar of the oracle
    o64, l64 = oracle_seq(oracle_mod, q[:, :N], k[:, :N], v[:, :N], True, dtype)
    for o, lse in ((o_full, l_full), (o_ch, l_ch)):
        assert np.abs(o.transpose(0, 1).float().cpu().numpy() - o64).max() < TOL_O[dtype] and np.abs(lse.cpu().numpy() - l64).max() < tol_l
    # a last chunk of one token: the 128-row kernel against the paged decode
    sl.fill_(N + 1)
    cu = i32([0, 1])
    fa.kv_append_paged(kd[N:], vd[N:], kp, vpool, cu, table, sl, 1)
    o1, l1 = fa.flash_attention_varlen_paged(qd[N:], kp, vpool, cu, table, sl, 1, is_causal=True)
    od, ld = fa.flash_attention_decode_paged(qd[N:].view(1, Hq, 1, D), kp, vpool, table, sl, is_causal=True)
    torch.cuda.synchronize()
    assert float((o1.transpose(0, 1).float() - od[0].float()).abs().max()) < 2 * TOL_O[dtype]
    assert float((l1 - ld[0]).abs().max()) < 2 * tol_l
    o64, l64 = oracle_seq(oracle_mod, q[:, N:], k, v, True, dtype)
    assert np.abs(o1.transpose(0, 1).float().cpu().numpy() - o64).max() < TOL_O[dtype] and np.abs(l1.cpu().numpy() - l64).max() < tol_l


# ---- 7. append -------------------------------------------------------------------------------------------------------------------
def _torch_dtype(dtype):
    import torch

    return {"f16": torch.float16, "bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn}[dtype]


@pytest.mark.parametrize("P", [16, 256])
@pytest.mark.parametrize("layout", ["HND", "NHD"])
@pytest.mark.parametrize("dtype", ["f16", "bf16", "fp8"])
def test_append_writes_the_named_slots_and_nothing_else(fa, dtype, layout, P):
    import torch

    Hkv, D, mp = 2, 64, 3
    cap, esz = mp * P, (1 if dtype == "fp8" else 2)
    # (n_b, length after the append): into an empty cache; across a page edge; nothing new; positions below 0; positions at and above the
    # capacity; onto a table entry outside the pool (both kinds)
    seqs = [(5, 5), (20, 37), (0, 9), (7, 3), (6, cap + 2), (10, P + 5), (4, P + 2)]
    B = len(seqs)
    num_pages = B * mp + 2
    rng = np.random.default_rng(P + esz)
    table = rng.permutation(num_pages)[:B * mp].reshape(B, mp).astype(np.int32)
    table[5, 1], table[6, 1] = -1, num_pages
    total = sum(n for n, _ in seqs)
    cu = np.cumsum([0] + [n for n, _ in seqs])
    # byte images: new rows under wide strides ([total + 2, Hkv + 1, D] storage), pools with a row pitch of 2 D elements
    new_k = rng.integers(0, 120, (total + 2, Hkv + 1, D * esz), dtype=np.uint8)
    new_v = rng.integers(0, 120, (total + 2, Hkv + 1, D * esz), dtype=np.uint8)
    shape = (num_pages, Hkv, P, 2 * D * esz) if layout == "HND" else (num_pages, P, Hkv, 2 * D * esz)
    want_k, want_v = np.full(shape, 0xA5, np.uint8), np.full(shape, 0x5A, np.uint8)
    kinds = dict(written=0, below=0, above=0, bad_page=0)
    for b, (n, L) in enumerate(seqs):
        for i, pos in enumerate(vp.append_positions(n, L, cap)):
            if pos is None:
                kinds["below" if L - n + i < 0 else "above"] += 1
                continue
            pg = int(table[b, pos // P])
            if not 0 <= pg < num_pages:
                kinds["bad_page"] += 1
                continue
            kinds["written"] += 1
            for h in range(Hkv):
                idx = (pg, h, pos % P) if layout == "HND" else (pg, pos % P, h)
                want_k[idx][:D * esz] = new_k[cu[b] + i, h]
                want_v[idx][:D * esz] = new_v[cu[b] + i, h]
    assert kinds["below"] == 4 and kinds["above"] == 2 and kinds["bad_page"] > 0 and kinds["written"] > 30, kinds
    tdt = _torch_dtype(dtype)
    kp = torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")
    vpool = torch.full(shape, 0x5A, dtype=torch.uint8, device="cuda")
    nk, nv = torch.from_numpy(new_k).cuda(), torch.from_numpy(new_v).cuda()
    fa.kv_append_paged(nk.view(tdt)[:total, :Hkv], nv.view(tdt)[:total, :Hkv], kp.view(tdt)[..., :D], vpool.view(tdt)[..., :D], i32(cu),
                       i32(table), i32([L for _, L in seqs]), 20, layout=layout)
    torch.cuda.synchronize()
    assert np.array_equal(kp.cpu().numpy(), want_k), "K pool: a named slot does not hold the new bytes, or another byte changed"
    assert np.array_equal(vpool.cpu().numpy(), want_v), "V pool: a named slot does not hold the new bytes, or another byte changed"


def test_append_stops_a_sequence_at_max_seqlen_new(fa):
    """n_b is clamped to max_seqlen_new: a sequence that owns more tokens than that appends its first max_seqlen_new ones, at the positions
    the clamped count gives (seqlens_k[b] - max_seqlen_new + i), and its tail is written nowhere."""
    import torch

    Hkv, D, P, mp, max_new = 2, 64, 16, 3, 8
    seqs = [(5, 5), (12, 30), (3, 10)]  # (tokens owned, length after the append): the second owns 12 > max_seqlen_new
    B = len(seqs)
    num_pages = B * mp + 1
    rng = np.random.default_rng(812)
    table = rng.permutation(num_pages)[:B * mp].reshape(B, mp).astype(np.int32)
    total = sum(n for n, _ in seqs)
    cu = np.cumsum([0] + [n for n, _ in seqs])
    new_k = rng.integers(0, 120, (total, Hkv, D * 2), dtype=np.uint8)
    new_v = rng.integers(0, 120, (total, Hkv, D * 2), dtype=np.uint8)
    shape = (num_pages, Hkv, P, D * 2)
    want_k, want_v = np.full(shape, 0xA5, np.uint8), np.full(shape, 0x5A, np.uint8)
    written = 0
    for b, (owned, L) in enumerate(seqs):
        n = min(owned, max_new)
        assert (n < owned) == (b == 1)
        for i, pos in enumerate(vp.append_positions(n, L, mp * P)):
            want_k[table[b, pos // P], :, pos % P] = new_k[cu[b] + i]
            want_v[table[b, pos // P], :, pos % P] = new_v[cu[b] + i]
            written += 1
    assert written == 5 + 8 + 3
    kp = torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")
    vpool = torch.full(shape, 0x5A, dtype=torch.uint8, device="cuda")
    nk, nv = torch.from_numpy(new_k).cuda(), torch.from_numpy(new_v).cuda()
    fa.kv_append_paged(nk.view(torch.float16), nv.view(torch.float16), kp.view(torch.float16), vpool.view(torch.float16), i32(cu), i32(table),
                       i32([L for _, L in seqs]), max_new)
    torch.cuda.synchronize()
    assert np.array_equal(kp.cpu().numpy(), want_k), "K pool: the tail past max_seqlen_new was written, or the first rows sit elsewhere"
    assert np.array_equal(vpool.cpu().numpy(), want_v), "V pool: the tail past max_seqlen_new was written, or the first rows sit elsewhere"


@pytest.mark.parametrize("dtype,D,P,layout", [("bf16", 64, 16, "HND"), ("f16", 128, 16, "NHD"), ("bf16", 128, 256, "NHD"), ("f16", 64, 256, "HND")])
def test_attention_after_the_append_is_bit_identical_to_varlen_on_the_concatenated_cache(fa, oracle_mod, dtype, D, P, layout):
    import torch

    Hq, Hkv = 8, 2
    lens = [(5, 5), (20, 37), (48, 300), (1, 129), (130, 130)]  # (new tokens = queries, length after the append)
    rng = np.random.default_rng(70 + D + P)
    seqs = vp.draw_seqs(oracle_mod.round_to, rng, Hq, Hkv, D, dtype, lens)
    ks, vs = [s[1] for s in seqs], [s[2] for s in seqs]
    # the pool holds each sequence's prefix; its pages are allotted for the length after the append
    pool = vp.build_pool(ks, vs, P, rng=rng, spare=2)
    for b, (n, L) in enumerate(lens):
        for j in range(L - n, L):
            pool["k"][pool["table"][b, j // P], :, j % P] = np.nan
            pool["v"][pool["table"][b, j // P], :, j % P] = np.nan
    kp, vpool = to_layout(pool["k"], dtype, layout), to_layout(pool["v"], dtype, layout)
    kn, cu = vp.pack_rows([k[:, L - n:] for k, (n, L) in zip(ks, lens)])
    vn, _ = vp.pack_rows([v[:, L - n:] for v, (n, L) in zip(vs, lens)])
    qn, cu_q = vp.pack_rows([s[0] for s in seqs])
    assert list(cu) == list(cu_q)
    q, sl, bt, cud = to_dev(qn, dtype), i32([L for _, L in lens]), i32(pool["table"]), i32(cu)
    fa.kv_append_paged(to_dev(kn, dtype), to_dev(vn, dtype), kp, vpool, cud, bt, sl, 130, layout=layout)
    o, lse = fa.flash_attention_varlen_paged(q, kp, vpool, cud, bt, sl, 130, is_causal=True, layout=layout)
    torch.cuda.synchronize()
    od, ld = dense_varlen(fa, q, ks, vs, cu_q, 130, True, dtype)
    assert torch.equal(o.view(torch.int16), od.view(torch.int16)) and torch.equal(lse.view(torch.int32), ld.view(torch.int32))


# ---- 8. exact arithmetic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,Lq,Lk", [("A", 64, 130), ("B", 130, 257)])
@pytest.mark.parametrize("dtype,D,causal", [(t, d, c) for t in ("f16", "bf16") for d in (64, 128) for c in (False, True)])
def test_exact_arithmetic_inputs_in_pages(fa, dtype, D, causal, family, Lq, Lk):
    Hq, Hkv, P, kexp = 4, 2, 16, (0 if D == 64 else -1)
    case = ef.build(family, 1, Hq, Hkv, Lq, Lk, D, dtype, causal, kexp=kexp, span=ef.span_for(dtype, False, Lk) if family == "A" else 3,
                    seed=17 + D + (1 if causal else 0))
    assert ef.representable(case.q, dtype) and ef.representable(case.k, dtype) and ef.representable(case.v, dtype)
    pool = vp.build_pool([case.k[0]], [case.v[0]], P, rng=np.random.default_rng(D), spare=2)
    o, lse = paged(fa, to_dev(case.q[0].transpose(1, 0, 2), dtype), to_layout(pool["k"], dtype, "HND"), to_layout(pool["v"], dtype, "HND"),
                   [0, Lq], pool["table"], [Lk], Lq, causal, "HND", scale=case.scale)
    ob, lb = o.transpose(0, 1), lse
    worst = dict(o=0.0, lse=0.0)
    for h in range(Hq):
        ref = ef.reference_head(case, 0, h)
        r = ef.ratios(case, ref, ob[h].float().cpu().numpy(), lb[h].cpu().numpy(), 0, 0.0)
        assert r["o"] <= 1.0 and r["lse"] <= 1.0, (dtype, D, causal, family, h, r)
        assert family == "B" or r["proven"] == 1.0, (h, "a family-A row is not proven exact: bar A would not apply")
        worst = dict(o=max(worst["o"], r["o"]), lse=max(worst["lse"], r["lse"]))
    print(f"EXACT fa_fwd_varlen_paged {dtype} {family} D={D} causal={causal}: O {worst['o']:.3f} LSE {worst['lse']:.3f} of bar")


# ---- 9. graph capture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_graph_replay_after_the_tables_change(fa, oracle_mod, dtype, D):
    import torch

    Hq, Hkv, P, mp, B, total, max_q = 8, 2, 16, 30, 3, 400, 200
    rng = np.random.default_rng(90 + D)
    q = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, total, Hq, D), dtype)
    kn = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, total, Hkv, D), dtype)
    vn = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, total, Hkv, D), dtype)
    num_pages = B * mp + 4
    init_k = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, num_pages, Hkv, P, D), dtype)  # every slot holds a finite value: any prefix is a cache
    init_v = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, num_pages, Hkv, P, D), dtype)
    steps = [  # (cu of the chunk = queries and new rows, block table, lengths after the append)
        ([0, 100, 250, 400], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [100, 400, 151]),
        ([0, 200, 200, 330], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [480, 77, 130]),   # a sequence without a chunk; 70 tokens nobody owns
        ([0, 1, 2, 3], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [1, 300, 17]),            # a decode-like step
    ]
    cu, bt, sl = i32(steps[0][0]), i32(steps[0][1]), i32(steps[0][2])
    kp, vpool = init_k.clone(), init_v.clone()
    o = torch.empty_like(q)
    lse = torch.empty(Hq, total, dtype=torch.float32, device="cuda")

    def step(kp_, vp_, o_, lse_):
        fa.kv_append_paged(kn, vn, kp_, vp_, cu, bt, sl, max_q)
        fa.flash_attention_varlen_paged(q, kp_, vp_, cu, bt, sl, max_q, is_causal=True, out=o_, lse=lse_)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(kp, vpool, o, lse)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(kp, vpool, o, lse)
    for c, t, l in (steps[1], steps[0], steps[2], steps[1]):
        cu.copy_(i32(c))
        bt.copy_(i32(t))
        sl.copy_(i32(l))
        kp.copy_(init_k)
        vpool.copy_(init_v)
        o.fill_(float("nan"))
        lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        k2, v2 = init_k.clone(), init_v.clone()
        o2 = torch.full_like(o, float("nan"))
        l2 = torch.full_like(lse, float("nan"))
        step(k2, v2, o2, l2)
        torch.cuda.synchronize()
        assert torch.equal(kp.view(torch.int16), k2.view(torch.int16)) and torch.equal(vpool.view(torch.int16), v2.view(torch.int16)), (c, "pools")
        assert torch.equal(o.view(torch.int16), o2.view(torch.int16)) and torch.equal(lse.view(torch.int32), l2.view(torch.int32)), (c, "O / LSE")
        n = c[-1]
        assert bool(torch.isfinite(o[:n].float()).all()) and bool(torch.isnan(o[n:].float()).all()), (c, "owned tokens written, the others not")
        assert not bool(torch.equal(kp.view(torch.int16), init_k.view(torch.int16))), (c, "the append wrote nothing")


# ---- 10. a pool above 4 GiB ------------------------------------------------------------------------------------------------------
def test_pool_above_4_gib(fa, oracle_mod):
    """A bf16 pool of 4.5 GiB with every used page past byte offset 2^32 gives the bits the same data gives in low pages."""
    import torch

    Hq, Hkv, D, P = 16, 8, 128, 256
    page_bytes = Hkv * P * D * 2
    num_pages = (9 << 29) // page_bytes  # 4.5 GiB
    lens = [(130, 700), (40, 300)]
    rng = np.random.default_rng(11)
    seqs = vp.draw_seqs(oracle_mod.round_to, rng, Hq, Hkv, D, "bf16", lens)
    pool = vp.build_pool([s[1] for s in seqs], [s[2] for s in seqs], P, rng=rng, spare=1, fill=0.0)
    used = pool["num_pages"]
    first_hi = (1 << 32) // page_bytes + 3
    assert first_hi + used <= num_pages
    qn, cu_q = vp.pack_rows([s[0] for s in seqs])
    q = to_dev(qn, "bf16")
    lo_k, lo_v = to_layout(pool["k"], "bf16", "HND"), to_layout(pool["v"], "bf16", "HND")
    o_lo, l_lo = paged(fa, q, lo_k, lo_v, cu_q, pool["table"], [L for _, L in lens], 130, True, "HND")
    try:
        kp = torch.empty(num_pages, Hkv, P, D, dtype=torch.bfloat16, device="cuda")
        vpool = torch.empty_like(kp)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no room for two pools of 4.5 GiB on this device")
    kp[first_hi:first_hi + used] = lo_k
    vpool[first_hi:first_hi + used] = lo_v
    o_hi, l_hi = paged(fa, q, kp, vpool, cu_q, pool["table"] + first_hi, [L for _, L in lens], 130, True, "HND")
    assert torch.equal(o_hi.view(torch.int16), o_lo.view(torch.int16)) and torch.equal(l_hi.view(torch.int32), l_lo.view(torch.int32))
    del kp, vpool
    torch.cuda.empty_cache()
    for b, s in enumerate(seqs):
        o64, l64 = oracle_seq(oracle_mod, *s, True, "bf16")
        ob, lb = piece(o_lo, l_lo, cu_q, b)
        assert np.abs(ob.float().cpu().numpy() - o64).max() < TOL_O["bf16"] and np.abs(lb.cpu().numpy() - l64).max() < lse_tol("bf16", 1, s[0], s[1])


# ---- 11. return_lse=False ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,causal", [("bf16", 64, True), ("f16", 128, False)])
def test_without_an_lse_the_output_keeps_its_bits(fa, oracle_mod, dtype, D, causal):
    import torch

    heads = (8, 2)
    seqs, q, cu_q = data(oracle_mod, dtype, D, heads)
    pool = vp.build_pool([s[1] for s in seqs], [s[2] for s in seqs], 16, rng=np.random.default_rng(16 + D), spare=3)
    o, lse = paged(fa, q, to_layout(pool["k"], dtype, "HND"), to_layout(pool["v"], dtype, "HND"), cu_q, pool["table"], [L for _, L in vp.BASE], 130,
                   causal, "HND", return_lse=False)
    assert lse is None
    with_lse = run(fa, oracle_mod, dtype, D, heads, 16, "HND", causal)
    assert torch.equal(o.view(torch.int16), with_lse[0].view(torch.int16))
