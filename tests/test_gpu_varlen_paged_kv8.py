"""GPU: fa_fwd_varlen_paged_kv8 (bf16 queries on e4m3 page pools: flash_attention_varlen_paged with float8_e4m3fn pools) and
fa_kv_append_paged_quant (kv_append_paged with 16-bit new rows into e4m3 pools). Helpers and references live in tests/kv8.py (held to the
header's words by tests/test_kv8_cases.py on the CPU). The inputs: window.SEQS as one packed batch with three trailing tokens nobody owns
(dead rows, Lk = 0, Lq > Lk, a sequence of 1000 keys), K / V drawn on the e4m3 grid so both pools are exact, pools of P = 16 HND with
shuffled pages and P = 256 NHD, NaN bytes (0x7F / 0xFF) in every slot nobody may read and one table entry outside the pool past each
sequence's last page.
  1. O and LSE bit for bit those of the bf16 call on the widened twin pool, seven windows, without sinks and with; unowned tokens keep a
     sentinel;
  2. parity with the fp64 reference at util.o_tol / lse_tol (with sinks: sink.py's bars) under (200, 0) and (127, 5), both pools;
  3. q as a view of a packed projection, pool strides padded by 16 elements, lse = None;
  4. the quantising append byte for byte over all 65536 patterns of bf16 and of f16, and nothing else written;
  5. append-quant + causal KV8 prefill in two chunks against one call on the full prompt; the last token against the paged decode;
  6. the append-quant + prefill pair in one captured graph, replayed after tables, sinks and new rows changed in place;
  7. the dtype errors of the wrapper.

Worst error / bar measured on an MI355X (printed by test 2): O 0.17, LSE 0.20."""
import numpy as np
import pytest

import kv8
import sink as sk
import varlen_paged as vp
import window as wn
from util import TOL_LSE, TOL_O, lse_tol, o_tol

pytestmark = pytest.mark.gpu
INT_MAX = wn.INT_MAX
MAX_Q = max(lq for lq, _ in wn.SEQS)
CONFIGS = [(64, (4, 4), 16, "HND"), (64, (4, 4), 256, "NHD"), (128, (8, 2), 16, "HND"), (128, (8, 2), 256, "NHD")]
WINDOWS = ((-1, -1), (-1, 0), (15, 0), (63, 0), (64, 64), (127, 5), (200, 0))
SO, SL = -3.0e4, 12345.0  # no output is near them: |O| <= 1, |LSE| < 100, -inf or a sink


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


def i32(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()


def bits(t):
    import torch

    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    import torch

    return torch.equal(bits(a[0]), bits(b[0])) and (a[1] is None or torch.equal(bits(a[1]), bits(b[1])))


def laid(x, layout):
    return np.ascontiguousarray(x if layout == "HND" else x.transpose(0, 2, 1, 3))


_DATA, _REF = {}, {}


def data(oracle, D, heads, P, layout):
    """One batch, drawn once per key: numpy sequences, packed bf16 q on the device, the e4m3 pool pair and its bf16 twin."""
    import torch

    key = (D, heads, P, layout)
    if key not in _DATA:
        rng = np.random.default_rng(19000 + D + 10 * heads[0] + heads[1] + P)
        seqs = [(wn.draw(oracle.round_to, rng, "bf16", heads[0], Lq, D), kv8.draw_e4m3(rng, heads[1], Lk, D), kv8.draw_e4m3(rng, heads[1], Lk, D))
                for Lq, Lk in wn.SEQS]
        qn, cu_q = vp.pack_rows([s[0] for s in seqs], tail=3)
        longest = max(vp.pages_of(lk, P) for _, lk in wn.SEQS)
        t = kv8.twin_pools([s[1] for s in seqs], [s[2] for s in seqs], P, np.random.default_rng(P + D), spare=2, max_pages=longest + 1)
        _DATA[key] = dict(
            seqs=seqs, lens=wn.SEQS, cu_q=cu_q, table=t["table"], layout=layout, heads=heads, D=D, P=P,
            q=torch.from_numpy(qn).to(torch.bfloat16).cuda(),
            e4m3=tuple(torch.from_numpy(laid(t[n], layout)).cuda().view(kv8.E4M3) for n in ("k8", "v8")),
            bf16=tuple(torch.from_numpy(laid(t[n], layout)).to(torch.bfloat16).cuda() for n in ("k16", "v16")))
    return _DATA[key]


def refs(d, wl, wr):
    key = (id(d), wl, wr)
    if key not in _REF:
        _REF[key] = [wn.reference(*s, wl, wr) for s in d["seqs"]]
    return _REF[key]


def call(fa, d, kind, window, sinks=None, q=None, pools=None, **kw):
    import torch

    kp, vpool = pools or d[kind]
    r = fa.flash_attention_varlen_paged(d["q"] if q is None else q, kp, vpool, i32(d["cu_q"]), i32(d["table"]), i32([lk for _, lk in d["lens"]]),
                                        MAX_Q, layout=d["layout"], window=window, sinks=sinks, **kw)
    torch.cuda.synchronize()
    return r


def twin_window(wl, wr, sinks):
    """The window under which the bf16 call runs the same kernel family: with sinks the same pair (fa_fwd_varlen_paged_sink always runs the
    window kernels); without, fa_fwd_varlen_paged_window routes by sign, so an unbounded side becomes INT_MAX."""
    return (wl, wr) if sinks is not None else (INT_MAX if wl < 0 else wl, INT_MAX if wr < 0 else wr)


def sentinels(d):
    import torch

    q = d["q"]
    return dict(out=torch.full_like(q, SO), lse=torch.full((d["heads"][0], q.shape[0]), SL, dtype=torch.float32, device="cuda"))


def piece(r, cu_q, b):
    s, e = int(cu_q[b]), int(cu_q[b + 1])
    return r[0][s:e].transpose(0, 1), r[1][:, s:e]


# ---- 1. bit-identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,heads,P,layout", CONFIGS)
def test_bit_identical_to_the_bf16_call_on_the_widened_pool(fa, oracle_mod, D, heads, P, layout):
    import torch

    d = data(oracle_mod, D, heads, P, layout)
    n = int(d["cu_q"][-1])
    blank = sentinels(d)
    for wl, wr in WINDOWS:
        for sinks in (None, dev(sk.sinks_for(heads[0]))):
            a = call(fa, d, "e4m3", (wl, wr), sinks, **sentinels(d))
            b = call(fa, d, "bf16", twin_window(wl, wr, sinks), sinks, **sentinels(d))
            assert same_bits(a, b), ((wl, wr), sinks is not None, "O / LSE differ from the bf16 call on the widened pool")
            # tokens nobody owns keep the sentinel; every owned row of a sequence was written, and holds no NaN from the hidden slots
            assert same_bits((a[0][n:], a[1][:, n:]), (blank["out"][n:], blank["lse"][:, n:])), (wl, wr)
            assert not bool((a[0][:n] == blank["out"][:n]).any()) and not bool((a[1][:, :n] == SL).any()), (wl, wr)
            assert not bool(torch.isnan(a[0][:n].float()).any()) and not bool(torch.isnan(a[1][:, :n]).any()), (wl, wr)
            for s, (Lq, Lk) in enumerate(d["lens"]):  # dead rows: O = 0; LSE = -inf, or sinks[h] bit for bit
                dead = torch.from_numpy(wn.dead_rows(Lq, Lk, wl, wr)).cuda()
                o, l = piece(a, d["cu_q"], s)
                assert not bool(o[:, dead].any()), ((wl, wr), s)
                want = torch.full_like(l, float("-inf")) if sinks is None else sinks[:, None].expand_as(l)
                assert torch.equal(bits(l[:, dead].contiguous()), bits(want[:, dead].contiguous())), ((wl, wr), s)


# ---- 2. parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,heads,P,layout", CONFIGS)
def test_parity_with_the_fp64_reference(fa, oracle_mod, D, heads, P, layout):
    d = data(oracle_mod, D, heads, P, layout)
    worst = [0.0, 0.0]
    for wl, wr in ((200, 0), (127, 5)):
        for sinks in (None, sk.sinks_for(heads[0])):
            r = call(fa, d, "e4m3", (wl, wr), None if sinks is None else dev(sinks))
            for b, (Lq, Lk) in enumerate(d["lens"]):
                q, k, v = d["seqs"][b]
                ob, lb = piece(r, d["cu_q"], b)
                on, ln = ob.float().cpu().numpy(), lb.cpu().numpy()
                o64, l64 = refs(d, wl, wr)[b]
                live = ~wn.dead_rows(Lq, Lk, wl, wr)
                if Lk == 0 or not live.any():
                    continue
                tol_o, tol_l = o_tol("bf16", 1, q, k, v, None, TOL_O["bf16"]), lse_tol("bf16", 1, q, k)
                if sinks is None:
                    ro, rl = float(np.abs(on - o64).max() / tol_o), float(np.abs(ln[:, live] - l64[:, live]).max() / tol_l)
                else:
                    o2, l2 = sk.fold(o64, l64, sinks)
                    bar_o, bar_l = sk.bars(tol_l, tol_o, o2, l64, l2, sinks)
                    ro, rl = float((np.abs(on - o2) / bar_o).max()), float((np.abs(ln - l2) / bar_l).max())
                assert np.isfinite(on).all() and np.isfinite(ln[:, live]).all(), ((wl, wr), b)
                assert ro < 1.0 and rl < 1.0, ((wl, wr), sinks is not None, b, (Lq, Lk), "error / bar", ro, rl)
                worst = [max(worst[0], ro), max(worst[1], rl)]
    print(f"KV8 parity D={D} heads={heads} P={P} {layout}: worst error / bar O {worst[0]:.3f} LSE {worst[1]:.3f}")
    assert worst[0] > 0.01  # the bars are not vacuous


# ---- 3. layouts ------------------------------------------------------------------------------------------------------------------------
def widened_strides(pool, fill):
    """The same pool under strides padded by 16 elements: a [..., D + 16] allocation, `fill` in the padding, its [..., :D] view."""
    import torch

    raw = bits(pool)
    wide = torch.full(raw.shape[:-1] + (raw.shape[-1] + 16,), fill, dtype=raw.dtype, device="cuda")
    wide[..., :raw.shape[-1]] = raw
    return wide.view(pool.dtype)[..., :raw.shape[-1]]


@pytest.mark.parametrize("D,heads,P,layout", [CONFIGS[0], CONFIGS[3]])
def test_wide_and_odd_layouts(fa, oracle_mod, D, heads, P, layout):
    import torch

    d = data(oracle_mod, D, heads, P, layout)
    Hq, Hkv = heads
    n = int(d["cu_q"][-1])
    total = d["q"].shape[0]
    proj = torch.full((total, (Hq + 2 * Hkv) * D), float("nan"), dtype=torch.bfloat16, device="cuda")  # a packed QKV projection
    proj[:, :Hq * D] = d["q"].reshape(total, Hq * D)
    qv = proj[:, :Hq * D].unflatten(1, (Hq, D))
    assert qv.stride() == ((Hq + 2 * Hkv) * D, D, 1)
    wide8 = tuple(widened_strides(p, 0x7F) for p in d["e4m3"])
    wide16 = tuple(widened_strides(p, 0x7FC0) for p in d["bf16"])  # (a bf16 NaN)
    assert wide8[0].stride(-2) % 16 == 0 and wide8[0].stride(-2) >= D + 16 and not wide8[0].is_contiguous()
    sinks = dev(sk.sinks_for(Hq))
    for (wl, wr), s in (((127, 5), None), ((-1, 0), sinks), ((63, 0), None)):
        plain = call(fa, d, "e4m3", (wl, wr), s)
        a = call(fa, d, "e4m3", (wl, wr), s, q=qv, pools=wide8)
        b = call(fa, d, "bf16", twin_window(wl, wr, s), s, q=qv, pools=wide16)
        assert a[0].stride() == qv.stride()
        assert same_bits((a[0][:n].contiguous(), a[1][:, :n].contiguous()), (b[0][:n].contiguous(), b[1][:, :n].contiguous())), (wl, wr)
        assert same_bits((a[0][:n].contiguous(), a[1][:, :n].contiguous()), (plain[0][:n].contiguous(), plain[1][:, :n].contiguous())), (wl, wr)
        nol = call(fa, d, "e4m3", (wl, wr), s, return_lse=False)
        assert nol[1] is None and torch.equal(bits(nol[0][:n]), bits(plain[0][:n])), (wl, wr)
    assert bool(torch.isnan(proj[:, Hq * D:].float()).all())  # nothing was written beside q's columns


# ---- 4. the quantising append ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("muls", [(1.0, 1.0), (0.25, 3.0)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_quantising_append_byte_for_byte(fa, dtype, muls):
    import torch

    tdt = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    layout = "NHD" if muls == (1.0, 1.0) else "HND"
    Hkv, D, P, mp, total = 2, 64, 16, 12, 512
    cap = mp * P
    x, finite = kv8.all_patterns(tdt)  # total * Hkv * D = 65536: every pattern once, the non-finite ones replaced
    x = torch.where(finite, x, torch.full_like(x, 1.5))
    assert x.numel() == total * Hkv * D
    k_rows, v_rows = x.view(total, Hkv, D), x.flip(0).view(total, Hkv, D)
    # (cu entries, length after the append): into an empty cache; nothing new; positions below 0; positions at and past the capacity;
    # a last entry past total_new (clamped) on a row with two bad table entries
    cu = [0, 100, 100, 260, 400, 700]
    after = [100, 50, 120, 250, 112]
    B = len(after)
    num_pages = B * mp + 2
    table = np.random.default_rng(4).permutation(num_pages)[:B * mp].reshape(B, mp).astype(np.int32)
    table[4, 2], table[4, 5] = num_pages + 1, -1
    # wide strides on both sides: new rows in [total, Hkv, D + 8], pools with rows of D + 16 bytes, everything pre-filled with 0x55
    new = torch.full((2, total, Hkv, D + 8), 7.0, dtype=tdt)
    new[0, :, :, :D], new[1, :, :, :D] = k_rows, v_rows
    new = new.cuda()
    shape = (num_pages, Hkv, P, D + 16) if layout == "HND" else (num_pages, P, Hkv, D + 16)
    raw = torch.full((2,) + shape, 0x55, dtype=torch.uint8, device="cuda")
    kp, vpool = raw[0].view(kv8.E4M3)[..., :D], raw[1].view(kv8.E4M3)[..., :D]
    fa.kv_append_paged(new[0, :, :, :D], new[1, :, :, :D], kp, vpool, i32(cu), i32(table), i32(after), 160, layout=layout, k_mul=muls[0], v_mul=muls[1])
    torch.cuda.synchronize()
    want = np.full((2,) + shape, 0x55, np.uint8)
    ref = [kv8.quant_reference(k_rows, muls[0]), kv8.quant_reference(v_rows, muls[1])]
    written = 0
    for b in range(B):
        s0, e0 = min(cu[b], total), min(cu[b + 1], total)
        n_b = min(e0 - s0, 160)
        for i, pos in enumerate(vp.append_positions(n_b, after[b], cap)):
            if pos is None or not 0 <= table[b, pos // P] < num_pages:
                continue
            for t in range(2):
                if layout == "HND":
                    want[t, table[b, pos // P], :, pos % P, :D] = ref[t][s0 + i]
                else:
                    want[t, table[b, pos // P], pos % P, :, :D] = ref[t][s0 + i]
            written += 1
    assert written == 100 + 0 + 120 + 82 + (112 - 32)  # every kind of skip took place
    got = raw.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (dtype, muls, len(bad), "first differing byte (tensor, page, ...):", bad[:3].tolist(),
                           [hex(int(got[tuple(i)])) for i in bad[:3]], [hex(int(want[tuple(i)])) for i in bad[:3]])


# ---- 5. the serving chain ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
def test_append_quant_then_chunked_prefill_then_decode_on_one_pool(fa, oracle_mod, D):
    import torch

    Hq, Hkv, P, N = 8, 2, 16, 300
    rng = np.random.default_rng(190 + D)
    q = vp.draw(oracle_mod.round_to, rng, "bf16", Hq, N + 1, D)   # one more token: the decode step at the end
    k = vp.draw(oracle_mod.round_to, rng, "bf16", Hkv, N + 1, D)
    v = vp.draw(oracle_mod.round_to, rng, "bf16", Hkv, N + 1, D)
    qd, kd, vd = (torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(torch.bfloat16).cuda() for x in (q, k, v))  # [N + 1, H, D]
    kq, vq = (kv8.widen(kv8.quant_reference(torch.from_numpy(x).to(torch.bfloat16), 1.0)) for x in (k, v))  # what the pool will hold
    mp = vp.pages_of(N + 1, P)
    table = i32(np.random.default_rng(2).permutation(mp + 3)[:mp][None])
    kp = torch.full((mp + 3, Hkv, P, D), 0x7F, dtype=torch.uint8, device="cuda").view(kv8.E4M3)
    vpool = torch.full((mp + 3, Hkv, P, D), 0xFF, dtype=torch.uint8, device="cuda").view(kv8.E4M3)
    sl = i32([0])
    o_ch = torch.empty(N, Hq, D, dtype=torch.bfloat16, device="cuda")
    l_ch = torch.empty(Hq, N, dtype=torch.float32, device="cuda")
    for s, n in ((0, 160), (160, 140)):  # the prompt in two chunks: append-quant, then a causal call, seqlens_k advanced in place
        sl.fill_(s + n)
        cu = i32([0, n])
        fa.kv_append_paged(kd[s:s + n], vd[s:s + n], kp, vpool, cu, table, sl, n)
        oc, lc = fa.flash_attention_varlen_paged(qd[s:s + n], kp, vpool, cu, table, sl, n, is_causal=True)
        o_ch[s:s + n], l_ch[:, s:s + n] = oc, lc
    o_full, l_full = fa.flash_attention_varlen_paged(qd[:N], kp, vpool, i32([0, N]), table, sl, N, is_causal=True)  # one call on the full prompt
    torch.cuda.synchronize()
    tol_l = lse_tol("bf16", 1, q, kq)
    err_o, err_l = float((o_ch.float() - o_full.float()).abs().max()), float((l_ch - l_full).abs().max())
    print(f"KV8 chunked D={D}: O {err_o:.2e} (bar {2 * TOL_O['bf16']:.1e}) LSE {err_l:.2e} (bar {2 * tol_l:.2e})")
    assert err_o < 2 * TOL_O["bf16"] and err_l < 2 * tol_l
    # both sides are the operator on the quantised cache
    o64, l64 = wn.reference(q[:, :N], kq[:, :N], vq[:, :N], -1, 0)
    for o, lse in ((o_full, l_full), (o_ch, l_ch)):
        assert np.abs(o.transpose(0, 1).float().cpu().numpy() - o64).max() < o_tol("bf16", 1, q, kq, vq, None, TOL_O["bf16"])
        assert np.abs(lse.cpu().numpy() - l64).max() < tol_l
    # a last chunk of one token: the 128-row KV8 kernel against the paged decode, (bf16, e4m3)
    sl.fill_(N + 1)
    cu = i32([0, 1])
    fa.kv_append_paged(kd[N:], vd[N:], kp, vpool, cu, table, sl, 1)
    o1, l1 = fa.flash_attention_varlen_paged(qd[N:], kp, vpool, cu, table, sl, 1, is_causal=True)
    od, ld = fa.flash_attention_decode_paged(qd[N:].view(1, Hq, 1, D), kp, vpool, table, sl, is_causal=True)
    torch.cuda.synchronize()
    err_o, err_l = float((o1.transpose(0, 1).float() - od[0].float()).abs().max()), float((l1 - ld[0]).abs().max())
    print(f"KV8 last token against the decode D={D}: O {err_o:.2e} (bar {2 * TOL_O['bf16']:.1e}) LSE {err_l:.2e} (bar {2 * TOL_LSE['bf16']:.1e})")
    assert err_o < 2 * TOL_O["bf16"] and err_l < 2 * TOL_LSE["bf16"]


# ---- 6. graph capture --------------------------------------------------------------------------------------------------------------------
def test_append_quant_and_prefill_replay_in_a_graph(fa, oracle_mod):
    import torch

    B, Hq, Hkv, D, P, mp, total, max_q = 3, 8, 2, 64, 16, 40, 333, 200
    num_pages = B * mp + 5
    rng = np.random.default_rng(196)
    win = (127, 0)
    steps = [  # (cu of the chunk = queries and new rows, block table, lengths after the append)
        ([0, 100, 250, 330], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [100, 400, 81]),
        ([0, 200, 200, 330], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [480, 77, 130]),   # a sequence without a chunk
        ([0, 1, 2, 3], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [300, 1, 640]),           # three decode-sized chunks
    ]
    steps[1][1][1, 6] = num_pages + 9  # an entry outside the pool, past the sequence's last page
    rows = [tuple(torch.from_numpy(vp.draw(oracle_mod.round_to, rng, "bf16", total, h, D)).to(torch.bfloat16).cuda() for h in (Hq, Hkv, Hkv))
            for _ in steps]
    sinks_of = [dev(sk.sinks_for(Hq) + np.float32(j)) for j in range(len(steps))]
    init = torch.from_numpy(kv8.to_e4m3_bytes(rng.uniform(-1, 1, (2, num_pages, Hkv, P, D)))).cuda()  # a cache that holds something everywhere
    q, kn, vn = (t.clone() for t in rows[0])
    cu, bt, sl, sinks = i32(steps[0][0]), i32(steps[0][1]), i32(steps[0][2]), sinks_of[0].clone()

    def bufs():
        return (init[0].clone().view(kv8.E4M3), init[1].clone().view(kv8.E4M3), torch.full_like(q, float("nan")),
                torch.full((Hq, total), float("nan"), device="cuda"))

    def step(kp_, vp_, o_, lse_):
        fa.kv_append_paged(kn, vn, kp_, vp_, cu, bt, sl, max_q, k_mul=0.5, v_mul=2.0)
        fa.flash_attention_varlen_paged(q, kp_, vp_, cu, bt, sl, max_q, window=win, sinks=sinks, out=o_, lse=lse_)

    g = bufs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*g)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*g)
    for j in (1, 0, 2, 1):
        c, t, l = steps[j]
        cu.copy_(i32(c))
        bt.copy_(i32(t))
        sl.copy_(i32(l))
        sinks.copy_(sinks_of[j])
        for dst, src in zip((q, kn, vn), rows[j]):
            dst.copy_(src)
        for dst, src in zip(g, bufs()):
            bits(dst).copy_(bits(src))
        graph.replay()
        torch.cuda.synchronize()
        e = bufs()
        step(*e)  # the same two calls eagerly, on fresh buffers
        torch.cuda.synchronize()
        n = c[-1]
        assert torch.equal(bits(g[0]), bits(e[0])) and torch.equal(bits(g[1]), bits(e[1])), "the appended pools"
        assert not torch.equal(bits(g[0]), init[0]), "the append wrote nothing"
        assert torch.equal(bits(g[2][:n]), bits(e[2][:n])) and torch.equal(bits(g[3][:, :n]), bits(e[3][:, :n])), "the prefill"
        assert bool(torch.isnan(g[2][n:].float()).all()) and not bool(torch.isnan(g[2][:n].float()).any())


# ---- 7. dtype errors -----------------------------------------------------------------------------------------------------------------------
def test_dtype_errors(fa, oracle_mod):
    import torch

    d = data(oracle_mod, 64, (4, 4), 16, "HND")
    with pytest.raises(ValueError, match="unsupported / mixed dtypes"):
        call(fa, d, "e4m3", (-1, 0), q=d["q"].to(torch.float16))  # f16 queries on an e4m3 pool
    with pytest.raises(ValueError, match="unsupported / mixed dtypes"):
        call(fa, d, "e4m3", (-1, 0), q=d["q"].to(kv8.E4M3))
    total, Hq, D = d["q"].shape
    with pytest.raises(ValueError, match="out must be"):
        call(fa, d, "e4m3", (-1, 0), out=torch.empty(total, Hq, D + 8, dtype=torch.bfloat16, device="cuda")[..., :D])  # bf16, the wrong strides
    with pytest.raises(ValueError, match="out must be"):
        call(fa, d, "e4m3", (-1, 0), out=torch.empty(total, Hq, D, dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError, match="right side 0"):
        call(fa, d, "e4m3", (63, 5), is_causal=True)  # window and is_causal are mapped as the sink path maps them
    assert not fa.varlen_paged_kv8_supported("f16", "fp8_e4m3", 64, 16) and fa.varlen_paged_kv8_supported("bf16", "fp8_e4m3", 64, 16)
