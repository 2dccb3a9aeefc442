"""GPU: the soft-capping forwards fa_fwd_varlen_softcap, fa_fwd_varlen_paged_softcap and fa_fwd_decode_paged_softcap (softcap= of
flash_attention_varlen / _varlen_paged / _decode_paged). References and bars live in tests/softcap.py (held against an fp32 model of the
kernels' arithmetic, and shown to expose the planted mistakes, by tests/test_softcap_cases.py on the CPU):
  1. parity with the fp64 reference element by element on window.SEQS as one packed batch with trailing unowned tokens, five windows,
     both regimes (softcap 0.25 at the default scale; softcap 50 at scale 150 / sqrt(D)), at lse_tol + softcap tanh_err and
     o_tol + |O| softcap tanh_err (include/fa_mi355.h, "Logit soft-capping"); dead rows exactly O = 0 and LSE = -inf; sentinels on the
     unowned tokens; the paged prefill (P = 16 HND shuffled, P = 256 NHD, NaN in every slot nobody may read) bit for bit the packed call;
  2. the decode: Nq 1 / 4, L 0 / 63 / 200 / 1000 in a cache of 4096, the four dtype pairs;
  3. known answers: K = 0 makes every t exactly 0, so LSE = ln(visible keys) and O = the mean of V; scores of exactly +-64 softcap saturate,
     so LSE = ln(n_plus e^cap + n_minus e^-cap) and O the matching weighted mean (a missing cap gives a one-hot row);
  4. lse = None; q as a view of a packed projection; prefill and decode captured in a graph and replayed after the tables changed.

Worst error / bar measured on an MI355X (printed by the parity tests): prefill O 0.14, LSE 0.32 (bf16, head_dim 64); decode O 0.04, LSE 0.02."""
import numpy as np
import pytest

import chain_bound as cb
import softcap as sc
import varlen_paged as vp
import window as wn
from test_gpu_decode_paged import to_layout
from test_gpu_window import CAP, DECODE_PAIRS, bits, data, decode, decode_batch, i32, paged, piece, same_bits, varlen
from util import TOL_O, lse_tol, o_tol, to_dev

pytestmark = pytest.mark.gpu
MATRIX = [(t, d) for t in ("f16", "bf16") for d in (64, 128)]
_REF = {}


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


def refs(d, wl, wr, cap, scale):
    """The fp64 references of a batch, computed once and shared."""
    key = (id(d), wl, wr, cap, scale)
    if key not in _REF:
        _REF[key] = [sc.reference(*s, wl, wr, cap, scale) for s in d["seqs"]]
    return _REF[key]


def nan_pool(d, P, layout, ks=None):
    """Pages in random order, NaN in every slot no key occupies (the tail of a last page, the spare pages)."""
    ks = [s[1] for s in d["seqs"]] if ks is None else ks
    pool = vp.build_pool(ks, [s[2] for s in d["seqs"]], P, rng=np.random.default_rng(P + 20), spare=2, fill=np.nan)
    return to_layout(pool["k"], d["dtype"], layout), to_layout(pool["v"], d["dtype"], layout), pool["table"]


def check_parity(d, r, wl, wr, cap, scale, what):
    """Every sequence of the batch against the fp64 reference, element by element. Returns the worst error / bar (O, LSE)."""
    dtype, worst = d["dtype"], [0.0, 0.0]
    for b, (Lq, Lk) in enumerate(d["lens"]):
        q, k, v = d["seqs"][b]
        ob, lb = piece(r, d["cu_q"], b)
        on, ln = ob.float().cpu().numpy(), lb.cpu().numpy()
        o64, l64 = refs(d, wl, wr, cap, scale)[b]
        dead = wn.dead_rows(Lq, Lk, wl, wr)
        assert not on[:, dead].any() and np.isneginf(ln[:, dead]).all(), (what, b, "dead rows: O = 0 and LSE = -inf")
        if dead.all():
            continue
        live = ~dead
        assert np.isfinite(on).all() and np.isfinite(ln[:, live]).all(), (what, b)
        bar_o, bar_l = sc.bars(lse_tol(dtype, 1, q, k, scale), o_tol(dtype, 1, q, k, v, scale, TOL_O[dtype]), o64, cap)
        ro, rl = float((np.abs(on - o64) / bar_o).max()), float(np.abs(ln[:, live] - l64[:, live]).max() / bar_l)
        print(f"SOFTCAP parity {what} seq {b} {(Lq, Lk)}: error / bar O {ro:.3f} LSE {rl:.3f}")
        assert ro <= 1.0 and rl <= 1.0, (what, b, (Lq, Lk), "error / bar", ro, rl)
        worst = [max(worst[0], ro), max(worst[1], rl)]
    return worst


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", MATRIX)
def test_parity_with_the_fp64_reference(fa, oracle_mod, dtype, D):
    import torch

    worst = [0.0, 0.0]
    for heads in wn.HEADS:
        d = data(oracle_mod, dtype, D, heads)
        n_own = int(d["cu_q"][-1])
        pools = {cfg: nan_pool(d, *cfg) for cfg in ((16, "HND"), (256, "NHD"))}
        for name, cap, rs in sc.REGIMES:
            scale = sc.scale_of(rs, D)
            for n, (wl, wr) in enumerate(sc.WINDOWS):
                # into the caller's buffers: the trailing tokens nobody owns keep their sentinels
                out = torch.full_like(d["q"], float("nan"))
                lse = torch.full((heads[0], d["q"].shape[0]), float("nan"), device="cuda")
                a = varlen(fa, d, (wl, wr), softcap=cap, scale=scale, out=out, lse=lse)
                assert bool(torch.isnan(out[n_own:].float()).all()) and bool(torch.isnan(lse[:, n_own:]).all()), "unowned tokens are not written"
                w1 = check_parity(d, a, wl, wr, cap, scale, ("varlen", dtype, D, heads, name, (wl, wr)))
                cfg = ((16, "HND"), (256, "NHD"))[n % 2]
                p = paged(fa, d, *cfg, (wl, wr), pool=pools[cfg], softcap=cap, scale=scale)
                w2 = check_parity(d, p, wl, wr, cap, scale, ("paged",) + cfg + (dtype, D, heads, name, (wl, wr)))
                worst = [max(worst[0], w1[0], w2[0]), max(worst[1], w1[1], w2[1])]
                for b, (Lq, Lk) in enumerate(d["lens"]):  # the paged prefill is the packed call, bit for bit
                    if Lk >= Lq >= 1:
                        assert same_bits(piece(p, d["cu_q"], b), piece(a, d["cu_q"], b)), ("paged != packed", heads, name, (wl, wr), b)
    print(f"SOFTCAP parity {dtype} D={D}: worst error / bar O {worst[0]:.3f} LSE {worst[1]:.3f}")
    assert worst[1] > 0.01  # the bars are not vacuous


def test_window_none_lse_none_and_a_view_of_a_packed_projection(fa, oracle_mod):
    import torch

    d = data(oracle_mod, "bf16", 64, (8, 2))
    cap = 0.25
    for call in (lambda **kw: varlen(fa, d, **kw), lambda **kw: paged(fa, d, 16, "HND", **kw)):
        assert same_bits(call(window=None, causal=True, softcap=cap), call(window=(-1, 0), softcap=cap))
        assert same_bits(call(window=None, softcap=cap), call(window=(-1, -1), softcap=cap))
        assert same_bits(call(window=(63, -1), causal=True, softcap=cap), call(window=(63, 0), softcap=cap))
        nol = call(window=(63, 0), softcap=cap, return_lse=False)
        assert nol[1] is None and same_bits((nol[0], None), call(window=(63, 0), softcap=cap))
        # None and 0.0 are the calls without a cap, untouched; a cap changes the result
        assert same_bits(call(window=(63, 0), softcap=None), call(window=(63, 0))) and same_bits(call(window=(63, 0), softcap=0.0), call(window=(63, 0)))
        assert not same_bits(call(window=(63, 0), softcap=cap), call(window=(63, 0)))
    # q as a view of one packed [total, Hq + 2 Hkv, D] projection (k and v stay the batch's own): the same bits as the contiguous q
    total = d["q"].shape[0]
    buf = torch.zeros(total, 8 + 4, 64, dtype=torch.bfloat16, device="cuda")
    buf[:, :8] = d["q"]
    qv = buf[:, :8]
    lens = d["lens"]
    r = fa.flash_attention_varlen(qv, d["k"], d["v"], i32(d["cu_q"]), i32(d["cu_k"]), max(lq for lq, _ in lens), max(lk for _, lk in lens),
                                  window=(127, 5), softcap=cap)
    torch.cuda.synchronize()
    n = int(d["cu_q"][-1])
    assert r[0].stride() == qv.stride() and same_bits((r[0][:n].contiguous(), r[1][:, :n]), varlen(fa, d, (127, 5), softcap=cap))


# ---- 2. decode -------------------------------------------------------------------------------------------------------------------------
DECODE_L = (0, 63, 200, 1000)
DECODE_CASES = [(qdt, kvdt, D, Nq, P, layout) for (qdt, kvdt), (D, Nq, P, layout) in
                zip(DECODE_PAIRS * 2, [(64, 1, 16, "HND"), (128, 4, 256, "NHD"), (64, 4, 16, "NHD"), (128, 1, 256, "HND"),
                                       (128, 4, 16, "HND"), (64, 1, 256, "NHD"), (128, 1, 16, "NHD"), (64, 4, 256, "HND")])]


@pytest.mark.parametrize("qdt,kvdt,D,Nq,P,layout", DECODE_CASES)
def test_decode_parity_and_dead_rows(fa, oracle_mod, qdt, kvdt, D, Nq, P, layout):
    Hq, Hkv = 8, 2
    lens = list(DECODE_L)
    q, ks, vs = decode_batch(oracle_mod, qdt, kvdt, D, Hq, Hkv, Nq, P, layout, lens=DECODE_L, seed=20)
    pool = vp.build_pool(ks, vs, P, rng=np.random.default_rng(P + 21), spare=2, fill=np.nan, max_pages=CAP // P)  # NaN in unused slots
    pool = (to_layout(pool["k"], kvdt, layout), to_layout(pool["v"], kvdt, layout), pool["table"])
    bar = "bf16" if "fp8" in (qdt, kvdt) else qdt
    base_o = (2 if kvdt == "fp8" else 1) * TOL_O[bar]  # (an e4m3 cache at twice the amplitude, as tests/test_gpu_window.py)
    worst = [0.0, 0.0]
    for name, cap, rs in sc.REGIMES:
        scale = sc.scale_of(rs, D)
        for wl, wr in sc.WINDOWS:
            o, lse = decode(fa, q, qdt, pool, lens, layout, (wl, wr), softcap=cap, scale=scale)
            on, ln = o.float().cpu().numpy(), lse.cpu().numpy()
            for b, L in enumerate(lens):
                dead = wn.dead_rows(Nq, L, wl, wr)
                assert not on[b][:, dead].any() and np.isneginf(ln[b][:, dead]).all(), (name, (wl, wr), L, "dead rows")
                live = ~dead
                if not live.any():
                    continue
                o64, l64 = sc.reference(q[b], ks[b], vs[b], wl, wr, cap, scale)
                assert np.isfinite(on[b]).all() and np.isfinite(ln[b][:, live]).all(), (name, (wl, wr), L)
                bar_o, bar_l = sc.bars(lse_tol(bar, 1, q[b], ks[b], scale), o_tol(bar, 1, q[b], ks[b], vs[b], scale, base_o), o64, cap)
                ro, rl = float((np.abs(on[b] - o64) / bar_o).max()), float(np.abs(ln[b][:, live] - l64[:, live]).max() / bar_l)
                assert ro <= 1.0 and rl <= 1.0, (name, (wl, wr), L, "error / bar", ro, rl)
                worst = [max(worst[0], ro), max(worst[1], rl)]
    print(f"SOFTCAP decode {qdt}/{kvdt} D={D} Nq={Nq} P={P} {layout}: worst error / bar O {worst[0]:.3f} LSE {worst[1]:.3f}")
    # the wrapper: window=None is (-1, 0) under is_causal, else (-1, -1); lse = None
    assert same_bits(decode(fa, q, qdt, pool, lens, layout, None, causal=True, softcap=0.25), decode(fa, q, qdt, pool, lens, layout, (-1, 0), softcap=0.25))
    assert same_bits(decode(fa, q, qdt, pool, lens, layout, None, softcap=0.25), decode(fa, q, qdt, pool, lens, layout, (-1, -1), softcap=0.25))
    nol = decode(fa, q, qdt, pool, lens, layout, (63, 0), softcap=0.25, return_lse=False)
    assert nol[1] is None and same_bits((nol[0], None), decode(fa, q, qdt, pool, lens, layout, (63, 0), softcap=0.25))


# ---- 3. known answers ----------------------------------------------------------------------------------------------------------------
KNOWN_SEQS = ((130, 257), (200, 130), (64, 0))


def known_bars(dtype, o2, A, n, cap_term):
    """With every probability known exactly what is left is the fp32 sums over the n values (one addition per key, one pass per tile),
    ln, the rounding of O to the type and the cap's own term."""
    bar_l = 2.0 ** -22 * (np.abs(np.log(np.maximum(n, 1.0))) + 4.0) + cap_term
    out_round = np.maximum(cb.U_OUT[dtype] * np.abs(o2), 2.0 ** -25 if dtype == "f16" else 0.0)
    return out_round + 2.0 ** -24 * (n[None, :, None] + 8) * A + np.abs(o2) * bar_l[None, :, None], bar_l


@pytest.mark.parametrize("dtype,D", MATRIX)
def test_zero_keys_make_every_tanh_exactly_zero(fa, oracle_mod, dtype, D):
    Hq, Hkv = 8, 2
    d = data(oracle_mod, dtype, D, (Hq, Hkv), lens=KNOWN_SEQS, seed=3)
    kz = to_dev(np.zeros_like(d["kn"]), dtype)
    zero_pool = nan_pool(d, 16, "NHD", ks=[np.zeros_like(s[1]) for s in d["seqs"]])
    for wl, wr in sc.WINDOWS:
        for r, what in ((varlen(fa, d, (wl, wr), k=kz, softcap=50.0), "varlen"), (paged(fa, d, 16, "NHD", (wl, wr), pool=zero_pool, softcap=50.0), "paged")):
            for b, (Lq, Lk) in enumerate(KNOWN_SEQS):
                on, ln = (x.float().cpu().numpy() for x in piece(r, d["cu_q"], b))
                vis = wn.visible(Lq, Lk, wl, wr) if Lk else np.zeros((Lq, 0), bool)
                n = vis.sum(1).astype(np.float64)
                dead = n == 0
                assert not on[:, dead].any() and np.isneginf(ln[:, dead]).all(), (what, (wl, wr), b, "dead rows")
                if Lk == 0:
                    continue
                live = ~dead
                v = np.repeat(d["seqs"][b][2].astype(np.float64), Hq // Hkv, axis=0)  # [Hq, Lk, D]
                o2 = np.einsum("ij,hjd->hid", vis.astype(np.float64), v)[:, live] / n[live][None, :, None]
                A = np.einsum("ij,hjd->hid", vis.astype(np.float64), np.abs(v))[:, live] / n[live][None, :, None]
                # t = 0 exactly (2^0 = 1, 1 + 1 = 2, 1 / 2, 1 - 1): m = 0, every P = 1, l = n -- no tanh term in the bars
                bar_o, bar_l = known_bars(dtype, o2, A, n[live], 0.0)
                ro, rl = float((np.abs(on[:, live] - o2) / bar_o).max()), float((np.abs(ln[:, live] - np.log(n[live])[None]) / bar_l[None]).max())
                assert ro <= 1.0 and rl <= 1.0, (what, (wl, wr), (Lq, Lk), "error / bar", ro, rl)


@pytest.mark.parametrize("dtype,D", MATRIX)
def test_scores_far_beyond_the_cap_saturate_at_plus_and_minus_the_cap(fa, oracle_mod, dtype, D):
    """softcap = 2, scale = 1 and one non-zero coordinate, q_0 = 8 and k_0 = +-16: scale s = +-128 = +-64 softcap exactly, and the kernels'
    2^y overflows to inf / flushes to 0, so t = +-1 exactly. LSE = ln(n_plus e^2 + n_minus e^-2), O the matching weighted mean of V.
    Without the cap the row is one-hot over its positive keys and LSE = 128 + ln(n_plus)."""
    Hq, Hkv, cap = 4, 2, 2.0
    lens = ((70, 70), (130, 257))
    d = data(oracle_mod, dtype, D, (Hq, Hkv), lens=lens, seed=4)
    rng = np.random.default_rng(40 + D)
    ks = []
    for _, k, _ in d["seqs"]:
        kk = np.zeros_like(k)
        kk[..., 0] = np.where(rng.uniform(size=k.shape[:2]) < 0.5, 16.0, -16.0)
        ks.append(kk)
    qs = [np.zeros_like(q) for q, _, _ in d["seqs"]]
    for q in qs:
        q[..., 0] = 8.0
    scale = 1.0
    qn, _ = vp.pack_rows(qs, tail=3)
    kn, _ = vp.pack_rows(ks, tail=1)
    import torch

    for wl, wr in ((-1, 0), (63, 0), (-1, -1)):
        r = fa.flash_attention_varlen(to_dev(qn, dtype), to_dev(kn, dtype), d["v"], i32(d["cu_q"]), i32(d["cu_k"]), 130, 257, window=(wl, wr),
                                      softcap=cap, scale=scale)
        torch.cuda.synchronize()
        for b, (Lq, Lk) in enumerate(lens):
            on, ln = (x.float().cpu().numpy() for x in piece(r, d["cu_q"], b))
            vis = wn.visible(Lq, Lk, wl, wr).astype(np.float64)
            G = Hq // Hkv
            sign = np.repeat(np.sign(ks[b][..., 0]).astype(np.float64), G, axis=0)  # [Hq, Lk]
            w = np.where(sign > 0, np.exp(cap), np.exp(-cap))[:, None, :] * vis[None]  # [Hq, Lq, Lk]
            den = w.sum(-1)
            v = np.repeat(d["seqs"][b][2].astype(np.float64), G, axis=0)
            o2, A = (w @ v) / den[..., None], (w @ np.abs(v)) / den[..., None]
            l2 = np.log(den)
            n = vis.sum(1)
            # the bars of the known answer plus the cap's term: t = +-1 exactly here, what is left of it is C = fp32(softcap log2e) and the fma
            cap_term = cap * sc.TANH_ERR
            bar_l = 2.0 ** -22 * (np.abs(l2) + 4.0 + 2 * cap) + cap_term
            out_round = np.maximum(cb.U_OUT[dtype] * np.abs(o2), 2.0 ** -25 if dtype == "f16" else 0.0)
            # (every probability e^-4 relative to the row's largest is rounded to the type for the PV product)
            bar_o = out_round + (2.0 ** -24 * (n[None, :, None] + 8) + 2 * cb.U_OUT[dtype]) * A + np.abs(o2) * bar_l[..., None]
            ro, rl = float((np.abs(on - o2) / bar_o).max()), float((np.abs(ln - l2) / bar_l).max())
            assert ro <= 1.0 and rl <= 1.0, ((wl, wr), (Lq, Lk), "error / bar", ro, rl)
            both = (w > 0).any(-1) & ((sign[:, None, :] * vis[None]) > 0).any(-1) & ((sign[:, None, :] * vis[None]) < 0).any(-1)
            assert both.any()
            # a missing cap: weights e^128 against e^-128, LSE = 128 + ln(n_plus)
            assert np.abs(ln[both] - 128.0).min() > 100.0


# ---- 4. graph replay ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("f16", 128)])
def test_graph_replay_after_the_tables_change(fa, oracle_mod, dtype, D):
    import torch

    Hq, Hkv, P, mp, B, total, max_q = 8, 2, 16, 40, 3, 400, 200
    win, dwin, cap = (100, 0), (150, 0), 0.25
    rng = np.random.default_rng(200 + D)
    q = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, total, Hq, D), dtype)
    qd = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, B, Hq, 1, D), dtype)
    num_pages = B * mp + 4
    kp = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, num_pages, Hkv, P, D), dtype)  # every slot finite: any prefix is a cache
    vpool = to_dev(vp.draw(oracle_mod.round_to, rng, dtype, num_pages, Hkv, P, D), dtype)
    steps = [  # (cu of the chunk, block table, cache lengths)
        ([0, 100, 250, 400], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [100, 600, 151]),
        ([0, 200, 200, 330], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [480, 77, 130]),
        ([0, 1, 2, 3], rng.permutation(num_pages)[:B * mp].reshape(B, mp), [1, 300, 17]),
    ]
    cu, bt, sl = i32(steps[0][0]), i32(steps[0][1]), i32(steps[0][2])
    ws = torch.empty(fa.decode_paged_workspace_bytes(B, Hq, Hkv, 1, D, P, mp), dtype=torch.uint8, device="cuda")

    def bufs():
        return (torch.full_like(q, float("nan")), torch.full((Hq, total), float("nan"), device="cuda"),
                torch.full_like(qd, float("nan")), torch.full((B, Hq, 1), float("nan"), device="cuda"))

    def step(o_, lse_, od_, ld_):
        fa.flash_attention_varlen_paged(q, kp, vpool, cu, bt, sl, max_q, window=win, out=o_, lse=lse_, softcap=cap)
        fa.flash_attention_decode_paged(qd, kp, vpool, bt, sl, window=dwin, out=od_, lse=ld_, workspace=ws, softcap=cap)

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
    for c, t, l in (steps[1], steps[0], steps[2], steps[1]):
        cu.copy_(i32(c))
        bt.copy_(i32(t))
        sl.copy_(i32(l))
        for dst, src in zip(g, bufs()):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        e = bufs()
        step(*e)  # the same two calls eagerly, on fresh buffers
        torch.cuda.synchronize()
        n = c[-1]
        assert torch.equal(bits(g[0][:n]), bits(e[0][:n])) and torch.equal(bits(g[1][:, :n]), bits(e[1][:, :n])), "the capped prefill"
        assert torch.equal(bits(g[2]), bits(e[2])) and torch.equal(bits(g[3]), bits(e[3])), "the capped decode"
        assert bool(torch.isnan(g[0][n:].float()).all())  # tokens nobody owns stay untouched
        # and the replayed prefill is the operator: sequence 0 against the fp64 reference on its gathered cache
        L0, n0 = l[0], c[1] - c[0]
        if n0 and L0 <= mp * P:
            kg = vp.gather(kp.float().cpu().numpy(), t[0], L0, P)
            vg = vp.gather(vpool.float().cpu().numpy(), t[0], L0, P)
            q0 = q[:n0].float().cpu().numpy().transpose(1, 0, 2)
            o64, l64 = sc.reference(q0, kg, vg, *win, cap)
            on = g[0][:n0].float().cpu().numpy().transpose(1, 0, 2)
            live = ~wn.dead_rows(n0, L0, *win)
            bar_o, bar_l = sc.bars(lse_tol(dtype, 1, q0, kg), o_tol(dtype, 1, q0, kg, vg, None, TOL_O[dtype]), o64, cap)
            assert (np.abs(on - o64) <= bar_o).all() and np.abs(g[1][:, :n0].cpu().numpy()[:, live] - l64[:, live]).max() <= bar_l
