"""GPU: every call held to its 64-bit addressing promises (include/fa_mi355.h: "The tensors may exceed 4 GiB", "gradients are stored
through 64-bit addresses", "The pool may exceed 4 GiB", "only (max_seqlen + 128) * row_stride * 2 bytes must stay below 4 GiB", "one page
of one head stays below 2 GiB"), loads AND stores, in every family that forms its own base address.

The method: the data lives twice, once in compact tensors and once placed far inside large, real allocations (torch.empty, never filled;
outputs filled with a sentinel). Both placements go through the same entry point with the same scalars -- only addresses, tables and
strides differ -- and the far call must give the compact call's bits on every owned row, while tests/far.py's footprint checker finds the
far outputs untouched everywhere else (and names a store that wrapped at 2^32). So that "both wrong alike" cannot pass, the compact result
is also held to the fp64 references at the bars the family's own tests use (util.TOL_O / o_tol / lse_tol, sink.bars, softcap.bars, the
backward bounds of window_backward / sink / softcap, ksplit.bars). Where each case lies and which thresholds it crosses is planned in
integers by tests/far.py and shown on the CPU by tests/test_far_cases.py; the table is printed once by this file.

All allocations are real and as large as the addresses handed over: correct code cannot fault. Sequences are a few hundred rows, so the
cost is allocation and the sentinel pass. Every test frees its big allocations before it returns, also when it fails (Arena)."""
import numpy as np
import pytest

import backward_bound as bb
import far
import ksplit as ks_
import kv8
import sink as sk
import softcap as sc
import varlen_paged as vp
import window as wn
import window_backward as wb
from test_gpu_decode_paged import check as decode_check
from test_gpu_varlen import cu_dev, pack, seq_data
from test_gpu_varlen_bwd import pack4
from test_gpu_write_footprint import FA_DTYPE, KIND, OUT_KIND, VARIANTS
from util import LN2, TOL_LSE, TOL_O, effective_q, fp8pv_lse_term, fp8pv_term, is_prescaled, lse_tol, o_tol, rowsum_term, to_dev
from varlen_backward import draw_seq

pytestmark = pytest.mark.gpu
CASES = far.cases()
PEAK_LIMIT = 32 * far.GIB
SOFTCAP = 0.25  # softcap.REGIMES "cap_quarter": the default scale
WINDOW = (100, 0)
# name -> (keywords of the call, the (wl, wr) its mask is in tests/window.py)
CALLS = {"causal": (dict(is_causal=True), (-1, 0)), "full": (dict(), (-1, -1)), "window": (dict(window=WINDOW), WINDOW),
         "sink": (dict(is_causal=True), (-1, 0)), "softcap": (dict(is_causal=True, softcap=SOFTCAP), (-1, 0))}


@pytest.fixture(scope="module")
def fa():
    import torch

    import flash_attention_metal_amd as fa

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    fa.load_library()
    return fa


@pytest.fixture(scope="module", autouse=True)
def table_of_crossings():
    print("\nFAR case -> tensor -> thresholds")
    for plan in CASES.values():
        print("\n".join("FAR " + ln for ln in plan.table()))


@pytest.fixture(autouse=True)
def peak_memory(request):
    import torch

    def settle():  # a device error is sticky: after one, no later test of this file may start more work on the card
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"the device reported an error, nothing more of this file is run: {e}", returncode=3)
    settle()
    torch.cuda.reset_peak_memory_stats()
    yield
    settle()
    peak = torch.cuda.max_memory_allocated()
    print(f"FAR PEAK {request.node.name}: {peak / far.GIB:.2f} GiB at most, {torch.cuda.memory_allocated() / far.GIB:.2f} GiB left allocated")
    assert peak < PEAK_LIMIT, (request.node.name, peak)


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------
class Arena:
    """The big allocations of one test. On exit their storage is released whatever still refers to the tensors (a failing test's frames
    do), and the cache is returned to the device. An allocation that does not fit skips the test."""

    def __enter__(self):
        self.held = []
        return self

    def ints(self, kind, numel, sentinel=True):
        """A flat integer tensor for `numel` elements of `kind`: sentinel-filled (an output) or left as allocated (an input)."""
        import torch

        try:
            t = torch.empty(int(numel), dtype=getattr(torch, KIND[kind][1]), device="cuda")
        except torch.cuda.OutOfMemoryError:
            pytest.skip(f"no room for {numel * t_size(kind) / far.GIB:.1f} GiB more on this device")
        self.held.append(t)
        return t.fill_(sentinel_of(kind)) if sentinel else t

    def __exit__(self, *exc):
        import torch

        torch.cuda.synchronize()
        for t in self.held:
            t.untyped_storage().resize_(0)
        self.held = []
        torch.cuda.empty_cache()
        return False


def t_size(kind):
    return far.ITEMSIZE[kind]


def sentinel_of(kind):
    s, bits = KIND[kind][2], 8 * t_size(kind)
    return s - (1 << bits) if s >= (1 << (bits - 1)) and not KIND[kind][1].startswith("u") else s


def typed(ints, kind):
    import torch

    return ints.view(getattr(torch, KIND[kind][0]))


def bits(t):
    import torch

    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def moduli(kind):
    """Where a truncated offset lands, in elements: a 32-bit byte offset wraps at 2^32 / itemsize, a 32-bit element offset at 2^32."""
    return tuple(sorted({(1 << 32) // t_size(kind), 1 << 32}))


def clean(ints, kind, blocks, what):
    rep = far.footprint(ints, sentinel_of(kind), blocks, modulus=moduli(kind))
    assert rep.ok, (what, rep.describe())


def packed_view(ints, kind, total, H, D, rs, hs):
    return typed(ints, kind).as_strided((total, H, D), (rs, hs, 1))


def spots(plan):
    """[(rows of the far tensor, rows of the compact one)] as slices over tokens, sequence by sequence."""
    out, c0 = [], 0
    for t0, L in plan["owned"]:
        out.append((slice(t0, t0 + L), slice(c0, c0 + L)))
        c0 += L
    return out


def place(far_t, near_t, plan, dim=0):
    for f, c in spots(plan):
        far_t[(slice(None),) * dim + (f,)] = near_t[(slice(None),) * dim + (c,)]


def gathered(far_t, plan, dim=0):
    import torch

    return torch.cat([far_t[(slice(None),) * dim + (f,)] for f, _ in spots(plan)], dim=dim)


def lse_blocks(plan, Hq):
    return [(h * plan["total"] + t0, 1, L, L) for t0, L in plan["owned"] for h in range(Hq)]


def sinks_dev(Hq):
    import torch

    return torch.from_numpy(sk.sinks_for(Hq)).cuda()


def hold_forward(name, seqs, o, lse, cu_q, dtype, Hq, what):
    """The compact forward against the fp64 reference of its operator, sequence by sequence, at the bars its family's tests use."""
    wl, wr = CALLS[name][1]
    for b, (q, k, v) in enumerate(seqs):
        s, e = int(cu_q[b]), int(cu_q[b + 1])
        on, ln = o[s:e].transpose(0, 1).float().cpu().numpy(), lse[:, s:e].cpu().numpy()
        bar_o, bar_l = o_tol(dtype, 1, q, k, v, None, TOL_O[dtype]), lse_tol(dtype, 1, q, k)
        if name == "softcap":
            o64, l64 = sc.reference(q, k, v, wl, wr, SOFTCAP, None)
            bar_o, bar_l = sc.bars(bar_l, bar_o, o64, SOFTCAP)
        else:
            o64, l64 = wn.reference(q, k, v, wl, wr)
            if name == "sink":
                o2, l2 = sk.fold(o64, l64, sk.sinks_for(Hq))
                bar_o, bar_l = sk.bars(bar_l, bar_o, o2, l64, l2, sk.sinks_for(Hq))
                o64, l64 = o2, l2
        ro, rl = float((np.abs(on - o64) / bar_o).max()), float((np.abs(ln - l64) / bar_l).max())
        print(f"FAR {what} {name} seq {b}: error / bar O {ro:.3f} LSE {rl:.3f}")
        assert ro < 1.0 and rl < 1.0, (what, name, b, ro, rl)


def seq_bounds(name, seq, dtype, Hq):
    """The backward's reference and bound of one sequence, fed the forward's own O and LSE (chain bounds)."""
    wl, wr = CALLS[name][1]
    if name == "sink":
        return sk.SeqBounds(*seq, wl, wr, sk.sinks_for(Hq), None, dtype)
    if name == "softcap":
        return sc.SeqBounds(*seq, wl, wr, SOFTCAP, None, dtype)
    return wb.SeqBounds(*seq, wl, wr, None, dtype, chain=True)


def hold_backward(name, seq, grads, dtype, Hq, what):
    """grads: (dQ, dK, dV) of the sequence as [H, L, D] device tensors."""
    sb = seq_bounds(name, seq, dtype, Hq)
    g = [x.float().cpu().numpy() for x in grads]
    assert all(np.isfinite(x).all() for x in g), (what, name)
    r = max(bb.ratios(g, sb.ref, sb.bound))
    print(f"FAR {what} {name}: worst backward error / bound {r:.3f}")
    assert r <= 1.0, (what, name, r)


def fwd_kw(name, Hq):
    kw = dict(CALLS[name][0])
    if name == "sink":
        kw["sinks"] = sinks_dev(Hq)
    return kw


# ---- the checker on a real buffer ---------------------------------------------------------------------------------------------------------
def test_checker_reports_a_wrapped_row():
    """A real sentinel buffer above 4 GiB; one far row's data copied by hand to its offset mod 2^32 bytes, the far row left untouched:
    the checker names both."""
    import torch

    n, ln = (1 << 31) + (1 << 20), 128
    near, far_row = 4096, (1 << 31) + 70016
    blocks = [(near, 1, ln, ln), (far_row, 1, ln, ln)]
    with Arena() as a:
        buf = a.ints("bf16", n)
        row = torch.arange(ln, dtype=torch.int16, device="cuda")
        buf[near:near + ln] = row
        buf[far_row:far_row + ln] = row
        assert far.footprint(buf, sentinel_of("bf16"), blocks, modulus=moduli("bf16")).ok
        buf[far_row:far_row + ln] = sentinel_of("bf16")
        buf[far_row - (1 << 31):far_row - (1 << 31) + ln] = row  # where a byte offset truncated to 32 bits lands
        rep = far.footprint(buf, sentinel_of("bf16"), blocks, modulus=moduli("bf16"))
        assert rep.untouched == [(far_row, far_row, 70016, True)], rep.describe()
        assert rep.outside_count == ln and rep.outside == list(range(70016, 70016 + 64)), rep.describe()  # (the first 64 are kept)
        assert "a wrapped store" in rep.describe()


# ---- A. the packed forward with q / o far -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A-packed-forward-q-far", "A-packed-forward-q-far-head-major-f16"])
def test_packed_forward_with_q_and_o_far(fa, oracle_mod, case):
    import torch

    plan = CASES[case]
    dtype, D, Hq, Hkv, total, rs, hs = (plan[n] for n in ("dtype", "D", "Hq", "Hkv", "total", "row_stride", "head_stride"))
    rng = np.random.default_rng(41)
    seqs = [seq_data(oracle_mod, rng, Hq, Hkv, Lq, Lk, D, dtype) for Lq, Lk in zip(plan["lens_far"], plan["lens_near"])]
    q, k, v, cu_q, cu_k = pack(seqs, dtype, plan["layout"])
    assert list(cu_q) == [0, 300, 557] and list(cu_k) == plan["cu_near"]
    tq = plan.tensors["q"]
    with Arena() as a:
        q_far = packed_view(a.ints(dtype, tq.numel, sentinel=False), dtype, total, Hq, D, rs, hs)
        place(q_far, q, plan)
        o_ints, l_ints = a.ints(dtype, tq.numel), a.ints("f32", Hq * total)
        o_far, l_far = packed_view(o_ints, dtype, total, Hq, D, rs, hs), typed(l_ints, "f32").view(Hq, total)
        for name in CALLS:
            o_c, l_c = fa.flash_attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), plan["max_far"], plan["max_near"], **fwd_kw(name, Hq))
            o_ints.fill_(sentinel_of(dtype))
            l_ints.fill_(sentinel_of("f32"))
            fa.flash_attention_varlen(q_far, k, v, cu_dev(plan["cu_far"]), cu_dev(cu_k), plan["max_far"], plan["max_near"], out=o_far, lse=l_far,
                                      **fwd_kw(name, Hq))
            torch.cuda.synchronize()
            assert same(gathered(o_far, plan), o_c), (case, name, "O of the far placement differs from the compact call")
            assert same(gathered(l_far, plan, 1), l_c), (case, name, "LSE of the far placement differs from the compact call")
            clean(o_ints, dtype, plan.tensors["o"].blocks, (case, name, "O"))
            clean(l_ints, "f32", lse_blocks(plan, Hq), (case, name, "LSE"))
            hold_forward(name, seqs, o_c, l_c, cu_q, dtype, Hq, case)


# ---- B. the packed backward, one side far at a time ---------------------------------------------------------------------------------------
def _packed_backward(fa, case):
    import torch

    plan = CASES[case]
    side, dtype, D, Hq, Hkv, total, rs, hs = (plan[n] for n in ("side", "dtype", "D", "Hq", "Hkv", "total", "row_stride", "head_stride"))
    H = Hq if side == "q" else Hkv
    lens_q, lens_k = (plan["lens_far"], plan["lens_near"]) if side == "q" else (plan["lens_near"], plan["lens_far"])
    rng = np.random.default_rng(43)
    seqs = [draw_seq(rng, Hq, Hkv, Lq, Lk, D, dtype) for Lq, Lk in zip(lens_q, lens_k)]
    (q, k, v, do), _, cu_q, cu_k = pack4(seqs, dtype, "THD")
    near = {"q": q, "k": k, "v": v, "d_o": do}
    cq_far, ck_far = (plan["cu_far"], list(cu_k)) if side == "q" else (list(cu_q), plan["cu_far"])
    names = ("q", "o", "d_o") if side == "q" else ("k", "v")
    gnames = ("dq",) if side == "q" else ("dk", "dv")
    with Arena() as a:
        big = {n: packed_view(a.ints(dtype, plan.tensors[n].numel, sentinel=False), dtype, total, H, D, rs, hs) for n in names}
        for n in names:
            if n != "o":
                place(big[n], near[n], plan)
        g_ints = {n: a.ints("f32", plan.tensors[n].numel) for n in gnames}
        g_far = {n: packed_view(g_ints[n], "f32", total, H, D, rs, hs) for n in gnames}
        total_q = total if side == "q" else int(cu_q[-1])
        l_far = torch.empty(Hq, total_q, dtype=torch.float32, device="cuda")
        for name in CALLS:
            kw = fwd_kw(name, Hq)
            o_c, l_c = fa.flash_attention_varlen(q, k, v, cu_dev(cu_q), cu_dev(cu_k), 300, 300, **kw)
            g_c = fa.flash_attention_varlen_backward(q, k, v, o_c, do, l_c, cu_dev(cu_q), cu_dev(cu_k), 300, 300, **kw)
            if side == "q":
                place(big["o"], o_c, plan)
                place(l_far, l_c, plan, 1)
                args = (big["q"], k, v, big["o"], big["d_o"], l_far)
                gkw = dict(dq=g_far["dq"])
            else:
                args = (q, big["k"], big["v"], o_c, do, l_c)
                gkw = dict(dk=g_far["dk"], dv=g_far["dv"])
            for n in gnames:
                g_ints[n].fill_(sentinel_of("f32"))
            g_f = fa.flash_attention_varlen_backward(*args, cu_dev(cq_far), cu_dev(ck_far), 300, 300, **gkw, **kw)
            torch.cuda.synchronize()
            for i, n in enumerate(("dq", "dk", "dv")):
                got = gathered(g_f[i], plan) if n in gnames else g_f[i]
                assert same(got, g_c[i]), (case, name, n + " of the far placement differs from the compact call", float((got - g_c[i]).abs().max()))
            if name == "sink":
                assert same(g_f[3], g_c[3]), (case, "dsinks of the far placement differ from the compact call")
            for n in gnames:
                clean(g_ints[n], "f32", plan.tensors[n].blocks, (case, name, n))
            b = 1  # one sequence held to the fp64 reference: the one that lies far
            piece = lambda t, cu: t[int(cu[b]):int(cu[b + 1])].transpose(0, 1)
            hold_backward(name, seqs[b], (piece(g_c[0], cu_q), piece(g_c[1], cu_k), piece(g_c[2], cu_k)), dtype, Hq, case)


def test_packed_backward_with_the_q_side_far(fa):
    _packed_backward(fa, "B-packed-backward-q-far")


def test_packed_backward_with_the_kv_side_far(fa):
    _packed_backward(fa, "B-packed-backward-kv-far")


# ---- C. in-sequence offsets of 2 - 4 GiB through a wide row stride ------------------------------------------------------------------------
def _wide_data(oracle, plan, backward):
    dtype, D, Hq, Hkv, L = (plan[n] for n in ("dtype", "D", "Hq", "Hkv", "L"))
    rng = np.random.default_rng(47 + D)
    if backward:
        seq = draw_seq(rng, Hq, Hkv, L, L, D, dtype)
        (q, k, v, do), _, cu, _ = pack4([seq], dtype, "THD")
        return seq, dict(q=q, k=k, v=v, d_o=do), cu
    seq = seq_data(oracle, rng, Hq, Hkv, L, L, D, dtype)
    q, k, v, cu, _ = pack([seq], dtype, "THD")
    return seq, dict(q=q, k=k, v=v), cu


def _wide_view(ints, kind, plan, H):
    return packed_view(ints, kind, plan["L"], H, plan["D"], plan["row_stride"], plan["head_stride"])


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_wide_rows_forward(fa, oracle_mod, dtype):
    import torch

    case = f"C-wide-forward-{dtype}"
    plan = CASES[case]
    Hq, Hkv, L = plan["Hq"], plan["Hkv"], plan["L"]
    seq, near, cu = _wide_data(oracle_mod, plan, False)
    with Arena() as a:
        big = {n: _wide_view(a.ints(dtype, plan.tensors[n].numel, sentinel=False), dtype, plan, Hq if n == "q" else Hkv) for n in ("q", "k", "v")}
        for n in big:
            big[n].copy_(near[n])
        o_ints = a.ints(dtype, plan.tensors["o"].numel)
        o_far = _wide_view(o_ints, dtype, plan, Hq)
        for name in ("causal", "full"):
            kw = fwd_kw(name, Hq)
            o_c, l_c = fa.flash_attention_varlen(near["q"], near["k"], near["v"], cu_dev(cu), cu_dev(cu), L, L, **kw)
            o_ints.fill_(sentinel_of(dtype))
            l_far = torch.full((Hq, L), float("nan"), device="cuda")
            fa.flash_attention_varlen(big["q"], big["k"], big["v"], cu_dev(cu), cu_dev(cu), L, L, out=o_far, lse=l_far, **kw)
            torch.cuda.synchronize()
            assert same(o_far, o_c) and same(l_far, l_c), (case, name, "the wide placement differs from the compact call")
            clean(o_ints, dtype, plan.tensors["o"].blocks, (case, name, "O"))
            hold_forward(name, [seq[:3]], o_c, l_c, cu, dtype, Hq, case)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("side", ["q", "kv"])
def test_wide_rows_backward(fa, oracle_mod, side, dtype):
    import torch

    case = f"C-wide-backward-{side}-{dtype}"
    plan = CASES[case]
    Hq, Hkv, L = plan["Hq"], plan["Hkv"], plan["L"]
    H = Hq if side == "q" else Hkv
    seq, near, cu = _wide_data(oracle_mod, plan, True)
    names = ("q", "o", "d_o") if side == "q" else ("k", "v")
    gnames = ("dq",) if side == "q" else ("dk", "dv")
    with Arena() as a:
        big = {n: _wide_view(a.ints(dtype, plan.tensors[n].numel, sentinel=False), dtype, plan, H) for n in names}
        for n in names:
            if n != "o":
                big[n].copy_(near[n])
        g_ints = {n: a.ints("f32", plan.tensors[n].numel) for n in gnames}
        g_far = {n: _wide_view(g_ints[n], "f32", plan, H) for n in gnames}
        for name in ("causal", "full"):
            kw = fwd_kw(name, Hq)
            o_c, l_c = fa.flash_attention_varlen(near["q"], near["k"], near["v"], cu_dev(cu), cu_dev(cu), L, L, **kw)
            g_c = fa.flash_attention_varlen_backward(near["q"], near["k"], near["v"], o_c, near["d_o"], l_c, cu_dev(cu), cu_dev(cu), L, L, **kw)
            if side == "q":
                big["o"].copy_(o_c)
                args, gkw = (big["q"], near["k"], near["v"], big["o"], big["d_o"], l_c), dict(dq=g_far["dq"])
            else:
                args, gkw = (near["q"], big["k"], big["v"], o_c, near["d_o"], l_c), dict(dk=g_far["dk"], dv=g_far["dv"])
            for n in gnames:
                g_ints[n].fill_(sentinel_of("f32"))
            g_f = fa.flash_attention_varlen_backward(*args, cu_dev(cu), cu_dev(cu), L, L, **gkw, **kw)
            torch.cuda.synchronize()
            for i, n in enumerate(("dq", "dk", "dv")):
                assert same(g_f[i], g_c[i]), (case, name, n + " of the wide placement differs from the compact call")
            for n in gnames:
                clean(g_ints[n], "f32", plan.tensors[n].blocks, (case, name, n))
            hold_backward(name, seq, [g.transpose(0, 1) for g in g_c], dtype, Hq, case)


# ---- D, E, F. pools whose used pages lie past element 2^32 --------------------------------------------------------------------------------
def _pool_data(oracle, plan, Hq, e4m3):
    """Two sequences drawn once: bf16 q rows (packed [total_q, Hq, D]), K / V on the pool's grid, the compact pool in table order."""
    Hkv, P, D = plan["Hkv"], plan["P"], plan["D"]
    rng = np.random.default_rng(53 + (1 if e4m3 else 0))
    draw_kv = (lambda *s: kv8.draw_e4m3(rng, *s)) if e4m3 else (lambda *s: vp.draw(oracle.round_to, rng, "bf16", *s))
    seqs = [(vp.draw(oracle.round_to, rng, "bf16", Hq, Lq, D), draw_kv(Hkv, L, D), draw_kv(Hkv, L, D)) for Lq, L in plan["lens"]]
    pool = vp.build_pool([s[1] for s in seqs], [s[2] for s in seqs], P, rng=None, spare=1, fill=0.0)
    assert [[p + plan["first_page"] for p in row] for row in pool["pages"]] == plan["tables"] and pool["table"].shape[1] == plan["max_pages"]
    qn, cu_q = vp.pack_rows([s[0] for s in seqs])
    return seqs, pool, to_dev(qn, "bf16"), cu_q


def _laid(x, layout):
    return x if layout == "HND" else x.transpose(1, 2)


def _far_pool(a, plan, kind, sentinel=False):
    """(ints, pool) of one far pool: [num_pages, Hkv, P, D] storage in the plan's layout."""
    Hkv, P, D, n = plan["Hkv"], plan["P"], plan["D"], plan["num_pages"]
    ints = a.ints(kind, n * plan["page_stride"], sentinel=sentinel)
    shape = (n, Hkv, P, D) if plan["layout"] == "HND" else (n, P, Hkv, D)
    return ints, typed(ints, kind).view(shape)


def _compact_pool(pool, name, kind, layout):
    import torch

    x = torch.from_numpy(pool[name] if layout == "HND" else np.ascontiguousarray(pool[name].transpose(0, 2, 1, 3)))
    return x.to(kv8.E4M3 if kind == "fp8" else torch.bfloat16).cuda()


def _hold_prefill(seqs, o, lse, cu_q, sinks, what, S=None):
    for b, (q, k, v) in enumerate(seqs):
        s, e = int(cu_q[b]), int(cu_q[b + 1])
        on, ln = o[s:e].transpose(0, 1).float().cpu().numpy(), lse[:, s:e].cpu().numpy()
        o64, l64 = wn.reference(q, k, v, -1, 0)
        bar_o, bar_l = o_tol("bf16", 1, q, k, v, None, TOL_O["bf16"]), lse_tol("bf16", 1, q, k)
        if S is not None:
            bar_o, bar_l, o64, l64 = ks_.bars(S, bar_l, bar_o, o64, l64, ks_.absum_reference(q, k, v, -1, 0), sinks)
        elif sinks is not None:
            o2, l2 = sk.fold(o64, l64, sinks)
            bar_o, bar_l = sk.bars(bar_l, bar_o, o2, l64, l2, sinks)
            o64, l64 = o2, l2
        ro, rl = float((np.abs(on - o64) / bar_o).max()), float((np.abs(ln - l64) / bar_l).max())
        print(f"FAR {what} seq {b}: error / bar O {ro:.3f} LSE {rl:.3f}")
        assert ro < 1.0 and rl < 1.0, (what, b, ro, rl)


@pytest.mark.parametrize("layout", ["HND", "NHD"])
def test_e4m3_pools_far(fa, oracle_mod, layout):
    """D: the kv8 prefill with and without sinks, and the decode with bf16 and with e4m3 queries, on pages past element 2^32."""
    import torch

    case = f"D-e4m3-pool-{layout}"
    plan = CASES[case]
    Hq, Hkv, D = 16, plan["Hkv"], plan["D"]
    seqs, pool, q, cu_q = _pool_data(oracle_mod, plan, Hq, True)
    first, used = plan["first_page"], plan["used_pages"]
    lens_k = [L for _, L in plan["lens"]]
    kc, vc = (_compact_pool(pool, n, "fp8", layout) for n in ("k", "v"))
    tab_c, tab_f = cu_dev(pool["table"]), cu_dev(pool["table"] + first)
    rng = np.random.default_rng(59)
    qd = {kind: oracle_mod.round_to(rng.uniform(-1.0, 1.0, (2, Hq, 1, D)).astype(np.float32), kind) for kind in ("bf16", "fp8")}
    with Arena() as a:
        (_, kf), (_, vf) = _far_pool(a, plan, "fp8"), _far_pool(a, plan, "fp8")
        bits(kf)[first:first + used] = bits(kc)[:used]
        bits(vf)[first:first + used] = bits(vc)[:used]
        for sinks in (None, sk.sinks_for(Hq)):
            kw = dict(is_causal=True, layout=layout, sinks=None if sinks is None else sinks_dev(Hq))
            o_c, l_c = fa.flash_attention_varlen_paged(q, kc, vc, cu_dev(cu_q), tab_c, cu_dev(lens_k), 130, **kw)
            o_f, l_f = fa.flash_attention_varlen_paged(q, kf, vf, cu_dev(cu_q), tab_f, cu_dev(lens_k), 130, **kw)
            torch.cuda.synchronize()
            assert same(o_f, o_c) and same(l_f, l_c), (case, "kv8 prefill", sinks is not None, "the far pool differs from the compact one")
            _hold_prefill(seqs, o_c, l_c, cu_q, sinks, (case, "kv8 prefill", "sinks" if sinks is not None else "plain"))
        for kind in ("bf16", "fp8"):
            qq = to_dev(qd[kind], kind)
            o_c, l_c = fa.flash_attention_decode_paged(qq, kc, vc, tab_c, cu_dev(lens_k), is_causal=True, layout=layout)
            o_f, l_f = fa.flash_attention_decode_paged(qq, kf, vf, tab_f, cu_dev(lens_k), is_causal=True, layout=layout)
            torch.cuda.synchronize()
            assert same(o_f, o_c) and same(l_f, l_c), (case, "decode", kind, "the far pool differs from the compact one")
            decode_check(oracle_mod, o_c, l_c, qd[kind], [s[1] for s in seqs], [s[2] for s in seqs], lens_k, True, "fp8", (case, "decode", kind),
                         tol_o=2 * TOL_O["bf16"], strict=False)


def test_bf16_pool_with_element_offsets_past_2_32(fa, oracle_mod):
    """E: the plain paged prefill and its key split (S = 2) on an 8.5 GiB pool pair: page * page_stride passes 2^32 ELEMENTS."""
    import torch

    case = "E-bf16-pool-HND"
    plan = CASES[case]
    Hq = 16
    seqs, pool, q, cu_q = _pool_data(oracle_mod, plan, Hq, False)
    first, used = plan["first_page"], plan["used_pages"]
    lens_k = [L for _, L in plan["lens"]]
    kc, vc = (_compact_pool(pool, n, "bf16", "HND") for n in ("k", "v"))
    tab_c, tab_f = cu_dev(pool["table"]), cu_dev(pool["table"] + first)
    with Arena() as a:
        (_, kf), (_, vf) = _far_pool(a, plan, "bf16"), _far_pool(a, plan, "bf16")
        kf[first:first + used] = kc[:used]
        vf[first:first + used] = vc[:used]
        for S in (None, 2):
            kw = dict(is_causal=True, layout="HND", num_splits=S)
            o_c, l_c = fa.flash_attention_varlen_paged(q, kc, vc, cu_dev(cu_q), tab_c, cu_dev(lens_k), 130, **kw)
            o_f, l_f = fa.flash_attention_varlen_paged(q, kf, vf, cu_dev(cu_q), tab_f, cu_dev(lens_k), 130, **kw)
            torch.cuda.synchronize()
            assert same(o_f, o_c) and same(l_f, l_c), (case, S, "the far pool differs from the compact one")
            _hold_prefill(seqs, o_c, l_c, cu_q, None, (case, "splits", S), S=S)




# ---- F. appends into far pages ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,new_kind", [("F-append-bf16-pool-HND", "bf16"), ("F-append-e4m3-pool-HND", "fp8"), ("F-append-e4m3-pool-HND", "bf16"),
                                           ("F-append-e4m3-pool-HND", "f16")])
def test_appends_into_far_pages(fa, oracle_mod, case, new_kind):
    """The last n_b keys of every sequence appended into far, sentinel-filled pools (the byte copy in bf16 and in e4m3, the quantising
    append from bf16 and from f16): the far pages hold byte for byte what the same append leaves in a compact pool, every other byte of
    the far pools is the sentinel, and with the older keys filled in by hand the prefill of D / E reads the appended pages."""
    import torch

    plan = CASES[case]
    kind, Hq, Hkv, P, D, ps = plan["kind"], 16, plan["Hkv"], plan["P"], plan["D"], plan["page_stride"]
    seqs, pool, q, cu_q = _pool_data(oracle_mod, plan, Hq, kind == "fp8")
    first, used, n_c = plan["first_page"], plan["used_pages"], pool["num_pages"]
    lens_k = [L for _, L in plan["lens"]]
    kn, cu_n = vp.pack_rows([s[1][:, L - n:] for s, (n, L) in zip(seqs, plan["lens"])])
    vn, _ = vp.pack_rows([s[2][:, L - n:] for s, (n, L) in zip(seqs, plan["lens"])])
    k_new, v_new = (to_dev(x, new_kind) for x in (kn, vn))  # (K / V of an e4m3 pool lie on the e4m3 grid: exact in bf16 and f16 too)
    tab_c, tab_f = cu_dev(pool["table"]), cu_dev(pool["table"] + first)
    sent = sentinel_of(kind)
    ci = [torch.full((n_c * ps,), sent, dtype=getattr(torch, KIND[kind][1]), device="cuda") for _ in range(2)]
    kc, vc = (typed(x, kind).view(n_c, Hkv, P, D) for x in ci)
    with Arena() as a:
        (ki, kf), (vi, vf) = _far_pool(a, plan, kind, sentinel=True), _far_pool(a, plan, kind, sentinel=True)
        fa.kv_append_paged(k_new, v_new, kc, vc, cu_dev(cu_n), tab_c, cu_dev(lens_k), 130)
        fa.kv_append_paged(k_new, v_new, kf, vf, cu_dev(cu_n), tab_f, cu_dev(lens_k), 130)
        torch.cuda.synchronize()
        for name, c, f in (("k", ci[0], ki), ("v", ci[1], vi)):
            assert bool((c != sent).any()), (case, new_kind, "the append wrote nothing")
            assert torch.equal(f[first * ps:(first + used) * ps], c[:used * ps]), (case, new_kind, name + ": the far pages differ from the compact pool's")
            clean(f, kind, plan.tensors[name + "_pages"].blocks, (case, new_kind, name))
        # the older keys by hand, into both placements; then the prefill on the appended pages against the pool that was laid out whole
        whole = [_compact_pool(pool, n, kind, "HND") for n in ("k", "v")]
        old = torch.zeros(n_c, Hkv, P, dtype=torch.bool, device="cuda")
        for b, (n, L) in enumerate(plan["lens"]):
            for j in range(L - n):
                old[int(pool["table"][b, j // P]), :, j % P] = True
        for w, c, f in zip(whole, (kc, vc), (kf, vf)):
            bits(c)[old] = bits(w)[old]
            bits(f)[first:first + used][old[:used]] = bits(w)[:used][old[:used]]
        kw = dict(is_causal=True, layout="HND")
        o_w, l_w = fa.flash_attention_varlen_paged(q, whole[0], whole[1], cu_dev(cu_q), tab_c, cu_dev(lens_k), 130, **kw)
        o_c, l_c = fa.flash_attention_varlen_paged(q, kc, vc, cu_dev(cu_q), tab_c, cu_dev(lens_k), 130, **kw)
        o_f, l_f = fa.flash_attention_varlen_paged(q, kf, vf, cu_dev(cu_q), tab_f, cu_dev(lens_k), 130, **kw)
        torch.cuda.synchronize()
        assert same(o_c, o_w) and same(l_c, l_w), (case, new_kind, "the prefill on the appended compact pool differs from the pool laid out whole")
        assert same(o_f, o_w) and same(l_f, l_w), (case, new_kind, "the prefill on the appended far pages differs from the compact pool")
        _hold_prefill(seqs, o_w, l_w, cu_q, None, (case, new_kind, "prefill after the append"))


# ---- G. the key-split workspace above 2^31 elements ---------------------------------------------------------------------------------------
def test_key_split_workspace_above_2_31_elements(fa, oracle_mod):
    """64 splits of one tile each on 16512 query rows: the workspace is 8.1 GiB and the indices of both launches pass 2^31 elements.
    Every row against an fp64 reference (formed on the device, head by head) at the bars of tests/ksplit.py, the un-split call at its own
    bars, the numpy reference on three 128-row blocks of heads 0 and 15, two runs bit for bit, every slot of the workspace written and the
    guard behind it intact."""
    import torch

    plan = CASES["G-ksplit-workspace"]
    S, Hq, Hkv, D, Lq, Lk, P = (plan[n] for n in ("S", "Hq", "Hkv", "D", "Lq", "Lk", "P"))
    rng = np.random.default_rng(61)
    qn = vp.draw(oracle_mod.round_to, rng, "bf16", Hq, Lq, D)
    kn, vn = (vp.draw(oracle_mod.round_to, rng, "bf16", Hkv, Lk, D) for _ in range(2))
    pool = vp.build_pool([kn], [vn], P, rng=np.random.default_rng(62), spare=1, fill=0.0)
    kp, vpool = (_compact_pool(pool, n, "bf16", "HND") for n in ("k", "v"))
    q = to_dev(qn.transpose(1, 0, 2), "bf16")
    cu, tab, lens = cu_dev([0, Lq]), cu_dev(pool["table"]), cu_dev([Lk])
    need = fa.varlen_paged_split_workspace_bytes(1, Hq, Lq, Lq, D, P, pool["table"].shape[1], S)
    assert need == plan["workspace_bytes"] == ks_.workspace_bytes(S, Hq, Lq, D) and need // 4 > (1 << 31)
    guard = 1 << 18
    with Arena() as a:
        ws = a.ints("f32", need // 4 + guard)
        call = lambda **kw: fa.flash_attention_varlen_paged(q, kp, vpool, cu, tab, lens, Lq, layout="HND", window=(-1, -1), **kw)
        o1, l1 = call(num_splits=1)
        o, l = call(num_splits=S, workspace=ws.view(torch.uint8)[:need])
        torch.cuda.synchronize()
        rep = far.footprint(ws, sentinel_of("f32"), plan.tensors["workspace"].blocks, modulus=moduli("f32"))
        assert rep.ok, ("the workspace: slots left unwritten or the guard touched", rep.describe())
        ws.fill_(sentinel_of("f32"))
        o2, l2 = call(num_splits=S, workspace=ws.view(torch.uint8)[:need])
        torch.cuda.synchronize()
        assert same(o2, o) and same(l2, l), "two runs differ"
        assert bool((ws[need // 4:] == sentinel_of("f32")).all()), "the guard behind the workspace was written"
    # every row: fp64 on the device, head by head (16512 x 4096 scores each)
    bar_l0, bar_o0 = lse_tol("bf16", 1, qn, kn), o_tol("bf16", 1, qn, kn, vn, None, TOL_O["bf16"])
    k64, v64 = (to_dev(x, "bf16").double() for x in (kn, vn))
    worst = [0.0] * 4
    for h in range(Hq):
        hk = h // (Hq // Hkv)
        s = (q[:, h].double() @ k64[hk].T) * (D ** -0.5)
        l64 = torch.logsumexp(s, dim=1)
        p = torch.exp(s - l64[:, None])
        o64, absum = (p @ v64[hk]).cpu().numpy()[None], (p @ v64[hk].abs()).cpu().numpy()[None]
        l64 = l64.cpu().numpy()[None]
        bar_o, bar_l, _, _ = ks_.bars(S, bar_l0, bar_o0, o64, l64, absum)
        got = [(x[:, h].float().cpu().numpy()[None], y[h].cpu().numpy()[None]) for x, y in ((o, l), (o1, l1))]
        r = [float((np.abs(got[0][0] - o64) / bar_o).max()), float((np.abs(got[0][1] - l64) / bar_l).max()),
             float(np.abs(got[1][0] - o64).max() / bar_o0), float(np.abs(got[1][1] - l64).max() / bar_l0)]
        worst = [max(a_, b_) for a_, b_ in zip(worst, r)]
        del s, p
    print(f"FAR G: worst error / bar, {S} splits O {worst[0]:.3f} LSE {worst[1]:.3f}; un-split O {worst[2]:.3f} LSE {worst[3]:.3f}")
    assert max(worst) < 1.0, worst
    # the numpy reference on the first, a middle and the last 128-row block of heads 0 and 15
    for h in (0, Hq - 1):
        hk = h // (Hq // Hkv)
        for r0 in (0, 64 * 128, Lq - 128):
            qs = qn[h:h + 1, r0:r0 + 128]
            o64, l64 = wn.reference(qs, kn[hk:hk + 1], vn[hk:hk + 1], -1, -1)
            bar_o, bar_l, _, _ = ks_.bars(S, lse_tol("bf16", 1, qs, kn), o_tol("bf16", 1, qs, kn, vn, None, TOL_O["bf16"]), o64, l64,
                                          ks_.absum_reference(qs, kn[hk:hk + 1], vn[hk:hk + 1], -1, -1))
            on, ln = o[r0:r0 + 128, h].float().cpu().numpy()[None], l[h, r0:r0 + 128].cpu().numpy()[None]
            assert float((np.abs(on - o64) / bar_o).max()) < 1.0 and float((np.abs(ln - l64) / bar_l).max()) < 1.0, (h, r0)


# ---- H. the dense calls with batch entry 1 past 2^32 bytes --------------------------------------------------------------------------------
SMALL_BYTES = (1 << 32) + (2 << 20)      # one tensor of any input type under the 4 GiB + 1 MiB batch stride
BIG_BYTES = 2 * ((1 << 32) + (1 << 20)) + (1 << 20)  # ... and of an fp32 gradient (or e4m3's bf16 output) under a 16-bit (1-byte) element stride


@pytest.fixture(scope="module")
def dense_buffers():
    """One set of big byte buffers for every dense case: three of 4 GiB and two of 8 GiB, released when the module is done."""
    import torch

    with Arena() as a:
        yield dict(small=[a.ints("u8", SMALL_BYTES, sentinel=False) for _ in range(3)], big=[a.ints("u8", BIG_BYTES, sentinel=False) for _ in range(2)])


def _as(buf, kind, numel):
    """(ints, [..] view maker) of the first numel elements of `kind` in a byte buffer."""
    import torch

    assert numel * t_size(kind) <= buf.numel()
    return buf[:numel * t_size(kind)].view(getattr(torch, KIND[kind][1]))


def _dense_view(ints, kind, B, H, N, D, bs, hs):
    return typed(ints, kind).as_strided((B, H, N, D), (bs, hs, D, 1))


def _hold_dense(fa, oracle, o, lse, q, k, v, dtype, causal, variant):
    """util.check's bars on an O / LSE that is already there (fa_fwd on compact tensors); e4m3 as tests/test_gpu_parity.py holds it."""
    on, ln = o.float().cpu().numpy(), lse.cpu().numpy()
    assert np.isfinite(on).all() and np.isfinite(ln).all()
    if dtype == "fp8":
        o64, l64 = oracle.attn_fwd_ex_f64(q, k, v, causal, None)
        assert np.abs(on - o64).max() < TOL_O["bf16"] + fp8pv_term(variant, "fp8", v), (variant, causal, np.abs(on - o64).max())
        assert np.abs(ln - l64).max() < 1e-4 + fp8pv_lse_term(variant, "fp8"), (variant, causal)
        return
    pre = is_prescaled(fa, dtype, variant, *q.shape, causal)
    if pre:
        o64, l64 = oracle.attn_fwd_ex_f64(effective_q(oracle, q, dtype), k, v, causal, LN2)
        assert np.abs(on - o64).max() < TOL_O[dtype] and np.abs(ln - l64).max() < TOL_LSE[dtype] + rowsum_term(dtype, pre), (variant, dtype, causal, "on Q~")
    o64, l64 = oracle.attn_fwd_ex_f64(q, k, v, causal, None)
    assert np.abs(on - o64).max() < o_tol(dtype, pre, q, k, v, None, TOL_O[dtype]), (variant, dtype, causal, np.abs(on - o64).max())
    assert np.abs(ln - l64).max() < lse_tol(dtype, pre, q, k, None, TOL_LSE[dtype]), (variant, dtype, causal, np.abs(ln - l64).max())


def _dense_forward(fa, oracle, bufs, kind, variants, Hkv=None):
    import torch

    lib = fa.load_library()
    plan = CASES[f"H-dense-forward-{kind}"]
    B, H, N, D, bs, hs = (plan[n] for n in ("B", "H", "N", "D", "batch_stride", "head_stride"))
    Hkv = H if Hkv is None else Hkv
    okind = OUT_KIND[kind]
    rng = np.random.default_rng(67)
    qn = oracle.round_to(rng.uniform(-1.0, 1.0, (B, H, N, D)).astype(np.float32), kind)
    kn, vn = (oracle.round_to(rng.uniform(-1.0, 1.0, (B, Hkv, N, D)).astype(np.float32), kind) for _ in range(2))
    near = [to_dev(x, kind) for x in (qn, kn, vn)]
    tq = plan.tensors["q"]
    big = [_dense_view(_as(b, kind, tq.numel), kind, B, h, N, D, bs, hs) for b, h in zip(bufs["small"], (H, Hkv, Hkv))]
    for f, c in zip(big, near):
        f.copy_(c)
    o_ints = _as(bufs["big"][0], okind, tq.numel)
    o_far = _dense_view(o_ints, okind, B, H, N, D, bs, hs)
    scale, ran = D ** -0.5, []
    for variant in variants:
        if not lib.fa_supported(FA_DTYPE[kind], VARIANTS[variant], D):
            continue
        ran.append(variant)
        for causal in (0, 1):
            what = (kind, variant, causal, Hkv)
            o_c, l_c = torch.empty(B, H, N, D, dtype=o_far.dtype, device="cuda"), torch.empty(B, H, N, dtype=torch.float32, device="cuda")
            l_f = torch.full((B, H, N), float("nan"), device="cuda")
            o_ints.fill_(sentinel_of(okind))

            def run(q, k, v, o, l, qbs, qhs, kbs, khs):
                if Hkv == H:
                    st = lib.fa_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), l.data_ptr(), B, H, N, D, scale, qbs, qhs, causal,
                                    FA_DTYPE[kind], VARIANTS[variant], None)
                else:
                    st = lib.fa_fwd_exv(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), l.data_ptr(), B, H, Hkv, N, N, D, scale, qbs, qhs,
                                        kbs, khs, causal, FA_DTYPE[kind], VARIANTS[variant], None)
                assert st == 0, (what, lib.fa_last_error())
            run(*near, o_c, l_c, H * N * D, N * D, Hkv * N * D, N * D)
            run(*big, o_far, l_f, bs, hs, bs, hs)
            torch.cuda.synchronize()
            assert same(o_far, o_c) and same(l_f, l_c), (what, "the far batch entry differs from the compact call")
            clean(o_ints, okind, plan.tensors["o"].blocks, (what, "O"))
            _hold_dense(fa, oracle, o_c, l_c, qn, kn, vn, kind, bool(causal), variant)
    return ran


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16", "fp8"])
def test_dense_forward_with_batch_entry_1_past_4_gib(fa, oracle_mod, dense_buffers, kind):
    """fa_fwd in every variant fa_supported answers 1 for at head_dim 64: each kernel file forms its own batch base."""
    ran = _dense_forward(fa, oracle_mod, dense_buffers, kind, list(VARIANTS))
    print(f"FAR H {kind}: {ran}")
    assert "auto" in ran and len(ran) >= 2, ran


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_dense_splitkv_grouped_heads_with_batch_entry_1_past_4_gib(fa, oracle_mod, dense_buffers, kind):
    """fa_fwd_exv on the key-split kernel, two query heads on one key head, q / o and k / v each one batch stride apart."""
    assert _dense_forward(fa, oracle_mod, dense_buffers, kind, ["mfma_splitkv"], Hkv=1) == ["mfma_splitkv"]


@pytest.mark.parametrize("side", ["q", "kv"])
def test_dense_backward_with_batch_entry_1_past_4_gib(fa, oracle_mod, dense_buffers, side):
    """fa_bwd_ex with the q side (q, o, d_o, dq) or the kv side (k, v, dk, dv) one 4 GiB-plus batch stride apart; fp32 gradients of
    entry 1 lie past 2^33 bytes."""
    import torch

    lib = fa.load_library()
    kind = "bf16"
    plan = CASES[f"H-dense-backward-{side}-{kind}"]
    B, H, N, D, bs, hs = (plan[n] for n in ("B", "H", "N", "D", "batch_stride", "head_stride"))
    rng = np.random.default_rng(71)
    qn, kn, vn, don = (bb.rnd(rng.uniform(-1.0, 1.0, (B, H, N, D)).astype(np.float32), kind) for _ in range(4))
    names = ("q", "o", "d_o") if side == "q" else ("k", "v")
    gnames = ("dq",) if side == "q" else ("dk", "dv")
    numel = plan.tensors[names[0]].numel
    big = {n: _dense_view(_as(b, kind, numel), kind, B, H, N, D, bs, hs) for n, b in zip(names, dense_buffers["small"])}
    g_ints = {n: _as(b, "f32", numel) for n, b in zip(gnames, dense_buffers["big"])}
    g_far = {n: _dense_view(g_ints[n], "f32", B, H, N, D, bs, hs) for n in gnames}
    cbs, chs = H * N * D, N * D
    for causal in (0, 1):
        X = bb.Bounds(qn, kn, vn, don, bool(causal), None, kind)
        near = dict(q=to_dev(qn, kind), k=to_dev(kn, kind), v=to_dev(vn, kind), d_o=to_dev(don, kind), o=to_dev(bb.rnd(X.o.astype(np.float32), kind), kind))
        lse = torch.from_numpy(X.lse.astype(np.float32)).cuda()
        for n in names:
            big[n].copy_(near[n])
        for n in gnames:
            g_ints[n].fill_(sentinel_of("f32"))
        g_c = {n: torch.full((B, H, N, D), float("nan"), device="cuda") for n in ("dq", "dk", "dv")}
        qs, kvs = ((bs, hs), (cbs, chs)) if side == "q" else ((cbs, chs), (bs, hs))
        need = max(lib.fa_bwd_workspace_bytes_ex(FA_DTYPE[kind], B, H, H, N, N, D, *s1, *s2) for s1, s2 in (((cbs, chs), (cbs, chs)), (qs, kvs)))
        assert need > 0
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")

        def run(t, g, s1, s2):
            st = lib.fa_bwd_ex(t["q"].data_ptr(), t["k"].data_ptr(), t["v"].data_ptr(), t["o"].data_ptr(), t["d_o"].data_ptr(), lse.data_ptr(),
                               g["dq"].data_ptr(), g["dk"].data_ptr(), g["dv"].data_ptr(), ws.data_ptr(), B, H, H, N, N, D, D ** -0.5, *s1, *s2, causal,
                               FA_DTYPE[kind], None)
            assert st == 0, (side, causal, lib.fa_last_error())
            torch.cuda.synchronize()
        run(near, g_c, (cbs, chs), (cbs, chs))
        g_f = {n: torch.full((B, H, N, D), float("nan"), device="cuda") for n in ("dq", "dk", "dv")}
        g_f.update(g_far)
        run({**near, **big}, g_f, qs, kvs)
        for n in ("dq", "dk", "dv"):
            assert same(g_f[n], g_c[n]), (side, causal, n + " of the far batch entry differs from the compact call")
        for n in gnames:
            clean(g_ints[n], "f32", plan.tensors[n].blocks, (side, causal, n))
        g = [g_c[n].cpu().numpy() for n in ("dq", "dk", "dv")]
        r = bb.ratios(g, X.ref, X.bound)
        print(f"FAR H backward {side} causal={causal}: error / bound dq {r[0]:.3f} dk {r[1]:.3f} dv {r[2]:.3f}")
        assert all(np.isfinite(x).all() for x in g) and max(r) <= 1.0, (side, causal, r)
