"""GPU: the MLA family held to its 64-bit addressing promises (include/fa_mi355.h: "The pool may exceed 4 GiB; one page stays below
2 GiB", three long long strides each for q and o of the decode, "q, k, v and o EACH have their own (row, head) element strides" with the
4 GiB rule per sequence and per tensor only, fp32 gradients "addressed under the element strides of q, k, v respectively") --
fa_fwd_mla_decode_paged, fa_fwd_mla_decode_paged_wide, fa_fwd_mla_decode_paged_kv8, fa_fwd_varlen_mla and fa_bwd_varlen_mla, with the
aliased appends the header prescribes for the latent pool.

The method is tests/test_gpu_far_addresses.py's, and so are the helpers (imported, not copied): the data lives twice, once compact and
once placed far inside real allocations as large as the addresses handed over (torch.empty; inputs unfilled, outputs sentinel-filled).
Both placements go through the same Python entry point with the same scalars; the far call must give the compact call's BITS on every
owned row, tests/far.py's footprint checker must find every far output untouched elsewhere (it names a store that wrapped at 2^32 bytes or
elements), and the compact result is held to the fp64 reference at the bars its family already uses -- mla.check for the decodes,
mla_prefill.check for the prefill, mla_bwd.SeqBounds / worst_ratio with chain=True for the backward on the forward's own O and LSE -- so
that "both wrong alike" cannot pass. No tolerance is introduced here. Where each case lies and what it crosses is planned in integers by
far.mla_cases() and shown on the CPU by tests/test_far_cases.py and tests/test_far_cases_mla.py; the table is printed once by this file.

All allocations are real: correct code cannot fault. Every test frees its big allocations before it returns, also when it fails."""
import numpy as np
import pytest

import far
import kv8
import mla
import mla_bwd as mb
import mla_kv8
import mla_prefill as mp
from test_gpu_far_addresses import (Arena, bits, clean, fa, gathered, lse_blocks, moduli, packed_view, peak_memory, place, same,  # noqa: F401
                                    sentinel_of, typed)  # (fa, peak_memory: fixtures -- the peak and the sticky-error exit of that file)
from test_gpu_varlen import cu_dev
from test_gpu_write_footprint import KIND
from util import to_dev

pytestmark = pytest.mark.gpu
CASES = far.mla_cases()
DQK, DV, DSCALE = mla.DQK, mla.DV, mla.SCALE
PQK, PV, PSCALE = mp.DQK, mp.DV, mp.SCALE


@pytest.fixture(scope="module", autouse=True)
def table_of_crossings():
    print("\nFAR MLA case -> tensor -> thresholds")
    for plan in CASES.values():
        print("\n".join("FAR " + ln for ln in plan.table()))


def clean_t(ints, t, what):
    """clean() for a planned tensor; a tensor whose pointer names element t.base of the allocation wraps relative to that element."""
    if t.base == 0:
        return clean(ints, t.kind, t.blocks, what)
    rep = far.footprint(ints, sentinel_of(t.kind), t.blocks, modulus=moduli(t.kind), base=t.base)
    assert rep.ok, (what, rep.describe())


def strided(ints, kind, shape, strides, base=0):
    return typed(ints, kind).as_strided(tuple(shape), tuple(strides), base)


# ---- M-D, M-F, M-H, M-G: the decodes ---------------------------------------------------------------------------------------------------------
def latent_pool(rng, lens, P, kind, rs=DQK, pad_page=False):
    """The compact pool in table order, as far.mla_pool() plans the far one: (full device tensor [n, P (+ 1), rs] of the pool's type, the
    [n, P, 576] view the call takes, table int32 [B, max_pages] of compact page numbers, kvs). One spare page behind the used ones, which
    the unused table entries name; every slot, column and row nobody may read holds NaN (0x7F / 0xFF in e4m3)."""
    import torch

    npb = [(L + P - 1) // P for L in lens]
    n = sum(npb) + 1
    pool = np.full((n, P + (1 if pad_page else 0), rs), np.nan, np.float32)
    table = np.full((len(lens), max(npb)), n - 1, np.int32)
    kvs, pg = [], 0
    for b, L in enumerate(lens):
        kv = kv8.draw_e4m3(rng, L, DQK) if kind == "fp8" else mp.round_to(rng.uniform(-1.0, 1.0, (L, DQK)).astype(np.float32), kind)
        for j in range(npb[b]):
            m = min(P, L - j * P)
            pool[pg, :m, :DQK] = kv[j * P:j * P + m]
            table[b, j] = pg
            pg += 1
        kvs.append(kv.astype(np.float32))
    full = torch.from_numpy(mla_kv8.codes_of(pool)).cuda().view(kv8.E4M3) if kind == "fp8" else to_dev(pool, kind)
    return full, full[:, :P, :DQK], table, kvs


def far_pool(a, plan, full_c, sentinel=False):
    """(ints, full far pool [num_pages, P (+ 1), rs], its [num_pages, P, 576] view); the compact pool's pages copied to first_page .."""
    kind, P, rs, n = plan["kind"], plan["P"], plan["row_stride"], plan["num_pages"]
    ints = a.ints(kind, n * plan["page_stride"], sentinel=sentinel)
    full = typed(ints, kind).view(n, plan["page_stride"] // rs, rs)
    if full_c is not None:
        bits(full)[plan["first_page"]:plan["first_page"] + full_c.shape[0]] = bits(full_c)
    return ints, full, full[:, :P, :DQK]


def decode(fa, q, view, table, lens, causal, wide, **kw):
    import torch

    o, lse = fa.flash_attention_mla_decode_paged(q, view, cu_dev(table), cu_dev(lens), DSCALE, is_causal=causal, wide=wide, **kw)
    torch.cuda.synchronize()
    return o, lse


def hold_decode(oracle, o, lse, q, kvs, lens, causal, what):
    return mla.check(oracle, o.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64), q, kvs, lens, causal, "bf16",
                     ("FAR",) + tuple(what), DSCALE)


def pool_table(plan, table):
    assert [[p + plan["first_page"] for p in row if p != table.max()] for row in table.tolist()] == plan["tables"] and table.shape[1] == plan["max_pages"]
    return table + plan["first_page"]  # the far table is the compact table plus first_page (the spare page moves with it)


@pytest.mark.parametrize("case", ["M-D-bf16-pool", "M-D-bf16-pool-padded", "M-D-e4m3-pool"])
def test_decodes_on_latent_pools_past_element_2_32(fa, oracle_mod, case):
    """M-D: every decode call of the family on a pool whose used pages lie past element 2^32 (8.5 GiB in bf16, 4.5 GiB in e4m3), at the row
    counts that choose the wave count and the entry point; B, Hq, Nq and max_pages_per_seq are equal in both placements, so the split
    count and the workspace are, and the bits comparable."""
    plan = CASES[case]
    kind, P, lens = plan["kind"], plan["P"], plan["lens"]
    rng = np.random.default_rng(101 + len(case))
    full_c, view_c, table, kvs = latent_pool(rng, lens, P, kind, plan["row_stride"], plan["pad_page"])
    assert full_c.stride(0) == plan["page_stride"] and full_c.shape[0] == plan["used_pages"] + 1
    table_f = pool_table(plan, table)
    with Arena() as a:
        _, _, view_f = far_pool(a, plan, full_c)
        assert view_f.shape[0] == plan["num_pages"] != view_c.shape[0] and view_f.stride() == view_c.stride()
        for Hq, Nq, causal, wide in plan["calls"]:
            q = mp.round_to(rng.uniform(-1.0, 1.0, (len(lens), Hq, Nq, DQK)).astype(np.float32), "bf16")
            qd = to_dev(q, "bf16")
            o_c, l_c = decode(fa, qd, view_c, table, lens, causal, wide)
            o_f, l_f = decode(fa, qd, view_f, table_f, lens, causal, wide)
            what = (case, Hq * Nq, "rows", "wide" if wide else "kv8" if wide is None else "one-wave", "causal" if causal else "full")
            assert same(o_f, o_c) and same(l_f, l_c), (what, "the far pool differs from the compact one")
            hold_decode(oracle_mod, o_c, l_c, q, kvs, lens, causal, what)


@pytest.mark.parametrize("case,new_kind", [("M-F-append-bf16-pool", "bf16"), ("M-F-append-e4m3-pool", "bf16"), ("M-F-append-e4m3-pool", "f16")])
def test_appends_into_far_latent_pages_and_the_decode_behind_them(fa, oracle_mod, case, new_kind):
    """M-F: the aliased form the header prescribes -- Hkv = 1, D = 576, k_new == v_new, k_pages == v_pages -- into a sentinel-filled far pool:
    the byte copy in bf16, the quantising append from bf16 and from f16 rows in e4m3. Only the appended slots change, they hold byte for
    byte what the same append leaves in a compact pool, and with the older keys filled in by hand the decode on the appended far pool gives
    the bits of the same chain on the compact pool."""
    import torch

    plan = CASES[case]
    kind, P, rs, ps, lens, new, first = (plan[n] for n in ("kind", "P", "row_stride", "page_stride", "lens", "new", "first_page"))
    rng = np.random.default_rng(103)
    whole, _, table, kvs = latent_pool(rng, lens, P, kind)  # the pool laid out whole: the older keys are taken from it
    n_c = whole.shape[0]
    table_f = pool_table(plan, table)
    rows = np.concatenate([kv[L - n:] for kv, n, L in zip(kvs, new, lens)])
    k_new = to_dev(rows, new_kind).view(-1, 1, DQK)  # (the values of an e4m3 pool lie on the e4m3 grid: exact in bf16 and f16 too)
    cu = cu_dev(np.concatenate([[0], np.cumsum(new)]))
    sent = sentinel_of(kind)
    c_ints = torch.full((n_c * ps,), sent, dtype=getattr(torch, KIND[kind][1]), device="cuda")
    full_c = typed(c_ints, kind).view(n_c, P, rs)
    four = lambda full: full.as_strided((full.shape[0], P, 1, DQK), (ps, rs, DQK, 1))  # [num_pages, P, 1, 576]: NHD with one latent head
    old = torch.zeros(n_c, P, dtype=torch.bool, device="cuda")
    for b, (n, L) in enumerate(zip(new, lens)):
        for j in range(L - n):
            old[int(table[b, j // P]), j % P] = True
    with Arena() as a:
        f_ints, full_f, view_f = far_pool(a, plan, None, sentinel=True)
        fa.kv_append_paged(k_new, k_new, four(full_c), four(full_c), cu, cu_dev(table), cu_dev(lens), max(new), layout="NHD")
        fa.kv_append_paged(k_new, k_new, four(full_f), four(full_f), cu, cu_dev(table_f), cu_dev(lens), max(new), layout="NHD")
        torch.cuda.synchronize()
        assert bool((c_ints != sent).any()), (case, new_kind, "the append wrote nothing")
        assert torch.equal(f_ints[first * ps:(first + n_c) * ps], c_ints), (case, new_kind, "the far pages differ from the compact pool's")
        clean(f_ints, kind, plan.tensors["kv_pages"].blocks, (case, new_kind, "kv_pages"))
        appended = ~old & (bits(full_c)[:, :, 0] != sent)
        assert torch.equal(bits(full_c)[appended], bits(whole)[appended]), (case, new_kind, "the appended slots do not hold the new rows")
        for full in (full_c, full_f[first:first + n_c]):  # the older keys by hand, into both placements
            bits(full)[old] = bits(whole)[old]
        Hq, Nq, causal, wide = plan["calls"][1]
        q = mp.round_to(rng.uniform(-1.0, 1.0, (len(lens), Hq, Nq, DQK)).astype(np.float32), "bf16")
        qd = to_dev(q, "bf16")
        o_w, l_w = decode(fa, qd, whole, table, lens, causal, wide)
        o_c, l_c = decode(fa, qd, full_c, table, lens, causal, wide)
        o_f, l_f = decode(fa, qd, view_f, table_f, lens, causal, wide)
        assert same(o_c, o_w) and same(l_c, l_w), (case, new_kind, "the decode on the appended compact pool differs from the pool laid out whole")
        assert same(o_f, o_c) and same(l_f, l_c), (case, new_kind, "the decode on the appended far pages differs from the compact chain")
        hold_decode(oracle_mod, o_c, l_c, q, kvs, lens, causal, (case, new_kind, "decode after the append"))


@pytest.mark.parametrize("case", [n for n in CASES if n.startswith("M-H")])
def test_decode_q_and_o_far_through_their_batch_strides(fa, oracle_mod, case):
    """M-H: B = 2 with batch entry 1 lying 2^32 bytes plus 1 MiB behind entry 0, for q and independently for o; head-major and token-major
    (there o's rows are 576 apart: rows of 512 are written, never 576). Causal, Nq = 2."""
    import torch

    plan = CASES[case]
    call, B, Hq, Nq, P, lens = (plan[n] for n in ("call", "B", "Hq", "Nq", "P", "lens"))
    kind = "fp8" if call == "kv8" else "bf16"
    wide = {"one": False, "wide": True, "kv8": None}[call]
    rng = np.random.default_rng(107 + Hq)
    _, view, table, kvs = latent_pool(rng, lens, P, kind)
    q = mp.round_to(rng.uniform(-1.0, 1.0, (B, Hq, Nq, DQK)).astype(np.float32), "bf16")
    qc = to_dev(q, "bf16")
    if plan["token_major"]:
        qc = qc.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    tq, to = plan.tensors["q"], plan.tensors["o"]
    with Arena() as a:
        q_far = strided(a.ints("bf16", tq.numel, sentinel=False), "bf16", (B, Hq, Nq, DQK), plan["q_strides"] + (1,))
        q_far.copy_(qc)
        o_ints = a.ints("bf16", to.numel)
        o_far = strided(o_ints, "bf16", (B, Hq, Nq, DV), plan["o_strides"] + (1,))
        l_far = torch.full((B, Hq, Nq), float("nan"), device="cuda")
        o_c, l_c = decode(fa, qc, view, table, lens, True, wide)
        decode(fa, q_far, view, table, lens, True, wide, out=o_far, lse=l_far)
        assert same(o_far, o_c) and same(l_far, l_c), (case, "the far batch entry differs from the compact call")
        clean_t(o_ints, to, (case, "O"))
        hold_decode(oracle_mod, o_c, l_c, q, kvs, lens, True, (case,))


def test_wide_decode_workspace_above_2_31_floats(fa, oracle_mod):
    """M-G: 128 packed rows and B = 32768, where the workspace is 8.6 GB and S = 1 (taken from the library's size). All but three
    sequences are empty: their rows come back O = 0 exactly and LSE = -inf. The live ones lie where their workspace slots start past
    element 2^31 and their q and o rows past byte 2^32, and are held to fp64. The workspace is NaN-filled beforehand (the f32 sentinel
    is a NaN) with a guard behind it. No compact twin has this S, so there is no bit comparison here; two runs must agree."""
    import torch

    plan = CASES["M-G-wide-workspace"]
    B, Hq, Nq, P, S, rows16, live = (plan[n] for n in ("B", "Hq", "Nq", "P", "S", "rows16", "live"))
    need = fa.mla_decode_paged_wide_workspace_bytes(B, Hq, Nq, DV, P, plan["max_pages"])
    assert need == plan["workspace_bytes"] and need // (B * rows16 * (DV + 2) * 4) == S == 1 and need // 4 > (1 << 31)
    print(f"FAR M-G: B = {B}, rows16 = {rows16}, S = {S}, workspace {need / far.GIB:.2f} GiB")
    rng = np.random.default_rng(109)
    idx, lens_live = list(live), list(live.values())
    _, view, table_live, kvs = latent_pool(rng, lens_live, P, "bf16")
    spare = int(view.shape[0]) - 1
    table = np.full((B, plan["max_pages"]), spare, np.int32)
    table[idx] = table_live
    lens = np.zeros(B, np.int32)
    lens[idx] = lens_live
    q = mp.round_to(rng.uniform(-1.0, 1.0, (len(idx), Hq, Nq, DQK)).astype(np.float32), "bf16")
    tq, to = plan.tensors["q"], plan.tensors["o"]
    guard = 1 << 18
    with Arena() as a:
        q_far = strided(a.ints("bf16", tq.numel, sentinel=False), "bf16", (B, Hq, Nq, DQK), plan["q_strides"] + (1,))
        bits(q_far).zero_()  # the empty sequences' queries: defined values, read by nobody's result
        q_far[idx] = to_dev(q, "bf16")
        o_ints = a.ints("bf16", to.numel)
        o_far = strided(o_ints, "bf16", (B, Hq, Nq, DV), plan["o_strides"] + (1,))
        ws = a.ints("f32", need // 4 + guard)
        assert bool(torch.isnan(typed(ws, "f32")[:4]).all())
        l_far = torch.full((B, Hq, Nq), float("nan"), device="cuda")
        td, ld = cu_dev(table), cu_dev(lens)
        call = lambda out, lse: fa.flash_attention_mla_decode_paged(q_far, view, td, ld, DSCALE, is_causal=True, wide=True, out=out, lse=lse,
                                                                    workspace=ws.view(torch.uint8)[:need])
        call(o_far, l_far)
        torch.cuda.synchronize()
        assert bool((ws[need // 4:] == sentinel_of("f32")).all()), "the guard behind the workspace was written"
        clean_t(o_ints, to, ("M-G", "O"))
        dead = torch.ones(B, dtype=torch.bool, device="cuda")
        dead[idx] = False
        assert not bool(torch.isnan(l_far).any()) and bool(torch.isneginf(l_far[dead]).all()), "an empty sequence: LSE = -inf"
        touched = torch.stack([(bits(o_far[b0:b0 + 4096]) != 0).flatten(1).any(1) for b0 in range(0, B, 4096)]).flatten()
        assert not bool((touched & dead).any()), "an empty sequence: O = 0 exactly"
        o_live, l_live = o_far[idx].clone(), l_far[idx].clone()
        ws.fill_(sentinel_of("f32"))
        o_ints.fill_(sentinel_of("bf16"))
        call(o_far, l_far)
        torch.cuda.synchronize()
        assert same(o_far[idx], o_live) and same(l_far[idx], l_live), "two runs differ"
    hold_decode(oracle_mod, o_live, l_live, q, kvs, lens_live, True, ("M-G", "live sequences", idx))


# ---- M-A, M-B, M-C: the prefill and its backward ------------------------------------------------------------------------------------------------
_DATA = {}


def prefill_data(key, dtype, Hq, Hkv, lens):
    """A case of tests/mla_prefill.py's shape (so that its references and bars apply) plus dO; drawn once per key, read-only."""
    if key not in _DATA:
        rng = np.random.default_rng(113 + sum(map(ord, key)))
        tq, tk = sum(a for a, _ in lens), sum(b for _, b in lens)
        q, k, v, do = (mp.round_to(rng.uniform(-1.0, 1.0, s).astype(np.float32), dtype) for s in ((tq, Hq, PQK), (tk, Hkv, PQK), (tk, Hkv, PV), (tq, Hq, PV)))
        cu_q, cu_k = (np.concatenate([[0], np.cumsum(x)]).astype(np.int32) for x in ([a for a, _ in lens], [b for _, b in lens]))
        c = dict(name="far:" + key, heads=(Hq, Hkv), dtype=dtype, lens=tuple(lens), cu_q=cu_q, cu_k=cu_k, q=q, k=k, v=v, do=do,
                 max_q=max(a for a, _ in lens), max_k=max(b for _, b in lens))
        for x in (q, k, v, do):
            x.setflags(write=False)
        _DATA[key] = c
    return _DATA[key]


def compact(x, dtype, layout="THD", half=False):
    """The compact twin of [T, H, W] data in the far tensor's kind of view: token-major or head-major storage; half: the upper half of a
    buffer whose heads are 2 W wide (v of the kv up-projection)."""
    import torch

    t = to_dev(np.array(x, copy=True), dtype)  # (a copy: the shared data is read-only)
    T, H, W = t.shape
    if half:
        buf = torch.zeros((T, H, 2 * W) if layout == "THD" else (H, T, 2 * W), dtype=t.dtype, device="cuda")
        view = (buf if layout == "THD" else buf.permute(1, 0, 2))[:, :, W:]
        view.copy_(t)
        return view
    return t if layout == "THD" else t.permute(1, 0, 2).contiguous().permute(1, 0, 2)


def far_view(ints, kind, T, H, W, strides, base=0):
    return packed_view(ints, kind, T, H, W, *strides) if base == 0 else strided(ints, kind, (T, H, W), tuple(strides) + (1,), base)


def hold_prefill(c, o, lse, causal, what):
    return mp.check(o.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64), c, causal, ("FAR",) + tuple(what), PSCALE)


def hold_backward(c, b, grads, causal, what):
    """Sequence b of the compact gradients (dq, dk, dv packed [T, H, W]) inside the chain bound of tests/mla_bwd.py."""
    sb = mb.SeqBounds(*(x.transpose(1, 0, 2) for x in (c["q"][c["cu_q"][b]:c["cu_q"][b + 1]], c["k"][c["cu_k"][b]:c["cu_k"][b + 1]],
                                                      c["v"][c["cu_k"][b]:c["cu_k"][b + 1]], c["do"][c["cu_q"][b]:c["cu_q"][b + 1]])),
                      causal, PSCALE, c["dtype"], chain=True)
    cu = (c["cu_q"], c["cu_k"], c["cu_k"])
    got = [g[int(u[b]):int(u[b + 1])].cpu().numpy().astype(np.float64).transpose(1, 0, 2) for g, u in zip(grads, cu)]
    r = mb.worst_ratio(got, sb)
    print(f"FAR {what} seq {b}: worst backward error / chain bound {r:.3f}")
    assert r <= 1.0, (what, b, r)


def forward(fa, t, cu_q, cu_k, causal, **kw):
    import torch

    out = fa.flash_attention_varlen_mla(t["q"], t["k"], t["v"], cu_dev(cu_q), cu_dev(cu_k), far.L_SEQ, far.L_SEQ, is_causal=causal, scale=PSCALE, **kw)
    torch.cuda.synchronize()
    return out


def backward(fa, t, lse, cu_q, cu_k, causal, **kw):
    import torch

    g = fa.flash_attention_varlen_mla_backward(t["q"], t["k"], t["v"], t["o"], t["d_o"], lse, cu_dev(cu_q), cu_dev(cu_k), far.L_SEQ, far.L_SEQ,
                                               is_causal=causal, scale=PSCALE, **kw)
    torch.cuda.synchronize()
    return g


def packed_setup(case):
    plan = CASES[case]
    side, dtype, Hq, Hkv = (plan[n] for n in ("side", "dtype", "Hq", "Hkv"))
    lens_q, lens_k = (plan["lens_far"], plan["lens_near"]) if side == "q" else (plan["lens_near"], plan["lens_far"])
    c = prefill_data(f"packed-{side}-{dtype}", dtype, Hq, Hkv, list(zip(lens_q, lens_k)))
    cq_far, ck_far = (plan["cu_far"], list(c["cu_k"])) if side == "q" else (list(c["cu_q"]), plan["cu_far"])
    return plan, c, cq_far, ck_far


@pytest.mark.parametrize("case", [n for n in CASES if n.startswith("M-A")])
def test_packed_prefill_with_one_side_far(fa, case):
    """M-A: q and o (6 and 4 GiB), or k and v, far: each of the four under its own strides crosses byte 2^32 and element 2^31. bf16
    token-major, and f16 with head-major [H, total, D] views, where the head stride is the large one. On the kv side v is the upper half
    of a far buffer whose heads are 256 wide (head stride 256, base 128). Causal and full."""
    import torch

    plan, c, cq_far, ck_far = packed_setup(case)
    side, dtype, layout, Hq, Hkv, total, st, base = (plan[n] for n in ("side", "dtype", "layout", "Hq", "Hkv", "total", "strides", "base"))
    near = dict(q=compact(c["q"], dtype, layout), k=compact(c["k"], dtype, layout), v=compact(c["v"], dtype, layout, half=plan["half_v"]))
    with Arena() as a:
        big = dict(near)
        for n in (("q",) if side == "q" else ("k", "v")):
            H, W = (Hq if n == "q" else Hkv), far.MLA_ROW[n]
            big[n] = far_view(a.ints(dtype, plan.tensors[n].numel, sentinel=False), dtype, total, H, W, st[n], base[n])
            place(big[n], near[n], plan)
        kw = {}
        if side == "q":
            o_ints, l_ints = a.ints(dtype, plan.tensors["o"].numel), a.ints("f32", Hq * total)
            o_far, l_far = far_view(o_ints, dtype, total, Hq, PV, st["o"]), typed(l_ints, "f32").view(Hq, total)
            kw = dict(out=o_far, lse=l_far)
        for causal in (True, False):
            what = (case, "causal" if causal else "full")
            out_c = compact(np.zeros((len(c["q"]), Hq, PV), np.float32), dtype, layout)  # o in the layout of the far one
            o_c, l_c = forward(fa, near, c["cu_q"], c["cu_k"], causal, out=out_c)
            if side == "q":
                o_ints.fill_(sentinel_of(dtype))
                l_ints.fill_(sentinel_of("f32"))
            o_f, l_f = forward(fa, big, cq_far, ck_far, causal, **kw)
            if side == "q":
                o_f, l_f = gathered(o_f, plan), gathered(l_f, plan, 1)
            assert same(o_f, o_c), (what, "O of the far placement differs from the compact call")
            assert same(l_f, l_c), (what, "LSE of the far placement differs from the compact call")
            if side == "q":
                clean_t(o_ints, plan.tensors["o"], (what, "O"))
                clean(l_ints, "f32", lse_blocks(plan, Hq), (what, "LSE"))
            hold_prefill(c, o_c, l_c, causal, what)


@pytest.mark.parametrize("case", ["M-B-backward-q-far", "M-B-backward-kv-far"])
def test_packed_backward_with_one_side_far(fa, case):
    """M-B: the q side far -- q, o, d_o far loads, dq a far fp32 store past byte 2^33, 26 GiB -- or the kv side -- k and dk past 2^32 / 2^33
    bytes, v past 2^31, dv past 2^32, 20 GiB. The gradients are sentinel-filled: only owned rows change, 192 elements of dq and dk, 128
    of dv, nothing between heads. The backward runs on the forward's own O and LSE. (dv past 2^33: not covered, see far.mla_packed.)"""
    import torch

    plan, c, cq_far, ck_far = packed_setup(case)
    side, dtype, Hq, Hkv, total, st = (plan[n] for n in ("side", "dtype", "Hq", "Hkv", "total", "strides"))
    near = dict(q=compact(c["q"], dtype), k=compact(c["k"], dtype), v=compact(c["v"], dtype), d_o=compact(c["do"], dtype))
    names, gnames = (("q", "o", "d_o"), ("dq",)) if side == "q" else (("k", "v"), ("dk", "dv"))
    H = Hq if side == "q" else Hkv
    like = {"q": "q", "o": "o", "d_o": "o", "k": "k", "v": "v", "dq": "q", "dk": "k", "dv": "v"}
    with Arena() as a:
        big = {n: far_view(a.ints(dtype, plan.tensors[n].numel, sentinel=False), dtype, total, H, far.MLA_ROW[n], st[like[n]]) for n in names}
        for n in names:
            if n != "o":
                place(big[n], near[n], plan)
        g_ints = {n: a.ints("f32", plan.tensors[n].numel) for n in gnames}
        g_far = {n: far_view(g_ints[n], "f32", total, H, far.MLA_ROW[n], st[like[n]]) for n in gnames}
        l_far = torch.empty(Hq, total, dtype=torch.float32, device="cuda") if side == "q" else None
        for causal in (True, False):
            what = (case, "causal" if causal else "full")
            o_c, l_c = forward(fa, near, c["cu_q"], c["cu_k"], causal)
            g_c = backward(fa, {**near, "o": o_c}, l_c, c["cu_q"], c["cu_k"], causal)
            if side == "q":
                place(big["o"], o_c, plan)
                place(l_far, l_c, plan, 1)
                t, lse = {**near, **big}, l_far
            else:
                t, lse = {**near, **big, "o": o_c}, l_c
            for n in gnames:
                g_ints[n].fill_(sentinel_of("f32"))
            g_f = backward(fa, t, lse, cq_far, ck_far, causal, **g_far)
            for i, n in enumerate(("dq", "dk", "dv")):
                got = gathered(g_f[i], plan) if n in gnames else g_f[i]
                assert same(got, g_c[i]), (what, n + " of the far placement differs from the compact call", float((got - g_c[i]).abs().max()))
            for n in gnames:
                clean_t(g_ints[n], plan.tensors[n], (what, n))
            hold_backward(c, 1, g_c, causal, what)  # one sequence held to the fp64 reference: the one that lies far


def wide_setup(case):
    plan = CASES[case]
    dtype, Hq, Hkv, L = (plan[n] for n in ("dtype", "Hq", "Hkv", "L"))
    c = prefill_data(f"wide-{dtype}", dtype, Hq, Hkv, [(L, L)])
    near = dict(q=compact(c["q"], dtype), k=compact(c["k"], dtype), v=compact(c["v"], dtype, half=True), d_o=compact(c["do"], dtype))
    return plan, c, near


def wide_view(a, plan, n, kind=None, sentinel=False):
    """(ints, view) of tensor n of a wide case under the stride pair of the tensor it is addressed like"""
    like = {"d_o": "o", "dq": "q", "dk": "k", "dv": "v"}.get(n, n)
    H = plan["Hq"] if like in "qo" else plan["Hkv"]
    ints = a.ints(kind or plan["dtype"], plan.tensors[n].numel, sentinel=sentinel)
    return ints, far_view(ints, kind or plan["dtype"], plan["L"], H, far.MLA_ROW[n], plan["strides"][like], plan["base"][like])


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_wide_rows_prefill(fa, dtype):
    """M-C, forward: one sequence of 300 rows under FOUR different row strides near 2^22 (q, k, v, o), v a 128-offset half-view: rows
    >= 256 start past byte 2^31. A load or store made under a neighbour's stride lands between the rows."""
    case = f"M-C-wide-forward-{dtype}"
    plan, c, near = wide_setup(case)
    with Arena() as a:
        big = {}
        for n in ("q", "k", "v"):
            _, big[n] = wide_view(a, plan, n)
            big[n].copy_(near[n])
        o_ints, o_far = wide_view(a, plan, "o", sentinel=True)
        for causal in (True, False):
            what = (case, "causal" if causal else "full")
            o_c, l_c = forward(fa, near, c["cu_q"], c["cu_k"], causal)
            o_ints.fill_(sentinel_of(dtype))
            o_f, l_f = forward(fa, big, c["cu_q"], c["cu_k"], causal, out=o_far)
            assert same(o_f, o_c) and same(l_f, l_c), (what, "the wide placement differs from the compact call")
            clean_t(o_ints, plan.tensors["o"], (what, "O"))
            hold_prefill(c, o_c, l_c, causal, what)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("side", ["q", "kv"])
def test_wide_rows_backward(fa, side, dtype):
    """M-C, backward, one side wide at a time: q, o, d_o and dq, or k, v, dk and dv, each under its own row stride; fp32 rows >= 128 start
    past byte 2^31 and rows >= 256 past 2^32. dv is a 128-offset half-view of an fp32 buffer: its footprint is taken with base = 128."""
    case = f"M-C-wide-backward-{side}-{dtype}"
    plan, c, near = wide_setup(case)
    names, gnames = (("q", "o", "d_o"), ("dq",)) if side == "q" else (("k", "v"), ("dk", "dv"))
    with Arena() as a:
        big, g_ints, g_far = {}, {}, {}
        for n in names:
            _, big[n] = wide_view(a, plan, n)
            if n != "o":
                big[n].copy_(near[n])
        for n in gnames:
            g_ints[n], g_far[n] = wide_view(a, plan, n, kind="f32", sentinel=True)
        for causal in (True, False):
            what = (case, "causal" if causal else "full")
            o_c, l_c = forward(fa, near, c["cu_q"], c["cu_k"], causal)
            g_c = backward(fa, {**near, "o": o_c}, l_c, c["cu_q"], c["cu_k"], causal)
            if side == "q":
                big["o"].copy_(o_c)
            for n in gnames:
                g_ints[n].fill_(sentinel_of("f32"))
            g_f = backward(fa, {**near, "o": o_c, **big}, l_c, c["cu_q"], c["cu_k"], causal, **g_far)
            for i, n in enumerate(("dq", "dk", "dv")):
                assert same(g_f[i], g_c[i]), (what, n + " of the wide placement differs from the compact call")
            for n in gnames:
                clean_t(g_ints[n], plan.tensors[n], (what, n))
            hold_backward(c, 0, g_c, causal, what)
