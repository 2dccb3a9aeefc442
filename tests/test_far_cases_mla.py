"""CPU: the far-address cases of the MLA family (tests/far.py, mla_cases()) beyond what tests/test_far_cases.py holds for every case.

  * the catalogue covers what it must: each of q, k, v, o of the prefill, the latent pool, the decode's q and o, the decode workspace, dq
    and dk is claimed past byte 2^32 (2^33 in fp32) in some case, dv past 2^32; the wide rows lie where the case says, under four
    different row strides; the workspace of case M-G is the size the library asks for;
  * the restated MLA rules refuse what the library refuses and nothing else: through the C ABI, which validates before any launch (fake
    aligned pointers), one value just inside and one just outside each rule. A value inside passes on to the last rule before the launch,
    which is broken on purpose ("grid too large"), so nothing launches;
  * the footprint checker with base != 0 (a half-view of a wider buffer): a row stored at its offset modulo the modulus MEASURED FROM THE
    BASE is named, and rows stored under a neighbour's pitch are reported where a brute-force walk finds them."""
import numpy as np
import pytest

import far
from test_mla_abi import BF16, FP8, fa, lib, mla_call as one_call  # noqa: F401  (fa, lib: fixtures)
from test_mla_bwd_abi import bwd_call
from test_mla_kv8_abi import kv8_call
from test_mla_prefill_abi import mla_call as prefill_call
from test_mla_wide_abi import wide_call

MLA = far.mla_cases()
ok = lambda rules: all(r[1] for r in rules)


# ---- the catalogue -------------------------------------------------------------------------------------------------------------------------
def claimed(tensor, unit, threshold, prefix):
    return [p.name for p in MLA.values() if p.name.startswith(prefix) and (tensor, unit, threshold) in p.claims]


def test_the_mla_catalogue_covers_the_thresholds_of_the_issue():
    for t in ("q", "k", "v", "o"):  # the prefill's four tensors, each under its own strides
        assert claimed(t, "byte", 1 << 32, "M-A") and claimed(t, "elem", 1 << 31, "M-A"), t
    assert claimed("kv_pages", "byte", 1 << 32, "M-D") and claimed("kv_pages", "elem", 1 << 32, "M-D")  # loads from far latent pages
    assert claimed("kv_pages", "elem", 1 << 32, "M-F")                                                   # ... and appends into them
    assert {MLA[n]["kind"] for n in claimed("kv_pages", "elem", 1 << 32, "M-D")} == {"bf16", "fp8"}
    for call in ("one", "wide", "kv8"):  # the decode's q and o through their batch strides, per call
        assert claimed("q", "byte", 1 << 32, f"M-H-decode-{call}") and claimed("o", "byte", 1 << 32, f"M-H-decode-{call}"), call
    assert claimed("workspace", "elem", 1 << 31, "M-G") and claimed("workspace", "byte", 1 << 33, "M-G")
    assert claimed("dq", "byte", 1 << 33, "M-B") and claimed("dk", "byte", 1 << 33, "M-B") and claimed("dv", "byte", 1 << 32, "M-B")
    # the gap the catalogue states: no case takes dv past 2^33 (it does not fit under the peak limit)
    assert not any(t.name == "dv" and t.crosses("byte", 1 << 33) for p in MLA.values() for t in p.tensors.values())
    # every claim is one the integers bear out (tests/test_far_cases.py re-derives them row by row)
    for p in MLA.values():
        assert all((u, th) in p.tensors[n].crossings() for n, u, th in p.claims), p.name


def test_the_row_counts_of_the_pool_cases():
    rows = lambda kind: [(h * n, wide) for h, n, _, wide in far.MLA_POOL_CALLS[kind]]
    assert rows("bf16") == [(16, False), (32, False), (32, True), (33, True), (128, True)] and rows("fp8") == [(16, None), (33, None), (128, None)]
    for kind in ("bf16", "fp8"):
        assert any(causal and n == 2 for _, n, causal, _ in far.MLA_POOL_CALLS[kind])
    pad = MLA["M-D-bf16-pool-padded"]
    assert pad["row_stride"] == 640 and pad["page_stride"] == 257 * 640
    for name in ("M-D-bf16-pool", "M-D-bf16-pool-padded", "M-D-e4m3-pool"):
        p = MLA[name]
        assert p["first_page"] * p["page_stride"] >= (1 << 32) + 2 * p["page_stride"] and p["first_page"] + p["used_pages"] < p["num_pages"]
        assert p.device_bytes() <= (17 if p["kind"] == "bf16" else 9) << 29


def test_mla_wide_rows_cross_where_the_issue_says():
    """Case M-C: four different legal row strides; 16-bit rows >= 256 start at >= 2^31 bytes, fp32 rows >= 128 at >= 2^31 and rows >= 256
    at >= 2^32; nothing reaches 2^32 bytes in 16 bits; v and dv are counted from their base, 128 elements into the buffer."""
    st = far.MLA_WIDE_STRIDES
    assert len(set(st.values())) == 4 and all(s % 8 == 0 and s >= (1 << 22) and (300 + 128) * s * 2 < (1 << 32) for s in st.values())
    for dtype in ("bf16", "f16"):
        fwd, bq, bk = (MLA[f"M-C-wide-{n}-{dtype}"] for n in ("forward", "backward-q", "backward-kv"))
        Hq, Hkv = fwd["Hq"], fwd["Hkv"]
        for t, H in ((fwd.tensors["q"], Hq), (fwd.tensors["o"], Hq), (fwd.tensors["k"], Hkv), (fwd.tensors["v"], Hkv), (bq.tensors["d_o"], Hq)):
            assert t.rows_at_or_past("byte", 1 << 31) == (300 - 256) * H and not t.crosses("byte", 1 << 32), t.name
        for t, H in ((bq.tensors["dq"], Hq), (bk.tensors["dk"], Hkv), (bk.tensors["dv"], Hkv)):
            assert t.rows_at_or_past("byte", 1 << 31) == (300 - 128) * H and t.rows_at_or_past("byte", 1 << 32) == (300 - 256) * H, t.name
            assert t.hi_byte < 5 * far.GIB
        for plan in (fwd, bk):
            for n in ("v", "dv"):
                if n in plan.tensors:
                    t = plan.tensors[n]
                    assert t.base == 128 and t.lo_elem == 0 and t.blocks[0][0] == 128 and t.blocks[1][0] == 128 + 256


def test_the_workspace_of_case_g_is_what_the_library_asks_for(lib):
    p = MLA["M-G-wide-workspace"]
    need = lib.fa_fwd_mla_decode_paged_wide_workspace_bytes(p["B"], p["Hq"], p["Nq"], 512, p["P"], p["max_pages"])
    assert need == p["workspace_bytes"] and need // (p["B"] * p["rows16"] * 514 * 4) == p["S"] == 1  # S from the size, not from the split rule
    assert p["rows16"] == 128 and p["B"] == 32768  # neither was shrunk: the grid rule and the peak limit admit the shape
    assert need // 4 > (1 << 31) and need > (1 << 33)


# ---- the restated rules against the library ------------------------------------------------------------------------------------------------
GRID = dict(B=1 << 23, Hq=1 << 8, Hkv=1 << 8)   # the prefill's last rule before the launch, broken
DGRID = dict(B=1 << 23, wsb=1 << 60)            # ... and the decode's


def said(lib, status, word):
    msg = lib.fa_last_error().decode()
    assert status == -1 and word in msg, (status, msg)


@pytest.mark.parametrize("call", [prefill_call, bwd_call], ids=["forward", "backward"])
@pytest.mark.parametrize("t", ["q", "k", "v", "o"])
def test_the_prefill_rules_per_tensor_refuse_what_the_library_refuses(lib, call, t):
    d = far.MLA_ROW[t]
    good = {"q": (8 * 192, 192), "k": (2 * 192, 192), "v": (2 * 128, 128), "o": (8 * 128, 128)}[t]
    rows = (400 if t in "qo" else 500)  # the calls' max_seqlen_q / max_seqlen_k
    edge = (-(-(1 << 31) // (rows + 128)) + 7) // 8 * 8  # the smallest legal-looking row stride that reaches 4 GiB
    # the sequence rule, per tensor: one stride outside, one inside
    assert not ok(far.sequence_rule(t, rows, edge)) and ok(far.sequence_rule(t, rows, edge - 8))
    said(lib, call(lib, strides={t: (edge, good[1])}), "one head exceeds 4 GiB")
    said(lib, call(lib, strides={t: (edge - 8, good[1])}, **GRID), "grid too large")
    # the stride pair: a row of the tensor's own width, multiples of 8
    for pair, legal in (((d, d), True), ((d - 8, good[1]), False), ((good[0], d - 8), False), ((good[0] + 4, good[1]), False),
                        ((good[0] + 8, good[1]), True), ((good[0], good[1] + 4), False)):
        assert ok(far.stride_rules(t, *pair, d)) == legal, (t, pair)
        said(lib, call(lib, strides={t: pair}, **(GRID if legal else {})), "grid too large" if legal else "strides")
    # a stride that is legal for q or k (192) is not for v or o (128) and the other way round: the rule is the tensor's own
    assert ok(far.stride_rules(t, 128, 128, d)) == (d == 128)
    said(lib, call(lib, strides={t: (128, 128)}, **GRID), "grid too large" if d == 128 else "strides")
    # prefill_rules: all four at once, and the grid
    st = {"q": (8 * 192, 192), "k": (2 * 192, 192), "v": (2 * 128, 128), "o": (8 * 128, 128)}
    assert ok(far.prefill_rules(st, 400, 500, 700, 900, 3, 8)) and not ok(far.prefill_rules({**st, t: (edge, good[1])}, 400, 500, 700, 900, 3, 8))
    assert not ok(far.prefill_rules(st, 400, 500, 700, 900, 1 << 23, 1 << 8)) and not ok(far.prefill_rules(st, 701, 500, 700, 900, 3, 8))


@pytest.mark.parametrize("call,isz", [(one_call, 2), (wide_call, 2), (kv8_call, 1)], ids=["one", "wide", "kv8"])
def test_the_latent_pool_rules_refuse_what_the_library_refuses(lib, call, isz):
    unit = 16 if isz == 1 else 8
    P = 256
    rules = lambda krs, kps=None, mp=8: far.latent_pool_rules(P, P * krs if kps is None else kps, krs, isz, mp)

    def lib_says(legal, word, **kw):
        said(lib, call(lib, P_=P, **kw, **(DGRID if legal else {})), "grid too large" if legal else word)
    # one page below 2^31 bytes
    edge = (1 << 31) // (P * isz)
    assert not ok(rules(edge)) and ok(rules(edge - unit))
    lib_says(False, "one page of one head exceeds 2 GiB", krs=edge, kps=P * edge)
    lib_says(True, "", krs=edge - unit, kps=P * (edge - unit))
    # strides at least 576 and multiples of 8 (16 for e4m3)
    for krs, legal in ((576, True), (576 - unit, False), (576 + unit // 2, False), (576 + unit, True), (640, True)):
        assert ok(rules(krs)) == legal, krs
        lib_says(legal, "bad page strides", krs=krs, kps=P * krs)
    assert not ok(rules(576, kps=P * 576 + unit // 2)) and ok(rules(576, kps=(P + 1) * 576)) and not ok(rules(576, kps=568 if isz == 2 else 560))
    lib_says(False, "bad page strides", kps=P * 576 + unit // 2)
    lib_says(True, "", kps=(P + 1) * 576)
    lib_says(False, "bad page strides", kps=568 if isz == 2 else 560)
    if isz == 1:  # a multiple of 8 that is no multiple of 16: legal for a 16-bit pool only
        assert not ok(rules(584)) and ok(far.latent_pool_rules(P, P * 584, 584, 2, 8))
    # capacity at most 2^30 keys
    mp = (1 << 30) // P
    assert ok(rules(576, mp=mp)) and not ok(rules(576, mp=mp + 1))
    lib_says(True, "", max_pages=mp, bts=mp)
    said(lib, call(lib, P_=P, max_pages=mp + 1, bts=mp + 1, wsb=1 << 60), "capacity above 2^30 keys")


@pytest.mark.parametrize("call", [one_call, wide_call, kv8_call], ids=["one", "wide", "kv8"])
def test_the_decode_stride_and_grid_rules_refuse_what_the_library_refuses(lib, call):
    Hq, Nq = 16, 2
    for what, D, key in (("q", 576, "qs"), ("o", 512, "os_")):
        good = (Hq * Nq * D, Nq * D, D)
        for st, legal in ((good, True), ((good[0], good[1], D - 8), False), ((good[0], D - 8, Hq * D), False), ((D - 8, good[1], D), False),
                          ((good[0] + 4, good[1], D), False), ((good[0], good[1] + 4, D), False), ((good[0], good[1], D + 4), False),
                          (((1 << 31) + (1 << 19), good[1], D), True), ((good[0], D, Hq * D), True), ((-8, good[1], D), False)):
            assert ok(far.decode_stride_rules(what, 2, D, *st)) == legal, (what, st)
            said(lib, call(lib, **{key: st}, **(DGRID if legal else {})), "grid too large" if legal else "strides")
        # B = 1: any batch stride >= 0, multiples of 8 still
        assert ok(far.decode_stride_rules(what, 1, D, 0, good[1], D)) and not ok(far.decode_stride_rules(what, 2, D, 0, good[1], D))
        said(lib, call(lib, B=2, **{key: (0, good[1], D)}), "strides")
    # the grid: B * 256 * rblk fits an int (rblk = 2 here). The inside of this rule is the launch itself: it is not called here.
    edge = (1 << 31) // (256 * 2)
    assert not ok(far.decode_grid_rule(edge, Hq, Nq)) and ok(far.decode_grid_rule(edge - 1, Hq, Nq))
    said(lib, call(lib, B=edge, wsb=1 << 60), "grid too large")
    for p in MLA.values():  # ... and the cases' own shapes pass it
        if "Nq" in p.scalars:
            assert ok(far.decode_grid_rule(p["B"], p["Hq"], p["Nq"])), p.name


# ---- the checker with base != 0 ------------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FA5
MOD, BASE, HS, PITCH, NEIGHBOUR, ROW, ROWS, H = 1 << 16, 128, 256, 1200, 1216, 128, 150, 2  # v's half-view: heads 256 wide, base 128
BLOCKS = [(BASE + h * HS, ROWS, ROW, PITCH) for h in range(H)]


def fresh():
    import torch

    return torch.full((ROWS * PITCH + 600,), SENTINEL, dtype=torch.int16)


def store(buf, h, row, at=None):
    """What a kernel leaves of row `row` of head h, at element offset `at` FROM THE BASE (default: where it belongs)."""
    import torch

    at = row * PITCH + h * HS if at is None else at
    buf[BASE + at:BASE + at + ROW] = torch.arange(ROW, dtype=torch.int16) + row


def test_a_clean_footprint_with_a_base_passes():
    buf = fresh()
    for h in range(H):
        for r in range(ROWS):
            store(buf, h, r)
    assert far.footprint(buf, SENTINEL, BLOCKS, modulus=MOD, base=BASE, chunk=4999).ok
    assert bool((buf[:BASE] == SENTINEL).all())  # the lower half of head 0 of row 0 (k's nope part in the real layout) is not the call's


@pytest.mark.parametrize("chunk", [1 << 27, 4999])
def test_a_row_stored_modulo_the_modulus_from_the_base_is_named(chunk):
    h, row = 0, 140
    off = row * PITCH + h * HS  # from the base
    w = off % MOD
    assert off >= 2 * MOD and all((w - hh * HS) % PITCH >= ROW and (w - hh * HS) % PITCH + ROW <= PITCH for hh in range(H))  # between rows
    buf = fresh()
    for hh in range(H):
        for r in range(ROWS):
            store(buf, hh, r, w if (hh, r) == (h, row) else None)
    rep = far.footprint(buf, SENTINEL, BLOCKS, modulus=MOD, base=BASE, chunk=chunk, keep=ROW)
    assert rep.untouched == [(BASE + off, off, w, True)], rep.describe()
    assert rep.outside_count == ROW and rep.outside == list(range(BASE + w, BASE + w + ROW))
    assert "a wrapped store" in rep.describe() and str(w) in rep.describe()


@pytest.mark.parametrize("chunk", [1 << 27, 4999])
def test_rows_stored_under_a_neighbours_pitch_are_reported(chunk):
    """Head 0's rows stored at row * NEIGHBOUR (another tensor's row stride) in place of row * PITCH: the report is a brute-force walk's."""
    buf = fresh()
    for r in range(ROWS):
        store(buf, 1, r)
        if BASE + r * NEIGHBOUR + ROW <= buf.numel():
            store(buf, 0, r, r * NEIGHBOUR)
    written = (buf != SENTINEL).numpy()
    owned = np.zeros_like(written)
    starts = [s + i * p for s, n, _, p in BLOCKS for i in range(n)]
    for s in starts:
        owned[s:s + ROW] = True
    want_outside = np.flatnonzero(written & ~owned)
    want_untouched = sorted(s for s in starts if not written[s:s + ROW].any())
    assert len(want_outside) > ROW and len(want_untouched) > ROWS // 2  # most of head 0 is missing, and it shows between the rows
    rep = far.footprint(buf, SENTINEL, BLOCKS, modulus=MOD, base=BASE, chunk=chunk, keep=1 << 20)
    assert not rep.ok and rep.outside_count == len(want_outside) and rep.outside == want_outside.tolist()
    assert sorted(u[0] for u in rep.untouched) == want_untouched
    assert all(u[1] == u[0] - BASE for u in rep.untouched)


def test_the_mla_table_of_crossings_prints():
    lines = [ln for p in MLA.values() for ln in p.table()]
    print("\n".join(lines))
    assert any("dq" in ln and "claimed: byte 2^33" in ln for ln in lines) and any("kv_pages" in ln and "claimed: byte 2^32, elem 2^32" in ln for ln in lines)
    assert any("dv" in ln and "claimed: byte 2^32" in ln for ln in lines) and any("workspace" in ln and "claimed: elem 2^31, byte 2^33" in ln for ln in lines)
