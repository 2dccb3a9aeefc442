"""CPU: the far-address cases are what they claim to be (tests/far.py), and the footprint checker sees what it must.

  * every case of both catalogues (cases(), and mla_cases() of the MLA family: tests/test_far_cases_mla.py holds what is particular to
    it) crosses the thresholds it names: asserted from the planner's integers, re-derived here row by row;
  * every planned call satisfies the host rules of include/fa_mi355.h, and the restated rules refuse what the library refuses;
  * the checker on small CPU tensors under a wrap modulus of 2^16: a clean footprint passes; a row stored at its offset modulo the
    modulus, a row stored at the offset of a sign-extended 16-bit product, one stray element between two rows under a wide stride and
    an owned far row left untouched are each reported at the right position."""
import numpy as np
import pytest

import far

CASES = far.cases()
MLA = far.mla_cases()
ALL = {**CASES, **MLA}
SENTINEL = 0x7FA5


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL))
def test_case_crosses_what_it_claims(name):
    plan = ALL[name]
    assert plan.claims, name
    for tname, unit, threshold in plan.claims:
        t = plan.tensors[tname]
        per = t.itemsize if unit == "byte" else 1
        # the last element of the last row of every block, from the block's own integers
        last = max((s + (n - 1) * p + ln - 1) for s, n, ln, p in t.blocks) - t.base  # (offsets count from the element the pointer names)
        assert last == t.hi_elem and (last * per + per - 1 if unit == "byte" else last) >= threshold, (name, tname, unit, threshold, last)
        # ... and not by a row's tail alone: whole rows START at or past the threshold
        assert t.rows_at_or_past(unit, threshold) >= 1, (name, tname, unit, threshold)
        assert (unit, threshold) in t.crossings()
        assert t.numel * t.itemsize > threshold * (1 if unit == "byte" else t.itemsize) - t.itemsize, (name, tname, "the allocation is that large")


@pytest.mark.parametrize("name", list(ALL))
def test_case_is_legal_and_fits(name):
    plan = ALL[name]
    assert plan.rules and plan.legal(), (name, [text for text, ok in plan.rules if not ok])
    for t in plan.tensors.values():  # rows disjoint inside a block, every row inside the allocation
        assert all(p >= ln or n == 1 for _, n, ln, p in t.blocks) and 0 <= t.lo_elem <= t.hi_elem < t.numel - t.base, (name, t.name)
    assert plan.device_bytes() < 30 * far.GIB, (name, plan.device_bytes() / far.GIB)  # under 32 GiB with the compact twins


def test_rows_at_or_past_counts_rows():
    t = far.Tensor("x", "bf16", 1 << 20, "store", [(100, 50, 8, 1000), (60000, 1, 8, 8)])
    brute = lambda unit, th: sum(1 for s, n, ln, p in t.blocks for i in range(n) if (s + i * p) * (2 if unit == "byte" else 1) >= th)
    for unit in ("byte", "elem"):
        for th in (0, 99, 100, 101, 1100, 1101, 49100, 49101, 60000, 98201, 120000, 120001):
            assert t.rows_at_or_past(unit, th) == brute(unit, th), (unit, th)


def test_the_catalogue_covers_the_thresholds_of_the_issue():
    crossed = {(t.role, t.kind, c) for p in CASES.values() for t in p.tensors.values() for c in t.crossings()}
    assert ("store", "bf16", ("byte", 1 << 32)) in crossed and ("store", "bf16", ("elem", 1 << 31)) in crossed  # A: O
    assert ("store", "f32", ("byte", 1 << 33)) in crossed and ("load", "bf16", ("byte", 1 << 32)) in crossed    # B
    assert ("load", "fp8", ("elem", 1 << 32)) in crossed and ("store", "fp8", ("elem", 1 << 32)) in crossed     # D, F
    assert ("load", "bf16", ("elem", 1 << 32)) in crossed and ("store", "bf16", ("elem", 1 << 32)) in crossed   # E, F
    assert ("store", "f32", ("elem", 1 << 31)) in crossed                                                       # G


def test_wide_rows_cross_where_the_issue_says():
    """Case C: 16-bit rows >= 256 start at >= 2^31 bytes; fp32 rows >= 128 at >= 2^31 and rows >= 256 at >= 2^32; nothing reaches 2^32 in 16 bits."""
    for dtype in ("bf16", "f16"):
        fwd, bq, bk = (CASES[f"C-wide-{n}-{dtype}"] for n in ("forward", "backward-q", "backward-kv"))
        Hq, Hkv = fwd["Hq"], fwd["Hkv"]
        for t, H in ((fwd.tensors["o"], Hq), (fwd.tensors["k"], Hkv), (bq.tensors["d_o"], Hq)):
            assert t.rows_at_or_past("byte", 1 << 31) == (300 - 256) * H and not t.crosses("byte", 1 << 32)
        for t, H in ((bq.tensors["dq"], Hq), (bk.tensors["dk"], Hkv), (bk.tensors["dv"], Hkv)):
            assert t.rows_at_or_past("byte", 1 << 31) == (300 - 128) * H and t.rows_at_or_past("byte", 1 << 32) == (300 - 256) * H
        assert (300 + 128) * far.WIDE_STRIDE * 2 < (1 << 32)


def test_the_restated_rules_refuse_what_the_library_refuses():
    assert not far.sequence_rule("q", 300, 1 << 23)[0][1] and far.sequence_rule("q", 300, 1 << 22)[0][1]
    big_rows = (1 << 32) // (64 * 2) - 64  # tests/test_varlen_abi.py: 4 GiB minus one tile at row pitch 64 is refused
    assert not far.sequence_rule("q", big_rows, 64)[0][1]
    assert not far.stride_rules("q", 2052, 128, 128)[0][1] and not far.stride_rules("q", 64, 64, 128)[0][1]
    assert not far.stride_rules("kv8", 136, 136, 128, itemsize=1)[0][1] and far.stride_rules("kv8", 144, 144, 128, itemsize=1)[0][1]
    ok = lambda rules: all(r[1] for r in rules)
    assert not ok(far.pool_rules(256, 128, 1 << 31, 1 << 23, 1 << 23, 2, 4)) and ok(far.pool_rules(256, 128, 1 << 29, 1 << 21, 1 << 21, 2, 4))
    assert not ok(far.pool_rules(256, 128, 1 << 31, 1 << 23, 1 << 23, 1, 4)) and ok(far.pool_rules(256, 128, 1 << 30, 1 << 22, 1 << 22, 1, 4))
    assert not ok(far.pool_rules(256, 128, 1 << 18, 1 << 15, 128, 2, (1 << 22) + 1))  # capacity above 2^30
    assert not far.grid_rule(1 << 31)[0][1]


def test_the_table_of_crossings_prints():
    lines = [ln for p in CASES.values() for ln in p.table()]
    print("\n".join(lines))
    assert any("claimed: byte 2^33" in ln for ln in lines) and any("claimed: byte 2^32, elem 2^32" in ln for ln in lines)


# ---- the checker ---------------------------------------------------------------------------------------------------------------------------
MOD, BASE, PITCH, ROW, ROWS = 1 << 16, 40000, 1000, 64, 150  # offsets reach 149064: past twice the modulus; sign-extension reaches back 32768
BLOCKS = [(BASE, ROWS, ROW, PITCH)]


def fresh():
    import torch

    return torch.full((BASE + ROWS * PITCH + 500,), SENTINEL, dtype=torch.int16)


def store(buf, row, at=None):
    """What a kernel leaves of row `row`, at element offset `at` from the base (default: where it belongs)."""
    import torch

    at = row * PITCH if at is None else at
    buf[BASE + at:BASE + at + ROW] = torch.arange(ROW, dtype=torch.int16) + row


def sext16(x):
    return ((x & 0xFFFF) ^ 0x8000) - 0x8000


@pytest.mark.parametrize("chunk", [1 << 27, 4999, 64])
def test_a_clean_footprint_passes(chunk):
    buf = fresh()
    for r in range(ROWS):
        store(buf, r)
    rep = far.footprint(buf, SENTINEL, BLOCKS, modulus=MOD, base=BASE, chunk=chunk)
    assert rep.ok and rep.describe() == "clean"


@pytest.mark.parametrize("chunk", [1 << 27, 4999])
def test_a_row_stored_modulo_the_modulus_is_named(chunk):
    row = 140
    off = row * PITCH
    assert off >= 2 * MOD and (off % MOD) % PITCH >= ROW  # far, and the wrapped place lies between two rows
    buf = fresh()
    for r in range(ROWS):
        store(buf, r, off % MOD if r == row else None)
    rep = far.footprint(buf, SENTINEL, BLOCKS, modulus=MOD, base=BASE, chunk=chunk)
    assert not rep.ok
    assert rep.untouched == [(BASE + off, off, off % MOD, True)]
    assert rep.outside_count == ROW and rep.outside == list(range(BASE + off % MOD, BASE + off % MOD + ROW))
    assert "a wrapped store" in rep.describe() and str(off % MOD) in rep.describe()


def test_a_row_stored_at_a_sign_extended_product_is_reported():
    row = 50
    off = row * PITCH  # 50000: negative as a signed 16-bit product
    wrong = sext16(off)
    assert wrong == off - MOD and BASE + wrong >= 0
    buf = fresh()
    for r in range(ROWS):
        store(buf, r, wrong if r == row else None)
    rep = far.footprint(buf, SENTINEL, BLOCKS, modulus=MOD, base=BASE, chunk=4999)
    assert [u[:2] for u in rep.untouched] == [(BASE + off, off)] and rep.untouched[0][2] is None  # a near row: no wrap to look for
    assert rep.outside_count == ROW and rep.outside == list(range(BASE + wrong, BASE + wrong + ROW))


def test_one_stray_element_between_two_rows_is_reported():
    buf = fresh()
    for r in range(ROWS):
        store(buf, r)
    stray = BASE + 77 * PITCH + ROW  # the first element behind row 77
    buf[stray] = 0
    rep = far.footprint(buf, SENTINEL, BLOCKS, modulus=MOD, base=BASE, chunk=4999)
    assert not rep.untouched and rep.outside_count == 1 and rep.outside == [stray]
    buf[stray] = SENTINEL
    buf[BASE - 1] = 0  # ... and the element in front of the base
    rep = far.footprint(buf, SENTINEL, BLOCKS, modulus=MOD, base=BASE, chunk=4999)
    assert rep.outside == [BASE - 1]


def test_an_untouched_far_row_is_reported_with_its_wrapped_offset():
    row = 149
    off = row * PITCH
    buf = fresh()
    for r in range(ROWS - 1):
        store(buf, r)
    rep = far.footprint(buf, SENTINEL, BLOCKS, modulus=MOD, base=BASE, chunk=4999)
    assert rep.outside_count == 0 and rep.untouched == [(BASE + off, off, off % MOD, False)]
    assert "nothing written there either" in rep.describe()


def test_blocks_of_single_rows_and_several_blocks():
    import torch

    buf = torch.full((5000,), 0x5A, dtype=torch.uint8)
    blocks = [(10, 1, 100, 100), (200, 4, 16, 32), (4000, 3, 8, 8)]
    for s, n, ln, p in blocks:
        for i in range(n):
            buf[s + i * p:s + i * p + ln] = 1
    assert far.footprint(buf, 0x5A, blocks, modulus=1 << 12, chunk=150).ok
    buf[216] = 1
    buf[4008:4016] = 0x5A
    rep = far.footprint(buf, 0x5A, blocks, modulus=1 << 12, chunk=150)
    assert rep.outside == [216] and [u[0] for u in rep.untouched] == [4008]
