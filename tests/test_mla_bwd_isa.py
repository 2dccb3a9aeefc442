"""What the compiler made of the MLA prefill backward (csrc/fa_bwd_mla_kernels.hip; cross-compiled here, no GPU; the approach of
tests/test_mla_wide_isa.py): eight kernels -- {dQ, dK/dV} x {f16, bf16} x {causal, full} -- and nothing else in the file, none with
scratch or static LDS, registers inside the budget of the occupancy each kernel declares (dQ: two workgroups per CU, 256; dK/dV: one,
512), the dynamic LDS figures of the two-part image, every LDS-DMA statement setting M0 itself with the whole offset in voffset, names
that none of the existing ISA tests' patterns match, and the file at the END of the Makefile's lists with the backward's flags."""
import os
import re

import pytest

from test_isa_audit import makefile_flags
from test_ksplit_isa import rows_of
from test_mla_isa import CSRC
from test_mla_wide_isa import OTHERS as WIDE_OTHERS
from test_mla_wide_isa import WIDE
from test_varlen_paged_isa import _compile

STEM = "fa_bwd_mla_kernels"
DQ, DKDV = "mla_grad_q_kernel", "mla_grad_kv_kernel"
OTHERS = WIDE_OTHERS + (WIDE,)
BUDGET = {3: 168, 2: 256, 1: 512}  # registers per lane at n workgroups of four waves per CU
OCC = {DQ: 2, DKDV: 1}             # the occupancy each kernel declares (csrc/fa_bwd_mla_kernels.hip, LG_Q_OCC / LG_KV_OCC)


@pytest.fixture(scope="module")
def listing():
    return _compile(STEM)


def kernel_of(name):
    return DQ if DQ in name else DKDV


def test_eight_kernels_and_nothing_else_without_scratch_inside_their_budget(listing):
    seen = {**rows_of(listing[1], DQ), **rows_of(listing[1], DKDV)}
    assert len(seen) == 8 == len(re.findall(r"Function Name: ", listing[1])), sorted(seen)
    assert {(kernel_of(n), "F16" if "3F16" in n else "BF16", "ELb1E" in n) for n in seen} == \
        {(k, t, c) for k in (DQ, DKDV) for t in ("F16", "BF16") for c in (False, True)}
    src = open(os.path.join(CSRC, STEM + ".hip")).read()
    assert re.search(r"constexpr int LG_Q_OCC = 2, LG_KV_OCC = 1;", src)
    assert re.search(r"__launch_bounds__\(NTHREADS, LG_Q_OCC\) void " + DQ, src) and re.search(r"__launch_bounds__\(NTHREADS, LG_KV_OCC\) void " + DKDV, src)
    for name, (vg, ag, scratch, occ) in seen.items():
        want = OCC[kernel_of(name)]
        assert re.match(r"_ZN2fa1[78]" + kernel_of(name) + r"I\S+BwdMlaParamsE$", name), name
        assert scratch == 0, (name, scratch)
        assert vg + ag <= BUDGET[want] and occ == want, (name, vg, ag, occ)


def test_no_static_lds_and_the_dynamic_figures(listing):
    sizes = dict(re.findall(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", listing[1], re.S))
    assert len(sizes) == 8 and all(int(v) == 0 for v in sizes.values()), sizes
    src = open(os.path.join(CSRC, STEM + ".hip")).read()
    # a buffer = the 64 x 384-byte two-part image + the 64 x 256-byte image; two buffers; the dK/dV kernel adds 1 KiB of row constants
    assert "constexpr size_t mla_grad_q_lds_bytes() { return (size_t)2 * LG_BUF; }" in src
    assert "constexpr size_t mla_grad_kv_lds_bytes() { return (size_t)2 * LG_BUF + 2 * 2 * BN * 4; }" in src
    assert re.search(r"LG_NRB = 256, LG_RRB = 128;", src) and "LG_IMGN = BN * LG_NRB, LG_IMGR = BN * LG_RRB;" in src
    assert "LG_WIDE = LG_IMGN + LG_IMGR, LG_BUF = LG_WIDE + LG_IMGN;" in src
    buf = 64 * 384 + 64 * 256
    assert 2 * buf == 80 * 1024 and OCC[DQ] * 2 * buf <= 160 * 1024       # two dQ workgroups fill the CU's LDS exactly
    assert OCC[DKDV] * (2 * buf + 1024) <= 160 * 1024 < 2 * (2 * buf + 1024)  # 81 KiB: two dK/dV workgroups do not fit


def bodies(asm):
    out = {}
    for m in re.finditer(r"^(_ZN2fa\d+(?:" + DQ + "|" + DKDV + r")\S+):.*?\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        out[m.group(1)] = [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
    return out


def test_every_lds_dma_statement_owns_m0_with_the_whole_offset_in_voffset(listing):
    seen = bodies(listing[0])
    assert len(seen) == 8
    for name, lines in seen.items():
        code = [ln for ln in lines if ln]
        # a wave stages 4 + 4 pieces of the two 256-byte images and 2 of the rotary image per tile; the dQ kernel has two staging sites
        # (prologue, loop), the dK/dV kernel three (prologue, the next query head of a group, loop)
        want = 10 * (2 if kernel_of(name) == DQ else 3)
        dma = [i for i, ln in enumerate(code) if re.match(r"buffer_load_dwordx4 v\d+, s\[\d+:\d+\], 0 offen lds$", ln)]
        assert len(dma) == want, (name, len(dma), want)
        assert sum("lds" in ln.split() for ln in code) == want  # no other LDS-DMA, none with an soffset
        for i in dma:  # the statement is: M0 <- the piece's LDS address, a wait state, the load
            # (a scalar register: with the dK/dV kernel's scalar pressure the allocator also hands out the halves of vcc)
            assert re.match(r"s_mov_b32 m0, (s\d+|vcc_lo|vcc_hi)$", code[i - 2]) and code[i - 1] == "s_nop 0", (name, code[i - 2:i + 1])
        assert sum(ln.startswith("s_mov_b32 m0,") for ln in code) == want


def test_matrix_work_per_tile(listing):
    # per 64-row tile a wave issues 2 halves x (12 + 8 first products + 12 (dQ) or 12 + 8 (dK, dV) second products) 32x32x16 MFMAs
    for name, lines in bodies(listing[0]).items():
        mfma = sum(1 for ln in lines if ln.startswith("v_mfma_f32_32x32x16"))
        assert mfma == (2 * (20 + 12) if kernel_of(name) == DQ else 2 * (20 + 20)), (name, mfma)


def test_names_stay_clear_of_the_existing_counts(listing):
    for word in OTHERS:
        for mine in (DQ, DKDV):
            assert word not in mine and mine not in word, (word, mine)
    for name in {**rows_of(listing[1], DQ), **rows_of(listing[1], DKDV)}:
        assert not any(w in name for w in OTHERS), name


def test_makefile_lists_the_file_last_with_the_backwards_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    asm = re.search(r"^ASM_KERNELS\s*:=(.*)$", mk, re.M).group(1).split()
    assert srcs[-1] == STEM + ".hip" and asm[-1] == STEM  # at the end: every existing object keeps its place on the link line
    assert makefile_flags(STEM) == makefile_flags("fa_bwd_kernels") == makefile_flags("fa_bwd_varlen_kernels")
    assert "-fno-honor-nans" in makefile_flags(STEM) and "-fno-slp-vectorize" in makefile_flags(STEM)
