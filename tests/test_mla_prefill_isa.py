"""What the compiler made of the MLA prefill kernels (csrc/fa_mfma_kernel.hip, MLA mode; cross-compiled here, no GPU; the approach of
tests/test_varlen_paged_isa.py): exactly four kernels, {f16, bf16} x {causal, full}, no scratch, inside the register budget of two
workgroups per CU, the M0 convention and the count of their LDS-DMA statements, the dynamic LDS figure the launcher passes, names that
none of the existing ISA tests' patterns match, and the Makefile entries."""
import os
import re

import pytest

from test_isa_audit import makefile_flags
from test_ksplit_isa import OTHERS as KSPLIT_OTHERS, rows_of
from test_varlen_paged_isa import BUDGET, _compile

KERNEL = "fwd_mfma_mla_kernel"
# the substrings and prefixes by which the other ISA tests count their kernels in the listing of fa_mfma_kernel.hip
OTHERS = KSPLIT_OTHERS + ("fwd_mfma_ksplit_paged_kernel", "ksplit_combine_kernel", "fwd_mfma_kernel", "mla_partial_kernel", "mla_combine_kernel",
                          "dsink_kernel", "kv_quant_append_paged_kernel", "bwd_")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flash_attention_metal_amd", "csrc")
LDS = 2 * 64 * (256 + 128) + 2 * 64 * 256  # K double buffer ([64][128] + [64][64] elements per tile) + V double buffer ([64][128])


@pytest.fixture(scope="module")
def listing():
    return _compile("fa_mfma_kernel")


def test_four_kernels_without_scratch_inside_the_budget_of_two_workgroups(listing):
    seen = rows_of(listing[1], KERNEL)
    assert len(seen) == 4, sorted(seen)
    assert {("F16" if "3F16" in n else "BF16", "ELb1E" in n) for n in seen} == {(t, c) for t in ("F16", "BF16") for c in (False, True)}
    for name, (vg, ag, scratch, occ) in seen.items():
        assert re.match(r"_ZN2fa19" + KERNEL + r"I\S+VarlenMlaParamsE$", name), name
        assert scratch == 0, (name, scratch)
        assert vg + ag <= BUDGET[2] and occ == 2, (name, vg, ag, occ)


def test_dynamic_lds_is_eighty_kib_and_two_workgroups_fill_the_cu():
    assert LDS == 80 * 1024 and 2 * LDS == 160 * 1024
    src = open(os.path.join(CSRC, "fa_mfma_kernel.hip")).read()
    # the launcher passes the body's own figure: mfma_lds_bytes with the two head dims, K rows of D * 2 bytes and V rows of DV * 2
    assert re.search(r"constexpr size_t lds = mfma_lds_bytes<Tag, 192, 1, BM, 128>\(\);", src)
    assert "KRB = std::is_same<Tag, FP8>::value ? D : (DV != D) ? D * 2 : RB;" in src and "RB = (D == 96) ? 256 : DV * 2" in src
    assert "return std::max(SPLIT * (2 * BN * KRB + 2 * BN * RB), SPLIT == 2 ? merge_end : otiles);" in src
    assert re.search(r"__launch_bounds__\(NTHREADS, 2\) void " + KERNEL, src)


def test_lds_dma_statements_own_m0_and_count_ten_per_tile(listing):
    text = listing[0]
    names = re.findall(r"^(_ZN2fa19" + KERNEL + r"\S+):", text, re.M)
    assert len(names) == 4
    for name in names:
        start = re.search(r"^" + re.escape(name) + r":", text, re.M).start()
        body = text[start:text.index(".Lfunc_end", start)].splitlines()
        in_asm, own_m0, dma = False, False, 0
        for ln, t in enumerate(body, 1):
            u = t.strip()
            if u.startswith(";;#ASMSTART"):
                in_asm, own_m0 = True, False
            elif u.startswith(";;#ASMEND"):
                in_asm = False
            elif u and not u.startswith((";", ".")):
                if "m0" in u.replace(",", " ").split():
                    assert in_asm, (name, ln, u, "M0 touched outside an asm block")
                    if u.startswith("s_mov_b32 m0"):
                        own_m0 = True
                if u.startswith("buffer_load") and u.endswith(" lds"):
                    assert in_asm and own_m0, (name, ln, u, "LDS-DMA without its own M0 write in the same statement")
                    dma += 1
        # per wave and tile: four nope pieces and two rotary pieces of K, four pieces of V; staged in the prologue and in both tile bodies
        assert dma == 3 * (4 + 2 + 4), (name, dma)
        # twelve k-steps of two 32-key blocks and 2 x 2 x 4 PV steps per tile body; the exact path's recompute adds 24 more
        mfma = sum(1 for t in body if t.strip().startswith("v_mfma_f32_32x32x16"))
        assert mfma == 2 * (24 + 16 + 24), (name, mfma)


def test_names_stay_clear_of_the_existing_counts(listing):
    for word in OTHERS:
        assert word not in KERNEL and (KERNEL not in word), word
    for name in rows_of(listing[1], KERNEL):
        assert not any(w in name for w in OTHERS), name
        for params in ("VarlenPagedParams", "DecodeSoftcapParams", "DecodeWindowParams", "DecodePagedParams"):
            assert params not in name
    # and the other way round: no existing kernel of the file is counted as one of these
    assert all(KERNEL + "I" in n for n in rows_of(listing[1], KERNEL))


def test_makefile_lists_the_file_with_the_matrix_core_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bfa_mfma_kernel\.hip\b", text, re.M)
    assert re.search(r"^ASM_KERNELS\s*:=.*\bfa_mfma_kernel\b", text, re.M)
    assert makefile_flags("fa_mfma_kernel")[-2:] == ["-fno-honor-nans", "-fno-slp-vectorize"]
