"""What the compiler made of the multi-wave latent-attention decode kernels (csrc/fa_mla_wide_kernel.hip; cross-compiled here, no GPU;
the approach of tests/test_mla_isa.py): eight partial kernels ({f16, bf16} x {without, with} the causal mask x {2, 4} waves), none with
scratch or static LDS, one wave per SIMD inside the 512-entry register file, the shared double buffer inside the CU's 160 KiB of LDS,
the LDS-DMA statements the piece split derives -- each setting M0 itself -- one barrier behind one explicit wait, names that none of the
existing ISA tests' patterns match, and the file on the Makefile's lists with the decode kernel's flags."""
import os
import re

import pytest

from test_isa_audit import makefile_flags
from test_ksplit_isa import rows_of
from test_mla_isa import COMBINE, CSRC, OTHERS, PARTIAL, image_is_stated_in_the_body_header_alone, launch_tail_uses_the_double_buffer
from test_varlen_paged_isa import _compile

WIDE = "mla_wide_partial_kernel"
OTHERS = OTHERS + (PARTIAL, COMBINE, "fwd_mfma_kernel", "fwd_mfma_mla_kernel", "dsink_kernel", "kv_quant_append_paged_kernel", "bwd_")


@pytest.fixture(scope="module")
def listing():
    return _compile("fa_mla_wide_kernel")


def waves_of(name):
    return int(re.search(r"ELb[01]ELi(\d)E", name).group(1))


def test_eight_kernels_without_scratch_one_wave_per_simd(listing):
    seen = rows_of(listing[1], WIDE)
    assert len(seen) == 8, sorted(seen)
    assert {("F16" if "3F16" in n else "BF16", "ELb1E" in n, waves_of(n)) for n in seen} == \
        {(t, c, nw) for t in ("F16", "BF16") for c in (False, True) for nw in (2, 4)}
    for name, (vg, ag, scratch, occ) in seen.items():
        assert re.match(r"_ZN2fa23" + WIDE + r"I\S+MlaDecodeParamsE$", name), name
        assert scratch == 0 and vg + ag <= 512 and occ == 1, (name, vg, ag, scratch, occ)
    # nothing else is compiled in this file: the combine kernel is fa_mla_kernel.hip's
    assert len(re.findall(r"Function Name: ", listing[1])) == 8


def test_no_static_lds_and_the_shared_double_buffer_fits_the_cu(listing):
    sizes = dict(re.findall(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", listing[1], re.S))
    assert len(sizes) == 8 and all(int(v) == 0 for v in sizes.values()), sizes
    src = open(os.path.join(CSRC, "fa_mla_wide_kernel.hip")).read()
    # the double buffer as fa_mla_body.h states it: two tiles of 64 keys x (512 + 64) elements of two bytes, ONE per workgroup
    launch_tail_uses_the_double_buffer(image_is_stated_in_the_body_header_alone(), src, "nw")
    lds = 2 * 64 * (512 + 64) * 2
    assert lds == 144 * 1024 and lds <= 160 * 1024


def bodies(asm):
    out = {}
    for m in re.finditer(r"^(_ZN2fa\d+" + WIDE + r"\S+):.*?\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        out[m.group(1)] = [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
    return out


def test_lds_dma_statements_follow_the_piece_split_and_each_owns_m0(listing):
    seen = bodies(listing[0])
    assert len(seen) == 8
    for name, lines in seen.items():
        code = [ln for ln in lines if ln]
        nw = waves_of(name)
        # a wave stages 64 / NW latent rows (one 1-KiB piece each) and 8 / NW rotary pieces of a tile; one staging site, compiled for
        # pages of 16, of 32 and of 64 keys and more
        want = 3 * (64 // nw + 8 // nw)
        dma = [i for i, ln in enumerate(code) if re.match(r"buffer_load_dwordx4 v\d+, s\[\d+:\d+\], 0 offen lds$", ln)]
        assert len(dma) == want == {2: 108, 4: 54}[nw], (name, len(dma), want)
        assert sum("lds" in ln.split() for ln in code) == want  # no other LDS-DMA
        for i in dma:  # the statement is: M0 <- the piece's LDS address, a wait state, the load
            assert re.match(r"s_mov_b32 m0, s\d+$", code[i - 2]) and code[i - 1] == "s_nop 0", (name, code[i - 2:i + 1])
        assert sum(ln.startswith("s_mov_b32 m0,") for ln in code) == want


def test_one_barrier_per_tile_behind_the_explicit_wait(listing):
    for name, lines in bodies(listing[0]).items():
        code = [ln for ln in lines if ln and not ln.startswith(".") and not ln.startswith(";")]
        bars = [i for i, ln in enumerate(code) if ln == "s_barrier"]
        assert len(bars) == 1, (name, len(bars))  # one site: every wave of the workgroup meets it once per iteration
        before = code[:bars[0]]
        wait = max(i for i, ln in enumerate(before) if ln == "s_waitcnt vmcnt(0)")
        # between the wait and the barrier: no memory instruction of any kind (register moves and scalar compares only)
        assert not any(re.match(r"(buffer_|global_|flat_|ds_|s_load|s_buffer_load|scratch_)", ln) for ln in code[wait + 1:bars[0]]), name


def test_names_stay_clear_of_the_existing_counts(listing):
    for word in OTHERS:
        assert word not in WIDE and WIDE not in word, word
    for name in rows_of(listing[1], WIDE):
        assert not any(w in name for w in OTHERS), name


def test_makefile_lists_the_file_with_the_decode_kernels_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    asm = re.search(r"^ASM_KERNELS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "fa_mla_wide_kernel.hip" in srcs and "fa_mla_wide_kernel" in asm
    assert makefile_flags("fa_mla_wide_kernel") == makefile_flags("fa_decode_kernel") == makefile_flags("fa_mla_kernel")
    # the per-wave text both files include is a prerequisite of every object
    assert re.search(r"^%\.o:.*\bfa_mla_body\.h\b", mk, re.M)
