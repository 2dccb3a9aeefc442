"""What the compiler made of the e4m3-pool latent-attention decode kernels (csrc/fa_mla_kv8_kernel.hip; cross-compiled here, no GPU; the
approach of tests/test_mla_wide_isa.py): two partial kernels (bf16, without and with the causal mask) and nothing else, neither with
scratch or static LDS, one wave per SIMD inside the 512-entry register file, the shared double buffer inside the CU's 160 KiB of LDS,
no LDS-DMA anywhere, the register staging the row split derives -- nine 16-byte loads and eighteen 16-byte LDS writes per staging site
-- one barrier behind one explicit wait, names that none of the existing ISA tests' patterns match, and the file on the Makefile's
lists with the decode kernel's flags."""
import os
import re

import pytest

from test_isa_audit import makefile_flags
from test_ksplit_isa import rows_of
from test_mla_isa import CSRC, image_is_stated_in_the_body_header_alone, launch_tail_uses_the_double_buffer
from test_mla_wide_isa import OTHERS, WIDE
from test_varlen_paged_isa import _compile

KV8 = "mla_kv8_partial_kernel"
OTHERS = OTHERS + (WIDE,)
SITES = 2  # the prologue (tile t0) and the loop (tile t + 1 under the arithmetic of tile t)


@pytest.fixture(scope="module")
def listing():
    return _compile("fa_mla_kv8_kernel")


def test_two_kernels_and_nothing_else_without_scratch_one_wave_per_simd(listing):
    seen = rows_of(listing[1], KV8)
    assert len(seen) == 2 and {"ILb1E" in n for n in seen} == {False, True}, sorted(seen)
    for name, (vg, ag, scratch, occ) in seen.items():
        assert re.match(r"_ZN2fa22" + KV8 + r"ILb[01]EEEvNS_15MlaDecodeParamsE$", name), name
        assert scratch == 0 and vg + ag <= 512 and occ == 1, (name, vg, ag, scratch, occ)
    # nothing else is compiled in this file: the combine kernel is fa_mla_kernel.hip's
    assert len(re.findall(r"Function Name: ", listing[1])) == 2
    assert "scratch_" not in listing[0]


def test_no_static_lds_and_the_shared_double_buffer_fits_the_cu(listing):
    sizes = dict(re.findall(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", listing[1], re.S))
    assert len(sizes) == 2 and all(int(v) == 0 for v in sizes.values()), sizes
    src = open(os.path.join(CSRC, "fa_mla_kv8_kernel.hip")).read()
    # the double buffer as fa_mla_body.h states it: two tiles of 64 keys x (512 + 64) bf16 elements, ONE per workgroup of four waves
    assert "constexpr int MLA_KV8_NW = 4;" in src
    launch_tail_uses_the_double_buffer(image_is_stated_in_the_body_header_alone(), src, "MLA_KV8_NW")
    lds = 2 * 64 * (512 + 64) * 2
    assert lds == 144 * 1024 and lds <= 160 * 1024
    # from LDS onwards the text is the wide kernel's: the four parts of fa_mla_body.h, each included once
    for part in range(4):
        assert len(re.findall(r"#define FA_MLA_BODY_PART %d\b[^\n]*\n#include \"fa_mla_body.h\"" % part, src)) == 1, part


def bodies(asm):
    out = {}
    for m in re.finditer(r"^(_ZN2fa\d+" + KV8 + r"\S+):.*?\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        out[m.group(1)] = [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
    return out


def test_register_staging_nine_loads_and_eighteen_writes_per_site_and_no_lds_dma(listing):
    seen = bodies(listing[0])
    assert len(seen) == 2
    for name, lines in seen.items():
        code = [ln for ln in lines if ln]
        assert not any("lds" in ln.split() for ln in code), name  # no `... offen lds` load: LDS-DMA cannot widen
        assert not any(ln.startswith("s_mov_b32 m0,") for ln in code), name
        loads = [i for i, ln in enumerate(code) if re.match(r"buffer_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\], 0 offen$", ln)]
        writes = [i for i, ln in enumerate(code) if re.match(r"ds_write_b128 v\d+, v\[\d+:\d+\]( offset:\d+)?$", ln)]
        # a wave stages 16 rows of 576 bytes: eight latent loads (two rows each) and one rotary load per lane, every 16-byte e4m3 chunk
        # written as two 16-byte bf16 chunks
        assert len(loads) == SITES * 9 and len(writes) == SITES * 18, (name, len(loads), len(writes))
        assert sum(ln.startswith("buffer_load") for ln in code) == SITES * 9 and sum(ln.startswith("ds_write") for ln in code) == SITES * 18
        bar = code.index("s_barrier")
        # the prologue's site in front of the loop's barrier, the loop's behind it
        assert sum(i < bar for i in loads) == 9 and sum(i < bar for i in writes) == 18, name
        # the page table entry comes through the scalar cache: the vector memory counter sees the nine raw loads alone
        assert not any(ln.startswith("global_load_dword ") for ln in code), name


def test_one_barrier_per_tile_behind_the_explicit_wait(listing):
    for name, lines in bodies(listing[0]).items():
        code = [ln for ln in lines if ln and not ln.startswith(".") and not ln.startswith(";")]
        bars = [i for i, ln in enumerate(code) if ln == "s_barrier"]
        assert len(bars) == 1, (name, len(bars))  # one site: every wave of the workgroup meets it once per iteration
        before = code[:bars[0]]
        wait = max(i for i, ln in enumerate(before) if ln == "s_waitcnt lgkmcnt(0)")
        # between the wait and the barrier: no memory instruction of any kind (register moves and scalar compares only)
        assert not any(re.match(r"(buffer_|global_|flat_|ds_|s_load|s_buffer_load|scratch_)", ln) for ln in code[wait + 1:bars[0]]), name
        assert not any(ln.startswith("s_cbranch") for ln in code[wait + 1:bars[0]]), name


def test_names_stay_clear_of_the_existing_counts(listing):
    for word in OTHERS:
        assert word not in KV8 and KV8 not in word, word
    for name in rows_of(listing[1], KV8):
        assert not any(w in name for w in OTHERS), name


def test_makefile_lists_the_file_with_the_decode_kernels_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    asm = re.search(r"^ASM_KERNELS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "fa_mla_kv8_kernel.hip" in srcs and "fa_mla_kv8_kernel" in asm
    assert makefile_flags("fa_mla_kv8_kernel") == makefile_flags("fa_decode_kernel") == makefile_flags("fa_mla_wide_kernel")
    assert re.search(r"^%\.o:.*\bfa_mla_body\.h\b", mk, re.M)
