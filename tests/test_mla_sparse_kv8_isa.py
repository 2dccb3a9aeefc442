"""What the compiler made of the sparse e4m3-pool latent-attention decode kernel (csrc/fa_mla_sparse_kv8_kernel.hip; cross-compiled here,
no GPU; the approach of tests/test_mla_kv8_isa.py): one partial kernel and nothing else, without scratch or static LDS, one wave per SIMD
inside the 512-entry register file, the shared double buffer of 144 KiB, no LDS-DMA anywhere, the register staging -- nine 16-byte vector
loads under per-lane addresses and eighteen 16-byte LDS writes per staging site, at two sites -- one barrier behind its explicit wait with
no memory instruction between, the four parts of the body included once each, and the file on the Makefile's lists, in front of the MLA
backward, with the flags of its two parents."""
import os
import re

import pytest

from test_isa_audit import makefile_flags
from test_ksplit_isa import rows_of
from test_mla_isa import CSRC, image_is_stated_in_the_body_header_alone, launch_tail_uses_the_double_buffer
from test_varlen_paged_isa import _compile

KERNEL = "mla_sparse_kv8_partial_kernel"
SITES = 2  # the prologue (tile t0) and the loop (tile t + 1 under the arithmetic of tile t)
QLOADS = 18  # the query fragments of fa_mla_body.h part 1: one 16-byte load per k-step, in front of everything


@pytest.fixture(scope="module")
def listing():
    return _compile("fa_mla_sparse_kv8_kernel")


def test_one_kernel_and_nothing_else_without_scratch_one_wave_per_simd(listing):
    seen = rows_of(listing[1], KERNEL)
    assert list(seen) == ["_ZN2fa29" + KERNEL + "ENS_15MlaSparseParamsE"], sorted(seen)
    for name, (vg, ag, scratch, occ) in seen.items():
        assert scratch == 0 and vg + ag <= 512 and occ == 1, (name, vg, ag, scratch, occ)
    # nothing else is compiled in this file: the combine kernel is fa_mla_kernel.hip's
    assert len(re.findall(r"Function Name: ", listing[1])) == 1
    assert "scratch_" not in listing[0]


def test_no_static_lds_and_the_shared_double_buffer_is_144_kib(listing):
    sizes = dict(re.findall(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", listing[1], re.S))
    assert len(sizes) == 1 and all(int(v) == 0 for v in sizes.values()), sizes
    src = open(os.path.join(CSRC, "fa_mla_sparse_kv8_kernel.hip")).read()
    assert "constexpr int MLA_SPARSE_KV8_NW = 4;" in src
    launch_tail_uses_the_double_buffer(image_is_stated_in_the_body_header_alone(), src, "MLA_SPARSE_KV8_NW")
    lds = 2 * 64 * (512 + 64) * 2
    assert lds == 144 * 1024 and lds <= 160 * 1024
    # from LDS onwards the text is the wide kernel's: the four parts of fa_mla_body.h, each included once
    for part in range(4):
        assert len(re.findall(r"#define FA_MLA_BODY_PART %d\b[^\n]*\n#include \"fa_mla_body.h\"" % part, src)) == 1, part


def body(asm):
    seen = re.findall(r"^(_ZN2fa\d+" + KERNEL + r"\S+):.*?\n(.*?)^\.Lfunc_end", asm, re.S | re.M)
    assert len(seen) == 1
    return [ln.split(";")[0].strip() for ln in seen[0][1].splitlines()]


def test_register_staging_nine_loads_and_eighteen_writes_per_site_and_no_lds_dma(listing):
    code = [ln for ln in body(listing[0]) if ln]
    assert not any("lds" in ln.split() for ln in code)  # no `... offen lds` load: LDS-DMA cannot widen
    assert not any(ln.startswith("s_mov_b32 m0,") for ln in code)
    assert not any(ln.startswith("buffer_load") for ln in code)  # two rows share a load, the pool may exceed 4 GiB: no descriptor
    loads = [i for i, ln in enumerate(code) if re.match(r"global_load_dwordx4 v\[\d+:\d+\], v\[\d+:\d+\], off( offset:\d+)?$", ln)]
    writes = [i for i, ln in enumerate(code) if re.match(r"ds_write_b128 v\d+, v\[\d+:\d+\]( offset:\d+)?$", ln)]
    # a wave stages 16 rows of 576 bytes: eight latent loads (two rows each) and one rotary load per lane, each under the 64-bit address of
    # its lane's row, every 16-byte e4m3 chunk written as two 16-byte bf16 chunks
    assert len(loads) == QLOADS + SITES * 9 and len(writes) == SITES * 18, (len(loads), len(writes))
    assert sum(ln.startswith("global_load_dwordx4") for ln in code) == len(loads) and sum(ln.startswith("ds_write") for ln in code) == len(writes)
    bar = code.index("s_barrier")
    # the query fragments and the prologue's site in front of the loop's barrier, the loop's site behind it
    assert sum(i < bar for i in loads) == QLOADS + 9 and sum(i < bar for i in writes) == 18


def test_one_barrier_per_tile_behind_the_explicit_wait(listing):
    code = [ln for ln in body(listing[0]) if ln and not ln.startswith(".") and not ln.startswith(";")]
    bars = [i for i, ln in enumerate(code) if ln == "s_barrier"]
    assert len(bars) == 1, len(bars)  # one site: every wave of the workgroup meets it once per iteration
    before = code[:bars[0]]
    wait = max(i for i, ln in enumerate(before) if ln == "s_waitcnt lgkmcnt(0)")
    # between the wait and the barrier: no memory instruction of any kind (register moves and scalar compares only)
    assert not any(re.match(r"(buffer_|global_|flat_|ds_|s_load|s_buffer_load|scratch_)", ln) for ln in code[wait + 1:bars[0]])
    assert not any(ln.startswith("s_cbranch") for ln in code[wait + 1:bars[0]])


def test_makefile_lists_the_file_in_front_of_the_mla_backward_with_its_parents_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    asm = re.search(r"^ASM_KERNELS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "fa_mla_sparse_kv8_kernel.hip" in srcs and "fa_mla_sparse_kv8_kernel" in asm
    assert srcs[-1] == "fa_bwd_mla_kernels.hip" and asm[-1] == "fa_bwd_mla_kernels"
    assert makefile_flags("fa_mla_sparse_kv8_kernel") == makefile_flags("fa_mla_kv8_kernel") == makefile_flags("fa_mla_sparse_kernel")
    assert re.search(r"^%\.o:.*\bfa_mla_body\.h\b", mk, re.M)
