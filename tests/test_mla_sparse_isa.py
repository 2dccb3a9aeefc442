"""What the compiler made of the sparse latent-attention decode kernels (csrc/fa_mla_sparse_kernel.hip; cross-compiled here, no GPU; the
approach of tests/test_mla_kv8_isa.py): two partial kernels (f16, bf16) and nothing else, neither with scratch or static LDS, one wave
per SIMD inside the 512-entry register file, the shared double buffer of 144 KiB inside the CU's 160 KiB of LDS, the staging the head of
the file derives -- sixteen LDS-DMA pieces, one descriptor each, two predicated 16-byte rotary loads and their two 16-byte LDS writes
per lane, at ONE staging site -- one barrier behind one explicit wait, names that none of the existing ISA tests' patterns match, and
the file on the Makefile's lists with the wide kernel's flags."""
import os
import re

import pytest

from test_isa_audit import makefile_flags
from test_ksplit_isa import rows_of
from test_mla_isa import CSRC, image_is_stated_in_the_body_header_alone, launch_tail_uses_the_double_buffer
from test_mla_kv8_isa import KV8
from test_mla_kv8_isa import OTHERS as KV8_OTHERS
from test_varlen_paged_isa import _compile

SPARSE = "mla_sparse_partial_kernel"
OTHERS = KV8_OTHERS + (KV8,)


@pytest.fixture(scope="module")
def listing():
    return _compile("fa_mla_sparse_kernel")


def test_two_kernels_and_nothing_else_without_scratch_one_wave_per_simd(listing):
    seen = rows_of(listing[1], SPARSE)
    assert len(seen) == 2, sorted(seen)
    for name, (vg, ag, scratch, occ) in seen.items():
        assert re.match(r"_ZN2fa25" + SPARSE + r"INS_(3F16|4BF16)EEEvNS_15MlaSparseParamsE$", name), name
        assert scratch == 0 and vg + ag <= 512 and occ == 1, (name, vg, ag, scratch, occ)
    # nothing else is compiled in this file: the combine kernel is fa_mla_kernel.hip's
    assert len(re.findall(r"Function Name: ", listing[1])) == 2
    assert "scratch_" not in listing[0]


def test_no_static_lds_and_the_shared_double_buffer_fits_the_cu(listing):
    sizes = dict(re.findall(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", listing[1], re.S))
    assert len(sizes) == 2 and all(int(v) == 0 for v in sizes.values()), sizes
    src = open(os.path.join(CSRC, "fa_mla_sparse_kernel.hip")).read()
    # the double buffer as fa_mla_body.h states it: two tiles of 64 keys x (512 + 64) 16-bit elements, ONE per workgroup of four waves
    assert "constexpr int MLA_SPARSE_NW = 4;" in src
    launch_tail_uses_the_double_buffer(image_is_stated_in_the_body_header_alone(), src, "MLA_SPARSE_NW")
    lds = 2 * 64 * (512 + 64) * 2
    assert lds == 144 * 1024 and lds <= 160 * 1024
    # from LDS onwards the text is the wide kernel's: the four parts of fa_mla_body.h, each included once, under CAUSAL = false
    for part in range(4):
        assert len(re.findall(r"#define FA_MLA_BODY_PART %d\b[^\n]*\n#include \"fa_mla_body.h\"" % part, src)) == 1, part
    assert "constexpr bool CAUSAL = false;" in src


def bodies(asm):
    out = {}
    for m in re.finditer(r"^(_ZN2fa\d+" + SPARSE + r"\S+):.*?\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        out[m.group(1)] = [ln.split(";")[0].strip() for ln in m.group(2).splitlines()]
    return out


def test_one_staging_site_sixteen_pieces_two_rotary_loads_two_writes(listing):
    seen = bodies(listing[0])
    assert len(seen) == 2
    for name, lines in seen.items():
        code = [ln for ln in lines if ln]
        # a wave stages 16 rows: sixteen 1-KiB latent pieces by LDS-DMA, each behind its own m0 and under its own descriptor ...
        dma = [ln for ln in code if re.match(r"buffer_load_dwordx4 v\d+, s\[\d+:\d+\], 0 offen lds$", ln)]
        assert len(dma) == 16 and sum(ln.startswith("buffer_load") for ln in code) == 16, (name, len(dma))
        assert sum(ln.startswith("s_mov_b32 m0,") for ln in code) == 16, name
        assert sum(ln.startswith("v_readlane_b32") for ln in code) >= 16, name  # the entries come out of their lanes
        # ... and the rotary 128 bytes of its rows through registers: two 16-byte loads and two 16-byte LDS writes per lane, the only
        # LDS writes of the kernel
        rot = [i for i, ln in enumerate(code) if re.match(r"global_load_dwordx4 [va]\[\d+:\d+\], ", ln)]
        writes = [i for i, ln in enumerate(code) if re.match(r"ds_write_b128 v\d+, [va]\[\d+:\d+\]( offset:\d+)?$", ln)]
        assert len(writes) == 2 and sum(ln.startswith("ds_write") for ln in code) == 2, (name, len(writes))
        bar = code.index("s_barrier")
        # the one staging site stands behind the barrier; in front of it only the queries are loaded (18 fragments of 16 bytes)
        assert sum(i > bar for i in rot) == 2 and sum(i < bar for i in rot) == 18, (name, rot, bar)
        assert all(i > bar for i in writes), name
        assert all(i > bar for i, ln in enumerate(code) if ln.endswith("offen lds")), name
        # the rotary writes stand behind the tile's arithmetic: no MFMA follows them before the loop closes
        mfma = [i for i, ln in enumerate(code) if ln.startswith("v_mfma")]
        assert len(mfma) == 136 and max(mfma) < min(writes), (name, len(mfma))


def test_one_barrier_per_tile_behind_the_explicit_wait(listing):
    for name, lines in bodies(listing[0]).items():
        code = [ln for ln in lines if ln and not ln.startswith(".") and not ln.startswith(";")]
        bars = [i for i, ln in enumerate(code) if ln == "s_barrier"]
        assert len(bars) == 1, (name, len(bars))  # one site: every wave of the workgroup meets it once per iteration
        before = code[:bars[0]]
        wait = max(i for i, ln in enumerate(before) if ln == "s_waitcnt vmcnt(0) lgkmcnt(0)")
        # between the wait and the barrier: no memory instruction of any kind (register moves and scalar compares only)
        assert not any(re.match(r"(buffer_|global_|flat_|ds_|s_load|s_buffer_load|scratch_)", ln) for ln in code[wait + 1:bars[0]]), name
        assert not any(ln.startswith("s_cbranch") for ln in code[wait + 1:bars[0]]), name


def test_names_stay_clear_of_the_existing_counts(listing):
    for word in OTHERS:
        assert word not in SPARSE and SPARSE not in word, word
    for name in rows_of(listing[1], SPARSE):
        assert not any(w in name for w in OTHERS), name


def test_makefile_lists_the_file_with_the_wide_kernels_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    asm = re.search(r"^ASM_KERNELS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "fa_mla_sparse_kernel.hip" in srcs and "fa_mla_sparse_kernel" in asm
    assert makefile_flags("fa_mla_sparse_kernel") == makefile_flags("fa_mla_wide_kernel") == makefile_flags("fa_mla_kv8_kernel")
    assert re.search(r"^%\.o:.*\bfa_mla_body\.h\b", mk, re.M)
