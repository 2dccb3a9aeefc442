"""What the compiler made of the latent-attention decode kernels (csrc/fa_mla_kernel.hip; cross-compiled here, no GPU; the approach of
tests/test_ksplit_isa.py): four partial kernels ({f16, bf16} x {without, with} the causal mask) and two combine kernels, none with
scratch, the partial kernels' double buffer inside the CU's 160 KiB of LDS, names that none of the existing ISA tests' patterns match,
and the file on the Makefile's lists with the decode kernel's flags."""
import os
import re

import pytest

from test_isa_audit import makefile_flags
from test_ksplit_isa import OTHERS, rows_of
from test_varlen_paged_isa import ROOT, _compile

PARTIAL, COMBINE = "mla_partial_kernel", "mla_combine_kernel"
OTHERS = OTHERS + ("fwd_mfma_ksplit_paged_kernel", "ksplit_combine_kernel")
CSRC = os.path.join(ROOT, "flash_attention_metal_amd", "csrc")


@pytest.fixture(scope="module")
def remarks():
    return _compile("fa_mla_kernel")[1]


def test_partial_and_combine_kernels_exist_for_both_types_without_scratch(remarks):
    partial, combine = rows_of(remarks, PARTIAL), rows_of(remarks, COMBINE)
    assert len(partial) == 4 and len(combine) == 2, (sorted(partial), sorted(combine))
    for seen in (partial, combine):
        assert sum("3F16" in n for n in seen) == len(seen) // 2 and sum("4BF16" in n for n in seen) == len(seen) // 2, sorted(seen)
    assert sum("ELb1E" in n for n in partial) == 2  # the causal instantiations
    for name, (vg, ag, scratch, occ) in {**partial, **combine}.items():
        assert scratch == 0 and vg + ag <= 512, (name, vg, ag, scratch)


def test_dynamic_lds_fits_the_cu():
    src = open(os.path.join(CSRC, "fa_mla_kernel.hip")).read()
    # the double buffer as the file states it: two tiles of 64 keys x (512 + 64) elements of two bytes
    assert "constexpr size_t mla_lds_bytes() { return 2 * (size_t)MLA_IMG; }" in src
    assert re.search(r"MLA_DQK = 576, MLA_DV = 512", src) and "MLA_IMG = MLA_LAT + MLA_ROT" in src
    lds = 2 * 64 * (512 + 64) * 2
    assert lds == 144 * 1024 and lds <= 160 * 1024


def test_static_lds_is_the_combine_kernels_weights_only(remarks):
    sizes = dict(re.findall(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", remarks, re.S))
    assert all(int(v) == 0 for n, v in sizes.items() if PARTIAL in n) and all(int(v) == 1024 for n, v in sizes.items() if COMBINE in n), sizes


def test_names_stay_clear_of_the_existing_counts(remarks):
    for word in OTHERS:
        assert word not in PARTIAL and word not in COMBINE and PARTIAL not in word and COMBINE not in word, word
    for name in list(rows_of(remarks, PARTIAL)) + list(rows_of(remarks, COMBINE)):
        assert not any(w in name for w in OTHERS), name


def test_makefile_lists_the_file_with_the_decode_kernels_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*)$", mk, re.M).group(1).split()
    asm = re.search(r"^ASM_KERNELS\s*:=(.*)$", mk, re.M).group(1).split()
    assert "fa_mla_kernel.hip" in srcs and "fa_mla_kernel" in asm
    assert makefile_flags("fa_mla_kernel") == makefile_flags("fa_decode_kernel")
