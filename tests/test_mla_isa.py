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


MLA_HIPS = ("fa_mla_kernel.hip", "fa_mla_wide_kernel.hip", "fa_mla_kv8_kernel.hip", "fa_mla_sparse_kernel.hip")
PAGED_INC = "fa_mla_paged_partial.inc"


def read(name):
    return open(os.path.join(CSRC, name)).read()


def image_is_stated_in_the_body_header_alone():
    """The double buffer as fa_mla_body.h (part 0) states it for every file of the family: two tiles of 64 keys x (512 + 64) elements of
    two bytes; no .hip file states the image itself any more. Returns the header's text."""
    src = read("fa_mla_body.h")
    assert "constexpr size_t mla_lds_bytes() { return 2 * (size_t)MLA_IMG; }" in src
    assert re.search(r"MLA_DQK = 576, MLA_DV = 512", src) and "MLA_IMG = MLA_LAT + MLA_ROT" in src
    for name in MLA_HIPS:
        hip = read(name)
        assert "mla_lds_bytes() {" not in hip and "MLA_DQK =" not in hip and "MLA_IMG =" not in hip and "mla_swz(int" not in hip, name
    return src


def launch_tail_uses_the_double_buffer(body_h, hip, nw):
    """What `dim3(64 * nw), mla_lds_bytes(), s, p)` in each file's launch said: the one launch helper starts dim3(64 * nw) threads under
    mla_lds_bytes() of dynamic LDS, declared for the kernel first, and `hip` hands it its own wave count."""
    helper = re.search(r"inline hipError_t launch_mla_partial_and_combine\(K partial, dim3 grid, int nw, .*?\n}\n", body_h, re.S).group(0)
    assert "set_dyn_lds_once((const void *)partial, (int)mla_lds_bytes())" in helper
    assert "hipLaunchKernelGGL(partial, grid, dim3(64 * nw), mla_lds_bytes(), s, p);" in helper
    assert helper.index("set_dyn_lds_once") < helper.index("hipLaunchKernelGGL") < helper.index("launch_mla_combine(pc, dtype, s)")
    calls = re.findall(r"launch_mla_partial_and_combine\([^;]*?\),\s+(\w+), p, \w+, \w+, s\);", hip)
    assert calls == [nw], (calls, nw)
    assert "hipLaunchKernelGGL(partial" not in hip and "set_dyn_lds_once" not in hip


def test_dynamic_lds_fits_the_cu():
    src = image_is_stated_in_the_body_header_alone()
    launch_tail_uses_the_double_buffer(src, read("fa_mla_kernel.hip"), "1")
    lds = 2 * 64 * (512 + 64) * 2
    assert lds == 144 * 1024 and lds <= 160 * 1024


def test_the_paged_partial_kernel_and_the_image_are_one_text_each():
    inc = read(PAGED_INC)
    for name in ("fa_mla_kernel.hip", "fa_mla_wide_kernel.hip"):
        hip = read(name)
        assert len(re.findall(r'#include "%s"' % re.escape(PAGED_INC), hip)) == 1, name
        # the descriptors and the LDS-DMA statements of the 16-bit paged pool: in the text, in neither file
        assert "make_buffer_rsrc" not in hip and "offen lds" not in hip, name
    assert "make_buffer_rsrc" in inc and "offen lds" in inc
    for part in (1, 2, 3):
        assert len(re.findall(r"#define FA_MLA_BODY_PART %d\b[^\n]*\n#include \"fa_mla_body.h\"" % part, inc)) == 1, part
    sources = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".inc"))]
    assert [f for f in sources if "MLA_DQK = 576" in read(f)] == ["fa_mla_body.h"]
    mk = read("Makefile")
    assert re.search(r"^%\.o:.*\b" + re.escape(PAGED_INC) + r"\b", mk, re.M) and re.search(r"^asm:.*\b" + re.escape(PAGED_INC) + r"\b", mk, re.M)


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
