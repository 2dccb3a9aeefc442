"""What the compiler made of the sliding-window backward kernels (cross-compiled here, no GPU; the pattern of tests/test_window_isa.py
and tests/test_varlen_bwd_isa.py): exactly the eight kernels of csrc/fa_bwd_window_kernels.hip, the occupancy of the varlen backward
kernel of their head dim (three workgroups per CU at head_dim 64, two at 128), no scratch -- the head_dim-128 dK/dV kernel is allowed
the dense kernel's 32 bytes (tests/test_isa_audit.py) and uses none --, the M0 convention of their LDS-DMA statements with the whole
offset in voffset, and a Makefile that builds the file with the dense kernels' flags."""
import os
import re
import subprocess
import tempfile

import pytest

from test_isa_audit import makefile_flags
from test_varlen_bwd_isa import BUDGET, HIPCC, ROOT

STEM = "fa_bwd_window_kernels"
KERNELS = ("bwd_dq_window_kernel", "bwd_dkdv_window_kernel")
ROW = r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"


@pytest.fixture(scope="module")
def listing():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    flags = makefile_flags(STEM)
    src = os.path.join(ROOT, "flash_attention_metal_amd", "csrc", STEM + ".hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", src, "-o", out],
                           cwd=tmp, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(out).read(), r.stderr


def test_names_stay_clear_of_the_existing_counts():
    # tests/test_varlen_bwd_isa.py and tests/test_isa_audit.py count the kernels of the two existing backward files by these substrings
    for k in KERNELS:
        assert "bwd_dq_varlen_kernel" not in k and "bwd_dkdv_varlen_kernel" not in k and k.startswith("bwd_")


def test_makefile_builds_the_new_translation_unit_with_the_dense_flags():
    text = open(os.path.join(ROOT, "flash_attention_metal_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bfa_bwd_window_kernels\.hip\b", text, re.M)
    assert re.search(r"^ASM_KERNELS\s*:=.*\bfa_bwd_window_kernels\b", text, re.M)
    flags = makefile_flags(STEM)
    assert flags == makefile_flags("fa_bwd_kernels") == makefile_flags("fa_bwd_varlen_kernels")
    assert "-fno-honor-nans" in flags and "-fno-slp-vectorize" in flags


def test_all_eight_kernels_fit_their_occupancy_without_scratch(listing):
    _, remarks = listing
    seen = {n: (int(vg), int(ag), int(sc), int(occ)) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S)}
    # nothing but the kernels: the shared bodies are part of them, not functions beside them
    assert all(any(re.match(r"_ZN2fa\d+" + k + "I", n) for k in KERNELS) for n in seen), sorted(seen)
    # {dq, dkdv} x {f16, bf16} x {64, 128}
    assert len(seen) == 8, sorted(seen)
    assert {("dq" if "bwd_dq_" in n else "dkdv", "F16" if "3F16" in n else "BF16", int(re.search(r"ELi(\d+)E", n).group(1))) for n in seen} == \
        {(k, t, d) for k in ("dq", "dkdv") for t in ("F16", "BF16") for d in (64, 128)}
    for name, (vg, ag, scratch, occ) in seen.items():
        want = 3 if "ELi64E" in name else 2
        allowed = 32 if ("bwd_dkdv_" in name and "ELi128E" in name) else 0  # the ceiling the dense kernel of that shape already has
        assert scratch <= allowed, (name, scratch)
        assert vg + ag <= BUDGET[want] and occ >= want, (name, vg, ag, occ, want)


def test_lds_dma_statements_own_m0(listing):
    text, _ = listing
    found = 0
    for name in re.findall(r"^(_ZN2fa\d+bwd_(?:dq|dkdv)_window_kernelI\S+):", text, re.M):
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
                    # as in the varlen kernels: the whole offset is in voffset, inside the descriptor's range check; soffset is 0
                    assert re.search(r"\], 0 offen lds$", u), (name, ln, u)
                    dma += 1
        assert dma > 0, name
        found += 1
    assert found == 8
