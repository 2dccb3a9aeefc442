"""What the compiler made of the varlen backward kernels (cross-compiled here, no GPU; the approach of tests/test_varlen_isa.py): all
sixteen are there, none uses scratch, each stays inside the register budget of the occupancy its __launch_bounds__ declare, and
their LDS-DMA statements keep the M0 convention."""
import os
import re
import subprocess
import tempfile

import pytest

from test_isa_audit import makefile_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
STEM = "fa_bwd_varlen_kernels"
# waves per SIMD = workgroups per CU for these four-wave workgroups -> registers per lane (512 in all, allocated in blocks of 8)
BUDGET = {3: 168, 2: 256, 1: 512}


def declared_occupancy(name):
    """bwd_dq_varlen_kernel / bwd_dkdv_varlen_kernel <Tag, D, CAUSAL>: the dense kernels' occupancy (csrc/fa_bwd_varlen_kernels.hip,
    bwd_varlen_occ): three workgroups per CU at head_dim 64, two at 128."""
    return {64: 3, 128: 2}[int(re.search(r"ELi(\d+)E", name).group(1))]


@pytest.fixture(scope="module")
def listing():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    flags = makefile_flags(STEM)
    assert flags == makefile_flags("fa_bwd_kernels")  # the same bodies under other flags would not give the dense kernels' bits
    assert "-fno-honor-nans" in flags and "-fno-slp-vectorize" in flags
    src = os.path.join(ROOT, "flash_attention_metal_amd", "csrc", STEM + ".hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", src, "-o", out],
                           cwd=tmp, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(out).read(), r.stderr


def test_makefile_builds_and_lists_the_new_translation_unit():
    text = open(os.path.join(ROOT, "flash_attention_metal_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bfa_bwd_varlen_kernels\.hip\b", text, re.M)
    assert re.search(r"^ASM_KERNELS\s*:=.*\bfa_bwd_varlen_kernels\b", text, re.M)
    rule = re.search(r"^%\.o:(.*)$", text, re.M).group(1)
    for dep in ("fa_bwd_body.h", "fa_bwd_dq_body.inc", "fa_bwd_dkdv_body.inc"):
        assert dep in rule, dep


def test_all_sixteen_kernels_fit_their_occupancy_without_scratch(listing):
    _, remarks = listing
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)",
                      remarks, re.S)
    seen = {n: (int(vg), int(ag), int(sc), int(occ)) for n, vg, ag, sc, occ in rows}
    # nothing but the kernels: the shared bodies are part of them, not functions beside them
    assert all("bwd_dq_varlen_kernel" in n or "bwd_dkdv_varlen_kernel" in n for n in seen), sorted(seen)
    # {dq, dkdv} x {f16, bf16} x {64, 128} x {causal, full}
    assert len(seen) == 16, sorted(seen)
    assert {("dq" if "bwd_dq_" in n else "dkdv", "F16" if "3F16" in n else "BF16", int(re.search(r"ELi(\d+)E", n).group(1)), "ELb1E" in n) for n in seen} == \
        {(k, t, d, c) for k in ("dq", "dkdv") for t in ("F16", "BF16") for d in (64, 128) for c in (False, True)}
    for name, (vg, ag, scratch, occ) in seen.items():
        want = declared_occupancy(name)
        assert scratch == 0, (name, scratch)
        assert vg + ag <= BUDGET[want] and occ == want, (name, vg, ag, occ, want)


def test_lds_dma_statements_own_m0(listing):
    text, _ = listing
    found = 0
    for name in re.findall(r"^(_ZN2fa\d+bwd_(?:dq|dkdv)_varlen_kernel\S+):", text, re.M):
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
                    # varlen: the whole offset is in voffset, inside the descriptor's range check; soffset is the constant 0
                    assert re.search(r"\], 0 offen lds$", u), (name, ln, u)
                    dma += 1
        assert dma > 0, name
        found += 1
    assert found == 16
