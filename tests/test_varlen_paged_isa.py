"""What the compiler made of the varlen paged kernels (cross-compiled here, no GPU; the approach of tests/test_varlen_isa.py): exactly the
eight attention kernels, no scratch, the register budget of the occupancy their __launch_bounds__ declare, the M0 convention of their
LDS-DMA statements -- and no scratch in the append kernels."""
import os
import re
import subprocess
import tempfile

import pytest

from test_isa_audit import makefile_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
# waves per SIMD = workgroups per CU for these four-wave workgroups -> registers per lane (512 in all, allocated in blocks of 8)
BUDGET = {4: 128, 3: 168, 2: 256}
KERNEL = "fwd_mfma_varlen_paged_kernel"
MANGLED = "_ZN2fa28" + KERNEL


def declared_occupancy(name):
    """fwd_mfma_varlen_paged_kernel<Tag, D, CAUSAL>: the varlen kernels' occupancy (csrc/fa_mfma_kernel.hip, varlen_paged_occupancy):
    head_dim 64 under the mask four workgroups per CU, without the mask three; head_dim 128 two."""
    d = int(re.search(r"ELi(\d+)E", name).group(1))
    causal = "ELb1E" in name
    return {64: 4 if causal else 3, 128: 2}[d]


def _compile(unit):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "flash_attention_metal_amd", "csrc", unit + ".hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run([HIPCC] + makefile_flags(unit) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S", src, "-o", out],
                           cwd=tmp, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(out).read(), r.stderr


@pytest.fixture(scope="module")
def listing():
    return _compile("fa_mfma_kernel")


def test_varlen_paged_kernels_fit_their_occupancy_without_scratch(listing):
    _, remarks = listing
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)",
                      remarks, re.S)
    seen = {n: (int(vg), int(ag), int(sc), int(occ)) for n, vg, ag, sc, occ in rows if KERNEL in n}
    # {f16, bf16} x {64, 128} x {causal, full}
    assert len(seen) == 8, sorted(seen)
    assert {(("F16" if "3F16" in n else "BF16"), int(re.search(r"ELi(\d+)E", n).group(1)), "ELb1E" in n) for n in seen} == \
        {(t, d, c) for t in ("F16", "BF16") for d in (64, 128) for c in (False, True)}
    for name, (vg, ag, scratch, occ) in seen.items():
        want = declared_occupancy(name)
        assert scratch == 0, (name, scratch)
        assert vg + ag <= BUDGET[want] and occ == want, (name, vg, ag, occ, want)


def test_varlen_paged_lds_dma_statements_own_m0(listing):
    text, _ = listing
    found = 0
    for name in re.findall(r"^(" + MANGLED + r"\S+):", text, re.M):
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
        assert dma > 0, name
        found += 1
    assert found == 8


def test_the_varlen_kernels_keep_their_names_apart():
    # tests/test_varlen_isa.py finds its eight kernels by these two substrings: the new kernels must not match them
    assert "fwd_mfma_varlen_kernel" not in KERNEL and not MANGLED.startswith("_ZN2fa22fwd_mfma_varlen_kernel")


def test_append_kernels_use_no_scratch():
    _, remarks = _compile("fa_decode_kernel")
    rows = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", remarks, re.S)
    seen = {n: int(sc) for n, sc in rows if "kv_append_paged_kernel" in n}
    assert len(seen) == 2, sorted(seen)  # element sizes 1 and 2
    assert all(sc == 0 for sc in seen.values()), seen
