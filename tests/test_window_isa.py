"""What the compiler made of the sliding-window kernels (cross-compiled here, no GPU; the approach of tests/test_varlen_paged_isa.py):
exactly the eight 128-row kernels and the twelve decode partial kernels, no scratch, the occupancy of the unmasked varlen kernel of
their head dim (three workgroups per CU at head_dim 64, two at 128), the M0 convention of their LDS-DMA statements."""
import re

import pytest

from test_varlen_paged_isa import BUDGET, _compile

KERNELS = ("fwd_mfma_window_kernel", "fwd_mfma_window_paged_kernel")
DECODE_PARAMS = "DecodeWindowParams"
ROW = r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"


@pytest.fixture(scope="module")
def forward():
    return _compile("fa_mfma_kernel")


@pytest.fixture(scope="module")
def decode():
    return _compile("fa_decode_kernel")


def is_window_forward(name):
    return any(re.match(r"_ZN2fa\d+" + k + "I", name) for k in KERNELS)


def test_names_stay_clear_of_the_existing_counts():
    # tests/test_varlen_isa.py, test_varlen_paged_isa.py and test_decode_paged_abi.py count kernels by these substrings
    for k in KERNELS:
        assert "fwd_mfma_varlen_kernel" not in k and "fwd_mfma_varlen_paged_kernel" not in k and k.startswith("fwd_")
    assert "DecodePagedParams" not in DECODE_PARAMS


def test_forward_kernels_fit_their_occupancy_without_scratch(forward):
    _, remarks = forward
    seen = {n: (int(vg), int(ag), int(sc), int(occ)) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S) if is_window_forward(n)}
    # {varlen, varlen paged} x {f16, bf16} x {64, 128}
    assert {(("paged" in n), ("F16" if "3F16" in n else "BF16"), int(re.search(r"ELi(\d+)E", n).group(1))) for n in seen} == \
        {(p, t, d) for p in (False, True) for t in ("F16", "BF16") for d in (64, 128)}
    assert len(seen) == 8, sorted(seen)
    for name, (vg, ag, scratch, occ) in seen.items():
        want = 3 if "ELi64E" in name else 2
        assert scratch == 0, (name, scratch)
        assert vg + ag <= BUDGET[want] and occ >= want, (name, vg, ag, occ, want)


def test_decode_kernels_are_the_support_tables_and_use_no_scratch(decode):
    _, remarks = decode
    rows = {n: (int(sc), int(occ)) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S) if "decode_partial_kernel" in n}
    win = {n: v for n, v in rows.items() if DECODE_PARAMS in n}

    def key(n):  # (Tag, D, QT, KV8) of decode_partial_kernel<Tag, D, QT, CAUSAL, KV8, PRM>
        m = re.search(r"decode_partial_kernelINS_\d(B?F16)ELi(\d+)ELi(\d)ELb([01])ELb([01])E", n)
        return m.group(1), int(m.group(2)), int(m.group(3)), m.group(5) == "1"

    # what fa_fwd_decode_paged_supported instantiates, once (the window mode has one flavour where the paged decode has causal / full):
    # {f16, bf16, e4m3 and bf16-on-e4m3 (one kernel: bf16 arithmetic on the widened cache)} x {64, 128} x {16, 32 packed rows}
    paged = {key(n) for n in rows if "DecodePagedParams" in n}
    assert {key(n) for n in win} == paged and len(win) == 12 and len(paged) == 12, sorted(win)
    assert all("ELb1ELb" in n for n in win)  # instantiated under the upper bound
    assert all(sc == 0 for sc, _ in win.values()), win
    # and an occupancy no lower than the paged decode's causal kernel of the same shape
    for n, (_, occ) in win.items():
        twin = [v for m, v in rows.items() if "DecodePagedParams" in m and key(m) == key(n) and "ELb1ELb" in m]
        assert len(twin) == 1 and occ >= twin[0][1], (n, occ, twin)


def _audit_m0(text, pattern, expect):
    found = 0
    for name in re.findall(r"^(" + pattern + r"):", text, re.M):
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
        if expect(name):
            assert dma > 0, name
        found += 1
    return found


def test_lds_dma_statements_own_m0(forward, decode):
    assert _audit_m0(forward[0], r"_ZN2fa\d+fwd_mfma_window_(?:paged_)?kernelI\S+", lambda n: True) == 8
    # (the e4m3 decode kernels stage through registers: no LDS-DMA statement to audit there)
    assert _audit_m0(decode[0], r"_ZN2fa\d+decode_partial_kernelI\S+" + DECODE_PARAMS + r"\S*", lambda n: "ELb1ELb0E" in n) == 12
