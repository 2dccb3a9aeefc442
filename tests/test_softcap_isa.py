"""What the compiler made of the soft-capping kernels (cross-compiled here, no GPU; the approach of tests/test_sink_isa.py and
tests/test_window_bwd_isa.py): exactly the eight 128-row kernels, the twelve decode partial kernels and the eight backward kernels; no
scratch at the window kernels' occupancy (three workgroups per CU at head_dim 64, two at 128; the decode no lower than its windowed twin;
the head_dim-128 dK/dV kernel within the 32 bytes the dense kernel of that shape is allowed); the M0 convention of their LDS-DMA
statements; names that none of the existing counts match; a Makefile that builds the new translation unit with the backward's flags."""
import os
import re

import pytest

from test_isa_audit import makefile_flags
from test_varlen_paged_isa import BUDGET, _compile
from test_window_isa import ROW, _audit_m0

KERNELS = ("fwd_mfma_softcap_kernel", "fwd_mfma_softcap_paged_kernel")
BWD_KERNELS = ("bwd_dq_softcap_kernel", "bwd_dkdv_softcap_kernel")
PARAMS = ("VarlenSoftcapParams", "VarlenPagedSoftcapParams", "DecodeSoftcapParams", "BwdSoftcapParams")
STEM = "fa_bwd_softcap_kernels"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def forward():
    return _compile("fa_mfma_kernel")


@pytest.fixture(scope="module")
def decode():
    return _compile("fa_decode_kernel")


@pytest.fixture(scope="module")
def backward():
    return _compile(STEM)


def is_softcap_forward(name):
    return any(re.match(r"_ZN2fa\d+" + k + "I", name) for k in KERNELS)


def test_names_stay_clear_of_the_existing_counts():
    # test_window_isa.py, test_sink_isa.py, test_varlen_isa.py, test_varlen_paged_isa.py, test_varlen_paged_kv8_isa.py,
    # test_decode_paged_abi.py, test_window_bwd_isa.py, test_varlen_bwd_isa.py and test_isa_audit.py count kernels by these
    for k in KERNELS:
        for taken in ("fwd_mfma_varlen_kernel", "fwd_mfma_varlen_paged_kernel", "fwd_mfma_window_kernel", "fwd_mfma_window_paged_kernel",
                      "fwd_mfma_sink_kernel", "fwd_mfma_sink_paged_kernel", "fwd_mfma_kv8_kernel", "fwd_mfma_kv8_sink_kernel", "fwd_mfma_kernel",
                      "decode_partial_kernel", "decode_combine_kernel", "kv_append_paged_kernel", "bwd_"):
            assert taken not in k, (k, taken)
        assert not re.match(r"fwd_mfma_(?:window|sink)_(?:paged_)?kernel", k) and k.startswith("fwd_")
    for k in BWD_KERNELS:
        for taken in ("bwd_dq_varlen_kernel", "bwd_dkdv_varlen_kernel", "bwd_dq_window_kernel", "bwd_dkdv_window_kernel", "bwd_dq_kernel", "bwd_dkdv_kernel"):
            assert taken not in k, (k, taken)
        assert not re.match(r"bwd_(?:dq|dkdv)_(?:varlen|window)_kernel", k) and k.startswith("bwd_")
    for p in PARAMS:
        for taken in ("DecodeWindowParams", "DecodePagedParams", "VarlenSinkParams", "VarlenPagedSinkParams", "CombineSinkParams",
                      "VarlenPagedKv8Params", "VarlenPagedKv8SinkParams"):
            assert taken not in p, (p, taken)


def test_makefile_builds_the_translation_unit_with_the_backward_flags():
    text = open(os.path.join(ROOT, "flash_attention_metal_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\b" + STEM + r"\.hip\b", text, re.M)
    assert re.search(r"^ASM_KERNELS\s*:=.*\b" + STEM + r"\b", text, re.M)
    assert makefile_flags(STEM) == makefile_flags("fa_bwd_kernels") == makefile_flags("fa_bwd_window_kernels")


def test_forward_kernels_fit_their_occupancy_without_scratch(forward):
    _, remarks = forward
    seen = {n: (int(vg), int(ag), int(sc), int(occ)) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S) if is_softcap_forward(n)}
    # {varlen, varlen paged} x {f16, bf16} x {64, 128}
    assert {(("paged" in n), ("F16" if "3F16" in n else "BF16"), int(re.search(r"ELi(\d+)E", n).group(1))) for n in seen} == \
        {(p, t, d) for p in (False, True) for t in ("F16", "BF16") for d in (64, 128)}
    assert len(seen) == 8, sorted(seen)
    for name, (vg, ag, scratch, occ) in seen.items():
        want = 3 if "ELi64E" in name else 2
        assert scratch == 0, (name, scratch)
        assert vg + ag <= BUDGET[want] and occ >= want, (name, vg, ag, occ, want)


def test_decode_kernels_are_the_windowed_twins_and_use_no_scratch(decode):
    _, remarks = decode
    rows = {n: (int(sc), int(occ)) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S) if "decode_partial_kernel" in n}
    cap = {n: v for n, v in rows.items() if "DecodeSoftcapParams" in n}

    def key(n):  # (Tag, D, QT, KV8) of decode_partial_kernel<Tag, D, QT, CAUSAL, KV8, PRM>
        m = re.search(r"decode_partial_kernelINS_\d(B?F16)ELi(\d+)ELi(\d)ELb([01])ELb([01])E", n)
        return m.group(1), int(m.group(2)), int(m.group(3)), m.group(5) == "1"

    win = {key(n): v for n, v in rows.items() if "DecodeWindowParams" in n}
    assert {key(n) for n in cap} == set(win) and len(cap) == 12 and len(win) == 12, sorted(cap)
    assert all("ELb1ELb" in n for n in cap)  # instantiated under the upper bound, as the windowed ones
    assert all(sc == 0 for sc, _ in cap.values()), cap
    for n, (_, occ) in cap.items():  # an occupancy no lower than the windowed twin of the same shape
        assert occ >= win[key(n)][1], (n, occ, win[key(n)])


def test_backward_kernels_fit_their_occupancy(backward):
    _, remarks = backward
    seen = {n: (int(vg), int(ag), int(sc), int(occ)) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S)}
    assert all(any(re.match(r"_ZN2fa\d+" + k + "I", n) for k in BWD_KERNELS) for n in seen), sorted(seen)
    assert {(("dkdv" in n), ("F16" if "3F16" in n else "BF16"), int(re.search(r"ELi(\d+)E", n).group(1))) for n in seen} == \
        {(p, t, d) for p in (False, True) for t in ("F16", "BF16") for d in (64, 128)}
    assert len(seen) == 8, sorted(seen)
    for name, (vg, ag, scratch, occ) in seen.items():
        want = 3 if "ELi64E" in name else 2
        # head_dim 64: no scratch; 128: at most the 32 bytes tests/test_isa_audit.py allows the dense dK/dV kernel of that shape
        allowed = 32 if ("ELi128E" in name and "dkdv" in name) else 0
        assert scratch <= allowed, (name, scratch)
        assert vg + ag <= BUDGET[want] and occ >= want, (name, vg, ag, occ, want)


def test_softcap_arithmetic_is_in_the_new_kernels_only(forward, decode, backward):
    """tanh costs one v_rcp_f32 per score: the reciprocal shows the mode was compiled in (the first build of the backward file compiled the
    window kernels under new names), and its count per kernel that it was compiled in once per score of a tile."""
    for text, pat, per in ((forward[0], r"_ZN2fa\d+fwd_mfma_softcap_(?:paged_)?kernelI\S+", 32), (backward[0], r"_ZN2fa\d+bwd_(?:dq|dkdv)_softcap_kernelI\S+", 32),
                           (decode[0], r"_ZN2fa\d+decode_partial_kernelI\S+DecodeSoftcapParams\S*", 16)):
        names = re.findall(r"^(" + pat + r"):", text, re.M)
        assert names
        for name in names:
            start = re.search(r"^" + re.escape(name) + r":", text, re.M).start()
            body = text[start:text.index(".Lfunc_end", start)]
            assert len(re.findall(r"\bv_rcp_f32", body)) >= per, name


def test_lds_dma_statements_own_m0(forward, decode, backward):
    assert _audit_m0(forward[0], r"_ZN2fa\d+fwd_mfma_softcap_(?:paged_)?kernelI\S+", lambda n: True) == 8
    # (the e4m3 decode kernels stage through registers: no LDS-DMA statement to audit there)
    assert _audit_m0(decode[0], r"_ZN2fa\d+decode_partial_kernelI\S+DecodeSoftcapParams\S*", lambda n: "ELb1ELb0E" in n) == 12
    assert _audit_m0(backward[0], r"_ZN2fa\d+bwd_(?:dq|dkdv)_softcap_kernelI\S+", lambda n: True) == 8
