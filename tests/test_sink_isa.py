"""What the compiler made of the attention-sink kernels (cross-compiled here, no GPU; the approach of tests/test_window_isa.py): exactly
the eight 128-row sink kernels, no scratch, the window kernels' occupancy (three workgroups per CU at head_dim 64, two at 128), the M0
convention of their LDS-DMA statements; no scratch in the decode's sink combine and in the dsink reduction; names that none of the
existing counts match; a Makefile that builds the new translation unit."""
import os
import re

import pytest

from test_varlen_paged_isa import BUDGET, _compile
from test_window_isa import ROW, _audit_m0

KERNELS = ("fwd_mfma_sink_kernel", "fwd_mfma_sink_paged_kernel")
COMBINE, DSINK = "decode_combine_sink_kernel", "dsink_kernel"
PARAMS = ("VarlenSinkParams", "VarlenPagedSinkParams", "CombineSinkParams")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def forward():
    return _compile("fa_mfma_kernel")


def is_sink_forward(name):
    return any(re.match(r"_ZN2fa\d+" + k + "I", name) for k in KERNELS)


def test_names_stay_clear_of_the_existing_counts():
    # test_window_isa.py, test_varlen_isa.py, test_varlen_paged_isa.py, test_decode_paged_abi.py, test_window_bwd_isa.py and
    # test_isa_audit.py count kernels by these substrings and patterns
    for k in KERNELS + (COMBINE, DSINK):
        for taken in ("fwd_mfma_varlen_kernel", "fwd_mfma_varlen_paged_kernel", "fwd_mfma_window_kernel", "fwd_mfma_window_paged_kernel",
                      "decode_partial_kernel", "decode_combine_kernel", "kv_append_paged_kernel", "bwd_"):
            assert taken not in k, (k, taken)
        assert not re.match(r"fwd_mfma_window_(?:paged_)?kernel", k)
    for p in PARAMS:
        assert "DecodeWindowParams" not in p and "DecodePagedParams" not in p
    assert all(k.startswith("fwd_") for k in KERNELS)  # test_isa_audit.py holds every forward kernel to no scratch: these too


def test_makefile_builds_the_dsink_translation_unit():
    text = open(os.path.join(ROOT, "flash_attention_metal_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bfa_sink_kernels\.hip\b", text, re.M)


def test_forward_kernels_fit_their_occupancy_without_scratch(forward):
    _, remarks = forward
    seen = {n: (int(vg), int(ag), int(sc), int(occ)) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S) if is_sink_forward(n)}
    # {varlen, varlen paged} x {f16, bf16} x {64, 128}
    assert {(("paged" in n), ("F16" if "3F16" in n else "BF16"), int(re.search(r"ELi(\d+)E", n).group(1))) for n in seen} == \
        {(p, t, d) for p in (False, True) for t in ("F16", "BF16") for d in (64, 128)}
    assert len(seen) == 8, sorted(seen)
    for name, (vg, ag, scratch, occ) in seen.items():
        want = 3 if "ELi64E" in name else 2
        assert scratch == 0, (name, scratch)
        assert vg + ag <= BUDGET[want] and occ >= want, (name, vg, ag, occ, want)


def test_combine_and_dsink_kernels_use_no_scratch():
    _, remarks = _compile("fa_decode_kernel")
    comb = {n: int(sc) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S) if COMBINE in n}
    # {f16, bf16} x {64, 128} x {16, 32 packed rows}: the plain combine's instantiations of the paged decode
    assert len(comb) == 8 and all(sc == 0 for sc in comb.values()), comb
    _, remarks = _compile("fa_sink_kernels")
    rows = {n: int(sc) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S)}
    assert len(rows) == 1 and DSINK in next(iter(rows)) and next(iter(rows.values())) == 0, rows


def test_lds_dma_statements_own_m0(forward):
    assert _audit_m0(forward[0], r"_ZN2fa\d+fwd_mfma_sink_(?:paged_)?kernelI\S+", lambda n: True) == 8
