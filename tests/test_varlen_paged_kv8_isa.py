"""What the compiler made of the KV8 kernels (cross-compiled here, no GPU; the approach of tests/test_sink_isa.py): exactly the four
128-row kernels of fa_fwd_varlen_paged_kv8 -- the paged window and the paged sink mode at head_dim 64 and 128 --, no scratch, at least two
workgroups per CU (head_dim 64 keeps the bf16 kernels' three: README, round 19), no LDS-DMA statement (their tiles travel through
registers); no scratch in the quantising append kernels; names that none of the existing counts match."""
import re

import pytest

from test_varlen_paged_isa import BUDGET, _compile
from test_window_isa import ROW, _audit_m0

KERNELS = ("fwd_mfma_kv8_kernel", "fwd_mfma_kv8_sink_kernel")
APPEND = "kv_quant_append_paged_kernel"
PARAMS = ("VarlenPagedKv8Params", "VarlenPagedKv8SinkParams")


@pytest.fixture(scope="module")
def forward():
    return _compile("fa_mfma_kernel")


def is_kv8_forward(name):
    return any(re.match(r"_ZN2fa\d+" + k + "I", name) for k in KERNELS)


def test_names_stay_clear_of_the_existing_counts():
    # test_window_isa.py, test_varlen_isa.py, test_varlen_paged_isa.py, test_sink_isa.py, test_decode_paged_abi.py, test_window_bwd_isa.py
    # and test_isa_audit.py count kernels by these substrings and patterns
    for k in KERNELS + (APPEND,):
        for taken in ("fwd_mfma_varlen_kernel", "fwd_mfma_varlen_paged_kernel", "fwd_mfma_window_kernel", "fwd_mfma_window_paged_kernel",
                      "fwd_mfma_sink_kernel", "fwd_mfma_sink_paged_kernel", "fwd_mfma_kernel", "decode_partial_kernel", "decode_combine_kernel",
                      "decode_combine_sink_kernel", "dsink_kernel", "kv_append_paged_kernel", "bwd_"):
            assert taken not in k, (k, taken)
        assert not re.match(r"fwd_mfma_window_(?:paged_)?kernel", k) and not re.match(r"fwd_mfma_sink_(?:paged_)?kernel", k)
    for p in PARAMS:
        assert "DecodeWindowParams" not in p and "DecodePagedParams" not in p
    assert all(k.startswith("fwd_") for k in KERNELS)  # test_isa_audit.py holds every forward kernel to no scratch: these too


def test_four_forward_kernels_without_scratch_at_two_workgroups_or_more(forward):
    _, remarks = forward
    seen = {n: (int(vg), int(ag), int(sc), int(occ)) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S) if is_kv8_forward(n)}
    # {window, sink} x {64, 128}; bf16 queries only
    assert {("sink" in n, int(re.search(r"ILi(\d+)E", n).group(1))) for n in seen} == {(s, d) for s in (False, True) for d in (64, 128)}
    assert len(seen) == 4, sorted(seen)
    for name, (vg, ag, scratch, occ) in seen.items():
        assert scratch == 0, (name, scratch)
        assert occ >= 2 and vg + ag <= BUDGET[2], (name, vg, ag, occ)
        if "ILi64E" in name:  # the occupancy found and written into the README: three, as the bf16 paged window / sink kernels
            assert occ == 3 and vg + ag <= BUDGET[3], (name, vg, ag, occ)


def test_the_tiles_travel_through_registers(forward):
    text, _ = forward
    for name in re.findall(r"^(_ZN2fa\d+fwd_mfma_kv8_(?:sink_)?kernelI\S+):", text, re.M):
        start = re.search(r"^" + re.escape(name) + r":", text, re.M).start()
        body = text[start:text.index(".Lfunc_end", start)]
        assert not re.search(r"buffer_load\S* .* lds\s*$", body, re.M), name      # no LDS-DMA
        assert len(re.findall(r"v_cvt_pk_f32_fp8", body)) >= 16, name             # the widening
        assert "m0" not in re.sub(r";.*", "", body).replace(",", " ").split(), name
    # ... and the audit of the existing kernels' LDS-DMA statements finds none to look at here
    assert _audit_m0(text, r"_ZN2fa\d+fwd_mfma_kv8_(?:sink_)?kernelI\S+", lambda n: False) == 4


def test_quantising_append_kernels_use_no_scratch():
    _, remarks = _compile("fa_decode_kernel")
    rows = {n: int(sc) for n, vg, ag, sc, occ in re.findall(ROW, remarks, re.S) if APPEND in n}
    assert len(rows) == 2 and all(sc == 0 for sc in rows.values()), rows  # new rows of f16 and of bf16
