"""What the compiler made of the key-split kernels of the paged prefill (cross-compiled here, no GPU; the approach of
tests/test_varlen_paged_isa.py): four partial kernels at the occupancy of fwd_mfma_window_paged_kernel -- three workgroups per CU at
head_dim 64, two at 128 -- and eight combine kernels ({f16, bf16} x {64, 128} x {without, with} the sink), none with scratch; and names
that none of the existing ISA tests' patterns match."""
import re

import pytest

from test_varlen_paged_isa import BUDGET, _compile

PARTIAL, COMBINE = "fwd_mfma_ksplit_paged_kernel", "ksplit_combine_kernel"
# the substrings by which the other ISA tests count their kernels in this listing
OTHERS = ("fwd_mfma_varlen_kernel", "fwd_mfma_varlen_paged_kernel", "fwd_mfma_window_kernel", "fwd_mfma_window_paged_kernel", "fwd_mfma_sink_kernel",
          "fwd_mfma_sink_paged_kernel", "fwd_mfma_softcap_kernel", "fwd_mfma_softcap_paged_kernel", "fwd_mfma_kv8_kernel", "fwd_mfma_kv8_sink_kernel",
          "decode_combine_kernel", "decode_combine_sink_kernel", "decode_partial_kernel", "kv_append_paged_kernel")


@pytest.fixture(scope="module")
def remarks():
    return _compile("fa_mfma_kernel")[1]


def rows_of(remarks, word):
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)",
                      remarks, re.S)
    return {n: (int(vg), int(ag), int(sc), int(occ)) for n, vg, ag, sc, occ in rows if word in n}


def kinds(names):
    return {(("F16" if "3F16" in n else "BF16"), int(re.search(r"ELi(\d+)E", n).group(1))) for n in names}


def test_partial_kernels_keep_the_window_kernels_occupancy_without_scratch(remarks):
    seen = rows_of(remarks, PARTIAL)
    assert len(seen) == 4 and kinds(seen) == {(t, d) for t in ("F16", "BF16") for d in (64, 128)}, sorted(seen)
    window = rows_of(remarks, "fwd_mfma_window_paged_kernel")
    assert len(window) == 4
    for name, (vg, ag, scratch, occ) in seen.items():
        d = int(re.search(r"ELi(\d+)E", name).group(1))
        want = {64: 3, 128: 2}[d]
        assert scratch == 0, (name, scratch)
        assert vg + ag <= BUDGET[want] and occ == want, (name, vg, ag, occ, want)
        twin = [v for n, v in window.items() if kinds([n]) == kinds([name])]
        assert len(twin) == 1 and twin[0][3] == occ, (name, twin)


def test_combine_kernels_use_no_scratch(remarks):
    seen = rows_of(remarks, COMBINE)
    assert len(seen) == 8 and kinds(seen) == {(t, d) for t in ("F16", "BF16") for d in (64, 128)}, sorted(seen)
    assert sum("ELb1E" in n for n in seen) == 4  # the sink instantiations
    assert all(v[2] == 0 for v in seen.values()), seen


def test_names_stay_clear_of_the_existing_counts(remarks):
    for word in OTHERS:
        assert word not in PARTIAL and word not in COMBINE and PARTIAL not in word and COMBINE not in word, word
    for name in list(rows_of(remarks, PARTIAL)) + list(rows_of(remarks, COMBINE)):
        assert not any(w in name for w in OTHERS), name
