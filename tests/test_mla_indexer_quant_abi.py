"""CPU: the C-ABI of the e4m3 indexer's input stage (include/fa_mi355.h, "The MLA indexer's input stage") -- the three symbols against the
header, the support table, the calls' own rules and a sample of the shared ones, textually identical to fa_mla_kv_append_paged_scaled's
and the indexer's after the function name, each with its status and text (fake aligned pointers: nothing may launch)."""
import pytest

from test_mla_abi import BF16, F16, F32, FP8, INT_OK, INT_ODD, ODD, OK, P, fa, header_args, lib  # noqa: F401  (fa, lib: fixtures)
from test_mla_indexer_abi import F_ODD, logits_call, text

KAPPEND, QQUANT, SCALED, LOGITS = "fa_mla_indexer_k_append_paged_quant", "fa_mla_indexer_q_quant", "fa_mla_kv_append_paged_scaled", "fa_mla_indexer_logits_paged"


def k_call(lib, new=OK, k=OK, ks=OK, cu=INT_OK, bt=INT_OK, sl=INT_OK, B=2, T=8, mn=4, Di=128, P_=64, num_pages=100, mp=8, nrs=128, kps=64 * 128,
           krs=128, ksps=64, bts=8, rotate=1, dtype=BF16, **_):
    return lib.fa_mla_indexer_k_append_paged_quant(new, k, ks, cu, bt, sl, B, T, mn, Di, P_, num_pages, mp, nrs, kps, krs, ksps, bts, rotate, dtype, None)


def scaled_twin(lib, new=OK, k=OK, cu=INT_OK, bt=INT_OK, sl=INT_OK, B=2, T=8, mn=4, P_=64, num_pages=100, mp=8, bts=8, **_):
    return lib.fa_mla_kv_append_paged_scaled(new, k, cu, bt, sl, B, T, mn, P_, num_pages, mp, 576, 64 * 656, 656, bts, BF16, None)


def q_call(lib, q=OK, hw=OK, qo=OK, wo=OK, T=8, Hi=64, Di=128, w_mul=0.5, qs=(64 * 128, 128), wrs=64, qos=(64 * 128, 128), wors=64, rotate=1,
           dtype=BF16, **_):
    return lib.fa_mla_indexer_q_quant(q, hw, qo, wo, T, Hi, Di, w_mul, *qs, wrs, *qos, wors, rotate, dtype, None)


def test_symbols_match_the_headers_argument_lists(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((KAPPEND, 21), (QQUANT, 17), ("fa_mla_indexer_quant_supported", 2)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds) and hasattr(lib, name), name
    assert lib.fa_version() == 400


def test_support_table_and_refusals_that_name_what_was_given(lib):
    sup = lib.fa_mla_indexer_quant_supported
    assert sup(F16, 128) == 1 and sup(BF16, 128) == 1 and not any(sup(*a) for a in ((F32, 128), (FP8, 128), (BF16, 64), (BF16, 256), (9, 128)))
    for call, name, kw, word in ((k_call, KAPPEND, {"dtype": F32}, "new_dtype=f32"), (k_call, KAPPEND, {"Di": 64, "nrs": 64}, "Di=64"),
                                 (k_call, KAPPEND, {"P_": 48}, "page_size=48"), (k_call, KAPPEND, {"dtype": FP8}, "new_dtype=fp8_e4m3"),
                                 (q_call, QQUANT, {"dtype": F32}, "dtype=f32"), (q_call, QQUANT, {"Di": 256}, "Di=256")):
        assert call(lib, **kw) == -2 and word in text(lib, name), (name, kw)


SHARED = [({"new": None}, "null pointer"), ({"sl": None}, "null pointer"), ({"B": 0}, "sizes must be >= 1"), ({"num_pages": 0}, "sizes must be >= 1"),
          ({"mn": 9}, "max_seqlen_new=9 exceeds the token count 8"), ({"bts": 7}, "block_table_stride=7"), ({"bt": INT_ODD}, "int32-aligned"),
          ({"mp": 1 << 25, "bts": 1 << 25}, "capacity above 2^30 keys"), ({"new": ODD}, "tensors must be 16-byte aligned"),
          ({"k": ODD}, "tensors must be 16-byte aligned"), ({"cu": INT_ODD}, "cu_seqlens_new must be int32-aligned"),
          ({"B": 1 << 30, "T": 1 << 30, "mn": 8}, "grid too large")]


def test_shared_rules_carry_the_other_calls_status_and_text(lib):
    for kw, word in SHARED:
        assert k_call(lib, **kw) == -1, kw
        got = text(lib, KAPPEND)
        assert scaled_twin(lib, **kw) == -1 and got == text(lib, SCALED) and word in got, (kw, got)
    # the pool's byte strides are the e4m3 logits call's rule, q_idx's element strides the 16-bit indexer call's
    for kw in ({"krs": 120}, {"kps": 64 * 128 + 8}):
        assert k_call(lib, **kw) == -1 and "bad page strides" in text(lib, KAPPEND), kw
    for qs in ((64 * 128, 120), (64 * 128 + 4, 128)):
        assert q_call(lib, qs=qs) == -1, qs
        got = text(lib, QQUANT)
        assert logits_call(lib, qs=qs) == -1 and got == text(lib, LOGITS) and "bad strides" in got, (qs, got)


def test_rules_of_their_own(lib):
    own = [(k_call, KAPPEND, {"ks": None}, "null pointer"), (k_call, KAPPEND, {"ks": F_ODD}, "k_scale_pages must be fp32-aligned"),
           (k_call, KAPPEND, {"ksps": 63}, "k_scale_page_stride=63 < page_size=64"), (k_call, KAPPEND, {"nrs": 132}, "bad new key/value strides"),
           (q_call, QQUANT, {"q": None}, "null pointer"), (q_call, QQUANT, {"wo": None}, "null pointer"), (q_call, QQUANT, {"Hi": 0}, "sizes must be >= 1"),
           (q_call, QQUANT, {"w_mul": 0.0}, "w_mul=0 must be > 0 and finite"), (q_call, QQUANT, {"w_mul": float("inf")}, "must be > 0 and finite"),
           (q_call, QQUANT, {"w_mul": float("nan")}, "must be > 0 and finite"), (q_call, QQUANT, {"qos": (64 * 128, 120)}, "bad output strides"),
           (q_call, QQUANT, {"qos": (64 * 128 + 8, 128)}, "strides are multiples of 16"), (q_call, QQUANT, {"q": ODD}, "tensors must be 16-byte aligned"),
           (q_call, QQUANT, {"qo": ODD}, "tensors must be 16-byte aligned"), (q_call, QQUANT, {"hw": F_ODD}, "head_w must be fp32-aligned"),
           (q_call, QQUANT, {"wo": F_ODD}, "w_out must be fp32-aligned"), (q_call, QQUANT, {"wrs": 63}, "w_row_stride=63 < Hi=64"),
           (q_call, QQUANT, {"wors": 63}, "wo_row_stride=63 < Hi=64"), (q_call, QQUANT, {"T": 1 << 26, "Hi": 64}, "grid too large")]
    for call, name, kw, word in own:
        assert call(lib, **kw) == -1 and word in text(lib, name), (name, kw, lib.fa_last_error())
