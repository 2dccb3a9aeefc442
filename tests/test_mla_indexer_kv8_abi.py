"""CPU: the C-ABI of the e4m3 MLA indexer (include/fa_mi355.h, "The MLA indexer (e4m3 keys)") -- the three symbols against the header, the
support table, each rule of the calls' own with one value inside and one outside (fake aligned pointers: nothing may launch), and the
16-bit calls' rules textually equal after the function name on the same bad argument."""
import pytest

from test_mla_abi import BF16, FP8, INT_OK, ODD, OK, fa, header_args, lib  # noqa: F401  (fa, lib: fixtures)
from test_mla_indexer_abi import F_ODD, LOGITS, TOPK, logits_call, text, topk_call

LOGITS8, TOPK8 = LOGITS + "_kv8", TOPK + "_kv8"


def logits8(lib, q=OK, w=OK, k=OK, ks=INT_OK, lg=OK, cu=INT_OK, bt=INT_OK, sl=INT_OK, B=2, Hi=64, T=8, mq=4, Di=128, P_=64, num_pages=100, mp=8,
            qs=(64 * 128, 128), wrs=64, kps=64 * 128, krs=128, sps=64, bts=8, ls=512, qd=FP8, kd=FP8, **_):
    return lib.fa_mla_indexer_logits_paged_kv8(q, w, k, ks, lg, cu, bt, sl, B, Hi, T, mq, Di, P_, num_pages, mp, *qs, wrs, kps, krs, sps, bts, ls,
                                               qd, kd, None)


def topk8(lib, q=OK, w=OK, k=OK, ks=INT_OK, idx=OK, cnt=INT_OK, cu=INT_OK, bt=INT_OK, sl=INT_OK, B=2, Hi=64, T=8, mq=4, Di=128, topk=64, P_=64,
          num_pages=100, mp=8, qs=(64 * 128, 128), wrs=64, kps=64 * 128, krs=128, sps=64, bts=8, ist=64, qd=FP8, kd=FP8, ws=OK,
          wsb=8 * 512 * 4, **_):
    return lib.fa_mla_indexer_topk_paged_kv8(q, w, k, ks, idx, cnt, cu, bt, sl, B, Hi, T, mq, Di, topk, P_, num_pages, mp, *qs, wrs, kps, krs, sps,
                                             bts, ist, qd, kd, ws, wsb, None)


CALLS = [(logits8, LOGITS8, logits_call, LOGITS), (topk8, TOPK8, topk_call, TOPK)]


def test_symbols_and_the_support_table(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((LOGITS8, 27), (TOPK8, 31), ("fa_mla_indexer_kv8_supported", 5)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds), name
    sup = lib.fa_mla_indexer_kv8_supported
    assert all(sup(FP8, FP8, h, 128, p) == 1 for h in (32, 64) for p in (16, 32, 64, 128, 256))
    assert not any(sup(*a) for a in ((BF16, FP8, 64, 128, 64), (FP8, BF16, 64, 128, 64), (BF16, BF16, 64, 128, 64), (FP8, FP8, 16, 128, 64),
                                     (FP8, FP8, 128, 128, 64), (FP8, FP8, 64, 64, 64), (FP8, FP8, 64, 128, 48)))
    assert lib.fa_mla_indexer_supported(FP8, 64, 128, 64) == 0 and lib.fa_version() == 400
    for mine, name, _, _ in CALLS:
        for kw, word in (({"qd": BF16}, "q=bf16 kv=fp8_e4m3"), ({"kd": BF16}, "q=fp8_e4m3 kv=bf16"), ({"Hi": 48}, "Hi=48"), ({"P_": 48}, "page_size=48")):
            assert mine(lib, **kw) == -2 and word in text(lib, name), (name, kw)


@pytest.mark.parametrize("mine,name,wide,wide_name", CALLS)
def test_rules_of_their_own_and_the_shared_ones(lib, mine, name, wide, wide_name):
    # inside: byte strides that are multiples of 16, and (the composite, whose workspace rule comes behind the scales') a scale stride of P
    # and the packed page's 33 P -- each gets as far as a later rule
    late, word = ({"wsb": 1}, "workspace of 1 bytes") if mine is topk8 else ({"ls": 511}, "logits_stride=511")
    for kw in [{"qs": (64 * 128 + 16, 144), "krs": 144, "kps": 64 * 144}] + ([{"sps": 64}, {"sps": 33 * 64, "kps": 132 * 64}] if mine is topk8 else []):
        assert mine(lib, **kw, **late) == -1 and word in text(lib, name), (name, kw, lib.fa_last_error())
    for kw, word in (({"ks": None}, "null pointer"), ({"ks": F_ODD}, "k_scale_pages must be fp32-aligned"),
                     ({"sps": 63}, "k_scale_page_stride=63 < page_size=64"), ({"qs": (64 * 128, 136)}, "multiples of 16"),
                     ({"qs": (64 * 128 + 8, 128)}, "multiples of 16"), ({"krs": 136}, "bad page strides"), ({"kps": 64 * 128 + 8}, "bad page strides")):
        assert mine(lib, **kw) == -1 and word in text(lib, name), (name, kw, lib.fa_last_error())
    # shared with the 16-bit call: the same status and the same text behind the function name
    for kw in ({"q": None}, {"mq": 9}, {"bts": 7}, {"k": ODD}, {"wrs": 63}, {"mp": 1 << 25, "bts": 1 << 25, "ls": 1 << 31, "wsb": 1 << 60}):
        assert mine(lib, **kw) == -1 and wide(lib, **kw) == -1, kw
        got = text(lib, wide_name)
        assert mine(lib, **kw) == -1 and text(lib, name) == got, (kw, got)
