"""CPU: the C-ABI of fa_fwd_mla_decode_sparse_kv8_scaled and fa_mla_kv_append_paged_scaled (include/fa_mi355.h, "656-byte rows"): the
symbols against the header, each rule of their own with its status before any launch (fake aligned pointers: nothing may launch), the
rules shared with fa_fwd_mla_decode_sparse_kv8 with that call's text after the function name, and the workspace size."""
from test_mla_abi import BF16, F16, F32, FP8, INT_OK, ODD, OK, P, fa, header_args, lib  # noqa: F401  (fa, lib: fixtures)
from test_mla_sparse_kv8_abi import kv8_call

SCALED, KV8, APPEND = "fa_fwd_mla_decode_sparse_kv8_scaled", "fa_fwd_mla_decode_sparse_kv8", "fa_mla_kv_append_paged_scaled"


def scaled_call(lib, q=OK, kv=OK, o=OK, idx=OK, cnt=INT_OK, ws=OK, T=2, Hq=16, Dqk=576, Dv=512, topk=320, P_=64, num_pages=100, scale=0.0722,
                kps=64 * 656, krs=656, ist=320, q_dtype=BF16, kv_dtype=FP8, wsb=None):
    wsb = lib.fa_fwd_mla_decode_sparse_kv8_scaled_workspace_bytes(2, 16, 512, 320) if wsb is None else wsb
    return lib.fa_fwd_mla_decode_sparse_kv8_scaled(q, kv, o, None, idx, cnt, T, Hq, Dqk, Dv, topk, P_, num_pages, scale, Hq * 576, 576, Hq * 512,
                                                   512, kps, krs, ist, q_dtype, kv_dtype, ws, wsb, None)


def append_call(lib, new=OK, kv=OK, cu=INT_OK, bt=INT_OK, sl=INT_OK, B=2, total=40, max_new=21, P_=16, num_pages=50, mp=8, nrs=576, kps=16 * 656,
                krs=656, bts=8, dtype=BF16):
    return lib.fa_mla_kv_append_paged_scaled(new, kv, cu, bt, sl, B, total, max_new, P_, num_pages, mp, nrs, kps, krs, bts, dtype, None)


def last(lib):
    return lib.fa_last_error().decode()


def test_symbols_match_the_header_and_the_workspace_is_the_sparse_calls(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((SCALED, 26), (SCALED + "_workspace_bytes", 4), (SCALED + "_supported", 6), (APPEND, 17)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds) and hasattr(lib, name), name
    assert header_args(SCALED)[1] == header_args(KV8)[1]
    size, sparse = lib.fa_fwd_mla_decode_sparse_kv8_scaled_workspace_bytes, lib.fa_fwd_mla_decode_sparse_workspace_bytes
    for args in [(T, Hq, 512, topk) for T in (1, 3, 128, 5000) for Hq in (1, 16, 17, 64, 65, 128) for topk in (1, 64, 65, 2048, 1 << 20)]:
        assert size(*args) == sparse(*args) > 0, args
    for bad in ((0, 16, 512, 320), (2, 129, 512, 320), (2, 16, 576, 320), (2, 16, 512, 0), (2, 16, 512, (1 << 30) + 1)):
        assert size(*bad) == 0, bad
    sup = lib.fa_fwd_mla_decode_sparse_kv8_scaled_supported
    assert all(sup(BF16, FP8, 576, 512, hq, p) == 1 for hq in (1, 17, 128) for p in (16, 32, 64, 128, 256))
    assert not any(sup(*a) for a in ((F16, FP8, 576, 512, 16, 64), (BF16, BF16, 576, 512, 16, 64), (FP8, FP8, 576, 512, 16, 64),
                                     (BF16, FP8, 576, 512, 129, 64), (BF16, FP8, 656, 512, 16, 64), (BF16, FP8, 576, 512, 16, 48)))


def test_rules_of_the_attention_call_each_refused_before_any_launch(lib):
    def passes(**kw):  # as far as the workspace rule, the last one in front of the launch, under the sizer's own name
        assert scaled_call(lib, wsb=1, **kw) == -1 and last(lib).startswith(f"{SCALED}: workspace of 1 bytes, {SCALED}_workspace_bytes() asks for "), kw

    passes()
    passes(cnt=None)
    passes(krs=672, kps=64 * 672 + 16)
    for p in (16, 256):
        passes(P_=p, kps=p * 656)
    # the row: 656 bytes at least (576, the e4m3 call's row, and 640 are refused), strides multiples of 16, a 16-byte aligned base
    for kw in ({"krs": 576}, {"krs": 640}, {"kps": 640}, {"krs": 664, "kps": 64 * 664}, {"kps": 64 * 656 + 8}):
        assert scaled_call(lib, **kw) == -1 and last(lib) == SCALED + ": bad page strides", kw
    assert scaled_call(lib, kv=ODD) == -1 and last(lib) == SCALED + ": tensors and workspace must be 16-byte aligned"
    assert scaled_call(lib, P_=256, krs=1 << 23, kps=1 << 31) == -1 and last(lib) == SCALED + ": one page of one head exceeds 2 GiB"
    for kw, word in (({"q_dtype": F16}, "q=f16 kv=fp8_e4m3"), ({"kv_dtype": BF16}, "q=bf16 kv=bf16"), ({"q_dtype": FP8}, "q=fp8_e4m3"),
                     ({"Hq": 129}, "Hq=129"), ({"Dqk": 656}, "Dqk=656"), ({"P_": 48}, "page_size=48")):
        assert scaled_call(lib, **kw) == -2 and last(lib).startswith(SCALED + ": needs bf16 queries on an e4m3 pool of 656-byte rows") and word in last(lib), kw
    # every rule shared with the e4m3 call: the same status, the same text after the function name, on the same bad argument
    for kw in ({"idx": None}, {"topk": 0}, {"ist": 316}, {"ist": 322}, {"idx": ODD}, {"idx": P(0x2004)}, {"cnt": P(0x2002)}, {"scale": 0.0},
               {"num_pages": (1 << 24) + 1}, {"topk": (1 << 30) + 1, "ist": (1 << 30) + 4, "wsb": 1 << 60}, {"T": 1 << 23, "wsb": 1 << 60},
               {"q": ODD}, {"ws": ODD}, {"kps": 64 * 656 + 8}, {"P_": 256, "krs": 1 << 23, "kps": 1 << 31}):
        st, mine = scaled_call(lib, **kw), last(lib)
        other = dict(kw, kps=kw.get("kps", 64 * 576), krs=kw.get("krs", 576))  # (the e4m3 call's own legal strides where none is given)
        assert kv8_call(lib, **other) == st == -1 and mine.split(": ", 1) == [SCALED, last(lib).split(": ", 1)[1]], (kw, mine, last(lib))


def test_rules_of_the_append_each_refused_before_any_launch(lib):
    for kw, st, text in (({"new": None}, -1, "null pointer"), ({"total": 0}, -1, "sizes must be >= 1"),
                         ({"dtype": F16}, -2, "needs bf16 new rows of 576 elements"), ({"dtype": FP8}, -2, "new_dtype=fp8_e4m3"),
                         ({"P_": 48}, -2, "page_size=48"), ({"max_new": 41}, -1, "max_seqlen_new=41 exceeds the token count 40"),
                         ({"nrs": 568}, -1, "bad new key/value strides"), ({"nrs": 580}, -1, "bad new key/value strides"),
                         ({"krs": 640}, -1, "bad page strides"), ({"krs": 664, "kps": 16 * 664}, -1, "bad page strides"),
                         ({"kps": 16 * 656 + 8}, -1, "bad page strides"), ({"bts": 7}, -1, "block_table_stride=7 < max_pages_per_seq=8"),
                         ({"kv": ODD}, -1, "tensors must be 16-byte aligned"), ({"new": ODD}, -1, "tensors must be 16-byte aligned"),
                         ({"cu": P(0x2002)}, -1, "cu_seqlens_new must be int32-aligned"), ({"sl": P(0x2002)}, -1, "int32-aligned"),
                         ({"P_": 256, "mp": (1 << 22) + 1, "bts": 1 << 23, "kps": 256 * 656}, -1, "capacity above 2^30 keys")):
        assert append_call(lib, **kw) == st and last(lib).startswith(APPEND + ": ") and text in last(lib), (kw, last(lib))

