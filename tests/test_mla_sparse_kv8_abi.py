"""CPU: the C-ABI of fa_fwd_mla_decode_sparse_kv8 (include/fa_mi355.h, "Multi-head latent attention (decode, sparse, e4m3 pool)") -- the
three symbols against the header's argument lists, the support table (one dtype pair, every head count 1..128, every page size; the two
existing tables unmoved), every argument rule with its status and its text (fake aligned pointers: nothing may launch), each of
fa_fwd_mla_decode_sparse's bad arguments refused by both calls with the same text after the function name, the 16-element stride rule of
e4m3 pools on its own for the page stride and for the row stride, the workspace size -- the sparse call's on a grid of inputs -- and the
Python wrapper's routing and errors."""
import pytest

from test_mla_abi import BF16, F16, F32, FP8, INT_OK, INT_ODD, ODD, OK, P, fa, header_args, lib  # noqa: F401  (fa, lib: fixtures)
from test_mla_sparse_abi import SHARED, sparse_call

KV8, SPARSE, DENSE8 = "fa_fwd_mla_decode_sparse_kv8", "fa_fwd_mla_decode_sparse", "fa_fwd_mla_decode_paged_kv8"
IST = 16 * 514  # floats of one 16-row slot of the workspace


def kv8_call(lib, q=OK, kv=OK, o=OK, idx=OK, cnt=INT_OK, ws=OK, T=2, Hq=16, Dqk=576, Dv=512, topk=320, P_=64, num_pages=100, scale=0.0722,
             qs=None, os_=None, kps=64 * 576, krs=576, ist=320, q_dtype=BF16, kv_dtype=FP8, wsb=None):
    """sparse_call's arguments (tests/test_mla_sparse_abi.py) into the e4m3 entry point"""
    qs = (Hq * 576, 576) if qs is None else qs
    os_ = (Hq * 512, 512) if os_ is None else os_
    if wsb is None:
        wsb = lib.fa_fwd_mla_decode_sparse_kv8_workspace_bytes(2, 16, 512, 320)
    return lib.fa_fwd_mla_decode_sparse_kv8(q, kv, o, None, idx, cnt, T, Hq, Dqk, Dv, topk, P_, num_pages, scale, *qs, *os_, kps, krs, ist,
                                            q_dtype, kv_dtype, ws, wsb, None)


def test_three_symbols_match_the_headers_argument_lists(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((KV8, 26), (KV8 + "_workspace_bytes", 4), (KV8 + "_supported", 6)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds), name
        assert hasattr(lib, name)
    # the sparse call's list with `int dtype` replaced by `int q_dtype, int kv_dtype`
    s, k = header_args(SPARSE)[1], header_args(KV8)[1]
    assert k[:21] == s[:21] and k[21] == k[22] == s[21] and k[23:] == s[22:]
    assert header_args(KV8 + "_workspace_bytes") == header_args(SPARSE + "_workspace_bytes")
    assert lib.fa_version() == 400


def test_support_table(lib):
    sup = lib.fa_fwd_mla_decode_sparse_kv8_supported
    for hq in range(1, 129):
        for p in (16, 32, 64, 128, 256):
            assert sup(BF16, FP8, 576, 512, hq, p) == 1, (hq, p)
    for pair in ((F16, FP8), (FP8, FP8), (BF16, BF16), (F16, F16), (F32, FP8), (BF16, F16), (FP8, BF16), (9, FP8), (BF16, 9)):
        assert not sup(*pair, 576, 512, 16, 64), pair
    assert not sup(BF16, FP8, 576, 512, 0, 64) and not sup(BF16, FP8, 576, 512, 129, 64) and not sup(BF16, FP8, 576, 512, -1, 64)
    assert not sup(BF16, FP8, 192, 128, 16, 64) and not sup(BF16, FP8, 576, 576, 16, 64) and not sup(BF16, FP8, 512, 512, 16, 64)
    for p in (0, 8, 48, 512):
        assert not sup(BF16, FP8, 576, 512, 64, p)
    # the two existing tables have not moved: the sparse call still has no e4m3, the dense e4m3 call is where it was
    old, dense = lib.fa_fwd_mla_decode_sparse_supported, lib.fa_fwd_mla_decode_paged_kv8_supported
    assert not old(FP8, 576, 512, 16, 64) and old(BF16, 576, 512, 128, 64) == 1 and old(F16, 576, 512, 33, 16) == 1
    assert not old(BF16, 576, 512, 129, 64)
    assert dense(BF16, FP8, 576, 512, 16, 8, 64) == 1 and not dense(BF16, FP8, 576, 512, 16, 9, 64) and not dense(F16, FP8, 576, 512, 16, 1, 64)
    # and the sparse call keeps refusing such a pool, in its own words
    assert sparse_call(lib, dtype=FP8) == -2
    assert lib.fa_last_error().decode().startswith(SPARSE + ": needs f16 / bf16 (q and the pool alike)") and "dtype=fp8_e4m3" in lib.fa_last_error().decode()


def test_the_dtype_pair_and_the_shape_are_refused_with_what_was_given(lib):
    for kw, word in (({"q_dtype": F16}, "q=f16 kv=fp8_e4m3"), ({"q_dtype": FP8}, "q=fp8_e4m3 kv=fp8_e4m3"), ({"kv_dtype": BF16}, "q=bf16 kv=bf16"),
                     ({"q_dtype": F32}, "q=f32"), ({"Dqk": 512}, "Dqk=512"), ({"Dv": 576}, "Dv=576"), ({"P_": 48}, "page_size=48"),
                     ({"Hq": 129}, "Hq=129")):
        assert kv8_call(lib, **kw) == -2, kw
        msg = lib.fa_last_error().decode()
        assert msg.startswith(KV8 + ": needs bf16 queries on an e4m3 pool, (Dqk, Dv) = (576, 512), Hq <= 128 heads") and word in msg, (kw, msg)


def test_every_bad_argument_of_the_sparse_call_gives_both_calls_the_same_text(lib):
    own = [({"idx": None}, "null pointer"), ({"topk": 0}, "sizes must be >= 1"),
           ({"ist": 316}, "indices_stride=316 must be a multiple of 4 and >= topk=320"),
           ({"ist": 322}, "indices_stride=322 must be a multiple of 4 and >= topk=320"),
           ({"topk": 1, "ist": 0}, "indices_stride=0 must be a multiple of 4"),
           ({"idx": ODD}, "indices must be 16-byte aligned"), ({"idx": P(0x2004)}, "indices must be 16-byte aligned"),
           ({"cnt": INT_ODD}, "index_counts must be int32-aligned"),
           ({"num_pages": (1 << 24) + 1}, "num_pages * page_size = 1073741888 slots, above 2^30"),
           ({"P_": 16, "kps": 16 * 576, "num_pages": (1 << 26) + 1}, "num_pages * page_size = 1073741840 slots, above 2^30"),
           ({"topk": (1 << 30) + 1, "ist": (1 << 30) + 4, "wsb": 1 << 60}, "capacity above 2^30 keys"),
           ({"T": 1 << 23, "wsb": 1 << 60}, "grid too large"),
           ({"P_": 256, "krs": 1 << 23, "kps": 1 << 31}, "one page of one head exceeds 2 GiB")]
    # (SHARED's 2 GiB case is 2 GiB of bf16 and 1 GiB of e4m3: legal here, see the next test; the one above is too large for both)
    shared = [r for r in SHARED if "2 GiB" not in r[1]]
    assert len(shared) == len(SHARED) - 1
    for kw, word in shared + own:
        assert kv8_call(lib, **kw) == -1, kw
        mine = lib.fa_last_error().decode()
        assert sparse_call(lib, **kw) == -1, kw
        theirs = lib.fa_last_error().decode()
        assert mine.startswith(KV8 + ": ") and theirs.startswith(SPARSE + ": ") and word in mine, (kw, mine, theirs)
        assert mine.split(": ", 1)[1] == theirs.split(": ", 1)[1], (kw, mine, theirs)


def test_rules_of_its_own_each_refused_on_its_own(lib):
    def passes(**kw):  # as far as the workspace rule, the last one in front of the launch, under the sizer's own name
        assert kv8_call(lib, wsb=1, **kw) == -1, kw
        assert lib.fa_last_error().decode().startswith(KV8 + ": workspace of 1 bytes, " + KV8 + "_workspace_bytes() asks for "), kw

    passes()
    passes(cnt=None)
    passes(topk=1, ist=4)
    passes(ist=324)
    passes(topk=317)
    passes(cnt=P(0x2004))
    passes(num_pages=1 << 24)
    for hq in (1, 17, 33, 64, 65, 128):
        passes(Hq=hq)
    for p in (16, 32, 128, 256):
        passes(P_=p, kps=p * 576)
    # the 16-element stride rule of e4m3 pools, each stride on its own: a multiple of 8 that the sparse call takes and this one refuses
    for kw in ({"kps": 64 * 576 + 8}, {"krs": 584, "kps": 64 * 592}):
        assert sparse_call(lib, wsb=1, **kw) == -1 and "workspace of 1 bytes" in lib.fa_last_error().decode(), kw  # (its next rule)
        assert kv8_call(lib, **kw) == -1 and lib.fa_last_error().decode() == KV8 + ": bad page strides", kw
    passes(krs=592, kps=64 * 592)  # 16 | 592
    passes(kps=64 * 576 + 16)
    assert kv8_call(lib, krs=560) == -1 and lib.fa_last_error().decode() == KV8 + ": bad page strides"  # a row holds 576 bytes
    # one page below 2 GiB counted in bytes of 1: 256 rows of 2^22 elements are 1 GiB here (legal) and 2 GiB in the sparse call
    passes(P_=256, krs=1 << 22, kps=1 << 30)
    assert sparse_call(lib, P_=256, krs=1 << 22, kps=1 << 30) == -1 and lib.fa_last_error().decode() == SPARSE + ": one page of one head exceeds 2 GiB"
    assert kv8_call(lib, P_=256, krs=1 << 23, kps=1 << 31) == -1 and lib.fa_last_error().decode() == KV8 + ": one page of one head exceeds 2 GiB"
    # the same statuses and texts as the dense e4m3 call's pool rules
    from test_mla_kv8_abi import kv8_call as dense_call

    for kw in ({"kps": 64 * 576 + 8}, {"krs": 584, "kps": 64 * 592}, {"P_": 256, "krs": 1 << 23, "kps": 1 << 31}, {"kv": ODD}):
        assert kv8_call(lib, **kw) == -1
        mine = lib.fa_last_error().decode()
        assert dense_call(lib, **kw) == -1
        assert mine.split(": ", 1)[1] == lib.fa_last_error().decode().split(": ", 1)[1], kw


def test_workspace_size_is_the_sparse_calls_and_a_workspace_one_byte_short(lib):
    size, sparse = lib.fa_fwd_mla_decode_sparse_kv8_workspace_bytes, lib.fa_fwd_mla_decode_sparse_workspace_bytes
    for T in (1, 2, 3, 8, 16, 100, 128, 1024, 5000):
        for Hq in (1, 16, 17, 32, 33, 64, 65, 128):
            for topk in (1, 63, 64, 65, 320, 2047, 2048, 2049, 16384, 1 << 20):
                assert size(T, Hq, 512, topk) == sparse(T, Hq, 512, topk) > 0, (T, Hq, topk)
    assert size(1, 16, 512, 2048) == 8 * IST * 4 and size(2, 128, 512, 2048) == 2 * 8 * 8 * IST * 4
    need = size(2, 16, 512, 320)
    assert need == 2 * 1 * 1 * IST * 4  # five tiles: S = 1
    assert kv8_call(lib, wsb=need - 1) == -1
    assert lib.fa_last_error().decode() == f"{KV8}: workspace of {need - 1} bytes, {KV8}_workspace_bytes() asks for {need}"
    for bad in ((0, 16, 512, 320), (2, 0, 512, 320), (2, 129, 512, 320), (2, 16, 576, 320), (2, 16, 512, 0), (2, 16, 512, -5), (-1, 16, 512, 320),
                (2, 16, 512, (1 << 30) + 1), (2, 16, 512, (1 << 31) - 1)):
        assert size(*bad) == 0 == sparse(*bad), bad
    assert size(2, 16, 512, 1 << 30) > 0


def test_python_wrapper_routing_and_errors(fa):
    import torch

    pool = torch.zeros(4, 64, 576, dtype=torch.uint8).view(torch.float8_e4m3fn)
    q, idx = torch.zeros(2, 16, 576, dtype=torch.bfloat16), torch.zeros(2, 64, dtype=torch.int32)
    # the route reaches the device check: there is no CPU path behind it
    with pytest.raises(ValueError, match="no CPU path"):
        fa.flash_attention_mla_decode_sparse(q, pool, idx, 0.07)
    with pytest.raises(ValueError, match="no CPU path"):
        fa.flash_attention_mla_decode_sparse(q, pool[:, :, None], idx, 0.07, index_counts=torch.zeros(2, dtype=torch.int32))
    for dt in (torch.float16, torch.float32):  # before the library is called: no device, no library error
        with pytest.raises(ValueError, match="takes bf16 queries only"):
            fa.flash_attention_mla_decode_sparse(q.to(dt), pool, idx, 0.07)
    with pytest.raises(ValueError, match="needs the model's scale"):
        fa.flash_attention_mla_decode_sparse(q, pool, idx, None)
    with pytest.raises(ValueError, match="latent pool"):
        fa.flash_attention_mla_decode_sparse(q[0], pool, idx, 0.07)
    # the existing routes are where they were: a bf16 pool under f16 q is still the mixed-dtype error's business, behind the device check
    with pytest.raises(ValueError, match="no CPU path"):
        fa.flash_attention_mla_decode_sparse(q.to(torch.float16), torch.zeros(4, 64, 576, dtype=torch.bfloat16), idx, 0.07)
    assert fa.mla_decode_sparse_kv8_supported("bf16", "fp8_e4m3", 576, 512, 128, 64)
    assert not fa.mla_decode_sparse_kv8_supported("f16", "fp8_e4m3", 576, 512, 16, 64)
    assert not fa.mla_decode_sparse_kv8_supported("bf16", "bf16", 576, 512, 16, 64)
    assert not fa.mla_decode_sparse_kv8_supported("bf16", "fp8_e4m3", 576, 512, 129, 64)
    assert not fa.mla_decode_sparse_supported("fp8_e4m3", 576, 512, 16, 64)
    assert fa.mla_decode_sparse_kv8_workspace_bytes(1, 16, 512, 2048) == 8 * IST * 4 == fa.mla_decode_sparse_workspace_bytes(1, 16, 512, 2048)
    assert fa.mla_decode_sparse_kv8_workspace_bytes(2, 129, 512, 320) == 0
    assert "fa_fwd_mla_decode_sparse_kv8" in fa.flash_attention_mla_decode_sparse.__doc__
