"""CPU: the C-ABI of fa_fwd_mla_decode_sparse (include/fa_mi355.h, "Multi-head latent attention (decode, sparse)") -- the three symbols
against the header's argument lists, the support table, every argument rule with its status and its text (fake aligned pointers: nothing
may launch), the rules it shares with fa_fwd_mla_decode_paged_wide textually identical after the function name on the same bad argument,
each rule of its own refused on its own with one value inside and one outside, the workspace size against the wide call's -- and the
Python wrapper's errors."""
import pytest

from test_mla_abi import BF16, F16, F32, FP8, INT_OK, INT_ODD, ODD, OK, P, fa, header_args, lib  # noqa: F401  (fa, lib: fixtures)

SPARSE, WIDE = "fa_fwd_mla_decode_sparse", "fa_fwd_mla_decode_paged_wide"
IST = 16 * 514  # floats of one 16-row slot of the workspace


def sparse_call(lib, q=OK, kv=OK, o=OK, idx=OK, cnt=INT_OK, ws=OK, T=2, Hq=16, Dqk=576, Dv=512, topk=320, P_=64, num_pages=100, scale=0.0722,
                qs=None, os_=None, kps=64 * 576, krs=576, ist=320, dtype=BF16, wsb=None):
    qs = (Hq * 576, 576) if qs is None else qs
    os_ = (Hq * 512, 512) if os_ is None else os_
    if wsb is None:
        wsb = lib.fa_fwd_mla_decode_sparse_workspace_bytes(2, 16, 512, 320)
    return lib.fa_fwd_mla_decode_sparse(q, kv, o, None, idx, cnt, T, Hq, Dqk, Dv, topk, P_, num_pages, scale, *qs, *os_, kps, krs, ist, dtype, ws,
                                        wsb, None)


def wide_twin_call(lib, q=OK, kv=OK, o=OK, ws=OK, T=2, Hq=16, Dqk=576, Dv=512, P_=64, num_pages=100, scale=0.0722, qs=None, os_=None,
                   kps=64 * 576, krs=576, dtype=BF16, wsb=None, **_):
    """the same arguments as the wide call sees them: B = T, Nq = 1, a row stride of one row, a table of five pages"""
    qs = (Hq * 576, 576) if qs is None else qs
    os_ = (Hq * 512, 512) if os_ is None else os_
    if wsb is None:
        wsb = lib.fa_fwd_mla_decode_paged_wide_workspace_bytes(2, 16, 1, 512, 64, 5)
    return lib.fa_fwd_mla_decode_paged_wide(q, kv, o, None, INT_OK, INT_OK, T, Hq, 1, Dqk, Dv, P_, num_pages, 5, scale, *qs, 576, *os_, 512, kps, krs,
                                            8, 0, dtype, ws, wsb, None)


def test_three_symbols_match_the_headers_argument_lists(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((SPARSE, 25), (SPARSE + "_workspace_bytes", 4), (SPARSE + "_supported", 5)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds), name
        assert hasattr(lib, name)
    assert lib.fa_version() == 400


def test_support_table(lib):
    sup = lib.fa_fwd_mla_decode_sparse_supported
    for dtype in (F16, BF16):
        for hq in (1, 16, 17, 32, 33, 64, 65, 128):
            for p in (16, 32, 64, 128, 256):
                assert sup(dtype, 576, 512, hq, p) == 1, (dtype, hq, p)
    assert not sup(BF16, 576, 512, 0, 64) and not sup(BF16, 576, 512, 129, 64) and not sup(BF16, 576, 512, -1, 64)
    assert not sup(BF16, 192, 128, 16, 64) and not sup(BF16, 576, 576, 16, 64) and not sup(BF16, 512, 512, 16, 64)
    assert not sup(F32, 576, 512, 16, 64) and not sup(FP8, 576, 512, 16, 64) and not sup(9, 576, 512, 16, 64)
    for p in (0, 8, 48, 512):
        assert not sup(BF16, 576, 512, 64, p)
    # the refusal names what was given
    for kw, word in (({"Hq": 129}, "Hq=129"), ({"Dqk": 512}, "Dqk=512"), ({"Dv": 576}, "Dv=576"), ({"dtype": F32}, "dtype=f32"),
                     ({"dtype": FP8}, "dtype=fp8_e4m3"), ({"P_": 48}, "page_size=48")):
        assert sparse_call(lib, **kw) == -2, kw
        msg = lib.fa_last_error().decode()
        assert msg.startswith(SPARSE + ": needs f16 / bf16 (q and the pool alike), (Dqk, Dv) = (576, 512), Hq <= 128 heads") and word in msg, msg


SHARED = [({"q": None}, "null pointer"), ({"kv": None}, "null pointer"), ({"o": None}, "null pointer"), ({"ws": None}, "null pointer"),
          ({"T": 0}, "sizes must be >= 1"), ({"Hq": 0}, "sizes must be >= 1"), ({"num_pages": 0}, "sizes must be >= 1"),
          ({"scale": 0.0}, "scale"), ({"scale": float("nan")}, "scale"),
          ({"qs": (16 * 576, 568)}, "bad strides"), ({"qs": (-576, 576)}, "bad strides"), ({"qs": (16 * 576 + 4, 576)}, "bad strides"),
          ({"qs": (512, 576)}, "bad strides"),
          ({"os_": (16 * 512, 504)}, "bad output strides"), ({"os_": (16 * 512 + 2, 512)}, "bad output strides"),
          ({"krs": 8}, "bad page strides"), ({"krs": 512}, "bad page strides"), ({"kps": 64 * 576 + 4}, "bad page strides"),
          ({"P_": 256, "krs": 1 << 22, "kps": 1 << 30}, "one page of one head exceeds 2 GiB"),
          ({"q": ODD}, "tensors and workspace must be 16-byte aligned"), ({"kv": ODD}, "16-byte aligned"), ({"o": ODD}, "16-byte aligned"),
          ({"ws": ODD}, "16-byte aligned"),
          ({"T": 1 << 23, "wsb": 1 << 60}, "grid too large")]


def test_rules_shared_with_the_wide_call_have_its_status_and_text(lib):
    for kw, word in SHARED:
        assert sparse_call(lib, **kw) == -1, kw
        mine = lib.fa_last_error().decode()
        assert wide_twin_call(lib, **kw) == -1, kw
        theirs = lib.fa_last_error().decode()
        assert mine.startswith(SPARSE + ": ") and theirs.startswith(WIDE + ": ") and word in mine, (kw, mine, theirs)
        assert mine.split(": ", 1)[1] == theirs.split(": ", 1)[1], (kw, mine, theirs)
    # the token stride is free when T = 1, as the wide call's batch stride is when B = 1
    one = {"T": 1, "qs": (8, 576), "os_": (0, 512), "wsb": 1}
    assert sparse_call(lib, **one) == -1 and "workspace of 1 bytes" in lib.fa_last_error().decode()
    assert wide_twin_call(lib, **one) == -1 and "workspace of 1 bytes" in lib.fa_last_error().decode()


def test_rules_of_its_own_each_refused_on_its_own(lib):
    def refused(word, **kw):
        assert sparse_call(lib, **kw) == -1, kw
        msg = lib.fa_last_error().decode()
        assert msg.startswith(SPARSE + ": ") and word in msg, (kw, msg)

    def passes(**kw):  # as far as the workspace rule, the last one in front of the launch
        assert sparse_call(lib, wsb=1, **kw) == -1, kw
        assert lib.fa_last_error().decode().startswith(SPARSE + ": workspace of 1 bytes, " + SPARSE + "_workspace_bytes() asks for "), kw

    passes()
    refused("null pointer", idx=None)
    passes(cnt=None)  # no counts: every list holds topk entries
    refused("sizes must be >= 1", topk=0)
    passes(topk=1, ist=4)
    refused("indices_stride=316 must be a multiple of 4 and >= topk=320", ist=316)
    refused("indices_stride=322 must be a multiple of 4 and >= topk=320", ist=322)
    refused("indices_stride=0 must be a multiple of 4", topk=1, ist=0)
    passes(ist=324)
    passes(topk=317)
    refused("indices must be 16-byte aligned", idx=ODD)
    refused("indices must be 16-byte aligned", idx=P(0x2004))
    refused("index_counts must be int32-aligned", cnt=INT_ODD)
    passes(cnt=P(0x2004))
    refused("num_pages * page_size = 1073741888 slots, above 2^30", num_pages=(1 << 24) + 1)
    passes(num_pages=1 << 24)
    refused("num_pages * page_size = 1073741840 slots, above 2^30", P_=16, kps=16 * 576, num_pages=(1 << 26) + 1)
    refused("capacity above 2^30 keys", topk=(1 << 30) + 1, ist=(1 << 30) + 4, wsb=1 << 60)
    assert sparse_call(lib, topk=1 << 30, ist=1 << 30, wsb=1) == -1 and "workspace of 1 bytes" in lib.fa_last_error().decode()
    refused("grid too large", T=1 << 23, wsb=1 << 60)
    assert sparse_call(lib, T=(1 << 23) - 1, wsb=1) == -1 and "workspace of 1 bytes" in lib.fa_last_error().decode()


def test_workspace_size_is_the_wide_calls_and_a_workspace_one_byte_short(lib):
    size, wide = lib.fa_fwd_mla_decode_sparse_workspace_bytes, lib.fa_fwd_mla_decode_paged_wide_workspace_bytes
    for T in (1, 2, 3, 8, 16, 100, 128, 1024, 5000):
        for Hq in (1, 16, 17, 32, 33, 64, 65, 128):
            for topk in (1, 63, 64, 65, 320, 2047, 2048, 2049, 16384, 1 << 20):
                assert size(T, Hq, 512, topk) == wide(T, Hq, 1, 512, 64, -(-topk // 64)) > 0, (T, Hq, topk)
    assert size(1, 16, 512, 2048) == 8 * IST * 4 and size(2, 128, 512, 2048) == 2 * 8 * 8 * IST * 4
    assert size(1, 64, 512, 65536) == 256 * 4 * IST * 4  # one token, one block of 64 heads, 1024 tiles: S = 256
    need = size(2, 16, 512, 320)
    assert need == 2 * 1 * 1 * IST * 4  # five tiles: S = 1
    assert sparse_call(lib, wsb=need - 1) == -1
    assert lib.fa_last_error().decode() == f"{SPARSE}: workspace of {need - 1} bytes, {SPARSE}_workspace_bytes() asks for {need}"
    for bad in ((0, 16, 512, 320), (2, 0, 512, 320), (2, 129, 512, 320), (2, 16, 576, 320), (2, 16, 512, 0), (2, 16, 512, -5), (-1, 16, 512, 320),
                (2, 16, 512, (1 << 30) + 1), (2, 16, 512, (1 << 31) - 1)):
        assert size(*bad) == 0, bad
    assert size(2, 16, 512, 1 << 30) > 0


def test_python_wrapper_errors(fa):
    import torch

    pool = torch.zeros(4, 64, 576, dtype=torch.bfloat16)
    q, idx = torch.zeros(2, 16, 576, dtype=torch.bfloat16), torch.zeros(2, 64, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU path"):
        fa.flash_attention_mla_decode_sparse(q, pool, idx, 0.07)
    with pytest.raises(ValueError, match="no CPU path"):
        fa.flash_attention_mla_decode_sparse(q, pool, idx, 0.07, index_counts=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="scale"):
        fa.flash_attention_mla_decode_sparse(q, pool, idx, None)
    with pytest.raises(ValueError, match="latent pool"):
        fa.flash_attention_mla_decode_sparse(q[0], pool, idx, 0.07)
    with pytest.raises(ValueError, match="latent pool"):
        fa.flash_attention_mla_decode_sparse(q[:, None], pool, idx, 0.07)
    assert fa.mla_decode_sparse_supported("bf16", 576, 512, 128, 64) and not fa.mla_decode_sparse_supported("bf16", 576, 512, 129, 64)
    assert fa.mla_decode_sparse_supported("f16", 576, 512, 33, 16) and not fa.mla_decode_sparse_supported("f16", 576, 512, 33, 48)
    assert fa.mla_decode_sparse_workspace_bytes(1, 16, 512, 2048) == 8 * IST * 4 and fa.mla_decode_sparse_workspace_bytes(2, 129, 512, 320) == 0
    assert fa.mla_decode_sparse_workspace_bytes(2, 128, 512, 2048) == fa.mla_decode_paged_wide_workspace_bytes(2, 128, 1, 512, 64, 32)
    assert "SLOT" in fa.flash_attention_mla_decode_sparse.__doc__
