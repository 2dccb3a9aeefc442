"""CPU: the C-ABI of fa_fwd_mla_decode_paged_kv8 (include/fa_mi355.h, "Multi-head latent attention (decode, e4m3 pool)") -- the three
symbols against the header's argument lists, the support table (one dtype pair, every row count 1..128, every page size; the two
existing MLA tables unmoved), every argument rule with its status and its text (fake aligned pointers: nothing may launch), the rules
it shares with fa_fwd_mla_decode_paged_wide textually identical after the function name, the 16-element stride rule of e4m3 pools on
its own, the workspace size -- the wide call's on a grid of inputs -- and the Python wrapper's errors and routing."""
import pytest

from test_mla_abi import BF16, F16, F32, FP8, INT_OK, ODD, OK, SHARED, fa, header_args, lib  # noqa: F401  (fa, lib: fixtures)
from test_mla_wide_abi import wide_call

KV8, WIDE = "fa_fwd_mla_decode_paged_kv8", "fa_fwd_mla_decode_paged_wide"
IST = 16 * 514  # floats of one 16-row slot of the workspace


def kv8_call(lib, q=OK, kv=OK, o=OK, bt=INT_OK, sl=INT_OK, ws=OK, B=2, Hq=16, Nq=2, Dqk=576, Dv=512, P_=64, num_pages=100, max_pages=8,
             scale=0.0722, qs=None, os_=None, kps=64 * 576, krs=576, bts=8, causal=1, q_dtype=BF16, kv_dtype=FP8, wsb=None):
    """wide_call's arguments (tests/test_mla_wide_abi.py) into the e4m3 entry point"""
    qs = (Hq * Nq * 576, Nq * 576, 576) if qs is None else qs
    os_ = (Hq * Nq * 512, Nq * 512, 512) if os_ is None else os_
    if wsb is None:
        wsb = lib.fa_fwd_mla_decode_paged_kv8_workspace_bytes(2, 16, 2, 512, 64, 8)
    return lib.fa_fwd_mla_decode_paged_kv8(q, kv, o, None, bt, sl, B, Hq, Nq, Dqk, Dv, P_, num_pages, max_pages, scale, *qs, *os_, kps, krs, bts,
                                           causal, q_dtype, kv_dtype, ws, wsb, None)


def test_three_symbols_match_the_headers_argument_lists(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((KV8, 30), (KV8 + "_workspace_bytes", 6), (KV8 + "_supported", 7)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds), name
        assert hasattr(lib, name)
    # the wide call's list with `int dtype` replaced by `int q_dtype, int kv_dtype`
    w, k = header_args(WIDE)[1], header_args(KV8)[1]
    assert k[:25] == w[:25] and k[25] == k[26] == w[25] and k[27:] == w[26:]
    assert header_args(KV8 + "_workspace_bytes") == header_args(WIDE + "_workspace_bytes")
    assert lib.fa_version() == 400


def test_support_table(lib):
    sup = lib.fa_fwd_mla_decode_paged_kv8_supported
    for rows in range(1, 129):  # every row count, as heads and as tokens
        for p in (16, 32, 64, 128, 256):
            assert sup(BF16, FP8, 576, 512, rows, 1, p) == 1 and sup(BF16, FP8, 576, 512, 1, rows, p) == 1, (rows, p)
    assert sup(BF16, FP8, 576, 512, 5, 7, 16) == 1 and sup(BF16, FP8, 576, 512, 16, 8, 256) == 1
    for pair in ((F16, FP8), (FP8, FP8), (BF16, BF16), (F16, F16), (F32, FP8), (BF16, F16), (FP8, BF16), (9, FP8), (BF16, 9)):
        assert not sup(*pair, 576, 512, 16, 1, 64), pair
    assert not sup(BF16, FP8, 576, 512, 0, 1, 64) and not sup(BF16, FP8, 576, 512, 16, 0, 64) and not sup(BF16, FP8, 576, 512, 129, 1, 64)
    assert not sup(BF16, FP8, 576, 512, 16, 9, 64) and not sup(BF16, FP8, 192, 128, 16, 1, 64) and not sup(BF16, FP8, 576, 576, 16, 1, 64)
    assert not sup(BF16, FP8, 576, 512, 1 << 16, 1 << 16, 64)
    for p in (0, 8, 48, 512):
        assert not sup(BF16, FP8, 576, 512, 64, 1, p)
    # the two existing MLA tables have not moved: e4m3 is still none of theirs
    wide, old = lib.fa_fwd_mla_decode_paged_wide_supported, lib.fa_fwd_mla_decode_paged_supported
    assert not wide(FP8, 576, 512, 16, 1, 64) and not old(FP8, 576, 512, 16, 1, 64)
    assert wide(BF16, 576, 512, 128, 1, 64) == 1 and wide(F16, 576, 512, 33, 1, 16) == 1 and not wide(BF16, 576, 512, 129, 1, 64)
    assert old(BF16, 576, 512, 32, 1, 64) == 1 and not old(BF16, 576, 512, 33, 1, 64)


def test_rules_shared_with_the_wide_call_have_its_status_and_text(lib):
    own = [({"qs": (32 * 576, 2 * 576, 512)}, -1, "bad strides"), ({"qs": (-576, 2 * 576, 576)}, -1, "bad strides"),
           ({"qs": (32 * 576, 2 * 576 + 4, 576)}, -1, "bad strides"),
           ({"os_": (32 * 512, 2 * 512, 504)}, -1, "bad output strides"), ({"os_": (32 * 512 + 2, 2 * 512, 512)}, -1, "bad output strides"),
           ({"krs": 512}, -1, "bad page strides"), ({"o": ODD}, -1, "16-byte aligned"), ({"bt": None}, -1, "null pointer"),
           ({"Hq": 0}, -1, "sizes must be >= 1"), ({"num_pages": 0}, -1, "sizes must be >= 1"), ({"scale": -1.0}, -1, "scale"),
           ({"P_": 256, "krs": 1 << 23, "kps": 1 << 31}, -1, "one page of one head exceeds 2 GiB")]
    # (SHARED's 2 GiB case is 2 GiB of bf16 and 1 GiB of e4m3: legal here, see test_rules_of_its_own; the one above is too large for both)
    shared = [r for r in SHARED if "2 GiB" not in r[2]]
    assert len(shared) == len(SHARED) - 1
    for kw, status, word in shared + own:
        assert kv8_call(lib, **kw) == status, kw
        mine = lib.fa_last_error().decode()
        assert wide_call(lib, **kw) == status, kw
        theirs = lib.fa_last_error().decode()
        assert mine.startswith(KV8 + ": ") and theirs.startswith(WIDE + ": ") and word in mine, (kw, mine, theirs)
        assert mine.split(": ", 1)[1] == theirs.split(": ", 1)[1], (kw, mine, theirs)


def test_rules_of_its_own(lib):
    # the dtype pair and the shape: FA_ERR_UNSUPPORTED with a message that names what was given
    for kw, word in (({"q_dtype": F16}, "q=f16 kv=fp8_e4m3"), ({"q_dtype": FP8}, "q=fp8_e4m3 kv=fp8_e4m3"), ({"kv_dtype": BF16}, "q=bf16 kv=bf16"),
                     ({"q_dtype": F32}, "q=f32"), ({"Dqk": 512}, "Dqk=512"), ({"Dv": 576}, "Dv=576"), ({"P_": 48}, "page_size=48"),
                     ({"Hq": 129, "Nq": 1}, "Hq=129 Nq=1"), ({"Hq": 16, "Nq": 9}, "Hq=16 Nq=9")):
        assert kv8_call(lib, **kw) == -2, kw
        msg = lib.fa_last_error().decode()
        assert msg.startswith(KV8 + ": needs bf16 queries on an e4m3 pool") and "Hq * Nq <= 128 packed query rows" in msg and word in msg, (kw, msg)
    # the 16-element stride rule of e4m3 pools, each stride on its own: a multiple of 8 that the wide call takes and this one refuses
    for kw in ({"kps": 64 * 576 + 8}, {"krs": 584, "kps": 64 * 592}):
        assert wide_call(lib, wsb=1, **kw) == -1 and "workspace of 1 bytes" in lib.fa_last_error().decode(), kw  # (its next rule)
    assert kv8_call(lib, kps=64 * 576 + 8) == -1 and lib.fa_last_error().decode() == KV8 + ": bad page strides"
    assert kv8_call(lib, krs=584, kps=64 * 592) == -1 and lib.fa_last_error().decode() == KV8 + ": bad page strides"
    assert kv8_call(lib, krs=592, kps=64 * 592, wsb=1) == -1 and "workspace of 1 bytes" in lib.fa_last_error().decode()  # (16 | 592: the next rule)
    # one page below 2 GiB counted in bytes of 1: 256 rows of 2^22 elements are 1 GiB here (legal) and 2 GiB in the wide call
    assert kv8_call(lib, P_=256, krs=1 << 22, kps=1 << 30, wsb=1) == -1 and "workspace of 1 bytes" in lib.fa_last_error().decode()
    assert kv8_call(lib, P_=256, krs=1 << 23, kps=1 << 31) == -1 and lib.fa_last_error().decode() == KV8 + ": one page of one head exceeds 2 GiB"
    # every legal row count passes the support check and reaches the workspace rule, under the sizer's own name
    for hq, nq in ((1, 1), (17, 1), (33, 1), (16, 3), (128, 1), (16, 8)):
        assert kv8_call(lib, Hq=hq, Nq=nq, wsb=1) == -1
        assert lib.fa_last_error().decode().startswith(KV8 + ": workspace of 1 bytes, " + KV8 + "_workspace_bytes() asks for ")


def test_workspace_size_is_the_wide_calls_and_a_workspace_one_byte_short(lib):
    size, wide = lib.fa_fwd_mla_decode_paged_kv8_workspace_bytes, lib.fa_fwd_mla_decode_paged_wide_workspace_bytes
    for B in (1, 2, 3, 16, 128, 300):
        for hq, nq in ((1, 1), (16, 1), (17, 1), (32, 1), (16, 2), (33, 1), (64, 1), (65, 1), (5, 13), (128, 1), (16, 8), (1, 128)):
            for p in (16, 64, 256):
                for mp in (1, 7, 64, 1024):
                    assert size(B, hq, nq, 512, p, mp) == wide(B, hq, nq, 512, p, mp) > 0, (B, hq, nq, p, mp)
    assert size(1, 64, 1, 512, 64, 1024) == 1 * 256 * 4 * IST * 4  # one sequence, one block of 64 rows, 65536 keys: S = 256
    assert size(1, 16, 1, 512, 64, 1024) == 1 * 256 * 1 * IST * 4  # 16 rows: still one (four-wave) block, the wide call's S
    need = size(2, 16, 2, 512, 64, 8)
    assert need == 2 * 2 * 2 * IST * 4
    assert kv8_call(lib, wsb=need - 1) == -1
    assert lib.fa_last_error().decode() == f"{KV8}: workspace of {need - 1} bytes, {KV8}_workspace_bytes() asks for {need}"
    for bad in ((0, 16, 1, 512, 64, 8), (2, 0, 1, 512, 64, 8), (2, 16, 0, 512, 64, 8), (2, 16, 9, 512, 64, 8), (2, 129, 1, 512, 64, 8),
                (2, 16, 1, 576, 64, 8), (2, 16, 1, 512, 48, 8), (2, 16, 1, 512, 64, 0), (2, 16, 1, 512, 256, (1 << 22) + 1), (-1, 16, 1, 512, 64, 8)):
        assert size(*bad) == 0 == wide(*bad), bad


def test_python_wrapper_errors_and_routing(fa):
    import torch

    pool = torch.zeros(4, 64, 576, dtype=torch.uint8).view(torch.float8_e4m3fn)
    bt, sl = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for hq, nq in ((16, 1), (48, 1), (16, 8)):
        q = torch.zeros(2, hq, nq, 576, dtype=torch.bfloat16)
        for wide in (None, True):  # the route reaches the device check: there is no CPU path behind it
            with pytest.raises(ValueError, match="no CPU path"):
                fa.flash_attention_mla_decode_paged(q, pool, bt, sl, 0.07, wide=wide)
        with pytest.raises(ValueError, match="wide=False on a float8_e4m3fn latent pool"):
            fa.flash_attention_mla_decode_paged(q, pool, bt, sl, 0.07, wide=False)
        for dt in (torch.float16, torch.float32):  # before the library is called: no device, no library error
            with pytest.raises(ValueError, match="takes bf16 queries only"):
                fa.flash_attention_mla_decode_paged(q.to(dt), pool, bt, sl, 0.07)
    # the existing routes are where they were: a bf16 pool under f16 q is still the mixed-dtype error's business, behind the device check
    with pytest.raises(ValueError, match="no CPU path"):
        fa.flash_attention_mla_decode_paged(q.to(torch.float16), torch.zeros(4, 64, 576, dtype=torch.bfloat16), bt, sl, 0.07)
    assert fa.mla_decode_paged_kv8_supported("bf16", "fp8_e4m3", 576, 512, 16, 8, 64)
    assert not fa.mla_decode_paged_kv8_supported("f16", "fp8_e4m3", 576, 512, 16, 8, 64)
    assert not fa.mla_decode_paged_kv8_supported("bf16", "bf16", 576, 512, 16, 8, 64)
    assert not fa.mla_decode_paged_kv8_supported("bf16", "fp8_e4m3", 576, 512, 16, 9, 64)
    assert fa.mla_decode_paged_kv8_workspace_bytes(1, 128, 1, 512, 64, 1024) == 128 * 8 * IST * 4 == fa.mla_decode_paged_wide_workspace_bytes(1, 128, 1, 512, 64, 1024)
    assert fa.mla_decode_paged_kv8_workspace_bytes(2, 129, 1, 512, 64, 8) == 0
    assert "fa_fwd_mla_decode_paged_kv8" in fa.flash_attention_mla_decode_paged.__doc__
    # kv_append_paged takes the aliased latent call as far as the device check: Hkv = 1, D = 576, one pool twice, 16-bit rows
    p4 = pool.view(4, 64, 1, 576)
    new = torch.zeros(3, 1, 576, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa.kv_append_paged(new, new, p4, p4, torch.tensor([0, 1, 3], dtype=torch.int32), bt, sl, 2, layout="NHD", k_mul=0.5, v_mul=0.5)
