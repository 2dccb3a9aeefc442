"""CPU: the C-ABI of fa_fwd_mla_decode_paged_wide (include/fa_mi355.h, "Multi-head latent attention (decode, wide)") -- the three symbols
against the header's argument lists, the support table (and the one-wave call's, which must not have moved), every argument rule with
its status and its text (fake aligned pointers: nothing may launch), the rules it shares with fa_fwd_mla_decode_paged textually
identical after the function name, the workspace size -- and the Python wrapper's errors and its `wide=` routing."""
import pytest

from test_mla_abi import BF16, F16, F32, FP8, INT_OK, ODD, OK, SHARED, fa, header_args, lib, mla_call  # noqa: F401  (fa, lib: fixtures)

WIDE, OLD = "fa_fwd_mla_decode_paged_wide", "fa_fwd_mla_decode_paged"
IST = 16 * 514  # floats of one 16-row slot of the workspace


def wide_call(lib, q=OK, kv=OK, o=OK, bt=INT_OK, sl=INT_OK, ws=OK, B=2, Hq=16, Nq=2, Dqk=576, Dv=512, P_=64, num_pages=100, max_pages=8,
              scale=0.0722, qs=None, os_=None, kps=64 * 576, krs=576, bts=8, causal=1, dtype=BF16, wsb=None):
    """mla_call's arguments (tests/test_mla_abi.py) into the wide entry point"""
    qs = (Hq * Nq * 576, Nq * 576, 576) if qs is None else qs
    os_ = (Hq * Nq * 512, Nq * 512, 512) if os_ is None else os_
    if wsb is None:
        wsb = lib.fa_fwd_mla_decode_paged_wide_workspace_bytes(2, 16, 2, 512, 64, 8)
    return lib.fa_fwd_mla_decode_paged_wide(q, kv, o, None, bt, sl, B, Hq, Nq, Dqk, Dv, P_, num_pages, max_pages, scale, *qs, *os_, kps, krs, bts,
                                            causal, dtype, ws, wsb, None)


def test_three_symbols_match_the_headers_argument_lists(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in ((WIDE, 29), (WIDE + "_workspace_bytes", 6), (WIDE + "_supported", 6)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds), name
        assert hasattr(lib, name)
    assert header_args(WIDE) == header_args(OLD)  # the argument list is the one-wave call's
    assert lib.fa_version() == 400


def test_support_table(lib):
    sup, old = lib.fa_fwd_mla_decode_paged_wide_supported, lib.fa_fwd_mla_decode_paged_supported
    for dtype in (F16, BF16):
        for (hq, nq) in ((1, 1), (16, 1), (17, 1), (32, 1), (16, 2), (33, 1), (16, 3), (5, 7), (16, 8), (128, 1), (1, 128)):
            for p in (16, 32, 64, 128, 256):
                assert sup(dtype, 576, 512, hq, nq, p) == 1, (dtype, hq, nq, p)
    assert not sup(BF16, 576, 512, 0, 1, 64) and not sup(BF16, 576, 512, 16, 0, 64) and not sup(BF16, 576, 512, 129, 1, 64)
    assert not sup(BF16, 576, 512, 16, 9, 64) and not sup(BF16, 192, 128, 16, 1, 64) and not sup(BF16, 576, 576, 16, 1, 64)
    assert not sup(BF16, 576, 512, 1 << 16, 1 << 16, 64)  # (a product past 2^31 is no small number of rows)
    assert not sup(F32, 576, 512, 16, 1, 64) and not sup(FP8, 576, 512, 16, 1, 64) and not sup(9, 576, 512, 16, 1, 64)
    for p in (0, 8, 48, 512):
        assert not sup(BF16, 576, 512, 64, 1, p)
    # the one-wave call's table has not moved
    assert old(BF16, 576, 512, 32, 1, 64) == 1 and not old(BF16, 576, 512, 33, 1, 64) and not old(BF16, 576, 512, 16, 3, 64)
    assert not old(BF16, 576, 512, 128, 1, 64)


def test_rules_shared_with_the_one_wave_call_have_its_status_and_text(lib):
    own = [({"qs": (32 * 576, 2 * 576, 512)}, -1, "bad strides"), ({"qs": (-576, 2 * 576, 576)}, -1, "bad strides"),
           ({"os_": (32 * 512, 2 * 512, 504)}, -1, "bad output strides"), ({"os_": (32 * 512 + 2, 2 * 512, 512)}, -1, "bad output strides"),
           ({"krs": 512}, -1, "bad page strides"), ({"o": ODD}, -1, "16-byte aligned"),
           ({"Dqk": 512}, -2, "Dqk=512"), ({"Dv": 576}, -2, "Dv=576"), ({"dtype": F32}, -2, "dtype=f32"), ({"dtype": FP8}, -2, "fp8_e4m3"),
           ({"P_": 48}, -2, "page_size=48")]
    for kw, status, word in SHARED + own:
        assert wide_call(lib, **kw) == status, kw
        mine = lib.fa_last_error().decode()
        assert mla_call(lib, **kw) == status, kw
        theirs = lib.fa_last_error().decode()
        assert mine.startswith(WIDE + ": ") and theirs.startswith(OLD + ": ") and word in mine, (kw, mine, theirs)
        # the row limit is the one figure of the text that differs (the message that states the support table)
        assert mine.split(": ", 1)[1].replace("Hq * Nq <= 128", "Hq * Nq <= 32") == theirs.split(": ", 1)[1], (kw, mine, theirs)


def test_rules_of_its_own(lib):
    for kw, word in (({"Hq": 129, "Nq": 1}, "Hq=129 Nq=1"), ({"Hq": 16, "Nq": 9}, "Hq=16 Nq=9")):
        assert wide_call(lib, **kw) == -2, kw
        msg = lib.fa_last_error().decode()
        assert msg.startswith(WIDE + ": ") and "Hq * Nq <= 128 packed query rows" in msg and word in msg, (kw, msg)
    # what the one-wave call refuses and this one takes as far as the next rule: 33 and 128 rows pass the support check
    for hq, nq in ((33, 1), (16, 3), (128, 1), (16, 8)):
        assert mla_call(lib, Hq=hq, Nq=nq) == -2 and "Hq * Nq <= 32" in lib.fa_last_error().decode()
        assert wide_call(lib, Hq=hq, Nq=nq, wsb=1) == -1
        assert lib.fa_last_error().decode().startswith(WIDE + ": workspace of 1 bytes, " + WIDE + "_workspace_bytes() asks for ")


def test_workspace_size_and_a_workspace_one_byte_short(lib):
    size, old = lib.fa_fwd_mla_decode_paged_wide_workspace_bytes, lib.fa_fwd_mla_decode_paged_workspace_bytes
    # B * S * ceil(rows / 16) slots of 16 * (512 + 2) floats; S = min(ceil(256 / (B * WB)), tiles / 4, 256), WB = ceil(rows / (16 NW))
    need = size(2, 16, 2, 512, 64, 8)
    assert need == 2 * 2 * 2 * IST * 4  # 32 rows, NW = 2: WB = 1; capacity 512 keys = 8 tiles: S = min(128, 2) = 2
    assert size(1, 64, 1, 512, 64, 1024) == 1 * 256 * 4 * IST * 4   # one sequence, one block of 64 rows, 65536 keys: S = 256
    assert size(1, 128, 1, 512, 64, 1024) == 1 * 128 * 8 * IST * 4  # two blocks: S = 128
    assert size(1, 33, 1, 512, 64, 1024) == 1 * 256 * 3 * IST * 4   # 33 rows: three 16-row slots (the fourth wave has none), one block
    assert size(128, 128, 1, 512, 16, 256) == 128 * 1 * 8 * IST * 4  # 256 (sequence, block) pairs already: S = 1
    assert size(4, 16, 1, 512, 16, 256) == 4 * 16 * 1 * IST * 4     # 4096 keys = 64 tiles: S = min(64, 16) = 16
    assert wide_call(lib, wsb=need - 1) == -1
    assert lib.fa_last_error().decode() == f"{WIDE}: workspace of {need - 1} bytes, {WIDE}_workspace_bytes() asks for {need}"
    for bad in ((0, 16, 1, 512, 64, 8), (2, 0, 1, 512, 64, 8), (2, 16, 0, 512, 64, 8), (2, 16, 9, 512, 64, 8), (2, 129, 1, 512, 64, 8),
                (2, 16, 1, 576, 64, 8), (2, 16, 1, 512, 48, 8), (2, 16, 1, 512, 64, 0), (2, 16, 1, 512, 256, (1 << 22) + 1), (-1, 16, 1, 512, 64, 8)):
        assert size(*bad) == 0, bad
    assert old(2, 16, 3, 512, 64, 8) == 0 and old(2, 16, 2, 512, 64, 8) == 2 * 2 * 2 * IST * 4  # the one-wave call's has not moved


def test_python_wrapper_errors_and_routing(fa):
    import torch

    pool = torch.zeros(4, 64, 576, dtype=torch.bfloat16)
    bt, sl = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for hq, nq in ((16, 1), (48, 1), (16, 8)):
        q = torch.zeros(2, hq, nq, 576, dtype=torch.bfloat16)
        for wide in (None, True, False):  # every route reaches the device check: there is no CPU path behind any of them
            with pytest.raises(ValueError, match="no CPU path"):
                fa.flash_attention_mla_decode_paged(q, pool, bt, sl, 0.07, wide=wide)
    q = torch.zeros(2, 48, 1, 576, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="scale"):
        fa.flash_attention_mla_decode_paged(q, pool, bt, sl, None, wide=True)
    with pytest.raises(ValueError, match="latent pool"):
        fa.flash_attention_mla_decode_paged(q[0], pool, bt, sl, 0.07, wide=True)
    assert fa.mla_decode_paged_wide_supported("bf16", 576, 512, 16, 8, 64) and not fa.mla_decode_paged_wide_supported("bf16", 576, 512, 16, 9, 64)
    assert fa.mla_decode_paged_wide_supported("f16", 576, 512, 33, 1, 16) and not fa.mla_decode_paged_supported("f16", 576, 512, 33, 1, 16)
    assert fa.mla_decode_paged_wide_workspace_bytes(1, 128, 1, 512, 64, 1024) == 128 * 8 * IST * 4
    assert fa.mla_decode_paged_wide_workspace_bytes(2, 129, 1, 512, 64, 8) == 0
    assert "up to 128" in " ".join(fa.flash_attention_mla_decode_paged.__doc__.split())
