"""CPU: the C-ABI of fa_fwd_mla_decode_paged (include/fa_mi355.h, "Multi-head latent attention (decode)") -- the three symbols against
the header's argument lists, the support table, every argument rule with its status and its text (fake aligned pointers: nothing may
launch), the rules it shares with fa_fwd_decode_paged textually identical after the function name, the workspace size -- and the
ValueErrors of the Python wrapper."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p
OK, ODD = P(0x1000), P(0x1008)  # 16-byte aligned / 8-byte aligned only
INT_OK, INT_ODD = P(0x2000), P(0x2002)
F16, BF16, F32, FP8 = 1, 2, 0, 3


@pytest.fixture(scope="module")
def fa():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    return fa


@pytest.fixture(scope="module")
def lib(fa):
    return fa.load_library()


def header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fa_mi355.h")).read(), flags=re.S)
    res, args = re.search(r"([a-z ]+?)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", src).groups()
    kinds = []
    for a in args.split(","):
        a = a.strip()
        kinds.append(ctypes.c_void_p if "*" in a else {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}[a.rsplit(" ", 1)[0]])
    return {"int": ctypes.c_int, "long long": ctypes.c_longlong}[res.strip()], kinds


def test_three_symbols_match_the_headers_argument_lists(lib):
    from flash_attention_metal_amd._lib import SYMBOLS

    for name, nargs in (("fa_fwd_mla_decode_paged", 29), ("fa_fwd_mla_decode_paged_workspace_bytes", 6), ("fa_fwd_mla_decode_paged_supported", 6)):
        res, kinds = header_args(name)
        assert len(kinds) == nargs and SYMBOLS[name] == (res, kinds), name
        assert hasattr(lib, name)
    assert lib.fa_version() == 400


def test_support_table(lib):
    sup = lib.fa_fwd_mla_decode_paged_supported
    for dtype in (F16, BF16):
        for (hq, nq) in ((16, 1), (16, 2), (8, 4), (5, 3), (32, 1), (1, 32), (1, 1)):
            for p in (16, 32, 64, 128, 256):
                assert sup(dtype, 576, 512, hq, nq, p) == 1
    assert not sup(F32, 576, 512, 16, 1, 64) and not sup(FP8, 576, 512, 16, 1, 64) and not sup(9, 576, 512, 16, 1, 64)
    assert not sup(BF16, 512, 512, 16, 1, 64) and not sup(BF16, 576, 576, 16, 1, 64) and not sup(BF16, 192, 128, 16, 1, 64)
    assert not sup(BF16, 576, 512, 33, 1, 64) and not sup(BF16, 576, 512, 16, 3, 64) and not sup(BF16, 576, 512, 128, 1, 64)
    assert not sup(BF16, 576, 512, 0, 1, 64) and not sup(BF16, 576, 512, 16, 0, 64)
    for p in (0, 8, 48, 512):
        assert not sup(BF16, 576, 512, 16, 1, p)


def mla_call(lib, q=OK, kv=OK, o=OK, bt=INT_OK, sl=INT_OK, ws=OK, B=2, Hq=16, Nq=2, Dqk=576, Dv=512, P_=64, num_pages=100, max_pages=8,
             scale=0.0722, qs=None, os_=None, kps=64 * 576, krs=576, bts=8, causal=1, dtype=BF16, wsb=None):
    qs = (Hq * Nq * 576, Nq * 576, 576) if qs is None else qs
    os_ = (Hq * Nq * 512, Nq * 512, 512) if os_ is None else os_
    if wsb is None:
        wsb = lib.fa_fwd_mla_decode_paged_workspace_bytes(2, 16, 2, 512, 64, 8)
    return lib.fa_fwd_mla_decode_paged(q, kv, o, None, bt, sl, B, Hq, Nq, Dqk, Dv, P_, num_pages, max_pages, scale, *qs, *os_, kps, krs, bts,
                                       causal, dtype, ws, wsb, None)


def decode_call(lib, q=OK, kv=OK, o=OK, bt=INT_OK, sl=INT_OK, ws=OK, B=2, Hq=16, Nq=2, P_=64, num_pages=100, max_pages=8, scale=0.0722,
                kps=64 * 128, krs=128, bts=8, wsb=None, **_):
    if wsb is None:
        wsb = lib.fa_fwd_decode_paged_workspace_bytes(2, 16, 1, 2, 128, 64, 8)
    return lib.fa_fwd_decode_paged(q, kv, kv, o, None, bt, sl, B, Hq, 1, Nq, 128, P_, num_pages, max_pages, scale, Hq * Nq * 128, Nq * 128, kps,
                                   P_ * krs, krs, bts, 1, BF16, BF16, ws, wsb, None)


# the rules both calls apply through the shared helpers: what to break, the status, a word of the message
SHARED = [({"q": None}, -1, "null pointer"), ({"ws": None}, -1, "null pointer"), ({"sl": None}, -1, "null pointer"),
          ({"B": 0}, -1, "sizes must be >= 1"), ({"max_pages": 0}, -1, "sizes must be >= 1"),
          ({"scale": 0.0}, -1, "scale"), ({"scale": float("nan")}, -1, "scale"),
          ({"bts": 7}, -1, "block_table_stride"),
          ({"krs": 8}, -1, "bad page strides"), ({"kps": 64 * 576 + 4}, -1, "bad page strides"), ({"bts": 1 << 31}, -1, "bad page strides"),
          ({"P_": 256, "krs": 1 << 22, "kps": 1 << 30}, -1, "one page of one head exceeds 2 GiB"),
          ({"kv": ODD}, -1, "tensors and workspace must be 16-byte aligned"), ({"ws": ODD}, -1, "16-byte aligned"),
          ({"bt": INT_ODD}, -1, "int32-aligned"), ({"sl": INT_ODD}, -1, "int32-aligned"),
          ({"P_": 256, "max_pages": (1 << 22) + 1, "bts": (1 << 22) + 1, "wsb": 1 << 40}, -1, "capacity above 2^30 keys"),
          ({"B": 1 << 23, "wsb": 1 << 60}, -1, "grid too large")]


def test_rules_shared_with_the_paged_decode_have_its_status_and_text(lib):
    for kw, status, word in SHARED:
        assert mla_call(lib, **kw) == status, kw
        mine = lib.fa_last_error().decode()
        assert decode_call(lib, **kw) == status, kw
        theirs = lib.fa_last_error().decode()
        assert mine.startswith("fa_fwd_mla_decode_paged: ") and theirs.startswith("fa_fwd_decode_paged: ") and word in mine, (kw, mine, theirs)
        assert mine.split(": ", 1)[1] == theirs.split(": ", 1)[1], (kw, mine, theirs)


def test_rules_of_its_own(lib):
    rules = [({"Dqk": 512}, -2, "Dqk=512"), ({"Dv": 576}, -2, "Dv=576"), ({"dtype": F32}, -2, "dtype=f32"), ({"dtype": FP8}, -2, "fp8_e4m3"),
             ({"Hq": 17}, -2, "Hq=17 Nq=2"), ({"P_": 48}, -2, "page_size=48"),
             ({"qs": (32 * 576, 2 * 576, 512)}, -1, "bad strides"), ({"qs": (32 * 576, 2 * 576 + 4, 576)}, -1, "bad strides"),
             ({"qs": (-576, 2 * 576, 576)}, -1, "bad strides"), ({"qs": (8, 2 * 576, 576)}, -1, "bad strides"),
             ({"os_": (32 * 512, 2 * 512, 504)}, -1, "bad output strides"), ({"os_": (32 * 512 + 2, 2 * 512, 512)}, -1, "bad output strides"),
             ({"krs": 512}, -1, "bad page strides"), ({"o": ODD}, -1, "16-byte aligned")]
    for kw, status, word in rules:
        assert mla_call(lib, **kw) == status, kw
        msg = lib.fa_last_error().decode()
        assert msg.startswith("fa_fwd_mla_decode_paged: ") and word in msg, (kw, msg)
    # (every case above breaks one rule of a valid call, so none of them launches; the legal layouts -- token-major q and o, padded rows --
    # run in tests/test_gpu_mla_decode.py)


def test_workspace_size_and_a_workspace_one_byte_short(lib):
    size = lib.fa_fwd_mla_decode_paged_workspace_bytes
    need = size(2, 16, 2, 512, 64, 8)
    # capacity 512 keys = 8 tiles: S = min(ceil(256 / (2 sequences * 2 row blocks)), 8 / 4) = 2; B * S * rows16 * (Dv + 2) floats
    assert need == 2 * 2 * 32 * 514 * 4
    assert size(1, 16, 1, 512, 64, 1024) == 1 * 256 * 16 * 514 * 4  # 65536 keys, one sequence, one row block: S = 256
    assert size(128, 16, 1, 512, 16, 256) == 128 * 2 * 16 * 514 * 4
    assert mla_call(lib, wsb=need - 1) == -1
    msg = lib.fa_last_error().decode()
    assert msg == f"fa_fwd_mla_decode_paged: workspace of {need - 1} bytes, fa_fwd_mla_decode_paged_workspace_bytes() asks for {need}"
    for bad in ((0, 16, 1, 512, 64, 8), (2, 0, 1, 512, 64, 8), (2, 16, 0, 512, 64, 8), (2, 16, 3, 512, 64, 8), (2, 16, 1, 576, 64, 8),
                (2, 16, 1, 512, 48, 8), (2, 16, 1, 512, 64, 0), (2, 16, 1, 512, 256, (1 << 22) + 1), (-1, 16, 1, 512, 64, 8)):
        assert size(*bad) == 0, bad


def test_python_wrapper_refuses_bad_arguments(fa):
    import torch

    q = torch.zeros(2, 16, 1, 576, dtype=torch.bfloat16)
    pool = torch.zeros(4, 64, 576, dtype=torch.bfloat16)
    bt, sl = torch.zeros(2, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(TypeError):
        fa.flash_attention_mla_decode_paged(q, pool, bt, sl)  # scale is required
    with pytest.raises(ValueError, match="scale"):
        fa.flash_attention_mla_decode_paged(q, pool, bt, sl, None)
    with pytest.raises(ValueError, match="no CPU path"):
        fa.flash_attention_mla_decode_paged(q, pool, bt, sl, 0.07)
    with pytest.raises(ValueError, match="latent pool"):
        fa.flash_attention_mla_decode_paged(q[0], pool, bt, sl, 0.07)
    with pytest.raises(ValueError, match="latent pool"):
        fa.flash_attention_mla_decode_paged(q, pool.reshape(4, 32, 2, 576), bt, sl, 0.07)
    assert fa.mla_decode_paged_supported("bf16", 576, 512, 16, 2, 64) and not fa.mla_decode_paged_supported("bf16", 576, 512, 16, 3, 64)
    assert fa.mla_decode_paged_workspace_bytes(2, 16, 2, 512, 64, 8) == 2 * 2 * 32 * 514 * 4
    assert fa.mla_decode_paged_workspace_bytes(2, 16, 2, 512, 48, 8) == 0
