"""fa_fwd_varlen without a GPU: the symbols, the support table, every argument rule refused before any launch (fake aligned pointers, as
tests/test_abi.py), and what the Python wrapper refuses."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def fa():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    return fa


def test_symbols_exported_and_bound(fa):
    from flash_attention_metal_amd._lib import SYMBOLS

    raw = ctypes.CDLL(fa.lib_path())
    for name in ("fa_fwd_varlen", "fa_fwd_varlen_supported"):
        assert hasattr(raw, name) and name in SYMBOLS
    lib = fa.load_library()
    assert lib.fa_fwd_varlen.restype is ctypes.c_int and len(lib.fa_fwd_varlen.argtypes) == 23
    assert callable(fa.flash_attention_varlen) and callable(fa.varlen_supported)
    assert lib.fa_version() == 400


def test_support_table(fa):
    lib = fa.load_library()
    for name, code in fa.DTYPES.items():
        for D in (8, 32, 40, 64, 96, 128, 256):
            want = int(name in ("f16", "bf16") and D in (64, 128))
            assert lib.fa_fwd_varlen_supported(code, D) == want, (name, D)
            assert fa.varlen_supported(name, D) == bool(want)
    assert lib.fa_fwd_varlen_supported(9, 64) == 0


def test_each_rule_refused_before_launch(fa):
    lib = fa.load_library()
    P = ctypes.c_void_p
    ok, odd, odd4 = P(0x1000), P(0x1008), P(0x1002)

    def call(q=ok, k=ok, v=ok, o=ok, lse=None, cu_q=ok, cu_k=ok, B=3, Hq=8, Hkv=2, total_q=1000, total_k=1500, max_q=400, max_k=600, D=64,
             scale=0.125, q_rs=None, q_hs=None, kv_rs=None, kv_hs=None, causal=1, dtype=2):
        q_rs = Hq * D if q_rs is None else q_rs
        kv_rs = Hkv * D if kv_rs is None else kv_rs
        return lib.fa_fwd_varlen(q, k, v, o, lse, cu_q, cu_k, B, Hq, Hkv, total_q, total_k, max_q, max_k, D, scale, q_rs, D if q_hs is None else q_hs,
                                 kv_rs, D if kv_hs is None else kv_hs, causal, dtype, None)

    big_rows = (1 << 32) // (64 * 2) - 64  # one sequence of 4 GiB minus one tile at row pitch 64: refused with fa_fwd's +128-row margin
    rules = [
        ({"q": None}, -1, "null"), ({"k": None}, -1, "null"), ({"v": None}, -1, "null"), ({"o": None}, -1, "null"),
        ({"cu_q": None}, -1, "null"), ({"cu_k": None}, -1, "null"),
        ({"B": 0}, -1, ">= 1"), ({"Hq": 0}, -1, ">= 1"), ({"Hkv": 0}, -1, ">= 1"), ({"total_q": 0}, -1, ">= 1"), ({"total_k": 0}, -1, ">= 1"),
        ({"max_q": 0}, -1, ">= 1"), ({"max_k": 0}, -1, ">= 1"), ({"D": 0}, -1, ">= 1"),
        ({"Hkv": 3}, -1, "Hkv"),
        ({"scale": 0.0}, -1, "scale"), ({"scale": float("nan")}, -1, "scale"),
        ({"dtype": 0}, -2, "f16 / bf16"), ({"dtype": 3}, -2, "f16 / bf16"), ({"D": 96, "q_rs": 8 * 96, "kv_rs": 2 * 96}, -2, "D = 64 | 128"),
        ({"D": 256, "q_rs": 8 * 256, "kv_rs": 2 * 256}, -2, "D = 64 | 128"),
        ({"max_q": 1001}, -1, "max_seqlen"), ({"max_k": 1501}, -1, "max_seqlen"),
        ({"q_rs": 8 * 64 + 4}, -1, "stride"), ({"q_hs": 68}, -1, "stride"), ({"q_rs": 56}, -1, "stride"), ({"q_hs": 56}, -1, "stride"),
        ({"kv_rs": 2 * 64 + 4}, -1, "key/value strides"), ({"kv_hs": 68}, -1, "key/value strides"), ({"kv_rs": 32}, -1, "key/value strides"),
        ({"q": odd}, -1, "aligned"), ({"k": odd}, -1, "aligned"), ({"v": odd}, -1, "aligned"), ({"o": odd}, -1, "aligned"),
        ({"cu_q": odd4}, -1, "int32"), ({"cu_k": odd4}, -1, "int32"),
        ({"Hq": 1, "Hkv": 1, "q_rs": 64, "total_q": big_rows, "max_q": big_rows}, -1, "4 GiB"),
        ({"Hq": 1, "Hkv": 1, "q_rs": 64, "kv_rs": 64, "total_k": big_rows, "max_k": big_rows}, -1, "4 GiB"),
        ({"q_rs": 1 << 24, "total_q": 1 << 20, "max_q": 1 << 10}, -1, "4 GiB"),  # a wide row pitch counts, not D
        ({"B": 65536, "Hq": 65536, "Hkv": 65536, "q_rs": 64, "q_hs": 64, "kv_rs": 64, "kv_hs": 64}, -1, "grid"),
    ]
    for kw, status, word in rules:
        assert call(**kw) == status, (kw, lib.fa_last_error())
        msg = lib.fa_last_error().decode()
        assert msg.startswith("fa_fwd_varlen:") and word in msg, (kw, msg)
    # just inside the 4 GiB rule nothing is refused by it: the next rule to fail is the one broken on purpose (still no launch)
    assert call(Hq=1, Hkv=1, q_rs=64, total_q=big_rows - 128, max_q=big_rows - 128, o=None) == -1 and b"null" in lib.fa_last_error()


def test_wrapper_refuses_what_the_kernel_cannot_take(fa):
    import torch

    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16)
    k = torch.zeros(12, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 10], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa.flash_attention_varlen(q, k, k, cu, cu, 10, 12)
    # shapes, dtypes, strides and tables are checked first
    with pytest.raises(ValueError, match="dtypes"):
        fa.flash_attention_varlen(q, k.to(torch.float16), k, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="dtypes"):
        fa.flash_attention_varlen(q.float(), k.float(), k.float(), cu, cu, 10, 12)
    with pytest.raises(ValueError, match="shape"):
        fa.flash_attention_varlen(q[None], k, k, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="incompatible"):
        fa.flash_attention_varlen(q, torch.zeros(12, 3, 64, dtype=torch.bfloat16), torch.zeros(12, 3, 64, dtype=torch.bfloat16), cu, cu, 10, 12)


def test_wrapper_checks_strides_and_tables(fa):
    import torch

    # (shapes, dtypes, strides and tables are checked before the device is: CPU tensors reach these checks)
    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16)
    k = torch.zeros(12, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    wide = torch.zeros(10, 4, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="unit element stride"):
        fa.flash_attention_varlen(wide[:, :, ::2], k, k, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="unit element stride"):
        fa.flash_attention_varlen(q, torch.zeros(12, 2, 128, dtype=torch.bfloat16)[:, :, ::2], k, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="share row/head strides"):
        fa.flash_attention_varlen(q, k, torch.zeros(12, 4, 64, dtype=torch.bfloat16)[:, ::2], cu, cu, 10, 12)
    for bad in (torch.tensor([0, 4, 10], dtype=torch.int64), torch.zeros(3, 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                torch.zeros(6, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="cu_seqlens_q must be a contiguous int32"):
            fa.flash_attention_varlen(q, k, k, bad, cu, 10, 12)
        with pytest.raises(ValueError, match="cu_seqlens_k must be a contiguous int32"):
            fa.flash_attention_varlen(q, k, k, cu, bad, 10, 12)
    with pytest.raises(ValueError, match=r"both be \[B \+ 1\]"):
        fa.flash_attention_varlen(q, k, k, cu, torch.tensor([0, 12], dtype=torch.int32), 10, 12)
