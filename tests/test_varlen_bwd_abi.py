"""fa_bwd_varlen without a GPU: the symbols, the support table, every argument rule refused before any launch (fake aligned pointers, as
tests/test_varlen_abi.py), what the Python wrapper refuses, and the shapes the torch op propagates on the meta device."""
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
    for name in ("fa_bwd_varlen", "fa_bwd_varlen_workspace_bytes", "fa_bwd_varlen_supported"):
        assert hasattr(raw, name) and name in SYMBOLS
    lib = fa.load_library()
    assert lib.fa_bwd_varlen.restype is ctypes.c_int and len(lib.fa_bwd_varlen.argtypes) == 28
    assert lib.fa_bwd_varlen_workspace_bytes.restype is ctypes.c_longlong
    assert callable(fa.flash_attention_varlen_backward) and callable(fa.varlen_backward_supported) and callable(fa.varlen_backward_workspace_bytes)
    assert lib.fa_version() == 400


def test_support_table_and_workspace_size(fa):
    lib = fa.load_library()
    for name, code in fa.DTYPES.items():
        for D in (8, 32, 40, 64, 96, 128, 256):
            want = int(name in ("f16", "bf16") and D in (64, 128))
            assert lib.fa_bwd_varlen_supported(code, D) == want, (name, D)
            assert fa.varlen_backward_supported(name, D) == bool(want)
    assert lib.fa_bwd_varlen_supported(9, 64) == 0
    assert lib.fa_bwd_varlen_workspace_bytes(8, 1000) == 8 * 1000 * 4 == fa.varlen_backward_workspace_bytes(8, 1000)
    assert lib.fa_bwd_varlen_workspace_bytes(65536, 65536) == 65536 * 65536 * 4  # no 32-bit overflow
    assert lib.fa_bwd_varlen_workspace_bytes(0, 10) == 0 and lib.fa_bwd_varlen_workspace_bytes(4, 0) == 0 and lib.fa_bwd_varlen_workspace_bytes(-1, 5) == 0


def test_each_rule_refused_before_launch(fa):
    lib = fa.load_library()
    P = ctypes.c_void_p
    ok, odd, odd4 = P(0x1000), P(0x1008), P(0x1002)
    ptrs = ("q", "k", "v", "o", "d_o", "lse", "dq", "dk", "dv", "ws", "cu_q", "cu_k")

    def call(B=3, Hq=8, Hkv=2, total_q=1000, total_k=1500, max_q=400, max_k=600, D=64, scale=0.125, q_rs=None, q_hs=None, kv_rs=None,
             kv_hs=None, causal=1, dtype=2, **p):
        q_rs = Hq * D if q_rs is None else q_rs
        kv_rs = Hkv * D if kv_rs is None else kv_rs
        return lib.fa_bwd_varlen(*[p.get(n, ok) for n in ptrs], B, Hq, Hkv, total_q, total_k, max_q, max_k, D, scale, q_rs,
                                 D if q_hs is None else q_hs, kv_rs, D if kv_hs is None else kv_hs, causal, dtype, None)

    big_rows = (1 << 32) // (64 * 2) - 64  # one sequence of 4 GiB minus one tile at row pitch 64: refused with the forward's +128-row margin
    rules = [({n: None}, -1, "null") for n in ptrs]
    rules += [
        ({"B": 0}, -1, ">= 1"), ({"Hq": 0}, -1, ">= 1"), ({"Hkv": 0}, -1, ">= 1"), ({"total_q": 0}, -1, ">= 1"), ({"total_k": 0}, -1, ">= 1"),
        ({"max_q": 0}, -1, ">= 1"), ({"max_k": 0}, -1, ">= 1"), ({"D": 0}, -1, ">= 1"),
        ({"Hkv": 3}, -1, "Hkv"),
        ({"scale": 0.0}, -1, "scale"), ({"scale": -1.0}, -1, "scale"), ({"scale": float("nan")}, -1, "scale"),
        ({"dtype": 0}, -2, "f16 / bf16"), ({"dtype": 3}, -2, "f16 / bf16"), ({"D": 96, "q_rs": 8 * 96, "kv_rs": 2 * 96}, -2, "D = 64 | 128"),
        ({"D": 256, "q_rs": 8 * 256, "kv_rs": 2 * 256}, -2, "D = 64 | 128"), ({"D": 32, "q_rs": 8 * 32, "kv_rs": 2 * 32}, -2, "D = 64 | 128"),
        ({"max_q": 1001}, -1, "max_seqlen"), ({"max_k": 1501}, -1, "max_seqlen"),
        ({"q_rs": 8 * 64 + 4}, -1, "stride"), ({"q_hs": 68}, -1, "stride"), ({"q_rs": 56}, -1, "stride"), ({"q_hs": 56}, -1, "stride"),
        ({"kv_rs": 2 * 64 + 4}, -1, "key/value strides"), ({"kv_hs": 68}, -1, "key/value strides"), ({"kv_rs": 32}, -1, "key/value strides"),
    ]
    rules += [({n: odd}, -1, "aligned") for n in ("q", "k", "v", "o", "d_o", "dq", "dk", "dv")]
    rules += [
        ({"cu_q": odd4}, -1, "int32"), ({"cu_k": odd4}, -1, "int32"), ({"lse": odd4}, -1, "fp32"), ({"ws": odd4}, -1, "fp32"),
        ({"Hq": 1, "Hkv": 1, "q_rs": 64, "total_q": big_rows, "max_q": big_rows}, -1, "4 GiB"),
        ({"Hq": 1, "Hkv": 1, "q_rs": 64, "kv_rs": 64, "total_k": big_rows, "max_k": big_rows}, -1, "4 GiB"),
        ({"q_rs": 1 << 24, "total_q": 1 << 20, "max_q": 1 << 10}, -1, "4 GiB"),  # a wide row pitch counts, not D
        ({"B": 65536, "Hq": 65536, "Hkv": 65536, "q_rs": 64, "q_hs": 64, "kv_rs": 64, "kv_hs": 64}, -1, "grid"),
        # the dK/dV grid alone: few query blocks, many key blocks
        ({"B": 1 << 14, "Hq": 1 << 10, "Hkv": 1 << 10, "q_rs": 64, "q_hs": 64, "kv_rs": 64, "kv_hs": 64, "max_q": 128, "total_k": 1 << 20,
          "max_k": 1 << 15}, -1, "grid"),
    ]
    for kw, status, word in rules:
        assert call(**kw) == status, (kw, lib.fa_last_error())
        msg = lib.fa_last_error().decode()
        assert msg.startswith("fa_bwd_varlen:") and word in msg, (kw, msg)
    # just inside the 4 GiB rule nothing is refused by it: the next rule to fail is the one broken on purpose (still no launch)
    assert call(Hq=1, Hkv=1, q_rs=64, total_q=big_rows - 128, max_q=big_rows - 128, dv=odd) == -1 and b"aligned" in lib.fa_last_error()


def _tensors(torch, dtype=None):
    dtype = dtype or torch.bfloat16
    q = torch.zeros(10, 4, 64, dtype=dtype)
    k = torch.zeros(12, 2, 64, dtype=dtype)
    lse = torch.zeros(4, 10)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    return q, k, lse, cu


def test_wrapper_refuses_what_the_kernel_cannot_take(fa):
    import torch

    q, k, lse, cu = _tensors(torch)
    bw = fa.flash_attention_varlen_backward
    with pytest.raises(RuntimeError, match="no CPU path"):
        bw(q, k, k, q, q, lse, cu, cu, 10, 12)
    # shapes, dtypes, strides and tables are checked before the device is: CPU tensors reach these checks
    with pytest.raises(ValueError, match="dtypes"):
        bw(q, k.to(torch.float16), k, q, q, lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="dtypes"):
        bw(q, k, k, q, q.float(), lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="dtypes"):
        bw(q.float(), k.float(), k.float(), q.float(), q.float(), lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="shape"):
        bw(q[None], k, k, q[None], q[None], lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="shape"):
        bw(q, k, k, q[:9], q, lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="incompatible"):
        k3 = torch.zeros(12, 3, 64, dtype=torch.bfloat16)
        bw(q, k3, k3, q, q, lse, cu, cu, 10, 12)


def test_wrapper_checks_strides_tables_lse_outputs_and_workspace(fa):
    import torch

    q, k, lse, cu = _tensors(torch)
    bw = fa.flash_attention_varlen_backward
    wide = torch.zeros(10, 4, 128, dtype=torch.bfloat16)[:, :, ::2]
    with pytest.raises(ValueError, match="unit element stride"):
        bw(wide, k, k, wide, wide, lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="q, o and d_o must share"):
        bw(q, k, k, torch.zeros(4, 10, 64, dtype=torch.bfloat16).transpose(0, 1), q, lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="q, o and d_o must share"):
        bw(q, k, k, q, torch.zeros(4, 10, 64, dtype=torch.bfloat16).transpose(0, 1), lse, cu, cu, 10, 12)
    with pytest.raises(ValueError, match="k and v must share"):
        bw(q, k, torch.zeros(12, 4, 64, dtype=torch.bfloat16)[:, ::2], q, q, lse, cu, cu, 10, 12)
    for bad in (torch.tensor([0, 4, 10], dtype=torch.int64), torch.zeros(3, 1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                torch.zeros(6, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match="cu_seqlens_q must be a contiguous int32"):
            bw(q, k, k, q, q, lse, bad, cu, 10, 12)
        with pytest.raises(ValueError, match="cu_seqlens_k must be a contiguous int32"):
            bw(q, k, k, q, q, lse, cu, bad, 10, 12)
    with pytest.raises(ValueError, match=r"both be \[B \+ 1\]"):
        bw(q, k, k, q, q, lse, cu, torch.tensor([0, 12], dtype=torch.int32), 10, 12)
    for bad in (torch.zeros(10, 4), torch.zeros(4, 10, dtype=torch.float64), torch.zeros(4, 20)[:, ::2]):
        with pytest.raises(ValueError, match=r"lse must be contiguous fp32 \[Hq, total_q\]"):
            bw(q, k, k, q, q, bad, cu, cu, 10, 12)


def test_meta_device_shape_propagation_of_the_op(fa):
    import torch

    from flash_attention_metal_amd import torch_op

    assert callable(torch_op.attention_varlen)
    q = torch.empty(10, 8, 128, dtype=torch.float16, device="meta")
    k = torch.empty(12, 2, 128, dtype=torch.float16, device="meta")
    cu = torch.empty(3, dtype=torch.int32, device="meta")
    o, lse = torch.ops.fa_mi355.attention_varlen(q, k, k, cu, cu, 10, 12, True, 0.0)
    assert o.shape == q.shape and o.dtype == q.dtype and o.device.type == "meta"
    assert lse.shape == (8, 10) and lse.dtype == torch.float32
    # a view of a packed QKV projection keeps its strides
    buf = torch.empty(10, 12, 128, dtype=torch.float16, device="meta")
    o, _ = torch_op.attention_varlen(buf[:, :8], buf[:, 8:10], buf[:, 10:], cu, cu, 10, 10)
    assert o.shape == (10, 8, 128)
