"""fa_bwd_varlen_window and fa_window_query_range without a GPU: the symbols, every argument rule of fa_bwd_varlen refused identically
through the new entry point (same status, same text behind the function's name; fake aligned pointers, as tests/test_varlen_bwd_abi.py),
the range function against brute force and against fa_window_key_range, what the Python wrapper refuses, the op's meta shapes."""
import ctypes
import os

import numpy as np
import pytest

import window as W
import window_backward as wb


@pytest.fixture(scope="module")
def fa():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    return fa


def test_symbols_exported_and_bound(fa):
    from flash_attention_metal_amd._lib import SYMBOLS

    raw = ctypes.CDLL(fa.lib_path())
    for name in ("fa_bwd_varlen_window", "fa_window_query_range"):
        assert hasattr(raw, name) and name in SYMBOLS
    lib = fa.load_library()
    assert lib.fa_bwd_varlen_window.restype is ctypes.c_int and len(lib.fa_bwd_varlen_window.argtypes) == 29
    assert len(lib.fa_window_query_range.argtypes) == 8
    assert lib.fa_version() == 400


def test_each_rule_of_fa_bwd_varlen_refused_identically(fa):
    lib = fa.load_library()
    P = ctypes.c_void_p
    ok, odd, odd4 = P(0x1000), P(0x1008), P(0x1002)
    ptrs = ("q", "k", "v", "o", "d_o", "lse", "dq", "dk", "dv", "ws", "cu_q", "cu_k")

    def call(fn, mask, B=3, Hq=8, Hkv=2, total_q=1000, total_k=1500, max_q=400, max_k=600, D=64, scale=0.125, q_rs=None, q_hs=None,
             kv_rs=None, kv_hs=None, dtype=2, **p):
        q_rs = Hq * D if q_rs is None else q_rs
        kv_rs = Hkv * D if kv_rs is None else kv_rs
        st = getattr(lib, fn)(*[p.get(n, ok) for n in ptrs], B, Hq, Hkv, total_q, total_k, max_q, max_k, D, scale, q_rs,
                              D if q_hs is None else q_hs, kv_rs, D if kv_hs is None else kv_hs, *mask, dtype, None)
        return st, lib.fa_last_error().decode()

    big_rows = (1 << 32) // (64 * 2) - 64
    rules = [{n: None} for n in ptrs]
    rules += [{"B": 0}, {"Hq": 0}, {"Hkv": 0}, {"total_q": 0}, {"total_k": 0}, {"max_q": 0}, {"max_k": 0}, {"D": 0}, {"Hkv": 3},
              {"scale": 0.0}, {"scale": -1.0}, {"scale": float("nan")}, {"dtype": 0}, {"dtype": 3},
              {"D": 96, "q_rs": 8 * 96, "kv_rs": 2 * 96}, {"D": 256, "q_rs": 8 * 256, "kv_rs": 2 * 256}, {"D": 32, "q_rs": 8 * 32, "kv_rs": 2 * 32},
              {"max_q": 1001}, {"max_k": 1501}, {"q_rs": 8 * 64 + 4}, {"q_hs": 68}, {"q_rs": 56}, {"q_hs": 56}, {"kv_rs": 2 * 64 + 4},
              {"kv_hs": 68}, {"kv_rs": 32}]
    rules += [{n: odd} for n in ("q", "k", "v", "o", "d_o", "dq", "dk", "dv")]
    rules += [{"cu_q": odd4}, {"cu_k": odd4}, {"lse": odd4}, {"ws": odd4},
              {"Hq": 1, "Hkv": 1, "q_rs": 64, "total_q": big_rows, "max_q": big_rows},
              {"Hq": 1, "Hkv": 1, "q_rs": 64, "kv_rs": 64, "total_k": big_rows, "max_k": big_rows},
              {"q_rs": 1 << 24, "total_q": 1 << 20, "max_q": 1 << 10},
              {"B": 65536, "Hq": 65536, "Hkv": 65536, "q_rs": 64, "q_hs": 64, "kv_rs": 64, "kv_hs": 64},
              {"B": 1 << 14, "Hq": 1 << 10, "Hkv": 1 << 10, "q_rs": 64, "q_hs": 64, "kv_rs": 64, "kv_hs": 64, "max_q": 128, "total_k": 1 << 20,
               "max_k": 1 << 15}]
    for kw in rules:
        st0, msg0 = call("fa_bwd_varlen", (1,), **kw)
        assert st0 < 0 and msg0.startswith("fa_bwd_varlen: "), (kw, st0, msg0)
        for window in ((63, 0), (-1, 0), (-1, -1), (W.INT_MAX, W.INT_MAX)):  # whichever kernels the pair would route to
            st, msg = call("fa_bwd_varlen_window", window, **kw)
            assert st == st0 and msg == "fa_bwd_varlen_window: " + msg0[len("fa_bwd_varlen: "):], (kw, window, st, msg)


def _range(lib, fn, *args):
    a, b = ctypes.c_int(-7), ctypes.c_int(-7)
    assert getattr(lib, fn)(*args, ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


def _brute(vis, k0, k1):
    """window_backward.query_range on a visibility matrix built once."""
    rows = np.nonzero(vis[:, max(k0, 0):max(k1 + 1, 0)].any(1))[0]
    return (int(rows[0]), int(rows[-1]) + 1) if len(rows) else None


def test_query_range_matches_brute_force(fa):
    lib = fa.load_library()
    for Lq, Lk in W.SEQS:
        edges = sorted({0, 1, 31, 32, 63, 64, 127, 128, 255, 256, Lk - 1, Lk, Lk + 5, -3})
        for wl in W.WL:
            for wr in W.WR + (W.INT_MAX,):
                vis = W.visible(Lq, Lk, wl, wr)
                assert wb.query_range(Lq, Lk, wl, wr, 0, 127) == _brute(vis, 0, 127)
                for k0 in edges:
                    for k1 in (k0, k0 + 31, k0 + 127, W.INT_MAX):
                        lo, hi = _range(lib, "fa_window_query_range", Lq, Lk, wl, wr, k0, k1)
                        want = _brute(vis, k0, min(k1, Lk))
                        assert (None if lo >= hi else (lo, hi)) == want, ((Lq, Lk), (wl, wr), (k0, k1), (lo, hi), want)
                        assert 0 <= lo <= Lq and 0 <= hi <= Lq
    assert lib.fa_window_query_range(-1, 5, 0, 0, 0, 0, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())) == -1
    assert b"fa_window_query_range" in lib.fa_last_error()
    assert lib.fa_window_query_range(5, 5, 0, 0, 0, 0, None, ctypes.byref(ctypes.c_int())) == -1
    # extreme arguments: 64-bit arithmetic inside
    assert _range(lib, "fa_window_query_range", W.INT_MAX, W.INT_MAX, W.INT_MAX, W.INT_MAX, 0, W.INT_MAX) == (0, W.INT_MAX)
    assert _range(lib, "fa_window_query_range", W.INT_MAX, 1, 0, 0, -2 ** 31, W.INT_MAX) == (W.INT_MAX - 1, W.INT_MAX)


def test_query_range_is_the_inverse_of_key_range(fa):
    lib = fa.load_library()
    for Lq, Lk in W.SEQS[:6]:
        for wl in (0, 31, 64, 200, -1):
            for wr in (0, 5, 64, -1):
                keys_of = [_range(lib, "fa_window_key_range", Lq, Lk, wl, wr, i, i) for i in range(Lq)]
                rows_of = [_range(lib, "fa_window_query_range", Lq, Lk, wl, wr, j, j) for j in range(Lk)]
                a = np.array([[lo <= j < hi for j in range(Lk)] for lo, hi in keys_of], bool).reshape(Lq, Lk)
                b = np.array([[lo <= i < hi for lo, hi in rows_of] for i in range(Lq)], bool).reshape(Lq, Lk)
                assert (a == b).all() and (a == W.visible(Lq, Lk, wl, wr)).all(), ((Lq, Lk), (wl, wr))


def test_wrapper_refuses_bad_windows_as_the_forward_wrappers_do(fa):
    import torch

    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16)
    k = torch.zeros(12, 2, 64, dtype=torch.bfloat16)
    lse = torch.zeros(4, 10)
    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    bw = fa.flash_attention_varlen_backward
    # the keyword reaches validation before anything touches a device: CPU tensors are refused as without it
    with pytest.raises(RuntimeError, match="no CPU path"):
        bw(q, k, k, q, q, lse, cu, cu, 10, 12, window=(3, 0))
    with pytest.raises(ValueError, match="dtypes"):
        bw(q, k.to(torch.float16), k, q, q, lse, cu, cu, 10, 12, window=(3, 0))
    from flash_attention_metal_amd import torch_op

    qm = torch.empty(10, 8, 128, dtype=torch.float16, device="meta")
    km = torch.empty(12, 2, 128, dtype=torch.float16, device="meta")
    cum = torch.empty(3, dtype=torch.int32, device="meta")
    for bad in ((1,), (1, 2, 3), "ab", (2 ** 31, 0), (None, 0)):
        with pytest.raises(ValueError, match="window"):
            torch_op.attention_varlen(qm, km, km, cum, cum, 10, 12, window=bad)
    with pytest.raises(ValueError, match="is_causal"):
        torch_op.attention_varlen(qm, km, km, cum, cum, 10, 12, True, window=(3, 5))


def test_meta_device_shape_propagation_of_the_window_op(fa):
    import torch

    from flash_attention_metal_amd import torch_op

    q = torch.empty(10, 8, 128, dtype=torch.float16, device="meta")
    k = torch.empty(12, 2, 128, dtype=torch.float16, device="meta")
    cu = torch.empty(3, dtype=torch.int32, device="meta")
    o, lse = torch.ops.fa_mi355.attention_varlen_window(q, k, k, cu, cu, 10, 12, 63, 0, 0.0)
    assert o.shape == q.shape and o.dtype == q.dtype and o.device.type == "meta"
    assert lse.shape == (8, 10) and lse.dtype == torch.float32
    buf = torch.empty(10, 12, 128, dtype=torch.float16, device="meta")
    o, _ = torch_op.attention_varlen(buf[:, :8], buf[:, 8:10], buf[:, 10:], cu, cu, 10, 10, window=(63, -1))
    assert o.shape == (10, 8, 128)
    # the existing op and its schema stay as they are
    o, _ = torch_op.attention_varlen(q, k, k, cu, cu, 10, 12, True)
    assert o.shape == q.shape
    names = [a.name for a in torch.ops.fa_mi355.attention_varlen.default._schema.arguments]
    assert names == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "is_causal", "scale"]
