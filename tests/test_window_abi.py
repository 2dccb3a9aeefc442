"""The sliding-window entry points without a GPU: exported and bound, every argument rule of the three un-windowed calls refused identically
(fake aligned pointers, as test_varlen_paged_abi.py does: no call here may pass validation), fa_window_key_range against brute force over
the visibility rule, and the Python keyword."""
import ctypes
import os

import numpy as np
import pytest

import window as wn

F16, BF16, FP8 = 1, 2, 3
INT_MAX = wn.INT_MAX
P_ = ctypes.c_void_p
OK, OK4 = 0x10000, 0x20000
WINDOWS = ((63, 0), (-1, -1), (-1, 0), (INT_MAX, INT_MAX), (0, 5))


@pytest.fixture(scope="module")
def fa():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    return fa


def test_symbols_exported_and_bound(fa):
    from flash_attention_metal_amd._lib import SYMBOLS

    lib = ctypes.CDLL(fa.lib_path())
    for old, new in (("fa_fwd_varlen", "fa_fwd_varlen_window"), ("fa_fwd_varlen_paged", "fa_fwd_varlen_paged_window"),
                     ("fa_fwd_decode_paged", "fa_fwd_decode_paged_window")):
        assert hasattr(lib, new) and new in SYMBOLS, new
        assert len(SYMBOLS[new][1]) == len(SYMBOLS[old][1]) + 1  # is_causal -> window_left, window_right
    assert hasattr(lib, "fa_window_key_range") and len(SYMBOLS["fa_window_key_range"][1]) == 8
    assert fa.load_library().fa_version() == 400
    header = open(os.path.join(os.path.dirname(fa.lib_path()), "..", "..", "include", "fa_mi355.h")).read()
    for word in ("ROUTING IS BY SIGN ONLY", "CLAMPED ON THE HOST", "fa_window_key_range", "t_lo + floor(s n / S)"):
        assert word in header, word


def _ptrs(*xs):
    return [None if x is None else P_(x) for x in xs]


def _varlen(lib, mask, q=OK, k=OK, v=OK, o=OK, lse=None, cu_q=OK4, cu_k=OK4, B=3, Hq=8, Hkv=2, total_q=1000, total_k=1500, max_q=400, max_k=600,
            D=64, scale=0.125, q_rs=None, q_hs=None, kv_rs=None, kv_hs=None, dtype=BF16):
    q_rs, kv_rs = (Hq * D if q_rs is None else q_rs), (Hkv * D if kv_rs is None else kv_rs)
    fn = lib.fa_fwd_varlen if len(mask) == 1 else lib.fa_fwd_varlen_window
    return fn(*_ptrs(q, k, v, o, lse, cu_q, cu_k), B, Hq, Hkv, total_q, total_k, max_q, max_k, D, scale, q_rs, D if q_hs is None else q_hs, kv_rs,
              D if kv_hs is None else kv_hs, *mask, dtype, None)


def _paged(lib, mask, q=OK, k=OK, v=OK, o=OK, lse=None, cu=OK4, bt=OK4, sl=OK4, B=2, Hq=8, Hkv=2, total_q=300, max_q=200, D=64, P=16,
           num_pages=100, mp=8, scale=0.125, qrs=None, qhs=None, ps=None, hs=None, rs=None, bts=None, dt=BF16):
    qrs, qhs = (Hq * D if qrs is None else qrs), (D if qhs is None else qhs)
    ps, hs, rs = (Hkv * P * D if ps is None else ps), (P * D if hs is None else hs), (D if rs is None else rs)
    bts = mp if bts is None else bts
    fn = lib.fa_fwd_varlen_paged if len(mask) == 1 else lib.fa_fwd_varlen_paged_window
    return fn(*_ptrs(q, k, v, o, lse, cu, bt, sl), B, Hq, Hkv, total_q, max_q, D, P, num_pages, mp, scale, qrs, qhs, ps, hs, rs, bts, *mask, dt, None)


def _decode(lib, mask, q=OK, k=OK, v=OK, o=OK, bt=OK4, sl=OK4, B=2, Hq=8, Hkv=2, Nq=1, D=64, P=16, num_pages=100, mp=8, scale=0.125,
            qbs=None, qhs=None, ps=None, hs=None, rs=None, bts=None, qdt=BF16, kvdt=BF16, ws=OK, wsb=0):
    qhs = Nq * D if qhs is None else qhs
    qbs = Hq * qhs if qbs is None else qbs
    ps, hs, rs = (Hkv * P * D if ps is None else ps), (P * D if hs is None else hs), (D if rs is None else rs)
    bts = mp if bts is None else bts
    fn = lib.fa_fwd_decode_paged if len(mask) == 1 else lib.fa_fwd_decode_paged_window
    return fn(*_ptrs(q, k, v, o, None, bt, sl), B, Hq, Hkv, Nq, D, P, num_pages, mp, scale, qbs, qhs, ps, hs, rs, bts, *mask, qdt, kvdt,
              None if ws is None else P_(ws), wsb, None)


BIG_ROWS = (1 << 32) // (64 * 2) - 64
VARLEN_RULES = (
    [{n: None} for n in ("q", "k", "v", "o", "cu_q", "cu_k")] + [{n: 0} for n in ("B", "Hq", "Hkv", "total_q", "total_k", "max_q", "max_k", "D")] +
    [{"Hkv": 3}, {"scale": 0.0}, {"scale": float("nan")}, {"dtype": 0}, {"dtype": 3}, {"D": 96, "q_rs": 8 * 96, "kv_rs": 2 * 96},
     {"D": 256, "q_rs": 8 * 256, "kv_rs": 2 * 256}, {"max_q": 1001}, {"max_k": 1501}, {"q_rs": 8 * 64 + 4}, {"q_hs": 68}, {"q_rs": 56}, {"q_hs": 56},
     {"kv_rs": 2 * 64 + 4}, {"kv_hs": 68}, {"kv_rs": 32}, {"q": OK + 8}, {"k": OK + 8}, {"v": OK + 8}, {"o": OK + 8}, {"cu_q": OK4 + 2},
     {"cu_k": OK4 + 2}, {"Hq": 1, "Hkv": 1, "q_rs": 64, "total_q": BIG_ROWS, "max_q": BIG_ROWS},
     {"Hq": 1, "Hkv": 1, "q_rs": 64, "kv_rs": 64, "total_k": BIG_ROWS, "max_k": BIG_ROWS}, {"q_rs": 1 << 24, "total_q": 1 << 20, "max_q": 1 << 10},
     {"B": 65536, "Hq": 65536, "Hkv": 65536, "q_rs": 64, "q_hs": 64, "kv_rs": 64, "kv_hs": 64},
     {"lse": OK, "B": 65536, "Hq": 65536, "Hkv": 65536, "q_rs": 64, "q_hs": 64, "kv_rs": 64, "kv_hs": 64}])
PAGED_RULES = (
    [{n: None} for n in ("q", "k", "v", "o", "cu", "bt", "sl")] + [{n: 0} for n in ("B", "Hq", "Hkv", "total_q", "max_q", "D", "P", "num_pages", "mp")] +
    [{"Hq": 6, "Hkv": 4}, {"scale": 0.0}, {"scale": -1.0}, {"P": 8}, {"P": 48}, {"P": 512}, {"D": 32}, {"D": 96}, {"D": 256},
     {"dt": FP8, "qrs": 1024, "rs": 64}, {"dt": 0}, {"max_q": 301}, {"qrs": 100}, {"qrs": 32}, {"qhs": 8}, {"qhs": -64}, {"bts": 7}, {"rs": 100},
     {"rs": 32}, {"hs": -1024}, {"ps": 8}, {"bts": 1 << 31}, {"P": 256, "rs": 1 << 22, "hs": 1 << 22, "ps": 1 << 30}, {"P": 256, "mp": (1 << 22) + 1},
     {"q": OK + 8}, {"k": OK + 8}, {"v": OK + 8}, {"o": OK + 8}, {"bt": OK4 + 2}, {"sl": OK4 + 1}, {"cu": OK4 + 2},
     {"total_q": 1 << 20, "max_q": 1 << 20, "qrs": 2048}, {"B": 1 << 20, "Hq": 1 << 10, "total_q": 256, "max_q": 256},
     {"lse": OK, "B": 1 << 20, "Hq": 1 << 10, "total_q": 256, "max_q": 256}])
DECODE_RULES = (
    [{n: None} for n in ("q", "k", "v", "o", "bt", "sl", "ws")] + [{n: 0} for n in ("B", "Hq", "Hkv", "Nq", "D", "num_pages", "mp", "P")] +
    [{"Hq": 6, "Hkv": 4}, {"scale": 0.0}, {"P": 8}, {"P": 48}, {"P": 512}, {"D": 96}, {"qdt": F16, "kvdt": FP8}, {"qdt": FP8, "kvdt": BF16},
     {"Hq": 64, "Hkv": 1}, {"bts": 7}, {"rs": 100}, {"rs": 32}, {"hs": -1024}, {"qhs": 8}, {"qdt": BF16, "kvdt": FP8, "rs": 72, "hs": 16 * 72, "ps": 2 * 16 * 72},
     {"q": OK + 8}, {"k": OK + 4}, {"ws": OK + 8}, {"bt": OK4 + 2}, {"P": 256, "rs": 1 << 22, "hs": 1 << 22, "ps": 1 << 30}, {"P": 256, "mp": (1 << 22) + 1},
     {"wsb": 0}, {"wsb": 1000}, {"qdt": FP8, "kvdt": FP8, "wsb": 1000}, {"B": 1 << 30, "Hq": 8, "Hkv": 8}])


@pytest.mark.parametrize("old,new,call,rules", [("fa_fwd_varlen", "fa_fwd_varlen_window", _varlen, VARLEN_RULES),
                                                ("fa_fwd_varlen_paged", "fa_fwd_varlen_paged_window", _paged, PAGED_RULES),
                                                ("fa_fwd_decode_paged", "fa_fwd_decode_paged_window", _decode, DECODE_RULES)])
def test_every_rule_is_refused_as_the_unwindowed_call_refuses_it(fa, old, new, call, rules):
    lib = fa.load_library()
    for kw in rules:
        want = call(lib, (1,), **kw)
        msg = lib.fa_last_error().decode()
        assert want in (-1, -2) and msg.startswith(old + ":"), (kw, want, msg)  # no call here passes validation
        for win in WINDOWS:
            got = call(lib, win, **kw)
            assert got == want and lib.fa_last_error().decode() == new + msg[len(old):], (kw, win, got, lib.fa_last_error())


def test_key_range_matches_brute_force(fa):
    lib = fa.load_library()
    lo, hi = ctypes.c_int(), ctypes.c_int()

    def rng(*a):
        assert lib.fa_window_key_range(*a, ctypes.byref(lo), ctypes.byref(hi)) == 0
        return lo.value, hi.value

    for Lq in range(10):
        for Lk in range(10):
            for wl in (-1, 0, 1, 2, 5, INT_MAX):
                for wr in (-1, 0, 1, 2, 5, INT_MAX):
                    for r0 in range(Lq):
                        for r1 in range(r0, Lq):
                            got, want = rng(Lq, Lk, wl, wr, r0, r1), wn.key_range(Lq, Lk, wl, wr, r0, r1)
                            assert (got[0] >= got[1]) if want is None else (got == want), (Lq, Lk, wl, wr, r0, r1, got, want)
                    # rows outside the sequence are clamped away
                    assert rng(Lq, Lk, wl, wr, -5, Lq + 5) == rng(Lq, Lk, wl, wr, 0, Lq - 1) or Lq == 0
    # sizes near 2^30 with INT_MAX windows: Python integers know no wrap
    M = 1 << 30
    for Lq, Lk in ((M, M), (M - 1, M), (M, M - 7), (1, M), (M, 1), (INT_MAX, INT_MAX), (INT_MAX, 1), (5, INT_MAX)):
        for wl, wr in ((INT_MAX, INT_MAX), (INT_MAX, 0), (0, INT_MAX), (INT_MAX, -1), (-1, INT_MAX), (0, 0), (M, M)):
            for r0, r1 in ((0, Lq - 1), (0, 0), (Lq - 1, Lq - 1), (Lq // 2, Lq // 2 + 127), (Lq - 128, INT_MAX), (-INT_MAX, 3)):
                c0, c1 = max(r0, 0), min(r1, Lq - 1)
                a = 0 if wl < 0 else c0 + Lk - Lq - wl
                b = Lk if wr < 0 else c1 + Lk - Lq + wr + 1
                a, b = min(max(a, 0), Lk), min(max(b, 0), Lk)
                got = rng(Lq, Lk, wl, wr, r0, r1)
                assert (got[0] >= got[1]) if (c0 > c1 or a >= b) else (got == (a, b)), (Lq, Lk, wl, wr, r0, r1, got, (a, b))
    # the closed form used above is the brute force on small sizes (so the large sizes are checked against the rule too)
    for Lq, Lk, wl, wr, r0, r1 in ((7, 9, 2, 1, 1, 4), (9, 4, 1, 0, 0, 8), (3, 8, 0, 5, 2, 2)):
        c = Lk - Lq
        assert wn.key_range(Lq, Lk, wl, wr, r0, r1) == (min(max(r0 + c - wl, 0), Lk), min(max(r1 + c + wr + 1, 0), Lk))
    assert lib.fa_window_key_range(4, 4, 0, 0, 0, 3, None, ctypes.byref(hi)) == -1 and b"null" in lib.fa_last_error()
    assert lib.fa_window_key_range(-1, 4, 0, 0, 0, 3, ctypes.byref(lo), ctypes.byref(hi)) == -1


def test_python_keyword(fa):
    import torch

    from flash_attention_metal_amd.ops import _window

    assert _window((63, 0), False) == (63, 0) and _window((-5, -9), False) == (-1, -1) and _window((INT_MAX, INT_MAX), False) == (INT_MAX, INT_MAX)
    assert _window((63, -1), True) == (63, 0) and _window((63, 0), True) == (63, 0) and _window([7, 0], True) == (7, 0)
    for bad, causal in (((63, 5), True), ((1, 2, 3), False), (5, False), ((1 << 31, 0), False), (("a", 0), False)):
        with pytest.raises(ValueError):
            _window(bad, causal)
    # the keyword reaches validation before anything touches a device: CPU tensors are refused as without it
    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16)
    k = torch.zeros(12, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 10], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa.flash_attention_varlen(q, k, k, cu, cu, 10, 12, window=(3, 0))
    kp = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16)
    bt, sl = torch.zeros(1, 3, dtype=torch.int32), torch.tensor([12], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa.flash_attention_varlen_paged(q, kp, kp.clone(), cu, bt, sl, 10, window=(3, 0))
    with pytest.raises(ValueError):
        fa.flash_attention_decode_paged(q[None, :, :1], kp, kp.clone(), bt, sl, window=(3, 0))  # CPU tensors
