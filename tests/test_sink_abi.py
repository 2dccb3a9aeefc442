"""The attention-sink entry points without a GPU: the four symbols exported and bound with the header's argument lists, a NULL (or
misaligned) `sinks` refused, every argument rule of the matching *_window call refused identically (same status, same text behind the
function's name; fake aligned pointers as in tests/test_window_abi.py: no call here may pass validation), and the Python keywords."""
import ctypes
import os
import re

import pytest

import window as wn
from test_window_abi import BF16, DECODE_RULES, OK, OK4, P_, PAGED_RULES, VARLEN_RULES, _ptrs

WINDOWS = ((63, 0), (-1, -1), (-1, 0), (wn.INT_MAX, wn.INT_MAX))
NAMES = ("fa_fwd_varlen_sink", "fa_fwd_varlen_paged_sink", "fa_fwd_decode_paged_sink", "fa_bwd_varlen_sink")


@pytest.fixture(scope="module")
def fa():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    return fa


def test_symbols_exported_and_bound_as_the_header_declares_them(fa):
    from flash_attention_metal_amd._lib import SYMBOLS

    raw = ctypes.CDLL(fa.lib_path())
    header = open(os.path.join(os.path.dirname(fa.lib_path()), "..", "..", "include", "fa_mi355.h")).read()
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}
    for name in NAMES:
        assert hasattr(raw, name) and name in SYMBOLS, name
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S).group(1)
        want = [ctypes.c_void_p if "*" in a else ctype[a.strip().rsplit(" ", 1)[0]] for a in decl.replace("\n", " ").split(",")]
        assert SYMBOLS[name] == (ctypes.c_int, want), name
        # the matching *_window signature with `sinks` (the backward: and `dsinks`) added behind the window
        old = SYMBOLS[name.replace("_sink", "_window")][1]
        extra = 2 if name == "fa_bwd_varlen_sink" else 1
        at = [i for i, a in enumerate(decl.split(",")) if "window_right" in a][0] + 1
        assert want[:at] + want[at + extra:] == old and want[at:at + extra] == [ctypes.c_void_p] * extra, name
        assert re.search(r"const float \*sinks", decl) and ("float *dsinks" in decl) == (extra == 2)
    for word in ("Attention sinks", "NOT applied", "BIT-IDENTICAL to the *_window call", "LSE = sinks[h]", "ALWAYS run the window-mode kernels",
                 "0.2-6 %", "WRITTEN, not accumulated"):
        assert word in header, word
    assert fa.load_library().fa_version() == 400


def _varlen(lib, fn, mask, q=OK, k=OK, v=OK, o=OK, lse=None, cu_q=OK4, cu_k=OK4, B=3, Hq=8, Hkv=2, total_q=1000, total_k=1500, max_q=400,
            max_k=600, D=64, scale=0.125, q_rs=None, q_hs=None, kv_rs=None, kv_hs=None, dtype=BF16):
    q_rs, kv_rs = (Hq * D if q_rs is None else q_rs), (Hkv * D if kv_rs is None else kv_rs)
    return getattr(lib, fn)(*_ptrs(q, k, v, o, lse, cu_q, cu_k), B, Hq, Hkv, total_q, total_k, max_q, max_k, D, scale, q_rs,
                            D if q_hs is None else q_hs, kv_rs, D if kv_hs is None else kv_hs, *mask, dtype, None)


def _paged(lib, fn, mask, q=OK, k=OK, v=OK, o=OK, lse=None, cu=OK4, bt=OK4, sl=OK4, B=2, Hq=8, Hkv=2, total_q=300, max_q=200, D=64, P=16,
           num_pages=100, mp=8, scale=0.125, qrs=None, qhs=None, ps=None, hs=None, rs=None, bts=None, dt=BF16):
    qrs, qhs = (Hq * D if qrs is None else qrs), (D if qhs is None else qhs)
    ps, hs, rs = (Hkv * P * D if ps is None else ps), (P * D if hs is None else hs), (D if rs is None else rs)
    return getattr(lib, fn)(*_ptrs(q, k, v, o, lse, cu, bt, sl), B, Hq, Hkv, total_q, max_q, D, P, num_pages, mp, scale, qrs, qhs, ps, hs, rs,
                            mp if bts is None else bts, *mask, dt, None)


def _decode(lib, fn, mask, q=OK, k=OK, v=OK, o=OK, bt=OK4, sl=OK4, B=2, Hq=8, Hkv=2, Nq=1, D=64, P=16, num_pages=100, mp=8, scale=0.125,
            qbs=None, qhs=None, ps=None, hs=None, rs=None, bts=None, qdt=BF16, kvdt=BF16, ws=OK, wsb=0):
    qhs = Nq * D if qhs is None else qhs
    qbs = Hq * qhs if qbs is None else qbs
    ps, hs, rs = (Hkv * P * D if ps is None else ps), (P * D if hs is None else hs), (D if rs is None else rs)
    return getattr(lib, fn)(*_ptrs(q, k, v, o, None, bt, sl), B, Hq, Hkv, Nq, D, P, num_pages, mp, scale, qbs, qhs, ps, hs, rs,
                            mp if bts is None else bts, *mask, qdt, kvdt, None if ws is None else P_(ws), wsb, None)


BWD_PTRS = ("q", "k", "v", "o", "d_o", "lse", "dq", "dk", "dv", "ws", "cu_q", "cu_k")


def _bwd(lib, fn, mask, B=3, Hq=8, Hkv=2, total_q=1000, total_k=1500, max_q=400, max_k=600, D=64, scale=0.125, q_rs=None, q_hs=None,
         kv_rs=None, kv_hs=None, dtype=BF16, **p):
    q_rs, kv_rs = (Hq * D if q_rs is None else q_rs), (Hkv * D if kv_rs is None else kv_rs)
    return getattr(lib, fn)(*_ptrs(*[p.get(n, OK) for n in BWD_PTRS]), B, Hq, Hkv, total_q, total_k, max_q, max_k, D, scale, q_rs,
                            D if q_hs is None else q_hs, kv_rs, D if kv_hs is None else kv_hs, *mask, dtype, None)


BWD_RULES = ([{n: None} for n in BWD_PTRS] + [{n: 0} for n in ("B", "Hq", "Hkv", "total_q", "total_k", "max_q", "max_k", "D")] +
             [{"Hkv": 3}, {"scale": 0.0}, {"scale": float("nan")}, {"dtype": 0}, {"dtype": 3}, {"D": 96, "q_rs": 8 * 96, "kv_rs": 2 * 96},
              {"max_q": 1001}, {"max_k": 1501}, {"q_rs": 8 * 64 + 4}, {"q_hs": 56}, {"kv_hs": 68}, {"kv_rs": 32}] +
             [{n: OK + 8} for n in ("q", "k", "v", "o", "d_o", "dq", "dk", "dv")] +
             [{"cu_q": OK4 + 2}, {"cu_k": OK4 + 2}, {"lse": OK4 + 2}, {"ws": OK4 + 2},
              {"B": 65536, "Hq": 65536, "Hkv": 65536, "q_rs": 64, "q_hs": 64, "kv_rs": 64, "kv_hs": 64}])
ENTRIES = [("fa_fwd_varlen", _varlen, VARLEN_RULES, 1), ("fa_fwd_varlen_paged", _paged, PAGED_RULES, 1),
           ("fa_fwd_decode_paged", _decode, DECODE_RULES, 1), ("fa_bwd_varlen", _bwd, BWD_RULES, 2)]


@pytest.mark.parametrize("stem,call,rules,extra", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_null_sinks_refused_and_every_window_rule_inherited(fa, stem, call, rules, extra):
    lib = fa.load_library()
    old, new = stem + "_window", stem + "_sink"
    good = (P_(OK4),) * extra  # sinks (and dsinks): fake, fp32-aligned
    for win in WINDOWS:
        # valid but for the sinks: nothing else is wrong with these calls' arguments up to the point where sinks are looked at
        assert call(lib, new, win + (None,) + good[1:]) == -1 and lib.fa_last_error().decode() == new + ": null pointer", win
        assert call(lib, new, win + (P_(OK4 + 2),) + good[1:]) == -1 and "sinks must be fp32-aligned" in lib.fa_last_error().decode()
    if extra == 2:  # dsinks may be NULL, but not misaligned
        assert call(lib, new, (63, 0, P_(OK4), P_(OK4 + 2)), q=None) == -1 and lib.fa_last_error().decode() == new + ": null pointer"
        assert call(lib, new, (63, 0, P_(OK4), P_(OK4 + 2))) == -1 and "dsinks must be fp32-aligned" in lib.fa_last_error().decode()
    for kw in rules:
        for win in WINDOWS:
            want = call(lib, old, win, **kw)
            msg = lib.fa_last_error().decode()
            assert want in (-1, -2) and msg.startswith(old + ":"), (kw, want, msg)  # no call here passes validation
            for tail in (good, (good[0], None)[:extra]):
                got = call(lib, new, win + tail, **kw)
                assert got == want and lib.fa_last_error().decode() == new + msg[len(old):], (kw, win, got, lib.fa_last_error())


def test_python_keywords(fa):
    import torch

    from flash_attention_metal_amd.ops import _sink_window, _sinks

    assert _sink_window(None, True) == (-1, 0) and _sink_window(None, False) == (-1, -1)
    assert _sink_window((127, -1), True) == (127, 0) and _sink_window((64, 64), False) == (64, 64)
    with pytest.raises(ValueError):
        _sink_window((63, 5), True)
    for bad in (torch.zeros(3), torch.zeros(4, 1), [0.0] * 4, torch.zeros(4)):  # wrong length, rank, type; not on a device
        with pytest.raises(ValueError):
            _sinks(bad, 4, torch.device("cuda", 0))
    # the keyword reaches validation before anything touches a device: CPU tensors are refused as without it
    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16)
    k = torch.zeros(12, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 10], dtype=torch.int32)
    s = torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa.flash_attention_varlen(q, k, k, cu, cu, 10, 12, sinks=s)
    kp = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16)
    bt, sl = torch.zeros(1, 3, dtype=torch.int32), torch.tensor([12], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa.flash_attention_varlen_paged(q, kp, kp.clone(), cu, bt, sl, 10, window=(3, 0), sinks=s)
    with pytest.raises(ValueError):
        fa.flash_attention_decode_paged(q[None, :, :1], kp, kp.clone(), bt, sl, sinks=s)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa.flash_attention_varlen_backward(q, k, k, q, q, torch.zeros(4, 10), cu, cu, 10, 12, sinks=s)


def test_the_op_is_defined_with_meta_shapes():
    import torch

    from flash_attention_metal_amd import torch_op  # noqa: F401

    qm = torch.empty(10, 8, 128, dtype=torch.float16, device="meta")
    km = torch.empty(12, 2, 128, dtype=torch.float16, device="meta")
    cum = torch.empty(3, dtype=torch.int32, device="meta")
    sm = torch.empty(8, dtype=torch.bfloat16, device="meta")
    om, lm = torch.ops.fa_mi355.attention_varlen_sink(qm, km, km, sm, cum, cum, 10, 12, 127, 0, 0.0)
    assert om.shape == qm.shape and om.dtype == qm.dtype and lm.shape == (8, 10) and lm.dtype == torch.float32
