"""fa_fwd_varlen_paged_kv8 and fa_kv_append_paged_quant without a GPU (include/fa_mi355.h, "e4m3 pools in the prefill"): both symbols and
both support functions exported and bound with the header's argument lists; the support table; sinks == NULL accepted; every rule shared
with fa_fwd_varlen_paged_sink / fa_kv_append_paged refused with the identical status and text (both entry points driven with the same bad
argument; fake aligned pointers as in tests/test_window_abi.py: no call here may pass validation); what differs -- the dtype pair, the
16-element stride rule, a page counted in bytes of 1, the multipliers -- on its own; and the Python routing."""
import ctypes
import os
import re

import pytest

from test_sink_abi import _paged as _sink_call
from test_varlen_paged_abi import _append as _copy_append
from test_window_abi import BF16, F16, FP8, OK, OK4, P_, PAGED_RULES, _ptrs

INVALID, UNSUPPORTED = -1, -2
NEW, OLD = "fa_fwd_varlen_paged_kv8", "fa_fwd_varlen_paged_sink"
QUANT, COPY = "fa_kv_append_paged_quant", "fa_kv_append_paged"
WINDOWS = ((63, 0), (-1, -1), (-1, 0), (2 ** 31 - 1, 2 ** 31 - 1))
SINKS = P_(OK4)
BIG = dict(B=1 << 20, Hq=1 << 10, total_q=256, max_q=256)  # valid up to the last rule (the grid): where a call that is otherwise right ends


@pytest.fixture(scope="module")
def fa():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    return fa


def _kv8(lib, mask, q=OK, k=OK, v=OK, o=OK, lse=None, cu=OK4, bt=OK4, sl=OK4, B=2, Hq=8, Hkv=2, total_q=300, max_q=200, D=64, P=16,
         num_pages=100, mp=8, scale=0.125, qrs=None, qhs=None, ps=None, hs=None, rs=None, bts=None, qdt=BF16, kvdt=FP8):
    qrs, qhs = (Hq * D if qrs is None else qrs), (D if qhs is None else qhs)
    ps, hs, rs = (Hkv * P * D if ps is None else ps), (P * D if hs is None else hs), (D if rs is None else rs)
    return lib.fa_fwd_varlen_paged_kv8(*_ptrs(q, k, v, o, lse, cu, bt, sl), B, Hq, Hkv, total_q, max_q, D, P, num_pages, mp, scale, qrs, qhs, ps, hs,
                                       rs, mp if bts is None else bts, *mask, qdt, kvdt, None)


def _quant(lib, kn=OK, vn=OK, kp=OK, vp=OK, cu=OK4, bt=OK4, sl=OK4, B=2, Hkv=2, total=300, max_new=200, D=64, P=16, num_pages=100, mp=8,
           nrs=None, nhs=None, ps=None, hs=None, rs=None, bts=None, dt=BF16, k_mul=1.0, v_mul=1.0):
    nrs, nhs = (Hkv * D if nrs is None else nrs), (D if nhs is None else nhs)
    ps, hs, rs = (Hkv * P * D if ps is None else ps), (P * D if hs is None else hs), (D if rs is None else rs)
    return lib.fa_kv_append_paged_quant(*_ptrs(kn, vn, kp, vp, cu, bt, sl), B, Hkv, total, max_new, D, P, num_pages, mp, nrs, nhs, ps, hs, rs,
                                        mp if bts is None else bts, dt, k_mul, v_mul, None)


def test_symbols_exported_and_bound_as_the_header_declares_them(fa):
    from flash_attention_metal_amd._lib import SYMBOLS

    raw = ctypes.CDLL(fa.lib_path())
    header = open(os.path.join(os.path.dirname(fa.lib_path()), "..", "..", "include", "fa_mi355.h")).read()
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}
    want = {}
    for name in (NEW, NEW + "_supported", QUANT):
        assert hasattr(raw, name) and name in SYMBOLS, name
        decl = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S).group(1)
        want[name] = [ctypes.c_void_p if "*" in a else ctype[a.strip().rsplit(" ", 1)[0]] for a in decl.replace("\n", " ").split(",")]
        assert SYMBOLS[name] == (ctypes.c_int, want[name]), name
    # fa_fwd_varlen_paged_sink with `int dtype` replaced by `int q_dtype, int kv_dtype`; fa_kv_append_paged with `int dtype` replaced by
    # `int new_dtype` and the two multipliers added
    old = SYMBOLS[OLD][1]
    assert want[NEW] == old[:-2] + [ctypes.c_int, ctypes.c_int, ctypes.c_void_p] and old[-2:] == [ctypes.c_int, ctypes.c_void_p]
    assert want[QUANT] == SYMBOLS[COPY][1][:-1] + [ctypes.c_float, ctypes.c_float, ctypes.c_void_p]
    assert want[NEW + "_supported"] == [ctypes.c_int] * 4
    assert re.search(r"int q_dtype, int kv_dtype, void \*hip_stream\);", header) and "int new_dtype, float k_mul, float v_mul" in header
    for word in ("e4m3 pools in the prefill", "NO SCALES", "BIT-IDENTICAL to the bf16 call", "0x7F / 0xFF", "e4m3_rne(clamp(fp32(x) * mul, -448, 448))",
                 "the clamp FIRST", "-0 keeps its sign"):
        assert word in header, word
    assert fa.load_library().fa_version() == 400
    assert callable(fa.varlen_paged_kv8_supported)


def test_support_table(fa):
    lib = fa.load_library()
    sup = lib.fa_fwd_varlen_paged_kv8_supported
    for D in (64, 128):
        for P in (16, 32, 64, 128, 256):
            assert sup(BF16, FP8, D, P) == 1, (D, P)
            for pair in ((F16, FP8), (FP8, FP8), (BF16, BF16), (F16, F16), (0, FP8), (BF16, 0), (FP8, BF16)):
                assert sup(*pair, D, P) == 0, (pair, D, P)
        for P in (0, 8, 24, 48, 512, -16):
            assert sup(BF16, FP8, D, P) == 0, (D, P)
    for D in (0, 32, 96, 256):
        assert sup(BF16, FP8, D, 64) == 0, D
    # the un-quantised table does not move
    assert lib.fa_fwd_varlen_paged_supported(FP8, 64, 64) == 0 and lib.fa_fwd_varlen_paged_supported(BF16, 64, 64) == 1
    assert fa.varlen_paged_kv8_supported("bf16", "fp8_e4m3", 128, 16) and not fa.varlen_paged_kv8_supported("f16", "fp8_e4m3", 128, 16)
    assert not fa.varlen_paged_supported("fp8_e4m3", 64, 16)


def test_unsupported_pairs_and_the_paged_calls_stay_as_they_were(fa):
    lib = fa.load_library()
    for pair in ((F16, FP8), (FP8, FP8), (BF16, BF16)):
        assert _kv8(lib, (63, 0, SINKS), qdt=pair[0], kvdt=pair[1]) == UNSUPPORTED
        msg = lib.fa_last_error().decode()
        assert msg.startswith(NEW + ":") and "bf16 queries on an fp8_e4m3 pool" in msg, msg
    for kw in (dict(D=96), dict(P=8)):
        assert _kv8(lib, (63, 0, None), **kw) == UNSUPPORTED and lib.fa_last_error().decode().startswith(NEW + ":")
    assert _sink_call(lib, OLD, (63, 0, SINKS), dt=FP8, qrs=1024, rs=64) == UNSUPPORTED  # an e4m3 pool is still refused there
    assert "fa_fwd_decode_paged" in lib.fa_last_error().decode()


def test_null_sinks_are_accepted_and_misaligned_ones_refused(fa):
    lib = fa.load_library()
    for win in WINDOWS:
        for sinks in (None, SINKS):  # both get to the last rule
            assert _kv8(lib, win + (sinks,), **BIG) == INVALID and lib.fa_last_error().decode() == NEW + ": grid too large", (win, sinks)
        assert _kv8(lib, win + (P_(OK4 + 2),)) == INVALID and "sinks must be fp32-aligned" in lib.fa_last_error().decode()


def test_every_shared_rule_is_refused_as_the_sink_call_refuses_it(fa):
    lib = fa.load_library()
    checked = 0
    for kw in PAGED_RULES:
        if "dt" in kw or kw.get("rs") == 1 << 22:  # the dtype rules and the 2 GiB page (counted in bytes of 1 here): below
            continue
        for win in WINDOWS:
            want = _sink_call(lib, OLD, win + (SINKS,), **kw)
            msg = lib.fa_last_error().decode()
            assert want in (INVALID, UNSUPPORTED) and msg.startswith(OLD + ":"), (kw, want, msg)
            for sinks in (SINKS, None):
                got = _kv8(lib, win + (sinks,), **kw)
                new = lib.fa_last_error().decode()
                assert got == want and new.startswith(NEW + ":"), (kw, win, got, new)
                if want == INVALID:  # (the support rule names each call's own types: its status is shared, its text is not)
                    assert new == NEW + msg[len(OLD):], (kw, win, new, msg)
                checked += 1
    assert checked >= 8 * 45


def test_the_rules_that_differ(fa):
    lib = fa.load_library()

    def refused(word, **kw):
        assert _kv8(lib, (63, 0, None), **kw) == INVALID and word in lib.fa_last_error().decode(), (kw, lib.fa_last_error())

    # kv strides: multiples of 16 elements (8 k with k odd passes the 16-bit call's rule, not this one), at least D
    refused("page strides", rs=72, hs=16 * 72, ps=2 * 16 * 72)
    refused("page strides", hs=16 * 64 + 8)
    refused("page strides", ps=2 * 16 * 64 + 24)
    assert _sink_call(lib, OLD, (63, 0, SINKS), rs=72, hs=16 * 72, ps=2 * 16 * 72, **BIG) == INVALID and "grid" in lib.fa_last_error().decode()
    assert _kv8(lib, (63, 0, None), rs=80, hs=16 * 80, ps=2 * 16 * 80, **BIG) == INVALID and "grid" in lib.fa_last_error().decode()
    # q strides stay multiples of 8 (bf16)
    assert _kv8(lib, (63, 0, None), qrs=8 * 64 + 8, **BIG) == INVALID and "grid" in lib.fa_last_error().decode()
    refused("strides", qrs=8 * 64 + 4)
    # a page of one head below 2 GiB, in bytes of 1: 256 rows of 2^22 elements are 1 GiB here (2 GiB in the 16-bit call)
    assert _sink_call(lib, OLD, (63, 0, SINKS), P=256, rs=1 << 22, hs=1 << 22, ps=1 << 30) == INVALID and "2 GiB" in lib.fa_last_error().decode()
    assert _kv8(lib, (63, 0, None), P=256, rs=1 << 22, hs=1 << 22, ps=1 << 30, **BIG) == INVALID and "grid" in lib.fa_last_error().decode()
    refused("one page of one head exceeds 2 GiB", P=256, rs=1 << 23, hs=1 << 23, ps=1 << 31)


APPEND_RULES = (
    [{n: None} for n in ("kn", "vn", "kp", "vp", "cu", "bt", "sl")] + [{n: 0} for n in ("B", "Hkv", "total", "max_new", "D", "P", "num_pages", "mp")] +
    [{"P": 48}, {"P": 8}, {"dt": 0}, {"max_new": 301}, {"nrs": 100}, {"nhs": 8}, {"nrs": 32}, {"bts": 7}, {"rs": 100}, {"rs": 32}, {"hs": -1024}, {"ps": 8},
     {"bts": 1 << 31}, {"P": 256, "mp": (1 << 22) + 1}, {"kn": OK + 8}, {"vn": OK + 8}, {"kp": OK + 8}, {"vp": OK + 8}, {"cu": OK4 + 2},
     {"bt": OK4 + 2}, {"sl": OK4 + 1}, {"Hkv": 65536, "nrs": 65536 * 64}, {"B": 1 << 30, "total": 1 << 10, "max_new": 1 << 10}])


def test_every_shared_append_rule_is_refused_as_the_copy_refuses_it(fa):
    lib = fa.load_library()
    for kw in APPEND_RULES:
        want = _copy_append(lib, **kw)
        msg = lib.fa_last_error().decode()
        assert want in (INVALID, UNSUPPORTED) and msg.startswith(COPY + ":"), (kw, want, msg)
        for dt in ((BF16, F16) if "dt" not in kw else (None,)):
            got = _quant(lib, **(kw if dt is None else dict(kw, dt=dt)))
            new = lib.fa_last_error().decode()
            assert got == want and new.startswith(QUANT + ":"), (kw, got, new)
            if want == INVALID:
                assert new == QUANT + msg[len(COPY):], (kw, new, msg)


def test_the_append_rules_that_differ(fa):
    lib = fa.load_library()
    last = dict(B=1 << 30, total=1 << 10, max_new=1 << 10)  # valid up to the grid rule

    def refused(code, word, **kw):
        assert _quant(lib, **kw) == code and word in lib.fa_last_error().decode() and lib.fa_last_error().decode().startswith(QUANT + ":"), \
            (kw, lib.fa_last_error())

    refused(INVALID, "grid", **last)
    refused(INVALID, "grid", dt=F16, k_mul=0.25, v_mul=3.0, **last)
    refused(UNSUPPORTED, "new_dtype", dt=FP8)   # the new rows are 16-bit
    refused(UNSUPPORTED, "new_dtype", dt=0)
    refused(UNSUPPORTED, "16-byte", D=24, nrs=48, nhs=24, rs=32, hs=512, ps=1024)
    refused(INVALID, "page strides", rs=72, hs=16 * 72, ps=2 * 16 * 72)  # pool strides: multiples of 16
    refused(INVALID, "grid", nrs=2 * 64 + 8, **last)                     # new-row strides: multiples of 8
    refused(INVALID, "strides", nrs=2 * 64 + 4)
    refused(INVALID, "grid", P=256, rs=1 << 22, hs=1 << 22, ps=1 << 30, **last)  # 1 GiB in bytes of 1
    refused(INVALID, "2 GiB", P=256, rs=1 << 23, hs=1 << 23, ps=1 << 31)
    for bad in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
        refused(INVALID, "must be > 0 and finite", k_mul=bad)
        refused(INVALID, "must be > 0 and finite", v_mul=bad)


def test_python_routing(fa):
    import torch

    B, Hq, Hkv, D, P, total = 2, 4, 2, 64, 16, 40
    q = torch.zeros(total, Hq, D, dtype=torch.bfloat16)
    kp8 = torch.zeros(6, Hkv, P, D, dtype=torch.float8_e4m3fn)
    cu = torch.tensor([0, 10, 40], dtype=torch.int32)
    bt = torch.zeros(B, 3, dtype=torch.int32)
    sl = torch.tensor([10, 30], dtype=torch.int32)
    # bf16 q on e4m3 pools gets past the dtype check (and stops where every CPU tensor stops); every other mix keeps the ValueError
    for kw in (dict(), dict(window=(63, 0)), dict(sinks=torch.zeros(Hq)), dict(is_causal=True)):
        with pytest.raises((RuntimeError, ValueError), match="no CPU path|q's device"):
            fa.flash_attention_varlen_paged(q, kp8, kp8.clone(), cu, bt, sl, 30, **kw)
    for qq, pool in ((q.to(torch.float16), kp8), (q.to(torch.float8_e4m3fn), kp8), (q.float(), kp8), (q, kp8.to(torch.float16))):
        with pytest.raises(ValueError, match="unsupported / mixed dtypes"):
            fa.flash_attention_varlen_paged(qq, pool, pool.clone(), cu, bt, sl, 30)
    with pytest.raises(ValueError):
        fa.flash_attention_varlen_paged(q, kp8, kp8.to(torch.bfloat16), cu, bt, sl, 30)  # k and v pools of two types
    kn = torch.zeros(total, Hkv, D, dtype=torch.bfloat16)
    for rows in (kn, kn.to(torch.float16)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fa.kv_append_paged(rows, rows.clone(), kp8, kp8.clone(), cu, bt, sl, 30, k_mul=0.25, v_mul=3.0)
    with pytest.raises(ValueError, match="mixed dtypes"):
        fa.kv_append_paged(kn.float(), kn.float(), kp8, kp8.clone(), cu, bt, sl, 30)
    with pytest.raises(ValueError, match="mixed dtypes"):
        fa.kv_append_paged(kn, kn.to(torch.float16), kp8, kp8.clone(), cu, bt, sl, 30)
    kp = torch.zeros(6, Hkv, P, D, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="k_mul"):
        fa.kv_append_paged(kn, kn.clone(), kp, kp.clone(), cu, bt, sl, 30, k_mul=0.5)  # the byte copy has no multipliers
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa.kv_append_paged(kn, kn.clone(), kp, kp.clone(), cu, bt, sl, 30)
