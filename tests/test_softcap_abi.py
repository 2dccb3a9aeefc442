"""The soft-capping entry points without a GPU: the four symbols exported and bound with the header's argument lists, a cap of 0, below 0,
infinite or NaN refused, every argument rule of the matching *_window call refused identically (same status, same text behind the
function's name; fake aligned pointers as in tests/test_window_abi.py: no call here may pass validation), the Python keywords and the op."""
import ctypes
import os
import re

import pytest

import window as wn
from test_sink_abi import BWD_RULES, _bwd, _decode, _paged, _varlen
from test_window_abi import DECODE_RULES, PAGED_RULES, VARLEN_RULES

WINDOWS = ((63, 0), (-1, -1), (-1, 0), (wn.INT_MAX, wn.INT_MAX))
NAMES = ("fa_fwd_varlen_softcap", "fa_fwd_varlen_paged_softcap", "fa_fwd_decode_paged_softcap", "fa_bwd_varlen_softcap")
BAD_CAPS = (0.0, -1.0, -0.0, float("inf"), float("-inf"), float("nan"))


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
        # the matching *_window signature with `float softcap` added directly behind window_right
        old = SYMBOLS[name.replace("_softcap", "_window")][1]
        at = [i for i, a in enumerate(decl.split(",")) if "window_right" in a][0] + 1
        assert want[:at] + want[at + 1:] == old and want[at] is ctypes.c_float and "float softcap" in decl.split(",")[at], name
    for word in ("Logit soft-capping", "AFTER the cap", "softcap must be finite and", "tanh_err", "1 - t_ij^2", "BIT-IDENTICAL to the",
                 "The cap gets no gradient"):
        assert word in header, word
    assert fa.load_library().fa_version() == 400


ENTRIES = [("fa_fwd_varlen", _varlen, VARLEN_RULES), ("fa_fwd_varlen_paged", _paged, PAGED_RULES),
           ("fa_fwd_decode_paged", _decode, DECODE_RULES), ("fa_bwd_varlen", _bwd, BWD_RULES)]


@pytest.mark.parametrize("stem,call,rules", ENTRIES, ids=[e[0] for e in ENTRIES])
def test_bad_caps_refused_and_every_window_rule_inherited(fa, stem, call, rules):
    lib = fa.load_library()
    old, new = stem + "_window", stem + "_softcap"
    for win in WINDOWS:
        # valid but for the cap: nothing else is wrong with these calls' arguments up to the point where the cap is looked at
        for cap in BAD_CAPS:
            assert call(lib, new, win + (cap,)) == -1 and lib.fa_last_error().decode() == new + ": softcap must be finite and > 0", (win, cap)
    for kw in rules:
        for win in WINDOWS:
            want = call(lib, old, win, **kw)
            msg = lib.fa_last_error().decode()
            assert want in (-1, -2) and msg.startswith(old + ":"), (kw, want, msg)  # no call here passes validation
            for cap in (50.0, 0.25):
                got = call(lib, new, win + (cap,), **kw)
                assert got == want and lib.fa_last_error().decode() == new + msg[len(old):], (kw, win, got, lib.fa_last_error())


def test_python_keywords(fa):
    import torch

    from flash_attention_metal_amd.ops import _softcap

    assert _softcap(None, None) is None and _softcap(0.0, None) is None and _softcap(0, torch.zeros(4)) is None
    assert _softcap(50, None) == 50.0 and isinstance(_softcap(50, None), float)
    with pytest.raises(ValueError, match="sinks"):
        _softcap(50.0, torch.zeros(4))
    q = torch.zeros(10, 4, 64, dtype=torch.bfloat16)
    k = torch.zeros(12, 2, 64, dtype=torch.bfloat16)
    cu = torch.tensor([0, 10], dtype=torch.int32)
    s = torch.zeros(4)
    kp = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16)
    bt, sl = torch.zeros(1, 3, dtype=torch.int32), torch.tensor([12], dtype=torch.int32)
    # together with sinks: ValueError from all four wrappers, before anything else is looked at
    with pytest.raises(ValueError, match="sinks"):
        fa.flash_attention_varlen(q, k, k, cu, cu, 10, 12, sinks=s, softcap=50.0)
    with pytest.raises(ValueError, match="sinks"):
        fa.flash_attention_varlen_paged(q, kp, kp.clone(), cu, bt, sl, 10, sinks=s, softcap=50.0)
    with pytest.raises(ValueError, match="sinks"):
        fa.flash_attention_decode_paged(q[None, :, :1], kp, kp.clone(), bt, sl, sinks=s, softcap=50.0)
    with pytest.raises(ValueError, match="sinks"):
        fa.flash_attention_varlen_backward(q, k, k, q, q, torch.zeros(4, 10), cu, cu, 10, 12, sinks=s, softcap=50.0)
    # e4m3 pools in the prefill
    if hasattr(torch, "float8_e4m3fn"):
        kp8 = torch.zeros(6, 2, 16, 64, dtype=torch.float8_e4m3fn)
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            fa.flash_attention_varlen_paged(q, kp8, kp8.clone(), cu, bt, sl, 10, softcap=50.0)
    # the keyword reaches validation before anything touches a device: CPU tensors are refused as without it; None and 0.0 are today's path
    for cap in (50.0, None, 0.0):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fa.flash_attention_varlen(q, k, k, cu, cu, 10, 12, softcap=cap)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fa.flash_attention_varlen_paged(q, kp, kp.clone(), cu, bt, sl, 10, window=(3, 0), softcap=cap)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fa.flash_attention_varlen_backward(q, k, k, q, q, torch.zeros(4, 10), cu, cu, 10, 12, softcap=cap)
    with pytest.raises(ValueError):
        fa.flash_attention_decode_paged(q[None, :, :1], kp, kp.clone(), bt, sl, softcap=50.0)  # (as without the keyword: CPU tensors)


def test_the_op_is_defined_with_meta_shapes():
    import torch

    from flash_attention_metal_amd import torch_op

    qm = torch.empty(10, 8, 128, dtype=torch.float16, device="meta")
    km = torch.empty(12, 2, 128, dtype=torch.float16, device="meta")
    cum = torch.empty(3, dtype=torch.int32, device="meta")
    om, lm = torch.ops.fa_mi355.attention_varlen_softcap(qm, km, km, cum, cum, 10, 12, 4095, 0, 50.0, 0.0)
    assert om.shape == qm.shape and om.dtype == qm.dtype and lm.shape == (8, 10) and lm.dtype == torch.float32
    with pytest.raises(ValueError, match="sinks"):
        torch_op.attention_varlen(qm, km, km, cum, cum, 10, 12, sinks=torch.empty(8, device="meta"), softcap=50.0)
    om, _ = torch_op.attention_varlen(qm, km, km, cum, cum, 10, 12, is_causal=True, softcap=50.0)  # dispatches to the new op
    assert om.shape == qm.shape
