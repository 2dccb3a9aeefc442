"""fa_fwd_varlen_paged_split, fa_fwd_varlen_paged_num_splits and fa_fwd_varlen_paged_split_workspace_bytes without a GPU
(include/fa_mi355.h, "Key split in the paged prefill"): the three symbols exported and bound with the header's argument lists; every rule
shared with fa_fwd_varlen_paged_sink refused with the identical status and text (both entry points driven with the same bad argument; fake
aligned pointers as in tests/test_window_abi.py: no call here may pass validation -- a call that is right ends at the grid rule, the last
one); sinks == NULL accepted; num_splits out of range; a workspace that is NULL, misaligned or one byte short at two splits; one split
with a NULL workspace accepted; the size function and the heuristic on hand-computed cases and their zeros; the Python ValueErrors."""
import ctypes
import os
import re

import pytest

import ksplit as ks
from test_sink_abi import _paged as _sink_call
from test_window_abi import BF16, F16, FP8, OK, OK4, P_, PAGED_RULES, _ptrs

INVALID, UNSUPPORTED = -1, -2
NEW, OLD = "fa_fwd_varlen_paged_split", "fa_fwd_varlen_paged_sink"
SPLITS, BYTES = "fa_fwd_varlen_paged_num_splits", "fa_fwd_varlen_paged_split_workspace_bytes"
WINDOWS = ((63, 0), (-1, -1), (-1, 0), (2 ** 31 - 1, 2 ** 31 - 1))
SINKS = P_(OK4)
BIG = dict(B=1 << 20, Hq=1 << 10, total_q=256, max_q=256)  # valid up to the last rule (the grid): where a call that is otherwise right ends


@pytest.fixture(scope="module")
def fa():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    return fa


def _split(lib, mask, S=2, ws=OK, wsb=1 << 40, q=OK, k=OK, v=OK, o=OK, lse=None, cu=OK4, bt=OK4, sl=OK4, B=2, Hq=8, Hkv=2, total_q=300, max_q=200,
           D=64, P=16, num_pages=100, mp=8, scale=0.125, qrs=None, qhs=None, ps=None, hs=None, rs=None, bts=None, dt=BF16):
    qrs, qhs = (Hq * D if qrs is None else qrs), (D if qhs is None else qhs)
    ps, hs, rs = (Hkv * P * D if ps is None else ps), (P * D if hs is None else hs), (D if rs is None else rs)
    return lib.fa_fwd_varlen_paged_split(*_ptrs(q, k, v, o, lse, cu, bt, sl), B, Hq, Hkv, total_q, max_q, D, P, num_pages, mp, scale, qrs, qhs, ps, hs,
                                         rs, mp if bts is None else bts, *mask, dt, S, None if ws is None else P_(ws), wsb, None)


def test_symbols_exported_and_bound_as_the_header_declares_them(fa):
    from flash_attention_metal_amd._lib import SYMBOLS

    raw = ctypes.CDLL(fa.lib_path())
    header = open(os.path.join(os.path.dirname(fa.lib_path()), "..", "..", "include", "fa_mi355.h")).read()
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "long long": ctypes.c_longlong}
    want = {}
    for name, ret in ((NEW, "int"), (SPLITS, "int"), (BYTES, "long long")):
        assert hasattr(raw, name) and name in SYMBOLS, name
        decl = re.search(r"^" + ret + " " + name + r"\(([^;]*)\);", header, re.M | re.S).group(1)
        want[name] = [ctypes.c_void_p if "*" in a else ctype[a.strip().rsplit(" ", 1)[0]] for a in decl.replace("\n", " ").split(",")]
        assert SYMBOLS[name] == (ctype[ret], want[name]), name
    # fa_fwd_varlen_paged_sink's list up to and including `const float *sinks, int dtype`, then the three new arguments and the stream
    old = SYMBOLS[OLD][1]
    assert want[NEW] == old[:-1] + [ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p] and old[-2:] == [ctypes.c_int, ctypes.c_void_p]
    assert want[SPLITS] == [ctypes.c_int] * 6 and want[BYTES] == [ctypes.c_int] * 8
    assert int(re.search(r"#define FA_VARLEN_PAGED_MAX_SPLITS (\d+)", header).group(1)) == ks.MAX_SPLITS
    for word in ("Key split in the paged prefill", "tb + floor(s * n / S) .. tb + floor((s + 1) * n / S) - 1", "lse2_s = m + log2 l",
                 "skipped, never multiplied", "2 (S + 3) 2^-24 sum_j P_ij |v_jd|", "BIT-IDENTICAL to the S = 1 call"):
        assert word in header, word
    assert callable(fa.varlen_paged_num_splits) and callable(fa.varlen_paged_split_workspace_bytes)


def test_every_shared_rule_is_refused_as_the_sink_call_refuses_it(fa):
    lib = fa.load_library()
    checked = 0
    for kw in PAGED_RULES:
        for win in WINDOWS:
            want = _sink_call(lib, OLD, win + (SINKS,), **kw)
            msg = lib.fa_last_error().decode()
            assert want in (INVALID, UNSUPPORTED) and msg.startswith(OLD + ":"), (kw, want, msg)
            for sinks in (SINKS, None):
                for S, ws in ((2, OK), (1, None), (0, OK)):
                    got = _split(lib, win + (sinks,), S=S, ws=ws, **kw)
                    new = lib.fa_last_error().decode()
                    assert got == want and new == NEW + msg[len(OLD):], (kw, win, S, got, new, msg)
                    checked += 1
    assert checked >= 6 * 4 * 45


def test_null_sinks_and_one_split_without_a_workspace_are_accepted(fa):
    lib = fa.load_library()
    for win in WINDOWS:
        for sinks in (None, SINKS):  # all get to the last rule
            for S, ws, wsb in ((1, None, 0), (2, OK, 1 << 40), (0, OK, 1 << 40), (ks.MAX_SPLITS, OK, 1 << 40)):
                assert _split(lib, win + (sinks,), S=S, ws=ws, wsb=wsb, **BIG) == INVALID and lib.fa_last_error().decode() == NEW + ": grid too large", \
                    (win, sinks, S)
        assert _split(lib, win + (P_(OK4 + 2),)) == INVALID and "sinks must be fp32-aligned" in lib.fa_last_error().decode()


def test_num_splits_and_the_workspace_rules(fa):
    lib = fa.load_library()

    def refused(word, **kw):
        assert _split(lib, (63, 0, None), **kw) == INVALID, kw
        msg = lib.fa_last_error().decode()
        assert msg.startswith(NEW + ":") and word in msg, (kw, msg)

    refused("num_splits=-1", S=-1)
    refused(f"num_splits={ks.MAX_SPLITS + 1}", S=ks.MAX_SPLITS + 1)
    need = lib.fa_fwd_varlen_paged_split_workspace_bytes(2, 8, 300, 200, 64, 16, 8, 2)
    assert need == ks.workspace_bytes(2, 8, 300, 64) == 2 * 8 * 300 * 65 * 4
    refused("null pointer", S=2, ws=None)
    refused("workspace must be 16-byte aligned", S=2, ws=OK + 8)
    refused(f"workspace of {need - 1} bytes, fa_fwd_varlen_paged_split_workspace_bytes() asks for {need}", S=2, wsb=need - 1)
    # num_splits = 0 resolves through the heuristic: 2 sequences x 8 heads x 2 blocks against 512 slots asks for 16, the capacity of
    # 8 pages x 16 keys = 2 tiles allows 1 -- one split, no workspace asked for
    assert lib.fa_fwd_varlen_paged_num_splits(2, 8, 200, 64, 16, 8) == 1
    assert _split(lib, (63, 0, None), S=0, ws=None, wsb=0, **BIG) == INVALID and "grid" in lib.fa_last_error().decode()
    # ... and with 1024 pages it is 16: the workspace is wanted
    assert lib.fa_fwd_varlen_paged_num_splits(2, 8, 200, 64, 16, 1024) == 16
    refused("null pointer", S=0, ws=None, mp=1024)
    need0 = lib.fa_fwd_varlen_paged_split_workspace_bytes(2, 8, 300, 200, 64, 16, 1024, 0)
    assert need0 == ks.workspace_bytes(16, 8, 300, 64)
    refused(f"asks for {need0}", S=0, mp=1024, wsb=need0 - 1)


def test_the_heuristic_and_the_size_function(fa):
    lib = fa.load_library()
    n, b = lib.fa_fwd_varlen_paged_num_splits, lib.fa_fwd_varlen_paged_split_workspace_bytes
    # blocks = B Hq ceil(max_q / 128); slots = 256 x 2 at both head dims; smallest S with blocks S >= slots; a full-capacity split keeps 4 tiles
    assert n(1, 8, 512, 128, 16, 8192) == 16      # 32 blocks, 512 slots
    assert n(1, 8, 512, 64, 16, 8192) == 16       # the same at head_dim 64
    assert n(1, 8, 8, 128, 16, 8192) == 64        # 8 blocks: 64 fill the chip, and MAX is 64
    assert n(1, 1, 8, 64, 16, 8192) == 64         # 512 wanted, capped by FA_VARLEN_PAGED_MAX_SPLITS
    assert n(16, 32, 512, 128, 16, 8192) == 1     # 2048 blocks >= slots: the un-split kernel
    assert n(4, 8, 512, 128, 16, 8192) == 4
    assert n(1, 8, 512, 128, 16, 64) == 4         # 1024 keys = 16 tiles: at most 4 splits of 4 tiles
    assert n(1, 8, 512, 128, 256, 1) == 1         # 4 tiles
    assert n(1, 7, 129, 64, 64, 1000) == 37       # 14 blocks: ceil(512 / 14)
    for args in ((1, 8, 512, 128, 16, 8192), (3, 5, 77, 64, 32, 100), (16, 32, 512, 128, 16, 8192), (1, 7, 129, 64, 64, 1000)):
        assert n(*args) == ks.num_splits(*args), args
    for bad in ((0, 8, 512, 128, 16, 64), (1, 0, 512, 128, 16, 64), (1, 8, 0, 128, 16, 64), (1, 8, 512, 96, 16, 64), (1, 8, 512, 128, 24, 64),
                (1, 8, 512, 128, 16, 0), (1, 8, 512, 128, 256, (1 << 22) + 1), (1 << 20, 1 << 10, 256, 128, 16, 64), (-1, 8, 512, 128, 16, 64)):
        assert n(*bad) == 0, bad
        assert b(bad[0], bad[1], max(bad[2], 1) * 2, bad[2], *bad[3:], 2) == 0, bad
    # S * Hq * total_q * (D + 1) floats, rounded up to 16 bytes; 0 for one split, a bad count, total_q < max_seqlen_q
    assert b(1, 8, 512, 512, 128, 16, 8192, 16) == 16 * 8 * 512 * 129 * 4 == b(1, 8, 512, 512, 128, 16, 8192, 0)
    assert b(1, 1, 3, 3, 64, 16, 64, 3) == (3 * 1 * 3 * 65 * 4 + 15) // 16 * 16 == 2352
    assert b(1, 8, 512, 512, 128, 16, 8192, 1) == 0 and b(16, 32, 8192, 512, 128, 16, 8192, 0) == 0
    assert b(1, 8, 512, 512, 128, 16, 8192, -1) == 0 and b(1, 8, 512, 512, 128, 16, 8192, ks.MAX_SPLITS + 1) == 0
    assert b(1, 8, 100, 512, 128, 16, 8192, 4) == 0 and b(1, 8, 0, 512, 128, 16, 8192, 4) == 0
    # any int is a legal argument: nothing wraps at the top of the range (64-bit arithmetic), and a size no long long holds is 0
    assert n(1, 1, 2 ** 31 - 1, 128, 16, 8192) == 1 and n(2 ** 31 - 1, 1, 1, 64, 16, 8192) == 1 and n(1, 2 ** 31 - 1, 2 ** 31 - 1, 64, 16, 8192) == 0
    assert b(1, 2 ** 31 - 1, 2 ** 31 - 1, 1, 128, 16, 8192, 64) == 0
    assert b(1, 2 ** 20, 2 ** 20, 1, 128, 16, 8192, 64) == 64 * 2 ** 40 * 129 * 4
    assert fa.varlen_paged_num_splits(1, 8, 512, 128, 16, 8192) == 16
    assert fa.varlen_paged_split_workspace_bytes(1, 8, 512, 512, 128, 16, 8192) == 16 * 8 * 512 * 129 * 4


def test_python_routing_and_errors(fa):
    import torch

    B, Hq, Hkv, D, P, total = 2, 4, 2, 64, 16, 40
    q = torch.zeros(total, Hq, D, dtype=torch.bfloat16)
    kp = torch.zeros(6, Hkv, P, D, dtype=torch.bfloat16)
    cu = torch.tensor([0, 10, 40], dtype=torch.int32)
    bt = torch.zeros(B, 3, dtype=torch.int32)
    sl = torch.tensor([10, 30], dtype=torch.int32)

    def call(**kw):
        return fa.flash_attention_varlen_paged(q, kp, kp.clone(), cu, bt, sl, 30, **kw)

    for bad in (-1, 2.0, "2", True):
        with pytest.raises(ValueError, match="num_splits"):
            call(num_splits=bad)
    with pytest.raises(ValueError, match="softcap"):
        call(num_splits=2, softcap=30.0)
    with pytest.raises(ValueError, match="softcap"):
        call(num_splits=0, softcap=30.0, window=(63, 0))
    kp8 = torch.zeros(6, Hkv, P, D, dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        fa.flash_attention_varlen_paged(q, kp8, kp8.clone(), cu, bt, sl, 30, num_splits=2)
    # a call that is right stops where every CPU tensor stops, with or without the new keywords
    for kw in (dict(num_splits=0), dict(num_splits=2, sinks=torch.zeros(Hq)), dict(num_splits=1, window=(63, 0)), dict()):
        with pytest.raises((RuntimeError, ValueError), match="no CPU path|q's device"):
            call(**kw)
