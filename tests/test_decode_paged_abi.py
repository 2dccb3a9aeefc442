"""fa_fwd_decode_paged without a GPU: the entry points are exported and bound, the support table and the workspace size answer as the
header says, every bad argument is refused before any launch (fake aligned pointers, as test_abi.py does: no call here may pass
validation), and the paged decode kernels -- compiled with the Makefile's flags -- use no scratch and keep the M0 convention of every
LDS-DMA statement (test_isa_audit.py::test_lds_dma_statements_own_m0, restated for csrc/fa_decode_kernel.hip)."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "flash_attention_metal_amd", "csrc", "fa_decode_kernel.hip")
F16, BF16, FP8 = 1, 2, 3


@pytest.fixture(scope="module")
def fa():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    return fa


def test_paged_symbols_exported_and_bound(fa):
    from flash_attention_metal_amd._lib import SYMBOLS

    lib = ctypes.CDLL(fa.lib_path())
    for n in ("fa_fwd_decode_paged", "fa_fwd_decode_paged_workspace_bytes", "fa_fwd_decode_paged_supported"):
        assert hasattr(lib, n) and n in SYMBOLS, n
    assert len(SYMBOLS["fa_fwd_decode_paged"][1]) == 28
    assert callable(fa.flash_attention_decode_paged) and callable(fa.decode_paged_workspace_bytes)


def test_paged_support_table(fa):
    sup = fa.load_library().fa_fwd_decode_paged_supported
    for D in (64, 128):
        for P in (16, 32, 64, 128, 256):
            for q, kv in ((F16, F16), (BF16, BF16), (FP8, FP8), (BF16, FP8)):
                assert sup(q, kv, D, 32, 8, 1, P) == 1, (q, kv, D, P)
                assert sup(q, kv, D, 8, 1, 4, P) == 1  # 32 packed rows
                assert sup(q, kv, D, 8, 1, 5, P) == 0  # 40
                assert sup(q, kv, D, 32, 32, 33, P) == 0
    for P in (8, 48, 512, 0, 24, 1024):
        assert sup(BF16, BF16, 64, 32, 8, 1, P) == 0, P
    for D in (32, 96, 256):
        assert sup(BF16, BF16, D, 32, 8, 1, 64) == 0, D
    for q, kv in ((F16, FP8), (FP8, BF16), (F16, BF16), (BF16, F16), (0, 0), (FP8, F16)):
        assert sup(q, kv, 64, 32, 8, 1, 64) == 0, (q, kv)
    assert sup(BF16, BF16, 64, 6, 4, 1, 64) == 0  # Hq % Hkv


def test_paged_workspace_is_the_dense_decode_at_capacity(fa):
    lib = fa.load_library()
    for (B, Hq, Hkv, Nq, D, P, mp) in ((1, 32, 32, 1, 64, 16, 1024), (16, 32, 8, 1, 128, 64, 128), (3, 8, 2, 4, 64, 256, 3),
                                       (2, 4, 4, 16, 128, 32, 7), (1, 8, 1, 1, 64, 16, 1)):
        got = lib.fa_fwd_decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, P, mp)
        assert got > 0 and got == lib.fa_fwd_decode_workspace_bytes(B, Hq, Hkv, Nq, P * mp, D), (B, Hq, Hkv, Nq, D, P, mp)
        assert fa.decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, P, mp) == got
    assert lib.fa_fwd_decode_paged_workspace_bytes(1, 8, 8, 1, 64, 16, 0) == 0
    assert lib.fa_fwd_decode_paged_workspace_bytes(1, 8, 8, 1, 96, 16, 4) == 0


def test_paged_bad_arguments_are_rejected_before_launch(fa):
    lib = fa.load_library()
    P_ = ctypes.c_void_p
    ok, ok4 = P_(0x10000), P_(0x20000)

    def call(q=ok, k=ok, v=ok, o=ok, bt=ok4, sl=ok4, B=2, Hq=8, Hkv=2, Nq=1, D=64, P=16, num_pages=100, mp=8, scale=0.125,
             qbs=None, qhs=None, ps=None, hs=None, rs=None, bts=None, causal=0, qdt=BF16, kvdt=BF16, ws=ok, wsb=None):
        qhs = Nq * D if qhs is None else qhs
        qbs = Hq * qhs if qbs is None else qbs
        ps, hs, rs = (Hkv * P * D if ps is None else ps), (P * D if hs is None else hs), (D if rs is None else rs)  # HND
        bts = mp if bts is None else bts
        if wsb is None:
            wsb = max(lib.fa_fwd_decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, P, mp), 1 << 20)
        return lib.fa_fwd_decode_paged(q, k, v, o, None, bt, sl, B, Hq, Hkv, Nq, D, P, num_pages, mp, scale, qbs, qhs, ps, hs, rs, bts,
                                       causal, qdt, kvdt, ws, wsb, None)

    def err():
        return lib.fa_last_error().decode()

    # pointers and sizes
    for kw in ({"q": None}, {"k": None}, {"v": None}, {"o": None}, {"bt": None}, {"sl": None}, {"ws": None}):
        assert call(wsb=0, **kw) == -1 and "null" in err(), kw
    for kw in ({"B": 0}, {"Hq": 0}, {"Nq": 0}, {"num_pages": 0}, {"mp": 0}, {"P": 0}):
        assert call(wsb=0, **kw) == -1, kw
    assert call(Hq=6, Hkv=4, wsb=0) == -1 and "Hkv" in err()
    assert call(scale=0.0, wsb=0) == -1 and "scale" in err()
    # unsupported combinations (checked before strides, alignment and the workspace: the short workspace does not mask them)
    for P in (8, 48, 512):
        assert call(P=P, wsb=0) == -2 and "page" in err(), P
    assert call(D=96, wsb=0) == -2
    assert call(qdt=F16, kvdt=FP8, wsb=0) == -2 and "f16" in err()
    assert call(qdt=FP8, kvdt=BF16, wsb=0) == -2
    assert call(Hq=64, Hkv=1, wsb=0) == -2  # 64 packed rows
    # the table stride, strides, alignment
    assert call(bts=7, wsb=0) == -1 and "block_table_stride" in err()
    assert call(rs=100, wsb=0) == -1 and "stride" in err()
    assert call(rs=32, wsb=0) == -1  # a row shorter than D
    assert call(hs=-1024, wsb=0) == -1
    assert call(qhs=8, wsb=0) == -1
    assert call(qdt=BF16, kvdt=FP8, rs=72, hs=16 * 72, ps=2 * 16 * 72, wsb=0) == -1  # e4m3 strides are multiples of 16 elements
    assert call(q=P_(0x10008), wsb=0) == -1 and "aligned" in err()
    assert call(k=P_(0x10004), wsb=0) == -1 and "aligned" in err()
    assert call(bt=P_(0x20002), wsb=0) == -1 and "int32" in err()
    assert call(P=256, rs=1 << 22, hs=1 << 22, ps=1 << 30, wsb=0) == -1 and "2 GiB" in err()
    # a short workspace
    need = lib.fa_fwd_decode_paged_workspace_bytes(2, 8, 2, 1, 64, 16, 8)
    assert call(wsb=need - 1) == -1 and "workspace" in err()
    assert call(qdt=FP8, kvdt=FP8, wsb=need - 16) == -1 and "workspace" in err()


def _makefile_flags():
    text = open(os.path.join(ROOT, "flash_attention_metal_amd", "csrc", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    own = re.search(r"^FLAGS_fa_decode_kernel\s*:=\s*(.*)$", text, re.M)
    return cxx + (own.group(1).split() if own else [])


@pytest.fixture(scope="module")
def decode_isa():
    """(ISA text, resource-usage remarks) of csrc/fa_decode_kernel.hip, compiled with the Makefile's flags."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc] + _makefile_flags() + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", SRC,
                                                          "-o", os.path.join(tmp, "k.s")], cwd=tmp, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(os.path.join(tmp, "k.s")).read(), r.stderr


def test_paged_kernels_use_no_scratch(decode_isa):
    _, remarks = decode_isa
    rows = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", remarks, re.S)
    paged = {n: int(sc) for n, sc in rows if "DecodePagedParams" in n or ("decode_combine_kernel" in n and "ELb1E" in n)}
    # {f16, bf16, e4m3 / bf16 on e4m3} x {64, 128} x {16, 32 packed rows} x {causal, full} partial kernels + {f16, bf16} x 4 combines
    assert len([n for n in paged if "partial" in n]) == 24 and len(paged) == 32, sorted(paged)
    assert all(sc == 0 for sc in paged.values()), paged


def test_decode_lds_dma_statements_own_m0(decode_isa):
    # as test_isa_audit.py::test_lds_dma_statements_own_m0: every `buffer_load ... lds` is preceded, inside its own asm block, by the
    # s_mov_b32 m0 that belongs to it, and M0 appears nowhere outside such blocks -- for the dense and the paged decode kernels
    text, _ = decode_isa
    in_asm, own_m0, dma = False, False, 0
    for ln, t in enumerate(text.splitlines(), 1):
        u = t.strip()
        if u.startswith(";;#ASMSTART"):
            in_asm, own_m0 = True, False
        elif u.startswith(";;#ASMEND"):
            in_asm = False
        elif u and not u.startswith((";", ".")):
            if "m0" in u.replace(",", " ").split():
                assert in_asm, (ln, u, "M0 touched outside an asm block")
                if u.startswith("s_mov_b32 m0"):
                    own_m0 = True
            if u.startswith("buffer_load") and u.endswith(" lds"):
                assert in_asm and own_m0, (ln, u, "LDS-DMA without its own M0 write in the same statement")
                dma += 1
    assert dma > 0
