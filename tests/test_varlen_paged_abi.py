"""fa_fwd_varlen_paged and fa_kv_append_paged without a GPU: the entry points are exported and bound, the support table answers as the
header says, every bad argument is refused before any launch with its own message (fake aligned pointers, as test_abi.py does: no call
here may pass validation), and the Python wrappers refuse bad tensors with a ValueError before they touch the library."""
import ctypes
import os

import pytest

F16, BF16, FP8 = 1, 2, 3
INVALID, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def fa():
    import flash_attention_metal_amd as fa

    if not os.path.exists(fa.lib_path()):
        fa.build_library()
    return fa


def test_symbols_exported_and_bound(fa):
    from flash_attention_metal_amd._lib import SYMBOLS

    lib = ctypes.CDLL(fa.lib_path())
    for n in ("fa_fwd_varlen_paged", "fa_fwd_varlen_paged_supported", "fa_kv_append_paged"):
        assert hasattr(lib, n) and n in SYMBOLS, n
    assert len(SYMBOLS["fa_fwd_varlen_paged"][1]) == 27
    assert len(SYMBOLS["fa_kv_append_paged"][1]) == 23
    assert callable(fa.flash_attention_varlen_paged) and callable(fa.kv_append_paged) and callable(fa.varlen_paged_supported)
    assert fa.load_library().fa_version() == 400


def test_support_table(fa):
    sup = fa.load_library().fa_fwd_varlen_paged_supported
    for dt in (F16, BF16):
        for D in (64, 128):
            for P in (16, 32, 64, 128, 256):
                assert sup(dt, D, P) == 1, (dt, D, P)
            for P in (0, 8, 24, 48, 512, 1024, -16):
                assert sup(dt, D, P) == 0, (dt, D, P)
        for D in (32, 96, 256, 0):
            assert sup(dt, D, 64) == 0, (dt, D)
    for D in (64, 128):
        assert sup(FP8, D, 64) == 0 and sup(0, D, 64) == 0  # an e4m3 pool is the paged decode's; f32 has no matrix-core kernel
    assert fa.varlen_paged_supported("bf16", 64, 16) and not fa.varlen_paged_supported("fp8_e4m3", 64, 16)
    assert not fa.varlen_paged_supported("f16", 128, 48)


def _ptr(x):
    return ctypes.c_void_p(x)


OK, OK4 = 0x10000, 0x20000


def _attend(lib, q=OK, k=OK, v=OK, o=OK, lse=None, cu=OK4, bt=OK4, sl=OK4, B=2, Hq=8, Hkv=2, total_q=300, max_q=200, D=64, P=16,
            num_pages=100, mp=8, scale=0.125, qrs=None, qhs=None, ps=None, hs=None, rs=None, bts=None, causal=1, dt=BF16):
    qrs, qhs = (Hq * D if qrs is None else qrs), (D if qhs is None else qhs)
    ps, hs, rs = (Hkv * P * D if ps is None else ps), (P * D if hs is None else hs), (D if rs is None else rs)  # HND
    bts = mp if bts is None else bts
    p = [None if x is None else _ptr(x) for x in (q, k, v, o, lse, cu, bt, sl)]
    return lib.fa_fwd_varlen_paged(*p, B, Hq, Hkv, total_q, max_q, D, P, num_pages, mp, scale, qrs, qhs, ps, hs, rs, bts, causal, dt, None)


def _append(lib, kn=OK, vn=OK, kp=OK, vp=OK, cu=OK4, bt=OK4, sl=OK4, B=2, Hkv=2, total=300, max_new=200, D=64, P=16, num_pages=100, mp=8,
            nrs=None, nhs=None, ps=None, hs=None, rs=None, bts=None, dt=BF16):
    nrs, nhs = (Hkv * D if nrs is None else nrs), (D if nhs is None else nhs)
    ps, hs, rs = (Hkv * P * D if ps is None else ps), (P * D if hs is None else hs), (D if rs is None else rs)
    bts = mp if bts is None else bts
    p = [None if x is None else _ptr(x) for x in (kn, vn, kp, vp, cu, bt, sl)]
    return lib.fa_kv_append_paged(*p, B, Hkv, total, max_new, D, P, num_pages, mp, nrs, nhs, ps, hs, rs, bts, dt, None)


def test_attention_bad_arguments_are_rejected_before_launch(fa):
    lib = fa.load_library()

    def err():
        return lib.fa_last_error().decode()

    def refused(code, word, **kw):
        assert _attend(lib, **kw) == code, (kw, err())
        assert word in err() and err().startswith("fa_fwd_varlen_paged:"), (kw, err())

    # pointers (lse may be NULL: the default above passes none and is refused for another reason only)
    for name in ("q", "k", "v", "o", "cu", "bt", "sl"):
        refused(INVALID, "null", **{name: None})
    # sizes
    for name in ("B", "Hq", "Hkv", "total_q", "max_q", "D", "P", "num_pages", "mp"):
        refused(INVALID, "sizes", **{name: 0})
    refused(INVALID, "Hkv", Hq=6, Hkv=4)
    refused(INVALID, "scale", scale=0.0)
    refused(INVALID, "scale", scale=-1.0)
    # unsupported combinations
    for P in (8, 48, 512):
        refused(UNSUPPORTED, "page size", P=P)
    for D in (32, 96, 256):
        refused(UNSUPPORTED, "D =", D=D)
    refused(UNSUPPORTED, "e4m3", dt=FP8, qrs=1024, rs=64)
    refused(UNSUPPORTED, "f16", dt=0)
    # max_seqlen_q > total_q
    refused(INVALID, "max_seqlen_q", max_q=301)
    # q strides
    refused(INVALID, "strides", qrs=100)   # not a multiple of 8
    refused(INVALID, "strides", qrs=32)    # a row shorter than D
    refused(INVALID, "strides", qhs=8)
    refused(INVALID, "strides", qhs=-64)
    # the table stride, page strides, 2 GiB per page of one head, the capacity
    refused(INVALID, "block_table_stride", bts=7)
    refused(INVALID, "page strides", rs=100)
    refused(INVALID, "page strides", rs=32)
    refused(INVALID, "page strides", hs=-1024)
    refused(INVALID, "page strides", ps=8)
    refused(INVALID, "page strides", bts=1 << 31)
    refused(INVALID, "2 GiB", P=256, rs=1 << 22, hs=1 << 22, ps=1 << 30)
    refused(INVALID, "2^30", P=256, mp=(1 << 22) + 1)
    # alignment
    for name in ("q", "k", "v", "o"):
        refused(INVALID, "16-byte aligned", **{name: OK + 8})
    refused(INVALID, "int32", bt=OK4 + 2)
    refused(INVALID, "int32", sl=OK4 + 1)
    refused(INVALID, "int32", cu=OK4 + 2)
    # (max_seqlen_q + 128) * q_row_stride * 2 < 4 GiB
    refused(INVALID, "4 GiB", total_q=1 << 20, max_q=1 << 20, qrs=2048)
    # B * Hq * ceil(max_seqlen_q / 128) fits an int
    refused(INVALID, "grid", B=1 << 20, Hq=1 << 10, total_q=256, max_q=256)
    # lse may be NULL: every call above passed none and was refused for its own reason, never for a null pointer; with one, the same
    refused(INVALID, "grid", lse=OK, B=1 << 20, Hq=1 << 10, total_q=256, max_q=256)


def test_append_bad_arguments_are_rejected_before_launch(fa):
    lib = fa.load_library()

    def err():
        return lib.fa_last_error().decode()

    def refused(code, word, **kw):
        assert _append(lib, **kw) == code, (kw, err())
        assert word in err() and err().startswith("fa_kv_append_paged:"), (kw, err())

    for name in ("kn", "vn", "kp", "vp", "cu", "bt", "sl"):
        refused(INVALID, "null", **{name: None})
    for name in ("B", "Hkv", "total", "max_new", "D", "P", "num_pages", "mp"):
        refused(INVALID, "sizes", **{name: 0})
    refused(UNSUPPORTED, "f16", dt=0)
    refused(UNSUPPORTED, "page size", P=48)
    refused(UNSUPPORTED, "16-byte", D=24, dt=FP8, nrs=64, nhs=32, rs=32, hs=512, ps=1024)  # 24 bytes per row
    refused(INVALID, "max_seqlen_new", max_new=301)
    refused(INVALID, "strides", nrs=100)
    refused(INVALID, "strides", nhs=8)
    refused(INVALID, "strides", dt=FP8, nrs=136)  # e4m3 strides are multiples of 16 elements
    refused(INVALID, "block_table_stride", bts=7)
    refused(INVALID, "page strides", rs=100)
    refused(INVALID, "page strides", dt=FP8, rs=72, hs=16 * 72, ps=2 * 16 * 72)
    refused(INVALID, "2 GiB", P=256, rs=1 << 22, hs=1 << 22, ps=1 << 30)
    refused(INVALID, "2^30", P=256, mp=(1 << 22) + 1)
    for name in ("kn", "vn", "kp", "vp"):
        refused(INVALID, "16-byte aligned", **{name: OK + 8})
    refused(INVALID, "int32", cu=OK4 + 2)
    refused(INVALID, "int32", bt=OK4 + 2)
    refused(INVALID, "grid", Hkv=65536, nrs=65536 * 64)
    refused(INVALID, "grid", B=1 << 30, total=1 << 10, max_new=1 << 10)
    # all three types and any head dim with whole 16-byte chunks are supported (a byte copy): they get past the support check and are
    # refused by the last rule only (no call here may pass validation)
    for dt in (F16, BF16, FP8):
        refused(INVALID, "grid", dt=dt, B=1 << 30, total=1 << 10, max_new=1 << 10)
    refused(INVALID, "grid", D=96, nrs=192, nhs=96, rs=96, hs=16 * 96, ps=2 * 16 * 96, B=1 << 30, total=1 << 10, max_new=1 << 10)


def test_python_wrappers_refuse_bad_tensors(fa):
    import torch

    B, Hq, Hkv, D, P, total = 2, 4, 2, 64, 16, 40
    q = torch.zeros(total, Hq, D, dtype=torch.bfloat16)
    kp = torch.zeros(6, Hkv, P, D, dtype=torch.bfloat16)
    cu = torch.tensor([0, 10, 40], dtype=torch.int32)
    bt = torch.zeros(B, 3, dtype=torch.int32)
    sl = torch.tensor([10, 30], dtype=torch.int32)

    def attend(**kw):
        a = dict(q=q, k_pages=kp, v_pages=kp.clone(), cu_seqlens_q=cu, block_table=bt, seqlens_k=sl, max_seqlen_q=30)
        a.update(kw)
        return fa.flash_attention_varlen_paged(**a)

    with pytest.raises(ValueError):
        attend(q=q[0])                                  # not [total_q, Hq, D]
    with pytest.raises(ValueError):
        attend(k_pages=kp[0])                           # not a 4-d pool
    with pytest.raises(ValueError):
        attend(layout="DHN")
    with pytest.raises(ValueError):
        attend(v_pages=torch.zeros(6, Hkv, P, D, dtype=torch.float16))  # k and v pools of two types
    with pytest.raises(ValueError):
        attend(q=q.to(torch.float16))                   # q and the pool of two types
    with pytest.raises(ValueError):
        attend(q=q.float(), k_pages=kp.float(), v_pages=kp.float())  # fp32
    with pytest.raises(ValueError):
        attend(q=torch.zeros(total, 3, D, dtype=torch.bfloat16))    # Hq % Hkv
    with pytest.raises(ValueError):
        attend(q=torch.zeros(total, Hq, 128, dtype=torch.bfloat16))  # another D
    with pytest.raises(ValueError):
        attend(q=torch.zeros(total, Hq, 2 * D, dtype=torch.bfloat16)[:, :, ::2])  # element stride 2
    with pytest.raises(ValueError):
        attend(cu_seqlens_q=cu.long())
    with pytest.raises(ValueError):
        attend(block_table=bt[:1])                      # B rows
    with pytest.raises(ValueError):
        attend(seqlens_k=sl.long())
    with pytest.raises(ValueError):
        attend(block_table=torch.zeros(B, 6, dtype=torch.int32)[:, ::2])  # not contiguous
    with pytest.raises(RuntimeError):
        attend()                                        # all well-formed, but CPU tensors: there is no CPU path

    kn = torch.zeros(total, Hkv, D, dtype=torch.bfloat16)

    def append(**kw):
        a = dict(k_new=kn, v_new=kn.clone(), k_pages=kp, v_pages=kp.clone(), cu_seqlens_new=cu, block_table=bt, seqlens_k=sl, max_seqlen_new=30)
        a.update(kw)
        return fa.kv_append_paged(**a)

    with pytest.raises(ValueError):
        append(k_new=kn[:, :1])                         # heads differ from the pool's
    with pytest.raises(ValueError):
        append(v_new=kn[:10].clone())                   # k_new / v_new shapes differ
    with pytest.raises(ValueError):
        append(k_new=kn.to(torch.float16), v_new=kn.to(torch.float16))  # another type than the pool
    with pytest.raises(ValueError):
        append(k_pages=kp.float(), v_pages=kp.float(), k_new=kn.float(), v_new=kn.float())
    with pytest.raises(ValueError):
        append(v_new=torch.zeros(total, 2 * Hkv, D, dtype=torch.bfloat16)[:, ::2])  # v_new under other strides
    with pytest.raises(ValueError):
        append(layout="XYZ")
    with pytest.raises(ValueError):
        append(cu_seqlens_new=cu[:1])
    with pytest.raises(RuntimeError):
        append()
