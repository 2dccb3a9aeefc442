#!/usr/bin/env python3
"""One call per launcher branch of a build of libfa_mi355.so, at the smallest shapes that reach it; prints the SHA-256 of every output.

usage: launch_census.py LIB.so

For comparing two builds whose host code differs: run it once per library under `rocprofv3 --kernel-trace` and compare the dispatches
(kernel name, grid, workgroup, LDS, scratch) and the hash lists. Inputs are drawn on the CPU from a fixed seed; outputs start as zeros,
so bytes a kernel does not write hash alike. A call the library refuses prints its status instead of hashes.
"""
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from flash_attention_metal_amd._lib import SYMBOLS  # noqa: E402

lib = ctypes.CDLL(os.path.abspath(sys.argv[1]))
for name, (res, args) in SYMBOLS.items():
    getattr(lib, name).restype, getattr(lib, name).argtypes = res, args

F16, BF16, FP8 = 1, 2, 3
TORCH = {F16: torch.float16, BF16: torch.bfloat16, FP8: torch.float8_e4m3fn}
NAME = {F16: "f16", BF16: "bf16", FP8: "e4m3"}
gen = torch.Generator().manual_seed(15)
st = None  # the default stream


def rnd(dtype, *shape):
    return (torch.rand(*shape, generator=gen) * 2 - 1).to(TORCH[dtype]).cuda()


def zeros(dtype, *shape):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def out_dtype(dtype):
    return torch.bfloat16 if dtype == FP8 else TORCH[dtype]


def i32(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def report(tag, rc, *outs):
    torch.cuda.synchronize()
    if rc != 0:
        print(f"{tag} status={rc} {lib.fa_last_error().decode()}", flush=True)
        return
    hashes = " ".join(hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:32] for t in outs)
    print(f"{tag} {hashes}", flush=True)


def ptr(t):
    return t.data_ptr()


def fwd(tag, variant, dtype, B, H, N, D, causal):
    q, k, v = (rnd(dtype, B, H, N, D) for _ in range(3))
    o, lse = zeros(out_dtype(dtype), B, H, N, D), zeros(torch.float32, B, H, N)
    rc = lib.fa_fwd(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, H, N, D, D ** -0.5, H * N * D, N * D, causal, dtype, variant, st)
    report(f"{tag} {lib.fa_variant_name(variant).decode()} {NAME[dtype]} B{B} H{H} N{N} D{D} causal{causal}", rc, o, lse)


def fwd_ex(dtype, variant, B, Hq, Hkv, Nq, Nk, D, causal):
    q, k, v = rnd(dtype, B, Hq, Nq, D), rnd(dtype, B, Hkv, Nk, D), rnd(dtype, B, Hkv, Nk, D)
    o, lse = zeros(out_dtype(dtype), B, Hq, Nq, D), zeros(torch.float32, B, Hq, Nq)
    rc = lib.fa_fwd_exv(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, Hq, Hkv, Nq, Nk, D, D ** -0.5, Hq * Nq * D, Nq * D, Hkv * Nk * D, Nk * D,
                        causal, dtype, variant, st)
    report(f"fwd_ex {lib.fa_variant_name(variant).decode()} {NAME[dtype]} Hq{Hq} Hkv{Hkv} Nq{Nq} Nk{Nk} D{D} causal{causal}", rc, o, lse)
    return q, k, v, o, lse, rc


def cu(lengths):
    out = [0]
    for n in lengths:
        out.append(out[-1] + n)
    return out


LQ, LK = (100, 200, 37), (150, 260, 300)  # three packed sequences, every Lk >= Lq
HQ, HKV, PAGE = 4, 2, 16


def page_pool(dtype, lengths, D):
    """an HND pool [num_pages, Hkv, PAGE, D] whose table deals the pages out in a shuffled order"""
    max_pages = (max(lengths) + PAGE - 1) // PAGE
    num_pages = len(lengths) * max_pages
    order = torch.randperm(num_pages, generator=gen).to(torch.int32).reshape(len(lengths), max_pages).cuda()
    return rnd(dtype, num_pages, HKV, PAGE, D), rnd(dtype, num_pages, HKV, PAGE, D), order.contiguous(), i32(list(lengths)), num_pages, max_pages


def varlen(dtype, D, causal, window):
    tq, tk = sum(LQ), sum(LK)
    q, k, v = rnd(dtype, tq, HQ, D), rnd(dtype, tk, HKV, D), rnd(dtype, tk, HKV, D)
    o, lse = zeros(TORCH[dtype], tq, HQ, D), zeros(torch.float32, HQ, tq)
    cq, ck = i32(cu(LQ)), i32(cu(LK))
    head = [ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), ptr(cq), ptr(ck), len(LQ), HQ, HKV, tq, tk, max(LQ), max(LK), D, D ** -0.5,
            HQ * D, D, HKV * D, D]
    if window is None:
        rc = lib.fa_fwd_varlen(*head, causal, dtype, st)
        report(f"varlen {NAME[dtype]} D{D} causal{causal}", rc, o, lse)
    else:
        rc = lib.fa_fwd_varlen_window(*head, window[0], window[1], dtype, st)
        report(f"varlen_window {NAME[dtype]} D{D} window{window}", rc, o, lse)
    return q, k, v, o, lse, cq, ck, rc


def varlen_paged(dtype, D, causal, window):
    tq = sum(LQ)
    q = rnd(dtype, tq, HQ, D)
    kp, vp, table, seqlens, num_pages, max_pages = page_pool(dtype, LK, D)
    o, lse = zeros(TORCH[dtype], tq, HQ, D), zeros(torch.float32, HQ, tq)
    cq = i32(cu(LQ))
    head = [ptr(q), ptr(kp), ptr(vp), ptr(o), ptr(lse), ptr(cq), ptr(table), ptr(seqlens), len(LQ), HQ, HKV, tq, max(LQ), D, PAGE, num_pages,
            max_pages, D ** -0.5, HQ * D, D, HKV * PAGE * D, PAGE * D, D, max_pages]
    if window is None:
        rc = lib.fa_fwd_varlen_paged(*head, causal, dtype, st)
        report(f"varlen_paged {NAME[dtype]} D{D} causal{causal}", rc, o, lse)
    else:
        rc = lib.fa_fwd_varlen_paged_window(*head, window[0], window[1], dtype, st)
        report(f"varlen_paged_window {NAME[dtype]} D{D} window{window}", rc, o, lse)


def decode(q_dtype, kv_dtype, D, Nq, causal):
    B, Hq, Nk = 2, 16, 1000  # (Hq / Hkv) * Nq = 8 * Nq packed rows
    q, k, v = rnd(q_dtype, B, Hq, Nq, D), rnd(kv_dtype, B, HKV, Nk, D), rnd(kv_dtype, B, HKV, Nk, D)
    o, lse = zeros(out_dtype(q_dtype), B, Hq, Nq, D), zeros(torch.float32, B, Hq, Nq)
    nbytes = lib.fa_fwd_decode_workspace_bytes(B, Hq, HKV, Nq, Nk, D)
    ws = zeros(torch.uint8, max(nbytes, 16))
    fn = lib.fa_fwd_decode if q_dtype == kv_dtype else lib.fa_fwd_decode_kv8
    rc = fn(ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, Hq, HKV, Nq, Nk, D, D ** -0.5, Hq * Nq * D, Nq * D, HKV * Nk * D, Nk * D, causal,
            q_dtype, ptr(ws), nbytes, st)
    report(f"decode q{NAME[q_dtype]} kv{NAME[kv_dtype]} D{D} Nq{Nq} causal{causal}", rc, o, lse)


def decode_paged(q_dtype, kv_dtype, D, Nq, causal, window):
    B, Hq, lengths = 2, 16, (1000, 517)
    q = rnd(q_dtype, B, Hq, Nq, D)
    kp, vp, table, seqlens, num_pages, max_pages = page_pool(kv_dtype, lengths, D)
    o, lse = zeros(out_dtype(q_dtype), B, Hq, Nq, D), zeros(torch.float32, B, Hq, Nq)
    nbytes = lib.fa_fwd_decode_paged_workspace_bytes(B, Hq, HKV, Nq, D, PAGE, max_pages)
    ws = zeros(torch.uint8, max(nbytes, 16))
    head = [ptr(q), ptr(kp), ptr(vp), ptr(o), ptr(lse), ptr(table), ptr(seqlens), B, Hq, HKV, Nq, D, PAGE, num_pages, max_pages, D ** -0.5,
            Hq * Nq * D, Nq * D, HKV * PAGE * D, PAGE * D, D, max_pages]
    if window is None:
        rc = lib.fa_fwd_decode_paged(*head, causal, q_dtype, kv_dtype, ptr(ws), nbytes, st)
        report(f"decode_paged q{NAME[q_dtype]} kv{NAME[kv_dtype]} D{D} Nq{Nq} causal{causal}", rc, o, lse)
    else:
        rc = lib.fa_fwd_decode_paged_window(*head, window[0], window[1], q_dtype, kv_dtype, ptr(ws), nbytes, st)
        report(f"decode_paged_window q{NAME[q_dtype]} kv{NAME[kv_dtype]} D{D} Nq{Nq} window{window}", rc, o, lse)


def append(dtype, D):
    new = (5, 20)
    kp, vp, table, seqlens, num_pages, max_pages = page_pool(dtype, (100, 200), D)  # seqlens: the lengths after the append
    kn, vn = rnd(dtype, sum(new), HKV, D), rnd(dtype, sum(new), HKV, D)
    cn = i32(cu(new))
    rc = lib.fa_kv_append_paged(ptr(kn), ptr(vn), ptr(kp), ptr(vp), ptr(cn), ptr(table), ptr(seqlens), len(new), HKV, sum(new), max(new), D, PAGE,
                                num_pages, max_pages, HKV * D, D, HKV * PAGE * D, PAGE * D, D, max_pages, dtype, st)
    report(f"kv_append_paged {NAME[dtype]} D{D}", rc, kp, vp)


def bwd_ex(dtype, D, causal):
    B, Nq, Nk = 1, 200, 300
    q, k, v, o, lse, rc = fwd_ex(dtype, 0, B, HQ, HKV, Nq, Nk, D, causal)
    if rc != 0:
        return
    do = rnd(BF16 if dtype == FP8 else dtype, B, HQ, Nq, D)
    dq, dk, dv = zeros(torch.float32, B, HQ, Nq, D), zeros(torch.float32, B, HKV, Nk, D), zeros(torch.float32, B, HKV, Nk, D)
    strides = (HQ * Nq * D, Nq * D, HKV * Nk * D, Nk * D)
    ws = zeros(torch.uint8, max(lib.fa_bwd_workspace_bytes_ex(dtype, B, HQ, HKV, Nq, Nk, D, *strides), 16))
    rc = lib.fa_bwd_ex(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(dq), ptr(dk), ptr(dv), ptr(ws), B, HQ, HKV, Nq, Nk, D, D ** -0.5,
                       *strides, causal, dtype, st)
    report(f"bwd_ex {NAME[dtype]} D{D} causal{causal}", rc, dq, dk, dv)


def bwd_varlen(dtype, D, causal):
    q, k, v, o, lse, cq, ck, rc = varlen(dtype, D, causal, None)
    if rc != 0:
        return
    tq, tk = sum(LQ), sum(LK)
    do = rnd(dtype, tq, HQ, D)
    dq, dk, dv = zeros(torch.float32, tq, HQ, D), zeros(torch.float32, tk, HKV, D), zeros(torch.float32, tk, HKV, D)
    ws = zeros(torch.uint8, max(lib.fa_bwd_varlen_workspace_bytes(HQ, tq), 16))
    rc = lib.fa_bwd_varlen(ptr(q), ptr(k), ptr(v), ptr(o), ptr(do), ptr(lse), ptr(dq), ptr(dk), ptr(dv), ptr(ws), ptr(cq), ptr(ck), len(LQ), HQ,
                           HKV, tq, tk, max(LQ), max(LK), D, D ** -0.5, HQ * D, D, HKV * D, D, causal, dtype, st)
    report(f"bwd_varlen {NAME[dtype]} D{D} causal{causal}", rc, dq, dk, dv)


MFMA, SPLITKV, EXACT, MFMA16 = 4, 6, 8, 10
# fa_fwd: every variant the library has a kernel for
for variant in range(1, 12):
    for dtype in (F16, BF16, FP8):
        for D in (32, 64, 96, 128, 256):
            if lib.fa_supported(dtype, variant, D):
                for causal in (0, 1):
                    fwd("fwd", variant, dtype, 1, 2, 200, D, causal)
# mfma16: padded head dims (four waves), and eight waves on the smallest grids mfma16_waves gives them
for dtype in (F16, BF16):
    for D in (40, 72):
        for causal in (0, 1):
            fwd("mfma16_padded", MFMA16, dtype, 1, 2, 200, D, causal)
    fwd("mfma16_eight_waves", MFMA16, dtype, 1, 256, 512, 64, 0)
    fwd("mfma16_eight_waves", MFMA16, dtype, 1, 64, 4096, 64, 1)
    fwd("mfma16_eight_waves", MFMA16, dtype, 1, 32, 8192, 128, 0)
# split-KV: 2, 4 and 8 waves
for dtype in (F16, BF16, FP8):
    for N in (128, 256, 1024):
        for causal in (0, 1):
            fwd("splitkv_waves", SPLITKV, dtype, 1, 2, N, 64, causal)
# grouped heads, Nq != Nk
for dtype in (F16, BF16):
    for D in (64, 128):
        for causal in (0, 1):
            for variant in (0, MFMA, EXACT, MFMA16) + ((SPLITKV,) if D == 64 else ()):
                fwd_ex(dtype, variant, 2, HQ, HKV, 100, 300, D, causal)
# packed sequences, dense and paged, masked, unmasked and windowed
for dtype in (F16, BF16):
    for D in (64, 128):
        for causal in (0, 1):
            varlen(dtype, D, causal, None)
            varlen_paged(dtype, D, causal, None)
        varlen(dtype, D, 0, (50, 10))
        varlen_paged(dtype, D, 0, (50, 10))
# decode: one and two query tiles (8 and 24 packed rows)
for q_dtype, kv_dtype in ((F16, F16), (BF16, BF16), (FP8, FP8), (BF16, FP8)):
    for D in (64, 128):
        for Nq in (1, 3):
            for causal in (0, 1):
                decode(q_dtype, kv_dtype, D, Nq, causal)
                decode_paged(q_dtype, kv_dtype, D, Nq, causal, None)
            decode_paged(q_dtype, kv_dtype, D, Nq, 0, (100, 0))
for dtype in (BF16, FP8):
    append(dtype, 64)
# backward: head dims with a kernel of their own, padded ones, e4m3 inputs, packed sequences
for dtype in (F16, BF16):
    for D in (64, 128, 256, 40, 96):
        for causal in (0, 1):
            bwd_ex(dtype, D, causal)
    for D in (64, 128):
        for causal in (0, 1):
            bwd_varlen(dtype, D, causal)
bwd_ex(FP8, 64, 1)
print("done", flush=True)
