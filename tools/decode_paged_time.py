#!/usr/bin/env python3
"""Decode steps against a PAGED KV cache (fa_fwd_decode_paged) next to fa_fwd_decode on a dense cache: raw C-ABI calls (the Python
wrappers' checks cost more than a short launch), time per call (both launches) and the TB/s of the K+V bytes the step needs,
sum_b L_b * Hkv * D * 2 * bytes. The dense cache holds every sequence at the longest length (what a host without paging pads to).
usage: decode_paged_time.py [--iters N]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import flash_attention_metal_amd as fa

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
args = ap.parse_args()
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(fn, argv):
    for _ in range(5):
        assert fn(*argv) == 0, lib.fa_last_error()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.iters):
        fn(*argv)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3


rng = np.random.default_rng(0)
shapes = [  # name, B, Hq, Hkv, D, lengths
    ("32kvh x 16384 D64", 1, 32, 32, 64, [16384]),
    ("32kvh x 16384 D128", 1, 32, 32, 128, [16384]),
    ("B16 8kvh/32qh mixed 1k-8k D128", 16, 32, 8, 128, [int(x) for x in rng.integers(1024, 8193, 16)]),
]
for (name, B, Hq, Hkv, D, lens) in shapes:
    Nq, L = 1, max(lens)
    for kv8 in (False, True):
        kvt = torch.float8_e4m3fn if kv8 else torch.bfloat16
        eb = 1 if kv8 else 2
        need = sum(lens) * Hkv * D * 2 * eb
        q = torch.randn(B, Hq, Nq, D, device="cuda", dtype=torch.bfloat16)
        o = torch.empty_like(q)
        lse = torch.empty(B, Hq, Nq, dtype=torch.float32, device="cuda")
        kd = torch.randn(B, Hkv, L, D, device="cuda", dtype=torch.bfloat16).to(kvt)
        vd = torch.randn_like(kd, dtype=torch.bfloat16).to(kvt)
        ws = torch.empty(fa.decode_workspace_bytes(B, Hq, Hkv, Nq, L, D), dtype=torch.uint8, device="cuda")
        dense = lib.fa_fwd_decode_kv8 if kv8 else lib.fa_fwd_decode
        us_d = timed(dense, (q.data_ptr(), kd.data_ptr(), vd.data_ptr(), o.data_ptr(), lse.data_ptr(), B, Hq, Hkv, Nq, L, D, D ** -0.5,
                             Hq * Nq * D, Nq * D, Hkv * L * D, L * D, 1, 2, ws.data_ptr(), ws.numel(), st))
        print(f"{name} {'bf16 on e4m3' if kv8 else 'bf16'}: dense fa_fwd_decode{'_kv8' if kv8 else ''} (Nk = {L}) {us_d:7.1f} us "
              f"{need / us_d / 1e6:5.2f} TB/s of needed K+V", flush=True)
        del kd, vd
        for P in (16, 64, 256):
            mp = (L + P - 1) // P
            npb = [(x + P - 1) // P for x in lens]
            num_pages = sum(npb) + 1
            perm = torch.randperm(num_pages, device="cuda", dtype=torch.int32)
            table = torch.zeros(B, mp, dtype=torch.int32, device="cuda")
            off = 0
            for b, n in enumerate(npb):
                table[b, :n] = perm[off:off + n]
                off += n
            sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
            wsp = torch.empty(fa.decode_paged_workspace_bytes(B, Hq, Hkv, Nq, D, P, mp), dtype=torch.uint8, device="cuda")
            for layout in ("HND", "NHD"):
                shp = (num_pages, Hkv, P, D) if layout == "HND" else (num_pages, P, Hkv, D)
                kp = torch.randn(shp, device="cuda", dtype=torch.bfloat16).to(kvt)
                vp = torch.randn(shp, device="cuda", dtype=torch.bfloat16).to(kvt)
                ps, a, b_, _ = kp.stride()
                hs, rs = (a, b_) if layout == "HND" else (b_, a)
                us = timed(lib.fa_fwd_decode_paged, (q.data_ptr(), kp.data_ptr(), vp.data_ptr(), o.data_ptr(), lse.data_ptr(), table.data_ptr(),
                                                     sl.data_ptr(), B, Hq, Hkv, Nq, D, P, num_pages, mp, D ** -0.5, Hq * Nq * D, Nq * D, ps, hs,
                                                     rs, mp, 1, 2, 3 if kv8 else 2, wsp.data_ptr(), wsp.numel(), st))
                print(f"  paged P={P:3d} {layout}: {us:7.1f} us {need / us / 1e6:5.2f} TB/s ({us / us_d:.2f}x dense)", flush=True)
                del kp, vp
