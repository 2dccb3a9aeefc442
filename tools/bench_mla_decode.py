#!/usr/bin/env python3
"""fa_fwd_mla_decode_paged next to three yardsticks on the same key counts, from the same build: raw C-ABI calls, device events, warm clocks
(a spin of --warm-ms in front of every measurement) and interleaved rounds (the candidates alternate inside every round and EACH RUNS
TWICE per round, as "#1" and "#2": the distance between the MLA call's two copies is the session's own scatter; a figure is the median
over the rounds of the time per call). Shapes: bf16, Hq = 16, Nq in {1, 2} (causal when 2), B in {1, 16, 128} sequences of 4k or 32k
cached keys (128k at B = 1), P in {16, 64}, pages dealt in a random order. Yardsticks:
  decode128   fa_fwd_decode_paged bf16, D = 128, Hq = 16, Hkv = 1 on the same key counts: the achieved TB/s of ITS needed bytes
              (sum L_b * 2 pools * 256 B) is what the existing decode design reaches;
  torch       the workaround without this call: gather the pages, two matmuls and a softmax, on the same tensors (no mask);
  mla #2      the call against its own second copy: scatter.
--alt NAME=PATH loads another build of the library (other split constants) as one more candidate, timed in the same rounds.
Per shape: us per call, TB/s of the bytes the step needs (sum L_b * 1152), the ratio of the two achieved bandwidths.
usage: bench_mla_decode.py [--rounds N] [--iters N] [--warm-ms MS] [--batches 1,16,128] [--keys 4096,32768] [--pages 16,64] [--nq 1,2]
                           [--alt NAME=PATH ...] [--no-torch] [--json FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import flash_attention_metal_amd as fa
from flash_attention_metal_amd._lib import SYMBOLS

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warm-ms", type=float, default=100.0)
ap.add_argument("--batches", default="1,16,128")
ap.add_argument("--keys", default="4096,32768")
ap.add_argument("--long-keys", type=int, default=131072, help="one more key count, at B = 1 only (0: none)")
ap.add_argument("--pages", default="16,64")
ap.add_argument("--nq", default="1,2")
ap.add_argument("--alt", action="append", default=[])
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_decode.py measures on the GPU: none found")
lib = fa.load_library()
libs = {"mla": lib}
for spec in args.alt:
    name, path = spec.split("=", 1)
    alt = ctypes.CDLL(os.path.abspath(path))
    for sym in ("fa_fwd_mla_decode_paged", "fa_fwd_mla_decode_paged_workspace_bytes", "fa_last_error"):
        getattr(alt, sym).restype, getattr(alt, sym).argtypes = SYMBOLS[sym]
    libs[name] = alt
st = torch.cuda.current_stream().cuda_stream
BF16, HQ, DQK, DV, SCALE = fa.DTYPES["bf16"], 16, 576, 512, 192.0 ** -0.5


def ab(cands, warm):
    """{name: median us per call} of callables measured in alternation, each twice per round, behind a spin that keeps the clocks up."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in cands.values():
        for _ in range(2):
            assert fn() in (0, None), lib.fa_last_error()
    torch.cuda.synchronize()
    twice = {f"{n} #{k}": fn for k in (1, 2) for n, fn in cands.items()}
    times = {n: [] for n in twice}
    for r in range(args.rounds):
        order = list(twice)
        order = order[r % len(order):] + order[:r % len(order)]
        for name in order:
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < args.warm_ms:
                warm()
                torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                twice[name]()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters * 1e3)
    return {n: statistics.median(t) for n, t in times.items()}


def mid(res, name):
    return (res[name + " #1"] + res[name + " #2"]) / 2


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
ints = lambda s: [int(x) for x in s.split(",")]
shapes = [(B, L) for L in ints(args.keys) for B in ints(args.batches)] + ([(1, args.long_keys)] if args.long_keys else [])
for P in ints(args.pages):
    for B, L in shapes:
        npb = (L + P - 1) // P
        mp, num_pages = npb, B * npb + 8
        g = torch.Generator(device="cuda").manual_seed(P + L + B)
        pool = torch.rand(num_pages, P, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
        kp = torch.rand(num_pages, P, 128, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)  # the yardstick's pools
        vp = torch.rand(num_pages, P, 128, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
        perm = np.random.default_rng(1).permutation(num_pages)
        table = torch.from_numpy(perm[:B * npb].reshape(B, npb).astype(np.int32)).cuda()
        tl = table.long()
        sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
        for Nq in ints(args.nq):
            causal = int(Nq > 1)
            q = torch.rand(B, HQ, Nq, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
            q128 = torch.rand(B, HQ, Nq, 128, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
            o, o128 = torch.empty(B, HQ, Nq, DV, device="cuda", dtype=torch.bfloat16), torch.empty_like(q128)
            lse = torch.empty(B, HQ, Nq, dtype=torch.float32, device="cuda")
            cands, keep = {}, []
            for name, l_ in libs.items():
                ws = torch.empty(max(l_.fa_fwd_mla_decode_paged_workspace_bytes(B, HQ, Nq, DV, P, mp), 16), dtype=torch.uint8, device="cuda")
                keep.append(ws)
                a = (q.data_ptr(), pool.data_ptr(), o.data_ptr(), lse.data_ptr(), table.data_ptr(), sl.data_ptr(), B, HQ, Nq, DQK, DV, P, num_pages, mp,
                     SCALE, HQ * Nq * DQK, Nq * DQK, DQK, HQ * Nq * DV, Nq * DV, DV, P * DQK, DQK, mp, causal, BF16, ws.data_ptr(), ws.numel(), st)
                cands[name] = (lambda l2, a2: lambda: l2.fa_fwd_mla_decode_paged(*a2))(l_, a)
            ws128 = torch.empty(max(lib.fa_fwd_decode_paged_workspace_bytes(B, HQ, 1, Nq, 128, P, mp), 16), dtype=torch.uint8, device="cuda")
            a128 = (q128.data_ptr(), kp.data_ptr(), vp.data_ptr(), o128.data_ptr(), lse.data_ptr(), table.data_ptr(), sl.data_ptr(), B, HQ, 1, Nq, 128, P,
                    num_pages, mp, 128 ** -0.5, HQ * Nq * 128, Nq * 128, P * 128, 128, 128, mp, causal, BF16, BF16, ws128.data_ptr(), ws128.numel(), st)
            cands["decode128"] = lambda: lib.fa_fwd_decode_paged(*a128)
            if not args.no_torch:
                q2 = q.reshape(B, HQ * Nq, DQK)

                def workaround():
                    kv = pool[tl].reshape(B, npb * P, DQK)[:, :L]
                    s = torch.bmm(q2, kv.transpose(1, 2)).float().mul_(SCALE)
                    torch.bmm(torch.softmax(s, -1).to(torch.bfloat16), kv[..., :DV])

                cands["torch"] = workaround
            res = ab(cands, cands["mla"])
            t = {n: mid(res, n) for n in cands}
            need, need128 = B * L * DQK * 2, B * L * 128 * 2 * 2
            tbs, tbs128 = need / t["mla"] * 1e-6, need128 / t["decode128"] * 1e-6
            scatter = abs(res["mla #1"] - res["mla #2"]) / t["mla"]
            row = dict(P=P, B=B, keys=L, Nq=Nq, us=t, raw=res, scatter=scatter, mla_tbs=tbs, decode128_tbs=tbs128, bandwidth_ratio=tbs / tbs128,
                       splits=int(keep[0].numel() // (B * ((HQ * Nq + 15) // 16) * 16 * (DV + 2) * 4)))
            out["results"].append(row)
            print(f"P={P} B={B} keys={L} Nq={Nq}: mla {t['mla']:9.1f} us = {tbs:5.2f} TB/s (S={row['splits']}, scatter {scatter * 100:.1f} %) | decode128 "
                  f"{t['decode128']:9.1f} us = {tbs128:5.2f} TB/s | mla / decode128 bandwidth {tbs / tbs128:.2f}"
                  + (f" | torch {t['torch']:9.1f} us ({t['torch'] / t['mla']:.1f}x)" if "torch" in t else "")
                  + "".join(f" | {n} {t[n] / t['mla']:.3f}" for n in libs if n != "mla"), flush=True)
            del q, q128, o, o128, keep, ws128
        del pool, kp, vp
        torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
