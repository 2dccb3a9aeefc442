#!/usr/bin/env python3
"""fa_fwd_mla_decode_paged_wide next to fa_fwd_mla_decode_paged on the same keys, from the same build, in the manner of
tools/bench_mla_decode.py: raw C-ABI calls, device events, warm clocks (a spin of --warm-ms in front of every measurement) and interleaved
rounds (the candidates alternate inside every round and EACH RUNS TWICE per round, as "#1" and "#2": the distance between a call's two
copies is the session's own scatter; a figure is the median over the rounds of the time per call). bf16, B in {1, 16, 128} sequences of
4k or 32k cached keys (128k at B = 1), P in {16, 64}, pages dealt in a random order. Candidates, per shape:
  old16    fa_fwd_mla_decode_paged at (Hq, Nq) = (16, 1): one one-wave item per split -- the yardstick of everything below
  old32    fa_fwd_mla_decode_paged at (16, 2), causal: two one-wave items per split over the same keys
  wide32   fa_fwd_mla_decode_paged_wide on old32's tensors: ONE workgroup of two waves per split
  wide16   the wide call at (16, 1): two waves, one of them idle, each staging half the pieces -- against old16 this separates "the one
           wave issues all the LDS-DMA" from the rest
  wide64   the wide call at (64, 1): four waves, one block
  wide128  the wide call at (128, 1): four waves, two blocks
  torch128 today's route at 128 heads without this call: gather the pages, two matmuls and a softmax (no mask)
Per candidate: us per call, TB/s of the bytes the step needs (sum L_b * 1152), rows * keys per second, the time against old16.
usage: bench_mla_decode_wide.py [--rounds N] [--iters N] [--warm-ms MS] [--batches 1,16,128] [--keys 4096,32768] [--long-keys N]
                                [--pages 16,64] [--no-torch] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import flash_attention_metal_amd as fa

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warm-ms", type=float, default=100.0)
ap.add_argument("--batches", default="1,16,128")
ap.add_argument("--keys", default="4096,32768")
ap.add_argument("--long-keys", type=int, default=131072, help="one more key count, at B = 1 only (0: none)")
ap.add_argument("--pages", default="16,64")
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_decode_wide.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, DQK, DV, SCALE = fa.DTYPES["bf16"], 576, 512, 192.0 ** -0.5


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


# candidate -> (entry point, Hq, Nq)
CALLS = {"old16": ("fa_fwd_mla_decode_paged", 16, 1), "old32": ("fa_fwd_mla_decode_paged", 16, 2), "wide32": ("fa_fwd_mla_decode_paged_wide", 16, 2),
         "wide16": ("fa_fwd_mla_decode_paged_wide", 16, 1), "wide64": ("fa_fwd_mla_decode_paged_wide", 64, 1),
         "wide128": ("fa_fwd_mla_decode_paged_wide", 128, 1)}
out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
ints = lambda s: [int(x) for x in s.split(",")]
shapes = [(B, L) for L in ints(args.keys) for B in ints(args.batches)] + ([(1, args.long_keys)] if args.long_keys else [])
for P in ints(args.pages):
    for B, L in shapes:
        npb = (L + P - 1) // P
        mp, num_pages = npb, B * npb + 8
        g = torch.Generator(device="cuda").manual_seed(P + L + B)
        pool = torch.rand(num_pages, P, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
        perm = np.random.default_rng(1).permutation(num_pages)
        table = torch.from_numpy(perm[:B * npb].reshape(B, npb).astype(np.int32)).cuda()
        tl = table.long()
        sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
        qall = torch.rand(B, 128, 2, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
        lse = torch.empty(B, 128, 2, dtype=torch.float32, device="cuda")
        cands, keep, splits = {}, [], {}
        for name, (entry, Hq, Nq) in CALLS.items():
            q = qall[:, :Hq, :Nq].contiguous()  # (old32 and wide32: the same tensor)
            o = torch.empty(B, Hq, Nq, DV, device="cuda", dtype=torch.bfloat16)
            need = getattr(lib, entry + "_workspace_bytes")(B, Hq, Nq, DV, P, mp)
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
            keep += [q, o, ws]
            splits[name] = need // (B * ((Hq * Nq + 15) // 16) * 16 * (DV + 2) * 4)
            a = (q.data_ptr(), pool.data_ptr(), o.data_ptr(), lse.data_ptr(), table.data_ptr(), sl.data_ptr(), B, Hq, Nq, DQK, DV, P, num_pages, mp,
                 SCALE, Hq * Nq * DQK, Nq * DQK, DQK, Hq * Nq * DV, Nq * DV, DV, P * DQK, DQK, mp, int(Nq > 1), BF16, ws.data_ptr(), ws.numel(), st)
            cands[name] = (lambda f, a2: lambda: f(*a2))(getattr(lib, entry), a)
        if not args.no_torch:
            q2 = qall[:, :, 0].contiguous()  # [B, 128, 576]

            def workaround():
                kv = pool[tl].reshape(B, npb * P, DQK)[:, :L]
                s = torch.bmm(q2, kv.transpose(1, 2)).float().mul_(SCALE)
                torch.bmm(torch.softmax(s, -1).to(torch.bfloat16), kv[..., :DV])

            cands["torch128"] = workaround
        res = ab(cands, cands["old16"])
        t = {n: (res[n + " #1"] + res[n + " #2"]) / 2 for n in cands}
        scatter = {n: abs(res[n + " #1"] - res[n + " #2"]) / t[n] for n in cands}
        need = B * L * DQK * 2
        rows = {n: (CALLS[n][1] * CALLS[n][2] if n in CALLS else 128) for n in cands}
        row = dict(P=P, B=B, keys=L, us=t, raw=res, scatter=scatter, splits=splits, tbs={n: need / t[n] * 1e-6 for n in cands},
                   row_keys_per_s={n: rows[n] * B * L / (t[n] * 1e-6) for n in cands}, vs_old16={n: t[n] / t["old16"] for n in cands},
                   wide32_vs_old32=t["wide32"] / t["old32"], old32_vs_old16=t["old32"] / t["old16"])
        out["results"].append(row)
        print(f"P={P} B={B} keys={L}: " + " | ".join(
            f"{n} {t[n]:8.1f} us {row['tbs'][n]:5.2f} TB/s x{row['vs_old16'][n]:.2f} (S={splits.get(n, 0)}, +-{scatter[n] * 100:.1f} %)" for n in cands)
            + f" | wide32 / old32 {row['wide32_vs_old32']:.3f}", flush=True)
        del cands, keep, qall, pool
        torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
