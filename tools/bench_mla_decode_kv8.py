#!/usr/bin/env python3
"""fa_fwd_mla_decode_paged_kv8 (bf16 queries, e4m3 latent pool) next to fa_fwd_mla_decode_paged_wide (bf16 pool) on the same keys -- the
e4m3 pool is drawn on the e4m3 grid and the bf16 pool is its exact widening, pages in the same random order -- from the same build, in
the manner of tools/bench_mla_decode_wide.py: raw C-ABI calls, device events, warm clocks (a spin of --warm-ms in front of every
measurement) and interleaved rounds (the candidates alternate inside every round and EACH RUNS TWICE per round, as "#1" and "#2": the
distance between a call's two copies is the session's own scatter; a figure is the median over the rounds of the time per call).
B in {1, 16, 128} sequences of 4k or 32k cached keys (128k at B = 1), P in {16, 64}. Candidates, per shape and per (Hq, Nq) in
(16, 1), (16, 2) causal, (64, 1), (128, 1):
  kv8<rows>   fa_fwd_mla_decode_paged_kv8: four waves, the tile staged through registers and widened
  wide<rows>  fa_fwd_mla_decode_paged_wide (bf16): two waves up to 32 rows, four above, the tile moved by LDS-DMA
Per pair: us per call of each, the time ratio kv8 / wide, TB/s of the bytes each step needs (sum L_b * 576 for e4m3, * 1152 for bf16),
and each call against its own second copy.
usage: bench_mla_decode_kv8.py [--rounds N] [--iters N] [--warm-ms MS] [--batches 1,16,128] [--keys 4096,32768] [--long-keys N]
                               [--pages 16,64] [--json FILE]"""
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
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_decode_kv8.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, FP8, DQK, DV, SCALE = fa.DTYPES["bf16"], fa.DTYPES["fp8_e4m3"], 576, 512, 192.0 ** -0.5
ROWS = [(16, 1), (16, 2), (64, 1), (128, 1)]


def ab(cands, warm):
    """{name: median us per call} of callables measured in alternation, each twice per round, behind a spin that keeps the clocks up."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in cands.values():
        for _ in range(2):
            assert fn() == 0, lib.fa_last_error()
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


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
ints = lambda s: [int(x) for x in s.split(",")]
shapes = [(B, L) for L in ints(args.keys) for B in ints(args.batches)] + ([(1, args.long_keys)] if args.long_keys else [])
for P in ints(args.pages):
    for B, L in shapes:
        npb = (L + P - 1) // P
        mp, num_pages = npb, B * npb + 8
        g = torch.Generator(device="cuda").manual_seed(P + L + B)
        pool8 = torch.rand(num_pages, P, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.float8_e4m3fn)
        pool16 = pool8.to(torch.bfloat16)  # exact: the same values
        perm = np.random.default_rng(1).permutation(num_pages)
        table = torch.from_numpy(perm[:B * npb].reshape(B, npb).astype(np.int32)).cuda()
        sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
        qall = torch.rand(B, 128, 2, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
        lse = torch.empty(B, 128, 2, dtype=torch.float32, device="cuda")
        cands, keep, splits = {}, [], {}
        for Hq, Nq in ROWS:
            rows = Hq * Nq
            q = qall[:, :Hq, :Nq].contiguous()
            need = lib.fa_fwd_mla_decode_paged_kv8_workspace_bytes(B, Hq, Nq, DV, P, mp)
            assert need == lib.fa_fwd_mla_decode_paged_wide_workspace_bytes(B, Hq, Nq, DV, P, mp) > 0
            splits[rows] = need // (B * ((rows + 15) // 16) * 16 * (DV + 2) * 4)
            for name, entry, pool, tail in ((f"kv8{rows}", "fa_fwd_mla_decode_paged_kv8", pool8, (BF16, FP8)),
                                            (f"wide{rows}", "fa_fwd_mla_decode_paged_wide", pool16, (BF16,))):
                o = torch.empty(B, Hq, Nq, DV, device="cuda", dtype=torch.bfloat16)
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")
                keep += [q, o, ws]
                a = (q.data_ptr(), pool.data_ptr(), o.data_ptr(), lse.data_ptr(), table.data_ptr(), sl.data_ptr(), B, Hq, Nq, DQK, DV, P, num_pages,
                     mp, SCALE, rows * DQK, Nq * DQK, DQK, rows * DV, Nq * DV, DV, P * DQK, DQK, mp, int(Nq > 1), *tail, ws.data_ptr(), ws.numel(), st)
                cands[name] = (lambda f, a2: lambda: f(*a2))(getattr(lib, entry), a)
        res = ab(cands, cands["wide16"])
        t = {n: (res[n + " #1"] + res[n + " #2"]) / 2 for n in cands}
        scatter = {n: abs(res[n + " #1"] - res[n + " #2"]) / t[n] for n in cands}
        tbs = {n: B * L * DQK * (1 if n.startswith("kv8") else 2) / t[n] * 1e-6 for n in cands}
        ratio = {Hq * Nq: t[f"kv8{Hq * Nq}"] / t[f"wide{Hq * Nq}"] for Hq, Nq in ROWS}
        out["results"].append(dict(P=P, B=B, keys=L, us=t, raw=res, scatter=scatter, splits=splits, tbs=tbs, kv8_vs_wide=ratio))
        print(f"P={P} B={B} keys={L}: " + " | ".join(
            f"{r} rows (S={splits[r]}): kv8 {t[f'kv8{r}']:8.1f} us {tbs[f'kv8{r}']:5.2f} TB/s +-{scatter[f'kv8{r}'] * 100:.1f} %, "
            f"wide {t[f'wide{r}']:8.1f} us {tbs[f'wide{r}']:5.2f} TB/s +-{scatter[f'wide{r}'] * 100:.1f} %, kv8 / wide {ratio[r]:.3f}"
            for r in ratio), flush=True)
        del cands, keep, qall, pool8, pool16
        torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
