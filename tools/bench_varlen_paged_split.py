#!/usr/bin/env python3
"""fa_fwd_varlen_paged_split next to the un-split fa_fwd_varlen_paged call on the same tensors, from the same build: raw C-ABI calls, device
events, warm clocks (a spin of --warm-ms in front of every measurement) and interleaved rounds (the candidates alternate inside every
round and EACH RUNS TWICE per round, as "#1" and "#2": the distance between the baseline's two copies is the session's own scatter; a
figure is the median over the rounds of the time per call). Shapes: bf16, causal, P = 16 pages dealt in a random order, D = 64 and 128,
heads (8, 1) and (32, 8), B in {1, 4, 16} sequences with a chunk of 512 or of 8 queries each behind 8k, 32k or 128k cached keys (the
chunk already appended). Candidates: the un-split call (the baseline: the parent's code), the split call at S = 2 .. 64 and at S = 0
(the heuristic). Per shape: the times, each ratio to the baseline, the baseline's scatter, the S the heuristic chose beside the best S
measured, min(S, slots / blocks) as what a perfect split would buy, and whether S = 0 is no slower than the baseline beyond its scatter.
usage: bench_varlen_paged_split.py [--rounds N] [--iters N] [--warm-ms MS] [--dims 64,128] [--batches 1,4,16] [--chunks 512,8]
                                   [--keys 8192,32768,131072] [--heads 8x1,32x8] [--json FILE]"""
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
ap.add_argument("--warm-ms", type=float, default=200.0)
ap.add_argument("--dims", default="64,128")
ap.add_argument("--batches", default="1,4,16")
ap.add_argument("--chunks", default="512,8")
ap.add_argument("--keys", default="8192,32768,131072")
ap.add_argument("--heads", default="8x1,32x8")
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_varlen_paged_split.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, P = fa.DTYPES["bf16"], 16
SPLITS = (2, 4, 8, 16, 32, 64)


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


def mid(res, name):
    return (res[name + " #1"] + res[name + " #2"]) / 2


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
ints = lambda s: [int(x) for x in s.split(",")]
for D in ints(args.dims):
    for Hq, Hkv in ([int(x) for x in h.split("x")] for h in args.heads.split(",")):
        for L in ints(args.keys):
            for B in ints(args.batches):
                npb = (L + P - 1) // P
                mp, num_pages = npb, B * npb + 8
                g = torch.Generator(device="cuda").manual_seed(D + L + B)
                kp = torch.rand(num_pages, P, Hkv, D, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)  # NHD pools
                vp = torch.rand(num_pages, P, Hkv, D, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
                perm = np.random.default_rng(1).permutation(num_pages)
                table = torch.from_numpy(perm[:B * npb].reshape(B, npb).astype(np.int32)).cuda()
                sl = torch.full((B,), L, dtype=torch.int32, device="cuda")
                for chunk in ints(args.chunks):
                    total_q = B * chunk
                    q = torch.rand(total_q, Hq, D, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
                    cu_q = torch.arange(0, (B + 1) * chunk, chunk, dtype=torch.int32, device="cuda")
                    o, o2 = torch.empty_like(q), torch.empty_like(q)
                    lse, lse2 = (torch.empty(Hq, total_q, dtype=torch.float32, device="cuda") for _ in range(2))
                    ws = torch.empty(max(lib.fa_fwd_varlen_paged_split_workspace_bytes(B, Hq, total_q, chunk, D, P, mp, max(SPLITS)), 16), dtype=torch.uint8,
                                     device="cuda")

                    def argv(o_, lse_, tail):
                        return (q.data_ptr(), kp.data_ptr(), vp.data_ptr(), o_.data_ptr(), lse_.data_ptr(), cu_q.data_ptr(), table.data_ptr(), sl.data_ptr(),
                                B, Hq, Hkv, total_q, chunk, D, P, num_pages, mp, D ** -0.5, Hq * D, D, P * Hkv * D, D, Hkv * D, mp) + tail + (st,)

                    base_argv = argv(o, lse, (1, BF16))
                    cands = {"unsplit": lambda: lib.fa_fwd_varlen_paged(*base_argv)}
                    for S in SPLITS + (0,):
                        a = argv(o2, lse2, (-1, 0, None, BF16, S, ws.data_ptr(), ws.numel()))
                        cands[f"S={S}"] = (lambda a_: lambda: lib.fa_fwd_varlen_paged_split(*a_))(a)
                    res = ab(cands, cands["unsplit"])
                    torch.cuda.synchronize()
                    err = float((o.float() - o2.float()).abs().max())  # (o2: the last candidate run, some split count)
                    base = mid(res, "unsplit")
                    scatter = abs(res["unsplit #1"] - res["unsplit #2"]) / base
                    t = {n: mid(res, n) for n in cands}
                    s0 = lib.fa_fwd_varlen_paged_num_splits(B, Hq, chunk, D, P, mp)
                    best = min((n for n in t if n not in ("unsplit", "S=0")), key=lambda n: t[n])
                    blocks, slots = B * Hq * ((chunk + 127) // 128), 512
                    row = dict(D=D, Hq=Hq, Hkv=Hkv, B=B, chunk=chunk, keys=L, us=t, raw=res, baseline_scatter=scatter, heuristic_S=s0, best=best,
                               s0_over_baseline=t["S=0"] / base, s0_over_best=t["S=0"] / min(t[best], base), ideal_speedup=min(s0, slots / blocks) if s0 > 1 else 1.0,
                               s0_no_slower=bool(t["S=0"] <= base * (1 + scatter)), max_abs_diff_o=err)
                    out["results"].append(row)
                    print(f"D={D} heads {Hq}x{Hkv} B={B} chunk={chunk} keys={L}: unsplit {base:9.1f} us (scatter {scatter * 100:.1f} %) | "
                          + " ".join(f"{n} {t[n] / base:.3f}" for n in t if n != "unsplit")
                          + f" | heuristic S={s0} ({base / t['S=0']:.2f}x, ideal {row['ideal_speedup']:.1f}x), best {best} ({base / t[best]:.2f}x), "
                          f"S=0 / best = {row['s0_over_best']:.3f}, S=0 no slower than the baseline: {row['s0_no_slower']}, max|dO| {err:.1e}", flush=True)
                    del q, o, o2, lse, lse2, ws
                del kp, vp
                torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
