#!/usr/bin/env python3
"""fa_fwd_varlen_paged_kv8 and fa_kv_append_paged_quant next to what a caller has without them, from the same build: raw C-ABI calls,
device events, warm clocks (a spin of --warm-ms in front of every measurement) and interleaved rounds (the candidates alternate inside
every round and EACH RUNS TWICE per round, as "#1" and "#2": the distance between the two is the session's own scatter; a figure is the
median over the rounds of the time per call). The shape of tools/bench_varlen_paged.py -- a chunked-prefill step: 16 sequences with 1k-8k
cached keys (seeded; the chunk already appended), chunks of 512 queries, 16 query heads on 16 key heads, bf16 queries, causal, P = 16
pages dealt in a random order, D = 64 and 128:
  (a) the KV8 call on the e4m3 pool against fa_fwd_varlen_paged_window (INT_MAX, 0) on the bf16 twin pool: the price of losing LDS-DMA
      and of the widening (both run the window-mode kernel family under a never-binding bound);
  (b) the KV8 call against widening the pool to a bf16 copy with torch (all but 8 of its pages are in use) and then the bf16 call: what
      a caller with an e4m3 cache does today;
  (c) fa_kv_append_paged_quant (bf16 rows into the e4m3 pool) against fa_kv_append_paged (the same rows into the bf16 pool); both are
      cache-resident figures;
also checks, at the sizes timed, that the KV8 result equals the bf16 call on the twin bit for bit.
usage: bench_varlen_paged_kv8.py [--rounds N] [--iters N] [--warm-ms MS] [--json FILE]"""
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
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warm-ms", type=float, default=400.0)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_varlen_paged_kv8.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, FP8, H, P, CHUNK, B, INT_MAX = fa.DTYPES["bf16"], fa.DTYPES["fp8_e4m3"], 16, 16, 512, 16, 2 ** 31 - 1


def ab(cands, warm):
    """{name: median us per call} of callables measured in alternation, each twice per round, behind a spin that keeps the clocks up."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in cands.values():
        for _ in range(3):
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
    return {n: dict(median_us=statistics.median(t), min_us=min(t), max_us=max(t)) for n, t in times.items()}


def mid(res, name):
    return (res[name + " #1"]["median_us"] + res[name + " #2"]["median_us"]) / 2


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
for D in (64, 128):
    lens = [int(x) for x in np.random.default_rng(0).integers(1024, 8193, B)]
    npb = [(L + P - 1) // P for L in lens]
    mp, num_pages, total_k, total_q = max(npb), sum(npb) + 8, sum(lens), B * CHUNK
    g = torch.Generator(device="cuda").manual_seed(D)

    def rnd(*shape):
        return torch.rand(*shape, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)

    q = rnd(total_q, H, D)
    k8, v8 = rnd(num_pages, P, H, D).to(torch.float8_e4m3fn), rnd(num_pages, P, H, D).to(torch.float8_e4m3fn)  # NHD pools
    k16, v16 = k8.to(torch.bfloat16), v8.to(torch.bfloat16)  # the twin
    kw, vw = torch.empty_like(k16), torch.empty_like(v16)    # (b): where the caller widens to
    perm = np.random.default_rng(1).permutation(num_pages)
    table_h, used = np.zeros((B, mp), np.int32), 0
    for b in range(B):
        table_h[b, :npb[b]] = perm[used:used + npb[b]]
        used += npb[b]
    table, sl = torch.from_numpy(table_h).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    cu_q = torch.arange(0, (B + 1) * CHUNK, CHUNK, dtype=torch.int32, device="cuda")
    o, o2, o3 = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    lse, lse2, lse3 = (torch.empty(H, total_q, dtype=torch.float32, device="cuda") for _ in range(3))

    def argv(kp, vp, o_, lse_, tail):
        return (q.data_ptr(), kp.data_ptr(), vp.data_ptr(), o_.data_ptr(), lse_.data_ptr(), cu_q.data_ptr(), table.data_ptr(), sl.data_ptr(),
                B, H, H, total_q, CHUNK, D, P, num_pages, mp, D ** -0.5, H * D, D, P * H * D, D, H * D, mp) + tail + (st,)

    kv8_argv = argv(k8, v8, o, lse, (-1, 0, None, BF16, FP8))
    twin_argv = argv(k16, v16, o2, lse2, (INT_MAX, 0, BF16))
    wide_argv = argv(kw, vw, o3, lse3, (INT_MAX, 0, BF16))

    def kv8():
        return lib.fa_fwd_varlen_paged_kv8(*kv8_argv)

    def twin():
        return lib.fa_fwd_varlen_paged_window(*twin_argv)

    def widen_then_bf16():
        kw.copy_(k8)
        vw.copy_(v8)
        return lib.fa_fwd_varlen_paged_window(*wide_argv)

    assert kv8() == 0 and twin() == 0 and widen_then_bf16() == 0, lib.fa_last_error()
    torch.cuda.synchronize()
    same = bool(torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(o, o3) and torch.equal(lse, lse3))
    res = ab({"fa_fwd_varlen_paged_kv8": kv8, "bf16 window call, twin pool": twin, "widen the pool + bf16 call": widen_then_bf16}, twin)
    fl = sum(2.0 * H * D * 2 * (CHUNK * (L - CHUNK) + CHUNK * (CHUNK + 1) / 2) for L in lens)
    for n, r in res.items():
        r["tflops"] = fl / r["median_us"] / 1e6
        print(f"D={D} 16 x 512 queries on 1k-8k cached keys ({total_k} keys), causal, bf16 q, P={P}: {n:34s} {r['median_us']:8.1f} us "
              f"(min {r['min_us']:.1f}, max {r['max_us']:.1f})  {r['tflops']:6.1f} TFLOP/s", flush=True)
    ra = mid(res, "fa_fwd_varlen_paged_kv8") / mid(res, "bf16 window call, twin pool")
    rb = mid(res, "fa_fwd_varlen_paged_kv8") / mid(res, "widen the pool + bf16 call")
    print(f"(a) D={D}: KV8 / bf16 call on the twin = {ra:.4f}   (b) KV8 / (widen + bf16 call) = {rb:.4f}   KV8 equals the bf16 call on the twin "
          f"bit for bit: {same}", flush=True)

    # ---- (c) the appends: the 16 chunks' K and V into their slots (each chunk is the tail of its sequence)
    kn, vn = rnd(total_q, H, D), rnd(total_q, H, D)
    head = (kn.data_ptr(), vn.data_ptr())
    rest = (cu_q.data_ptr(), table.data_ptr(), sl.data_ptr(), B, H, total_q, CHUNK, D, P, num_pages, mp, H * D, D, P * H * D, D, H * D, mp)
    quant_argv = head + (k8.data_ptr(), v8.data_ptr()) + rest + (BF16, 1.0, 1.0, st)
    copy_argv = head + (k16.data_ptr(), v16.data_ptr()) + rest + (BF16, st)

    def quant():
        return lib.fa_kv_append_paged_quant(*quant_argv)

    def copy():
        return lib.fa_kv_append_paged(*copy_argv)

    ar = ab({"fa_kv_append_paged_quant": quant, "fa_kv_append_paged": copy}, copy)
    rows_bytes = 2 * total_q * H * D  # K and V elements
    for n, r in ar.items():
        r["gb_per_s"] = rows_bytes * (2 + (1 if "quant" in n else 2)) / r["median_us"] / 1e3  # read 2 bytes, write 1 or 2
        print(f"(c) D={D}: {n:30s} of 16 x 512 rows: {r['median_us']:.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f})  {r['gb_per_s']:.0f} GB/s "
              "(cache-resident)", flush=True)
    rc = mid(ar, "fa_kv_append_paged_quant") / mid(ar, "fa_kv_append_paged")
    print(f"(c) D={D}: quantising append / byte-copy append = {rc:.4f}", flush=True)
    out["results"].append(dict(D=D, lens=lens, times=res, kv8_over_twin=ra, kv8_over_widen_plus_bf16=rb, bit_identical=same, append=ar,
                               quant_over_copy=rc))
    del q, k8, v8, k16, v16, kw, vw, o, o2, o3, lse, lse2, lse3, kn, vn
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
