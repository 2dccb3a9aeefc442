#!/usr/bin/env python3
"""fa_fwd_varlen_paged next to what a caller could do before it existed, from the same build: raw C-ABI calls, device events, warm
clocks (a spin of --warm-ms in front of every measurement) and interleaved A/B (the candidates alternate inside every round; the
figure of a candidate is the median over the rounds of its time per call). A chunked-prefill step: 16 sequences with 1k-8k cached keys
(seeded; the chunk already appended), chunks of 512 queries, 16 query heads on 16 key heads, bf16, causal, P = 16 pages dealt in a
random order, D = 64 and 128:
  (a) the paged call against fa_fwd_varlen on the PRE-GATHERED dense cache -- the parent's best case: the gather is not counted;
  (b) the paged call against gather + fa_fwd_varlen -- what a caller does today (index_select of the pages, then the call);
  (c) fa_kv_append_paged of the 16 chunks, in GB/s (bytes read + bytes written);
also checks, at the sizes timed, that the paged result equals fa_fwd_varlen on the gathered cache bit for bit.
usage: bench_varlen_paged.py [--rounds N] [--iters N] [--warm-ms MS] [--json FILE]"""
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
    sys.exit("bench_varlen_paged.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, H, P, CHUNK, B = fa.DTYPES["bf16"], 16, 16, 512, 16


def ab(cands, warm):
    """{name: median us per call} of callables measured in alternation, each round behind a spin that keeps the clocks up."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in cands.values():
        for _ in range(3):
            assert fn() == 0, lib.fa_last_error()
    torch.cuda.synchronize()
    times = {n: [] for n in cands}
    for r in range(args.rounds):
        order = list(cands)
        order = order[r % len(order):] + order[:r % len(order)]
        for name in order:
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < args.warm_ms:
                warm()
                torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                cands[name]()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters * 1e3)
    return {n: dict(median_us=statistics.median(t), min_us=min(t), max_us=max(t)) for n, t in times.items()}


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
for D in (64, 128):
    lens = [int(x) for x in np.random.default_rng(0).integers(1024, 8193, B)]
    npb = [(L + P - 1) // P for L in lens]
    mp, num_pages, total_k, total_q = max(npb), sum(npb) + 8, sum(lens), B * CHUNK
    g = torch.Generator(device="cuda").manual_seed(D)

    def rnd(*shape):
        return torch.rand(*shape, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)

    q, kpool_n, vpool_n = rnd(total_q, H, D), rnd(num_pages, P, H, D), rnd(num_pages, P, H, D)  # NHD pools
    perm = np.random.default_rng(1).permutation(num_pages)
    table_h, rows, used = np.zeros((B, mp), np.int32), [], 0
    for b in range(B):
        table_h[b, :npb[b]] = perm[used:used + npb[b]]
        rows.append(np.repeat(perm[used:used + npb[b]].astype(np.int64) * P, P)[:lens[b]] + np.tile(np.arange(P), npb[b])[:lens[b]])
        used += npb[b]
    table, sl = torch.from_numpy(table_h).cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")
    cu_q = torch.arange(0, (B + 1) * CHUNK, CHUNK, dtype=torch.int32, device="cuda")
    cu_k = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).cuda()
    slot = torch.from_numpy(np.concatenate(rows)).cuda()  # the slot (page * P + row) of every key, sequence after sequence
    o, o2 = torch.empty_like(q), torch.empty_like(q)
    lse, lse2 = (torch.empty(H, total_q, dtype=torch.float32, device="cuda") for _ in range(2))
    kd, vd = torch.empty(total_k, H, D, dtype=torch.bfloat16, device="cuda"), torch.empty(total_k, H, D, dtype=torch.bfloat16, device="cuda")

    kflat, vflat = kpool_n.view(num_pages * P, H, D), vpool_n.view(num_pages * P, H, D)

    def gather_nhd():  # [num_pages * P, H, D] -> [total_k, H, D]: one pass over the cache per operand
        torch.index_select(kflat, 0, slot, out=kd)
        torch.index_select(vflat, 0, slot, out=vd)
        return 0

    paged_argv = (q.data_ptr(), kpool_n.data_ptr(), vpool_n.data_ptr(), o.data_ptr(), lse.data_ptr(), cu_q.data_ptr(), table.data_ptr(), sl.data_ptr(),
                  B, H, H, total_q, CHUNK, D, P, num_pages, mp, D ** -0.5, H * D, D, P * H * D, D, H * D, mp, 1, BF16, st)
    dense_argv = (q.data_ptr(), kd.data_ptr(), vd.data_ptr(), o2.data_ptr(), lse2.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), B, H, H, total_q,
                  total_k, CHUNK, max(lens), D, D ** -0.5, H * D, D, H * D, D, 1, BF16, st)

    def paged():
        return lib.fa_fwd_varlen_paged(*paged_argv)

    def dense():
        return lib.fa_fwd_varlen(*dense_argv)

    def gather_dense():
        gather_nhd()
        return lib.fa_fwd_varlen(*dense_argv)

    gather_nhd()
    assert paged() == 0 and dense() == 0, lib.fa_last_error()
    torch.cuda.synchronize()
    same = bool(torch.equal(o, o2) and torch.equal(lse, lse2))
    res = ab({"fa_fwd_varlen_paged": paged, "fa_fwd_varlen, pre-gathered": dense, "gather + fa_fwd_varlen": gather_dense}, dense)
    fl = sum(2.0 * H * D * 2 * (CHUNK * (L - CHUNK) + CHUNK * (CHUNK + 1) / 2) for L in lens)
    for n, r in res.items():
        r["tflops"] = fl / r["median_us"] / 1e6
        print(f"D={D} 16 x 512 queries on 1k-8k cached keys ({total_k} keys), causal bf16, P={P}: {n:30s} {r['median_us']:8.1f} us "
              f"(min {r['min_us']:.1f}, max {r['max_us']:.1f})  {r['tflops']:6.1f} TFLOP/s", flush=True)
    ra = res["fa_fwd_varlen_paged"]["median_us"] / res["fa_fwd_varlen, pre-gathered"]["median_us"]
    rb = res["fa_fwd_varlen_paged"]["median_us"] / res["gather + fa_fwd_varlen"]["median_us"]
    print(f"(a) D={D}: paged / pre-gathered varlen = {ra:.4f}   (b) paged / (gather + varlen) = {rb:.4f}   paged equals varlen on the gathered "
          f"cache bit for bit: {same}", flush=True)

    # ---- (c) the append: the 16 chunks' K and V into their slots (lengths as above: each chunk is the tail of its sequence)
    kn, vn = rnd(total_q, H, D), rnd(total_q, H, D)
    app_argv = (kn.data_ptr(), vn.data_ptr(), kpool_n.data_ptr(), vpool_n.data_ptr(), cu_q.data_ptr(), table.data_ptr(), sl.data_ptr(), B, H,
                total_q, CHUNK, D, P, num_pages, mp, H * D, D, P * H * D, D, H * D, mp, BF16, st)

    def append():
        return lib.fa_kv_append_paged(*app_argv)

    ar = ab({"fa_kv_append_paged": append}, append)["fa_kv_append_paged"]
    nbytes = 2 * 2 * total_q * H * D * 2  # K and V, read and written, two bytes per element
    ar["gb_per_s"] = nbytes / ar["median_us"] / 1e3
    print(f"(c) D={D}: fa_kv_append_paged of 16 x 512 rows: {ar['median_us']:.1f} us (min {ar['min_us']:.1f}, max {ar['max_us']:.1f})  "
          f"{ar['gb_per_s']:.0f} GB/s", flush=True)
    out["results"].append(dict(D=D, lens=lens, times=res, paged_over_pregathered=ra, paged_over_gather_plus_varlen=rb, bit_identical=same, append=ar))
    del q, kpool_n, vpool_n, kflat, vflat, kd, vd, o, o2, lse, lse2, kn, vn
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
