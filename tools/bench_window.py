#!/usr/bin/env python3
"""The sliding-window entry points next to the un-windowed causal calls on the same tensors (the capability before they existed), from one
build: raw C-ABI calls, device events, warm clocks (a spin of --warm-ms in front of every measurement) and interleaved A/B (the
candidates alternate inside every round; a candidate's figure is the median over the rounds of its time per call), the method of
tools/bench_varlen_paged.py. bf16, 16 query heads, D = 64 and 128:
  (a) fa_fwd_varlen_window at wl = 511 / 1023 / 4095 / INT_MAX (wr = 0) against fa_fwd_varlen causal: 2 prompts of 16384 tokens;
  (b) fa_fwd_varlen_paged_window against fa_fwd_varlen_paged causal: the same prompts on a P = 16 pool dealt in a random order;
  (c) fa_fwd_decode_paged_window against fa_fwd_decode_paged causal: 16 sequences x 16384 keys, 4 key heads, one query each.
Beside every ratio the tile count predicts: a 128-row block walks about (wl + 128) / 64 + 1 tiles under the window against 128 on average
without; a decode step ceil((wl + 1) / 64) + 1 tiles of 256. wl = INT_MAX is the cost of the second bound.
usage: bench_window.py [--rounds N] [--iters N] [--warm-ms MS] [--json FILE]"""
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
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_window.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, H, P, N, B, INT_MAX = fa.DTYPES["bf16"], 16, 16, 16384, 2, 2 ** 31 - 1
WINDOWS = (511, 1023, 4095, INT_MAX)


def ab(cands, warm):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in cands.values():
        for _ in range(2):
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


def report(what, D, res, base, predict):
    rows = {}
    for n, r in res.items():
        ratio = r["median_us"] / res[base]["median_us"]
        pred = predict(n)
        rows[str(n)] = dict(r, ratio=ratio, predicted=pred)
        print(f"{what} D={D}: {str(n):>12s} {r['median_us']:9.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f})  ratio to the un-windowed causal call "
              f"{ratio:.3f}" + (f"  (tile count predicts {pred:.3f})" if pred else ""), flush=True)
    return rows


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
for D in (64, 128):
    g = torch.Generator(device="cuda").manual_seed(D)

    def rnd(*shape):
        return torch.rand(*shape, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)

    total = B * N
    q, k, v = rnd(total, H, D), rnd(total, H, D), rnd(total, H, D)
    o = torch.empty_like(q)
    lse = torch.empty(H, total, dtype=torch.float32, device="cuda")
    cu = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device="cuda")
    pre = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), cu.data_ptr(), B, H, H, total, total, N, N, D,
           D ** -0.5, H * D, D, H * D, D)
    cands = {"causal": lambda: lib.fa_fwd_varlen(*pre, 1, BF16, st)}
    for w in WINDOWS:
        cands[w] = lambda w=w: lib.fa_fwd_varlen_window(*pre, w, 0, BF16, st)
    tiles = lambda n: None if n in ("causal", INT_MAX) else ((n + 128) / 64 + 1) / 128
    ra = report("(a) fa_fwd_varlen_window, 2 x 16384 tokens", D, ab(cands, cands["causal"]), "causal", tiles)

    # (b) the same keys in a P = 16 pool (NHD), pages in a random order
    mp = N // P
    num_pages = B * mp + 8
    perm = np.random.default_rng(1).permutation(num_pages)[:B * mp]
    kpool, vpool = rnd(num_pages, P, H, D), rnd(num_pages, P, H, D)
    kpool.view(num_pages * P, H, D)[torch.from_numpy(np.repeat(perm.astype(np.int64) * P, P) + np.tile(np.arange(P), B * mp)).cuda()] = k
    table = torch.from_numpy(perm.reshape(B, mp).astype(np.int32)).cuda()
    sl = torch.full((B,), N, dtype=torch.int32, device="cuda")
    pre = (q.data_ptr(), kpool.data_ptr(), vpool.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), table.data_ptr(), sl.data_ptr(), B, H, H,
           total, N, D, P, num_pages, mp, D ** -0.5, H * D, D, P * H * D, D, H * D, mp)
    cands = {"causal": lambda: lib.fa_fwd_varlen_paged(*pre, 1, BF16, st)}
    for w in WINDOWS:
        cands[w] = lambda w=w: lib.fa_fwd_varlen_paged_window(*pre, w, 0, BF16, st)
    rb = report("(b) fa_fwd_varlen_paged_window, 2 x 16384 tokens, P=16", D, ab(cands, cands["causal"]), "causal", tiles)
    del q, k, v, o, lse, kpool, vpool

    # (c) decode: 16 sequences x 16384 keys, 16 query heads on 4 key heads, one query each
    Bd, Hkv = 16, 4
    num_pages = Bd * mp + 8
    kpool, vpool = rnd(num_pages, P, Hkv, D), rnd(num_pages, P, Hkv, D)
    table = torch.from_numpy(np.random.default_rng(2).permutation(num_pages)[:Bd * mp].reshape(Bd, mp).astype(np.int32)).cuda()
    sl = torch.full((Bd,), N, dtype=torch.int32, device="cuda")
    qd = rnd(Bd, H, 1, D)
    od = torch.empty_like(qd)
    ld = torch.empty(Bd, H, 1, dtype=torch.float32, device="cuda")
    wsb = lib.fa_fwd_decode_paged_workspace_bytes(Bd, H, Hkv, 1, D, P, mp)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    pre = (qd.data_ptr(), kpool.data_ptr(), vpool.data_ptr(), od.data_ptr(), ld.data_ptr(), table.data_ptr(), sl.data_ptr(), Bd, H, Hkv, 1, D, P,
           num_pages, mp, D ** -0.5, H * D, D, P * Hkv * D, D, Hkv * D, mp)
    post = (BF16, BF16, ws.data_ptr(), wsb, st)
    cands = {"causal": lambda: lib.fa_fwd_decode_paged(*pre, 1, *post)}
    for w in WINDOWS:
        cands[w] = lambda w=w: lib.fa_fwd_decode_paged_window(*pre, w, 0, *post)
    rc = report("(c) fa_fwd_decode_paged_window, 16 x 16384 keys", D, ab(cands, cands["causal"]), "causal",
                lambda n: None if n in ("causal", INT_MAX) else (-(-(n + 1) // 64) + 1) / 256)
    out["results"].append(dict(D=D, varlen=ra, varlen_paged=rb, decode_paged=rc))
    del kpool, vpool, qd, od, ld, ws
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
