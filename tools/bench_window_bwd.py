#!/usr/bin/env python3
"""fa_bwd_varlen_window next to the un-windowed causal fa_bwd_varlen on the same tensors (the capability before it existed), from one
build: raw C-ABI calls, device events, warm clocks (a spin of --warm-ms in front of every measurement) and interleaved A/B (the
candidates alternate inside every round; a candidate's figure is the median over the rounds of its time per call), the method of
tools/bench_window.py. bf16, 16 heads, 2 sequences of 16384 tokens, D = 64 and 128, wl = 511 / 1023 / 4095 / INT_MAX (wr = 0). Every
candidate runs on the O and LSE its own forward wrote. One call is both kernels (dQ, then dK/dV).
Beside every ratio the tile count predicts: a 128-row (dQ) or 128-key (dK/dV) block walks about (wl + 128) / 64 + 1 tiles under the
window against 128 on average without. wl = INT_MAX is the cost of the second bound over the causal kernels.
Exit status 1 if a wl = 1023 call is not faster than the un-windowed call (the tile skip does not happen).
usage: bench_window_bwd.py [--rounds N] [--iters N] [--warm-ms MS] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import flash_attention_metal_amd as fa

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warm-ms", type=float, default=200.0)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_window_bwd.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, H, N, B, INT_MAX = fa.DTYPES["bf16"], 16, 16384, 2, 2 ** 31 - 1
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


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
ok = True
for D in (64, 128):
    g = torch.Generator(device="cuda").manual_seed(D)

    def rnd(*shape):
        return torch.rand(*shape, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)

    total = B * N
    q, k, v, do = rnd(total, H, D), rnd(total, H, D), rnd(total, H, D), rnd(total, H, D)
    dq, dk, dv = (torch.empty(total, H, D, dtype=torch.float32, device="cuda") for _ in range(3))
    ws = torch.empty(lib.fa_bwd_varlen_workspace_bytes(H, total), dtype=torch.uint8, device="cuda")
    cu = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device="cuda")
    dims = (B, H, H, total, total, N, N, D, D ** -0.5, H * D, D, H * D, D)
    cands, keep = {}, []
    for name in ("causal",) + WINDOWS:
        o = torch.empty_like(q)
        lse = torch.empty(H, total, dtype=torch.float32, device="cuda")
        keep += [o, lse]
        fwd = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), cu.data_ptr()) + dims
        bwd = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
               ws.data_ptr(), cu.data_ptr(), cu.data_ptr()) + dims
        if name == "causal":
            assert lib.fa_fwd_varlen(*fwd, 1, BF16, st) == 0, lib.fa_last_error()
            cands[name] = lambda bwd=bwd: lib.fa_bwd_varlen(*bwd, 1, BF16, st)
        else:
            assert lib.fa_fwd_varlen_window(*fwd, name, 0, BF16, st) == 0, lib.fa_last_error()
            cands[name] = lambda bwd=bwd, w=name: lib.fa_bwd_varlen_window(*bwd, w, 0, BF16, st)
    torch.cuda.synchronize()
    res = ab(cands, cands[511])
    rows = {}
    for n, r in res.items():
        ratio = r["median_us"] / res["causal"]["median_us"]
        pred = None if n in ("causal", INT_MAX) else ((n + 128) / 64 + 1) / 128
        rows[str(n)] = dict(r, ratio=ratio, predicted=pred)
        print(f"fa_bwd_varlen_window, 2 x 16384 tokens D={D}: {str(n):>12s} {r['median_us']:9.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f})  "
              f"ratio to the un-windowed causal call {ratio:.3f}" + (f"  (tile count predicts {pred:.3f})" if pred else ""), flush=True)
    if not res[1023]["max_us"] < res["causal"]["min_us"]:
        ok = False
        print(f"D={D}: a wl = 1023 call is not faster than the un-windowed call", flush=True)
    out["results"].append(dict(D=D, varlen_backward=rows))
    del q, k, v, do, dq, dk, dv, ws, keep, cands
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
sys.exit(0 if ok else 1)
