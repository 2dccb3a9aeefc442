#!/usr/bin/env python3
"""fa_bwd_mla_sparse next to fa_fwd_mla_decode_sparse and the torch gather-plus-autograd formulation, ON THE SAME INPUTS, in the manner of
tools/bench_mla_indexer_select_split.py: device events, warm clocks (a spin of --warm-ms in front of every measurement), interleaved
rounds, and EVERY candidate measured TWICE under two names (x and x'): the ratio of a call to its own second copy is the noise a ratio
between two candidates has to beat. bf16, pages of 64, a pool of --slots rows, lists of topk distinct random slots, full counts.
  bwd      fa_bwd_mla_sparse into preallocated dq / dkv (dkv is accumulated into: it is not re-zeroed between calls)
  fwd      fa_fwd_mla_decode_sparse
  torch    gather rows [T, topk, 576], scores, softmax, O, and autograd's backward of it (forward + backward; only where --torch-max-T allows:
           the gathered rows and the probabilities are materialised)
The share of the five products' FLOPs is against --peak-tflops (dense bf16 matrix peak of the device).
usage: bench_mla_sparse_bwd.py [--rounds N] [--iters N] [--warm-ms MS] [--shapes T:Hq:topk,...] [--torch-max-T T] [--json FILE]"""
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
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--warm-ms", type=float, default=30.0)
ap.add_argument("--shapes", default="4096:128:2048,1024:128:2048")
ap.add_argument("--slots", type=int, default=65536)
ap.add_argument("--torch-max-T", type=int, default=1024)
ap.add_argument("--peak-tflops", type=float, default=2500.0)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_sparse_bwd.py measures on the GPU: none found")
fa.load_library()
P, DQK, DV, SCALE = 64, 576, 512, 192.0 ** -0.5


def ab(cands, warm):
    """{name: median us per call} of callables measured in alternation behind a spin that keeps the clocks up; each one twice"""
    cands = {n + c: f for n, f in cands.items() for c in ("", "'")}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n in cands}
    for r in range(args.rounds):
        order = list(cands)
        for name in order[r % len(order):] + order[:r % len(order)]:
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
    return {n: statistics.median(t) for n, t in times.items()}


def shape(T, Hq, topk):
    g = torch.Generator(device="cuda").manual_seed(36)
    q = torch.randn(T, Hq, DQK, device="cuda", generator=g).to(torch.bfloat16)
    pool = torch.randn(args.slots // P, P, DQK, device="cuda", generator=g).to(torch.bfloat16)
    do = torch.randn(T, Hq, DV, device="cuda", generator=g).to(torch.bfloat16)
    idx = torch.stack([torch.randperm(args.slots, device="cuda", generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    o, lse = torch.empty_like(do), torch.empty(T, Hq, device="cuda")
    ws_f = torch.empty(fa.mla_decode_sparse_workspace_bytes(T, Hq, DV, topk), dtype=torch.uint8, device="cuda")
    ws_b = torch.empty(fa.mla_sparse_backward_workspace_bytes(T, Hq), dtype=torch.uint8, device="cuda")
    dq, dkv = torch.empty(T, Hq, DQK, device="cuda"), torch.zeros(args.slots // P, P, DQK, device="cuda")
    fwd = lambda: fa.flash_attention_mla_decode_sparse(q, pool, idx, SCALE, out=o, lse=lse, workspace=ws_f)
    bwd = lambda: fa.flash_attention_mla_sparse_backward(q, pool, o, do, lse, idx, scale=SCALE, dq=dq, dkv=dkv, workspace=ws_b)
    fwd()
    cands = {"bwd": bwd, "fwd": fwd}
    if T <= args.torch_max_T:
        qg, pg = q.clone().requires_grad_(), pool.clone().requires_grad_()

        def torch_route():
            qg.grad = pg.grad = None
            rows = pg.view(-1, DQK)[idx.long()]
            p = torch.softmax(torch.einsum("thd,tkd->thk", qg, rows).float() * SCALE, -1).to(torch.bfloat16)
            torch.einsum("thk,tkd->thd", p, rows[..., :DV]).backward(do)

        cands["torch"] = torch_route
    res = ab(cands, fwd)
    noise = max(abs(res[n] / res[n + "'"] - 1) for n in cands)
    flops = 2.0 * T * Hq * topk * (3 * DQK + 2 * DV)  # S, dQ, dK over 576 columns; dP, dV over 512
    r = dict(T=T, Hq=Hq, topk=topk, us=res, noise=noise, bwd_tflops=flops / res["bwd"] / 1e6, bwd_share_of_peak=flops / res["bwd"] / 1e6 / args.peak_tflops,
             bwd_vs_fwd=res["bwd"] / res["fwd"], bwd_vs_torch=(res["bwd"] / res["torch"] if "torch" in res else None))
    print(f"T={T} Hq={Hq} topk={topk}: " + ", ".join(f"{n} {res[n]:10.1f}" for n in res) + f" us | bwd {r['bwd_tflops']:.1f} TFLOP/s "
          f"({100 * r['bwd_share_of_peak']:.1f} % of {args.peak_tflops:.0f}), bwd / fwd {r['bwd_vs_fwd']:.2f}"
          + (f", bwd / torch (fwd + bwd) {r['bwd_vs_torch']:.3f}" if "torch" in res else "") + f", a call against its own copy within {noise * 100:.1f} %",
          flush=True)
    return r


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, page_size=P, slots=args.slots, results=[])
for T, Hq, topk in [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",") if s]:
    out["results"].append(shape(T, Hq, topk))
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
