#!/usr/bin/env python3
"""fa_mla_indexer_k_append_paged_quant and fa_mla_indexer_q_quant next to the eager torch recipe callers run today, ON THE SAME INPUTS, in
the manner of tools/bench_mla_indexer_select_split.py: raw C-ABI calls, device events, warm clocks (a spin of --warm-ms in front of
every measurement) and interleaved rounds. EVERY candidate is measured TWICE under two names (x and x'): the ratio of a call to its own
second copy is the noise a ratio between two candidates has to beat. bf16, Hi = 64, pages of 64, rotate = 1.
  k_append    fa_mla_indexer_k_append_paged_quant         k_today   upcast, Hadamard matmul, amax, power-of-two scale, cast, scatter
  q_quant     fa_mla_indexer_q_quant                      q_today   the same on [T, Hi, 128], and w = head_w * w_mul * s
  stage       both library calls                          today     both torch chains
Shapes: a decode step (B sequences, one token each, --ctx keys behind them) and a prefill chunk (one sequence of T tokens).
The torch chain rounds the rotation differently (one matmul), so its bytes are compared as a share of equal codes, not asserted.
usage: bench_mla_indexer_quant.py [--rounds N] [--iters N] [--warm-ms MS] [--decode B,...] [--prefill T,...] [--ctx L] [--json FILE]"""
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
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warm-ms", type=float, default=30.0)
ap.add_argument("--decode", default="64")
ap.add_argument("--prefill", default="4096")
ap.add_argument("--ctx", type=int, default=4096)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_indexer_quant.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, HI, DI, P = fa.DTYPES["bf16"], 64, 128, 64
W_MUL = DI ** -0.5 * HI ** -0.5  # the softmax scale and Hi^-0.5, folded as callers do


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


def shape(kind, B, n, ctx):
    """B sequences that each append n tokens behind ctx keys"""
    g = torch.Generator(device="cuda").manual_seed(36)
    T, mp = B * n, -(-(ctx + n) // P)
    num_pages = B * mp
    k_new = torch.randn(T, DI, device="cuda", generator=g).to(torch.bfloat16)
    q = torch.randn(T, HI, DI, device="cuda", generator=g).to(torch.bfloat16)
    hw = torch.randn(T, HI, device="cuda", generator=g).abs_()
    bt = torch.randperm(num_pages, device="cuda", generator=g).to(torch.int32).view(B, mp)
    cu = torch.arange(B + 1, device="cuda", dtype=torch.int32) * n
    sk = torch.full((B,), ctx + n, device="cuda", dtype=torch.int32)
    pool, ks = torch.zeros(num_pages, P, DI, dtype=torch.uint8, device="cuda"), torch.zeros(num_pages, P, device="cuda")
    pool_t, ks_t = torch.zeros_like(pool), torch.zeros_like(ks)
    q8, w8 = torch.empty(T, HI, DI, dtype=torch.uint8, device="cuda"), torch.empty(T, HI, device="cuda")
    a_k = (k_new.data_ptr(), pool.data_ptr(), ks.data_ptr(), cu.data_ptr(), bt.data_ptr(), sk.data_ptr(), B, T, n, DI, P, num_pages, mp, DI, P * DI, DI,
           P, mp, 1, BF16, st)
    a_q = (q.data_ptr(), hw.data_ptr(), q8.data_ptr(), w8.data_ptr(), T, HI, DI, W_MUL, HI * DI, DI, HI, HI * DI, DI, HI, 1, BF16, st)

    def call(fn, a):
        assert fn(*a) == 0, lib.fa_last_error()

    k_append = lambda: call(lib.fa_mla_indexer_k_append_paged_quant, a_k)
    q_quant = lambda: call(lib.fa_mla_indexer_q_quant, a_q)
    had = ((-1.0) ** torch.tensor([[bin(a & b).count("1") for b in range(DI)] for a in range(DI)], device="cuda")).float() * DI ** -0.5
    pos = (ctx + torch.arange(n, device="cuda")).repeat(B)  # the scatter's slots through the block table, as an engine computes them per step
    seq = torch.arange(B, device="cuda").repeat_interleave(n)

    def quant(x):
        y = x.float() @ had
        s = torch.exp2(torch.ceil(torch.log2(y.abs().amax(-1, keepdim=True).clamp_min(1e-30) / 448.0)).clamp_(-32, 32))
        return (y / s).clamp_(-448.0, 448.0).to(torch.float8_e4m3fn), s

    def k_today():
        c, s = quant(k_new)
        slot = bt[seq, pos // P].long() * P + pos % P
        pool_t.view(-1, DI)[slot] = c.view(torch.uint8)
        ks_t.view(-1)[slot] = s[:, 0]

    out_t = {}

    def q_today():
        c, s = quant(q)
        out_t["q"], out_t["w"] = c, hw * W_MUL * s[..., 0]

    k_append(), q_quant(), k_today(), q_today()
    torch.cuda.synchronize()
    same = float((pool.view(-1) == pool_t.view(-1)).float().mean()), float((q8 == out_t["q"].view(torch.uint8)).float().mean())
    res = ab({"k_append": k_append, "k_today": k_today, "q_quant": q_quant, "q_today": q_today, "stage": lambda: (k_append(), q_quant()),
              "today": lambda: (k_today(), q_today())}, q_quant)
    names = [x for x in res if not x.endswith("'")]
    noise = max(abs(res[x] / res[x + "'"] - 1) for x in names)
    moved = T * (DI * 3 + 4) + T * HI * (DI * 3 + 8)  # bytes the stage has to read and write
    r = dict(kind=kind, B=B, tokens_per_seq=n, ctx=ctx, us=res, noise=noise, k_vs_today=res["k_append"] / res["k_today"],
             q_vs_today=res["q_quant"] / res["q_today"], stage_vs_today=res["stage"] / res["today"], stage_gb_per_s=moved / res["stage"] * 1e-3,
             equal_codes_k=same[0], equal_codes_q=same[1])
    print(f"{kind} B={B} n={n}: " + ", ".join(f"{x} {res[x]:8.1f}" for x in names) + f" us | k / today {r['k_vs_today']:.3f}, q / today "
          f"{r['q_vs_today']:.3f}, stage / today {r['stage_vs_today']:.3f}, stage {r['stage_gb_per_s']:.0f} GB/s of its own bytes, equal codes "
          f"k {same[0]:.4f} q {same[1]:.4f}, a call against its own copy within {noise * 100:.1f} %", flush=True)
    return r


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, Hi=HI, page_size=P, results=[])
for b in [int(x) for x in args.decode.split(",") if x]:
    out["results"].append(shape("decode", b, 1, args.ctx))
for t in [int(x) for x in args.prefill.split(",") if x]:
    out["results"].append(shape("prefill", 1, t, 0))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
