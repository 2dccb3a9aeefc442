#!/usr/bin/env python3
"""fa_mla_indexer_logits_paged_kv8 next to what a caller of an e4m3 index cache does without it, ON THE SAME KEY VALUES, in the manner of
tools/bench_mla_indexer.py: raw C-ABI calls, device events, warm clocks (a spin of --warm-ms in front of every measurement) and
interleaved rounds (the candidates alternate inside every round and each is measured TWICE per round; a figure is the median over all of
a candidate's measurements of the time per call). Hi = 64, pages of 64 under a shuffled block table, round 32's shapes. Candidates:
  kv8     fa_mla_indexer_logits_paged_kv8 on the e4m3 pool and its per-key scales
  again   the same call a second time: |kv8 - again| / kv8 is the NOISE figure of the shape
  floor   fa_mla_indexer_logits_paged in bf16 on the pool dequantised BEFOREHAND (k * k_scale, in bf16) and the query widened beforehand
  today   a torch dequantise of the whole pool to bf16 (widen, multiply by the scale, round) plus the floor call
  topk8 / topk16   the composites (logits + the unchanged select, topk = 2048) over the e4m3 pool and over the dequantised pool
Per shape: us per call of each, kv8 / floor and kv8 / today, and the logits stages' key bytes over their time (128 + 4 bytes a key for
kv8, 256 for floor) next to the HBM peak. The logits of kv8 and floor are compared on the visible columns (the bf16 pool rounds k * scale
to 8 bits, so they differ in the third digit: the largest difference relative to the largest logit is reported, not asserted).
usage: bench_mla_indexer_kv8.py [--rounds N] [--iters N] [--warm-ms MS] [--decode B:L,...] [--prefill Lq:L,...] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import flash_attention_metal_amd as fa

K = 1024
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--warm-ms", type=float, default=50.0)
ap.add_argument("--decode", default=",".join(f"{b}:{l}" for b in (1, 16, 128) for l in (4 * K, 32 * K, 128 * K)))
ap.add_argument("--prefill", default=",".join(f"{q}:{l}" for q in (512, 2048) for l in (8 * K, 64 * K)))
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_indexer_kv8.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, FP8, HI, DI, P, TOPK, HBM_TBS = fa.DTYPES["bf16"], fa.DTYPES["fp8_e4m3"], 64, 128, 64, 2048, 8.0  # (HBM3E peak of one MI355X: 8 TB/s)


def ab(cands, warm):
    """{name: median us per call} of callables measured in alternation, twice a round, behind a spin that keeps the clocks up"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n in cands}
    for r in range(args.rounds):
        order = list(cands)
        for name in 2 * (order[r % len(order):] + order[:r % len(order)]):
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


def shape(kind, B, Lq, L):
    g = torch.Generator(device="cuda").manual_seed(33)
    T, mp = B * Lq, -(-L // P)
    num_pages, cap = B * mp, mp * P
    q8 = torch.randn(T, HI, DI, device="cuda", generator=g).to(torch.float8_e4m3fn)
    w = torch.randn(T, HI, device="cuda", generator=g).abs_().mul_(DI ** -0.5 / HI)
    k8 = torch.randn(num_pages, P, DI, device="cuda", generator=g).to(torch.float8_e4m3fn)
    ks = torch.rand(num_pages, P, device="cuda", generator=g) * 2 + 0.25
    q16, k16 = q8.to(torch.bfloat16), torch.empty(num_pages, P, DI, device="cuda", dtype=torch.bfloat16)

    def dequant():
        torch.mul(k8.to(torch.bfloat16), ks.unsqueeze(-1), out=k16)

    dequant()
    bt = torch.randperm(num_pages, device="cuda", generator=g).to(torch.int32).view(B, mp)
    cu = torch.arange(B + 1, device="cuda", dtype=torch.int32) * Lq
    sk = torch.full((B,), L, device="cuda", dtype=torch.int32)
    idx = torch.empty(T, TOPK, device="cuda", dtype=torch.int32)
    cnt = torch.empty(T, device="cuda", dtype=torch.int32)
    need = lib.fa_mla_indexer_topk_paged_workspace_bytes(T, P, mp)
    ws, ws16 = torch.zeros(need, dtype=torch.uint8, device="cuda"), torch.zeros(need, dtype=torch.uint8, device="cuda")
    tabs = (cu.data_ptr(), bt.data_ptr(), sk.data_ptr())
    dims = (B, HI, T, Lq, DI, P, num_pages, mp)
    a_kv8 = (q8.data_ptr(), w.data_ptr(), k8.data_ptr(), ks.data_ptr(), ws.data_ptr(), *tabs, *dims, HI * DI, DI, HI, P * DI, DI, P, mp, cap, FP8, FP8, st)
    a_16 = (q16.data_ptr(), w.data_ptr(), k16.data_ptr(), ws16.data_ptr(), *tabs, *dims, HI * DI, DI, HI, P * DI, DI, mp, cap, BF16, st)
    dimk = (B, HI, T, Lq, DI, TOPK, P, num_pages, mp)
    a_top8 = (q8.data_ptr(), w.data_ptr(), k8.data_ptr(), ks.data_ptr(), idx.data_ptr(), cnt.data_ptr(), *tabs, *dimk, HI * DI, DI, HI, P * DI, DI, P, mp,
              TOPK, FP8, FP8, ws.data_ptr(), need, st)
    a_top16 = (q16.data_ptr(), w.data_ptr(), k16.data_ptr(), idx.data_ptr(), cnt.data_ptr(), *tabs, *dimk, HI * DI, DI, HI, P * DI, DI, mp, TOPK, BF16,
               ws16.data_ptr(), need, st)

    def call(fn, a):
        assert fn(*a) == 0, lib.fa_last_error()

    kv8 = lambda: call(lib.fa_mla_indexer_logits_paged_kv8, a_kv8)
    floor = lambda: call(lib.fa_mla_indexer_logits_paged, a_16)

    def today():
        dequant()
        floor()

    res = ab({"kv8": kv8, "again": kv8, "floor": floor, "today": today, "topk8": lambda: call(lib.fa_mla_indexer_topk_paged_kv8, a_top8),
              "topk16": lambda: call(lib.fa_mla_indexer_topk_paged, a_top16)}, kv8)
    kv8()
    floor()
    torch.cuda.synchronize()
    l8, l16 = ws.view(torch.float32).view(T, cap), ws16.view(torch.float32).view(T, cap)
    vis = (torch.arange(cap, device="cuda")[None, :] < (L - Lq + 1 + torch.arange(Lq, device="cuda").repeat(B))[:, None])
    diff = float(((l8 - l16).abs() * vis).max() / (l8.abs() * vis).max())
    kb8, kb16 = B * L * (DI + 4), B * L * DI * 2
    r = dict(kind=kind, B=B, Lq=Lq, L=L, us=res, noise=abs(res["kv8"] - res["again"]) / res["kv8"], kv8_vs_floor=res["kv8"] / res["floor"],
             kv8_vs_today=res["kv8"] / res["today"], kv8_key_bytes=kb8, floor_key_bytes=kb16, kv8_tbs=kb8 / res["kv8"] * 1e-6,
             floor_tbs=kb16 / res["floor"] * 1e-6, max_diff_vs_floor_rel=diff)
    print(f"{kind} B={B} Lq={Lq} L={L}: " + ", ".join(f"{n} {res[n]:9.1f} us" for n in res) + f" | noise {r['noise'] * 100:.1f} % | kv8 / floor "
          f"{r['kv8_vs_floor']:.3f}, kv8 / today {r['kv8_vs_today']:.3f} | key bytes: kv8 {r['kv8_tbs']:.2f} TB/s, floor {r['floor_tbs']:.2f} TB/s (HBM peak "
          f"{HBM_TBS:.0f}) | max |kv8 - floor| / max |logit| {diff:.2e}", flush=True)
    return r


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, Hi=HI, topk=TOPK, page_size=P,
           hbm_peak_tbs=HBM_TBS, results=[])
pairs = lambda s: [tuple(int(x) for x in p.split(":")) for p in s.split(",") if p]
for B, L in pairs(args.decode):
    out["results"].append(shape("decode", B, 1, L))
    torch.cuda.empty_cache()
for Lq, L in pairs(args.prefill):
    out["results"].append(shape("prefill", 1, Lq, L))
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
