#!/usr/bin/env python3
"""fa_mla_indexer_select_split next to fa_mla_indexer_select and the torch route, ON THE SAME INPUTS, in the manner of
tools/bench_mla_indexer.py: raw C-ABI calls, device events, warm clocks (a spin of --warm-ms in front of every measurement) and
interleaved rounds. EVERY candidate is measured TWICE under two names (x and x'): the ratio of a call to its own second copy is the
noise a ratio between two candidates has to beat. bf16, Hi = 64, topk = 2048, pages of 64, decode steps (Lq_b = 1) of B sequences of L keys.
  split       fa_mla_indexer_select_split at fa_mla_indexer_select_num_splits (--splits S,...: further candidates split@S)
  select      fa_mla_indexer_select, on the same logits
  topk        fa_mla_indexer_topk_paged            topk_split  fa_mla_indexer_logits_paged, then the split select
  today       round 32's torch route: gather, bf16 matmul, relu, weighted head sum, torch.topk, slots
The lists of split and select are compared bit for bit on every shape (asserted).
usage: bench_mla_indexer_select_split.py [--rounds N] [--iters N] [--warm-ms MS] [--decode B:L,...] [--splits S,...] [--json FILE]"""
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
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warm-ms", type=float, default=30.0)
ap.add_argument("--decode", default=",".join(f"{b}:{l}" for b in (1, 16, 128) for l in (4 * K, 32 * K, 128 * K)))
ap.add_argument("--splits", default="")
ap.add_argument("--torch-block", type=int, default=128)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_indexer_select_split.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, HI, DI, P, TOPK = fa.DTYPES["bf16"], 64, 128, 64, 2048


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


def shape(B, L):
    g = torch.Generator(device="cuda").manual_seed(35)
    T, mp = B, -(-L // P)
    num_pages, cap = B * mp, mp * P
    q = torch.randn(T, HI, DI, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(T, HI, device="cuda", generator=g).abs_().mul_(DI ** -0.5 / HI)
    k = torch.randn(num_pages, P, DI, device="cuda", generator=g).to(torch.bfloat16)
    bt = torch.randperm(num_pages, device="cuda", generator=g).to(torch.int32).view(B, mp)
    cu = torch.arange(B + 1, device="cuda", dtype=torch.int32)
    sk = torch.full((B,), L, device="cuda", dtype=torch.int32)
    idx, idx1 = (torch.full((T, TOPK), -7, device="cuda", dtype=torch.int32) for _ in range(2))
    cnt, cnt1 = (torch.full((T,), -7, device="cuda", dtype=torch.int32) for _ in range(2))
    rec = lib.fa_mla_indexer_select_num_splits(B, 1, P, mp)
    front = lib.fa_mla_indexer_topk_paged_workspace_bytes(T, P, mp)
    ws = torch.empty(front + lib.fa_mla_indexer_select_split_workspace_bytes(T, 64), dtype=torch.uint8, device="cuda")
    a_log = (q.data_ptr(), w.data_ptr(), k.data_ptr(), ws.data_ptr(), cu.data_ptr(), bt.data_ptr(), sk.data_ptr(), B, HI, T, 1, DI, P, num_pages, mp,
             HI * DI, DI, HI, P * DI, DI, mp, cap, BF16, st)
    sel = lambda i, c: (ws.data_ptr(), i.data_ptr(), c.data_ptr(), cu.data_ptr(), bt.data_ptr(), sk.data_ptr(), B, T, 1, TOPK, P, num_pages, mp, cap, TOPK, mp)
    a_sel = sel(idx1, cnt1) + (st,)
    a_spl = lambda S: sel(idx, cnt) + (S, ws.data_ptr() + front, lib.fa_mla_indexer_select_split_workspace_bytes(T, S), st)
    a_top = (q.data_ptr(), w.data_ptr(), k.data_ptr(), idx.data_ptr(), cnt.data_ptr(), cu.data_ptr(), bt.data_ptr(), sk.data_ptr(), B, HI, T, 1, DI, TOPK,
             P, num_pages, mp, HI * DI, DI, HI, P * DI, DI, mp, TOPK, BF16, ws.data_ptr(), front, st)

    def call(fn, a):
        assert fn(*a) == 0, lib.fa_last_error()

    logits = lambda: call(lib.fa_mla_indexer_logits_paged, a_log)
    split = lambda S: (lambda: call(lib.fa_mla_indexer_select_split, a_spl(S)))
    tidx = torch.empty(T, TOPK, device="cuda", dtype=torch.int64)

    def today():
        keys = k[bt.long()].view(B, cap, DI)[:, :L]  # the gather through the block table
        for r0 in range(0, B, args.torch_block):
            rows = slice(r0, min(r0 + args.torch_block, B))
            dots = torch.bmm(q[rows], keys[rows].transpose(1, 2))
            top = torch.topk((torch.relu_(dots).float() * w[rows, :, None]).sum(1), TOPK, dim=-1).indices
            tidx[rows] = bt[rows].long().gather(1, top // P) * P + top % P

    logits()
    call(lib.fa_mla_indexer_select, a_sel)
    for S in sorted({rec} | {int(s) for s in args.splits.split(",") if s}):  # the lists of every split count against the select's
        idx.fill_(-7)
        split(S)()
        torch.cuda.synchronize()
        assert torch.equal(idx, idx1) and torch.equal(cnt, cnt1), (B, L, S)
    cands = {"split": split(rec), "select": lambda: call(lib.fa_mla_indexer_select, a_sel), "topk": lambda: call(lib.fa_mla_indexer_topk_paged, a_top),
             "topk_split": lambda: (logits(), split(rec)()), "today": today}
    cands.update({f"split@{s}": split(int(s)) for s in args.splits.split(",") if s})
    res = ab(cands, logits)
    noise = max(abs(res[n] / res[n + "'"] - 1) for n in cands)
    r = dict(B=B, L=L, num_splits=rec, us=res, noise=noise, split_vs_select=res["split"] / res["select"],
             topk_split_vs_topk=res["topk_split"] / res["topk"], topk_split_vs_today=res["topk_split"] / res["today"])
    print(f"decode B={B} L={L} S={rec}: " + ", ".join(f"{n} {res[n]:8.1f}" for n in res) + f" us | split / select {r['split_vs_select']:.3f}, "
          f"topk_split / topk {r['topk_split_vs_topk']:.3f}, topk_split / today {r['topk_split_vs_today']:.3f}, a call against its own copy "
          f"within {noise * 100:.1f} %", flush=True)
    return r


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, Hi=HI, topk=TOPK, page_size=P, results=[])
for B, L in [tuple(int(x) for x in p.split(":")) for p in args.decode.split(",") if p]:
    out["results"].append(shape(B, L))
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
