#!/usr/bin/env python3
"""fa_mla_indexer_topk_paged and its two stages next to what a caller does without them, ON THE SAME INPUTS, in the manner of
tools/bench_mla_decode_sparse.py: raw C-ABI calls, device events, warm clocks (a spin of --warm-ms in front of every measurement) and
interleaved rounds (the candidates alternate inside every round; a figure is the median over the rounds of the time per call).
bf16, Hi = 64, topk = 2048, pages of 64 under a shuffled block table. Candidates:
  topk    fa_mla_indexer_topk_paged (both stages on the workspace)
  logits  fa_mla_indexer_logits_paged alone        select  fa_mla_indexer_select alone, on the logits of the line above
  today   the torch chain: gather of the index keys through the block table, bf16 matmul over the 64 heads, relu, fp32 weighted head
          sum, the causal mask, torch.topk, and the gather that turns positions into slots (tokens in blocks of --torch-block rows)
Shapes: decode steps (Lq_b = 1) over B sequences of L keys, and prefill chunks of one sequence (Lq tokens appended to L keys).
Per shape: us per call of each, topk / today, the decode logits stage's bytes of k_idx over its time next to the HBM peak, and the lists
of the two routes compared as SETS per token (the torch route rounds every dot to bf16, so near-ties may differ: the share of tokens
with equal sets and the mean overlap are reported, not asserted).
usage: bench_mla_indexer.py [--rounds N] [--iters N] [--warm-ms MS] [--decode B:L,...] [--prefill Lq:L,...] [--json FILE]"""
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
ap.add_argument("--torch-block", type=int, default=128)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_indexer.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, HI, DI, P, TOPK, HBM_TBS = fa.DTYPES["bf16"], 64, 128, 64, 2048, 8.0  # (HBM3E peak of one MI355X: 8 TB/s)


def ab(cands, warm):
    """{name: median us per call} of callables measured in alternation behind a spin that keeps the clocks up"""
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


def shape(kind, B, Lq, L):
    g = torch.Generator(device="cuda").manual_seed(32)
    T, mp = B * Lq, -(-L // P)
    num_pages = B * mp
    q = torch.randn(T, HI, DI, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.randn(T, HI, device="cuda", generator=g).abs_().mul_(DI ** -0.5 / HI)
    k = torch.randn(num_pages, P, DI, device="cuda", generator=g).to(torch.bfloat16)
    bt = torch.randperm(num_pages, device="cuda", generator=g).to(torch.int32).view(B, mp)
    cu = torch.arange(B + 1, device="cuda", dtype=torch.int32) * Lq
    sk = torch.full((B,), L, device="cuda", dtype=torch.int32)
    idx = torch.empty(T, TOPK, device="cuda", dtype=torch.int32)
    cnt = torch.empty(T, device="cuda", dtype=torch.int32)
    need = lib.fa_mla_indexer_topk_paged_workspace_bytes(T, P, mp)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    cap = mp * P
    a_log = (q.data_ptr(), w.data_ptr(), k.data_ptr(), ws.data_ptr(), cu.data_ptr(), bt.data_ptr(), sk.data_ptr(), B, HI, T, Lq, DI, P, num_pages, mp,
             HI * DI, DI, HI, P * DI, DI, mp, cap, BF16, st)
    a_sel = (ws.data_ptr(), idx.data_ptr(), cnt.data_ptr(), cu.data_ptr(), bt.data_ptr(), sk.data_ptr(), B, T, Lq, TOPK, P, num_pages, mp, cap, TOPK, mp, st)
    a_top = (q.data_ptr(), w.data_ptr(), k.data_ptr(), idx.data_ptr(), cnt.data_ptr(), cu.data_ptr(), bt.data_ptr(), sk.data_ptr(), B, HI, T, Lq, DI, TOPK,
             P, num_pages, mp, HI * DI, DI, HI, P * DI, DI, mp, TOPK, BF16, ws.data_ptr(), need, st)

    def call(fn, a):
        assert fn(*a) == 0, lib.fa_last_error()

    pos = torch.arange(L, device="cuda")
    tidx = torch.empty(T, TOPK, device="cuda", dtype=torch.int64)

    def today():
        keys = k[bt.long()].view(B, cap, DI)[:, :L]  # the gather through the block table
        for b in range(B if Lq > 1 else 1):
            for r0 in range(0, Lq if Lq > 1 else B, args.torch_block):
                if Lq > 1:  # a block of one sequence's tokens against its keys
                    rows = slice(b * Lq + r0, b * Lq + min(r0 + args.torch_block, Lq))
                    dots = torch.matmul(q[rows].view(-1, DI), keys[b].t()).view(-1, HI, L)
                    vis = L - Lq + torch.arange(rows.start - b * Lq, rows.stop - b * Lq, device="cuda") + 1
                    table = bt[b].long().expand(rows.stop - rows.start, mp)
                else:       # a block of decode tokens, one per sequence
                    rows = slice(r0, min(r0 + args.torch_block, B))
                    dots = torch.bmm(q[rows], keys[rows].transpose(1, 2))
                    vis, table = None, bt[rows].long()
                logit = (torch.relu_(dots).float() * w[rows, :, None]).sum(1)
                if vis is not None:
                    logit.masked_fill_(pos[None, :] >= vis[:, None], float("-inf"))
                top = torch.topk(logit, TOPK, dim=-1).indices
                tidx[rows] = table.gather(1, top // P) * P + top % P

    res = ab({"topk": lambda: call(lib.fa_mla_indexer_topk_paged, a_top), "logits": lambda: call(lib.fa_mla_indexer_logits_paged, a_log),
              "select": lambda: call(lib.fa_mla_indexer_select, a_sel), "today": today}, lambda: call(lib.fa_mla_indexer_logits_paged, a_log))
    call(lib.fa_mla_indexer_topk_paged, a_top)
    today()
    torch.cuda.synchronize()
    mine, theirs, counts = idx.cpu().numpy(), tidx.cpu().numpy(), cnt.cpu().numpy()
    full = [t for t in range(T) if counts[t] == TOPK]  # (tokens that see fewer than topk keys: torch.topk has no count to compare)
    over = [len(set(mine[t]) & set(theirs[t])) / TOPK for t in full]
    r = dict(kind=kind, B=B, Lq=Lq, L=L, us=res, topk_vs_today=res["topk"] / res["today"], tokens_compared=len(full),
             equal_sets=sum(o == 1.0 for o in over) / max(1, len(over)), mean_overlap=sum(over) / max(1, len(over)))
    line = f"{kind} B={B} Lq={Lq} L={L}: " + ", ".join(f"{n} {res[n]:9.1f} us" for n in res) + f" | topk / today {r['topk_vs_today']:.3f}"
    if kind == "decode":
        r["logits_k_bytes"], r["logits_tbs"] = B * L * DI * 2, B * L * DI * 2 / res["logits"] * 1e-6
        line += f" | logits stage {r['logits_tbs']:.2f} TB/s of k_idx (HBM peak {HBM_TBS:.0f})"
    print(line + f" | equal sets {r['equal_sets'] * 100:.0f} % of {len(full)} tokens, mean overlap {r['mean_overlap'] * 100:.2f} %", flush=True)
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
