#!/usr/bin/env python3
"""fa_fwd_mla_decode_sparse_kv8 (the absorbed MLA step over a list of slots per token of an e4m3 latent pool) next to the ways of doing
without it, ON THE SAME KEYS and from the same build, on the method of tools/bench_mla_decode_sparse.py: raw C-ABI calls, device events,
warm clocks (a spin of --warm-ms in front of every measurement) and interleaved rounds (the candidates alternate inside every round and
EACH RUNS TWICE per round, as "#1" and "#2": the distance between a call's two copies is the session's own scatter; a figure is the
median over the rounds of the time per call). bf16 queries, topk = 2048 entries per token drawn at random from a pool of --slots slots
(pages of 64), and the same lists sorted; Hq in {16, 64, 128}, T in {1, 16, 128, 1024} tokens. Candidates, checked bit-identical in O
before anything is timed:
  new    fa_fwd_mla_decode_sparse_kv8 on the e4m3 pool and the lists
  floor  fa_fwd_mla_decode_paged_kv8 on the pre-gathered e4m3 twin pool (B = T, Nq = 1, 32 pages of 64 per token): no gather at all
  today  what a caller does without the new call: torch.index_select of the listed 576-byte rows into that twin, then that call
  bf16   fa_fwd_mla_decode_sparse on the pool widened to bf16: what halving the bytes buys under a gather
Per shape: us per call of each, new / floor, new / today and new / bf16, TB/s of the bytes the step needs (T * topk * 576; bf16: twice
that), and each call against its own second copy.
usage: bench_mla_decode_sparse_kv8.py [--rounds N] [--iters N] [--warm-ms MS] [--tokens 1,16,128,1024] [--heads 16,64,128] [--topk N]
                                      [--slots N] [--json FILE]"""
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
ap.add_argument("--warm-ms", type=float, default=100.0)
ap.add_argument("--tokens", default="1,16,128,1024")
ap.add_argument("--heads", default="16,64,128")
ap.add_argument("--topk", type=int, default=2048)
ap.add_argument("--slots", type=int, default=131072)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_decode_sparse_kv8.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, FP8, DQK, DV, SCALE, P = fa.DTYPES["bf16"], fa.DTYPES["fp8_e4m3"], 576, 512, 192.0 ** -0.5, 64
topk = args.topk
assert topk % 64 == 0 and args.slots % P == 0 and topk <= args.slots
NAMES = ("new", "floor", "today", "bf16")


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


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, topk=topk, slots=args.slots, results=[])
ints = lambda s: [int(x) for x in s.split(",")]
g = torch.Generator(device="cuda").manual_seed(31)
pool8 = torch.rand(args.slots // P, P, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.float8_e4m3fn)
pool16 = pool8.to(torch.bfloat16)  # the same values widened
bytes_of_pool = pool8.view(torch.uint8).view(-1, DQK)
mp = topk // 64
for T in ints(args.tokens):
    lists = {"random": torch.stack([torch.randperm(args.slots, device="cuda", generator=g)[:topk] for _ in range(T)]).to(torch.int32)}
    lists["sorted"] = lists["random"].sort(dim=1).values.contiguous()
    twin = torch.empty(T * mp, P, DQK, device="cuda", dtype=torch.uint8)  # token t owns pages t * mp .. + mp - 1, in list order
    bytes_of_twin = twin.view(-1, DQK)
    table = torch.arange(T * mp, dtype=torch.int32, device="cuda").view(T, mp)
    sl = torch.full((T,), topk, dtype=torch.int32, device="cuda")
    qall = torch.rand(T, 128, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
    lse = torch.empty(T, 128, dtype=torch.float32, device="cuda")
    for kind, idx in lists.items():
        flat = idx.reshape(-1)
        torch.index_select(bytes_of_pool, 0, flat, out=bytes_of_twin)  # the floor's pool: gathered once, outside the measurement
        for Hq in ints(args.heads):
            q = qall[:, :Hq].contiguous()
            need = lib.fa_fwd_mla_decode_sparse_kv8_workspace_bytes(T, Hq, DV, topk)
            assert need == lib.fa_fwd_mla_decode_paged_kv8_workspace_bytes(T, Hq, 1, DV, P, mp) == lib.fa_fwd_mla_decode_sparse_workspace_bytes(T, Hq, DV, topk) > 0
            S = need // (T * ((Hq + 15) // 16) * 16 * (DV + 2) * 4)
            o = {n: torch.empty(T, Hq, DV, device="cuda", dtype=torch.bfloat16) for n in ("new", "floor", "bf16")}
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            lists_args = (idx.data_ptr(), None, T, Hq, DQK, DV, topk, P, args.slots // P, SCALE, Hq * DQK, DQK, Hq * DV, DV, P * DQK, DQK, topk)
            a_new = (q.data_ptr(), pool8.data_ptr(), o["new"].data_ptr(), lse.data_ptr()) + lists_args + (BF16, FP8, ws.data_ptr(), ws.numel(), st)
            a_bf16 = (q.data_ptr(), pool16.data_ptr(), o["bf16"].data_ptr(), lse.data_ptr()) + lists_args + (BF16, ws.data_ptr(), ws.numel(), st)
            a_dense = (q.data_ptr(), twin.data_ptr(), o["floor"].data_ptr(), lse.data_ptr(), table.data_ptr(), sl.data_ptr(), T, Hq, 1, DQK, DV, P,
                       T * mp, mp, SCALE, Hq * DQK, DQK, DQK, Hq * DV, DV, DV, P * DQK, DQK, mp, 0, BF16, FP8, ws.data_ptr(), ws.numel(), st)
            new = lambda: lib.fa_fwd_mla_decode_sparse_kv8(*a_new)  # noqa: E731
            bf16 = lambda: lib.fa_fwd_mla_decode_sparse(*a_bf16)  # noqa: E731
            floor = lambda: lib.fa_fwd_mla_decode_paged_kv8(*a_dense)  # noqa: E731

            def today():
                torch.index_select(bytes_of_pool, 0, flat, out=bytes_of_twin)
                return lib.fa_fwd_mla_decode_paged_kv8(*a_dense)

            # the same keys, the same bits: checked before anything is timed (today writes the twin the floor reads: the floor's bits)
            assert new() == 0 and floor() == 0 and bf16() == 0, lib.fa_last_error()
            torch.cuda.synchronize()
            bits = {n: o[n].view(torch.int16).clone() for n in o}
            assert today() == 0
            torch.cuda.synchronize()
            assert torch.equal(bits["new"], bits["floor"]) and torch.equal(bits["new"], bits["bf16"]) and torch.equal(bits["new"], o["floor"].view(torch.int16)), \
                "the new call's bits are the dense e4m3 call's on the twin and the sparse call's on the widened pool"
            res = ab({"new": new, "floor": floor, "today": today, "bf16": bf16}, floor)
            t = {n: (res[n + " #1"] + res[n + " #2"]) / 2 for n in NAMES}
            scatter = {n: abs(res[n + " #1"] - res[n + " #2"]) / t[n] for n in t}
            tbs = {n: T * topk * DQK * (2 if n == "bf16" else 1) / t[n] * 1e-6 for n in t}
            ratios = {"new_vs_" + n: t["new"] / t[n] for n in NAMES[1:]}
            out["results"].append(dict(T=T, Hq=Hq, lists=kind, S=S, us=t, raw=res, scatter=scatter, tbs=tbs, **ratios))
            print(f"T={T} Hq={Hq} {kind} (S={S}): " + ", ".join(f"{n} {t[n]:8.1f} us {tbs[n]:5.2f} TB/s +-{scatter[n] * 100:.1f} %" for n in t)
                  + " | " + ", ".join(f"new / {n} {t['new'] / t[n]:.3f}" for n in NAMES[1:]), flush=True)
    del twin, lists, qall
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
