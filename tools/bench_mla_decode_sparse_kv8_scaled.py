#!/usr/bin/env python3
"""fa_fwd_mla_decode_sparse_kv8_scaled (the absorbed MLA step over a list of slots per token of a pool of 656-byte rows: e4m3 latent, a
fp32 scale per 128 latent elements, bf16 rotary) next to the way of doing without it and to the floors it cannot beat, from the same
build, on the method of tools/bench_mla_decode_sparse_kv8.py: raw C-ABI calls, device events, warm clocks (a spin of --warm-ms in front
of every measurement) and interleaved rounds (the candidates alternate inside every round and EACH RUNS TWICE per round, as "#1" and
"#2": the distance between a call's two copies is the session's own scatter; a figure is the median over the rounds of the time per
call). bf16 queries, topk = 2048 entries per token drawn at random from a pool of --slots slots (pages of 64); Hq in {16, 64, 128}, T in
{1, 16, 128, 1024} tokens. Candidates:
  new    fa_fwd_mla_decode_sparse_kv8_scaled on the pool of 656-byte rows and the lists
  today  what a caller does without it: a torch dequantise of the listed rows into a bf16 pool in list order (index_select, e4m3 -> fp32,
         times the scales, -> bf16, the rotary part copied), then fa_fwd_mla_decode_sparse over that pool under identity lists
  bf16   floor: fa_fwd_mla_decode_sparse on the pool dequantised beforehand, under the same lists (twice the bytes, no conversion)
  kv8    floor: fa_fwd_mla_decode_sparse_kv8 on a pool of 576 plain e4m3 bytes per row (other values: timed, not compared)
new, today and bf16 are checked bit-identical in O before anything is timed. Per shape: us per call of each, new / today, new / bf16,
new / kv8, TB/s of the bytes the step needs (T * topk * 656; bf16: 1152; kv8: 576), and each call against its own second copy. Then the
append, fa_mla_kv_append_paged_scaled, over --append-rows new rows: us and GB/s of the bytes it moves (1152 read + 656 written per row).
usage: bench_mla_decode_sparse_kv8_scaled.py [--rounds N] [--iters N] [--warm-ms MS] [--tokens 1,16,128,1024] [--heads 16,64,128]
                                             [--topk N] [--slots N] [--append-rows N] [--json FILE]"""
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
ap.add_argument("--append-rows", type=int, default=16384)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_decode_sparse_kv8_scaled.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, FP8, DQK, DV, ROW, SCALE, P = fa.DTYPES["bf16"], fa.DTYPES["fp8_e4m3"], 576, 512, 656, 192.0 ** -0.5, 64
topk = args.topk
assert topk % 64 == 0 and args.slots % P == 0 and topk <= args.slots
NAMES = ("new", "today", "bf16", "kv8")
ROW_BYTES = {"new": ROW, "today": ROW, "bf16": 2 * DQK, "kv8": DQK}


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


def dequantise(rows, out):
    """rows uint8 [n, 656] -> out bf16 [n, 576] by the call's rule: one fp32 multiply, one rounding to bf16; the rotary part as it stands"""
    s = rows[:, DV:DV + 16].contiguous().view(torch.float32).repeat_interleave(128, dim=1)
    out[:, :DV] = (rows[:, :DV].contiguous().view(torch.float8_e4m3fn).to(torch.float32) * s).to(torch.bfloat16)
    out[:, DV:] = rows[:, DV + 16:].contiguous().view(torch.bfloat16)


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, topk=topk, slots=args.slots, results=[])
ints = lambda s: [int(x) for x in s.split(",")]
g = torch.Generator(device="cuda").manual_seed(34)
# the pool: values about U(-1, 1) under power-of-two scales 2^-8 .. 2^3 per 128 latent elements, written by the library's own append
kv_new = torch.rand(args.slots, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1)
kv_new[:, :DV] *= torch.exp2(torch.randint(-8, 4, (args.slots, 4), device="cuda", generator=g).float()).repeat_interleave(128, dim=1)
kv_new = kv_new.to(torch.bfloat16)
pool = torch.empty(args.slots // P, P, ROW, device="cuda", dtype=torch.uint8)
cu = torch.tensor([0, args.slots], dtype=torch.int32, device="cuda")
bt = torch.arange(args.slots // P, dtype=torch.int32, device="cuda").view(1, -1)
sl = torch.tensor([args.slots], dtype=torch.int32, device="cuda")
fa.mla_kv_append_paged_scaled(kv_new, pool, cu, bt, sl, args.slots)
rows_of_pool = pool.view(-1, ROW)
pool16 = torch.empty(args.slots // P, P, DQK, device="cuda", dtype=torch.bfloat16)  # dequantised beforehand: the bf16 floor's pool
dequantise(rows_of_pool, pool16.view(-1, DQK))
pool8 = torch.rand(args.slots // P, P, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.float8_e4m3fn)
for T in ints(args.tokens):
    idx = torch.stack([torch.randperm(args.slots, device="cuda", generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    flat = idx.reshape(-1)
    gathered = torch.empty(T * topk // P, P, DQK, device="cuda", dtype=torch.bfloat16)  # today's pool: token t's rows in list order
    ident = torch.arange(T * topk, dtype=torch.int32, device="cuda").view(T, topk)
    qall = torch.rand(T, 128, DQK, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
    lse = torch.empty(T, 128, dtype=torch.float32, device="cuda")
    for Hq in ints(args.heads):
        q = qall[:, :Hq].contiguous()
        need = lib.fa_fwd_mla_decode_sparse_kv8_scaled_workspace_bytes(T, Hq, DV, topk)
        assert need == lib.fa_fwd_mla_decode_sparse_workspace_bytes(T, Hq, DV, topk) == lib.fa_fwd_mla_decode_sparse_kv8_workspace_bytes(T, Hq, DV, topk) > 0
        S = need // (T * ((Hq + 15) // 16) * 16 * (DV + 2) * 4)
        o = {n: torch.empty(T, Hq, DV, device="cuda", dtype=torch.bfloat16) for n in NAMES}
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")

        def lists_args(lists, num_pages, row):
            return (lists.data_ptr(), None, T, Hq, DQK, DV, topk, P, num_pages, SCALE, Hq * DQK, DQK, Hq * DV, DV, P * row, row, topk)

        head = lambda pl, n: (q.data_ptr(), pl.data_ptr(), o[n].data_ptr(), lse.data_ptr())  # noqa: E731
        a_new = head(pool, "new") + lists_args(idx, args.slots // P, ROW) + (BF16, FP8, ws.data_ptr(), ws.numel(), st)
        a_kv8 = head(pool8, "kv8") + lists_args(idx, args.slots // P, DQK) + (BF16, FP8, ws.data_ptr(), ws.numel(), st)
        a_bf16 = head(pool16, "bf16") + lists_args(idx, args.slots // P, DQK) + (BF16, ws.data_ptr(), ws.numel(), st)
        a_today = head(gathered, "today") + lists_args(ident, T * topk // P, DQK) + (BF16, ws.data_ptr(), ws.numel(), st)
        new = lambda: lib.fa_fwd_mla_decode_sparse_kv8_scaled(*a_new)  # noqa: E731
        kv8 = lambda: lib.fa_fwd_mla_decode_sparse_kv8(*a_kv8)  # noqa: E731
        bf16 = lambda: lib.fa_fwd_mla_decode_sparse(*a_bf16)  # noqa: E731

        def today():
            dequantise(torch.index_select(rows_of_pool, 0, flat), gathered.view(-1, DQK))
            return lib.fa_fwd_mla_decode_sparse(*a_today)

        assert new() == 0 and today() == 0 and bf16() == 0 and kv8() == 0, lib.fa_last_error()
        torch.cuda.synchronize()
        bits = {n: o[n].view(torch.int16) for n in o}
        assert torch.equal(bits["new"], bits["bf16"]) and torch.equal(bits["new"], bits["today"]), \
            "the new call's bits are the sparse call's on the dequantised pool"
        res = ab({"new": new, "today": today, "bf16": bf16, "kv8": kv8}, bf16)
        t = {n: (res[n + " #1"] + res[n + " #2"]) / 2 for n in NAMES}
        scatter = {n: abs(res[n + " #1"] - res[n + " #2"]) / t[n] for n in t}
        tbs = {n: T * topk * ROW_BYTES[n] / t[n] * 1e-6 for n in t}
        ratios = {"new_vs_" + n: t["new"] / t[n] for n in NAMES[1:]}
        out["results"].append(dict(T=T, Hq=Hq, S=S, us=t, raw=res, scatter=scatter, tbs=tbs, **ratios))
        print(f"T={T} Hq={Hq} (S={S}): " + ", ".join(f"{n} {t[n]:8.1f} us {tbs[n]:5.2f} TB/s +-{scatter[n] * 100:.1f} %" for n in t)
              + " | " + ", ".join(f"new / {n} {t['new'] / t[n]:.3f}" for n in NAMES[1:]), flush=True)
    del gathered, ident, idx, qall
    torch.cuda.empty_cache()

# the append: --append-rows new rows of one sequence into the first pages of the pool
n = min(args.append_rows, args.slots)
sl_n = torch.tensor([n], dtype=torch.int32, device="cuda")
cu_n = torch.tensor([0, n], dtype=torch.int32, device="cuda")
a_app = (kv_new.data_ptr(), pool.data_ptr(), cu_n.data_ptr(), bt.data_ptr(), sl_n.data_ptr(), 1, n, n, P, args.slots // P, args.slots // P, DQK,
         P * ROW, ROW, args.slots // P, BF16, st)
append = lambda: lib.fa_mla_kv_append_paged_scaled(*a_app)  # noqa: E731
res = ab({"append": append}, append)
us = (res["append #1"] + res["append #2"]) / 2
out["append"] = dict(rows=n, us=us, gbs=n * (2 * DQK + ROW) / us * 1e-3, raw=res)
print(f"append: {n} rows, {us:.1f} us, {out['append']['gbs']:.1f} GB/s (1152 bytes read + 656 written per row)", flush=True)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
