#!/usr/bin/env python3
"""The soft-capping entry points next to the *_window calls on the same tensors, from one build: raw C-ABI calls, device events, warm
clocks (a spin of --warm-ms in front of every measurement) and interleaved A/B (the candidates alternate inside every round; a candidate's
figure is the median over the rounds of its time per call), the method of tools/bench_sink.py. bf16, 16 query heads, D = 64 and 128,
2 prompts of 16384 tokens, windows (-1, 0) and (4095, 0) -- the layer pair of Gemma-2 --, softcap = 50:
  (a) fa_fwd_varlen_softcap, (b) fa_fwd_varlen_paged_softcap (P = 16 pool in a random order), (c) fa_fwd_decode_paged_softcap (16 sequences
      x 16384 keys, 4 key heads, one query each), each against the *_window call -- which is among the candidates TWICE: the ratio of the
      two is the scatter of the cap-free call against itself in this session, the yardstick for the softcap ratio. Under (-1, 0) the
      *_window call routes to the un-windowed causal kernels; the window kernels under the never-binding (INT_MAX, 0), the softcap
      call's own family, are timed beside it;
  (d) fa_bwd_varlen_softcap against fa_bwd_varlen_window, on the capped forward's own O and LSE.
What the ratio prices: one v_exp_f32, one v_rcp_f32 and about three more VALU operations per score.
usage: bench_softcap.py [--rounds N] [--iters N] [--warm-ms MS] [--json FILE]"""
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
    sys.exit("bench_softcap.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, H, P, N, B, INT_MAX = fa.DTYPES["bf16"], 16, 16, 16384, 2, 2 ** 31 - 1
WINDOWS = ((-1, 0), (4095, 0))
CAP = 50.0


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


def group(what, D, win, window_call, softcap_call, extra=None):
    """One window: the *_window call twice (its own scatter), the softcap call, and under (-1, 0) the window kernels at (INT_MAX, 0)."""
    cands = {"window": window_call, "window again": window_call, "softcap": softcap_call}
    if extra:
        cands.update(extra)
    res = ab(cands, window_call)
    base = res["window"]["median_us"]
    rows = {}
    for n, r in res.items():
        rows[n] = dict(r, ratio=r["median_us"] / base)
        print(f"{what} D={D} {str(win):>10s}: {n:>22s} {r['median_us']:9.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f})  ratio to the *_window call "
              f"{rows[n]['ratio']:.3f}", flush=True)
    return rows


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
for D in (64, 128):
    g = torch.Generator(device="cuda").manual_seed(D)

    def rnd(*shape):
        return torch.rand(*shape, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)

    total = B * N
    q, k, v, do = rnd(total, H, D), rnd(total, H, D), rnd(total, H, D), rnd(total, H, D)
    o = torch.empty_like(q)
    lse = torch.empty(H, total, dtype=torch.float32, device="cuda")
    cu = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device="cuda")
    res = dict(D=D, varlen={}, varlen_paged={}, decode_paged={}, backward={})

    # (a) packed
    pre = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), cu.data_ptr(), B, H, H, total, total, N, N, D,
           D ** -0.5, H * D, D, H * D, D)
    for wl, wr in WINDOWS:
        extra = {"window (INT_MAX, 0)": lambda: lib.fa_fwd_varlen_window(*pre, INT_MAX, 0, BF16, st)} if wl < 0 else None
        res["varlen"][str((wl, wr))] = group("(a) fa_fwd_varlen_softcap", D, (wl, wr), lambda: lib.fa_fwd_varlen_window(*pre, wl, wr, BF16, st),
                                             lambda: lib.fa_fwd_varlen_softcap(*pre, wl, wr, CAP, BF16, st), extra)

    # (d) the backward on the capped forward's own O and LSE
    dq, dk, dv = (torch.empty(x.shape, dtype=torch.float32, device="cuda") for x in (q, k, k))
    ws = torch.empty(lib.fa_bwd_varlen_workspace_bytes(H, total), dtype=torch.uint8, device="cuda")
    for wl, wr in WINDOWS:
        assert lib.fa_fwd_varlen_softcap(*pre, wl, wr, CAP, BF16, st) == 0, lib.fa_last_error()
        bpre = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                ws.data_ptr(), cu.data_ptr(), cu.data_ptr(), B, H, H, total, total, N, N, D, D ** -0.5, H * D, D, H * D, D)
        res["backward"][str((wl, wr))] = group("(d) fa_bwd_varlen_softcap", D, (wl, wr), lambda: lib.fa_bwd_varlen_window(*bpre, wl, wr, BF16, st),
                                               lambda: lib.fa_bwd_varlen_softcap(*bpre, wl, wr, CAP, BF16, st))
    del dq, dk, dv, ws, do

    # (b) the same keys in a P = 16 pool (NHD), pages in a random order
    mp = N // P
    num_pages = B * mp + 8
    perm = np.random.default_rng(1).permutation(num_pages)[:B * mp]
    kpool, vpool = rnd(num_pages, P, H, D), rnd(num_pages, P, H, D)
    kpool.view(num_pages * P, H, D)[torch.from_numpy(np.repeat(perm.astype(np.int64) * P, P) + np.tile(np.arange(P), B * mp)).cuda()] = k
    table = torch.from_numpy(perm.reshape(B, mp).astype(np.int32)).cuda()
    sl = torch.full((B,), N, dtype=torch.int32, device="cuda")
    ppre = (q.data_ptr(), kpool.data_ptr(), vpool.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), table.data_ptr(), sl.data_ptr(), B, H, H,
            total, N, D, P, num_pages, mp, D ** -0.5, H * D, D, P * H * D, D, H * D, mp)
    for wl, wr in WINDOWS:
        extra = {"window (INT_MAX, 0)": lambda: lib.fa_fwd_varlen_paged_window(*ppre, INT_MAX, 0, BF16, st)} if wl < 0 else None
        res["varlen_paged"][str((wl, wr))] = group("(b) fa_fwd_varlen_paged_softcap", D, (wl, wr),
                                                   lambda: lib.fa_fwd_varlen_paged_window(*ppre, wl, wr, BF16, st),
                                                   lambda: lib.fa_fwd_varlen_paged_softcap(*ppre, wl, wr, CAP, BF16, st), extra)
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
    dpre = (qd.data_ptr(), kpool.data_ptr(), vpool.data_ptr(), od.data_ptr(), ld.data_ptr(), table.data_ptr(), sl.data_ptr(), Bd, H, Hkv, 1, D, P,
            num_pages, mp, D ** -0.5, H * D, D, P * Hkv * D, D, Hkv * D, mp)
    post = (BF16, BF16, ws.data_ptr(), wsb, st)
    for wl, wr in WINDOWS:
        extra = {"window (INT_MAX, 0)": lambda: lib.fa_fwd_decode_paged_window(*dpre, INT_MAX, 0, *post)} if wl < 0 else None
        res["decode_paged"][str((wl, wr))] = group("(c) fa_fwd_decode_paged_softcap", D, (wl, wr),
                                                   lambda: lib.fa_fwd_decode_paged_window(*dpre, wl, wr, *post),
                                                   lambda: lib.fa_fwd_decode_paged_softcap(*dpre, wl, wr, CAP, *post), extra)
    out["results"].append(res)
    del kpool, vpool, qd, od, ld, ws
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
