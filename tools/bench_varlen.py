#!/usr/bin/env python3
"""fa_fwd_varlen next to the dense 128-row kernel (fa_fwd_exv, FA_VARIANT_MFMA) from the same build: raw C-ABI calls, device events,
warm clocks (a spin of --warm-ms of the dense call in front of every measurement) and interleaved A/B (the candidates alternate inside
every round; the figure of a candidate is the median over the rounds of its time per call).
  (a) equal lengths, bf16 causal, 16 sequences x 4096 tokens, 16 heads, D = 64 and 128: the varlen call against the dense batched call
      on the same data -- the price of the run-time row pitch and the table reads;
  (b) 16 mixed lengths 1k-8k (seeded), 16 heads: the varlen call against the dense call padded to 8192 and against 16 per-sequence
      dense calls;
  (c) the share of the launched workgroups of (b) that find no rows and return at once;
also checks, at the sizes timed, that the varlen result of (a) equals the dense result bit for bit.
usage: bench_varlen.py [--rounds N] [--iters N] [--warm-ms MS] [--json FILE]"""
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
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warm-ms", type=float, default=400.0)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_varlen.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, MFMA, H = fa.DTYPES["bf16"], fa.VARIANTS["mfma"], 16


def dense_call(q, k, v, o, lse, B, N, D):
    argv = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, H, N, N, D, D ** -0.5, H * N * D, N * D, H * N * D,
            N * D, 1, BF16, MFMA, st)
    return lambda: lib.fa_fwd_exv(*argv)


def varlen_call(q, k, v, o, lse, cu, B, total, max_len, D):
    argv = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), cu.data_ptr(), B, H, H, total, total, max_len,
            max_len, D, D ** -0.5, H * D, D, H * D, D, 1, BF16, st)
    return lambda: lib.fa_fwd_varlen(*argv)


def ab(cands, warm):
    """{name: median us per call} of callables measured in alternation, each round behind a spin that keeps the clocks up."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in cands.values():
        for _ in range(3):
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


def causal_flops(lens, D):
    return sum(2.0 * H * L * L * D for L in lens)


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
for D in (64, 128):
    # ---- (a) equal lengths. The dense entry point wants rows of pitch D: it gets [B, H, N, D], the varlen call the same values packed as
    # [B * N, H, D]
    B, N = 16, 4096
    g = torch.Generator(device="cuda").manual_seed(D)
    qd, kd, vd = (torch.rand(B, H, N, D, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16) for _ in range(3))
    od = torch.empty_like(qd)
    ld = torch.empty(B, H, N, dtype=torch.float32, device="cuda")
    qp, kp, vp = (x.permute(0, 2, 1, 3).reshape(B * N, H, D).contiguous() for x in (qd, kd, vd))
    op = torch.empty_like(qp)
    lp = torch.empty(H, B * N, dtype=torch.float32, device="cuda")
    cu = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device="cuda")
    dense = dense_call(qd, kd, vd, od, ld, B, N, D)
    var = varlen_call(qp, kp, vp, op, lp, cu, B, B * N, N, D)
    res = ab({"dense fa_fwd_exv(mfma)": dense, "fa_fwd_varlen": var}, dense)
    same = bool(torch.equal(op.reshape(B, N, H, D).permute(0, 2, 1, 3), od) and torch.equal(lp.reshape(H, B, N).permute(1, 0, 2), ld))
    fl = causal_flops([N] * B, D)
    for n, r in res.items():
        r["tflops"] = fl / r["median_us"] / 1e6
        print(f"(a) D={D} 16 x 4096 causal bf16, 16 heads: {n:24s} {r['median_us']:8.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f})  {r['tflops']:6.1f} TFLOP/s", flush=True)
    ratio = res["fa_fwd_varlen"]["median_us"] / res["dense fa_fwd_exv(mfma)"]["median_us"]
    print(f"(a) D={D}: varlen / dense = {ratio:.4f}; varlen output equals dense output bit for bit: {same}", flush=True)
    out["results"].append(dict(case="a", D=D, B=B, N=N, times=res, varlen_over_dense=ratio, bit_identical=same))
    del qd, kd, vd, od, ld, qp, kp, vp, op, lp

    # ---- (b) 16 mixed lengths 1k-8k
    lens = [int(x) for x in np.random.default_rng(0).integers(1024, 8193, 16)]
    total, NP = sum(lens), 8192
    cu_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cu = torch.from_numpy(cu_h).cuda()
    qp, kp, vp = (torch.rand(total, H, D, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16) for _ in range(3))
    op = torch.empty_like(qp)
    lp = torch.empty(H, total, dtype=torch.float32, device="cuda")
    var = varlen_call(qp, kp, vp, op, lp, cu, len(lens), total, max(lens), D)
    var_loose = varlen_call(qp, kp, vp, op, lp, cu, len(lens), total, NP, D)  # max_seqlen = 8192, what a server with a fixed cap passes
    qd, kd, vd = (torch.zeros(len(lens), H, NP, D, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    for b, L in enumerate(lens):
        for dst, src in ((qd, qp), (kd, kp), (vd, vp)):
            dst[b, :, :L] = src[cu_h[b]:cu_h[b + 1]].transpose(0, 1)
    od = torch.empty_like(qd)
    ld = torch.empty(len(lens), H, NP, dtype=torch.float32, device="cuda")
    padded = dense_call(qd, kd, vd, od, ld, len(lens), NP, D)
    per = []
    for b, L in enumerate(lens):  # 16 dense calls on contiguous per-sequence copies
        qs, ks, vs = (x[cu_h[b]:cu_h[b + 1]].transpose(0, 1).contiguous()[None] for x in (qp, kp, vp))
        os_, ls = torch.empty_like(qs), torch.empty(1, H, L, dtype=torch.float32, device="cuda")
        per.append((dense_call(qs, ks, vs, os_, ls, 1, L, D), (qs, ks, vs, os_, ls)))

    def per_sequence():
        rc = 0
        for fn, _ in per:
            rc |= fn()
        return rc

    res = ab({"fa_fwd_varlen (max_seqlen = longest)": var, "fa_fwd_varlen (max_seqlen = 8192)": var_loose, "dense padded to 8192": padded,
              "16 per-sequence dense calls": per_sequence}, padded)
    fl = causal_flops(lens, D)
    for n, r in res.items():
        r["tflops_useful"] = fl / r["median_us"] / 1e6
        print(f"(b) D={D} 16 mixed 1k-8k ({total} tokens) causal bf16: {n:38s} {r['median_us']:8.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f})  "
              f"{r['tflops_useful']:6.1f} useful TFLOP/s", flush=True)
    # ---- (c) launched workgroups that return at once: ceil(max_seqlen / 128) per (sequence, head) against ceil(L_b / 128) with rows
    shares = {}
    for name, m in (("max_seqlen = longest", max(lens)), ("max_seqlen = 8192", NP)):
        launched = len(lens) * ((m + 127) // 128)
        busy = sum((L + 127) // 128 for L in lens)
        shares[name] = 1.0 - busy / launched
        print(f"(c) D={D} {name}: {launched * H} workgroups launched, {(launched - busy) * H} return at once ({100 * shares[name]:.1f} %)", flush=True)
    out["results"].append(dict(case="b", D=D, lens=lens, times=res, empty_block_share=shares))
    del qd, kd, vd, od, ld, qp, kp, vp, op, lp, per
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
