#!/usr/bin/env python3
"""fa_bwd_varlen next to the dense backward (fa_bwd_ex) from the same build: raw C-ABI calls, device events, warm clocks (a spin of
--warm-ms of the dense call in front of every measurement) and interleaved A/B (the candidates alternate inside every round; the figure
of a candidate is the median over the rounds of its time per call). O and LSE come from the forward of the same layout.
  (a) equal lengths, bf16 causal, 16 sequences x 4096 tokens, 16 heads, D = 64 and 128: the varlen call against the dense batched call
      on the same data, with the dense call entered TWICE (A/A) for the noise floor -- the price of the run-time row pitch and the table
      reads;
  (b) 16 mixed lengths 1k-8k (seeded), 16 heads: the varlen call against the dense call padded to 8192 and against 16 per-sequence
      dense calls;
  (c) the share of the launched workgroups of (b), dQ and dK/dV grids together, that own nothing and return at once;
also checks, at the sizes timed, that the varlen gradients of (a) equal the dense gradients bit for bit.
usage: bench_varlen_bwd.py [--rounds N] [--iters N] [--warm-ms MS] [--json FILE]"""
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
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warm-ms", type=float, default=400.0)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_varlen_bwd.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, MFMA, H = fa.DTYPES["bf16"], fa.VARIANTS["mfma"], 16


def rand16(g, *shape):
    return torch.rand(*shape, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)


def dense_problem(q, k, v, do, B, N, D):
    """Forward (FA_VARIANT_MFMA) once, then a callable for fa_bwd_ex on [B, H, N, D]; returns (call, (dq, dk, dv), keep-alive)."""
    o, lse = torch.empty_like(q), torch.empty(B, H, N, dtype=torch.float32, device="cuda")
    rc = lib.fa_fwd_exv(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, H, H, N, N, D, D ** -0.5, H * N * D, N * D,
                        H * N * D, N * D, 1, BF16, MFMA, st)
    assert rc == 0, lib.fa_last_error()
    grads = tuple(torch.empty(B, H, N, D, dtype=torch.float32, device="cuda") for _ in range(3))
    ws = torch.empty(lib.fa_bwd_workspace_bytes_ex(BF16, B, H, H, N, N, D, H * N * D, N * D, H * N * D, N * D), dtype=torch.uint8, device="cuda")
    argv = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), *(g.data_ptr() for g in grads), ws.data_ptr(),
            B, H, H, N, N, D, D ** -0.5, H * N * D, N * D, H * N * D, N * D, 1, BF16, st)
    return (lambda: lib.fa_bwd_ex(*argv)), grads, (o, lse, ws)


def varlen_problem(q, k, v, do, cu, B, total, max_len, D, o_lse=None):
    """Forward once (unless o_lse is given), then a callable for fa_bwd_varlen on [total, H, D]."""
    if o_lse is None:
        o, lse = torch.zeros_like(q), torch.empty(H, total, dtype=torch.float32, device="cuda")
        rc = lib.fa_fwd_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), cu.data_ptr(), B, H, H, total,
                               total, max_len, max_len, D, D ** -0.5, H * D, D, H * D, D, 1, BF16, st)
        assert rc == 0, lib.fa_last_error()
    else:
        o, lse = o_lse
    grads = tuple(torch.empty(total, H, D, dtype=torch.float32, device="cuda") for _ in range(3))
    ws = torch.empty(lib.fa_bwd_varlen_workspace_bytes(H, total), dtype=torch.uint8, device="cuda")
    argv = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), *(g.data_ptr() for g in grads), ws.data_ptr(),
            cu.data_ptr(), cu.data_ptr(), B, H, H, total, total, max_len, max_len, D, D ** -0.5, H * D, D, H * D, D, 1, BF16, st)
    return (lambda: lib.fa_bwd_varlen(*argv)), grads, (o, lse, ws)


def ab(cands, warm):
    """{name: median us per call} of callables measured in alternation, each round behind a spin that keeps the clocks up."""
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


def causal_bwd_flops(lens, D):  # 2.5 x the causal forward
    return sum(2.5 * 2.0 * H * L * L * D for L in lens)


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
for D in (64, 128):
    # ---- (a) equal lengths: the dense entry point gets [B, H, N, D], the varlen call the same values packed as [B * N, H, D]
    B, N = 16, 4096
    g = torch.Generator(device="cuda").manual_seed(D)
    qd, kd, vd, dod = (rand16(g, B, H, N, D) for _ in range(4))
    qp, kp, vp, dop = (x.permute(0, 2, 1, 3).reshape(B * N, H, D).contiguous() for x in (qd, kd, vd, dod))
    cu = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device="cuda")
    dense, gd, keep_d = dense_problem(qd, kd, vd, dod, B, N, D)
    var, gv, keep_v = varlen_problem(qp, kp, vp, dop, cu, B, B * N, N, D)
    res = ab({"dense fa_bwd_ex": dense, "dense fa_bwd_ex (A/A)": dense, "fa_bwd_varlen": var}, dense)
    same = all(bool(torch.equal(a.reshape(B, N, H, D).permute(0, 2, 1, 3), b)) for a, b in zip(gv, gd))
    fl = causal_bwd_flops([N] * B, D)
    for n, r in res.items():
        r["tflops"] = fl / r["median_us"] / 1e6
        print(f"(a) D={D} 16 x 4096 causal bf16, 16 heads: {n:24s} {r['median_us']:9.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f})  {r['tflops']:6.1f} TFLOP/s", flush=True)
    base = res["dense fa_bwd_ex"]["median_us"]
    ratio, aa = res["fa_bwd_varlen"]["median_us"] / base, res["dense fa_bwd_ex (A/A)"]["median_us"] / base
    print(f"(a) D={D}: varlen / dense = {ratio:.4f} (dense A/A = {aa:.4f}); varlen gradients equal the dense gradients bit for bit: {same}", flush=True)
    out["results"].append(dict(case="a", D=D, B=B, N=N, times=res, varlen_over_dense=ratio, dense_aa=aa, bit_identical=same))
    del qd, kd, vd, dod, qp, kp, vp, dop, gd, gv, keep_d, keep_v, dense, var
    torch.cuda.empty_cache()

    # ---- (b) 16 mixed lengths 1k-8k
    lens = [int(x) for x in np.random.default_rng(0).integers(1024, 8193, 16)]
    total, NP = sum(lens), 8192
    cu_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cu = torch.from_numpy(cu_h).cuda()
    qp, kp, vp, dop = (rand16(g, total, H, D) for _ in range(4))
    var, _, keep_v = varlen_problem(qp, kp, vp, dop, cu, len(lens), total, max(lens), D)
    var_loose, _, keep_l = varlen_problem(qp, kp, vp, dop, cu, len(lens), total, NP, D, o_lse=keep_v[:2])  # max_seqlen = 8192: a fixed cap
    qd, kd, vd, dod = (torch.zeros(len(lens), H, NP, D, device="cuda", dtype=torch.bfloat16) for _ in range(4))
    for b, L in enumerate(lens):
        for dst, src in ((qd, qp), (kd, kp), (vd, vp), (dod, dop)):
            dst[b, :, :L] = src[cu_h[b]:cu_h[b + 1]].transpose(0, 1)
    padded, _, keep_p = dense_problem(qd, kd, vd, dod, len(lens), NP, D)
    per = []
    for b, L in enumerate(lens):  # 16 dense calls on contiguous per-sequence copies
        seq = tuple(x[cu_h[b]:cu_h[b + 1]].transpose(0, 1).contiguous()[None] for x in (qp, kp, vp, dop))
        per.append((dense_problem(*seq, 1, L, D), seq))

    def per_sequence():
        rc = 0
        for (fn, _, _), _ in per:
            rc |= fn()
        return rc

    res = ab({"fa_bwd_varlen (max_seqlen = longest)": var, "fa_bwd_varlen (max_seqlen = 8192)": var_loose, "dense padded to 8192": padded,
              "16 per-sequence dense calls": per_sequence}, padded)
    fl = causal_bwd_flops(lens, D)
    for n, r in res.items():
        r["tflops_useful"] = fl / r["median_us"] / 1e6
        print(f"(b) D={D} 16 mixed 1k-8k ({total} tokens) causal bf16: {n:38s} {r['median_us']:9.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f})  "
              f"{r['tflops_useful']:6.1f} useful TFLOP/s", flush=True)
    # ---- (c) launched workgroups that return at once: both grids launch ceil(max_seqlen / 128) per (sequence, head), ceil(L_b / 128) own rows
    shares = {}
    for name, m in (("max_seqlen = longest", max(lens)), ("max_seqlen = 8192", NP)):
        launched = 2 * len(lens) * ((m + 127) // 128)
        busy = 2 * sum((L + 127) // 128 for L in lens)
        shares[name] = 1.0 - busy / launched
        print(f"(c) D={D} {name}: {launched * H} workgroups launched (dQ + dK/dV), {(launched - busy) * H} return at once ({100 * shares[name]:.1f} %)", flush=True)
    out["results"].append(dict(case="b", D=D, lens=lens, times=res, empty_block_share=shares))
    del qd, kd, vd, dod, qp, kp, vp, dop, per, keep_v, keep_l, keep_p, var, var_loose, padded
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
