#!/usr/bin/env python3
"""fa_bwd_varlen_mla (the MLA prefill backward, head dims 192 / 128) from this build: raw C-ABI calls, device events, warm clocks (a spin
of --warm-ms in front of every measurement) and interleaved rounds (every candidate is entered TWICE per round; the figure of a
candidate is the median over the rounds of its time per call). bf16, 16 heads, causal; shapes 2 x 16384, 16 x 2048 and 1 x 65536 tokens.
Per shape:
  * fa_bwd_varlen_mla, counted at 2 * 1152 FLOPs per visible (query, key) pair and head: 192 + 128 + 192 in the dQ kernel, 192 + 128 +
    128 + 192 in the dK/dV kernel;
  * its own second copy (A/A), the scatter of the method;
  * fa_bwd_varlen at D = 128 on the same tokens (the first 128 columns of q and k), at its own 2 * 896;
  * today's route where torch offers one: autograd through scaled_dot_product_attention on [B, H, N, 192] with V zero-padded to 192
    (fused backends only -- the math backend's N x N scores do not fit at these lengths); --no-sdpa leaves it out.
--trace: no timing, every shape's call three times (for a kernel trace that splits the call into its two kernels).
usage: bench_mla_bwd.py [--rounds N] [--iters N] [--warm-ms MS] [--json FILE] [--no-sdpa] [--trace]"""
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
ap.add_argument("--warm-ms", type=float, default=300.0)
ap.add_argument("--json", default=None)
ap.add_argument("--no-sdpa", action="store_true")
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_bwd.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, H, DQK, DV = fa.DTYPES["bf16"], 16, 192, 128
SCALE = DQK ** -0.5
SHAPES = ((2, 16384), (16, 2048), (1, 65536))


def rand16(g, *shape):
    return torch.rand(*shape, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)


def mla_problem(q, k, v, do, cu, B, total, N):
    o, lse = torch.zeros(total, H, DV, dtype=q.dtype, device="cuda"), torch.empty(H, total, dtype=torch.float32, device="cuda")
    rc = lib.fa_fwd_varlen_mla(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), cu.data_ptr(), B, H, H, total,
                               total, N, N, DQK, DV, SCALE, H * DQK, DQK, H * DQK, DQK, H * DV, DV, H * DV, DV, 1, BF16, st)
    assert rc == 0, lib.fa_last_error()
    grads = tuple(torch.empty(x.shape, dtype=torch.float32, device="cuda") for x in (q, k, v))
    ws = torch.empty(lib.fa_bwd_varlen_workspace_bytes(H, total), dtype=torch.uint8, device="cuda")
    argv = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), *(g.data_ptr() for g in grads), ws.data_ptr(),
            cu.data_ptr(), cu.data_ptr(), B, H, H, total, total, N, N, DQK, DV, SCALE, H * DQK, DQK, H * DQK, DQK, H * DV, DV, H * DV, DV, 1, BF16, st)
    return (lambda: lib.fa_bwd_varlen_mla(*argv)), (o, lse, ws, grads)


def varlen128_problem(q, k, v, do, cu, B, total, N):
    o, lse = torch.zeros_like(q), torch.empty(H, total, dtype=torch.float32, device="cuda")
    rc = lib.fa_fwd_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), cu.data_ptr(), B, H, H, total,
                           total, N, N, DV, SCALE, H * DV, DV, H * DV, DV, 1, BF16, st)
    assert rc == 0, lib.fa_last_error()
    grads = tuple(torch.empty(total, H, DV, dtype=torch.float32, device="cuda") for _ in range(3))
    ws = torch.empty(lib.fa_bwd_varlen_workspace_bytes(H, total), dtype=torch.uint8, device="cuda")
    argv = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), *(g.data_ptr() for g in grads), ws.data_ptr(),
            cu.data_ptr(), cu.data_ptr(), B, H, H, total, total, N, N, DV, SCALE, H * DV, DV, H * DV, DV, 1, BF16, st)
    return (lambda: lib.fa_bwd_varlen(*argv)), (o, lse, ws, grads)


def sdpa_problem(q, k, v, do, B, N):
    """autograd through SDPA on [B, H, N, 192], V and dO zero-padded to 192: a callable that runs the backward alone, or None"""
    from torch.nn.attention import SDPBackend, sdpa_kernel

    def dense(x, width):
        y = torch.zeros(B, H, N, DQK, dtype=x.dtype, device="cuda")
        y[..., :width] = x.view(B, N, H, width).permute(0, 2, 1, 3)
        return y

    try:
        qd, kd, vd = (dense(x, w).requires_grad_(True) for x, w in ((q, DQK), (k, DQK), (v, DV)))
        dod = dense(do, DV)
        with sdpa_kernel([SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION]):
            od = torch.nn.functional.scaled_dot_product_attention(qd, kd, vd, is_causal=True, scale=SCALE)

        def call():
            torch.autograd.grad(od, (qd, kd, vd), dod, retain_graph=True)
            return 0
        call()
        torch.cuda.synchronize()
        return call, (qd, kd, vd, dod, od)
    except Exception as e:  # no fused backend for the shape, or no memory for it
        print(f"    (torch SDPA route not available here: {type(e).__name__}: {str(e).splitlines()[0][:160]})", flush=True)
        return None, None


def rounds(cands, warm):
    """{name: median us per call}: interleaved rounds, every candidate twice per round, each measurement behind a warm spin"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in cands.values():
        assert fn() == 0, lib.fa_last_error()
    torch.cuda.synchronize()
    times = {n: [] for n in cands}
    for r in range(args.rounds):
        order = list(cands)
        order = order[r % len(order):] + order[:r % len(order)]
        for name in order + order:
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


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
for B, N in SHAPES:
    total = B * N
    g = torch.Generator(device="cuda").manual_seed(N)
    q, k, v, do = rand16(g, total, H, DQK), rand16(g, total, H, DQK), rand16(g, total, H, DV), rand16(g, total, H, DV)
    cu = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device="cuda")
    mla, keep_m = mla_problem(q, k, v, do, cu, B, total, N)
    if args.trace:
        for _ in range(3):
            assert mla() == 0, lib.fa_last_error()
        torch.cuda.synchronize()
        print(f"traced {B} x {N}", flush=True)
        del q, k, v, do, keep_m, mla
        torch.cuda.empty_cache()
        continue
    q128, k128 = q[:, :, :DV].contiguous(), k[:, :, :DV].contiguous()
    v128, keep_v = varlen128_problem(q128, k128, v, do, cu, B, total, N)
    cands = {"fa_bwd_varlen_mla": mla, "fa_bwd_varlen_mla (A/A)": mla, "fa_bwd_varlen D=128": v128}
    flops = {"fa_bwd_varlen_mla": 1152, "fa_bwd_varlen_mla (A/A)": 1152, "fa_bwd_varlen D=128": 896, "torch SDPA autograd (V padded to 192)": 1152}
    keep_s = None
    if not args.no_sdpa:
        sd, keep_s = sdpa_problem(q, k, v, do, B, N)
        if sd is not None:
            cands["torch SDPA autograd (V padded to 192)"] = sd
    res = rounds(cands, mla)
    pairs = B * H * (N * (N + 1) / 2.0)  # visible pairs under the causal mask
    for n, r in res.items():
        r["tflops"] = 2.0 * flops[n] * pairs / r["median_us"] / 1e6
        print(f"{B:2d} x {N:5d} causal bf16, 16 heads: {n:40s} {r['median_us']:10.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f})  {r['tflops']:6.1f} TFLOP/s",
              flush=True)
    base = res["fa_bwd_varlen_mla"]["median_us"]
    line = f"{B:2d} x {N:5d}: A/A = {res['fa_bwd_varlen_mla (A/A)']['median_us'] / base:.4f}; mla / varlen128 time = {base / res['fa_bwd_varlen D=128']['median_us']:.3f} " \
           f"(work 1.286); rate mla / varlen128 = {res['fa_bwd_varlen_mla']['tflops'] / res['fa_bwd_varlen D=128']['tflops']:.3f}"
    if "torch SDPA autograd (V padded to 192)" in res:
        line += f"; SDPA / mla time = {res['torch SDPA autograd (V padded to 192)']['median_us'] / base:.2f}"
    print(line, flush=True)
    out["results"].append(dict(B=B, N=N, times=res))
    del q, k, v, do, q128, k128, keep_m, keep_v, keep_s, mla, v128, cands
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
