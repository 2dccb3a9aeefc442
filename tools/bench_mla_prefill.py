#!/usr/bin/env python3
"""fa_fwd_varlen_mla (head dims 192 / 128) next to fa_fwd_varlen at D = 128 on the same token counts and next to torch SDPA on the same
packed data ("today's route"): raw C-ABI calls, device events, warm clocks (a spin of --warm-ms of the D = 128 call in front of every
measurement) and interleaved rounds in which every candidate is measured TWICE (the figure of a candidate is the median over all its
measurements of its time per call). The MLA call runs a second time on a copy of its buffers: the ratio of the two medians is the
scatter of the method itself.
Shapes: bf16, 16 heads, causal, 2 x 16384, 16 x 2048 and 1 x 65536 tokens. Work: 2 * (192 + 128) flops per visible (query, key) pair
for the MLA call and for SDPA, 4 * 128 for the D = 128 call.
usage: bench_mla_prefill.py [--rounds N] [--iters N] [--warm-ms MS] [--json FILE]"""
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
ap.add_argument("--warm-ms", type=float, default=200.0)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_prefill.py measures on the GPU: none found")
lib = fa.load_library()
st = torch.cuda.current_stream().cuda_stream
BF16, H, DQK, DV = fa.DTYPES["bf16"], 16, 192, 128
SCALE = DQK ** -0.5
SHAPES = ((2, 16384), (16, 2048), (1, 65536))


def mla_call(q, k, v, o, lse, cu, B, total, N):
    argv = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), cu.data_ptr(), B, H, H, total, total, N, N,
            DQK, DV, SCALE, H * DQK, DQK, H * DQK, DQK, H * DV, DV, H * DV, DV, 1, BF16, st)
    return lambda: lib.fa_fwd_varlen_mla(*argv)


def varlen_call(q, k, v, o, lse, cu, B, total, N):
    argv = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), cu.data_ptr(), cu.data_ptr(), B, H, H, total, total, N, N,
            DV, SCALE, H * DV, DV, H * DV, DV, 1, BF16, st)
    return lambda: lib.fa_fwd_varlen(*argv)


def sdpa_call(q, k, v, B, N):
    """torch SDPA on the packed data viewed as [B, H, N, D] (equal lengths), fused backends only (the math path holds N x N scores);
    (how, callable) or (reason, None)"""
    import torch.nn.functional as F
    from torch.nn.attention import SDPBackend, sdpa_kernel

    view = lambda x: x.view(B, N, H, x.shape[-1]).transpose(1, 2)
    qv, kv, vv = view(q), view(k), view(v)
    vpad = torch.nn.functional.pad(v, (0, DQK - DV)).view(B, N, H, DQK).transpose(1, 2)
    tried = []
    for how, fn in (("torch SDPA (192 / 128)", lambda: F.scaled_dot_product_attention(qv, kv, vv, is_causal=True, scale=SCALE)),
                    ("torch SDPA (V padded to 192, O sliced)", lambda: F.scaled_dot_product_attention(qv, kv, vpad, is_causal=True, scale=SCALE)[..., :DV])):
        def run(fn=fn):
            with sdpa_kernel([SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION]):
                fn()
            return 0
        try:
            run()
            torch.cuda.synchronize()
            return how, run
        except Exception as e:  # no fused kernel for the shape on this build
            tried.append(f"{how}: {type(e).__name__}: {str(e).splitlines()[0][:120]}")
    return "; ".join(tried), None


def ab(cands, warm):
    """{name: median us per call}: every candidate twice per round, in an order that rotates with the round, each measurement behind a spin"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in cands.values():
        for _ in range(2):
            assert fn() == 0, lib.fa_last_error()
    torch.cuda.synchronize()
    times = {n: [] for n in cands}
    for r in range(args.rounds):
        order = list(cands)
        order = order[r % len(order):] + order[:r % len(order)]
        for name in order + order[::-1]:
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
    return {n: dict(median_us=statistics.median(t), min_us=min(t), max_us=max(t), n=len(t)) for n, t in times.items()}


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, results=[])
for B, N in SHAPES:
    total = B * N
    g = torch.Generator(device="cuda").manual_seed(N)
    rnd = lambda d: torch.rand(total, H, d, device="cuda", generator=g, dtype=torch.float32).mul_(2).sub_(1).to(torch.bfloat16)
    q, k, v = rnd(DQK), rnd(DQK), rnd(DV)
    o, lse = torch.empty(total, H, DV, device="cuda", dtype=torch.bfloat16), torch.empty(H, total, device="cuda", dtype=torch.float32)
    q2, k2, v2, o2, lse2 = q.clone(), k.clone(), v.clone(), torch.empty_like(o), torch.empty_like(lse)
    q128, k128, o128, lse128 = q[:, :, :DV].contiguous(), k[:, :, :DV].contiguous(), torch.empty_like(o), torch.empty_like(lse)
    cu = torch.arange(0, (B + 1) * N, N, dtype=torch.int32, device="cuda")
    d128 = varlen_call(q128, k128, v, o128, lse128, cu, B, total, N)
    cands = {"fa_fwd_varlen_mla": mla_call(q, k, v, o, lse, cu, B, total, N),
             "fa_fwd_varlen_mla (second copy)": mla_call(q2, k2, v2, o2, lse2, cu, B, total, N),
             "fa_fwd_varlen D=128": d128}
    how, sdpa = sdpa_call(q, k, v, B, N)
    if sdpa is not None:
        cands[how] = sdpa
    res = ab(cands, d128)
    pairs = B * H * N * (N + 1) / 2.0
    for n, r in res.items():
        r["tflops"] = pairs * (4 * DV if "D=128" in n else 2 * (DQK + DV)) / r["median_us"] / 1e6
        print(f"{B} x {N} causal bf16, 16 heads: {n:42s} {r['median_us']:10.1f} us (min {r['min_us']:.1f}, max {r['max_us']:.1f}, n={r['n']})  "
              f"{r['tflops']:6.1f} TFLOP/s", flush=True)
    m, m2, d = (res[n] for n in ("fa_fwd_varlen_mla", "fa_fwd_varlen_mla (second copy)", "fa_fwd_varlen D=128"))
    line = (f"{B} x {N}: MLA rate / D=128 rate = {m['tflops'] / d['tflops']:.3f}; time MLA / D=128 = {m['median_us'] / d['median_us']:.3f} (1.25 x the work); "
            f"scatter, MLA / its second copy = {m['median_us'] / m2['median_us']:.4f}")
    if sdpa is not None:
        line += f"; {how} / MLA = {res[how]['median_us'] / m['median_us']:.2f} x the time"
    else:
        line += f"; torch SDPA: no fused kernel ran ({how})"
    print(line, flush=True)
    out["results"].append(dict(B=B, N=N, times=res, sdpa=how))
    del q, k, v, o, lse, q2, k2, v2, o2, lse2, q128, k128, o128, lse128, cands, d128, sdpa
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
