#!/usr/bin/env python3
"""fa_mla_sparse_head_probs and fa_mla_indexer_loss_sparse next to fa_fwd_mla_decode_sparse and the torch gather formulations, ON THE SAME
INPUTS, in the manner of tools/bench_mla_sparse_bwd.py: device events, warm clocks (a spin of --warm-ms in front of every measurement),
interleaved rounds, and EVERY candidate measured TWICE under two names (x and x'): the ratio of a call to its own second copy is the noise
a ratio between two candidates has to beat. bf16, pages of 64, pools of --slots rows, lists of topk distinct random slots, full counts.
  probs        fa_mla_sparse_head_probs               fwd          fa_fwd_mla_decode_sparse
  loss         the loss-only call                     full         loss and gradients (dk accumulated into: not re-zeroed)
  t_probs      torch: gather [T, topk, 576] rows, scores, exp(s - lse), the head sum
  t_loss/t_full torch: gather [T, topk, 128] index keys, relu, head sum, log-softmax, KL (and autograd's backward of it)
The torch routes run only where --torch-max-T allows: the gathered rows are materialised.
usage: bench_mla_indexer_loss.py [--rounds N] [--iters N] [--warm-ms MS] [--shapes T:Hq:Hi:topk,...] [--torch-max-T T] [--json FILE]"""
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
ap.add_argument("--warm-ms", type=float, default=30.0)
ap.add_argument("--shapes", default="1024:128:64:2048,4096:128:64:2048")
ap.add_argument("--slots", type=int, default=65536)
ap.add_argument("--torch-max-T", type=int, default=1024)
ap.add_argument("--peak-tflops", type=float, default=2500.0)
ap.add_argument("--json", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_mla_indexer_loss.py measures on the GPU: none found")
fa.load_library()
P, DQK, DV, DI, SCALE = 64, 576, 512, 128, 192.0 ** -0.5


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


def shape(T, Hq, Hi, topk):
    g = torch.Generator(device="cuda").manual_seed(38)
    q = torch.randn(T, Hq, DQK, device="cuda", generator=g).to(torch.bfloat16)
    pool = torch.randn(args.slots // P, P, DQK, device="cuda", generator=g).to(torch.bfloat16)
    qi = (0.3 * torch.randn(T, Hi, DI, device="cuda", generator=g)).to(torch.bfloat16)
    kpool = (0.3 * torch.randn(args.slots // P, P, DI, device="cuda", generator=g)).to(torch.bfloat16)
    w = 0.1 * torch.randn(T, Hi, device="cuda", generator=g)
    idx = torch.stack([torch.randperm(args.slots, device="cuda", generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    o, lse = torch.empty(T, Hq, DV, device="cuda", dtype=torch.bfloat16), torch.empty(T, Hq, device="cuda")
    ws_f = torch.empty(fa.mla_decode_sparse_workspace_bytes(T, Hq, DV, topk), dtype=torch.uint8, device="cuda")
    dk = torch.zeros(args.slots // P, P, DI, device="cuda")
    fwd = lambda: fa.flash_attention_mla_decode_sparse(q, pool, idx, SCALE, out=o, lse=lse, workspace=ws_f)
    fwd()
    target = fa.mla_sparse_head_probs(q, pool, lse, idx, None, SCALE)
    cands = {"probs": lambda: fa.mla_sparse_head_probs(q, pool, lse, idx, None, SCALE), "fwd": fwd,
             "loss": lambda: fa.mla_indexer_loss_sparse(qi, w, kpool, idx, None, target, need_grads=False),
             "full": lambda: fa.mla_indexer_loss_sparse(qi, w, kpool, idx, None, target, dk_idx=dk)}
    if T <= args.torch_max_T:
        qg, wg, kg = qi.clone().requires_grad_(), w.clone().requires_grad_(), kpool.clone().requires_grad_()

        def t_probs():
            rows = pool.view(-1, DQK)[idx.long()]
            return torch.exp(torch.einsum("thd,tkd->thk", q, rows).float() * SCALE - lse[:, :, None]).sum(1)

        def t_loss():
            keys = kg.view(-1, DI)[idx.long()]
            logits = (torch.relu(torch.einsum("thd,tkd->thk", qg, keys).float()) * wg[:, :, None]).sum(1)
            tau = target / target.sum(-1, keepdim=True)
            return (torch.xlogy(tau, tau) - tau * torch.log_softmax(logits, -1)).sum(-1)

        def t_full():
            qg.grad = wg.grad = kg.grad = None
            t_loss().sum().backward()

        cands.update(t_probs=t_probs, t_loss=lambda: t_loss().detach(), t_full=t_full)
    res = ab(cands, fwd)
    noise = max(abs(res[n] / res[n + "'"] - 1) for n in cands)
    f_probs, f_loss = 2.0 * T * Hq * topk * DQK, 2.0 * T * Hi * topk * DI
    r = dict(T=T, Hq=Hq, Hi=Hi, topk=topk, us=res, noise=noise, probs_tflops=f_probs / res["probs"] / 1e6, probs_vs_fwd=res["probs"] / res["fwd"],
             loss_tflops=f_loss / res["loss"] / 1e6, full_tflops=4 * f_loss / res["full"] / 1e6)
    for mine, theirs in (("probs", "t_probs"), ("loss", "t_loss"), ("full", "t_full")):
        r[mine + "_vs_torch"] = res[mine] / res[theirs] if theirs in res else None
    print(f"T={T} Hq={Hq} Hi={Hi} topk={topk}: " + ", ".join(f"{n} {res[n]:9.1f}" for n in res) + f" us | probs {r['probs_tflops']:.1f} TFLOP/s "
          f"({100 * r['probs_tflops'] / args.peak_tflops:.1f} % of {args.peak_tflops:.0f}), probs / fwd {r['probs_vs_fwd']:.2f}; loss {r['loss_tflops']:.1f}, "
          f"full {r['full_tflops']:.1f} TFLOP/s; a call against its own copy within {noise * 100:.1f} %", flush=True)
    return r


out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, iters=args.iters, warm_ms=args.warm_ms, page_size=P, slots=args.slots, results=[])
for T, Hq, Hi, topk in [tuple(int(x) for x in s.split(":")) for s in args.shapes.split(",") if s]:
    out["results"].append(shape(T, Hq, Hi, topk))
    torch.cuda.empty_cache()
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
