#!/usr/bin/env python3
"""bench.py -- attention-forward throughput on MI355X, one process per GPU.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Both forms work. Typed without a launcher and with N > 1, this process never touches the GPU: it
spawns N fresh children (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set before they import torch),
waits for them and relays rank 0's JSON line -- no exec of a GPU-initialised process.

Workload (BASELINE.json configs[2], the configuration the metric is quoted on):
seqlen=4096, head_dim=64, batch=4, heads=16, bf16, is_causal=true PER GPU.
The (batch, head) slices of the global [4*N_gpus, 16, 4096, 64] problem are
block-distributed over ranks (flash_attention_metal_amd.shard.shard_heads):
independent slices, no data-path collective, weak scaling. A "step" is one
fa_fwd() launch over the rank's shard with Q/K/V already resident in HBM.

Prints ONE JSON line on rank 0. `value` = algorithmic FLOPs of all ranks' steps
/ max-over-ranks wall time of the K timed steps (barrier + synchronize on both
sides). Before the W warm-up steps the GPU is additionally warmed BY TIME (>= WARM_MS of
back-to-back launches): a handful of 0.1 ms launches ends before the clocks have settled, and the
timed region would measure the ramp. `roofline.achieved` is measured with HIP events on the launch
stream over the same K launches (events bracket blocks of 10 launches).

A plain run does only that: set up, warm up, time the K steps, print the line. `--full` adds the
measurements beyond the headline, each with work of its own: `value_public_api` (the same K launches
through flash_attention_forward), `c4_slice`, `c5_fp8`, `sweep` and `cpu_baseline` (--no-c4,
--no-sweep and --no-cpu-baseline leave parts of it out). `cpu_baseline` times the
reference's own CPU loop (oracle/_ref, kind "reference") or our C port of it (kind "port") on
the host cores, rank 0 at N=1 only, on a bounded sample. `c4_slice` is BASELINE configs[3]'s
per-GPU shard (32 (batch,head) slices of seqlen 16384, head_dim 128): with --gpus 8 the ranks
together run config 4 itself.

`--dump-outputs DIR` writes what the last timed step computed on rank 0 to DIR as float32 .npy files
(see dump_outputs). The inputs are seeded, so two builds run with the same arguments can be compared
output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import tempfile
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# configs[2] of BASELINE.json, per GPU
B_PER_GPU, H, N, D = 4, 16, 4096, 64
DTYPE = "bf16"
CAUSAL = True
PEAK_TFLOPS_BF16 = 2500.0  # MI355X_MICROARCH.md: ~2.5 PF dense bf16/f16
PEAK_HBM_GBS = 8000.0      # 8 TB/s spec
WARM_MS = 300.0            # time-based warm-up in front of the counted warm-up steps
C4_SLICES, C4_N, C4_D = 32, 16384, 128  # BASELINE configs[3] per GPU: 8*32 heads over 8 GPUs
DUMP_ROWS, DUMP_SEED = 1 << 17, 1234   # --dump-outputs: half of the 64*4096 query rows of O (32 MiB in fp32)


def cpu_baseline(target_s: float = 15.0) -> dict:
    """Time the CPU path on a bounded sample of the workload: whole heads of
    N=4096, D=64, causal, fp32 -- the reference's loop at /root/reference/main.mm:551-578."""
    import oracle  # test infrastructure: used here ONLY as the timed CPU baseline

    q = oracle.init_random(N * D, 42).reshape(N, D)
    k = oracle.init_random(N * D, 43).reshape(N, D)
    v = oracle.init_random(N * D, 44).reshape(N, D)
    flops_per_head = 2.0 * N * N * D  # causal convention, SURVEY.md 8(d)
    if oracle.have_ref():
        kind, cores = "reference", 1
        fn = lambda: oracle.ref_causal(q, k, v)  # noqa: E731
    else:
        kind, cores = "port", 1
        fn = lambda: oracle.causal(q, k, v, 0.125)  # noqa: E731
    t0 = time.perf_counter()
    fn()
    t1 = time.perf_counter() - t0
    heads = 1
    total = t1
    while total + t1 < target_s and heads < B_PER_GPU * H:
        t0 = time.perf_counter()
        fn()
        total += time.perf_counter() - t0
        heads += 1
    return {
        "value": round(flops_per_head * heads / total / 1e12, 6),
        "unit": "TFLOP/s",
        "cores": cores,
        "kind": kind,
        "sample": f"{heads} of {B_PER_GPU * H} (batch,head) slices of the workload (N={N}, D={D}, causal, fp32), "
                  f"{total:.1f} s single-threaded like the reference (main.mm:551-578)",
        "seconds_per_head": round(total / heads, 3),
    }


def spawn_ranks(args) -> int:
    """`python bench.py --gpus N` typed without a launcher: start N fresh child processes, one per GPU.
    The parent imports neither torch nor the kernel library, so nothing here has initialised a GPU."""
    port = os.environ.get("MASTER_PORT", str(29500 + os.getpid() % 2000))
    base = dict(os.environ, WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=port,
                FA_BENCH_CHILD="1")
    base.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    # A profiler preload (rocprofv3 -- python bench.py ...) has already initialised the GPU in THIS process: starting
    # the ranks from it would be an exec hop out of a GPU-initialised process. Profile one rank (--gpus 1) instead.
    if not args.cpu_gloo_rehearsal and (os.environ.get("ROCP_TOOL_LIBRARIES") or "rocprof" in os.environ.get("LD_PRELOAD", "")):
        sys.exit("bench.py --gpus N > 1 under a profiler preload is refused: profile with --gpus 1")
    argv = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    procs = []
    out0 = tempfile.TemporaryFile()  # rank 0's stdout (a pipe nobody drains while polling could fill up)
    for r in range(args.gpus):
        env = dict(base, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen(argv, env=env, stdout=out0 if r == 0 else subprocess.DEVNULL))
    # poll ALL children: a rank that dies before the first barrier would leave the others waiting for the RCCL/gloo
    # timeout -- stop them and fail at once instead
    rcs = [None] * len(procs)
    while any(rc is None for rc in rcs):
        for i, pr in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = pr.poll()
        if any(rc not in (None, 0) for rc in rcs):
            for i, pr in enumerate(procs):
                if rcs[i] is None:
                    pr.terminate()
            for i, pr in enumerate(procs):
                if rcs[i] is None:
                    try:
                        rcs[i] = pr.wait(timeout=10)
                    except subprocess.TimeoutExpired:
                        pr.kill()
                        rcs[i] = pr.wait()
            break
        time.sleep(0.05)
    out0.seek(0)
    sys.stdout.write(out0.read().decode())
    sys.stdout.flush()
    return max(abs(rc) for rc in rcs)


def make_events(torch, stream, steps, block=None):
    """The event pairs of timed_launches, created AND used once before the timed region: a torch event allocates its HIP event
    at its first record (tens of microseconds of host time the 3 ms region of the driver's K = 20 would otherwise include)."""
    if block is None:
        block = max(20, steps // 4)
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(0, steps, block)]
    for a, b in evs:
        a.record(stream)
        b.record(stream)
    return evs


def timed_launches(torch, stream, step, steps, block=None, evs=None):
    """K launches, HIP events on the launch stream around blocks of launches (an event pair around every single launch puts
    a bubble between kernels, and so does every pair inside the timed region: a timing event is a barrier packet plus a
    signal -- with pairs every 10 launches the 20-step run's wall time read 6 % over its own kernel time). Blocks of
    max(20, K/4) launches: one pair for the driver's K = 20, four for the default K = 200."""
    if block is None:
        block = max(20, steps // 4)
    blocks = [(i, min(i + block, steps)) for i in range(0, steps, block)]
    if evs is None:
        evs = make_events(torch, stream, steps, block)
    for (lo_i, hi_i), (a, b) in zip(blocks, evs):
        a.record(stream)
        for _ in range(lo_i, hi_i):
            step()
        b.record(stream)
    return blocks, evs


def warm_by_time(torch, dev, step, ms=WARM_MS):
    """Launch back-to-back until `ms` of GPU time has passed (clock ramp + first-touch of caches/TLBs)."""
    t0 = time.perf_counter()
    n = 0
    while (time.perf_counter() - t0) * 1e3 < ms:
        for _ in range(20):
            step()
        torch.cuda.synchronize(dev)
        n += 20
    return n


def workload_qkv(torch, dev, slices, rank):
    """Q, K, V of a rank's shard: [1, slices, N, D] bf16, uniform(-1,1) from a generator seeded by the rank (same in every run)."""
    g = torch.Generator(device=dev).manual_seed(1000 + rank)
    mk = lambda: (torch.rand(1, slices, N, D, generator=g, device=dev, dtype=torch.float32) * 2 - 1).to(torch.bfloat16)  # noqa: E731
    return mk(), mk(), mk()


def dump_outputs(path, torch, o, lse, rows=DUMP_ROWS, seed=DUMP_SEED):
    """What a caller of the timed path receives, as float32 .npy files under `path` (33 MiB in all):
    lse.npy           LSE [1, B*H, N], whole
    o_rows_sample.npy O [1, B*H, N, D] (bf16, exact in fp32) viewed as [B*H*N, D] rows: the rows at the sorted indices
                      numpy.random.default_rng(seed).choice(B*H*N, rows, replace=False) -- the same rows in every run."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    flat = o.reshape(-1, o.shape[-1])
    idx = np.sort(np.random.default_rng(seed).choice(flat.shape[0], size=min(rows, flat.shape[0]), replace=False))
    sample = flat[torch.from_numpy(idx).to(o.device)].float().cpu().numpy()
    np.save(os.path.join(path, "o_rows_sample.npy"), sample)
    np.save(os.path.join(path, "lse.npy"), lse.float().cpu().numpy())


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="also measure beyond the headline: public-API launches, config 4 shard, config 5 fp8, seqlen sweep, "
                         "CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU baseline")
    ap.add_argument("--no-sweep", action="store_true", help="with --full: no seqlen sweep")
    ap.add_argument("--no-c4", action="store_true", help="with --full: no config 4 shard and config 5 fp8 blocks")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed (rank 0) to DIR/<name>.npy, float32")
    ap.add_argument("--cpu-gloo-rehearsal", action="store_true",
                    help="rank plumbing only, on CPU over gloo (tests): no kernel is launched, no throughput is claimed")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "RANK" not in os.environ:
        return spawn_ranks(args)

    import torch

    from flash_attention_metal_amd import ranks

    if args.cpu_gloo_rehearsal:
        return rehearsal(args, ranks)

    import flash_attention_metal_amd as fa

    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU: the attention operator has no CPU path")
    fa.load_library()  # fail loudly if the HIP library is missing
    info = ranks.init_ranks(use_gpu=True)  # backend "nccl" (= RCCL): control plane only (barrier + max/sum of scalars)
    rank, local_rank, world = info.rank, info.local_rank, info.world
    args.gpus = world
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    # ---- this rank's shard of the global (batch*head) slices -------------------------------
    lo, hi = ranks.my_slices(info, B_PER_GPU * H)
    my = hi - lo  # = B_PER_GPU * H
    q, k, v = workload_qkv(torch, dev, my, rank)  # random, never zeros (DVFS: zero data inflates MFMA clocks)
    o = torch.empty_like(q)
    lse = torch.empty(1, my, N, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev)

    # validated once, launched K times (the reference host encodes its argument table per dispatch too, main.mm:821-852):
    # the Python-side checks of flash_attention_forward cost ~15 us per call, which matters for a 3 ms timed region
    plan = fa.ForwardPlan(q, k, v, is_causal=CAUSAL, out=o, lse=lse)
    step = plan.launch

    def barrier():
        ranks.barrier(info, dev)

    warm_launches = warm_by_time(torch, dev, step)
    for _ in range(args.warmup):
        step()
    evs0 = make_events(torch, stream, args.steps)
    # The timed region runs twice: once as the tail of the warm-up (same calls, result discarded), then for the record. The
    # FIRST pass of this code in a process spends ~0.12 ms of host time in its first event record (per-statement timestamps:
    # 127 us against 2-10 us for every later one), 4-5 % of the driver's 2.8 ms region; the second pass is clean
    # (wall - events: 154 -> 34 us).
    elapsed_first = None
    for rehearsal_pass in (True, False):
        barrier()
        t0 = time.perf_counter()
        blocks, evs = timed_launches(torch, stream, step, args.steps, evs=evs0)
        barrier()
        elapsed = time.perf_counter() - t0
        if rehearsal_pass:
            elapsed_first = elapsed
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, torch, o, lse)
    elapsed_public = None
    if args.full:
        # the same K launches through the public entry point (per-call validation included): what a caller without a plan sees
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fa.flash_attention_forward(q, k, v, is_causal=CAUSAL, out=o, lse=lse)
        torch.cuda.synchronize(dev)
        barrier()
        elapsed_public = time.perf_counter() - t0
    kern_ms = sorted(a.elapsed_time(b) / (hi_i - lo_i) for (lo_i, hi_i), (a, b) in zip(blocks, evs))
    launches_total = sum(a.elapsed_time(b) for a, b in evs)  # ms over all K launches
    flops_step_rank = fa.algorithmic_flops(1, my, N, D, CAUSAL)
    bytes_step_rank = fa.algorithmic_bytes(1, my, N, D, DTYPE)
    my_tflops = flops_step_rank * args.steps / elapsed / 1e12  # this rank alone, over its own clock
    flops_per_s, elapsed = ranks.aggregate_throughput(info, flops_step_rank * args.steps, elapsed, dev)
    value = flops_per_s / 1e12
    per_rank = ranks.gather_over_ranks(info, my_tflops, dev)  # imbalance across the GPUs of the node

    c4 = c4_slice(fa, torch, ranks, info, dev) if args.full and not args.no_c4 else None

    if rank == 0:
        avg_ms = launches_total / args.steps  # average launch duration over the K timed launches
        achieved = flops_step_rank / (avg_ms * 1e-3) / 1e12
        traffic, traffic_src = None, None
        tpath = os.path.join(ROOT, "profiles", "hbm_traffic.json")  # result of the separate rocprofv3 --pmc passes
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                traffic, traffic_src = tj.get("bytes_per_launch"), tj.get("source")
            except Exception:
                traffic = None
        out = {
            "metric": "attn_fwd_tflops (seqlen=4096, head_dim=64, bf16, causal)",
            "value": round(value, 3),
            "unit": "TFLOP/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 5),
            # rank 0's own clock: the FIRST pass of the timed-region code in this process (its first event record costs ~0.12 ms of
            # host time: round-over-round comparisons should use roofline.kernel_ms_avg)
            "value_first_pass": round(flops_step_rank * args.steps / elapsed_first / 1e12, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic uniform(-1,1) Q/K/V, resident in HBM",
            "config": {"workload": "BASELINE.json configs[2]: seqlen=4096 head_dim=64 batch=4 heads=16 bf16 "
                                   "is_causal=true per GPU",
                       "batch_per_gpu": B_PER_GPU, "heads": H, "seq_len": N, "head_dim": D, "is_causal": CAUSAL,
                       "sharding": f"(batch,head) slices block-distributed over {world} rank(s), no collective",
                       "flops_per_step_per_gpu": flops_step_rank, "bytes_per_step_per_gpu": bytes_step_rank,
                       "time_warmup_launches": warm_launches},
            # every rank's own rate (its FLOPs over its own wall time); value <= sum of these, = when the ranks finish together
            "per_rank": {"tflops": [round(x, 2) for x in per_rank], "tflops_min": round(min(per_rank), 2),
                         "tflops_max": round(max(per_rank), 2)},
            "roofline": {"bound": "mfma", "achieved": round(achieved, 3), "peak": PEAK_TFLOPS_BF16,
                         "unit": "TFLOP/s", "frac": round(achieved / PEAK_TFLOPS_BF16, 4),
                         # whole job against the MFMA peak of all N GPUs (achieved/frac above: rank 0's kernel alone)
                         "frac_whole_job": round(value / (PEAK_TFLOPS_BF16 * world), 4), "traffic": traffic,
                         "traffic_source": traffic_src or "none recorded",
                         "kernel": fa.forward_kernel_name(DTYPE, D, CAUSAL),
                         "kernel_ms_avg": round(avg_ms, 5), "kernel_ms_median": round(kern_ms[len(kern_ms) // 2], 5),
                         "kernel_ms_min": round(kern_ms[0], 5),
                         "hbm_frac": round(bytes_step_rank / (avg_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, 4)},
        }
        if elapsed_public is not None:  # rank 0's own clock, K calls of flash_attention_forward
            out["value_public_api"] = round(flops_step_rank * args.steps / elapsed_public / 1e12, 3)
        if c4 is not None:
            out["c4_slice"] = c4
        if args.full and world == 1 and not args.no_c4:
            out["c5_fp8"] = c5_fp8(fa, torch, dev)
        if args.full and world == 1 and not args.no_sweep:
            out["sweep"] = sweep(fa, torch, dev)
            at = [r for r in out["sweep"] if r["seqlen"] == N]
            if at:  # the sweep's N=4096 row is the same workload: a ratio far from 1 means the timed region ramped
                out["sweep_vs_value"] = round(at[0]["tflops"] / value, 4)
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out), flush=True)
    ranks.finalize(info)
    return 0


def c4_slice(fa, torch, ranks, info, dev, iters=10):
    """BASELINE configs[3] per GPU: 32 (batch,head) slices of seqlen 16384, head_dim 128, bf16 causal.
    With 8 ranks the job is config 4 itself (8*32 heads sharded by (batch, head), no collective)."""
    g = torch.Generator(device=dev).manual_seed(7000 + info.rank)
    mk = lambda: (torch.rand(1, C4_SLICES, C4_N, C4_D, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)  # noqa: E731
    q, k, v = mk(), mk(), mk()
    o = torch.empty_like(q)
    lse = torch.empty(1, C4_SLICES, C4_N, dtype=torch.float32, device=dev)

    step = fa.ForwardPlan(q, k, v, is_causal=True, out=o, lse=lse).launch

    for _ in range(3):
        step()
    ranks.barrier(info, dev)
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    ranks.barrier(info, dev)
    el = time.perf_counter() - t0
    fl = fa.algorithmic_flops(1, C4_SLICES, C4_N, C4_D, True)
    per_s, worst = ranks.aggregate_throughput(info, fl * iters, el, dev)
    return {"workload": f"BASELINE.json configs[3] shard: {C4_SLICES} slices/GPU x {info.world} GPU(s), seqlen={C4_N}, "
                        f"head_dim={C4_D}, bf16, causal",
            "tflops_total": round(per_s / 1e12, 2), "ms_per_step": round(worst / iters * 1e3, 4),
            "mfma_frac": round(per_s / 1e12 / (PEAK_TFLOPS_BF16 * info.world), 4), "steps": iters}


def c5_fp8(fa, torch, dev, iters=10):
    """BASELINE configs[4]: seqlen 8192, head_dim 64, e4m3 Q/K/V with fp32 accumulate (bf16 O), causal, B=4 x H=16 as config 3 (the
    batch is not stated there). Informational block of the N=1 line: AUTO's kernel, HIP events around the launches."""
    g = torch.Generator(device=dev).manual_seed(8000)
    mk = lambda: (torch.rand(B_PER_GPU, H, 8192, D, generator=g, device=dev) * 2 - 1).to(torch.float8_e4m3fn)  # noqa: E731
    q, k, v = mk(), mk(), mk()
    step = fa.ForwardPlan(q, k, v, is_causal=True).launch
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.1:
        for _ in range(5):
            step()
        torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize(dev)
    ms = a.elapsed_time(b) / iters
    tf = fa.algorithmic_flops(B_PER_GPU, H, 8192, D, True) / (ms * 1e-3) / 1e12
    return {"workload": f"BASELINE.json configs[4]: seqlen=8192 head_dim={D} batch={B_PER_GPU} heads={H} fp8_e4m3 in / fp32 accumulate / bf16 out, causal",
            "tflops": round(tf, 2), "ms_per_step": round(ms, 4), "kernel": fa.forward_kernel_name("fp8_e4m3", D, True, B_PER_GPU, H, 8192),
            "frac_of_bf16_mfma_peak": round(tf / PEAK_TFLOPS_BF16, 4), "steps": iters}


def rehearsal(args, ranks) -> int:
    """The N>1 control path on CPU (gloo): rank discovery, sharding, barrier and the max/sum reductions
    with the real launcher/spawner in front -- what tests/test_sharding.py drives. No kernel runs."""
    if os.environ.get("FA_BENCH_FAIL_RANK") == os.environ.get("RANK"):  # tests: a rank that dies before the first barrier
        sys.exit(3)
    info = ranks.init_ranks(use_gpu=False)
    lo, hi = ranks.my_slices(info, B_PER_GPU * H)
    ranks.barrier(info)
    units = float(hi - lo) * args.steps
    mine = 0.001 * (info.rank + 1)  # rank r "takes" r+1 ms
    per_s, worst = ranks.aggregate_throughput(info, units, mine)
    per_rank = ranks.gather_over_ranks(info, units / mine)
    if info.rank == 0:
        print(json.dumps({"rehearsal": True, "n_gpus": info.world, "backend": info.backend, "slices_rank0": [lo, hi],
                          "slices_total": B_PER_GPU * H * info.world, "units_per_s": per_s, "worst_s": worst,
                          "per_rank": {"units_per_s": per_rank, "min": min(per_rank), "max": max(per_rank)}}), flush=True)
    ranks.finalize(info)
    return 0


def sweep(fa, torch, dev):
    """ms and TFLOP/s vs seqlen (the metric's other half): head_dim=64, bf16, causal, B*H=64."""
    rows = []
    for n in (128, 256, 512, 1024, 2048, 4096, 8192, 16384):
        bh = 64
        g = torch.Generator(device=dev).manual_seed(n)
        mk = lambda: (torch.rand(1, bh, n, D, generator=g, device=dev) * 2 - 1).to(torch.bfloat16)  # noqa: E731
        q, k, v = mk(), mk(), mk()
        o = torch.empty_like(q)
        lse = torch.empty(1, bh, n, dtype=torch.float32, device=dev)
        # validated once, launched many times: below N = 1024 the Python-side checks of flash_attention_forward cost
        # as much as the kernel runs and the row would measure the host
        plan = fa.ForwardPlan(q, k, v, is_causal=True, out=o, lse=lse)
        # per-row warm-up by time, like the headline: the short rows before this one leave the chip lightly loaded and
        # the clocks take tens of milliseconds to come back (5 warm-up launches put the N=4096 row 3-5 % under `value`)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.06:
            for _ in range(20 if n <= 4096 else 4):
                plan.launch()
            torch.cuda.synchronize(dev)
        # same method as the headline: HIP events around blocks of 10 back-to-back launches (an event pair around
        # every single launch adds a host-side gap of several microseconds, which dominated the short rows)
        nblk, per = (6, 10) if n <= 4096 else (3, 4)
        evs = []
        for _ in range(nblk):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per):
                plan.launch()
            b.record()
            evs.append((a, b))
        torch.cuda.synchronize(dev)
        ms = sorted(a.elapsed_time(b) / per for a, b in evs)[nblk // 2]
        tf = fa.algorithmic_flops(1, bh, n, D, True) / (ms * 1e-3) / 1e12
        rows.append({"seqlen": n, "ms": round(ms, 5), "tflops": round(tf, 2), "mfma_frac": round(tf / PEAK_TFLOPS_BF16, 4)})
    return rows


if __name__ == "__main__":
    sys.exit(main())
