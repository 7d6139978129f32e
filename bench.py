#!/usr/bin/env python3
"""bench.py — headline benchmark: queries/sec, FLAT-IP 10M x 768 float32, batch 256, k=10.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
      --master-port P bench.py --gpus N --steps K --warmup W

One "step" = one batch of `--batch` queries answered against the WHOLE collection.  With N>1 the
collection is row-sharded (global row g lives on rank g % N, VectorStore/cluster sharding §8e), every
rank scans its shard for the whole batch, per-shard (distance,row) candidates are exchanged with one
RCCL all-gather and merged on the device: total work is fixed -> "scaling": "strong".
Inputs (rows and queries) are resident in HBM before the timed region; the timed region is bracketed
by barrier + torch.cuda.synchronize() and the MAX over ranks is reported.

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints its line; "roofline" and the
pipeline figures on it come from HIP events recorded inside the timed steps.  Everything that takes work of its own —
the latency of one blocking batch, two batches in flight, verification against torch and the oracle, "cpu_baseline",
the other metrics, distribution and BASELINE configurations (c2), the second data set (c4) — runs only with --full.

Extra objects on the JSON line: "roofline" (dominant kernel k_scan_qs: the bytes it physically streams and its matrix
ops over the HIP-event duration of its launches on the launch stream inside the timed region, against 8 TB/s and the
dense MFMA peak; `bound` names the BINDING resource from the committed rocprofv3 --pmc pass of that kernel —
profiles/rNN_binding.json: the int8 matrix pipe at the power-capped clock for the headline —, `binding` carries its
counters, `hbm` / `mfma` both live fractions; the SURVEY 8(d) algorithmic-f32-bytes figure rides along) and
"cpu_baseline" (the oracle's restatement of the reference's rayon scan on a persistent pinned pool, timed on this host's
cores over a bounded row sample: ONE protocol — 20 warm-ups + 30 queries — for the thread sweep and the figure, the best
thread count run three times, median / best / spread / host CPU model and NUMA layout on the line; --full).
`configs` (--full) holds the other BASELINE.json configurations at one GPU's share: `ms` = the blocking C-ABI call through
ctypes with prebuilt arguments, `ms_python_wrapper` = the same through lynsedb_amd's Python wrapper + a torch synchronise.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense f16/bf16 MFMA peak (no sparsity)
MFMA_I8_PEAK_TOPS = 5000.0     # dense int8 MFMA: twice the f16 rate (MI355X_MICROARCH.md: i8 = 2x K per instruction at the same issue rate)
MFMA_FP4_PEAK_TOPS = 10000.0   # dense FP4 / FP6 MFMA (MI355X_MICROARCH.md: ~10 PF dense; v_mfma_scale_f32_32x32x64_f8f6f4)
GEN_BLOCK = 100_000     # rows per generation block (flat_search_bench.py:71-77 batches of 100k)


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rows", type=int, default=10_000_000, help="TOTAL rows of the collection")
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--metric", default="ip")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--full", action="store_true",
                   help="also run everything beyond the headline figure, outside the timed steps: the latency of one blocking batch, two batches "
                        "in flight, verification against torch / the oracle, the CPU baseline, the other metrics, distribution and BASELINE "
                        "configurations (c2), the second data set (c4); the --no-* switches below leave parts of it out")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--cpu-sample-rows", type=int, default=1_000_000)
    p.add_argument("--cpu-queries", type=int, default=30, help="timed CPU queries (flat_search_bench.py:94-97: 30 trials)")
    p.add_argument("--cpu-warmup", type=int, default=20, help="CPU warm-up queries (flat_search_bench.py:88-91: 20)")
    p.add_argument("--no-verify", action="store_true")
    p.add_argument("--verify-queries", type=int, default=16)
    p.add_argument("--stage0", type=int, default=0, help="override the stage-0 row count of the scan plan")
    p.add_argument("--growth", type=int, default=0, help="override the stage growth factor of the scan plan")
    p.add_argument("--profile-every", type=int, default=0, help="HIP-event timing of the scan launches on every n-th step of the timed region "
                   "(0 = default: 4; one GPU with batches in flight: 6, and those steps run as BLOCKING calls on a drained device)")
    p.add_argument("--settle-ms", type=float, default=60.0, help="untimed steps before the warm-up until the GPU's clocks have settled (0 = none)")
    p.add_argument("--no-configs", action="store_true", help="skip the extra keys: the other BASELINE configurations and the second data distribution")
    p.add_argument("--config", default="c2", choices=["c2", "c4", "c5"],
                   help="c2 (default): FLAT-IP 10M x 768, the headline; c4: IVF-Flat IP nlist 4096 / nprobe 32, 6.25M x 768 rows PER GPU "
                        "(50M x 768 at --gpus 8, BASELINE.json configs[3]), centroids trained over the sharded collection; c5: packed-binary Hamming, "
                        "12.5M x 1024-bit fingerprints PER GPU (100M at --gpus 8, configs[4]), k = 50")
    p.add_argument("--rows-per-gpu", type=int, default=6_250_000, help="--config c4: rows of every rank's shard")
    p.add_argument("--nlist", type=int, default=4096)
    p.add_argument("--nprobe", type=int, default=32)
    p.add_argument("--train-iters", type=int, default=20, help="--config c4: Lloyd iterations of the sharded k-means (IVFIndex::build trains 20: src/index/ivf.rs:163-170)")
    p.add_argument("--centres", type=int, default=4096, help="--config c4: generating centres of the clustered collection (benchmarks/ivf_kmeans_baseline.py:45-55)")
    p.add_argument("--no-second-dataset", action="store_true", help="--config c4: skip the second collection (1024 generating centres != nlist)")
    p.add_argument("--launch-timeout", type=float, default=1500.0, help="--gpus N without a launcher: seconds the self-started N-rank run may take")
    p.add_argument("--in-flight", type=int, default=int(os.environ.get("LYNSE_BENCH_IN_FLIGHT", "0")),
                   help="batches in flight (lynse_hip_flat_search_submit_* / _wait): step i+1 is enqueued before step i is waited "
                        "for; 1 = the blocking entry points (one host round trip per step); 0 = default: 1 on one GPU (the "
                        "kernel durations of the roofline stay undisturbed; in flight gains < 1 %% there), 3 on a sharded collection")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step returned (ids / distances / counts of the batch) to DIR/<name>.npy "
                        "(rank 0; float64 / float32): the inputs depend on the arguments only, so two builds can be compared output for output")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be at least 1")
    if args.warmup < 0:
        p.error("--warmup must not be negative")
    return args


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirpath, out, B, K):
    """--dump-outputs: the arrays a caller of the timed path receives for the batch — global row ids (`ids.npy`, float64: exact below
    2**53, an empty slot is 2**64 - 1), distances (`distances.npy`, float32 as returned) and the number of results per query (`counts.npy`) —
    written from the host copies of `out` (a ShardOutputs).  Above DUMP_LIMIT_BYTES a fixed, seeded sample of the queries is written, and
    `query_index.npy` names which."""
    d = Path(dirpath)
    d.mkdir(parents=True, exist_ok=True)
    ids = out.rows[:B].cpu().numpy().view(np.uint64).astype(np.float64)
    dists = out.dists[:B].cpu().numpy().astype(np.float32)
    counts = out.counts[:B].cpu().numpy().view(np.uint32).astype(np.float64)
    qidx = np.arange(B, dtype=np.float64)
    per_query = K * (8 + 4) + 8 + 8
    if B * per_query > DUMP_LIMIT_BYTES:
        sel = np.sort(np.random.default_rng(0).choice(B, DUMP_LIMIT_BYTES // per_query, replace=False))
        ids, dists, counts, qidx = ids[sel], dists[sel], counts[sel], qidx[sel]
    files = []
    for name, a in (("counts", counts), ("distances", dists), ("ids", ids), ("query_index", qidx)):
        np.save(d / ("%s.npy" % name), np.ascontiguousarray(a))
        files.append("%s.npy" % name)
    return files


def gen_block(block: int, rows_in_block: int, dim: int, seed: int, device) -> torch.Tensor:
    """Global rows [block*GEN_BLOCK, +rows_in_block): uniform[0,1) f32, identical for every world size."""
    g = torch.Generator(device=device)
    g.manual_seed(seed * 1_000_003 + block)
    return torch.rand((rows_in_block, dim), generator=g, device=device, dtype=torch.float32)


def self_launch(args) -> int:
    """`python bench.py --gpus N` without a launcher: start N ranks with torch.distributed.run on 127.0.0.1 and pass their
    output through (rank 0 prints the JSON line).  A rank that dies takes the others down with it (torchrun's agent kills the
    remaining workers), and the whole run is bounded by --launch-timeout: a hang ends with a JSON error line and a non-zero exit
    code instead of a silent stall (the fan-out this replaces: src/cluster.rs:173-217)."""
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    try:
        rc = subprocess.run(cmd, env=env, timeout=args.launch_timeout).returncode
    except subprocess.TimeoutExpired:
        rc = 124
    if rc != 0:
        print(json.dumps({"metric": "queries/sec, FLAT-%s %dx%d float32, batch=%d, k=%d" % (args.metric.upper(), args.rows, args.dim, args.batch, args.k),
                          "value": None, "n_gpus": args.gpus, "error": "the %d-rank run ended with exit code %d%s" % (
                              args.gpus, rc, " (launch timeout %.0f s)" % args.launch_timeout if rc == 124 else "")}), flush=True)
    return rc


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(self_launch(args))
    # ONE JSON line on stdout: everything else that writes to fd 1 during the run (RCCL prints a version / host banner when
    # its first communicator is created) goes to stderr instead; the result line is written to the saved descriptor.
    sys.stdout.flush()
    result_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    local_rank %= torch.cuda.device_count()  # (a 1-GPU box can still smoke-test the N>1 code path with LYNSE_BENCH_BACKEND=gloo)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    os.environ["LYNSE_HIP_DEVICE"] = str(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("LYNSE_BENCH_BACKEND", "nccl")  # "nccl" is RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)

    import lynsedb_amd as L
    from lynsedb_amd.sharded import ShardedFlat

    if args.config == "c4":
        return run_c4(args, rank, local_rank, world, dev, dist, result_out)
    if args.config == "c5":
        return run_c5(args, rank, local_rank, world, dev, dist, result_out)

    N, D, B, K = args.rows, args.dim, args.batch, args.k
    metric = L.metric_from_str(args.metric)

    # ---- build the shard: rows g with g % world == rank, generated block-wise on the device
    sh = ShardedFlat(D, rank=rank, world=world, device=local_rank, group=dist)
    native = False
    if world > 1 and os.environ.get("LYNSE_BENCH_EXCHANGE", "native") == "native" and (dist is None or dist.get_backend() == "nccl"):
        native = sh.enable_native_comm()   # RCCL inside the library; falls back to torch.distributed's all-gather
        if sh.ranks_seen is not None and sh.ranks_seen != world:   # a communicator that does not span the job: no number is better than a wrong one
            if rank == 0:
                result_out.write(json.dumps({"metric": "queries/sec", "value": None, "n_gpus": world,
                                             "error": "the RCCL communicator saw %s of %d ranks (%s)" % (sh.ranks_seen, world, sh.comm_error)}) + "\n")
                result_out.flush()
            raise SystemExit(3)
    if world == 1 and os.environ.get("LYNSE_BENCH_FORCE_COMM") == "1":
        # one GPU, but the batches in flight go through a 1-rank RCCL communicator: the exchange half of a sharded step
        # (status word in the result block, event hand-over to the exchange stream, merge kernel) without the all-gather
        from lynsedb_amd.sharded import NativeComm

        sh.comm = NativeComm(None, 0, 1, local_rank)
        native = True
    n_local = (N - rank + world - 1) // world if N > rank else 0
    sh.index.reserve(max(n_local, 1))
    if args.stage0 or args.growth:
        sh.index.set_plan(args.stage0 or 4096, args.growth or 8, 8192)
    qrng = np.random.default_rng(args.seed + 7)
    q_rows = np.sort(qrng.integers(0, N, size=B))
    q_src = torch.empty((B, D), device=dev, dtype=torch.float32)
    t0 = time.time()
    for b in range((N + GEN_BLOCK - 1) // GEN_BLOCK):
        r0 = b * GEN_BLOCK
        nb = min(GEN_BLOCK, N - r0)
        blk = gen_block(b, nb, D, args.seed, dev)
        sel = np.nonzero((q_rows >= r0) & (q_rows < r0 + nb))[0]
        if sel.size:
            q_src[torch.as_tensor(sel, device=dev)] = blk[torch.as_tensor(q_rows[sel] - r0, device=dev)]
        first = (rank - r0) % world  # first local row of this block owned by this rank
        mine = blk[first::world].contiguous()
        if mine.shape[0]:
            sh.index.write_device(mine)
        del blk, mine
    sh.index.finalize()
    torch.cuda.synchronize()
    build_s = time.time() - t0
    # the derived copies this workload reads (SQ8 codes of the certified int8 pass: +1 B per element) are built HERE, timed,
    # and not inside the first warm-up search
    t1 = time.time()
    sh.index.prepare(metric, B)
    torch.cuda.synchronize()
    prepare_s = time.time() - t1
    hbm_bytes = sh.index.hbm_bytes()
    assert len(sh.index) == n_local, (len(sh.index), n_local)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed + 11)
    queries = (q_src + 0.03 * torch.randn((B, D), generator=g, device=dev, dtype=torch.float32)).contiguous()

    # Batches in flight: the reference answers concurrent readers (Arc<RwLock<Collection>>, src/python/mod.rs:950, :1187);
    # here step i+1 is ENQUEUED (scan -> selects -> rescoring [-> all-gather -> merge]) before step i is waited for, each on
    # its own search context and output buffers.  Every one of the K steps is complete — overflow flags checked, results
    # final — inside the timed region.
    # One GPU: the timed steps are BLOCKING calls by default (kernel durations under rocprofv3 and the HIP-event brackets of the roofline
    # then agree; with tickets in flight a kernel's profiler duration includes the time it waits for CUs behind another batch).  Between
    # two blocking calls the device idles for the host's turn-around (completion -> Python -> the next call's first launch: 27-34 us in
    # the kernel trace of every step, 1.5 % of the 10M step); `--in-flight 2` hides it behind a second ticket (the steps whose scan
    # launches carry HIP events still run as blocking calls on a drained device) — that figure is reported as
    # `two_in_flight_ms_per_step`, measured right behind the timed region.
    in_flight = max(1, min(args.in_flight, 4)) if args.in_flight > 0 else (1 if world == 1 else 3)
    if world > 1 and not native:
        in_flight = 1   # (the torch.distributed fallback of the exchange is a blocking collective)
    if args.profile_every <= 0:
        args.profile_every = 6 if (world == 1 and in_flight > 1) else 4   # (one GPU with --in-flight N: fewer drained steps)
    outs_default = [sh.alloc_outputs(B, K) for _ in range(in_flight)]
    out = outs_default[0]

    def run_steps(n, drain_every=0, in_flight=in_flight, outs=None):
        # drain_every = n > 0 (one GPU, timed region): step 0, n, 2n, ... is the library's profiled search (profile_enable(n) counts
        # searches from 0): it runs blocking, after the tickets in flight have been waited for
        outs = outs if outs is not None else outs_default
        if in_flight == 1:
            for _ in range(n):
                sh.search_device(queries, K, metric, out)
            return
        pending = []
        trace = os.environ.get("LYNSE_BENCH_TRACE_STEPS") == "1"   # (development: completions that come > 1 ms apart, to stderr)
        last = time.perf_counter()
        for i in range(n):
            if drain_every and i % drain_every == 0:
                for t in pending:
                    t.wait()
                pending = []
                sh.search_device(queries, K, metric, out)
                continue
            pending.append(sh.search_submit(queries, K, metric, outs[i % in_flight]))
            if len(pending) >= in_flight:
                pending.pop(0).wait()
                if trace:
                    now = time.perf_counter()
                    if now - last > 1e-3:
                        print("slow completion: step %d of %d, %.2f ms" % (i, n, (now - last) * 1e3), file=sys.stderr)
                    last = now
        for t in pending:
            t.wait()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # Clock / power settling, BEFORE the W warm-up steps and outside every timed region: after any idle (the build, even a 50 ms
    # sleep) this GPU needs ~30 ms of continuous work to reach its steady state under this kernel — per-step times of the blocking
    # 10M x 768 x 256 search after an idle: 2.08 2.85 2.67 2.50 2.44 2.36 2.28 ... 2.06 from the 15th step on
    # (scripts/step_times.py, profiles/r03_step_times_after_idle.txt).  W = 5 steps of a 0.36 ms shard step would leave the whole
    # timed region of an 8-GPU run inside that ramp.  The settle phase runs the same step for --settle-ms (default 60 ms, at
    # least 3 steps); it is reported in config.settle_steps / settle_ms and is not counted in `warmup`.
    # (Python's cyclic GC is switched off from here to the end of the measurements, as timeit does: a full collection — it came
    # ~200 tickets into a run with batches in flight — stalls the submitting thread for ~43 ms, 130 shard steps)
    import gc
    gc.collect()
    gc.disable()
    settle_steps = 0
    if args.settle_ms > 0:
        # the number of settle steps must be the SAME on every rank (a sharded step is a collective): three steps timed on every
        # rank, the slowest rank's step time agreed on, then as many steps as fill settle_ms at that rate
        probe = max(3, in_flight)
        run_steps(probe)                     # (first calls: workspace / context creation, not a step time)
        torch.cuda.synchronize()
        t_settle = time.perf_counter()
        run_steps(probe)
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t_settle) * 1e3 / probe
        if dist is not None:
            t = torch.tensor([step_ms], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            step_ms = float(t.item())
        more = min(2000, max(0, int(np.ceil(args.settle_ms / max(step_ms, 1e-3))) - 2 * probe))
        if more:
            run_steps(more)
            torch.cuda.synchronize()
        settle_steps = 2 * probe + more
    run_steps(args.warmup)
    # HIP events around the scan launches of every 4th step inside the timed region (each recorded event costs the stream a
    # few microseconds: timing every step added 30-40 us to each)
    sh.index.profile_enable(args.profile_every)
    sh.index.profile_get(reset=True)
    barrier()
    t_start = time.perf_counter()
    drain_every = args.profile_every if (world == 1 and in_flight > 1) else 0
    run_steps(args.steps, drain_every)
    barrier()
    elapsed = time.perf_counter() - t_start
    prof = sh.index.profile_get(reset=True)
    sh.index.profile_enable(False)
    dumped = None
    if args.dump_outputs and rank == 0:   # the buffers the LAST timed step wrote (a drained step: `out`; a ticket: its own)
        last = out if (in_flight == 1 or (drain_every and (args.steps - 1) % drain_every == 0)) else outs_default[(args.steps - 1) % in_flight]
        dumped = dump_outputs(args.dump_outputs, last, B, K)
    lat_ms = two_ms = None
    if args.full:
        # (outside the timed region) latency of ONE blocking batch: the same step through the blocking entry points
        lat_steps = max(1, min(args.steps, 10))
        barrier()
        t_lat = time.perf_counter()
        for _ in range(lat_steps):
            sh.search_device(queries, K, metric, out)
        barrier()
        lat_ms = (time.perf_counter() - t_lat) / lat_steps * 1000.0
        if world == 1 and in_flight == 1 and not args.no_configs:   # (outside the timed region; not in the lean profiling command) the same K steps with two tickets in flight
            outs2 = [sh.alloc_outputs(B, K) for _ in range(2)]
            run_steps(4, 0, 2, outs2)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            run_steps(args.steps, 0, 2, outs2)
            torch.cuda.synchronize()
            two_ms = (time.perf_counter() - t2) / args.steps * 1000.0
    if dist is not None:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    gc.enable()
    # ---- verification (--full, outside the timed region): recall@k and score agreement vs torch fp32
    verify = None
    if args.full and not args.no_verify:
        verify = sh.verify_against_torch(queries, K, metric, out, nverify=min(args.verify_queries, B))
        if world == 1 and metric == 0 and rank == 0:
            verify.update(oracle_distance_bits(sh.index, queries, out, B, K))

    result = None
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1000.0
        qps = B * args.steps / elapsed
        scan_s = prof["scan_us"] * 1e-6
        launches = max(int(prof["scan_launches"]), 1)
        # one pass over the shard serves the whole batch -> algorithmic bytes per step = rows x row bytes.
        # (The launches of a step also re-scan the 65536 sample rows of the first stage: time counted, bytes not.)
        row_bytes = D * 4 if metric < 3 else ((D + 63) // 64) * 8
        timed_steps = max(int(prof["searches"]), 1)   # the steps whose launches carry HIP events (every --profile-every-th)
        alg_bytes = float(n_local) * row_bytes * timed_steps
        alg_gbps = (alg_bytes / scan_s / 1e9) if scan_s > 0 else 0.0
        prof["scan_bytes"] = int(alg_bytes)
        plan = int(prof.get("last_plan", 0))
        i8c = bool(plan & 4)
        # What the dominant kernel physically streams per row: the certified int8 coarse pass reads the 1-byte SQ8 codes,
        # the f16 coarse pass the 2-byte shadow (both resident copies built once at finalize); binary metrics the packed words.
        if metric >= 3:
            kernel, elem_bytes, mfma_peak, mfma_unit = "k_scan_binary_rows", None, None, None
            kernel_bytes = alg_bytes
        elif i8c:
            qs_tiling = ((plan >> 16) & 0xff) == 0x81   # threshold stages on the query-stationary tiling (scan_qs.h)
            kernel, elem_bytes, mfma_peak, mfma_unit = ("k_scan_qs<6,2,6,3,...> (int8, query-stationary)" if qs_tiling else "k_scan_h16<2,4,4,2,IP,i8c>"), 1, MFMA_I8_PEAK_TOPS, "TOP/s"
            kernel_bytes = float(n_local) * (-(-D // 16) * 16) * timed_steps
        else:
            kernel, elem_bytes, mfma_peak, mfma_unit = "k_scan_h16<f16>", 2, MFMA_F16_PEAK_TFLOPS, "TFLOP/s"
            kernel_bytes = float(n_local) * (-(-D // 8) * 8) * 2 * timed_steps
        hbm_gbps = (kernel_bytes / scan_s / 1e9) if scan_s > 0 else 0.0
        # matrix work of the launches (sample rows included: they are really multiplied)
        ops = 2.0 * B * prof["scan_rows"] * D if metric < 3 else 0.0
        mfma_rate = (ops / scan_s / 1e12) if scan_s > 0 else 0.0
        frac_hbm = hbm_gbps / HBM_PEAK_GBPS
        frac_mfma = (mfma_rate / mfma_peak) if mfma_peak else 0.0
        traffic, traffic_note = None, "no PMC summary under profiles/ for this kernel"
        try:  # HBM bytes per launch from the committed PMC pass (bench.py itself cannot run rocprofv3 --pmc)
            pm_file = next(f for f in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json") if (ROOT / "profiles" / f).exists())
            pm = json.loads((ROOT / "profiles" / pm_file).read_text())
            pm = pm["i8c" if i8c else ("binary" if metric >= 3 else "f16")]
            traffic = int(kernel_bytes / launches * pm["ratio_hbm_over_kernel_bytes"])
            traffic_note = "from profiles/: kernel stream bytes x %.4f (FETCH_SIZE of a separate rocprofv3 --pmc pass, gfx950-corrected x2; profiles/%s)" % (
                pm["ratio_hbm_over_kernel_bytes"], pm_file)
        except Exception:
            pass
        # WHICH roofline binds: the resource the rocprofv3 --pmc pass of this kernel shows saturated (profiles/rNN_binding.json — the int8
        # matrix pipe for the 256-query scan: ~76 % busy at the ~1.4 GHz the 1400 W socket cap leaves, HBM at ~55 %), not the larger of the two
        # live fractions.  Without a PMC record for the shape (other batch sizes / metrics): the larger fraction, as before.
        bind = binding_of({"ip": "c2", "l2": "l2", "cosine": "cosine"}.get(str(args.metric).lower(), "")) if (B > 128 and metric < 3 and i8c) else None
        if bind is not None:
            hbm_bound = not bind["binding"].startswith("matrix pipe")
            bind["note"] = ("the counters come from the committed profile of this kernel at this shape (another box of the pool); achieved / frac beside it are "
                            "THIS run's HIP-event rates.  mfma_busy_frac counts cycles the pipe is occupied at the capped clock; frac = ops / nominal dense peak")
        else:
            hbm_bound = frac_hbm >= frac_mfma
        roofline = {
            # the binding PHYSICAL resource of the dominant kernel (named from the PMC pass), with BOTH live fractions side by side below
            "bound": "hbm" if hbm_bound else "mfma", "kernel": kernel, "binding": bind,
            "achieved": round(hbm_gbps if hbm_bound else mfma_rate, 1),
            "peak": HBM_PEAK_GBPS if hbm_bound else mfma_peak, "unit": "GB/s" if hbm_bound else mfma_unit,
            "frac": round(frac_hbm if hbm_bound else frac_mfma, 4), "traffic": traffic, "traffic_note": traffic_note,
            "hbm": {"achieved": round(hbm_gbps, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(frac_hbm, 4),
                    "bytes_per_launch": int(kernel_bytes // launches), "element_bytes": elem_bytes},
            "mfma": {"achieved": round(mfma_rate, 1), "peak": mfma_peak, "unit": mfma_unit, "frac": round(frac_mfma, 4)},
            # SURVEY 8(d) accounting: algorithmic f32 bytes (rows x dim x 4 B per step) / the same HIP-event time.  NOT a
            # roofline for this design (the kernel never reads the f32 rows): kept as the figure 8(d) defines.
            "algorithmic": {"achieved": round(alg_gbps, 1), "unit": "GB/s", "frac_of_hbm_peak": round(alg_gbps / HBM_PEAK_GBPS, 4),
                            "bytes_per_launch": int(alg_bytes // launches)},
            "launches": launches, "avg_launch_us": round(prof["scan_us"] / launches, 2),
            "launches_per_step": round(launches / timed_steps, 2), "timed_steps": timed_steps,
            "plan": {"sampled": bool(plan & 1), "threshold_only_sample": bool(plan & 2), "int8_coarse_pass": i8c,
                     "segmented_emission": bool(plan & 8), "fused_sample_stage": bool(plan & 128), "stages": (plan >> 8) & 0xff,
                     "tiling": hex((plan >> 16) & 0xff), "self_tightening_single_launch": bool(plan & (1 << 24))},
            "note": ("rank-0 shard; time = sum of HIP-event durations of the scan launches on the launch stream, every %d-th step of the timed region" % max(args.profile_every, 1))
                    + ("; with %d batches in flight the event brackets of a launch also hold the time it waits for CUs behind other batches' kernels "
                       "(kernel durations proper: the one-GPU line / profiles/)" % in_flight if (in_flight > 1 and world > 1) else "")
                    + ("; %d batches in flight, the event-timed steps run as blocking calls on a drained device" % in_flight if (in_flight > 1 and world == 1) else ""),
        }
        result = {
            "metric": "queries/sec, FLAT-%s %dx%d float32, batch=%d, k=%d" % (args.metric.upper(), N, D, B, K),
            "value": round(qps, 1), "unit": "queries/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
            "scaling": "strong", "vs_baseline": None,
            "dtype": "f32" if metric < 3 else "u64", "data": "synthetic",
            "dtype_note": ("returned distances are exact f32 (reference accumulation order, bit-identical to the oracle); "
                           "the scan is a certified %s MFMA prefilter (per-query error bound), survivors are rescored "
                           "from the f32 rows; roofline.algorithmic (SURVEY 8(d): rows x dim x 4 B per step) exceeds the HBM peak because the "
                           "scan streams the resident %d-byte codes, never the f32 rows — the physical fractions are roofline.hbm / roofline.mfma"
                           % ("int8" if i8c else "f16", 1 if i8c else 2)) if metric < 3 else "popcount over packed u64 words",
            "config": {"workload": "FLAT-%s %dx%d f32 uniform[0,1), %d queries = perturbed rows, k=%d"
                                   % (args.metric.upper(), N, D, B, K),
                       "rows_per_gpu": n_local, "sharding": "row %% %d" % world,
                       "exchange": ("rccl all_gather of %d B/rank, %s" % (B * K * 12 + B * 4, "inside the library (C-ABI), one stream" if native
                                    else "through torch.distributed (%s)" % (sh.comm_error or os.environ.get("LYNSE_BENCH_BACKEND", "nccl")))) if world > 1
                                   else ("1-rank communicator: merge without all-gather" if sh.comm is not None else "none"),
                       "rccl_ranks_seen": (sh.ranks_seen if native else None),
                       "batches_in_flight": in_flight, "settle_steps": settle_steps, "settle_ms": args.settle_ms,
                       "build_s": round(build_s, 1), "derived_build_s": round(prepare_s, 3),
                       "hbm_bytes_per_gpu": int(hbm_bytes), "hbm_bytes_over_f32_rows": round(hbm_bytes / max(n_local * D * 4, 1), 3)},
            "roofline": roofline,
            "pipeline_us_per_step": round(prof["total_us"] / max(prof["searches"], 1), 1),
            "rescored_per_query": round(prof["pool_entries"] / max(prof["searches"] * B, 1), 1),
            "fallback_queries": int(prof["fallback_queries"]),
        }
        if args.full:
            result["blocking_ms_per_batch"] = round(lat_ms, 4)
            result["two_in_flight_ms_per_step"] = round(two_ms, 4) if two_ms is not None else None
        if verify is not None:
            result["verify"] = verify
        if dumped is not None:
            result["dumped_outputs"] = {"dir": str(args.dump_outputs), "files": dumped}
        if args.full and not args.no_cpu_baseline and world == 1:   # (rank 0 at N = 1 only: the other ranks of a sharded run would sit in the barrier)
            result["cpu_baseline"] = cpu_baseline(args, N, D, K, metric)
        if args.full and world == 1 and not args.no_configs and metric == 0:
            # OUTSIDE the headline's timed region: the same workload on a second distribution (the certified int8 margin is
            # data dependent) and the other BASELINE.json configurations at one GPU's share, each with its own time, rate,
            # roofline fraction and an oracle-parity bool.  The headline index is released first.
            try:
                result["same_shard_variants"] = same_shard_variants(sh.index, queries, B, K, n_local, D)
            except Exception as e:  # noqa: BLE001
                result["same_shard_variants"] = {"error": repr(e)}
            del sh, outs_default, out
            torch.cuda.empty_cache()
            try:
                result["second_distribution"] = second_distribution(args, dev)
            except Exception as e:  # noqa: BLE001
                result["second_distribution"] = {"error": repr(e)}
            result["configs"] = other_configs(dev)
        result_out.write(json.dumps(result) + "\n")
        result_out.flush()
    if dist is not None:
        dist.barrier()
        if sh.comm is not None:   # the library's communicator goes first, while every rank is still alive
            try:
                sh.comm.close()
            except Exception:  # noqa: BLE001
                pass
            sh.comm = None
        dist.destroy_process_group()


def run_c4(args, rank, local_rank, world, dev, dist, result_out):
    """BASELINE.json configs[3]: IVF-Flat IP, nlist 4096 / nprobe 32 / k 10 over a collection row-sharded across the ranks (6.25M x
    768 rows per GPU: 50M x 768 at 8 GPUs; "scaling": "weak").  Build inside the job, nothing supplied from outside: every rank
    generates ITS rows (global row g = l * world + rank: unit centre g % 4096 + sigma 0.03 noise, benchmarks/ivf_kmeans_baseline.py:45-55),
    the centroids are trained over the whole collection by the all-reduced k-means (lynse_hip_ivf_kmeans_sharded: one ncclAllReduce
    of nlist x D sums + nlist counts per Lloyd iteration), every rank files its rows under them.  A step = one batch of 256 queries:
    centroid ranking, local list scans (certified int8 pass), exact rescoring, ncclAllGather of the (distance, row) blocks, device
    merge — batches in flight through lynse_hip_ivf_search_submit_f32_device, every step final inside the timed region."""
    import lynsedb_amd as L
    from lynsedb_amd.sharded import ShardedIvf, ShardOutputs

    D, B, K, nlist, nprobe = args.dim, args.batch, args.k, args.nlist, args.nprobe
    n_local = args.rows_per_gpu
    N = n_local * world
    KC = int(getattr(args, "_c4_centres", args.centres))
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    centers = torch.randn((KC, D), generator=g, device=dev)      # the same on every rank
    centers /= centers.norm(dim=1, keepdim=True) + 1e-12

    def gen_block(b0, e):
        """rows [b0, e) of this rank: centre (global row % KC) + sigma 0.03 noise, RE-NORMALISED (ivf_kmeans_baseline.py:49-53: `data /= norm`)"""
        gids = torch.arange(b0, e, device=dev) * world + rank
        blk = centers[gids % KC] + 0.03 * torch.randn((e - b0, D), generator=g, device=dev)
        blk /= blk.norm(dim=1, keepdim=True) + 1e-12
        return gids, blk

    g.manual_seed(1000 + rank)                                   # the noise of this rank's rows
    t0 = time.time()
    rows_d = torch.empty((n_local, D), device=dev, dtype=torch.float32)
    for b0 in range(0, n_local, 250_000):
        e = min(n_local, b0 + 250_000)
        rows_d[b0:e] = gen_block(b0, e)[1]
    torch.cuda.synchronize()
    gen_s = time.time() - t0
    sh = ShardedIvf(D, rank=rank, world=world, device=local_rank, group=dist)
    native = False
    if world > 1 and (dist is None or dist.get_backend() == "nccl"):
        native = sh.enable_native_comm()
    t0 = time.time()
    cen, asg = sh.train(rows_d, N, nlist, args.train_iters, "ip")
    torch.cuda.synchronize()
    train_s = time.time() - t0
    t0 = time.time()
    sh.load_local_device(rows_d, cen, asg, "ip")
    del rows_d
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    load_s = time.time() - t0
    # queries: perturbed rows of the collection (every rank builds the same batch: rank 0's choice is broadcast)
    g.manual_seed(99)
    qsel = torch.randint(0, KC, (B,), generator=g, device=dev)
    queries = centers[qsel] + 0.03 * torch.randn((B, D), generator=g, device=dev)
    queries = (queries / (queries.norm(dim=1, keepdim=True) + 1e-12)).contiguous()
    if dist is not None:
        dist.broadcast(queries, src=0)
    in_flight = max(1, min(args.in_flight, 3)) if args.in_flight > 0 else 3
    if world > 1 and not native:
        in_flight = 1
    outs = [ShardOutputs(B, K, world, dev) for _ in range(in_flight)]

    def run_steps(n):
        if in_flight == 1:
            for _ in range(n):
                sh.search_device(queries, K, nprobe, outs[0])
            return
        pending = []
        for i in range(n):
            pending.append(sh.search_submit(queries, K, nprobe, outs[i % in_flight]))
            if len(pending) >= in_flight:
                pending.pop(0).wait()
        for t in pending:
            t.wait()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    import gc
    gc.collect()
    gc.disable()
    run_steps(max(3, in_flight) * 2)            # first calls: derived data (SQ8 codes), workspaces, contexts
    torch.cuda.synchronize()
    run_steps(20)                               # clocks
    run_steps(args.warmup)
    if args.full:
        sh.index.profile_enable(True)
        sh.index.profile_get(reset=True)
        barrier()
        for _ in range(3):                      # scan-launch timing on three BLOCKING steps outside the timed region (tickets are not profiled)
            sh.search_device(queries, K, nprobe, outs[0])
        prof = sh.index.profile_get(reset=True)
        sh.index.profile_enable(False)
    barrier()
    t_start = time.perf_counter()
    run_steps(args.steps)
    barrier()
    elapsed = time.perf_counter() - t_start
    dumped = None
    if args.dump_outputs and rank == 0 and not getattr(args, "_c4_second", False):   # (the headline collection's last timed step)
        dumped = dump_outputs(args.dump_outputs, outs[(args.steps - 1) % in_flight], B, K)
    if args.full:
        barrier()
        t_lat = time.perf_counter()
        for _ in range(5):
            sh.search_device(queries, K, nprobe, outs[0])
        barrier()
        lat_ms = (time.perf_counter() - t_lat) / 5 * 1000.0
    if dist is not None:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    gc.enable()
    stats = sh.index.ticket_stats()
    if args.full:
        # ---- verification, outside the timed region: (a) tickets == the blocking sharded search, bit for bit; (b) recall@k against the
        # exact top-k of the WHOLE collection (torch fp32 matmul over every rank's rows, candidates gathered and merged)
        o_t, o_b = ShardOutputs(B, K, world, dev), ShardOutputs(B, K, world, dev)
        sh.search_submit(queries, K, nprobe, o_t).wait()
        sh.search_device(queries, K, nprobe, o_b)
        torch.cuda.synchronize()
        same = bool(torch.equal(o_t.rows, o_b.rows) and torch.equal(o_t.dists, o_b.dists) and torch.equal(o_t.counts, o_b.counts))
        nv = min(args.verify_queries, B)
        best_s = torch.full((nv, K), -float("inf"), device=dev)
        best_r = torch.zeros((nv, K), dtype=torch.int64, device=dev)
        # (the slab-ordered rows live inside the library: this rank's rows are regenerated block-wise from the same generator state)
        g.manual_seed(1000 + rank)
        for b0 in range(0, n_local, 250_000):
            e = min(n_local, b0 + 250_000)
            gids, blk = gen_block(b0, e)
            sc = queries[:nv] @ blk.T
            cs, ci = torch.cat([best_s, sc], dim=1).topk(K, dim=1)
            allr = torch.cat([best_r, gids.unsqueeze(0).expand(nv, -1)], dim=1)
            best_s, best_r = cs, torch.gather(allr, 1, ci)
            del blk, sc
        if dist is not None:
            gs = [torch.empty_like(best_s) for _ in range(world)]
            gr = [torch.empty_like(best_r) for _ in range(world)]
            dist.all_gather(gs, best_s)
            dist.all_gather(gr, best_r)
            cs, ci = torch.cat(gs, dim=1).topk(K, dim=1)
            best_r = torch.gather(torch.cat(gr, dim=1), 1, ci)
        got = o_b.rows[:nv].cpu().numpy()
        exact = best_r.cpu().numpy()
        recall = float(np.mean([len(set(got[i].tolist()) & set(exact[i].tolist())) / K for i in range(nv)]))
        del o_t, o_b
    result = None
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1000.0
        qps = B * args.steps / elapsed
        result = {
            "metric": "queries/sec, IVF-Flat IP %dx%d float32, nlist=%d nprobe=%d, batch=%d, k=%d" % (N, D, nlist, nprobe, B, K),
            "value": round(qps, 1), "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": "C4 IVF-Flat IP %dx%d f32 (%d unit centres + sigma 0.03 noise, rows re-normalised: benchmarks/ivf_kmeans_baseline.py:45-55), "
                                   "nlist=%d nprobe=%d, %d queries, k=%d" % (N, D, KC, nlist, nprobe, B, K),
                       "what_it_measures": ("with as many generating centres as lists recall 1.0 is by construction; at 256 queries x %d probes the batch touches most of the "
                                            "%d lists (rows_scanned_per_step of rows_per_gpu): at this batch size the step is a FLAT scan of the probed share — "
                                            "`second_dataset` (centres != nlist) is the recall MEASUREMENT, blocking_ms_per_batch / the c4_share single-query figure say "
                                            "what the index buys" % (nprobe, nlist)) if KC == nlist else "centres != nlist: recall is a measurement",
                       "rows_per_gpu": n_local, "sharding": "row %% %d of every list, one set of centroids" % world,
                       "training": "all-reduced k-means over the sharded collection, %d Lloyd iterations (%s)" % (
                           args.train_iters, "ncclAllReduce inside the library" if native else ("torch.distributed" if world > 1 else "one rank")),
                       "exchange": ("rccl all_gather of %d B/rank inside the library" % (B * K * 12 + B * 4 + 16)) if native else
                                   ("torch.distributed" if world > 1 else "none"),
                       "batches_in_flight": in_flight, "generate_s": round(gen_s, 1), "train_s": round(train_s, 1), "load_s": round(load_s, 1),
                       "lists_trained": int(cen.shape[0])},
            "tickets": stats,
        }
        if args.full:
            plan = int(prof.get("last_plan", 0))
            i8c = bool(plan & 4)
            launches = max(int(prof["scan_launches"]), 1)
            scan_s = prof["scan_us"] * 1e-6
            elem = 1 if i8c else 2
            kernel_bytes = float(prof["scan_rows"]) * D * elem            # rows of the probed lists the tiled scans streamed (3 steps)
            hbm_gbps = kernel_bytes / scan_s / 1e9 if scan_s > 0 else 0.0
            result["roofline"] = {"bound": "hbm", "kernel": "k_scan_h16<..,TILED,%s> over the probed lists" % ("I8C" if i8c else "F16"), "binding": binding_of("c4_share_nq256"),
                                  "achieved": round(hbm_gbps, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(hbm_gbps / HBM_PEAK_GBPS, 4),
                                  "traffic": None, "launches": launches, "avg_launch_us": round(prof["scan_us"] / launches, 2),
                                  "rows_scanned_per_step": int(prof["scan_rows"] // max(int(prof["searches"]), 1)),
                                  "note": "rank-0 shard, three blocking steps outside the timed region (HIP events around the tiled scan launches); "
                                          "bytes = rows of the probed lists x %d B/element" % elem}
            result["blocking_ms_per_batch"] = round(lat_ms, 4)
            result["verify"] = {"tickets_equal_blocking_search": same, "queries": nv, "recall_at_k_vs_exact_top_k_of_the_collection": recall}
        if dumped is not None:
            result["dumped_outputs"] = {"dir": str(args.dump_outputs), "files": dumped}
        if args.full and not args.no_cpu_baseline and world == 1 and not getattr(args, "_c4_second", False):
            try:
                result["cpu_baseline"] = cpu_baseline_ivf(args, N, D, K, nlist, nprobe, KC)
            except Exception as e:  # noqa: BLE001
                result["cpu_baseline"] = {"error": repr(e)}
    if sh.comm is not None:   # the library's communicator goes first, while every rank is still alive
        if dist is not None:
            dist.barrier()
        try:
            sh.comm.close()
        except Exception:  # noqa: BLE001
            pass
        sh.comm = None
    del sh, outs
    torch.cuda.empty_cache()
    if getattr(args, "_c4_second", False):
        return result if rank == 0 else None
    # ---- the second collection (--full): 1024 generating centres under the same nlist — lists do NOT coincide with the data's clusters, recall@k
    # against the exact top-k is a measurement (tests/test_gpu_baseline_configs.py::test_c4_* builds the same shape against the oracle)
    if args.full and not args.no_second_dataset and KC == nlist and nlist > 1024 // 4:
        args._c4_second, args._c4_centres = True, max(nlist // 4, 1)
        try:
            second = run_c4(args, rank, local_rank, world, dev, dist, result_out)
        finally:
            args._c4_second = False
        if rank == 0 and second is not None:
            result["second_dataset"] = {"centres": args._c4_centres, "ms_per_step": second["ms_per_step"], "queries_per_s": second["value"],
                                        "blocking_ms_per_batch": second["blocking_ms_per_batch"], "train_s": second["config"]["train_s"],
                                        "rows_scanned_per_step": second["roofline"]["rows_scanned_per_step"], "frac_of_hbm_peak": second["roofline"]["frac"],
                                        "verify": second["verify"]}
    if rank == 0:
        result_out.write(json.dumps(result) + "\n")
        result_out.flush()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def run_c5(args, rank, local_rank, world, dev, dist, result_out):
    """BASELINE.json configs[4]: packed-binary Hamming over 1024-bit fingerprints, k = 50, the collection row-sharded across the ranks
    (12.5M rows per GPU: 100M at 8 GPUs; "scaling": "weak").  A step = one batch of 256 packed queries: the +-1 FP4 MFMA scan of the
    shard (exact: margin 0), selects, ncclAllGather of the (distance, row) blocks, device merge — batches in flight through
    lynse_hip_flat_search_submit_packed_u64_device.  Integer path: ids and distances are bit-exact (checked against the oracle's
    packed search on a sample of this rank's rows and against the blocking sharded search)."""
    import lynsedb_amd as L
    import oracle as O
    from lynsedb_amd.sharded import ShardedFlat

    bits, B = 1024, args.batch
    K = 50 if args.k == 10 else args.k
    W = bits // 64
    n_local = 12_500_000 if args.rows == 10_000_000 else max(1, args.rows // world)
    N = n_local * world
    metric = L.metric_from_str("hamming")
    sh = ShardedFlat(bits, rank=rank, world=world, device=local_rank, group=dist)
    native = False
    if world > 1 and (dist is None or dist.get_backend() == "nccl"):
        native = sh.enable_native_comm()
    sh.index.reserve(n_local)
    g = torch.Generator(device=dev)
    g.manual_seed(4242 + rank)
    t0 = time.time()
    first_words = None
    for b0 in range(0, n_local, 2_500_000):
        nb = min(2_500_000, n_local - b0)
        w = torch.randint(-2**63, 2**63 - 1, (nb, W), generator=g, device=dev, dtype=torch.int64)
        if first_words is None:
            first_words = w[:min(nb, 200_000)].clone()      # the sample the oracle checks, and the source of the queries
        sh.index.write_packed_device(w)
        del w
    sh.index.finalize()
    torch.cuda.synchronize()
    build_s = time.time() - t0
    t0 = time.time()
    sh.index.prepare(metric, B)                             # the +-1 FP4 copy of the batched scan
    torch.cuda.synchronize()
    prepare_s = time.time() - t0
    # queries: rows of rank 0's shard with 16 bits flipped (every rank gets the same batch)
    queries = first_words[torch.arange(B, device=dev) * 701 % first_words.shape[0]].clone()
    queries[:, 0] ^= 0xFFFF
    if dist is not None:
        dist.broadcast(queries, src=0)
    in_flight = max(1, min(args.in_flight, 4)) if args.in_flight > 0 else (1 if world == 1 else 3)
    if world > 1 and not native:
        in_flight = 1
    outs = [sh.alloc_outputs(B, K) for _ in range(in_flight)]

    def run_steps(n):
        if in_flight == 1:
            for _ in range(n):
                sh.search_packed_device(queries, K, metric, outs[0])
            return
        pending = []
        for i in range(n):
            pending.append(sh.search_submit(queries, K, metric, outs[i % in_flight]))
            if len(pending) >= in_flight:
                pending.pop(0).wait()
        for t in pending:
            t.wait()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    import gc
    gc.collect()
    gc.disable()
    run_steps(max(3, in_flight) * 2)
    torch.cuda.synchronize()
    run_steps(20)
    run_steps(args.warmup)
    sh.index.profile_enable((args.profile_every if args.profile_every > 0 else 4))
    sh.index.profile_get(reset=True)
    barrier()
    t_start = time.perf_counter()
    run_steps(args.steps)
    barrier()
    elapsed = time.perf_counter() - t_start
    prof = sh.index.profile_get(reset=True)
    sh.index.profile_enable(False)
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, outs[(args.steps - 1) % in_flight], B, K)
    if args.full:
        barrier()
        t_lat = time.perf_counter()
        for _ in range(5):
            sh.search_packed_device(queries, K, metric, outs[0])
        barrier()
        lat_ms = (time.perf_counter() - t_lat) / 5 * 1000.0
    if dist is not None:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    gc.enable()
    if args.full:
        # ---- verification (outside the timed region): tickets == blocking sharded search; the scan kernels against the oracle on a
        # 200k-row index of this rank's first rows (same kernels, same batch: bit-exact ids and distances)
        o_t, o_b = sh.alloc_outputs(B, K), sh.alloc_outputs(B, K)
        sh.search_submit(queries, K, metric, o_t).wait()
        sh.search_packed_device(queries, K, metric, o_b)
        torch.cuda.synchronize()
        same = bool(torch.equal(o_t.rows, o_b.rows) and torch.equal(o_t.dists, o_b.dists) and torch.equal(o_t.counts, o_b.counts))
        small = L.FlatIndex(None, bits, local_rank)
        small.write_packed_device(first_words)
        small.finalize()
        sr = torch.zeros((B, K), dtype=torch.int64, device=dev)
        sd = torch.zeros((B, K), dtype=torch.float32, device=dev)
        sc = torch.zeros(B, dtype=torch.int32, device=dev)
        small.search_packed_device(queries, K, metric, sr, sd, sc)
        torch.cuda.synchronize()
        host_rows = first_words.cpu().numpy().view(np.uint64)
        host_q = queries.cpu().numpy().view(np.uint64)
        orc = O.get()
        exact = True
        for qi in (0, B // 2, B - 1):
            e_ids, e_d = orc.canonical_topk_packed(host_q[qi], host_rows, K, O.HAMMING)
            exact = exact and np.array_equal(sr[qi].cpu().numpy().astype(np.uint32)[:len(e_ids)], e_ids) and np.array_equal(sd[qi].cpu().numpy()[:len(e_ids)], e_d)
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1000.0
        qps = B * args.steps / elapsed
        launches = max(int(prof["scan_launches"]), 1)
        scan_s = prof["scan_us"] * 1e-6
        timed_steps = max(int(prof["searches"]), 1)
        mfma = B >= 72                                       # >= 72 queries: the +-1 GEMM on the FP4 MFMA streams one nibble per bit
        kernel_bytes = float(n_local) * (bits // 2 if mfma else bits // 8) * timed_steps
        hbm_gbps = kernel_bytes / scan_s / 1e9 if scan_s > 0 else 0.0
        ops = 2.0 * B * float(prof["scan_rows"]) * bits
        result = {
            "metric": "queries/sec, packed-binary Hamming %dx%d-bit, batch=%d, k=%d" % (N, bits, B, K),
            "value": round(qps, 1), "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u64",
            "data": "synthetic",
            "config": {"workload": "C5 packed-binary Hamming %dx%d-bit uniform random fingerprints, %d queries = rows with 16 bits flipped, k=%d" % (N, bits, B, K),
                       "rows_per_gpu": n_local, "sharding": "row %% %d" % world,
                       "exchange": ("rccl all_gather of %d B/rank inside the library" % (B * K * 12 + B * 4 + 16)) if native else ("torch.distributed" if world > 1 else "none"),
                       "batches_in_flight": in_flight, "build_s": round(build_s, 1), "derived_build_s": round(prepare_s, 2),
                       "hbm_bytes_per_gpu": int(sh.index.hbm_bytes())},
            # the binding resource from the committed PMC pass (profiles/rNN_binding.json): the FP4 matrix pipe for the batched form (62 % busy at
            # 1.75 GHz, HBM at 0.56), HBM for the popcount kernels — `bound` / `frac` follow it, both live rates stay on the line
            "roofline": {"bound": "mfma" if (mfma and (binding_of("c5_share_nq256") or {}).get("binding", "").startswith("matrix pipe")) else "hbm",
                         "kernel": (("k_scan_qs<4,2,4,3,...,F4>" if ((int(prof.get("last_plan", 0)) >> 16) & 0xff) == 0x81 else "k_scan_h16<2,4,4,2,IP,fp4>") +
                                    " (v_mfma_scale_f32_32x32x64_f8f6f4) over the +-1 FP4 copy") if mfma else "k_scan_binary_rows",
                         "binding": binding_of("c5_share_nq256" if mfma else "c5_share_nq1"),
                         **({"achieved": round(ops / scan_s / 1e12, 1), "peak": MFMA_FP4_PEAK_TOPS, "unit": "TOP/s", "frac": round(ops / scan_s / 1e12 / MFMA_FP4_PEAK_TOPS, 4)}
                            if (mfma and scan_s > 0 and (binding_of("c5_share_nq256") or {}).get("binding", "").startswith("matrix pipe"))
                            else {"achieved": round(hbm_gbps, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(hbm_gbps / HBM_PEAK_GBPS, 4)}),
                         "hbm": {"achieved": round(hbm_gbps, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(hbm_gbps / HBM_PEAK_GBPS, 4)},
                         "traffic": None,
                         "mfma_TOPs": round(ops / scan_s / 1e12, 1) if (mfma and scan_s > 0) else None,
                         "launches": launches, "avg_launch_us": round(prof["scan_us"] / launches, 2), "timed_steps": timed_steps,
                         "note": "rank-0 shard; bytes = rows x %d B (%s); HIP events around the scan launches of every %d-th step" % (
                             bits // 2 if mfma else bits // 8, "one FP4 nibble per bit" if mfma else "packed words", (args.profile_every if args.profile_every > 0 else 4))},
        }
        if args.full:
            result["blocking_ms_per_batch"] = round(lat_ms, 4)
            result["verify"] = {"tickets_equal_blocking_search": same, "oracle_bit_exact_on_200k_row_sample": bool(exact)}
        if dumped is not None:
            result["dumped_outputs"] = {"dir": str(args.dump_outputs), "files": dumped}
        if args.full and not args.no_cpu_baseline and world == 1:
            try:
                result["cpu_baseline"] = cpu_baseline(args, N, bits, K, metric)
            except Exception as e:  # noqa: BLE001
                result["cpu_baseline"] = {"error": repr(e)}
        result_out.write(json.dumps(result) + "\n")
        result_out.flush()
    if dist is not None:
        dist.barrier()
        if sh.comm is not None:
            try:
                sh.comm.close()
            except Exception:  # noqa: BLE001
                pass
            sh.comm = None
        dist.destroy_process_group()


def oracle_distance_bits(index, queries, out, B, K):
    """Every (row, distance) pair the timed batch returned against the ORACLE's bit pattern: the rows come back from the
    index (HBM copy), the oracle scores them with the reference's batch-8 IP kernel (simd.rs:1452-1525, the form every row of
    a >= 4096-row store is scored with) and the f32 bits must be equal; ids: the recall figures above (torch fp32 top-k).
    The full ranking against the oracle's exact_flat_search is tests/test_gpu_baseline_configs.py::test_c2_* (2.4M rows)."""
    import oracle as O

    orc = O.get()
    rows = out.rows[:B].cpu().numpy().astype(np.int64)
    dists = out.dists[:B].cpu().numpy()
    qh = queries[:B].cpu().numpy()
    uniq = np.unique(rows.ravel())
    uniq = uniq[uniq >= 0]
    order = np.argsort(uniq)
    fetched = {}
    # contiguous runs would be nice, the result rows are scattered: one read per distinct row (a few thousand)
    for r in uniq[order]:
        fetched[int(r)] = index.read_rows(int(r), 1)[0]
    bad = 0
    for qi in range(B):
        for j in range(K):
            e = orc.ip_batch8_row(qh[qi], fetched[int(rows[qi, j])])
            bad += int(np.float32(e).view(np.uint32) != dists[qi, j].view(np.uint32))
    return {"oracle_distance_bits_checked": int(B * K), "oracle_distance_bits_equal": bad == 0, "oracle_distance_bits_mismatches": bad}


def _time_calls(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def _time_raw(call, args, warm, reps):
    """Median wall time of the bare C-ABI entry point through ctypes with prebuilt arguments — what the Rust FFI caller of INTEGRATION.md
    pays.  The entry points are BLOCKING (results final in the caller's device arrays on return), so nothing else belongs in the
    bracket: the Python wrapper of lynsedb_amd/core.py adds a torch.cuda.current_stream().synchronize() in front of the call and a
    metric-name lookup, and bench.py's own torch.cuda.synchronize() behind it used to be timed too (7-8 us of the 40 us C1 figure up to
    round 5: scripts/r6_latency.py); that figure stays on the line as `ms_python_wrapper`."""
    for _ in range(warm):
        assert call(*args) == 0
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rc = call(*args)
        ts.append(time.perf_counter() - t0)
        assert rc == 0
    ts.sort()
    return ts[len(ts) // 2]


_BINDING = None


def binding_of(name):
    """What LIMITS the dominant kernel of a configuration, from the committed rocprofv3 --pmc passes (profiles/r0N_binding.json, written by
    scripts/binding_from_pmc.py from profiles/r0N_<config>_pmc.json): matrix-pipe busy share (SQ_VALU_MFMA_BUSY_CYCLES / SIMDs over
    GRBM_GUI_ACTIVE / XCDs), the effective clock under the socket power cap, VALU instructions per MFMA instruction.  bench.py cannot
    run the counter passes itself; the JSON names the box-independent facts, the live line adds the rates of THIS run."""
    global _BINDING
    if _BINDING is None:
        _BINDING = {}
        for f in ("r06_binding.json", "r05_binding.json"):
            fp = ROOT / "profiles" / f
            if fp.exists():
                _BINDING = json.loads(fp.read_text())
                _BINDING["_file"] = f
                break
    b = _BINDING.get(name)
    if not b:
        return None
    b = dict(b)
    b["source"] = "profiles/%s" % _BINDING.get("_file")
    return b


def _scan_profile(idx, fn, reps, bytes_per_row):
    """HIP-event time of the scan launches of `reps` calls -> (scan us per call, GB/s of `bytes_per_row` x rows scanned)."""
    idx.profile_enable(True)
    idx.profile_get(reset=True)
    for _ in range(reps):
        fn()
    p = idx.profile_get(reset=True)
    idx.profile_enable(False)
    us = p["scan_us"] / max(reps, 1)
    gbps = (p["scan_rows"] * bytes_per_row / (p["scan_us"] * 1e-6) / 1e9) if p["scan_us"] else 0.0
    return round(us, 1), round(gbps, 1), p


def same_shard_variants(idx, queries, B, K, N, D):
    """The headline shard and queries under the other float metrics and under a subset filter (outside the timed region): squared
    L2 and cosine (certified int8 pass over the augmented / unit-row codes), FLAT-IP restricted to a random 50 % subset
    given as BitSet words (masked int8 scan; host entry point: the 1.25 MB of words are uploaded on every call).
    Oracle parity of these paths: tests/test_gpu_baseline_configs.py, tests/test_gpu_i8c_hostile.py."""
    out = {}
    rows = torch.zeros((B, K), dtype=torch.int64, device=queries.device)
    dists = torch.zeros((B, K), dtype=torch.float32, device=queries.device)
    counts = torch.zeros(B, dtype=torch.int32, device=queries.device)
    idx.search_device(queries, K, "ip", rows, dists, counts)
    torch.cuda.synchronize()
    rows_ip = rows.clone()
    for name in ("l2", "cosine"):
        t0 = time.time()
        idx.prepare(name, B)
        torch.cuda.synchronize()
        build_s = time.time() - t0
        fn = lambda: idx.search_device(queries, K, name, rows, dists, counts)  # noqa: E731
        ms = _time_calls(fn, 3, 10) * 1e3
        us, _, p = _scan_profile(idx, fn, 4, 0)
        plan = int(p["last_plan"])
        out[name] = {"ms_per_step": round(ms, 4), "queries_per_s": round(B / ms * 1e3, 1), "scan_us_per_step": us, "derived_build_s": round(build_s, 3),
                     "int8_coarse_pass": bool(plan & 4), "fallback_queries": int(p["fallback_queries"]),
                     "rescored_per_query": round(p["pool_entries"] / max(p["searches"] * B, 1), 1), "binding": binding_of(name)}
    # small batches on the same shard (the 128-row x 32-query tiling; from 256K rows on it streams the SQ8 codes as well): HBM-bound
    for nq in (1, 32, 128):
        dq = queries[:nq].contiguous()
        r1 = torch.zeros((nq, K), dtype=torch.int64, device=queries.device)
        d1 = torch.zeros((nq, K), dtype=torch.float32, device=queries.device)
        c1 = torch.zeros(nq, dtype=torch.int32, device=queries.device)
        fn = lambda: idx.search_device(dq, K, "ip", r1, d1, c1)  # noqa: E731
        ms = _time_calls(fn, 3, 10) * 1e3
        us, _, p = _scan_profile(idx, fn, 4, 0)
        same = bool(torch.equal(r1, rows_ip[:nq])) if rows_ip is not None else None
        out["ip_nq%d" % nq] = {"ms_per_call": round(ms, 4), "queries_per_s": round(nq / ms * 1e3, 1), "scan_us_per_call": us,
                               "int8_stream_GBps": round(N * D / (us * 1e-6) / 1e9, 1) if us else None,
                               "frac_of_hbm_peak": round(N * D / (us * 1e-6) / 1e9 / HBM_PEAK_GBPS, 4) if us else None,
                               "int8_coarse_pass": bool(int(p["last_plan"]) & 4), "same_rows_as_the_256_query_batch": same}
    rng = np.random.default_rng(7)
    member = rng.random(N) < 0.5
    ids = np.nonzero(member)[0].astype(np.uint64)
    words = np.zeros((N + 63) // 64, np.uint64)
    np.bitwise_or.at(words, (ids // 64).astype(np.int64), np.uint64(1) << (ids % np.uint64(64)))
    qh = np.ascontiguousarray(queries.cpu().numpy())
    fn = lambda: idx.search_filtered_bitset_batch_arrays(qh, K, "ip", words)  # noqa: E731
    ms = _time_calls(fn, 2, 8) * 1e3
    us, _, p = _scan_profile(idx, fn, 4, 0)
    out["ip_subset_50pct_bitset"] = {"ms_per_call_host_api": round(ms, 4), "scan_us_per_call": us, "int8_coarse_pass": bool(int(p["last_plan"]) & 4),
                                     "fallback_queries": int(p["fallback_queries"]), "subset_rows": int(ids.size)}
    out["hbm_bytes_with_l2_and_cosine_codes"] = int(idx.hbm_bytes())
    return out


def second_distribution(args, dev):
    """FLAT-IP on N(0,1) rows scaled to unit norm (SURVEY 8(d) names it next to uniform[0,1) for config 2), mixed-sign queries =
    perturbed rows: same size, batch and k as the headline.  The certified int8 margin is data dependent — rescored rows per
    query and ms per step go on the record for a distribution that is not the friendliest one."""
    import lynsedb_amd as L

    N, D, B, K = args.rows, args.dim, args.batch, args.k
    idx = L.FlatIndex(None, D, dev.index)
    idx.reserve(N)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed + 101)
    qrows = np.sort(np.random.default_rng(args.seed + 102).integers(0, N, size=B))
    q_src = torch.empty((B, D), device=dev, dtype=torch.float32)
    for b0 in range(0, N, GEN_BLOCK):
        nb = min(GEN_BLOCK, N - b0)
        blk = torch.randn((nb, D), generator=g, device=dev, dtype=torch.float32)
        blk /= blk.norm(dim=1, keepdim=True)
        sel = np.nonzero((qrows >= b0) & (qrows < b0 + nb))[0]
        if sel.size:
            q_src[torch.as_tensor(sel, device=dev)] = blk[torch.as_tensor(qrows[sel] - b0, device=dev)]
        idx.write_device(blk)
        del blk
    idx.finalize()
    queries = (q_src + 0.02 * torch.randn((B, D), generator=g, device=dev, dtype=torch.float32) / (D ** 0.5) * 4.0).contiguous()
    rows = torch.zeros((B, K), dtype=torch.int64, device=dev)
    dists = torch.zeros((B, K), dtype=torch.float32, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    fn = lambda: idx.search_device(queries, K, "ip", rows, dists, counts)  # noqa: E731
    ms = _time_calls(fn, 3, 10) * 1e3
    us, _, p = _scan_profile(idx, fn, 8, 0)
    plan = int(p["last_plan"])
    top1 = float((rows[:, 0].cpu().numpy() == qrows).mean())
    return {"workload": "FLAT-IP %dx%d f32, N(0,1) rows scaled to unit norm, %d queries = perturbed rows, k=%d" % (N, D, B, K),
            "ms_per_step": round(ms, 4), "queries_per_s": round(B / ms * 1e3, 1), "scan_us_per_step": us,
            "rescored_per_query": round(p["pool_entries"] / max(p["searches"] * B, 1), 1), "fallback_queries": int(p["fallback_queries"]),
            "int8_coarse_pass": bool(plan & 4), "started_on_int8": bool(plan & 64), "i8c_strikes": idx.coarse_state()["i8c_strikes"],
            "top1_is_the_perturbed_row": top1}


def other_configs(dev):
    """BASELINE.json configs 1, 3, 4 (one GPU's share), 5 (one GPU's share): median wall time of the call through the
    device API, HIP-event time of its scan launches, the kernel's stream rate against 8 TB/s, oracle parity on a few queries."""
    import lynsedb_amd as L
    import oracle as O

    orc = O.get()
    out = {}

    only = os.environ.get("LYNSE_BENCH_ONLY_CONFIG")   # (development: one of c1 / c3 / c5_share / c4_share)

    def guarded(name, fn):
        if only and name != only:
            return
        try:
            out[name] = fn()
        except Exception as e:  # noqa: BLE001
            out[name] = {"error": repr(e)}
        torch.cuda.empty_cache()

    def c1():
        rng = np.random.default_rng(42)          # benchmarks/flat_search_bench.py:71-97
        data = rng.random((100_000, 128), dtype=np.float32)
        q = rng.random(128, dtype=np.float32)
        idx = L.FlatIndex(None, 128, dev.index)
        idx.write(data)
        idx.finalize()
        dq = torch.as_tensor(q.reshape(1, -1), device=dev)
        rows = torch.zeros((1, 10), dtype=torch.int64, device=dev)
        d = torch.zeros((1, 10), dtype=torch.float32, device=dev)
        c = torch.zeros(1, dtype=torch.int32, device=dev)
        fn = lambda: idx.search_device(dq, 10, "ip", rows, d, c)  # noqa: E731
        ms_wrapped = _time_calls(fn, 20, 30) * 1e3
        raw = (idx._h, C.c_void_p(dq.data_ptr()), 1, 10, 0, C.c_void_p(rows.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(c.data_ptr()), None)
        ms = _time_raw(L._lib.lib.lynse_hip_flat_search_f32_device, raw, 20, 200) * 1e3      # (flat_search_bench.py: 20 warm-ups; median)
        us, gbps, _ = _scan_profile(idx, fn, 10, 128 * 4 / 1)   # (scan_rows of the fused search = rows x queries)
        e_ids, e_d = orc.canonical_topk(q, data, 10, O.IP)
        ok = np.array_equal(rows.cpu().numpy()[0].astype(np.uint32), e_ids) and np.array_equal(d.cpu().numpy()[0].view(np.uint32), e_d.view(np.uint32))
        return {"workload": "C1 FLAT-IP 100000x128 f32, single query, k=10 (flat_search_bench.py)", "ms": round(ms, 4),
                "ms_is": "median wall time of the blocking C-ABI call (ctypes, prebuilt arguments)", "ms_python_wrapper": round(ms_wrapped, 4),
                "launches_per_call": 1, "scan_us": us,
                "GBps": gbps, "frac_of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4), "frac_of_hbm_peak_end_to_end": round(100_000 * 128 * 4 / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                "bytes": "f32 rows (the one-launch exact search)", "binding": binding_of("c1"),
                "oracle_parity": bool(ok)}

    def c3():
        from lynsedb_amd.datasets import sift_like

        data = sift_like(1_000_000, 128, 42)
        qs = sift_like(256, 128, 43)
        idx = L.FlatIndex(None, 128, dev.index)
        idx.write(data)
        idx.finalize()
        dq = torch.as_tensor(qs, device=dev)
        rows = torch.zeros((256, 100), dtype=torch.int64, device=dev)
        d = torch.zeros((256, 100), dtype=torch.float32, device=dev)
        c = torch.zeros(256, dtype=torch.int32, device=dev)
        fn = lambda: idx.search_device(dq, 100, "l2", rows, d, c)  # noqa: E731
        ms_wrapped = _time_calls(fn, 3, 10) * 1e3
        raw = (idx._h, C.c_void_p(dq.data_ptr()), 256, 100, 1, C.c_void_p(rows.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(c.data_ptr()), None)
        ms = _time_raw(L._lib.lib.lynse_hip_flat_search_f32_device, raw, 5, 60) * 1e3
        us, gbps, p = _scan_profile(idx, fn, 5, 128 * 2)
        r, dd = rows.cpu().numpy(), d.cpu().numpy()
        # the same batches as tickets, two in flight (submit / wait: the host's launch-to-completion gap of a blocking call is hidden)
        outs = [(torch.zeros((256, 100), dtype=torch.int64, device=dev), torch.zeros((256, 100), dtype=torch.float32, device=dev),
                 torch.zeros(256, dtype=torch.int32, device=dev)) for _ in range(2)]
        def flight(n):
            tk = [None, None]
            for i in range(n):
                if tk[i & 1] is not None:
                    tk[i & 1].wait()
                tk[i & 1] = idx.search_submit(dq, 100, "l2", *outs[i & 1])
            for t in tk:
                if t is not None:
                    t.wait()
        ms_fl, same = None, True
        if not os.environ.get("LYNSE_BENCH_NO_INFLIGHT"):   # (profiler runs: kernels of two batches overlap and inflate each other's durations)
            flight(6)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            flight(40)
            torch.cuda.synchronize()
            ms_fl = (time.perf_counter() - t0) / 40 * 1e3
            same = bool(torch.equal(outs[0][0], rows) and torch.equal(outs[0][1], d))
        ok = same
        for i in (0, 100, 255):
            e_ids, e_d = orc.canonical_topk(qs[i], data, 100, O.L2)
            ok = ok and np.array_equal(r[i].astype(np.uint32), e_ids) and np.array_equal(dd[i].view(np.uint32), e_d.view(np.uint32))
        stages = (int(p.get("last_plan", 0)) >> 8) & 0xff          # scan launches of a batch: the sample stage + the threshold stages
        launches = {"scan_stages": stages, "kernels_per_batch": 2 * stages + 1,
                    "what": "query preparation + every scan stage + a select behind every stage but the last + the fused select / rescoring / order tail"}
        return {"workload": "C3 FLAT-L2 SIFT-like 1000000x128, 256 queries, k=100", "ms": round(ms, 4), "queries_per_s": round(256 / ms * 1e3, 1),
                "ms_is": "median wall time of the blocking C-ABI call (ctypes, prebuilt arguments)", "ms_python_wrapper": round(ms_wrapped, 4),
                "ms_two_in_flight": None if ms_fl is None else round(ms_fl, 4), "launches": launches, "binding": binding_of("c3"),
                "scan_us": us, "GBps": gbps, "frac_of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4), "bytes": "f16 shadow rows (incl. the re-scanned sample rows)",
                "fallback_queries": int(p["fallback_queries"]), "stages": (int(p.get("last_plan", 0)) >> 8) & 0xff,
                "rescored_per_query": round(p["pool_entries"] / max(int(p["searches"]) * 256, 1), 1), "oracle_parity": bool(ok)}

    def c5():
        n, bits = 12_500_000, 1024
        g = torch.Generator(device=dev)
        g.manual_seed(42)
        idx = L.FlatIndex(None, bits, dev.index)
        idx.reserve(n)
        host = np.empty((n, bits // 64), np.uint64)
        for b0 in range(0, n, 2_500_000):
            w = torch.randint(-2**63, 2**63 - 1, (2_500_000, bits // 64), generator=g, device=dev, dtype=torch.int64)
            idx.write_packed_device(w)
            host[b0:b0 + 2_500_000] = w.cpu().numpy().view(np.uint64)
            del w
        res = {"workload": "C5 share: Hamming 12500000x1024-bit (one GPU of 8), k=50"}
        for nq in (1, 256):
            qw = host[np.arange(nq) * 1000 + 7].copy()
            qw[:, 0] ^= np.uint64(0xFFFF)
            dq = torch.as_tensor(qw.view(np.int64), device=dev)
            rows = torch.zeros((nq, 50), dtype=torch.int64, device=dev)
            d = torch.zeros((nq, 50), dtype=torch.float32, device=dev)
            c = torch.zeros(nq, dtype=torch.int32, device=dev)
            fn = lambda: idx.search_packed_device(dq, 50, "hamming", rows, d, c)  # noqa: E731
            ms_wrapped = _time_calls(fn, 2, 6) * 1e3
            raw = (idx._h, C.c_void_p(dq.data_ptr()), nq, 50, 3, C.c_void_p(rows.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(c.data_ptr()), None)
            ms = _time_raw(L._lib.lib.lynse_hip_flat_search_packed_u64_device, raw, 2, 12) * 1e3
            us, gbps, pp = _scan_profile(idx, fn, 3, bits // 8)
            qs_f4 = ((int(pp.get("last_plan", 0)) >> 16) & 0xff) == 0x81
            r, dd = rows.cpu().numpy(), d.cpu().numpy()
            ok = True
            for i in sorted({0, nq - 1}):
                e_ids, e_d = orc.canonical_topk_packed(qw[i], host, 50, O.HAMMING)
                ok = ok and np.array_equal(r[i].astype(np.uint32), e_ids) and np.array_equal(dd[i], e_d)
            # >= 72 queries: the +-1 GEMM on the FP4 MFMA streams one NIBBLE per bit (4x the packed words); below: the popcount kernels
            mfma = nq >= 72
            kb = gbps * (4.0 if mfma else 1.0)
            res["nq%d" % nq] = {"ms": round(ms, 4), "ms_python_wrapper": round(ms_wrapped, 4), "queries_per_s": round(nq / ms * 1e3, 1), "scan_us": us, "packed_GBps": gbps,
                                "binding": binding_of("c5_share_nq%d" % nq),
                                "kernel": (("k_scan_qs<4,2,4,3,...,F4>" if qs_f4 else "k_scan_h16<2,4,4,2,IP,fp4>") + " (v_mfma_scale_f32_32x32x64_f8f6f4) over the +-1 FP4 copy") if mfma else "k_scan_binary_rows",
                                "GBps": round(kb, 1), "frac_of_hbm_peak": round(kb / HBM_PEAK_GBPS, 4),
                                "mfma_TOPs": round(2.0 * nq * n * bits / (us * 1e-6) / 1e12, 1) if mfma and us else None, "oracle_parity": bool(ok)}
        return res

    def c4():
        n, dim, nlist, nprobe, k = 6_250_000, 768, 4096, 32, 10
        res = {"workload": "C4 share: IVF-Flat IP 6250000x768 (one GPU of 8), nlist=4096, nprobe=32, k=10; unit centres + sigma 0.03 noise, rows re-normalised "
                           "(benchmarks/ivf_kmeans_baseline.py:45-55); 20 Lloyd rounds (src/index/ivf.rs:163-170)"}

        def one(KC):
            g = torch.Generator(device=dev)
            g.manual_seed(7)
            centers = torch.randn((KC, dim), generator=g, device=dev)
            centers /= centers.norm(dim=1, keepdim=True) + 1e-12
            rows_d = torch.empty((n, dim), device=dev, dtype=torch.float32)
            for b0 in range(0, n, 250_000):
                e = min(n, b0 + 250_000)
                ids = torch.arange(b0, e, device=dev) % KC
                blk = centers[ids] + 0.03 * torch.randn((e - b0, dim), generator=g, device=dev)
                rows_d[b0:e] = blk / (blk.norm(dim=1, keepdim=True) + 1e-12)
                del blk
            t0 = time.time()
            ivf = L.IvfFlatIndex.build_device(rows_d, dim, nlist, int(os.environ.get("LYNSE_BENCH_C4_ITERS", "20")), "ip", l2_partitions=False)   # IVFIndex: k-means with the routing metric, 20 rounds (ivf.rs:163-170; the profiler runs of scripts/gpu_r6_profile.sh train 2)
            torch.cuda.synchronize()
            r = {"centres": KC, "build_s": round(time.time() - t0, 2)}
            qsel = torch.randint(0, n, (256,), generator=g, device=dev)
            queries = rows_d[qsel] + 0.01 * torch.randn((256, dim), generator=g, device=dev)
            queries = (queries / (queries.norm(dim=1, keepdim=True) + 1e-12)).contiguous()
            flat = L.FlatIndex(None, dim, dev.index)
            flat.reserve(n)
            for b0 in range(0, n, 1_250_000):
                flat.write_device(rows_d[b0:b0 + 1_250_000])
            flat.finalize()
            del rows_d
            for nq in (1, 256):
                dq = queries[:nq].contiguous()
                rows = torch.zeros((nq, k), dtype=torch.int64, device=dev)
                d = torch.zeros((nq, k), dtype=torch.float32, device=dev)
                c = torch.zeros(nq, dtype=torch.int32, device=dev)
                fn = lambda: ivf.search_device(dq, k, nprobe, rows, d, c)  # noqa: E731
                ms_wrapped = _time_calls(fn, 3, 10) * 1e3
                raw = (ivf._h, C.c_void_p(dq.data_ptr()), nq, k, nprobe, C.c_void_p(rows.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(c.data_ptr()))
                ms = _time_raw(L._lib.lib.lynse_hip_ivf_search_f32_device, raw, 5, 100 if nq == 1 else 20) * 1e3
                ivf.profile_enable(True)
                ivf.profile_get(reset=True)
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                pr = ivf.profile_get(reset=True)
                ivf.profile_enable(False)
                fr = torch.zeros((nq, k), dtype=torch.int64, device=dev)
                fd = torch.zeros((nq, k), dtype=torch.float32, device=dev)
                fc = torch.zeros(nq, dtype=torch.int32, device=dev)
                flat.search_device(dq, k, "ip", fr, fd, fc)
                torch.cuda.synchronize()
                a, b = rows.cpu().numpy(), fr.cpu().numpy()
                rec = float(np.mean([len(set(a[i].tolist()) & set(b[i].tolist())) / k for i in range(nq)]))
                searches = max(int(pr.get("searches", 0)), 1)
                fused = bool(int(pr.get("last_plan", 0)) & 32)      # the few-query path: two launches (centroid ranking, probed lists), every row scored exactly from the f32 slab
                elem = 4 if fused else (1 if (int(pr.get("last_plan", 0)) & 4) else 2)
                scan_s = float(pr.get("scan_us", 0.0)) * 1e-6
                gbps = float(pr.get("scan_rows", 0)) * dim * elem / scan_s / 1e9 if scan_s > 0 else 0.0
                rows_step = int(pr.get("scan_rows", 0)) // searches
                r["nq%d" % nq] = {"ms": round(ms, 4), "ms_python_wrapper": round(ms_wrapped, 4), "queries_per_s": round(nq / ms * 1e3, 1), "recall_at_10_vs_exact_flat": round(rec, 4),
                                  "rows_scanned_per_step": rows_step, "scan_us_per_step": round(float(pr.get("scan_us", 0.0)) / searches, 1),
                                  "scan_bytes_per_row": dim * elem, "scan_GBps": round(gbps, 1),
                                  "frac_of_hbm_peak": round(gbps / HBM_PEAK_GBPS, 4),
                                  "frac_of_hbm_peak_end_to_end": round(rows_step * dim * elem / (ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                                  "path": "fused few-query search: 2 launches (centroid ranking, probed lists), every row scored exactly from the f32 slab; scan_us = the list-scan launch" if fused else "staged: routing, grouped tiled scans, selects",
                                  "binding": binding_of("c4_share_nq%d" % nq)}
            del ivf, flat
            torch.cuda.empty_cache()
            return r

        first = one(4096)      # as many generating centres as lists: recall 1.0 by construction
        res.update({kk: vv for kk, vv in first.items() if kk != "centres"})
        if not os.environ.get("LYNSE_BENCH_C4_NO_SECOND"):   # (profiler runs: the search kernels of the first data set are what is profiled)
            res["second_dataset_1024_centres"] = one(1024)   # lists do not coincide with the clusters: recall is a measurement
        res["oracle_parity"] = "tests/test_gpu_baseline_configs.py::test_c4_* (520k rows: the 19 GB share is not copied to the host here)"
        return res

    guarded("c1", c1)
    guarded("c3", c3)
    guarded("c5_share", c5)
    guarded("c4_share", c4)
    return out


def cpu_baseline_ivf(args, N, D, K, nlist, nprobe, KC):
    """the oracle's restatement of IVFIndex::search (ivf.rs:181-348: centroid ranking, the probed lists scored one row
    after the other — the reference's candidate scoring is serial) timed on ONE host core over a reduced collection of the same recipe:
    1,000,000 rows, the same nlist / nprobe, centroids = the 4096 generating centres with every row filed under its own centre (any
    centroids + assignments are an IVFIndex; a CPU k-means of this size would take hours).  The time of a query = ranking the nlist
    centroids + scoring the probed rows; the second part is scaled by the rows ratio to the full collection."""
    import oracle as O

    orc = O.get()
    n_s = min(N, 1_000_000)
    rng = np.random.default_rng(7)
    centers = rng.standard_normal((KC, D)).astype(np.float32)
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    data = np.empty((n_s, D), np.float32)
    for b0 in range(0, n_s, 100_000):
        e = min(n_s, b0 + 100_000)
        data[b0:e] = centers[np.arange(b0, e) % KC] + 0.03 * rng.standard_normal((e - b0, D)).astype(np.float32)
    asg = (np.arange(n_s) % KC).astype(np.uint32)
    cen = centers if nlist == KC else centers[:nlist]
    if nlist != KC:
        asg = (asg % nlist).astype(np.uint32)
    off, rows = orc.lists_from_assignments(asg, cen.shape[0])
    warm, trials = 5, 30
    qs = (centers[rng.integers(0, KC, warm + trials)] + 0.03 * rng.standard_normal((warm + trials, D))).astype(np.float32)
    for i in range(warm):
        orc.ivf_search(qs[i], data, cen, off, rows, nprobe, K, O.IP)
    ts, tc = [], []
    for i in range(warm, warm + trials):
        t0 = time.perf_counter()
        orc.ivf_search(qs[i], data, cen, off, rows, nprobe, K, O.IP)
        ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        orc.all_distances(qs[i], cen, O.IP)          # the centroid-ranking share (the same single-row kernel over nlist rows)
        tc.append(time.perf_counter() - t0)
    ts.sort()
    tc.sort()
    med, med_c = ts[len(ts) // 2], tc[len(tc) // 2]
    full = med_c + max(med - med_c, 0.0) * (N / n_s)
    return {"value": round(1.0 / full, 2), "unit": "queries/s", "cores": 1, "kind": "port",
            "sample": "%d-row sample (of %d) of the same recipe, nlist=%d nprobe=%d, %d warm-ups + %d timed single queries, median %.3f ms per query on the "
                      "sample (%.3f ms of it the centroid ranking); the probed-list share scaled by the rows ratio" % (n_s, N, cen.shape[0], nprobe, warm, trials, med * 1e3, med_c * 1e3),
            "median_ms_per_query_on_sample": round(med * 1e3, 3)}


def cpu_baseline(args, N, D, K, metric):
    """The oracle's restatement of the reference's chunked rayon scan (flat_mmap.rs:4845-4982; chunks of
    max(n / threads, 512) rows, AVX2+FMA batch-8 kernel, per-chunk top-k, serial merge) timed on this host's cores over a
    bounded row sample: a PERSISTENT pinned worker pool (rayon's global pool is created once, not per query), the sample
    first-touched by the workers that scan it, 20 warm-ups / 30 timed queries like benchmarks/flat_search_bench.py:88-97,
    one full pass per query as the reference's batch_search loops queries (engine.rs:5484-5496).  Reported for all host
    threads and for 4 threads (the reference's own gates default RAYON_NUM_THREADS to 4, scripts/perf_gate_local.py:218)."""
    import shutil
    import subprocess

    import oracle as O

    orc = O.get()
    cores = os.cpu_count() or 1
    sample = min(N, args.cpu_sample_rows)
    warm, trials = args.cpu_warmup, args.cpu_queries
    rng = np.random.default_rng(args.seed)

    def timed(threads, warm, trials):
        orc.pool_start(threads)
        try:
            if metric >= 3:   # packed fingerprints generated as words (D bits per row), queries = rows with 16 bits flipped
                W = (D + 63) // 64
                words = rng.integers(0, np.iinfo(np.int64).max, size=(sample, W), dtype=np.int64).view(np.uint64)
                qw = words[rng.integers(0, sample, size=warm + trials)].copy()
                qw[:, 0] ^= np.uint64(0xFFFF)
                run = lambda i: orc.packed_binary_search(qw[i], words, K, metric, n_threads=threads, mt=True)  # noqa: E731
                nbytes = words.nbytes
            else:
                data = orc.fill_uniform_mt(sample, D, args.seed)
                qs = data[rng.integers(0, sample, size=warm + trials)] + 0.03 * rng.standard_normal((warm + trials, D)).astype(np.float32)
                run = lambda i: orc.flat_search(qs[i], data, K, metric, n_threads=threads, mt=True)  # noqa: E731
                nbytes = data.nbytes
            for i in range(warm):
                run(i)
            ts = []
            for i in range(warm, warm + trials):
                t0 = time.perf_counter()
                run(i)
                ts.append(time.perf_counter() - t0)
            ts.sort()
            med = ts[len(ts) // 2]
            return {"threads": threads, "median_ms_per_query_on_sample": round(med * 1e3, 3), "GBps": round(nbytes / med / 1e9, 1),
                    "queries_per_s_full_size": round(1.0 / (med * (N / sample)), 3)}
        finally:
            orc.pool_stop()

    # The thread count that serves this host best (a container's CPU quota can make "all threads" slower than a few).  Round 6 ("a
    # stated number should be the same number twice" — the 3 + 7 sweep and the 20 + 30 figure disagreed 1.8x inside one process): EVERY figure
    # below is the SAME protocol (20 warm-ups + 30 timed queries, median; each run regenerates the sample so that the pool of that thread count
    # first-touches the pages it scans: on a multi-socket host the rows sit on the NUMA node of the worker that reads them), the sweep
    # included, and the winner is run three times: `value` is the median of the three medians, best and spread are on the line.
    usable = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else cores
    sweep = [timed(t, warm, trials) for t in sorted({t for t in (4, 16, 32, 64, 128, usable) if t <= usable})]
    best_t = max(sweep, key=lambda r: r["GBps"])["threads"]
    runs = [next(r for r in sweep if r["threads"] == best_t)] + [timed(best_t, warm, trials) for _ in range(2)]
    runs.sort(key=lambda r: r["median_ms_per_query_on_sample"])
    full, fastest, slowest = runs[1], runs[0], runs[2]
    four = next((r for r in sweep if r["threads"] == min(4, usable)), None) or timed(min(4, usable), warm, trials)
    cores = best_t
    cargo = shutil.which("cargo")
    if cargo:
        try:
            cargo = subprocess.run([cargo, "--version"], capture_output=True, text=True, timeout=10).stdout.strip()
        except Exception:  # noqa: BLE001
            cargo = "present, --version failed"
    host = {"threads_usable": usable, "cpu_model": None, "numa_nodes": None}
    try:
        host["cpu_model"] = next(ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name"))
        nodes = sorted(pth.name for pth in Path("/sys/devices/system/node").glob("node[0-9]*"))
        host["numa_nodes"] = {nd: (Path("/sys/devices/system/node") / nd / "cpulist").read_text().strip() for nd in nodes}
    except Exception:  # noqa: BLE001
        pass
    return {"value": full["queries_per_s_full_size"], "unit": "queries/s", "cores": cores, "kind": "port",
            "sample": "%d-row sample (of %d) first-touched by the pool, %d warm-ups + %d timed queries, median, run 3 times at %d threads (the best of the "
                      "thread sweep, same protocol): value = the median run; time scaled by the rows ratio; %.1f ms/query on the sample = %.1f GB/s" % (
                          sample, N, warm, trials, cores, full["median_ms_per_query_on_sample"], full["GBps"]),
            "best_threads": full, "best_threads_fastest_run": fastest, "best_threads_slowest_run": slowest,
            "spread_of_the_three_runs": round(slowest["median_ms_per_query_on_sample"] / max(fastest["median_ms_per_query_on_sample"], 1e-9), 3),
            "threads_4": four, "host_threads": usable, "host": host,
            "thread_sweep_GBps": {str(r["threads"]): r["GBps"] for r in sweep},
            "reference_build": "cargo: %s (the Rust reference cannot be built on this box; the port restates its scan)" % (cargo or "not found")}


if __name__ == "__main__":
    main()
