"""Measured points of DISKANN-L2 against the exact FLAT search and HNSW-L2 on the same handle.

  python scripts/diskann_point.py [--rows 1000000] [--dims 128,768] [--batches 1,16,256,4096] [--efs 64,200] [--hnsw-efs 50,200] [--k 10]
                                  [--reps 5] [--clusters 1000] [--spread 0.15] [--r 16] [--l 64] [--alpha 1.2] [--no-hnsw]

The shapes, data and protocol of scripts/hnsw_point.py.  Per width: the build time of FlatIndex.build_diskann (one un-profiled build:
every batch enqueued without a host round trip; then one build with profiling on, which waits after every stage, for the split into
search / prune / commit and the host random draws), and per batch size the median blocking time of
  diskann  FlatIndex.search_diskann_batch_arrays(queries, k, "l2", ef_query): k_vamana_search, one wave per query (ef = max(ef_query, l, 10 k))
  hnsw     FlatIndex.search_hnsw_batch_arrays(queries, k, "l2", ef) on the same handle
  flat     FlatIndex.search_batch_arrays(queries, k, "l2"): the exact scan, the yardstick
with recall@k against the exact answer, the distances scored per query and the kernel time from HIP events (one profiled call).
One JSON line per width.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts) * 1e6), 1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dims", default="128,768")
    p.add_argument("--batches", default="1,16,256,4096")
    p.add_argument("--efs", default="64,200")
    p.add_argument("--hnsw-efs", default="50,200")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--clusters", type=int, default=1000)
    p.add_argument("--spread", type=float, default=0.15)
    p.add_argument("--r", type=int, default=16)
    p.add_argument("--l", type=int, default=64)
    p.add_argument("--alpha", type=float, default=1.2)
    p.add_argument("--no-hnsw", action="store_true")
    p.add_argument("--no-staged-build", action="store_true")
    a = p.parse_args()
    import lynsedb_amd as L

    if L._lib.device_count() < 1:
        raise SystemExit("needs a HIP device")
    batches = [int(b) for b in a.batches.split(",")]
    for dim in (int(d) for d in a.dims.split(",")):
        rng = np.random.default_rng(7)
        cen = rng.standard_normal((a.clusters, dim)).astype(np.float32)
        idx = L.FlatIndex(None, dim, device=0)
        step = 100_000
        for r0 in range(0, a.rows, step):
            r = min(step, a.rows - r0)
            idx.write(cen[rng.integers(0, a.clusters, r)] + np.float32(a.spread) * rng.standard_normal((r, dim), dtype=np.float32))
        nq = max(batches)
        queries = (cen[rng.integers(0, a.clusters, nq)] + np.float32(a.spread) * rng.standard_normal((nq, dim), dtype=np.float32)).astype(np.float32)
        t0 = time.perf_counter()
        idx.build_diskann("l2", a.r, a.l, a.alpha)
        build_s = time.perf_counter() - t0
        st = idx.diskann_stage_times(reset=True)
        out = {"rows": a.rows, "dim": dim, "k": a.k, "r": a.r, "l": a.l, "alpha": a.alpha, "build_s": round(build_s, 3),
               "build_draws_s": round(st["build_draws_us"] * 1e-6, 3), "batches": 2 * ((a.rows + 255) // 256), "us": {}}
        out["build_us_per_batch"] = round(build_s * 1e6 / out["batches"], 1)
        if not a.no_staged_build:
            idx.profile_enable(True)
            t0 = time.perf_counter()
            idx.build_diskann("l2", a.r, a.l, a.alpha)
            out["staged_build_s"] = round(time.perf_counter() - t0, 3)
            idx.profile_enable(False)
            st = idx.diskann_stage_times(reset=True)
            out["staged_build_stages_s"] = {k: round(st[f"build_{k}_us"] * 1e-6, 3) for k in ("search", "prune", "commit", "draws")}
        adj = idx.diskann_params()["adj"]
        out["mean_degree"] = round(float((adj != 0xFFFFFFFF).sum(axis=1).mean()), 2)
        del adj
        if not a.no_hnsw:
            t0 = time.perf_counter()
            idx.build_hnsw("l2", 16, 128, 50)
            out["hnsw_build_s"] = round(time.perf_counter() - t0, 3)
        for b in batches:
            q = queries[:b]
            exact = idx.search_batch_arrays(q, a.k, "l2")
            out["us"][f"flat/{b}"] = timed(lambda: idx.search_batch_arrays(q, a.k, "l2"), a.reps)

            def point(name, search, times, ef):
                idx.profile_enable(True)
                times(reset=True)
                got = search(q, a.k, "l2", ef)
                prof = times(reset=True)
                idx.profile_enable(False)
                hit = sum(len(set(got[0][i, :int(got[2][i])].tolist()) & set(exact[0][i].tolist())) for i in range(b))
                rec = {"recall": round(hit / (a.k * b), 4), "scored_per_query": round(prof["scored"] / b, 1), "kernel_us_events": round(prof["search_us"], 1),
                       "us": timed(lambda: search(q, a.k, "l2", ef), a.reps)}
                rec["flat_over_this"] = round(out["us"][f"flat/{b}"] / rec["us"], 3)
                out["us"][f"{name}/{b}/ef{ef}"] = rec

            for ef in (int(e) for e in a.efs.split(",")):
                point("diskann", idx.search_diskann_batch_arrays, idx.diskann_stage_times, ef)
            if not a.no_hnsw:
                for ef in (int(e) for e in a.hnsw_efs.split(",")):
                    point("hnsw", idx.search_hnsw_batch_arrays, idx.hnsw_stage_times, ef)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
