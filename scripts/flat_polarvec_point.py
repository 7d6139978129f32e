"""Measured points of FLAT-*-POLARVEC<b> against FLAT-*-RABITQ and the exact FLAT scan on the same rows and handle.

  python scripts/flat_polarvec_point.py [--rows 1000000] [--dim 768] [--nq 256] [--k 10] [--warmup 3] [--reps 10] [--bits 4,8] [--metrics ip,l2]

One clustered collection on one handle.  Per metric: the exact FLAT search (blocking calls through the Python wrapper, host queries and
outputs; median and spread over --reps after --warmup), the RaBitQ two-pass at its oversample of 200 and, per bit count, the PolarVec
two-pass at its oversample of 20.  For the two-pass searches the scan stage (query transform + code scan + pool cut) and the exact rescore
come from HIP events on the search stream (lynse_hip_flat_*_stage_times, profiling on, one search per reading: median and spread), the
whole call from the host clock with profiling off.  recall@k is the overlap with the exact answer over all queries.  One JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def spread(ts):
    return {"median": round(float(np.median(ts)), 1), "min": round(float(np.min(ts)), 1), "max": round(float(np.max(ts)), 1)}


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return spread(ts)


def staged(idx, search, times, warmup, reps):
    """per-search scan and rescore microseconds of a two-pass search, from the handle's stage clock"""
    idx.profile_enable(True)
    for _ in range(warmup):
        search()
    scan, resc = [], []
    for _ in range(reps):
        times(reset=True)
        search()
        t = times(reset=True)
        scan.append(t["scan_us"])
        resc.append(t["rescore_us"])
    idx.profile_enable(False)
    return {"scan_us": spread(scan), "rescore_us": spread(resc)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--nq", type=int, default=256)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--bits", default="4,8")
    p.add_argument("--metrics", default="ip,l2")
    p.add_argument("--centres", type=int, default=1024)
    a = p.parse_args()
    import lynsedb_amd as L

    rng = np.random.default_rng(7)
    centres = rng.standard_normal((a.centres, a.dim), dtype=np.float32)
    data = np.empty((a.rows, a.dim), np.float32)
    step = 100_000
    for r0 in range(0, a.rows, step):
        r1 = min(a.rows, r0 + step)
        data[r0:r1] = centres[rng.integers(0, a.centres, r1 - r0)] + 0.4 * rng.standard_normal((r1 - r0, a.dim), dtype=np.float32)
    queries = (data[rng.integers(0, a.rows, a.nq)] + 0.05 * rng.standard_normal((a.nq, a.dim), dtype=np.float32)).astype(np.float32)
    idx = L.FlatIndex(None, a.dim, device=0)
    idx.write(data)
    idx.finalize()

    def recall(got, exact):
        return round(float(np.mean([len(set(got[i]) & set(exact[i])) / a.k for i in range(a.nq)])), 4)

    out = {"rows": a.rows, "dim": a.dim, "nq": a.nq, "k": a.k, "warmup": a.warmup, "reps": a.reps, "metrics": {}}
    t0 = time.perf_counter()
    idx.build_rabitq()
    out["rabitq_build_s"] = round(time.perf_counter() - t0, 3)
    for metric in a.metrics.split(","):
        m = {}
        exact = idx.search_batch_arrays(queries, a.k, metric)[0]
        m["flat_exact_us"] = timed(lambda: idx.search_batch_arrays(queries, a.k, metric), a.warmup, a.reps)
        rq = lambda: idx.search_rabitq_batch_arrays(queries, a.k, metric)
        m["rabitq"] = {"call_us": timed(rq, a.warmup, a.reps), **staged(idx, rq, idx.rabitq_stage_times, a.warmup, a.reps),
                       "recall": recall(rq()[0], exact), "bytes_per_row": idx.rabitq_params(arrays=False)["code_bytes"] + 4}
        for bits in (int(b) for b in a.bits.split(",")):
            t0 = time.perf_counter()
            idx.build_polarvec(bits, metric)
            build_s = time.perf_counter() - t0
            par = idx.polarvec_params(arrays=False)
            pv = lambda: idx.search_polarvec_batch_arrays(queries, a.k, metric)
            m[f"polarvec{bits}"] = {"build_s": round(build_s, 3), "bytes_per_row": par["bytes_per_vec"] + (4 if par["flags"] else 0),
                                    "call_us": timed(pv, a.warmup, a.reps), **staged(idx, pv, idx.polarvec_stage_times, a.warmup, a.reps),
                                    "recall": recall(pv()[0], exact)}
        out["metrics"][metric] = m
    print(json.dumps(out))


if __name__ == "__main__":
    main()
