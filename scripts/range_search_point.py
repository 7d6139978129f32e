"""One measured point of range search against the top-k search of the same collection.

  python scripts/range_search_point.py [--rows 1000000] [--dim 768] [--max-results 1000] [--reps 20] [--batches 1,32]

Fills a FLAT-IP Collection with clustered rows, takes each query's threshold at its 1000th-best (max-results-th) distance — from a
range search with the threshold at -inf and the same cap, whose distances the parity tests pin to the oracle's — and times, per
batch size (--reps blocking calls through the Python wrappers, host queries and outputs; median, fastest and slowest call):
  range   Collection.search_range for one query, FlatIndex.search_range_batch_arrays for a batch (the Collection has no batch form);
  topk    Collection.search / batch_search with k = max-results on the same collection, in the same process.
scan_bytes is what the scan launch reads once per query tile (rows x dim x 4); divide by the kernel's duration from
`rocprofv3 --kernel-trace --stats -- python scripts/range_search_point.py --batches N` for the fraction of peak.  Prints one JSON line.
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
    return {"median": round(float(np.median(ts) * 1e6), 1), "min": round(float(np.min(ts) * 1e6), 1), "max": round(float(np.max(ts) * 1e6), 1)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--max-results", type=int, default=1000)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--batches", default="1,32")
    p.add_argument("--centres", type=int, default=1024)
    a = p.parse_args()
    import lynsedb_amd as L

    rng = np.random.default_rng(7)
    centres = rng.standard_normal((a.centres, a.dim), dtype=np.float32)
    coll = L.Collection("range_point", a.dim, device=0)
    step = 100_000
    sample = None
    for r0 in range(0, a.rows, step):
        r1 = min(a.rows, r0 + step)
        block = centres[rng.integers(0, a.centres, r1 - r0)] + 0.4 * rng.standard_normal((r1 - r0, a.dim), dtype=np.float32)
        coll.add_items(block, list(range(r0, r1)))
        if sample is None:
            sample = block[:64].copy()
    coll.commit()
    batches = [int(b) for b in a.batches.split(",")]
    nq_max = max(batches)
    queries = (sample[rng.integers(0, sample.shape[0], nq_max)] + 0.05 * rng.standard_normal((nq_max, a.dim), dtype=np.float32)).astype(np.float32)
    cap = a.max_results
    flat = coll._flat
    _, d, c, _ = flat.search_range_batch_arrays(queries, np.full(nq_max, -np.inf, np.float32), cap, "ip")
    thr = np.array([d[i, int(c[i]) - 1] for i in range(nq_max)], np.float32)
    out = {"rows": a.rows, "dim": a.dim, "max_results": cap, "metric": "ip", "scan_bytes": a.rows * a.dim * 4, "us": {}}
    for nq in batches:
        q = queries[:nq]
        if nq == 1:
            t = {"range": timed(lambda: coll.search_range(q[0], float(thr[0]), cap), a.reps),
                 "topk": timed(lambda: coll.search(q[0], cap), a.reps)}
        else:
            t = {"range": timed(lambda: flat.search_range_batch_arrays(q, thr[:nq], cap, "ip"), a.reps),
                 "topk": timed(lambda: coll.batch_search(q, cap), a.reps)}
        passed = flat.search_range_batch_arrays(q, thr[:nq], cap, "ip")[3]
        t["passed_min_max"] = [int(passed.min()), int(passed.max())]
        t["range_over_topk"] = round(t["range"]["median"] / t["topk"]["median"], 3)
        out["us"][str(nq)] = t
    print(json.dumps(out))


if __name__ == "__main__":
    main()
