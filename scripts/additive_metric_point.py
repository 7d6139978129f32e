"""Measured points of the top-k search under the additive metrics against the plain scan of the same handle.

  python scripts/additive_metric_point.py [--rows 1000000] [--dims 128,768] [--batches 1,256] [--k 10] [--reps 7]

Per width, batch size and metric (l1, chebyshev, canberra, bray_curtis), the median blocking time of
  topk   FlatIndex.batch_search(queries, k, metric): k_additive_scan (lane-major LDS tiles, 8 queries' accumulators per lane) + the cut;
  plain  FlatIndex.search_range_batch_arrays(queries, +inf, k, metric) on the same handle: k_range_scan with additive_score — two
         ds_read_b32 per element and query — + the same cut (every row passes, so the selection does the same work).
Both return the same rows (checked).  `model` is the scan's element steps (rows x dim x queries) for the fraction of the VALU bound
(32 steps / clk / CU at 2 ops per step) once a kernel time from `rocprofv3 --kernel-trace --stats` is at hand; the blocking times
here include the upload of the queries, the radix selection over the score matrix, the sort and the copy back.  One JSON line per width.
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
    p.add_argument("--batches", default="1,256")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=7)
    a = p.parse_args()
    import lynsedb_amd as L

    if L._lib.device_count() < 1:
        raise SystemExit("needs a HIP device")
    batches = [int(b) for b in a.batches.split(",")]
    for dim in (int(d) for d in a.dims.split(",")):
        rng = np.random.default_rng(7)
        idx = L.FlatIndex(None, dim, device=0)
        step = 100_000
        for r0 in range(0, a.rows, step):
            idx.write(rng.random((min(step, a.rows - r0), dim), dtype=np.float32) + 0.01)
        queries = rng.random((max(batches), dim), dtype=np.float32) + 0.01
        out = {"rows": a.rows, "dim": dim, "k": a.k, "us": {}}
        for metric in ("l1", "chebyshev", "canberra", "bray_curtis"):
            for nq in batches:
                q = queries[:nq]
                inf = np.full(nq, np.inf, np.float32)
                top = idx.search_batch_arrays(q, a.k, metric)
                rng_ = idx.search_range_batch_arrays(q, inf, a.k, metric)
                assert np.array_equal(top[0], rng_[0]) and np.array_equal(top[1].view(np.uint32), rng_[1].view(np.uint32)), (metric, nq)
                t_top = timed(lambda: idx.batch_search(q, a.k, metric), a.reps)
                t_plain = timed(lambda: idx.search_range_batch_arrays(q, inf, a.k, metric), a.reps)
                out["us"][f"{metric}/{nq}"] = {"topk": t_top, "plain": t_plain, "plain_over_topk": round(t_plain / t_top, 3),
                                               "model_steps": a.rows * dim * nq}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
