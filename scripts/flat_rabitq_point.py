"""One measured point of FLAT-IP-RABITQ against exact FLAT-IP on the same rows.

  python scripts/flat_rabitq_point.py [--rows 1000000] [--dim 768] [--k 10] [--reps 20] [--metric ip] [--oversample 200]

Builds the RaBitQ index over a clustered collection (one encode pass on the device; wall time and the device memory the build took on
top of the rows, from hipMemGetInfo through torch), then times, per batch of 1 and 256 queries (--reps blocking calls through the
Python wrapper, host queries and outputs; median, and the fastest and slowest call as the spread):
  rabitq      the whole RaBitQ search (query transform + code scan + pool cut + exact rescore), profiling off;
  scan_stage  query transform + code scan + pool cut, HIP events (lynse_hip_flat_rabitq_stage_times, profiling on; mean per search);
  rescore     k_pool_rerank over the pool, the same way;
  flat        the exact FLAT search of the same handle, in the same process.
recall@k is the overlap of the RaBitQ answer with the exact FLAT answer over 256 queries.  Prints one JSON line.
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


def used_bytes():
    try:
        import torch

        free, total = torch.cuda.mem_get_info(0)
        return int(total - free)
    except Exception:
        return -1


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--metric", default="ip")
    p.add_argument("--oversample", type=int, default=200)
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
    queries = (data[rng.integers(0, a.rows, 256)] + 0.05 * rng.standard_normal((256, a.dim), dtype=np.float32)).astype(np.float32)
    idx = L.FlatIndex(None, a.dim, device=0)
    idx.write(data)
    idx.finalize()
    exact = idx.search_batch_arrays(queries, a.k, a.metric)[0]
    before = used_bytes()
    t0 = time.perf_counter()
    idx.build_rabitq()
    build_s = time.perf_counter() - t0
    par = idx.rabitq_params(arrays=False)
    out = {"rows": a.rows, "dim": a.dim, "k": a.k, "metric": a.metric, "oversample": a.oversample, "padded_dim": par["padded_dim"],
           "code_bytes_per_row": par["code_bytes"], "scan_bytes_per_row": par["code_bytes"] + 4,   # the code and the f32 norm
           "flat_int8_bytes_per_row": a.dim, "build_s": round(build_s, 3),
           "index_bytes_after_build": used_bytes() - before if before >= 0 else None, "us": {}}
    for nq in (1, 256):
        q = queries[:nq]
        t = {"flat": timed(lambda: idx.search_batch_arrays(q, a.k, a.metric), a.reps),
             "rabitq": timed(lambda: idx.search_rabitq_batch_arrays(q, a.k, a.metric, a.oversample), a.reps)}
        idx.profile_enable(True)
        idx.rabitq_stage_times(reset=True)
        for _ in range(a.reps):
            idx.search_rabitq_batch_arrays(q, a.k, a.metric, a.oversample)
        st = idx.rabitq_stage_times(reset=True)
        idx.profile_enable(False)
        t["scan_stage"] = round(st["scan_us"] / max(st["searches"], 1), 1)
        t["rescore"] = round(st["rescore_us"] / max(st["searches"], 1), 1)
        t["row_queries_per_s"] = a.rows * nq / (t["scan_stage"] * 1e-6) if t["scan_stage"] > 0 else None
        t["rabitq_over_flat"] = round(t["rabitq"]["median"] / t["flat"]["median"], 3)
        out["us"][str(nq)] = t
    got = idx.search_rabitq_batch_arrays(queries, a.k, a.metric, a.oversample)[0]
    out["recall_at_k"] = float(np.mean([len(set(got[i]) & set(exact[i])) / a.k for i in range(queries.shape[0])]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
