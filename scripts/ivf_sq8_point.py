"""One measured point of IVF-IP-SQ8 against IVF-Flat on the same box.

  python scripts/ivf_sq8_point.py [--rows 1000000] [--dim 768] [--nlist 1024] [--nprobe 32] [--k 10] [--reps 20]

Builds an SQ8 index over a clustered collection (device k-means on the decoded rows), then times, per batch of 1 and 256
queries (median of --reps blocking C-ABI calls through the Python wrapper, host queries and outputs):
  sq8          the whole SQ8 search (query codec + pool stage + rerank), profiling off;
  pool_stage   the SQ8 pool stage, HIP events on the search stream (lynse_hip_ivf_sq8_stage_times, profiling on; mean per search);
  rerank       k_pool_rerank, the same way;
  ivf_flat_k100  IVF-Flat over the DECODED rows with the same lists at k = pool = 10 k (the pool stage as a search of its own);
  ivf_flat     IVF-Flat over the ORIGINAL rows with the same centroids / lists at k.
Prints one JSON line.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def sq_codec(x, mn, sc):
    with np.errstate(all="ignore"):
        t = ((x - mn).astype(np.float32) / sc).astype(np.float32)
        t = np.where(np.isnan(t), np.float32(0), t)
        code = np.trunc(np.clip(t, 0, 255)).astype(np.uint8)
        return ((code.astype(np.float32) * sc).astype(np.float32) + mn).astype(np.float32)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e6)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--nlist", type=int, default=1024)
    p.add_argument("--nprobe", type=int, default=32)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=20)
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

    t0 = time.perf_counter()
    sq8 = L.IvfFlatIndex.build(None, data, a.dim, a.nlist, 20, "ip", quantizer="sq8")
    build_s = time.perf_counter() - t0
    mn, sc = sq8.sq8_params()
    cen, asg, _, _ = sq8.export()
    dec = np.empty_like(data)
    for r0 in range(0, a.rows, step):
        dec[r0:r0 + step] = sq_codec(data[r0:r0 + step], mn, sc)
    pool_ix = L.IvfFlatIndex.load(dec, cen, asg, "ip")
    del dec
    flat_ix = L.IvfFlatIndex.load(data, cen, asg, "ip")
    pool = 10 * a.k
    out = {"rows": a.rows, "dim": a.dim, "nlist": int(cen.shape[0]), "nprobe": a.nprobe, "k": a.k, "pool": pool,
           "build_sq8_s": round(build_s, 2), "us": {}}
    for nq in (1, 256):
        q = queries[:nq]
        r = {"sq8": timed(lambda: sq8.search_batch_arrays(q, a.k, a.nprobe), a.reps),
             "ivf_flat_k100": timed(lambda: pool_ix.search_batch_arrays(q, pool, a.nprobe), a.reps),
             "ivf_flat": timed(lambda: flat_ix.search_batch_arrays(q, a.k, a.nprobe), a.reps)}
        sq8.profile_enable(True)
        sq8.sq8_stage_times(reset=True)
        for _ in range(a.reps):
            sq8.search_batch_arrays(q, a.k, a.nprobe)
        st = sq8.sq8_stage_times(reset=True)
        sq8.profile_enable(False)
        r["pool_stage"] = st["pool_us"] / max(st["searches"], 1)
        r["rerank"] = st["rerank_us"] / max(st["searches"], 1)
        out["us"][str(nq)] = {kk: round(v, 1) for kk, v in r.items()}
    # recall@k of SQ8 and IVF-Flat against the exact top k of the probed lists is the same definition for both: report overlap
    g_sq8 = sq8.search_batch_arrays(queries, a.k, a.nprobe)[0]
    g_flat = flat_ix.search_batch_arrays(queries, a.k, a.nprobe)[0]
    out["overlap_sq8_vs_ivf_flat"] = float(np.mean([len(set(g_sq8[i]) & set(g_flat[i])) / a.k for i in range(256)]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
