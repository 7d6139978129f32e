"""One measured point of SPANN-L2 (replica_count 1) against IVF-Flat on the same box.

  python scripts/spann_point.py [--rows 1000000] [--dim 768] [--nlist 1024] [--k 10] [--reps 20] [--metric l2] [--centres 64] [--noise 1.0]

Builds SPANN and IVF-Flat (IVFIndex routing) over one clustered collection; both train the same k-means, so the centroids are the
same.  Reports the two build times, the mean lists per row, the median time of 1 and 256 queries at nprobe 8 and 32 (blocking
C-ABI calls through the Python wrapper, host queries and outputs), and recall@k of both against the exact FLAT top k at equal
nprobe.  Prints one JSON line.
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
    return float(np.median(ts) * 1e6)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--nlist", type=int, default=1024)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--centres", type=int, default=64)
    p.add_argument("--noise", type=float, default=1.0, help="sigma of the rows around their generating centre (unit-normal centres)")
    p.add_argument("--metric", default="l2")
    p.add_argument("--replicas", type=int, default=1)
    a = p.parse_args()
    import lynsedb_amd as L

    rng = np.random.default_rng(7)
    centres = rng.standard_normal((a.centres, a.dim), dtype=np.float32)
    data = np.empty((a.rows, a.dim), np.float32)
    step = 100_000
    for r0 in range(0, a.rows, step):
        r1 = min(a.rows, r0 + step)
        data[r0:r1] = centres[rng.integers(0, a.centres, r1 - r0)] + a.noise * rng.standard_normal((r1 - r0, a.dim), dtype=np.float32)
    queries = (data[rng.integers(0, a.rows, 256)] + 0.3 * rng.standard_normal((256, a.dim), dtype=np.float32)).astype(np.float32)

    t0 = time.perf_counter()
    ivf = L.IvfFlatIndex.build(None, data, a.dim, a.nlist, 20, a.metric, l2_partitions=False)
    ivf_build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    sp = L.SpannIndex.build(data, a.dim, a.nlist, 20, a.metric, replica_count=a.replicas)
    spann_build_s = time.perf_counter() - t0
    off, _ = sp.postings()
    flat = L.FlatIndex(None, a.dim)
    flat.write(data)
    flat.finalize()
    exact = flat.search_batch_arrays(queries, a.k, a.metric)[0]
    out = {"rows": a.rows, "centres": a.centres, "noise": a.noise, "dim": a.dim, "nlist": sp.n_partitions, "k": a.k, "metric": a.metric, "replica_count": a.replicas,
           "build_s": {"spann": round(spann_build_s, 2), "ivf_flat": round(ivf_build_s, 2)},
           "lists_per_row": round(float(off[-1]) / a.rows, 4), "us": {}, "recall": {}}
    for nprobe in (8, 32):
        for nq in (1, 256):
            q = queries[:nq]
            out["us"][f"nprobe{nprobe}_nq{nq}"] = {"spann": round(timed(lambda: sp.search_batch_arrays(q, a.k, nprobe), a.reps), 1),
                                                   "ivf_flat": round(timed(lambda: ivf.search_batch_arrays(q, a.k, nprobe), a.reps), 1)}
        g_sp = sp.search_batch_arrays(queries, a.k, nprobe)[0]
        g_ivf = ivf.search_batch_arrays(queries, a.k, nprobe)[0]
        rec = lambda g: float(np.mean([len(set(g[i].tolist()) & set(exact[i].tolist())) / a.k for i in range(queries.shape[0])]))
        out["recall"][f"nprobe{nprobe}"] = {"spann": round(rec(g_sp), 4), "ivf_flat": round(rec(g_ivf), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
