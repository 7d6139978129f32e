"""Measured points of the approximate flat search against the exact single-query search of the same shard.

  python scripts/approx_point.py [--rows 1000000] [--dims 768,128] [--k 10] [--reps 7] [--eps 1e-6,1e-4,1e-2]

Per width, over uniform rows and one query: the median blocking time of FlatIndex.search_approx and of the exact search
(FlatIndex.search_batch_arrays with one query — code this feature does not touch), the two ALTERNATED call by call, per path:
  path 1   l2, cosine (every byte of the rows is read: no gain expected)
  path 3   ip with a non-negative query (sum order, descending), a non-positive one (ascending) and a mixed one (hybrid: blocks)
  path 4   l1, chebyshev, canberra, bray_curtis (blocks)
with what ran (pool, sampled dimensions, fall-back) and recall@k of the approximate ids against the exact top-k.  `coarse_bytes` is
rows x sampled dimensions x 4, the bytes k_approx_coarse has to read: over its time from a separate `rocprofv3 --kernel-trace --stats`
run it gives the achieved bandwidth.  The blocking times include the upload of the query, the cut, the rescoring of the pool, the
sort (on the host beyond 16,384 keys) and the copy back.  One JSON line per width.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def alternated(fa, fb, reps):
    fa()
    fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fa()
        t1 = time.perf_counter()
        fb()
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tb.append(t2 - t1)
    return round(float(np.median(ta) * 1e6), 1), round(float(np.median(tb) * 1e6), 1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dims", default="768,128")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--eps", default="1e-6,1e-4,1e-2")
    a = p.parse_args()
    import lynsedb_amd as L

    if L._lib.device_count() < 1:
        raise SystemExit("needs a HIP device")
    eps_list = [float(e) for e in a.eps.split(",")]
    for dim in (int(d) for d in a.dims.split(",")):
        rng = np.random.default_rng(27)
        idx = L.FlatIndex(None, dim, device=0)
        step = 100_000
        for r0 in range(0, a.rows, step):
            idx.write(rng.random((min(step, a.rows - r0), dim), dtype=np.float32))
        pos = rng.random(dim, dtype=np.float32)
        cases = [("l2", "l2", pos), ("cosine", "cosine", pos), ("ip/sum_desc", "ip", pos), ("ip/sum_asc", "ip", -pos),
                 ("ip/hybrid", "ip", (pos - np.float32(0.5)).astype(np.float32))]
        cases += [(m, m, pos) for m in ("l1", "chebyshev", "canberra", "bray_curtis")]
        out = {"rows": a.rows, "dim": dim, "k": a.k, "points": {}}
        for name, metric, q in cases:
            exact_rows = idx.search_batch_arrays(q[None], a.k, metric)[0][0]
            for eps in (eps_list if metric not in ("l2", "cosine") else eps_list[1:2]):
                rows, _, info = idx.search_approx(q, a.k, metric, eps)
                t_apx, t_exact = alternated(lambda: idx.search_approx(q, a.k, metric, eps),
                                            lambda: idx.search_batch_arrays(q[None], a.k, metric), a.reps)
                sampled = info["sample_dims"] if info["sample_dims"] and not info["fell_back"] else (dim if info["path"] in (1, 2) else 0)
                out["points"][f"{name}/{eps:g}"] = {
                    "approx_us": t_apx, "exact_us": t_exact, "exact_over_approx": round(t_exact / t_apx, 3), "path": info["path"],
                    "ip_case": info["ip_case"], "pool": info["pool"], "sample_dims": info["sample_dims"], "fell_back": info["fell_back"],
                    "coarse_bytes": a.rows * sampled * 4, "recall": round(float(np.isin(rows, exact_rows).sum()) / max(1, exact_rows.size), 3)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
