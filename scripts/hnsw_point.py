"""Measured points of HNSW-L2 against the exact FLAT search of the same handle.

  python scripts/hnsw_point.py [--rows 1000000] [--dims 128,768] [--batches 1,16,256,4096] [--efs 50,200] [--k 10] [--reps 7]
                               [--clusters 1000] [--spread 0.15] [--m 16] [--ef-construction 128] [--profile-only]

Per width: Gaussian-cluster rows (centres standard normal, points centre + spread * normal), the build time of
FlatIndex.build_hnsw split into its stages (candidate lists = the exact searches of every row, selection = k_hnsw_select, reverse
edges = the host gather of U(i)), and per batch size and ef the median blocking time of
  hnsw   FlatIndex.search_hnsw_batch_arrays(queries, k, "l2", ef): k_hnsw_search, one wave per query
  flat   FlatIndex.search_batch_arrays(queries, k, "l2") on the same handle: the exact scan, the yardstick
with recall@k of the graph against the exact answer and the distances it scored per query.  Blocking times include the upload of the
queries and the copy back; kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/hnsw_point.py
--profile-only ...` run (one search per shape, no timing loop).  One JSON line per width.
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
    p.add_argument("--efs", default="50,200")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--clusters", type=int, default=1000)
    p.add_argument("--spread", type=float, default=0.15)
    p.add_argument("--m", type=int, default=16)
    p.add_argument("--ef-construction", type=int, default=128)
    p.add_argument("--profile-only", action="store_true")
    a = p.parse_args()
    import lynsedb_amd as L

    if L._lib.device_count() < 1:
        raise SystemExit("needs a HIP device")
    batches = [int(b) for b in a.batches.split(",")]
    efs = [int(e) for e in a.efs.split(",")]
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
        idx.build_hnsw("l2", a.m, a.ef_construction, efs[0])
        build_s = time.perf_counter() - t0
        st = idx.hnsw_stage_times(reset=True)
        prm = idx.hnsw_params(arrays=False)
        out = {"rows": a.rows, "dim": dim, "k": a.k, "m": a.m, "ef_construction": a.ef_construction, "levels": prm["top_level"] + 1,
               "build_s": round(build_s, 3), "build_stages_s": {"candidates": round(st["candidates_us"] * 1e-6, 3), "select": round(st["select_us"] * 1e-6, 3),
                                                                "reverse_edges": round(st["reverse_us"] * 1e-6, 3)}, "us": {}}
        for b in batches:
            q = queries[:b]
            exact = idx.search_batch_arrays(q, a.k, "l2")
            if not a.profile_only:
                out["us"][f"flat/{b}"] = timed(lambda: idx.search_batch_arrays(q, a.k, "l2"), a.reps)
            for ef in efs:
                idx.profile_enable(True)
                idx.hnsw_stage_times(reset=True)
                got = idx.search_hnsw_batch_arrays(q, a.k, "l2", ef)
                prof = idx.hnsw_stage_times(reset=True)
                idx.profile_enable(False)
                hit = sum(len(set(got[0][i, :int(got[2][i])].tolist()) & set(exact[0][i].tolist())) for i in range(b))
                rec = {"recall": round(hit / (a.k * b), 4), "scored_per_query": round(prof["scored"] / b, 1), "kernel_us_events": round(prof["search_us"], 1)}
                if not a.profile_only:
                    rec["hnsw"] = timed(lambda: idx.search_hnsw_batch_arrays(q, a.k, "l2", ef), a.reps)
                    rec["flat_over_hnsw"] = round(out["us"][f"flat/{b}"] / rec["hnsw"], 3)
                out["us"][f"hnsw/{b}/ef{ef}"] = rec
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
