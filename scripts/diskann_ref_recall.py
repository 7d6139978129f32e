"""recall@10 of the CPU restatements of DiskANN (tests/diskann_ref) and HNSW (tests/hnsw_ref) on the two data sets of DESIGN.md §19 / §21,
default parameters, 100 queries, L2.  No GPU: the GPU builds equal the restatements list for list.

  python scripts/diskann_ref_recall.py [--skip-hnsw]

  a  4096 x 32, 32 Gaussian clusters of spread 0.15 (hnsw_common.clustered(1, ...))
  b  the first 20,000 rows of the 1000-cluster set of scripts/hnsw_point.py at 128 columns (rng 7, spread 0.15), queries around
     the same centres from rng 8
One JSON line per data set.
"""
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def main():
    import diskann_common as D
    import hnsw_common as H
    import oracle as O

    orc = O.get()
    tmp = tempfile.mkdtemp()
    dref, href = D.build_ref(tmp, orc), H.build_ref(tmp, orc)
    rng = np.random.default_rng(7)
    cen = rng.standard_normal((1000, 128)).astype(np.float32)
    rows = (cen[rng.integers(0, 1000, 100_000)] + np.float32(0.15) * rng.standard_normal((100_000, 128), dtype=np.float32))[:20_000]
    rq = np.random.default_rng(8)
    queries = (cen[rq.integers(0, 1000, 100)] + np.float32(0.15) * rq.standard_normal((100, 128), dtype=np.float32)).astype(np.float32)
    sets = {"a: 4096 x 32, 32 clusters": H.clustered(1, 4096, 32, 32, 0.15, 100), "b: 20000 x 128, 1000 clusters": (np.ascontiguousarray(rows), queries)}
    for name, (data, q) in sets.items():
        n = data.shape[0]
        exact = [np.lexsort((np.arange(n), ((data - x) ** 2).sum(axis=1)))[:10] for x in q]
        recall = lambda res: round(sum(len(set(r[0].tolist()) & set(e.tolist())) for r, e in zip(res, exact)) / 1000, 4)
        out = {"data": name}
        t0 = time.perf_counter()
        g = D.ref_build(dref, data, D.L2, 16, 64, 1.2)
        out["diskann_build_s"] = round(time.perf_counter() - t0, 1)
        for efq in (0, 200):
            sc = []
            res = D.ref_search(dref, data, D.L2, g, q, 10, D.query_ef(g, n, 10, efq), scored=sc)
            out[f"diskann_ef{D.query_ef(g, n, 10, efq)}"] = {"recall": recall(res), "scored": round(sum(sc) / 100, 1)}
        if "--skip-hnsw" not in sys.argv:
            t0 = time.perf_counter()
            hg = H.ref_build(href, data, 1, 16, 128, H.ref_levels(href, 42, 16, None, n))
            out["hnsw_build_s"] = round(time.perf_counter() - t0, 1)
            for ef in (50, 200):
                sc = []
                res = H.ref_search(href, data, 1, hg, q, 10, ef, scored=sc)
                out[f"hnsw_ef{ef}"] = {"recall": recall(res), "scored": round(sum(sc) / 100, 1)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
