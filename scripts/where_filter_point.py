"""The measured points of field filters (`where=`).

  python scripts/where_filter_point.py [--rows 10000000] [--dim 768] [--batch 256] [--k 10] [--reps 15] [--out profiles/where_filter_point.json]

Fills the shard of a FLAT-IP Collection on the device (torch, as bench.py does), gives it numeric field columns in bulk
(FieldTable.append_columns) and reports
  1. k_field_filter's duration between two HIP events (lynse_hip_fields_filter's out_kernel_us; median, fastest and slowest of --reps) for a
     one-leaf numeric range, a 4-leaf AND and a 1,000-key IN, next to the bytes the leaves read (9 per row and referenced column);
  2. the blocking time of Collection.batch_search(where=) at selectivities 0.1 %, 10 % and 50 %, next to batch_search(subset=) given the
     same rows as an id array — what a caller pays without the filter (np.unique on the host, the ids over PCIe, the mask built from them).
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def stats(ts):
    return {"median": round(float(np.median(ts)), 1), "min": round(float(np.min(ts)), 1), "max": round(float(np.max(ts)), 1)}


def timed_us(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return stats(ts)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "where_filter_point.json"))
    a = p.parse_args()
    import torch

    import lynsedb_amd as L

    rng = np.random.default_rng(25)
    gen = torch.Generator(device="cuda").manual_seed(25)
    coll = L.Collection("where_point", a.dim, device=0)
    step = 500_000
    for r0 in range(0, a.rows, step):
        m = min(a.rows, r0 + step) - r0
        coll._flat.write_device(torch.randn((m, a.dim), generator=gen, device="cuda", dtype=torch.float32))
        coll._id_arrays.append(np.arange(r0, r0 + m, dtype=np.int64))
        coll._fields.append_columns(m, {"sel": rng.integers(0, 1000, m), "year": rng.integers(1950, 2025, m), "score": rng.random(m),
                                        "key": rng.integers(0, 100_000, m)})
    coll._flat.finalize()
    q = torch.randn((a.batch, a.dim), generator=gen, device="cuda", dtype=torch.float32).cpu().numpy()
    n = a.rows
    out = {"rows": n, "dim": a.dim, "batch": a.batch, "k": a.k, "reps": a.reps, "filter_kernel_us": {}, "batch_search_us": {}}

    kernels = {"range_1_leaf": ("sel < 100", 1), "and_4_leaves": ("year >= 2000 AND year < 2010 AND score > 0.5 AND sel < 500", 3),
               "in_1000_keys": ("key IN (" + ", ".join(str(i * 7) for i in range(1000)) + ")", 1)}
    for name, (expr, columns) in kernels.items():
        rw = coll._resolve_where(expr)     # (uploads the columns)
        ts = []
        for _ in range(a.reps):
            coll._resolve_where(expr)
            ts.append(coll._field_filter.last_kernel_us)
        out["filter_kernel_us"][name] = dict(stats(ts), matches=rw.count, columns=columns, bytes=9 * n * columns,
                                             resolve_us=timed_us(lambda: coll._resolve_where(expr), a.reps))
    for name, lit in (("0.1%", 1), ("10%", 100), ("50%", 500)):
        expr = f"sel < {lit}"
        rows = coll._where_rows(coll._resolve_where(expr)).copy()
        w = coll.batch_search(q, a.k, where=expr)
        s = coll.batch_search(q, a.k, subset=rows)
        same = all(np.array_equal(x.ids(), y.ids()) and np.array_equal(x.distances().view(np.uint32), y.distances().view(np.uint32)) for x, y in zip(w, s))
        out["batch_search_us"][name] = {"matches": int(rows.size), "same_results": bool(same),
                                        "where": timed_us(lambda: coll.batch_search(q, a.k, where=expr), a.reps),
                                        "subset_ids": timed_us(lambda: coll.batch_search(q, a.k, subset=rows), a.reps)}
    out["unfiltered_us"] = timed_us(lambda: coll.batch_search(q, a.k), a.reps)
    line = json.dumps(out)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
