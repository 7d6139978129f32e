"""The measured points of named vector fields: the device mask remap against the host route.

  python scripts/vector_field_point.py [--rows 10000000] [--dim 128] [--batch 256] [--k 10] [--reps 20] [--out profiles/vector_field_point.json]

A collection of --rows records with one numeric field column (`sel`, uniform in 0 .. 999) and a named field of --rows x --dim f32 rows
written on the device, attached to the ids in a seeded permutation — so row_of is a permutation of the collection's rows.  At
selectivities 1 % and 50 % it reports the median (fastest, slowest) of --reps calls of
  (a) remap_kernel_us   k_bitset_remap between two HIP events, as lynse_hip_rowmap_remap reports it;
  (b) device_us         Collection.batch_search_vector_field(where=) end to end: k_field_filter, k_bitset_remap, the exact filtered scan
                        of the field's shard taking the words on the device;
  (c) host_us           the same search with the remap done on the host from existing entry points: k_field_filter, the source words read
                        back, a numpy gather through row_of, repacked, FlatIndex.search_filtered_bitset_batch_arrays with host words;
and whether (b) and (c) return the same ids and distance bits.  Prints one JSON line and writes it to --out.
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
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "vector_field_point.json"))
    a = p.parse_args()
    import torch

    import lynsedb_amd as L

    n = a.rows
    rng = np.random.default_rng(26)
    gen = torch.Generator(device="cuda").manual_seed(26)
    coll = L.Collection("vector_field_point", 8, device=0)
    step = 1_000_000
    for r0 in range(0, n, step):
        m = min(n, r0 + step) - r0
        coll._flat.write_device(torch.randn((m, 8), generator=gen, device="cuda", dtype=torch.float32))
        coll._id_arrays.append(np.arange(r0, r0 + m, dtype=np.int64))
        coll._fields.append_columns(m, {"sel": rng.integers(0, 1000, m)})
    coll._flat.finalize()
    coll.create_vector_field("emb", a.dim, "ip")
    f = coll._vfields["emb"]
    for r0 in range(0, n, step):
        m = min(n, r0 + step) - r0
        f.flat.write_device(torch.randn((m, a.dim), generator=gen, device="cuda", dtype=torch.float32))
    f.flat.finalize()
    f.id_chunks = [rng.permutation(n).astype(np.int64)]   # field row -> user id (= collection row here); no tombstones are used below
    q = torch.randn((a.batch, a.dim), generator=gen, device="cuda", dtype=torch.float32).cpu().numpy()
    row_of = f.id_map()

    def host_route(expr):
        rw = coll._resolve_where(expr)
        bits = np.unpackbits(coll._field_filter.words().view(np.uint8), bitorder="little")[:n]
        words = np.packbits(np.concatenate([bits[row_of], np.zeros(-n % 64, np.uint8)]), bitorder="little").view(np.uint64)
        rows, dists, counts = f.flat.search_filtered_bitset_batch_arrays(q, a.k, f.metric, words)
        return rw.count, rows, dists, counts

    out = {"rows": n, "dim": a.dim, "batch": a.batch, "k": a.k, "reps": a.reps, "row_of": "permutation", "source_words_bytes": (n + 63) // 64 * 8,
           "row_of_bytes": 4 * n, "points": {}}
    for name, lit in (("1%", 10), ("50%", 500)):
        expr = f"sel < {lit}"
        dev = coll.batch_search_vector_field("emb", q, a.k, where=expr)
        matches, rows, dists, counts = host_route(expr)
        ids = f.id_map()
        same = all(np.array_equal(dev[i].ids(), ids[rows[i, :int(counts[i])].astype(np.int64)])
                   and np.array_equal(dev[i].distances().view(np.uint32), dists[i, :int(counts[i])].view(np.uint32)) for i in range(a.batch))
        kernel = []
        for _ in range(a.reps):
            coll._field_mask(f, expr, None)
            kernel.append(f.rowmap.last_kernel_us)
        out["points"][name] = {"matches": int(matches), "same_results": bool(same), "remap_kernel_us": stats(kernel),
                               "filter_kernel_us": round(coll._field_filter.last_kernel_us, 1),
                               "device_us": timed_us(lambda: coll.batch_search_vector_field("emb", q, a.k, where=expr), a.reps),
                               "host_us": timed_us(lambda: host_route(expr), a.reps)}
    out["unfiltered_us"] = timed_us(lambda: coll.batch_search_vector_field("emb", q, a.k), a.reps)
    line = json.dumps(out)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
