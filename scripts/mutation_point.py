"""Measured points of the row mutations of a FLAT handle: compaction, update, and the first search after either.

  python scripts/mutation_point.py [--rows 1000000] [--dims 128,768] [--reps 5] [--out profiles/mutation_point.json]

f32 shards of rows x dim.  All times are host clocks around blocking calls (each ends in a stream synchronise), medians of --reps.
Per width:
  compact   FlatIndex.compact(keep) for random deletions of 1 %, 10 % and 50 % and for "row 0 only" (every row moves by one: every
            window staged).  The shard is put back before every repetition (a new handle filled from a device tensor, not timed).
            Beside each: the bytes the call moves (live rows after the first cleared bit, twice for a staged window), yardstick (a)
            = one device-to-device copy of the shard's bytes (a torch tensor copy_ of the same size: a hipMemcpyAsync) and yardstick
            (b) = the route without the call: read_rows to the host, numpy selection, a new handle, write, finalize.
  update    FlatIndex.update_rows of 10,000 random rows beside FlatIndex.write of 10,000 rows (both host data through the staging buffer).
  first     the first 16-query ip search after an update / a compaction (it pays for the recomputed norms and copies) beside the second.
One JSON object, written to --out and printed.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def med(ts):
    return round(float(np.median(ts)), 3)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dims", default="128,768")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--host-reps", type=int, default=1)
    p.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "mutation_point.json"))
    a = p.parse_args()
    import torch

    import lynsedb_amd as L

    if L._lib.device_count() < 1:
        raise SystemExit("needs a HIP device")
    dev = torch.device("cuda", 0)
    n = a.rows
    result = {"rows": n, "reps": a.reps, "widths": []}
    for dim in (int(d) for d in a.dims.split(",")):
        rng = np.random.default_rng(7)
        data = rng.standard_normal((n, dim), dtype=np.float32)
        d_data = torch.as_tensor(data, device=dev)
        d_copy = torch.empty_like(d_data)
        row_bytes = -(-dim // 4) * 16
        queries = rng.standard_normal((16, dim), dtype=np.float32)

        def filled():
            h = L.FlatIndex(None, dim)
            h.reserve(n + 10_000)
            h.write_device(d_data)
            h.finalize()
            return h

        ts = []
        for _ in range(a.reps + 1):   # yardstick (a); the first repetition is the warm-up
            torch.cuda.synchronize()
            ts.append(clock(lambda: (d_copy.copy_(d_data), torch.cuda.synchronize()))[0])
        copy_ms = med(ts[1:])
        w = {"dim": dim, "shard_bytes": n * row_bytes, "device_copy_ms": copy_ms,
             "device_copy_gbps": round(n * row_bytes / copy_ms / 1e6, 1), "compact": []}
        keeps = [(f"random {int(s * 100)} %", rng.random(n) >= s) for s in (0.01, 0.1, 0.5)] + [("row 0 only", np.arange(n) != 0)]
        for name, keep in keeps:
            plan = L.FlatIndex.compact_plan(keep, n, 0, row_bytes)
            win = plan["windows"].astype(np.int64)
            moved = int(win[win[:, 3] == 1, 2].sum() + 2 * win[win[:, 3] == 2, 2].sum()) * row_bytes   # read + written once per copy
            ts = []
            for rep in range(a.reps + 1):
                h = filled()
                ts.append(clock(lambda: h.compact(keep))[0])
                if rep == 0:
                    first_ms = clock(lambda: h.search_batch_arrays(queries, 10, "ip"))[0]
                    second_ms = clock(lambda: h.search_batch_arrays(queries, 10, "ip"))[0]
                    sel = np.nonzero(keep)[0][[0, plan["live"] // 2, plan["live"] - 1]]
                    assert np.array_equal(h.gather_rows([0, plan["live"] // 2, plan["live"] - 1]), data[sel])
                del h
            ms = med(ts[1:])
            host = []
            for _ in range(a.host_reps):   # yardstick (b)
                h = filled()

                def route():
                    rows = h.read_rows(0, n)
                    g = L.FlatIndex(None, dim)
                    g.write(rows[keep])
                    g.finalize()
                    return g

                host.append(clock(route)[0])
                del h
            w["compact"].append({"case": name, "live": plan["live"], "window_rows": plan["window_rows"],
                                 "windows_direct": int((win[:, 3] == 1).sum()), "windows_staged": int((win[:, 3] == 2).sum()),
                                 "moved_bytes": moved, "compact_ms": ms, "compact_gbps_moved": round(moved / ms / 1e6, 1),
                                 "copy_scaled_ms": round(copy_ms * moved / (n * row_bytes), 3), "host_route_ms": med(host),
                                 "first_search_ms": round(first_ms, 3), "second_search_ms": round(second_ms, 3)})
        rows = rng.choice(n, 10_000, replace=False).astype(np.uint64)
        new = rng.standard_normal((10_000, dim), dtype=np.float32)
        h = filled()
        h.search_batch_arrays(queries, 10, "ip")
        up, ap = [], []
        for _ in range(a.reps + 1):
            up.append(clock(lambda: h.update_rows(rows, new))[0])
        first_ms = clock(lambda: h.search_batch_arrays(queries, 10, "ip"))[0]
        second_ms = clock(lambda: h.search_batch_arrays(queries, 10, "ip"))[0]
        assert np.array_equal(h.gather_rows(rows[:100]), new[:100])
        for _ in range(a.reps + 1):
            g = filled()
            ap.append(clock(lambda: g.write(new))[0])
            del g
        w["update"] = {"rows": 10_000, "update_ms": med(up[1:]), "append_ms": med(ap[1:]), "first_search_ms": round(first_ms, 3),
                       "second_search_ms": round(second_ms, 3)}
        result["widths"].append(w)
        del h, d_data, d_copy
        torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
