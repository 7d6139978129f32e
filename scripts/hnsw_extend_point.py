"""Measured points of the incremental HNSW insert against the plain build of the same handle.

  python scripts/hnsw_extend_point.py [--rows 1000000] [--dims 128,768] [--adds 1,100,10000] [--runs 3] [--clusters 1000]
                                      [--spread 0.15] [--m 16] [--ef-construction 128] [--out profiles/hnsw_extend_point.json]

Per width: the §19 data (Gaussian clusters, L2).  Per number of appended rows b and run: a fresh handle, FlatIndex.build_hnsw over the
first rows - b rows, the last b appended, FlatIndex.extend_hnsw(0) timed with its stats — and beside it, on the same handle, the
yardstick: FlatIndex.build_hnsw over all rows.  Where mode 0 answers with the plain build (path 1) the same shape is run once more
with mode 1, to show where the incremental path stops paying.  Medians over the runs; one JSON line per width, the whole list in --out.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def one_run(L, data, b, mode, a):
    n = data.shape[0]
    idx = L.FlatIndex(None, data.shape[1], device=0)
    step = 100_000
    for r0 in range(0, n - b, step):
        idx.write(data[r0:min(r0 + step, n - b)])
    idx.build_hnsw("l2", a.m, a.ef_construction, 50)
    idx.write(data[n - b:])
    t0 = time.perf_counter()
    idx.extend_hnsw(mode)
    extend_s = time.perf_counter() - t0
    st = idx.hnsw_extend_stats()
    assert idx.hnsw_params(arrays=False)["n"] == n
    t0 = time.perf_counter()
    idx.build_hnsw("l2", a.m, a.ef_construction, 50)
    build_s = time.perf_counter() - t0
    return extend_s, build_s, st


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--dims", default="128,768")
    p.add_argument("--adds", default="1,100,10000")
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--clusters", type=int, default=1000)
    p.add_argument("--spread", type=float, default=0.15)
    p.add_argument("--m", type=int, default=16)
    p.add_argument("--ef-construction", type=int, default=128)
    p.add_argument("--out", default="profiles/hnsw_extend_point.json")
    a = p.parse_args()
    import lynsedb_amd as L

    if L._lib.device_count() < 1:
        raise SystemExit("needs a HIP device")
    results = []
    for dim in (int(d) for d in a.dims.split(",")):
        rng = np.random.default_rng(7)
        cen = rng.standard_normal((a.clusters, dim)).astype(np.float32)
        data = np.empty((a.rows, dim), np.float32)
        step = 100_000
        for r0 in range(0, a.rows, step):
            r = min(step, a.rows - r0)
            data[r0:r0 + r] = cen[rng.integers(0, a.clusters, r)] + np.float32(a.spread) * rng.standard_normal((r, dim), dtype=np.float32)
        out = {"rows": a.rows, "dim": dim, "m": a.m, "ef_construction": a.ef_construction, "runs": a.runs, "points": []}
        for b in (int(x) for x in a.adds.split(",")):
            modes = [0]
            for mode in modes:
                runs = [one_run(L, data, b, mode, a) for _ in range(a.runs if mode == 0 else 1)]
                ext, bld = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
                st = sorted(runs, key=lambda r: r[0])[len(runs) // 2][2]
                out["points"].append({"added": b, "mode": mode, "extend_s": round(ext, 4), "build_s": round(bld, 4), "build_over_extend": round(bld / ext, 2),
                                      "extend_runs_s": [round(r[0], 4) for r in runs], "build_runs_s": [round(r[1], 4) for r in runs], "stats": st})
                if mode == 0 and st["path"] == 1:
                    modes.append(1)
                print(json.dumps(out["points"][-1]), flush=True)
        results.append(out)
        print(json.dumps(out), flush=True)
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
