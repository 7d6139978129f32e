"""Measured point of the sparse-vector search (SparseIndex, k_sparse_scan).

  python scripts/sparse_search_point.py [--rows 1000000] [--vocab 30522] [--mean-len 120] [--qnnz 40] [--batches 1,16,256] [--k 10] [--reps 7]

One process, one GPU initialisation.  The store: row lengths log-normal around `mean-len`, index popularity Zipf-like (weight
1 / (rank + 10)^0.8 over a shuffled vocabulary), values N(0, 1); queries of `qnnz` entries drawn from the same popularity.  Per batch
size the median blocking time of SparseIndex.search_batch_arrays, and from the handle's profile the scan launches, their summed time
(HIP events) and the bytes they stream (nnz * 8 + (n + 1) * 8 per query tile), with the fraction of 8 TB/s that makes.  Kernel times
proper come from a separate `rocprofv3 --kernel-trace --stats -- python scripts/sparse_search_point.py ...` run.  As context only, the
time of the test suite's C restatement (tests/sparse_ref/sparse_ref.c — a port, not the reference) on this host for the same batch,
single-threaded and threaded over the queries; the first query's result is checked against it.  One JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts) * 1e6), 1), round(float(np.min(ts) * 1e6), 1), round(float(np.max(ts) * 1e6), 1)


def draw(rng, cdf, perm, lens):
    """rows of about `lens` distinct indices each, drawn by popularity -> CSR (duplicates inside a row collapse)"""
    n = lens.size
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    idx = perm[np.searchsorted(cdf, rng.random(row.size))].astype(np.int64)
    key = np.unique(row * (1 << 32) + idx)   # ascending (row, index), distinct
    row, idx = key >> 32, (key & 0xFFFFFFFF).astype(np.uint32)
    indptr = np.zeros(n + 1, np.uint64)
    np.cumsum(np.bincount(row, minlength=n), out=indptr[1:])
    return indptr, idx, rng.standard_normal(idx.size).astype(np.float32) + np.float32(1e-3)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--vocab", type=int, default=30522)
    p.add_argument("--mean-len", type=float, default=120.0)
    p.add_argument("--qnnz", type=int, default=40)
    p.add_argument("--batches", default="1,16,256")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--no-host", action="store_true", help="skip the host restatement (a profiler run)")
    a = p.parse_args()
    import lynsedb_amd as L
    import sparse_common as sc

    if L._lib.device_count() < 1:
        raise SystemExit("needs a HIP device")
    rng = np.random.default_rng(18)
    w = 1.0 / (np.arange(a.vocab) + 10.0) ** 0.8
    cdf = np.cumsum(w / w.sum())
    cdf[-1] = 1.0
    perm = rng.permutation(a.vocab)
    lens = np.clip(rng.lognormal(np.log(a.mean_len), 0.5, a.rows), 1, 2000).astype(np.int64)
    indptr, indices, values = draw(rng, cdf, perm, lens)
    values[values == 0] = 1
    batches = [int(b) for b in a.batches.split(",")]
    q_ptr, q_idx, q_val = draw(rng, cdf, perm, np.full(max(batches), a.qnnz, np.int64))
    q_val[q_val == 0] = 1
    idx = L.SparseIndex(device=0)
    t0 = time.perf_counter()
    idx.set_rows(indptr, indices, values)
    out = {"rows": a.rows, "nnz": int(indices.size), "mean_len": round(indices.size / a.rows, 1), "vocab": a.vocab, "qnnz": a.qnnz, "k": a.k,
           "upload_s": round(time.perf_counter() - t0, 2), "hbm_bytes": idx.hbm_bytes(), "batches": {}}
    rows_csr = sc.Csr(indptr, indices, values)
    ref = None
    if not a.no_host:
        ref = sc.build_ref(tempfile.mkdtemp(prefix="sparse_ref_"))
    for nq in batches:
        e = int(q_ptr[nq])
        qp, qi, qv = q_ptr[:nq + 1], q_idx[:e], q_val[:e]
        got = idx.search_batch_arrays(qp, qi, qv, a.k)
        med, lo, hi = timed(lambda: idx.search_batch_arrays(qp, qi, qv, a.k), a.reps)
        idx.profile_enable(True)
        idx.profile_get(reset=True)
        idx.search_batch_arrays(qp, qi, qv, a.k)
        prof = idx.profile_get(reset=True)
        idx.profile_enable(False)
        point = {"blocking_us": med, "min_us": lo, "max_us": hi, "scan_launches": int(prof["scan_launches"]), "scan_us": round(prof["scan_us"], 1),
                 "scan_bytes": int(prof["scan_bytes"]), "pipeline_us": round(prof["total_us"], 1),
                 "scan_tb_per_s": round(prof["scan_bytes"] / max(prof["scan_us"], 1e-9) / 1e6, 3),
                 "fraction_of_8tbps": round(prof["scan_bytes"] / max(prof["scan_us"], 1e-9) / 1e6 / 8.0, 4),
                 "passed_mean": float(np.mean(got[3]))}
        if ref is not None:
            hq = nq if nq <= 16 else 4   # (a large batch: the check only, the host would take most of a minute)
            queries = sc.Csr(qp[:hq + 1], qi[:int(qp[hq])], qv[:int(qp[hq])])
            t0 = time.perf_counter()
            smat = ref.scores(queries, rows_csr)
            if hq == nq:
                point["host_threaded_us"] = round((time.perf_counter() - t0) * 1e6, 1)
                point["host_threads"] = min(32, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count())
            if nq == 1:
                one = sc.Csr(qp[:2], qi[:int(qp[1])], qv[:int(qp[1])])
                t0 = time.perf_counter()
                ref.scores(one, rows_csr)
                point["host_single_us"] = round((time.perf_counter() - t0) * 1e6, 1)
            sc.check_batch(got, smat[:4], a.k) if nq <= 4 else sc.check_batch(tuple(x[:4] for x in got), smat[:4], a.k)
        out["batches"][str(nq)] = point
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
