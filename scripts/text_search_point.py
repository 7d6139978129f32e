"""Measured point of the BM25 text search (TextIndex, k_text_scan).

  python scripts/text_search_point.py [--rows 1000000] [--vocab 30522] [--mean-len 120] [--qterms 6] [--batches 1,16,256] [--k 10] [--reps 7]

One process, one GPU initialisation.  The corpus is the one of scripts/sparse_search_point.py (same seed, same draws), so the two scans
can be set side by side: document lengths log-normal around `mean-len`, term popularity Zipf-like (weight 1 / (rank + 10)^0.8 over a
shuffled vocabulary); a term drawn twice into a document has tf 2 where the sparse store kept one entry.  Queries of `qterms` distinct
terms drawn from the same popularity.  Per batch size the median, min and max blocking time of TextIndex.search_batch_arrays, and from
the handle's profile the scan launches, their summed time (HIP events) and the bytes they read (12 per posting of the query's terms),
with the fraction of 8 TB/s that makes.  Kernel times proper come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/text_search_point.py --no-host ...` run.  The first queries' results are checked
against the test suite's C restatement (tests/text_ref/text_ref.c).  One JSON line.
"""
import argparse
import json
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


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--vocab", type=int, default=30522)
    p.add_argument("--mean-len", type=float, default=120.0)
    p.add_argument("--qterms", type=int, default=6)
    p.add_argument("--batches", default="1,16,256")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--no-host", action="store_true", help="skip the host restatement (a profiler run)")
    a = p.parse_args()
    import lynsedb_amd as L
    import text_common as tc

    if L._lib.device_count() < 1:
        raise SystemExit("needs a HIP device")
    rng = np.random.default_rng(18)
    w = 1.0 / (np.arange(a.vocab) + 10.0) ** 0.8
    pop = w / w.sum()
    cdf = np.cumsum(pop)
    cdf[-1] = 1.0
    perm = rng.permutation(a.vocab)
    lens = np.clip(rng.lognormal(np.log(a.mean_len), 0.5, a.rows), 1, 2000).astype(np.int64)
    row = np.repeat(np.arange(a.rows, dtype=np.int64), lens)
    term = perm[np.searchsorted(cdf, rng.random(row.size))].astype(np.int64)
    say("tokens drawn:", row.size)
    key, tf = np.unique(row * (1 << 32) + term, return_counts=True)   # ascending (document, term)
    del row, term
    doc_ptr = np.zeros(a.rows + 1, np.uint64)
    np.cumsum(np.bincount(key >> 32, minlength=a.rows), out=doc_ptr[1:])
    corpus = tc.Corpus(doc_ptr, (key & 0xFFFFFFFF).astype(np.uint32), tf.astype(np.uint32), a.vocab)
    del key, tf
    say("documents built:", corpus.doc_term.size, "postings")
    term_ptr, post_row, post_tf = corpus.csc()
    say("postings sorted")
    batches = [int(b) for b in a.batches.split(",")]
    qprob = pop[np.argsort(perm)]   # the popularity of term id t
    queries = tc.Queries([(rng.choice(a.vocab, a.qterms, replace=False, p=qprob), np.ones(a.qterms)) for _ in range(max(batches))])
    idx = L.TextIndex(device=0)
    t0 = time.perf_counter()
    idx.set(corpus.doc_len, term_ptr, post_row, post_tf)
    out = {"rows": a.rows, "nnz": int(post_row.size), "mean_len": round(float(corpus.doc_len.mean()), 1), "vocab": a.vocab, "qterms": a.qterms,
           "k": a.k, "upload_s": round(time.perf_counter() - t0, 2), "hbm_bytes": idx.hbm_bytes(), "batches": {}}
    say("store set")
    ref = None if a.no_host else tc.build_ref(tempfile.mkdtemp(prefix="text_ref_"))
    for nq in batches:
        q = tc.Queries(queries.lists[:nq])
        got = idx.search_batch_arrays(*q.arrays(), a.k)
        med, lo, hi = timed(lambda: idx.search_batch_arrays(*q.arrays(), a.k), a.reps)
        idx.profile_enable(True)
        idx.profile_get(reset=True)
        idx.search_batch_arrays(*q.arrays(), a.k)
        prof = idx.profile_get(reset=True)
        idx.profile_enable(False)
        point = {"blocking_ms": round(med / 1e3, 4), "min_ms": round(lo / 1e3, 4), "max_ms": round(hi / 1e3, 4),
                 "scan_launches": int(prof["scan_launches"]), "scan_us": round(prof["scan_us"], 1), "scan_bytes": int(prof["scan_bytes"]),
                 "pipeline_us": round(prof["total_us"], 1),
                 "scan_tb_per_s": round(prof["scan_bytes"] / max(prof["scan_us"], 1e-9) / 1e6, 4),
                 "fraction_of_8tbps": round(prof["scan_bytes"] / max(prof["scan_us"], 1e-9) / 1e6 / 8.0, 5),
                 "score_matrix_bytes": 4 * a.rows * nq, "passed_mean": float(np.mean(got[3]))}
        if ref is not None:
            hq = min(nq, 4)
            tc.check_batch(tuple(x[:hq] for x in got), ref.batch(corpus, tc.Queries(queries.lists[:hq]), a.k), a.k)
            point["checked_queries"] = hq
        out["batches"][str(nq)] = point
        say("batch", nq, point)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
