"""Candidate kernel against the masked scan at the point of DESIGN.md §28, by live share.

  python scripts/maxsim_rerank_point.py --dtype f16|i8 [--records 1000000] [--tokens 64] [--dim 128] [--tq 32] [--k 10] [--reps 7] [--out FILE]

One store (the block of scripts/maxsim_point.py appended over and over), one query.  For each live share 1/1024, 1/256, 1/64, 1/16, 1/4
the live records are evenly spaced rows; timed with the handle's HIP events on its stream (median of --reps): the candidate path through
MultiVectorIndex.rerank_batch_arrays and the filtered search through search_batch_arrays with the same rows as its BitSet — `path` says
which kernel answered that one (an int8 store routes small shares to the candidate kernel itself; the scan reads every token row whatever
the mask, so its time at the unrouted shares stands for the others).  Also: whether the two paths returned the same rows and score BITS.
One JSON line per dtype, appended to --out.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--records", type=int, default=1_000_000)
    p.add_argument("--tokens", type=int, default=64)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--tq", type=int, default=32)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--dtype", default="i8", choices=["f16", "i8"])
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import lynsedb_amd as L

    if L._lib.device_count() < 1:
        raise SystemExit("needs a HIP device")
    rng = np.random.default_rng(7)
    idx = L.MultiVectorIndex(a.dim, device=0, dtype=a.dtype)
    block = 20_000
    base = rng.standard_normal((block, a.tokens, a.dim)).astype(np.float32)
    for r0 in range(0, a.records, block):
        idx.append(list(base[:min(block, a.records - r0)]))
    q = rng.standard_normal((a.tq, a.dim)).astype(np.float32)

    def timed(call):
        call()   # warm-up: code objects, scratch
        idx.profile_enable(True)
        idx.profile_get(reset=True)
        kernel, pipeline = [], []
        for _ in range(a.reps):
            out = call()
            prof = idx.profile_get(reset=True)
            kernel.append(prof["scan_us"])
            pipeline.append(prof["total_us"])
        idx.profile_enable(False)
        return out, float(np.median(kernel)), float(np.median(pipeline)), "candidates" if prof["last_plan"] == 1 else "scan"

    table = []
    for den in (1024, 256, 64, 16, 4):
        rows = np.arange(0, a.records, den, dtype=np.uint64)
        words = L.BitSet.from_rows(rows, a.records).words
        (r1, s1, _), ck, cp, _ = timed(lambda: idx.rerank_batch_arrays([q], [rows], a.k))
        (r2, s2, _), sk, sp, path = timed(lambda: idx.search_batch_arrays([q], a.k, words))
        table.append({"share": f"1/{den}", "candidates": int(rows.size), "cand_kernel_us": round(ck, 1), "cand_pipeline_us": round(cp, 1),
                      "search_kernel_us": round(sk, 1), "search_pipeline_us": round(sp, 1), "search_path": path,
                      "same_rows": bool(np.array_equal(r1, r2)), "same_score_bits": bool(np.array_equal(s1.view(np.uint32), s2.view(np.uint32)))})
    # every candidate of the smallest share, not just the best k: the two paths' score bits side by side
    rows = np.arange(0, a.records, 1024, dtype=np.uint64)
    r1, s1, _ = idx.rerank_batch_arrays([q], [rows], rows.size)
    r2, s2, _ = idx.search_batch_arrays([q], rows.size, L.BitSet.from_rows(rows, a.records).words)
    table.append({"share": "1/1024, k = candidates", "candidates": int(rows.size), "same_rows": bool(np.array_equal(r1, r2)),
                  "scores_differing_in_bits": int((s1.view(np.uint32) != s2.view(np.uint32)).sum())})
    line = json.dumps({"dtype": a.dtype, "records": a.records, "tokens_per_record": a.tokens, "dim": a.dim, "tq": a.tq, "k": a.k, "reps": a.reps, "table": table})
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
