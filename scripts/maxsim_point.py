"""Measured point of the multi-vector (MaxSim) scan against its two bounds.

  python scripts/maxsim_point.py [--records 1000000] [--tokens 64] [--dim 128] [--tq 32] [--k 10] [--reps 7] [--dtype f32|f16|i8|mxfp4] [--out profiles/maxsim_point.json]

The store is one block of 20,000 random records appended over and over (the scan's time does not depend on the values).  Reported: the
median blocking time of MultiVectorIndex.search_batch_arrays for one query, and from the handle's HIP events the time of the scan kernel
alone (k_maxsim_scan, k_maxsim_h16 with --dtype f16, k_maxsim_i8 with --dtype i8, k_maxsim_mx4 with --dtype mxfp4), with the bytes it streams (token rows x ld x 4, x 2, x 1 + 4 of scale, or x 1/2 + the padded scale bytes) over that time against 8 TB/s and its multiply-adds (2 x round_up(tq, 32) x token
rows x ld) against the 157 TFLOP/s of v_mfma_f32_32x32x2_f32 on 256 CUs at 2.4 GHz.  One JSON line, also written to --out.
"""
import argparse
import json
import sys
import time
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
    p.add_argument("--dtype", default="f32", choices=["f32", "f16", "i8", "mxfp4"])
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
    counts = idx.counts()
    q = rng.standard_normal((a.tq, a.dim)).astype(np.float32)
    idx.search_batch_arrays([q], a.k)   # warm-up: code objects, scratch
    blocking = []
    idx.profile_enable(True)
    idx.profile_get(reset=True)
    for _ in range(a.reps):
        t0 = time.perf_counter()
        idx.search_batch_arrays([q], a.k)
        blocking.append(time.perf_counter() - t0)
    prof = idx.profile_get(reset=True)
    idx.profile_enable(False)
    ld = (a.dim + 31) // 32 * 32
    scan_s = prof["scan_us"] / prof["scan_launches"] * 1e-6
    row_bytes = {"f32": ld * 4, "f16": ld * 2, "i8": ld + 4, "mxfp4": ld // 2 + (ld // 32 + 3) // 4 * 4}[a.dtype]
    nbytes = counts["tokens"] * row_bytes
    flops = 2 * ((a.tq + 31) // 32 * 32) * counts["tokens"] * ld
    out = {"dtype": a.dtype, "kernel": {"f16": "k_maxsim_h16", "i8": "k_maxsim_i8", "mxfp4": "k_maxsim_mx4"}.get(a.dtype, "k_maxsim_scan"), "records": counts["records"], "tokens": counts["tokens"], "ranges": counts["ranges"], "dim": a.dim, "tq": a.tq, "k": a.k,
           "blocking_ms_median": round(float(np.median(blocking)) * 1e3, 3), "blocking_ms_min_max": [round(min(blocking) * 1e3, 3), round(max(blocking) * 1e3, 3)],
           "scan_ms": round(scan_s * 1e3, 3), "pipeline_ms": round(prof["total_us"] / prof["scan_launches"] * 1e-3, 3),
           "scan_bytes": nbytes, "scan_tb_s": round(nbytes / scan_s / 1e12, 3), "of_8_tb_s": round(nbytes / scan_s / 8e12, 3),
           "scan_flops": flops, "scan_tflop_s": round(flops / scan_s / 1e12, 2), "of_157_tflop_s": round(flops / scan_s / 157.3e12, 3)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
