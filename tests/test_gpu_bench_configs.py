"""`bench.py --config c4 / c5` (and the headline c2) end to end at reduced sizes (one GPU, and 2 / 3 / 4 gloo ranks sharing it): with `--full`
the line is printed, names the workload BASELINE.json names, and its own verification legs are green (tickets == the blocking search; recall
against the exact top-k of the whole collection for IVF, the oracle's packed search for Hamming).  At most four ranks share a test
box's one GPU (with the pytest process, five processes hold the device); the 8-rank exchange and merge are covered in one process
(tests/test_gpu_flat_parity.py::test_device_merge_matches_host_merge, tests/test_gpu_sharded_kmeans.py) and over 8 gloo processes on
the CPU (tests/test_sharded_gloo.py)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def run_bench(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    p = subprocess.run([sys.executable, str(ROOT / "bench.py")] + args, cwd=str(ROOT), env=e, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("gpus", [1, 2, 4])
def test_bench_config_c4_prints_a_verified_line(gpus):
    env = {"LYNSE_BENCH_BACKEND": "gloo"} if gpus > 1 else None       # two ranks share the one GPU of a test box: no RCCL between them
    d = run_bench(["--config", "c4", "--gpus", str(gpus), "--rows-per-gpu", "150000", "--nlist", "512", "--nprobe", "16", "--steps", "4", "--warmup", "1", "--full"], env)
    assert d["n_gpus"] == gpus and d["scaling"] == "weak" and d["unit"] == "queries/s" and d["value"] > 0
    assert "IVF-Flat IP %dx768" % (150000 * gpus) in d["metric"] and d["config"]["lists_trained"] == 512
    assert d["verify"]["tickets_equal_blocking_search"] is True
    assert d["verify"]["recall_at_k_vs_exact_top_k_of_the_collection"] >= 0.8      # (IVF is approximate: 512 lists over 4096 generating centres, 2 Lloyd iterations)
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["achieved"] > 0
    if gpus == 1:
        assert d["tickets"]["in_flight"] > 0 and d["tickets"]["redone_in_wait"] == 0
        assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["value"] > 0, d["cpu_baseline"]


@pytest.mark.parametrize("gpus", [1, 2, 4])
def test_bench_config_c5_prints_a_verified_line(gpus):
    env = {"LYNSE_BENCH_BACKEND": "gloo"} if gpus > 1 else None
    d = run_bench(["--config", "c5", "--gpus", str(gpus), "--rows", str(600000 * gpus), "--steps", "4", "--warmup", "1", "--full", "--no-cpu-baseline"], env)
    assert d["n_gpus"] == gpus and d["dtype"] == "u64" and d["value"] > 0
    assert "Hamming %dx1024-bit" % (600000 * gpus) in d["metric"] and "k=50" in d["metric"]
    assert d["verify"] == {"tickets_equal_blocking_search": True, "oracle_bit_exact_on_200k_row_sample": True}


@pytest.mark.parametrize("gpus", [3, 4])
def test_bench_headline_runs_sharded_over_3_and_4_ranks(gpus):
    """The headline workload (FLAT-IP, 256 queries, k = 10) row-sharded over 3 / 4 gloo ranks that share the one GPU (3: shards of unequal
    length): the exchange (torch all-gather under gloo) + canonical merge, recall against the exact top-k of the WHOLE collection."""
    d = run_bench(["--gpus", str(gpus), "--rows", "400000", "--steps", "4", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-configs", "--settle-ms", "0"],
                  {"LYNSE_BENCH_BACKEND": "gloo"})
    assert d["n_gpus"] == gpus and d["scaling"] == "strong" and d["value"] > 0
    assert d["verify"]["recall_at_k_tolerant"] == 1.0, d["verify"]


def test_bench_dump_outputs_repeat_from_run_to_run(tmp_path):
    """`--dump-outputs DIR`: the last timed step's batch (ids / distances / counts as float64 / float32 .npy) is written, and two runs with the
    same arguments write the same arrays (the inputs depend on the arguments only); `--steps` is the number of timed steps on the line."""
    import numpy as np

    args = ["--gpus", "1", "--rows", "400000", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-configs", "--settle-ms", "0"]
    runs = [run_bench(args + ["--dump-outputs", str(tmp_path / r)]) for r in ("a", "b")]
    for d in runs:
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["dumped_outputs"]["files"] == ["counts.npy", "distances.npy", "ids.npy", "query_index.npy"]
    got = [{n: np.load(tmp_path / r / ("%s.npy" % n)) for n in ("ids", "distances", "counts", "query_index")} for r in ("a", "b")]
    a, b = got
    assert a["ids"].shape == (256, 10) and a["distances"].shape == (256, 10) and a["counts"].shape == (256,)
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert np.all(a["counts"] == 10) and np.all((a["ids"] >= 0) & (a["ids"] < 400000))
    assert np.all(np.diff(a["distances"], axis=1) <= 0)          # IP: best first
    for n in a:
        assert np.array_equal(a[n], b[n]), n


def test_bench_plain_run_leaves_the_full_keys_out():
    """Without `--full` the run sets up, warms up, times its steps and prints the headline line: nothing that needs work of its own
    (verification, the blocking-batch latency, two batches in flight, the CPU baseline, the other configurations) is on it."""
    d = run_bench(["--gpus", "1", "--rows", "400000", "--steps", "3", "--warmup", "1"])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "queries/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and "FLAT-IP 400000x768" in d["metric"]
    assert d["roofline"]["launches"] > 0
    full_only = {"verify", "blocking_ms_per_batch", "two_in_flight_ms_per_step", "cpu_baseline", "same_shard_variants", "second_distribution", "configs"}
    assert not full_only & d.keys(), sorted(full_only & d.keys())
