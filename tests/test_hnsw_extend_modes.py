"""The incremental HNSW insert (rule 7 of the HNSW block of include/lynse_hip.h) without a GPU: the C ABI's NULL handles, the prefix
property of the level stream the rule rests on, a numpy model of the flag rule against brute force, and the new kernel's resources."""
import ctypes as C

import numpy as np
import pytest

import hnsw_common as H
from hnsw_extend_common import ask_list, flagged
from lynsedb_amd import _lib

IP, L2 = H.IP, H.L2


def test_null_handle():
    out = np.zeros(12, np.float64)
    assert _lib.lib.lynse_hip_flat_hnsw_extend(None, 0) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.lib.lynse_hip_flat_hnsw_extend(None, 7) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.lib.lynse_hip_flat_hnsw_extend_stats(None, out.ctypes.data_as(C.c_void_p)) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.lib.lynse_hip_abi_version() == 1


@pytest.mark.parametrize("seed,m,max_level", [(42, 16, None), (42, 4, None), (7, 2, None), (7, 2, 3), (0, 32, 0), (2**63 + 5, 3, 1)])
def test_level_stream_has_the_prefix_property(seed, m, max_level):
    """row i's level is the i-th draw whatever the number of rows: the levels of an extended graph begin with the stored ones"""
    def lib_levels(n):
        out = np.zeros(max(n, 1), np.uint32)
        assert _lib.lib.lynse_hip_hnsw_levels(seed, m, -1 if max_level is None else max_level, n, out.ctypes.data_as(C.c_void_p)) == 0
        return out[:n]

    full = lib_levels(1500)
    assert np.array_equal(full, H.levels_py(seed, m, max_level, 1500))
    for n in (0, 1, 2, 63, 64, 1000, 1499):
        assert np.array_equal(lib_levels(n), full[:n]), n


MODEL_CASES = [("random", 60, 12, 5), ("duplicates", 60, 12, 5), ("short", 4, 3, 5), ("short by one", 6, 2, 5), ("copies appended", 50, 8, 3)]


@pytest.mark.parametrize("metric", [L2, IP])
@pytest.mark.parametrize("name,n0,add,efc", MODEL_CASES)
def test_flag_rule_never_misses_a_changed_list(metric, name, n0, add, efc):
    """Integer-valued rows, so every score is exact in float64 and ties are real.  Brute force: the ask-lists (ask = ef_construction + 1,
    order (d, row)) of every old row over n0 and over n1 rows.  Every row whose list differs is flagged by the rule; so is every row whose
    list is short.  Rows that duplicate row i and have lower numbers push i out of its own list: the ask-th entry, not the
    ef_construction-th, is the threshold that covers it."""
    rng = np.random.default_rng(len(name) * 10 + metric)
    n1, ask = n0 + add, efc + 1
    data = rng.integers(-2, 3, (n1, 4)).astype(np.float64)
    if name == "duplicates":
        data = data[rng.integers(0, 9, n1)]      # nine distinct rows: more copies of a row than a list holds
    if name == "copies appended":
        data[n0:] = data[rng.integers(0, n0, add)]
    changed = flagged_n = 0
    for i in range(n0):
        before, after = ask_list(metric, data, i, n0, ask), ask_list(metric, data, i, n1, ask)
        f = flagged(metric, data, i, n0, n1, ask)
        if before != after:
            changed += 1
            assert f, (name, i, before, after)
        if len(before) < ask:
            assert f, (name, i, "short")
        flagged_n += f
    assert changed > 0, "the case exercises nothing"
    if name == "duplicates":   # some row does not come back from its own search
        assert any(i not in ask_list(metric, data, i, n0, ask) for i in range(n0))
    if name == "random" and metric == L2:
        assert flagged_n < n0   # and the rule is not "flag everything"


def test_reverse_scan_kernel_keeps_its_registers():
    """k_hnsw_reverse_scan in csrc/resource_usage.txt: no scratch, no spilled register, and registers for the 16 waves of its block (four
    per SIMD), which is what lets one block hold a CU's LDS"""
    import re
    from pathlib import Path

    import lynsedb_amd

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    assert rep.exists(), "the build writes csrc/resource_usage.txt"
    blocks = re.findall(r"Function Name: (\S+)(.*?)LDS Size", rep.read_text(), flags=re.S)
    mine = [(n, {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", body)})
            for n, body in blocks if "k_hnsw_reverse_scan" in n]
    assert mine, "k_hnsw_reverse_scan is not in the report"
    for name, f in mine:
        assert f["ScratchSize [bytes/lane]"] == 0 and f["SGPRs Spill"] == 0 and f["VGPRs Spill"] == 0, (name, f)
        assert f["Occupancy [waves/SIMD]"] >= 4, (name, f)
