"""CPU tests of range search (Collection::search_range, src/engine.rs:6410-6483): the C-ABI entry is declared, exported and bound, the
Python methods exist, and the early returns that touch no device behave as the reference's do.  No compute calls are made."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SYM = "lynse_hip_flat_search_range_f32"


def test_symbol_declared_exported_and_bound():
    import lynsedb_amd._lib as lb

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "lynse_hip.h").read_text(), flags=re.S)
    decl = re.search(r"\bint\s+" + SYM + r"\s*\(([^;]*)\)\s*;", text)
    assert decl, f"{SYM} is not declared in include/lynse_hip.h"
    n_args = len([a for a in decl.group(1).split(",") if a.strip()])
    assert hasattr(C.CDLL(str(lb.LIB_PATH)), SYM), f"{SYM} is not exported"
    res, args = lb.SIGNATURES[SYM]
    assert res is C.c_int and len(args) == n_args == 12
    assert lb.lib.lynse_hip_abi_version() == 1


def test_python_methods_exist():
    import inspect

    import lynsedb_amd as L

    p = inspect.signature(L.FlatIndex.search_range_batch_arrays).parameters
    assert list(p)[1:] == ["queries", "thresholds", "max_results", "metric", "bitset_words"] and p["bitset_words"].default is None
    p = inspect.signature(L.Collection.search_range).parameters
    assert list(p)[1:] == ["vector", "threshold", "max_results", "subset"]
    assert p["max_results"].default == 1000 and p["subset"].default is None


def test_max_results_zero_returns_empty_without_a_device():
    import lynsedb_amd as L

    # objects that never opened a device: the early return comes before anything touches the handle (engine.rs:6416-6418)
    coll = L.Collection.__new__(L.Collection)
    assert coll.search_range([0.0, 1.0], 0.5, max_results=0) == ([], [])
    flat = L.FlatIndex.__new__(L.FlatIndex)
    flat._h, flat._dim = None, 3
    rows, dists, counts, passed = flat.search_range_batch_arrays(np.zeros((2, 3), np.float32), [0.0, 1.0], 0, "l2")
    assert rows.shape == (2, 0) and dists.shape == (2, 0)
    assert counts.tolist() == [0, 0] and passed.tolist() == [0, 0]


def test_null_arguments_return_error_codes():
    import lynsedb_amd._lib as lb

    q = np.zeros(4, np.float32)
    thr = np.zeros(1, np.float32)
    rows, dists = np.zeros(2, np.uint64), np.zeros(2, np.float32)
    counts, passed = np.full(1, 7, np.uint32), np.full(1, 7, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fn = lb.lib.lynse_hip_flat_search_range_f32
    assert fn(None, p(q), 1, p(thr), 2, lb.METRIC_IP, None, 0, p(rows), p(dists), p(counts), p(passed)) == lb.ERR_INVALID_ARGUMENT
    assert "NULL" in lb.last_error()
    assert counts[0] == 7 and passed[0] == 7   # nothing was written
