"""Row mutation on the CPU: the plan of a compaction (lynse_hip_compact_plan) against numpy.cumsum over every keep set and window size
of the contract, and the refusals that come before any device is touched.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from lynsedb_amd import _lib
from lynsedb_amd.core import BitSet, FlatIndex

lib = _lib.lib
STAGE_BYTES = 64 << 20
UNTOUCHED, DIRECT, STAGED = 0, 1, 2
NS = (0, 1, 63, 64, 65, 1000)
WINDOWS = (0, 64, 128)
ROW_BYTES = 32   # (dim 5 at pitch 8: the default window is then 2M rows, one window at these n)


def keep_sets(n):
    rng = np.random.default_rng(1000 + n)
    idx = np.arange(n)
    sets = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "not_row0": idx != 0, "not_last": idx != n - 1,
            "clear_0_62": idx > 62, "clear_0_63": idx > 63, "clear_0_64": idx > 64, "alternating": idx % 2 == 0,
            "alternating_odd": idx % 2 == 1}
    for p in (0.1, 0.5, 0.9):
        sets[f"random_{p}"] = rng.random(n) >= p   # p = the share deleted
    return sets


def words_of(keep, extra_words=0, garbage=False):
    n = keep.size
    bits = np.concatenate([keep, np.full(-n % 64 + 64 * extra_words, garbage, bool)])
    return np.packbits(bits, bitorder="little").view(np.uint64) if bits.size else np.zeros(0, np.uint64)


def plan(words, n, window_rows, row_bytes=ROW_BYTES):
    live, wrows, nwin = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    w = np.ascontiguousarray(words, dtype=np.uint64)
    args = (w.ctypes.data_as(C.c_void_p), w.size, n, window_rows, row_bytes, C.byref(live), C.byref(wrows), C.byref(nwin))
    _lib.check(lib.lynse_hip_compact_plan(*args, None, None))
    base = np.full((n + 63) // 64, 0xdeadbeef, np.uint32)
    win = np.full((nwin.value, 4), 0xdeadbeef, np.uint64)
    _lib.check(lib.lynse_hip_compact_plan(*args, base.ctypes.data_as(C.c_void_p), win.ctypes.data_as(C.c_void_p)))
    return live.value, wrows.value, base, win


def model(keep, window_rows, row_bytes=ROW_BYTES):
    """the plan restated with numpy.cumsum: the destination of a row is the number of kept rows before it"""
    n = keep.size
    W = window_rows or max(64, STAGE_BYTES // row_bytes // 64 * 64)
    dest = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)   # dest[r] = kept rows below r
    base = dest[np.arange(0, n, 64)] if n else np.zeros(0, np.int64)
    win = []
    for s in range(0, n, W):
        e = min(s + W, n)
        d, live = int(dest[s]), int(dest[e] - dest[s])
        path = UNTOUCHED if (d == s and live == e - s) else (DIRECT if d + live <= s else STAGED)
        win.append((s, d, live, path))
    return int(dest[n]), W, base, np.array(win, np.int64).reshape(-1, 4)


CASES = [(n, w, name) for n in NS for w in WINDOWS for name in keep_sets(8)]   # (the names do not depend on n)


def test_compact_plan_matches_the_cumsum_model():
    paths = set()
    direct_rule_seen = {True: 0, False: 0}
    for n, w, name in CASES:
        keep = keep_sets(n)[name]
        for words in (words_of(keep), words_of(keep, extra_words=2, garbage=True)):   # garbage bits set beyond n, and words beyond ceil(n / 64)
            live, wrows, base, win = plan(words, n, w)
            e_live, e_w, e_base, e_win = model(keep, w)
            assert live == e_live == int(keep.sum()), (n, w, name)
            assert wrows == e_w
            assert np.array_equal(base.astype(np.int64), e_base), (n, w, name)
            assert np.array_equal(win.astype(np.int64), e_win), (n, w, name)
            for s, d, lv, path in win.astype(np.int64):
                assert (path == DIRECT) == (d + lv <= s)   # direct iff destinations and sources of the window are disjoint
                direct_rule_seen[bool(d + lv <= s)] += 1
                paths.add(int(path))
                assert d <= s and d + lv <= s + e_w   # every row moves down; a staged copy ends at or below its window's end
    assert paths == {UNTOUCHED, DIRECT, STAGED}
    assert direct_rule_seen[True] > 0 and direct_rule_seen[False] > 0


def test_the_window_edges_of_the_contract():
    # W = 64 over 1000 rows: a shift of 63 rows is staged everywhere, a shift of 64 makes every later window direct
    for cleared, first_path in ((63, STAGED), (64, DIRECT), (65, DIRECT)):
        keep = np.arange(1000) >= cleared
        _, _, _, win = plan(words_of(keep), 1000, 64)
        assert int(win[0, 3]) == (DIRECT if cleared >= 64 else STAGED)   # (window 0 of 64 cleared rows is live 0: nothing to move)
        assert all(int(p) == first_path for p in win[1:-1, 3]), cleared   # (every full window; the last one holds 40 rows)
        assert int(win[-1, 3]) == DIRECT
    # only row 0 cleared: every window staged, destination overlapping its own window by all but one row
    _, _, base, win = plan(words_of(np.arange(1000) != 0), 1000, 64)
    assert all(int(p) == STAGED for p in win[:, 3]) and np.array_equal(win[1:, 1], win[1:, 0] - 1)
    # only the last row cleared: the prefix is untouched, the last window staged
    _, _, _, win = plan(words_of(np.arange(1000) != 999), 1000, 64)
    assert [int(p) for p in win[:, 3]] == [UNTOUCHED] * 15 + [STAGED]


def test_default_window():
    for row_bytes, expect in ((32, 2097152), (512, 131072), (3072, 21824), (80000, 832), (2 << 20, 64), (STAGE_BYTES * 4, 64), (272, 246720)):
        assert plan(words_of(np.ones(70, bool)), 70, 0, row_bytes)[1] == expect
    assert FlatIndex.compact_plan(np.ones(70, bool), 70, 0, 512)["window_rows"] == 131072
    p = FlatIndex.compact_plan(BitSet.from_rows([1, 2, 69], 70), 70, 64)
    assert p["live"] == 3 and p["word_base"].tolist() == [0, 2] and p["windows"].tolist() == [[0, 0, 2, STAGED], [64, 2, 1, DIRECT]]


def test_refusals_before_any_device():
    live, wrows, nwin = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
    outs = (C.byref(live), C.byref(wrows), C.byref(nwin))
    w = np.zeros(2, np.uint64)
    wp = w.ctypes.data_as(C.c_void_p)
    E = _lib.ERR_INVALID_ARGUMENT
    assert lib.lynse_hip_compact_plan(wp, 1, 65, 64, 32, *outs, None, None) == E          # n_words too small
    assert "ceil(len / 64)" in _lib.last_error()
    assert lib.lynse_hip_compact_plan(wp, 2, 65, 64, 32, *outs, None, None) == _lib.OK
    for bad in (1, 63, 65, 100):
        assert lib.lynse_hip_compact_plan(wp, 2, 65, bad, 32, *outs, None, None) == E      # window_rows not a multiple of 64
        assert "multiple of 64" in _lib.last_error()
    assert lib.lynse_hip_compact_plan(None, 2, 65, 64, 32, *outs, None, None) == E        # NULL pointers
    assert lib.lynse_hip_compact_plan(None, 0, 0, 64, 32, *outs, None, None) == _lib.OK   # (no rows: no words needed)
    assert lib.lynse_hip_compact_plan(wp, 2, 65, 64, 32, None, C.byref(wrows), C.byref(nwin), None, None) == E
    assert lib.lynse_hip_compact_plan(wp, 2, 65, 64, 32, C.byref(live), None, C.byref(nwin), None, None) == E
    assert lib.lynse_hip_compact_plan(wp, 2, 65, 64, 32, C.byref(live), C.byref(wrows), None, None, None) == E
    with pytest.raises(ValueError):
        FlatIndex.compact_plan(np.ones(65, bool), 65, 100)
    # the device calls: a NULL handle is refused before anything else
    rows = np.zeros(1, np.uint64)
    data = np.zeros(4, np.float32)
    rp, dp = rows.ctypes.data_as(C.c_void_p), data.ctypes.data_as(C.c_void_p)
    assert lib.lynse_hip_flat_update_rows_f32(None, rp, dp, 1) == E
    assert lib.lynse_hip_flat_compact_rows(None, wp, 2, 0, None) == E
    assert lib.lynse_hip_flat_gather_rows(None, rp, 1, dp) == E


def test_symbols_exported_and_abi_version():
    raw = C.CDLL(str(_lib.LIB_PATH))
    for s in ("lynse_hip_flat_update_rows_f32", "lynse_hip_flat_compact_rows", "lynse_hip_flat_gather_rows", "lynse_hip_compact_plan"):
        assert hasattr(raw, s) and s in _lib.SIGNATURES
    assert lib.lynse_hip_abi_version() == 1
