"""Shared by the tests of the approximate flat search: the restatement (tests/approx_ref/approx_ref.c: plain C of the four paths with the
project's tie rule, checked on its own in tests/test_approx_modes.py) compiled and wrapped.  TEST INFRASTRUCTURE."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
f32 = np.float32
_vp = C.c_void_p
IP, L2, COS, L1, CHEB, CANB, BRAY = 0, 1, 2, 7, 8, 9, 10
NAME = {IP: "ip", L2: "l2", COS: "cosine", L1: "l1", CHEB: "chebyshev", CANB: "canberra", BRAY: "bray_curtis"}
IP_CASE = (0, "sum_desc", "sum_asc", "hybrid")


class Answer:
    def __init__(self, rows, dists, info, coarse, pool):
        self.rows, self.dists, self.coarse, self.pool = rows, dists, coarse, pool
        self.info = {"path": int(info[0]), "ip_case": IP_CASE[int(info[1])], "pool": int(info[2]), "sample_dims": int(info[3]),
                     "fell_back": bool(info[4])}


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def search(self, q, data, k, metric, eps=None, ip_form=0) -> Answer:
        """rows u64[c], RAW distances f32[c], what ran, the coarse score of every row and the pool in canonical coarse order"""
        q, data = np.ascontiguousarray(q, f32).reshape(-1), np.ascontiguousarray(data, f32)
        n, d = data.shape
        assert q.size == d
        rows, dists = np.zeros(max(k, 1), np.uint64), np.zeros(max(k, 1), f32)
        info, coarse = np.zeros(5, np.uint32), np.full(n, np.nan, f32)
        pool, pcnt = np.zeros(100000, np.uint32), C.c_uint32(0)
        c = self.lib.apx_search(q.ctypes.data_as(_vp), data.ctypes.data_as(_vp), n, d, int(k), int(metric), f32(np.nan if eps is None else eps),
                                int(ip_form), rows.ctypes.data_as(_vp), dists.ctypes.data_as(_vp), info.ctypes.data_as(_vp),
                                coarse.ctypes.data_as(_vp), pool.ctypes.data_as(_vp), C.byref(pcnt))
        return Answer(rows[:c], dists[:c], info, coarse, pool[:pcnt.value].copy())

    def round(self, dists, eps):
        return np.array([self.lib.apx_round_to_eps(f32(v), f32(eps)) for v in np.asarray(dists, f32).reshape(-1)], f32)

    def blocks(self, dim, sample):
        s, ln = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
        nb = self.lib.apx_blocks(int(dim), int(sample), s.ctypes.data_as(_vp), ln.ctypes.data_as(_vp))
        return [(int(s[i]), int(ln[i])) for i in range(nb)]


def build_ref(tmp_dir) -> Ref:
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no C compiler for tests/approx_ref/approx_ref.c"
    so = Path(tmp_dir) / "libapprox_ref.so"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-o", str(so),
                    str(HERE / "approx_ref" / "approx_ref.c"), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.apx_search.restype = C.c_uint32
    lib.apx_search.argtypes = [_vp, _vp, C.c_size_t, C.c_size_t, C.c_uint32, C.c_int, C.c_float, C.c_int, _vp, _vp, _vp, _vp, _vp,
                               C.POINTER(C.c_uint32)]
    lib.apx_normalize_eps.restype = C.c_float
    lib.apx_normalize_eps.argtypes = [C.c_float]
    lib.apx_round_to_eps.restype = C.c_float
    lib.apx_round_to_eps.argtypes = [C.c_float, C.c_float]
    lib.apx_row_sum.restype = C.c_float
    lib.apx_row_sum.argtypes = [_vp, C.c_size_t]
    for name in ("apx_ip_order_pool", "apx_hybrid_ip_pool", "apx_hybrid_pool"):
        getattr(lib, name).restype = C.c_uint64
        getattr(lib, name).argtypes = [C.c_uint64, C.c_uint64, C.c_float]
    for name in ("apx_hybrid_ip_sample", "apx_hybrid_sample"):
        getattr(lib, name).restype = C.c_uint32
        getattr(lib, name).argtypes = [C.c_uint32, C.c_float]
    lib.apx_blocks.restype = C.c_uint32
    lib.apx_blocks.argtypes = [C.c_uint32, C.c_uint32, _vp, _vp]
    return Ref(lib)


def f64_distances(q, data, metric) -> np.ndarray:
    """the metric's definition in float64 (no accumulation order): what the restatement is held to at the 1e-5 relative score contract"""
    q, x = np.asarray(q, np.float64), np.asarray(data, np.float64)
    if metric == IP:
        return x @ q
    if metric == L2:
        return ((x - q) ** 2).sum(1)
    if metric == COS:
        return 1.0 - (x @ q) / (np.sqrt((x * x).sum(1)) * np.sqrt((q * q).sum()))
    a = np.abs(x - q)
    if metric == L1:
        return a.sum(1)
    if metric == CHEB:
        return a.max(1)
    if metric == CANB:
        den = np.abs(x) + np.abs(q)
        return np.where(den != 0, a / np.where(den != 0, den, 1.0), 0.0).sum(1)
    return a.sum(1) / np.abs(x + q).sum(1)


def same_answer(rows, dists, ans: Answer) -> None:
    """ids equal and distance bits equal to the restatement"""
    assert np.array_equal(np.asarray(rows, np.uint64), ans.rows), (rows, ans.rows)
    assert np.array_equal(np.asarray(dists, f32).view(np.uint32), ans.dists.view(np.uint32)), (dists, ans.dists)
