"""Shared by the tests that compare against the restatement of the additive metrics (tests/additive_ref/additive_ref.c: plain C, eight
explicit lanes; checked on its own in tests/test_additive_metric_modes.py): the compiled library and its two entry points.
TEST INFRASTRUCTURE."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np

from conftest import oracle_for_every_query

HERE = Path(__file__).resolve().parent
f32 = np.float32
_vp = C.c_void_p
L1, CHEB, CANB, BRAY = 7, 8, 9, 10
NAME = {L1: "l1", CHEB: "chebyshev", CANB: "canberra", BRAY: "bray_curtis"}


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def dist(self, m, a, b):
        a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
        return np.float32(self.lib.add_dist(m, a.ctypes.data_as(_vp), b.ctypes.data_as(_vp), a.size))

    def raw_dists(self, m, queries, data):
        """[nq, n] distances as add_dists computes them (a NaN stays a NaN: the range search never passes it)"""
        queries, data = np.ascontiguousarray(queries, f32), np.ascontiguousarray(data, f32)
        out = np.empty((queries.shape[0], data.shape[0]), f32)

        def one(i):
            self.lib.add_dists(m, queries[i].ctypes.data_as(_vp), data.ctypes.data_as(_vp), data.shape[0], data.shape[1],
                               out[i].ctypes.data_as(_vp))

        oracle_for_every_query(one, queries.shape[0])
        return out

    def dists(self, m, queries, data):
        """[nq, n] distances as the searches report them: a NaN is +inf"""
        out = self.raw_dists(m, queries, data)
        out[np.isnan(out)] = np.inf
        return out


def build_ref(tmp_dir) -> Ref:
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no C compiler for tests/additive_ref/additive_ref.c"
    so = Path(tmp_dir) / "libadditive_ref.so"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-o", str(so),
                    str(HERE / "additive_ref" / "additive_ref.c"), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.add_dist.restype = C.c_float
    lib.add_dist.argtypes = [C.c_int, _vp, _vp, C.c_size_t]
    lib.add_dists.restype = None
    lib.add_dists.argtypes = [C.c_int, _vp, _vp, C.c_size_t, C.c_size_t, _vp]
    return Ref(lib)
