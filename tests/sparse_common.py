"""Shared by tests/test_sparse_modes.py and tests/test_gpu_sparse_search.py: the compiled restatement (tests/sparse_ref/sparse_ref.c), the
data generator of the sparse tests and the expected result of a search.  TEST INFRASTRUCTURE."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np

from conftest import oracle_for_every_query

HERE = Path(__file__).resolve().parent
f32, u32, u64 = np.float32, np.uint32, np.uint64
_vp = C.c_void_p


def _p(a):
    return a.ctypes.data_as(_vp)


class Csr:
    """n sparse vectors: indptr u64[n + 1], indices u32, values f32"""

    def __init__(self, indptr, indices, values):
        self.indptr = np.ascontiguousarray(indptr, u64)
        self.indices = np.ascontiguousarray(indices, u32)
        self.values = np.ascontiguousarray(values, f32)
        assert int(self.indptr[-1]) == self.indices.size == self.values.size

    @staticmethod
    def of(vectors):
        """[(indices, values) | {index: value}] -> Csr, entries as given"""
        vs = [(list(v.keys()), list(v.values())) if isinstance(v, dict) else v for v in vectors]
        ptr = np.zeros(len(vs) + 1, u64)
        ptr[1:] = np.cumsum([len(v[0]) for v in vs])
        idx = np.concatenate([np.asarray(v[0], u32) for v in vs]) if vs else np.zeros(0, u32)
        val = np.concatenate([np.asarray(v[1], f32) for v in vs]) if vs else np.zeros(0, f32)
        return Csr(ptr, idx, val)

    def __len__(self):
        return self.indptr.size - 1

    def row(self, i):
        a, b = int(self.indptr[i]), int(self.indptr[i + 1])
        return self.indices[a:b], self.values[a:b]

    def head(self, n):
        e = int(self.indptr[n])
        return Csr(self.indptr[:n + 1], self.indices[:e], self.values[:e])

    def arrays(self):
        return self.indptr, self.indices, self.values


class Ref:
    def __init__(self, lib):
        self.lib = lib

    def normalize(self, indices, values):
        """-> (indices, values), or None for a non-finite value"""
        idx, val = np.ascontiguousarray(indices, u32), np.ascontiguousarray(values, f32)
        o_i, o_v = np.zeros(max(idx.size, 1), u32), np.zeros(max(idx.size, 1), f32)
        m = self.lib.sr_normalize(_p(idx), _p(val), idx.size, _p(o_i), _p(o_v))
        return None if m < 0 else (o_i[:m].copy(), o_v[:m].copy())

    def ip(self, q, v, reversed_=False):
        qi, qv = np.ascontiguousarray(q[0], u32), np.ascontiguousarray(q[1], f32)
        vi, vv = np.ascontiguousarray(v[0], u32), np.ascontiguousarray(v[1], f32)
        fn = self.lib.sr_ip_reversed if reversed_ else self.lib.sr_ip
        return f32(fn(_p(qi), _p(qv), qi.size, _p(vi), _p(vv), vi.size))

    def scores(self, queries: Csr, rows: Csr, reversed_=False):
        """[nq, n] scores of every (query, row), the queries threaded"""
        out = np.empty((len(queries), len(rows)), f32)

        def one(i):
            qi, qv = queries.row(i)
            self.lib.sr_scores(_p(qi), _p(qv), qi.size, _p(rows.indptr), _p(rows.indices), _p(rows.values), len(rows), int(reversed_), _p(out[i]))

        oracle_for_every_query(one, len(queries))
        return out


def build_ref(tmp_dir) -> Ref:
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no C compiler for tests/sparse_ref/sparse_ref.c"
    so = Path(tmp_dir) / "libsparse_ref.so"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-o", str(so),
                    str(HERE / "sparse_ref" / "sparse_ref.c"), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.sr_normalize.restype = C.c_long
    lib.sr_normalize.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp]
    for fn in (lib.sr_ip, lib.sr_ip_reversed):
        fn.restype = C.c_float
        fn.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t]
    lib.sr_scores.restype = None
    lib.sr_scores.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp, _vp, C.c_size_t, C.c_int, _vp]
    return Ref(lib)


def gen_values(rng, m):
    """N(0, 1) * 2^e, e a uniform integer in [-12, 12], as f32; exact zeros become 1"""
    v = (rng.standard_normal(m) * np.exp2(rng.integers(-12, 13, m))).astype(f32)
    v[v == 0] = 1
    return v


def gen_vectors(rng, n, vocab, lo, hi) -> Csr:
    """row length uniform in [lo, hi], indices a sorted sample without replacement from range(vocab)"""
    lens = rng.integers(lo, hi + 1, n)
    ptr = np.zeros(n + 1, u64)
    ptr[1:] = np.cumsum(lens)
    idx = np.empty(int(ptr[-1]), u32)
    for r in range(n):
        idx[int(ptr[r]):int(ptr[r + 1])] = np.sort(rng.choice(vocab, int(lens[r]), replace=False))
    return Csr(ptr, idx, gen_values(rng, idx.size))


CONFIGS = {"A": (200, 1, 80, 30), "B": (1000, 1, 300, 64), "C": (30522, 20, 200, 40)}   # vocab, row length lo..hi, query nnz


def order_of(scores, live=None):
    """the rows of one query's results in result order: score != 0 (NaN passes), by (score descending with NaN as -inf, row)"""
    keep = scores != 0
    if live is not None:
        keep &= live
    rows = np.nonzero(keep)[0]
    s = scores[rows].astype(np.float64)
    s[np.isnan(s)] = -np.inf
    return rows[np.lexsort((rows, -s))]


def reported(scores, rows):
    s = scores[rows].copy()
    s[np.isnan(s)] = -np.inf
    return s


def check_batch(got, smat, k, live=None, what=None, orders=None):
    rows, scores, counts, passed = got
    assert rows.shape == (smat.shape[0], k) and scores.shape == (smat.shape[0], k)
    for qi in range(smat.shape[0]):
        order = orders[qi] if orders is not None else order_of(smat[qi], live)
        e_r = order[:k].astype(u64)
        e_s = reported(smat[qi], order[:k])
        c = int(counts[qi])
        assert int(passed[qi]) == order.size, (what, qi, int(passed[qi]), order.size)
        assert c == e_r.size, (what, qi, c, e_r.size)
        assert np.array_equal(rows[qi, :c], e_r), (what, qi, rows[qi, :c][:12], e_r[:12])
        assert np.array_equal(scores[qi, :c].view(u32), e_s.view(u32)), (what, qi, scores[qi, :c][:12], e_s[:12])
        assert np.all(rows[qi, c:] == u64(0xFFFFFFFFFFFFFFFF)) and np.all(np.isneginf(scores[qi, c:])), (what, qi)
