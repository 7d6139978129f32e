"""Shared by tests/test_hnsw_modes.py and tests/test_gpu_hnsw.py: the restatement of the HNSW rule block (tests/hnsw_ref/hnsw_ref.c,
distances through the oracle's lo_compute_distance), built here, and the graphs the tests search."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
_vp = C.c_void_p
PAD = 0xFFFFFFFF
M64 = (1 << 64) - 1
f32 = np.float32


def _p(a):
    return a.ctypes.data_as(_vp)


def build_ref(tmp_dir, oracle):
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no C compiler for tests/hnsw_ref/hnsw_ref.c"
    so = Path(tmp_dir) / "libhnsw_ref.so"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-o", str(so), str(HERE / "hnsw_ref" / "hnsw_ref.c"), "-lm"],
                   check=True)
    lib = C.CDLL(str(so))
    lib.hr_levels.argtypes = [C.c_uint64, C.c_uint32, C.c_int32, C.c_size_t, _vp]
    lib.hr_levels.restype = None
    lib.hr_build.argtypes = [_vp, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp]
    lib.hr_build.restype = C.c_uint32
    lib.hr_search.argtypes = [_vp, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32, _vp, _vp, _vp, C.c_uint32, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp]
    lib.hr_search.restype = C.c_size_t
    return lib, C.cast(oracle.lib.lo_compute_distance, _vp)


def levels_py(seed, m, max_level, n):
    """rule 1 in Python integers: the i-th next_u64 of SmallRng::seed_from_u64(seed) -> level i"""
    s, st = [], seed
    for _ in range(4):
        st = (st + 0x9E3779B97F4A7C15) & M64
        z = st
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        s.append(z ^ (z >> 31))
    rotl = lambda x, k: ((x << k) | (x >> (64 - k))) & M64
    out = []
    for _ in range(n):
        w = (rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64
        t17 = (s[1] << 17) & M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t17
        s[3] = rotl(s[3], 45)
        t, level = max(w >> 11, 1), 0
        while (max_level is None or level < max_level) and t * m < (1 << 53):
            t *= m
            level += 1
        out.append(level)
    return np.array(out, np.uint32)


def ref_levels(ref, seed, m, max_level, n):
    out = np.zeros(max(n, 1), np.uint32)
    ref[0].hr_levels(seed, m, -1 if max_level is None else max_level, n, _p(out))
    return out[:n]


def upper_layout(levels):
    """(upper_node, upper_level): one entry per (node, level >= 1), ascending"""
    node = np.repeat(np.arange(levels.size, dtype=np.uint32), levels.astype(np.int64))
    level = np.concatenate([np.arange(1, int(l) + 1, dtype=np.uint32) for l in levels]) if levels.sum() else np.zeros(0, np.uint32)
    return node, level.astype(np.uint32)


class Graph:
    def __init__(self, m, levels, adj0, upper_adj, entry):
        self.m, self.levels, self.adj0, self.upper_adj, self.entry = int(m), levels, adj0, upper_adj, int(entry)
        self.upper_node, self.upper_level = upper_layout(levels)


def ref_build(ref, data, metric, m, ef_construction, levels):
    lib, dist = ref
    data = np.ascontiguousarray(data, f32)
    n, dim = data.shape
    levels = np.ascontiguousarray(levels, np.uint32)
    adj0 = np.zeros((n, 2 * m), np.uint32)
    upper = np.zeros((int(levels.sum()), m), np.uint32)
    entry = lib.hr_build(_p(data), n, dim, metric, m, ef_construction, _p(levels), dist, _p(adj0), _p(upper))
    return Graph(m, levels, adj0, upper, entry)


def ref_search(ref, data, metric, g, queries, k, ef, scored=None):
    """per query (rows u64, distances f32); ef is the caller's max(ef, k)"""
    lib, dist = ref
    data = np.ascontiguousarray(data, f32)
    n, dim = data.shape
    lv, a0, ua = (np.ascontiguousarray(x, np.uint32) for x in (g.levels, g.adj0, g.upper_adj))
    if ua.size == 0:
        ua = np.zeros((1, g.m), np.uint32)
    out = []
    for q in np.ascontiguousarray(queries, f32):
        rows, d, sc = np.zeros(max(k, 1), np.uint64), np.zeros(max(k, 1), f32), np.zeros(1, np.uint64)
        c = lib.hr_search(_p(data), n, dim, metric, g.m, _p(lv), _p(a0), _p(ua), g.entry, _p(np.ascontiguousarray(q)), k, ef, dist, _p(rows), _p(d), _p(sc))
        out.append((rows[:c].copy(), d[:c].copy()))
        if scored is not None:
            scored.append(int(sc[0]))
    return out


def random_graph(rng, n, m, max_level=None, fill=0.8):
    """a random digraph with random valid levels: level-l lists name nodes of level >= l only, no node twice, pads at the end"""
    levels = np.minimum(rng.geometric(1.0 - 1.0 / m, n) - 1, 6).astype(np.uint32)
    if max_level is not None:
        levels = np.minimum(levels, max_level).astype(np.uint32)
    top = int(levels.max())
    entry = int(np.nonzero(levels == top)[0][0])
    adj0 = np.full((n, 2 * m), PAD, np.uint32)
    for i in range(n):
        deg = int(rng.integers(0, min(2 * m, n) + 1)) if rng.random() > fill else min(2 * m, n)
        adj0[i, :deg] = rng.choice(n, deg, replace=False)
    un, ul = upper_layout(levels)
    upper = np.full((un.size, m), PAD, np.uint32)
    for u in range(un.size):
        pool = np.nonzero(levels >= ul[u])[0]
        deg = int(rng.integers(0, min(m, pool.size) + 1))
        upper[u, :deg] = rng.choice(pool, deg, replace=False)
    return Graph(m, levels, adj0, upper, entry)


def flat_graph(n, m, lists):
    """a one-level graph from {node: [neighbours]}"""
    adj0 = np.full((n, 2 * m), PAD, np.uint32)
    for i, nb in lists.items():
        adj0[i, :len(nb)] = nb
    return Graph(m, np.zeros(n, np.uint32), adj0, np.zeros((0, m), np.uint32), 0)


def clustered(seed, n, dim, n_clusters, spread, nq):
    """Gaussian clusters: centres standard normal, points centre + spread * normal -> (data, queries)"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((n_clusters, dim))
    data = cen[rng.integers(0, n_clusters, n)] + spread * rng.standard_normal((n, dim))
    queries = cen[rng.integers(0, n_clusters, nq)] + spread * rng.standard_normal((nq, dim))
    return data.astype(f32), queries.astype(f32)


_recall = {}


def recall_case(ref):
    """the recall case of the issue, computed once per process: 4096 x 32 f32, 32 clusters of spread 0.15, L2, m = 16, ef_construction = 128,
    ef = 50, k = 10, 100 queries -> (data, queries, graph, results, distances scored)"""
    if not _recall:
        data, queries = clustered(1, 4096, 32, 32, 0.15, 100)
        g = ref_build(ref, data, 1, 16, 128, ref_levels(ref, 42, 16, None, 4096))
        scored = []
        _recall["v"] = (data, queries, g, ref_search(ref, data, 1, g, queries, 10, 50, scored=scored), scored)
    return _recall["v"]
