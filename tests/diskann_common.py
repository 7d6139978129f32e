"""Shared by tests/test_diskann_modes.py and tests/test_gpu_diskann.py: the restatement of the DiskANN rule block
(tests/diskann_ref/diskann_ref.c, distances through the oracle's lo_compute_distance), built here, the Python big-integer model of
rule 1, the designed inputs and the comparisons of the GPU tests."""
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
L2, COS = 1, 2
NAME = {L2: "l2", COS: "cosine"}
QUERY_ANCHORS = 8


def _p(a):
    return a.ctypes.data_as(_vp)


def build_ref(tmp_dir, oracle):
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no C compiler for tests/diskann_ref/diskann_ref.c"
    so = Path(tmp_dir) / "libdiskann_ref.so"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-o", str(so), str(HERE / "diskann_ref" / "diskann_ref.c"),
                    "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.dr_draws.argtypes = [C.c_uint64, C.c_size_t, C.c_uint32, _vp, _vp, _vp, _vp]
    lib.dr_draws.restype = None
    lib.dr_starts.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, _vp]
    lib.dr_starts.restype = C.c_size_t
    lib.dr_prune.argtypes = [_vp, C.c_size_t, C.c_int, _vp, C.c_uint32, _vp, _vp, C.c_size_t, C.c_uint32, C.c_float, _vp]
    lib.dr_prune.restype = C.c_size_t
    lib.dr_search.argtypes = [_vp, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32, _vp, C.c_uint32, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _vp]
    lib.dr_search.restype = C.c_size_t
    lib.dr_build.argtypes = [_vp, C.c_size_t, C.c_size_t, C.c_int, C.c_uint32, C.c_uint32, C.c_float, C.c_uint64, C.c_uint64, _vp, _vp, _vp]
    lib.dr_build.restype = C.c_uint32
    return lib, C.cast(oracle.lib.lo_compute_distance, _vp)


# ------------------------------------------------------------------------------------------ rule 1 ----
def words_py(seed):
    """the next_u64 stream of SmallRng::seed_from_u64(seed) in Python integers"""
    s, st = [], seed
    for _ in range(4):
        st = (st + 0x9E3779B97F4A7C15) & M64
        z = st
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        s.append(z ^ (z >> 31))
    rotl = lambda x, k: ((x << k) | (x >> (64 - k))) & M64
    while True:
        w = (rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64
        t17 = (s[1] << 17) & M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t17
        s[3] = rotl(s[3], 45)
        yield w


def draws_py(seed, n, r):
    """rule 1-4 without the rows -> (refs, cands, order before the entry swap, adj0 [n][r])"""
    adj0 = np.full((n, r), PAD, np.uint32)
    if n <= 1:
        z = np.zeros(n, np.uint32)
        return z, z.copy(), z.copy(), adj0
    w = words_py(seed)
    draw = lambda b: ((next(w) >> 32) * b) >> 32

    def shuffle():
        a = list(range(n))
        for i in range(n - 1, 0, -1):
            j = draw(i + 1)
            a[i], a[j] = a[j], a[i]
        return a

    refs, cands = shuffle()[:32], shuffle()[:64]
    for i in range(n):
        row = []
        while len(row) < min(r, n - 1):
            j = draw(n)
            if j != i and j not in row:
                row.append(j)
        adj0[i, :len(row)] = row
    return np.array(refs, np.uint32), np.array(cands, np.uint32), np.array(shuffle(), np.uint32), adj0


def draws_of(fn, seed, n, r):
    """the same four arrays from a C function with dr_draws' arguments"""
    refs, cands = np.zeros(max(min(32, n), 1), np.uint32), np.zeros(max(min(64, n), 1), np.uint32)
    order, adj0 = np.zeros(max(n, 1), np.uint32), np.zeros((max(n, 1), r), np.uint32)
    rc = fn(seed, n, r, _p(refs), _p(cands), _p(order), _p(adj0))
    assert not rc, rc
    return refs[:min(32, n)], cands[:min(64, n)], order[:n], adj0[:n]


def starts_py(n, entry, anchors):
    a = min(anchors, n)
    return [entry] + [x for x in (i * n // a for i in range(a)) if x != entry]


def ref_starts(ref, n, entry, anchors):
    out = np.zeros(64, np.uint32)
    c = ref[0].dr_starts(n, entry, anchors, _p(out))
    return out[:c].tolist()


# ------------------------------------------------------------------------------- the restatement ----
class Graph:
    def __init__(self, r, l, adj, entry, longest=0):
        self.r, self.l, self.adj, self.entry, self.longest = int(r), max(int(l), int(r)), np.ascontiguousarray(adj, np.uint32), int(entry), int(longest)


def ref_prune(ref, data, metric, p, cand_d, cand_n, r, alpha):
    lib, dist = ref
    data = np.ascontiguousarray(data, f32)
    cd, cn = np.ascontiguousarray(cand_d, f32), np.ascontiguousarray(cand_n, np.uint32)
    out = np.zeros(max(r, 1), np.uint32)
    c = lib.dr_prune(_p(data), data.shape[1], metric, dist, p, _p(cd), _p(cn), cn.size, r, alpha, _p(out))
    return out[:c].tolist()


def ref_build(ref, data, metric, r, l, alpha, seed=42, max_batches=0):
    lib, dist = ref
    data = np.ascontiguousarray(data, f32)
    n, dim = data.shape
    adj, longest = np.zeros((n, r), np.uint32), np.zeros(1, np.uint32)
    entry = lib.dr_build(_p(data), n, dim, metric, r, l, alpha, seed, max_batches, dist, _p(adj), _p(longest))
    return Graph(r, l, adj, entry, longest[0])


def query_ef(g, n, k, ef_query):
    """rule 8"""
    return min(max(ef_query, g.l, 10 * k), n)


def ref_search(ref, data, metric, g, queries, k, ef, anchors=QUERY_ANCHORS, scored=None):
    """per query (rows u64, distances f32); ef as search_graph takes it"""
    lib, dist = ref
    data = np.ascontiguousarray(data, f32)
    n, dim = data.shape
    out = []
    for q in np.ascontiguousarray(queries, f32):
        rows, d, sc = np.zeros(max(k, 1), np.uint64), np.zeros(max(k, 1), f32), np.zeros(1, np.uint64)
        c = lib.dr_search(_p(data), n, dim, metric, g.r, _p(g.adj), g.entry, _p(np.ascontiguousarray(q)), k, ef, anchors, dist, _p(rows), _p(d), _p(sc))
        out.append((rows[:c].copy(), d[:c].copy()))
        if scored is not None:
            scored.append(int(sc[0]))
    return out


def made_graph(n, r, lists, entry=0, l=1):
    adj = np.full((n, r), PAD, np.uint32)
    for i, nb in lists.items():
        adj[i, :len(nb)] = nb
    return Graph(r, l, adj, entry)


def random_graph(rng, n, r, fill=0.8, l=1):
    adj = np.full((n, r), PAD, np.uint32)
    for i in range(n):
        deg = int(rng.integers(0, min(r, n) + 1)) if rng.random() > fill else min(r, n)
        adj[i, :deg] = rng.choice(n, deg, replace=False)
    return Graph(r, l, adj, int(rng.integers(0, n)))


def clustered(seed, n, dim, n_clusters, spread, nq):
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((n_clusters, dim))
    data = cen[rng.integers(0, n_clusters, n)] + spread * rng.standard_normal((n, dim))
    queries = cen[rng.integers(0, n_clusters, nq)] + spread * rng.standard_normal((nq, dim))
    return data.astype(f32), queries.astype(f32)


_recall = {}


def recall_case(ref):
    """the recall case, computed once per process: 4096 x 32 f32, 32 clusters of spread 0.15 (the data of hnsw_common.recall_case), L2,
    the defaults r = 16, l = 64, alpha = 1.2, seed 42, k = 10, 100 queries -> (data, queries, graph, results)"""
    if not _recall:
        data, queries = clustered(1, 4096, 32, 32, 0.15, 100)
        g = ref_build(ref, data, L2, 16, 64, 1.2)
        _recall["v"] = (data, queries, g, ref_search(ref, data, L2, g, queries, 10, query_ef(g, 4096, 10, 0)))
    return _recall["v"]


def make_data(kind, rng, n, dim, nq):
    if kind == "gauss":
        return rng.standard_normal((n, dim)).astype(f32), rng.standard_normal((nq, dim)).astype(f32)
    if kind == "dup":   # rows drawn from 40 distinct vectors: ties everywhere
        base = rng.standard_normal((40, dim)).astype(f32)
        return base[rng.integers(0, 40, n)], base[rng.integers(0, 40, nq)]
    assert kind == "nonfinite"
    data, q = rng.standard_normal((n, dim)).astype(f32), rng.standard_normal((nq, dim)).astype(f32)
    for a in (data, q):
        r = a.shape[0]
        a[rng.integers(0, r, max(1, r // 7)), rng.integers(0, dim, max(1, r // 7))] = np.nan
        a[rng.integers(0, r, max(1, r // 9)), rng.integers(0, dim, max(1, r // 9))] = np.inf
        a[rng.integers(0, r, max(1, r // 9)), rng.integers(0, dim, max(1, r // 9))] = -np.inf
    return data, q


def hub_data(seed=7, n=520, dim=32):
    """row 0 at the origin, the others random unit vectors: row 0 is every row's nearest (1 against about 2)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x[0] = 0.0
    return x.astype(f32)


def fan_graph(ef=10):
    """A fan of 64 neighbours all at worst.dist behind a full R (1-D, L2, query 0, k = 1, the graph's l = ef = 10 so rule 8 gives 10).
    Rows: the entry 0 at 7 (distance 49), fillers 1 .. 8 at 0.5 i, the hub 9 at 6.5, then 64 rows at +-7 (n = 74).  Starts: 0, then the
    anchors 9, 18, 27, 37, 46, 55, 64 (anchor 0 is the entry): 8 entries, R not full.  Pop 9 (42.25): 10 and 11 (49) fill R, the other
    fan rows sit at exactly worst.dist and are refused.  The pops that follow are the ties at 49 in node order; 0 comes first and names
    1 .. 8, which evict eight of the ties.  The answer for k = 1 is row 1 at 0.25; 74 distances are scored.  Returns (data, graph, n)."""
    n = ef + 64
    x = [7.0] + [0.5 * i for i in range(1, ef - 1)] + [6.5] + [7.0 if i % 2 else -7.0 for i in range(64)]
    g = made_graph(n, 64, {0: list(range(1, ef)), ef - 1: list(range(ef, ef + 64))}, entry=0, l=ef)
    return np.asarray(x, f32).reshape(-1, 1), g, n


# ------------------------------------------------------------------------------ the GPU comparisons ----
def load(idx, g, metric):
    idx.load_diskann(metric, g.r, g.l, g.adj, g.entry)


def check(got, exp, what):
    rows, dists, counts = got
    for qi, (e_rows, e_d) in enumerate(exp):
        c = int(counts[qi])
        assert c == e_rows.size, (what, qi, c, e_rows.size)
        assert np.array_equal(rows[qi, :c], e_rows), (what, qi, rows[qi, :c], e_rows)
        assert np.array_equal(dists[qi, :c].view(np.uint32), e_d.view(np.uint32)), (what, qi, dists[qi, :c], e_d)
        assert (rows[qi, c:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (dists[qi, c:] == np.inf).all(), (what, qi)


def sweep(idx, ref, data, g, metric, queries, combos):
    """combos: (k, ef_query, nq) over the graph loaded here; with profiling on the distances scored equal the restatement's"""
    load(idx, g, metric)
    n = data.shape[0]
    idx.profile_enable(True)
    try:
        for k, efq, nq in combos:
            q = queries[np.arange(nq) % queries.shape[0]]
            sc = []
            exp = ref_search(ref, data, metric, g, q, k, query_ef(g, n, k, efq), scored=sc)
            idx.diskann_stage_times(reset=True)
            got = idx.search_diskann_batch_arrays(q, k, metric, efq)
            t = idx.diskann_stage_times(reset=True)
            check(got, exp, (NAME[metric], n, g.r, k, efq, nq))
            assert (t["searches"], t["scored"]) == (1, sum(sc)), (NAME[metric], n, g.r, k, efq, nq, t["scored"], sum(sc))
    finally:
        idx.profile_enable(False)


def assert_same_graph(p, g, what):
    assert p["entry"] == g.entry and p["r"] == g.r and p["n"] == g.adj.shape[0], (what, p["entry"], g.entry)
    bad = np.nonzero((p["adj"] != g.adj).any(axis=1))[0]
    assert bad.size == 0, (what, bad.size, bad[:5], p["adj"][bad[:2]], g.adj[bad[:2]])
