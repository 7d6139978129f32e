"""Shared by tests/test_hnsw_modes.py, tests/test_gpu_hnsw.py and tests/test_gpu_hnsw_limits.py: the restatement of the HNSW rule block
(tests/hnsw_ref/hnsw_ref.c, distances through the oracle's lo_compute_distance), built here, the graphs the tests search (random ones,
and designed ones whose answers are written out by hand), and the comparisons of the GPU tests."""
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


def random_graph(rng, n, m, max_level=None, fill=0.8, p_up=None):
    """a random digraph with random valid levels: level-l lists name nodes of level >= l only, no node twice, pads at the end.
    fill = 1.0: every list is as long as it can be (2 m at level 0, min(m, the nodes of the level) above); p_up: P(level >= l + 1 |
    level >= l) when it is not 1 / m (m = 32 leaves too few upper nodes to fill a list of 32 otherwise)"""
    levels = np.minimum(rng.geometric(1.0 - (1.0 / m if p_up is None else p_up), n) - 1, 6).astype(np.uint32)
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
        deg = min(m, pool.size) if fill >= 1.0 else int(rng.integers(0, min(m, pool.size) + 1))
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


# ------------------------------------------------------------------------------------ designed graphs ----
# Each has its answer written out by hand (tests/test_hnsw_modes.py holds the restatement to it, tests/test_gpu_hnsw_limits.py the
# kernel).  All are 1-D, L2, query 0: the distance of row i is x[i]^2, exact in f32 for the values used.
class Designed:
    def __init__(self, name, x, g, k, ef, rows, dists, scored):
        self.name, self.data, self.g, self.k, self.ef = name, np.asarray(x, f32).reshape(-1, 1), g, k, ef
        self.query = np.zeros((1, 1), f32)
        self.rows, self.dists, self.scored = np.asarray(rows, np.uint64), np.asarray(dists, f32), scored


def made_graph(m, levels, lists0, upper=None, entry=0):
    """a graph from {node: [level-0 neighbours]} and {(node, level >= 1): [neighbours]}"""
    levels = np.asarray(levels, np.uint32)
    adj0 = np.full((levels.size, 2 * m), PAD, np.uint32)
    for i, nb in lists0.items():
        adj0[i, :len(nb)] = nb
    g = Graph(m, levels, adj0, None, entry)
    slot = {(int(a), int(b)): u for u, (a, b) in enumerate(zip(g.upper_node, g.upper_level))}
    g.upper_adj = np.full((g.upper_node.size, m), PAD, np.uint32)
    for key, nb in (upper or {}).items():
        g.upper_adj[slot[key], :len(nb)] = nb
    return g


def tie_bridge():
    """ef = k = 3.  From 0 (100): 1, 2 fill R; 3 evicts 0; 4, 5, 6 (all 5) evict 1, 2, 3: R = {4, 5, 6}, worst.dist 25; 7 (4) evicts 6 and
    8 (3) evicts 5 (the largest (dist, node) leaves).  C now holds the 8 admitted entries, more than 2 ef: scoring 9 needs room, and the
    compaction must keep 5 and 6, out of R but tied with worst.dist.  9 (50) is refused.  Pops: 8, 7, then 4, 5, 6 — 25 is not > 25, so
    each is expanded, and 6 names 10 (0), which evicts 4.  Dropping the ties instead answers [8, 7, 4]."""
    x = [100, 90, 89, 88, 5, 5, 5, 4, 3, 50, 0]
    g = made_graph(32, np.zeros(11), {0: list(range(1, 10)), 6: [10]})
    return Designed("tie bridge", x, g, 3, 3, [10, 8, 7], [0, 9, 16], 11)


FAN_EFS = (1, 2, 3, 7, 8, 9)


def fan(kind, ef):
    """k = ef.  The entry (100) names 64 nodes.  "descending": 64, 63, ..., 1 — every one is closer than all before it and is admitted,
    so with 2 ef + 8 slots every scoring step after the first compacts; the answer is the last ef of the list.  "ascending": 1, 2, ...,
    64 — the first ef are admitted (the last of them evicts the entry), then nothing is < worst.dist.  "ties": the 64 sit at exactly
    worst.dist when they are scored, so none is admitted: for ef = 1 the entry (7) names them (+-7); for ef >= 2 the entry (7, distance
    49, the worst of R from then on) names ef - 2 fillers (0.5, 1, ...) and a hub (6.5), which fill R, and the hub names the 64."""
    if kind == "descending":
        x = [100] + [65 - i for i in range(1, 65)]
        g = made_graph(32, np.zeros(65), {0: list(range(1, 65))})
        return Designed(f"descending fan, ef {ef}", x, g, ef, ef, [64 - i for i in range(ef)], [(i + 1) ** 2 for i in range(ef)], 65)
    if kind == "ascending":
        x = [100] + list(range(1, 65))
        g = made_graph(32, np.zeros(65), {0: list(range(1, 65))})
        return Designed(f"ascending fan, ef {ef}", x, g, ef, ef, list(range(1, ef + 1)), [i * i for i in range(1, ef + 1)], 65)
    assert kind == "ties"
    ties = [7 if i % 2 else -7 for i in range(64)]
    if ef == 1:
        g = made_graph(32, np.zeros(65), {0: list(range(1, 65))})
        return Designed("tie fan, ef 1", [7] + ties, g, 1, 1, [0], [49], 65)
    hub = ef - 1
    x = [7] + [0.5 * i for i in range(1, ef - 1)] + [6.5] + ties
    g = made_graph(32, np.zeros(ef + 64), {0: list(range(1, ef)), hub: list(range(ef, ef + 64))})
    return Designed(f"tie fan, ef {ef}", x, g, ef, ef, list(range(1, ef - 1)) + [hub, 0], [0.25 * i * i for i in range(1, ef - 1)] + [42.25, 49], ef + 64)


def path_graph(n, m=2):
    return flat_graph(n, m, {i: [j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)})


ALL_TIES = ((1, 1), (1, 50), (10, 10), (10, 50))   # (k, ef)


def all_ties(k, ef, n=600):
    """n copies of one row (3) on the path graph: R fills with 0 .. ef - 1, nothing after that is < worst.dist, nothing is ever beyond
    it either, so every admitted node is popped and expanded: node ef - 1 scores node ef, and the walk ends when C runs empty"""
    return Designed(f"all ties, k {k} ef {ef}", [3] * n, path_graph(n), k, ef, list(range(k)), [9] * k, ef + 1)


def descent(kind):
    """"slot 31": the entry's level-1 list holds 32 ids (four scoring steps of 8) and only the last is closer.  "equal": the list names
    a node at exactly the current distance (5 and -5): `<` keeps the current node, whose level-0 list leads to 2, not to 3.  "same
    list": slot 0 of 0's list moves cur to 1 (8), slot 1 (9) does not, slot 2 moves it to 3 (6) — the pass keeps scanning 0's list; the
    next pass scans 3's list (4, distance 25) and the one after 4's empty list; 5 (0.5) is named by 1's list only, which no pass scans.
    "level 52" ("level 53": the same with a level the load refuses): node j has level 52 - j and its list at level 51 - j names
    j + 1, so the descent takes one step per level from 0 to 51; 51's level-0 list names 52."""
    if kind == "slot 31":
        x = [10] + list(range(11, 42)) + [2, 1]
        g = made_graph(32, [1] * 33 + [0], {32: [33]}, {(0, 1): list(range(1, 33))})
        return Designed(kind, x, g, 2, 2, [33, 32], [1, 4], 1 + 32 + 1)
    if kind == "equal":
        g = made_graph(2, [1, 1, 0, 0], {0: [2], 1: [3]}, {(0, 1): [1]})
        return Designed(kind, [5, -5, 4, 1], g, 1, 1, [2], [16], 3)
    if kind == "same list":
        g = made_graph(4, [1] * 6, {}, {(0, 1): [1, 2, 3], (3, 1): [4], (1, 1): [5]})
        return Designed(kind, [10, 8, 9, 6, 5, 0.5], g, 1, 1, [4], [25], 1 + 3 + 1)
    assert kind in ("level 52", "level 53")
    levels = [52 - j for j in range(53)]
    if kind == "level 53":
        levels[0] = 53
    g = made_graph(2, levels, {51: [52]}, {(j, 51 - j): [j + 1] for j in range(51)})
    return Designed(kind, [60 - j for j in range(53)], g, 1, 1, [52], [64], 1 + 51 + 1)


VISITED_NS = (32, 33, 64, 65)


def visited_words(n):
    """k = ef = n over rows 1, 2, ..., n (row i at i + 1): the entry's one expansion names 31, 32, 63 and 64 (those the graph has) —
    two lanes on one bitmap word, and the last, partial word — and 1 and 31 name them again.  Every reachable node is scored once."""
    ok = lambda l: [r for r in l if r < n]
    lists = {0: ok([31, 32, 63, 64, 1]), 1: ok([31, 32, 0, 64]), 31: ok([63, 64, 30, 32, 0])}
    reach = sorted(set([0]) | set(sum(lists.values(), [])))
    g = made_graph(4, np.zeros(n), lists)
    return Designed(f"visited words, n {n}", [i + 1 for i in range(n)], g, n, n, reach, [(i + 1) ** 2 for i in reach], len(reach))


def designed_cases():
    out = [tie_bridge()]
    out += [fan(kind, ef) for kind in ("descending", "ascending", "ties") for ef in FAN_EFS]
    out += [all_ties(k, ef) for k, ef in ALL_TIES]
    out += [descent(kind) for kind in ("slot 31", "equal", "same list", "level 52")]
    out += [visited_words(n) for n in VISITED_NS]
    return out


# ------------------------------------------------------------------------------ the GPU comparisons ----
IP, L2, COS = 0, 1, 2
NAME = {IP: "ip", L2: "l2", COS: "cosine"}


def make_data(kind, rng, n, dim, nq):
    if kind == "gauss":
        return rng.standard_normal((n, dim)).astype(f32), rng.standard_normal((nq, dim)).astype(f32)
    if kind == "int":   # integer-valued rows: exact ties and exact zeros
        return rng.integers(-3, 4, (n, dim)).astype(f32), rng.integers(-3, 4, (nq, dim)).astype(f32)
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


def load(idx, g, metric, ef_search=50):
    idx.load_hnsw(metric, g.m, ef_search, g.levels, g.adj0, g.upper_node, g.upper_level, g.upper_adj, g.entry)


def check(got, exp, k, metric, what):
    rows, dists, counts = got
    worst = -np.inf if metric == IP else np.inf
    for qi, (e_rows, e_d) in enumerate(exp):
        c = int(counts[qi])
        assert c == e_rows.size, (what, qi, c, e_rows.size)
        assert np.array_equal(rows[qi, :c], e_rows), (what, qi, rows[qi, :c], e_rows)
        assert np.array_equal(dists[qi, :c].view(np.uint32), e_d.view(np.uint32)), (what, qi, dists[qi, :c], e_d)
        assert (rows[qi, c:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (dists[qi, c:] == worst).all(), (what, qi)


def sweep(idx, ref, data, g, metric, queries, combos, ef_search=50):
    """combos: (k, ef_query, nq); ef_query 0 = the index's ef_search"""
    load(idx, g, metric, ef_search)
    n = data.shape[0]
    for k, efq, nq in combos:
        q = queries[np.arange(nq) % queries.shape[0]]
        ef = max(efq if efq else ef_search, k)
        exp = ref_search(ref, data[:n], metric, g, q, k, ef)
        check(idx.search_hnsw_batch_arrays(q, k, metric, efq), exp, k, metric, (NAME[metric], n, g.m, k, efq, nq))


def combos_for(n):
    """k in {1, 10, ef, N + 3}, ef in {k, 50 (the index's), N + 5}, nq in {1, 5, 300}"""
    return [(1, 1, 5), (10, 10, 300), (10, 0, 5), (50, 0, 1), (n + 3, n + 3, 5), (10, n + 5, 5), (n + 3, n + 5, 1), (n + 5, n + 5, 5), (1, n + 5, 1)]


def assert_same_graph(p, g, what):
    assert np.array_equal(p["levels"], g.levels), what
    assert p["entry"] == g.entry and p["top_level"] == int(g.levels.max()), what
    assert np.array_equal(p["upper_node"], g.upper_node) and np.array_equal(p["upper_level"], g.upper_level), what
    bad = np.nonzero((p["adj0"] != g.adj0).any(axis=1))[0]
    assert bad.size == 0, (what, "level 0", bad[:5], p["adj0"][bad[:2]], g.adj0[bad[:2]])
    bad = np.nonzero((p["upper_adj"] != g.upper_adj).any(axis=1))[0]
    assert bad.size == 0, (what, "upper", bad[:5])


def scored_sweep(idx, ref, data, g, metric, queries, combos, ef_search=50):
    """sweep over the graph the handle holds (g, built or loaded by the caller), and the one observable of the walk itself: with
    profiling on, the distances a batch scored (hnsw_stage_times) equal the sum of the restatement's per-query counts"""
    idx.profile_enable(True)
    try:
        for k, efq, nq in combos:
            q = queries[np.arange(nq) % queries.shape[0]]
            sc = []
            exp = ref_search(ref, data, metric, g, q, k, max(efq if efq else ef_search, k), scored=sc)
            idx.hnsw_stage_times(reset=True)
            got = idx.search_hnsw_batch_arrays(q, k, metric, efq)
            t = idx.hnsw_stage_times(reset=True)
            check(got, exp, k, metric, (NAME[metric], data.shape[0], g.m, k, efq, nq))
            assert (t["searches"], t["scored"]) == (1, sum(sc)), (NAME[metric], data.shape[0], g.m, k, efq, nq, t["scored"], sum(sc))
    finally:
        idx.profile_enable(False)
