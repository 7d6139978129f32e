"""HNSW-{IP,L2,COS} on the CPU: mode and option parsing, the integer level rule (lynse_hip_hnsw_levels against a Python restatement), and
the restatement the GPU tests compare against (tests/hnsw_ref/hnsw_ref.c) checked on its own: hand-made graphs with answers written out
by hand, and its recall against the exact search.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import hnsw_common as H
import oracle as O
from lynsedb_amd import _lib
from lynsedb_amd.core import HNSW_DEFAULTS, HNSW_SEED, hnsw_build_options, hnsw_mode_of

f32 = np.float32


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return H.build_ref(tmp_path_factory.mktemp("hnsw_ref"), oracle)


# ---- modes and options ------------------------------------------------------------------------------------------------------------
def test_modes():
    for mode, metric in (("HNSW-IP", _lib.METRIC_IP), ("HNSW-L2", _lib.METRIC_L2), ("HNSW-COS", _lib.METRIC_COSINE),
                         ("HNSW-COSINE", _lib.METRIC_COSINE), ("hnsw-l2", _lib.METRIC_L2), ("Hnsw-Cosine", _lib.METRIC_COSINE)):
        assert hnsw_mode_of(mode) == metric
    for mode in ("HNSW-IP-SQ8", "HNSW-L2-SQ8", "HNSW-COS-PQ", "DISKANN-IP", "HNSW", "HNSW-HAMMING", "HNSW-L1", "FLAT-IP", "IVF-L2", "HNSW-CORRELATION"):
        assert hnsw_mode_of(mode) is None


def test_build_options():
    assert HNSW_DEFAULTS == {"m": 16, "ef_construction": 128, "ef_search": 50} and HNSW_SEED == 42
    assert hnsw_build_options(None) == {"m": 16, "ef_construction": 128, "ef_search": 50, "max_level": None}
    assert hnsw_build_options({"m": 4, "ef_construction": 32, "ef_search": 7, "max_level": 2}) == {"m": 4, "ef_construction": 32, "ef_search": 7, "max_level": 2}
    # keys of the other index families are ignored, None means the default
    assert hnsw_build_options({"n_clusters": 9, "nprobe": 3, "alpha": 1.2, "m": None})["m"] == 16
    for name in ("m", "ef_construction", "ef_search", "n_clusters", "nprobe"):
        with pytest.raises(ValueError, match=f"Invalid argument: {name} must be greater than 0"):
            hnsw_build_options({name: 0})
    with pytest.raises(ValueError, match="unknown index build parameter 'ef'; supported keys: n_clusters, n_centroids, m, ef_construction"):
        hnsw_build_options({"ef": 10})
    assert hnsw_build_options({"max_level": 0})["max_level"] == 0   # (a cap of 0 is a one-level graph, not "greater than 0")


# ---- rule 1 -----------------------------------------------------------------------------------------------------------------------
def lib_levels(seed, m, max_level, n):
    out = np.zeros(max(n, 1), np.uint32)
    assert _lib.lib.lynse_hip_hnsw_levels(seed, m, -1 if max_level is None else max_level, n, out.ctypes.data_as(C.c_void_p)) == 0
    return out[:n]


@pytest.mark.parametrize("seed,m,max_level,n", [(42, 16, None, 3000), (42, 2, None, 500), (7, 4, None, 700), (0, 32, None, 2000), (42, 2, 3, 500),
                                                (42, 4, 0, 50), (1, 3, 1, 300)])
def test_levels_against_python_and_the_restatement(ref, seed, m, max_level, n):
    exp = H.levels_py(seed, m, max_level, n)
    assert np.array_equal(lib_levels(seed, m, max_level, n), exp)
    assert np.array_equal(H.ref_levels(ref, seed, m, max_level, n), exp)
    if max_level is not None:
        assert int(exp.max()) <= max_level


def test_levels_known_answers_and_edges():
    # w >> 11 is 53 bits: the level is how often it can be multiplied by m and stay below 2^53
    def level(t, m):
        l = 0
        while t * m < (1 << 53):
            t, l = t * m, l + 1
        return l
    assert [level(t, 2) for t in (1, (1 << 52) - 1, 1 << 52, (1 << 53) - 1)] == [52, 1, 0, 0]
    assert [level(t, 16) for t in (1, (1 << 49) - 1, 1 << 49)] == [13, 1, 0]
    a = lib_levels(42, 16, None, 64)
    assert np.array_equal(a, lib_levels(42, 16, None, 64))          # deterministic
    assert np.array_equal(a[:10], lib_levels(42, 16, None, 10))     # a prefix: level i does not depend on n
    assert not np.array_equal(a, lib_levels(43, 16, None, 64))
    assert lib_levels(42, 16, None, 0).size == 0
    assert _lib.lib.lynse_hip_hnsw_levels(42, 16, -1, 3, None) == _lib.ERR_INVALID_ARGUMENT
    for m in (0, 1, 33):
        assert _lib.lib.lynse_hip_hnsw_levels(42, m, -1, 3, np.zeros(3, np.uint32).ctypes.data_as(C.c_void_p)) == _lib.ERR_UNSUPPORTED


def test_level_distribution():
    """P(level >= 1) = 1 / m: at n = 100,000 and m = 16 the count is binomial, mean 6250, sigma 76.5"""
    lv = lib_levels(42, 16, None, 100_000)
    c1 = int((lv >= 1).sum())
    print("level >= 1:", c1, "level >= 2:", int((lv >= 2).sum()), "max:", int(lv.max()))
    assert abs(c1 - 6250) <= 5 * 76.5


# ---- the restatement on hand-made graphs ------------------------------------------------------------------------------------------
def line(n):
    return np.arange(n, dtype=f32).reshape(n, 1)


def path(n, m=2):
    return H.flat_graph(n, m, {i: [j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)})


def sq(x):
    return f32(x) * f32(x)


def test_ref_path_graph(ref):
    data, q = line(5), np.array([[3.2]], f32)
    (rows, d), = H.ref_search(ref, data, O.L2, path(5), q, 2, 2)
    # 0 -> 1 -> 2 -> 3 -> 4: each step admits the next node and evicts the farthest; 4 (0.64) ties nothing and stays with 3 (0.04)
    assert rows.tolist() == [3, 4]
    assert d.tolist() == [sq(f32(3.2) - f32(3)), sq(f32(3.2) - f32(4))]
    # ef = 1: R = {3} refuses 4 (0.64 is not < 0.04) and the search ends there
    (rows, d), = H.ref_search(ref, data, O.L2, path(5), q, 1, 1)
    assert rows.tolist() == [3]
    # ef = 5, k = 3: everything is visited; the order is by distance
    (rows, d), = H.ref_search(ref, data, O.L2, path(5), q, 3, 5)
    assert rows.tolist() == [3, 4, 2]


def test_ref_small_entry_component_and_empty_list(ref):
    g = H.flat_graph(5, 2, {0: [1], 1: [0]})   # 2, 3, 4 have empty lists and nobody names them
    (rows, d), = H.ref_search(ref, line(5), O.L2, g, np.array([[4.0]], f32), 4, 4)
    assert rows.tolist() == [1, 0] and d.tolist() == [9.0, 16.0]
    g = H.flat_graph(1, 2, {})
    (rows, d), = H.ref_search(ref, line(1), O.IP, g, np.array([[2.0]], f32), 3, 3)
    assert rows.tolist() == [0] and d.tolist() == [0.0]


def test_ref_ties_are_broken_by_node(ref):
    data = np.array([[0.0], [1.0], [1.0], [1.0]], f32)   # 1, 2, 3 tie
    g = H.flat_graph(4, 2, {0: [3, 2, 1], 1: [0], 2: [0], 3: [0]})
    (rows, d), = H.ref_search(ref, data, O.L2, g, np.array([[1.0]], f32), 2, 2)
    # from 0 (d 1): 3 is admitted (R not full); 2 is (0 < worst.dist 1) and evicts 0; 1 is not (0 is not < 0): R = {2, 3}
    assert rows.tolist() == [2, 3] and d.tolist() == [0.0, 0.0]
    (rows, d), = H.ref_search(ref, data, O.L2, g, np.array([[1.0]], f32), 1, 1)
    assert rows.tolist() == [3]   # ef = 1: 3 replaces 0; 2 and 1 are not strictly closer than 3


def test_ref_greedy_descent(ref):
    data = line(4)
    levels = np.array([1, 0, 0, 1], np.uint32)
    adj0 = np.full((4, 4), H.PAD, np.uint32)
    for i, nb in {0: [1], 1: [0, 2], 2: [1, 3], 3: [2]}.items():
        adj0[i, :len(nb)] = nb
    upper = np.array([[3, H.PAD], [0, H.PAD]], np.uint32)   # (0, 1) -> 3, (3, 1) -> 0
    g = H.Graph(2, levels, adj0, upper, 0)
    assert g.upper_node.tolist() == [0, 3] and g.upper_level.tolist() == [1, 1]
    sc = []
    (rows, d), = H.ref_search(ref, data, O.L2, g, np.array([[2.9]], f32), 1, 1, scored=sc)
    assert rows.tolist() == [3] and d.tolist() == [sq(f32(2.9) - f32(3))]
    assert sc == [4]   # the entry, 3 from 0's list, 0 from 3's list (no move), then 2 at level 0 (refused)


def test_ref_build_of_the_reference_unit_test_vectors(ref):
    """the four vectors of hnsw.rs:1353, searched unfiltered: with no more candidates than m every node links to every other, nearest first"""
    data = np.array([[0.0, 0.0], [0.1, 0.0], [10.0, 10.0], [10.1, 10.0]], f32)
    g = H.ref_build(ref, data, O.L2, 8, 16, np.zeros(4, np.uint32))
    assert g.entry == 0
    assert g.adj0[:, :3].tolist() == [[1, 2, 3], [0, 2, 3], [3, 1, 0], [2, 1, 0]] and (g.adj0[:, 3:] == H.PAD).all()
    (rows, d), = H.ref_search(ref, data, O.L2, g, np.array([[0.0, 0.0]], f32), 2, 32)
    assert rows.tolist() == [0, 1] and d.tolist() == [0.0, sq(0.1)]


def test_ref_heuristic_by_hand(ref):
    """x = 0, 1, 2, 3, 10 and 4.5 on a line, m = 2 (cap 4 at level 0), five candidates each, so the heuristic runs everywhere.
    Node 5 (4.5) sees 3 (2.25), 2 (6.25), 1 (12.25), 0 (20.25), 4 (30.25): 3 is kept; 2, 1, 0 are closer to 3 than to 4.5; 4 is not
    (49 > 30.25) and is kept; the free slots go to the nearest leftovers 2 and 1: F(5) = [3, 4, 2, 1].  Likewise F(0) = [1, 2, 3, 5],
    F(1) = [0, 2, 3, 5] (0 and 2 tie at 1: node order), F(2) = [1, 3, 0, 5], F(3) = [2, 5, 1, 0], F(4) = [5, 3, 2, 1].
    U(0) = {1, 2, 3, 5} and U(4) = {5, 3, 2, 1} fit and are stored by distance; U(5) and U(1) have five members and go through the
    heuristic again."""
    data = np.array([[0.0], [1.0], [2.0], [3.0], [10.0], [4.5]], f32)
    g = H.ref_build(ref, data, O.L2, 2, 16, np.zeros(6, np.uint32))
    assert g.adj0[5].tolist() == [3, 4, 2, 1]
    assert g.adj0[0].tolist() == [1, 2, 3, 5]
    assert g.adj0[4].tolist() == [5, 3, 2, 1]
    assert g.adj0[1].tolist() == [0, 2, 3, 5]


# ---- recall of the restatement ----------------------------------------------------------------------------------------------------
def test_ref_recall_on_clustered_data(ref, oracle):
    """4096 x 32, L2, 32 Gaussian clusters of spread 0.15, default parameters, 100 queries: recall@10 against lo_canonical_topk; the floor
    is the reference's own gate for HNSW (benchmarks/gate_index_modes.py:259-273)."""
    data, queries, g, res, scored = H.recall_case(ref)
    hit = 0
    for qi in range(queries.shape[0]):
        e_ids, _ = oracle.canonical_topk(queries[qi], data, 10, O.L2, O.IPFORM_SINGLE)
        hit += len(set(res[qi][0].tolist()) & set(int(x) for x in e_ids))
    recall = hit / (10 * queries.shape[0])
    print(f"restatement recall@10 = {recall:.4f}, distances scored per query = {np.mean(scored):.0f}, levels = {int(g.levels.max()) + 1}")
    assert recall >= 0.90


# ---- the designed cases of the limits tests: the restatement against answers derived by hand ------------------------------------------
def beam_model(x, lists0, ef, k, drop_ties=False):
    """The level-0 walk with the kernel's bounded candidate set, for the 1-D cases (L2, query 0, entry 0): C has 2 ef + 8 slots; before a
    scoring step of 8 that might not fit, the entries beyond worst.dist are dropped.  drop_ties: the faulty comparison (`<` for `<=`)."""
    d = [float(f32(v) * f32(v)) for v in x]
    R, C, seen = [(d[0], 0)], [(d[0], 0)], {0}
    while C:
        c = min(C)
        C.remove(c)
        if len(R) >= ef and c[0] > max(R)[0]:
            break
        fresh = [j for j in lists0.get(c[1], []) if j not in seen]
        seen.update(fresh)
        for b in range(0, len(fresh), 8):
            if len(C) + 8 > 2 * ef + 8:
                w = max(R)[0]
                C = [e for e in C if (e[0] < w if drop_ties else e[0] <= w)]
            for j in fresh[b:b + 8]:
                if len(R) < ef or d[j] < max(R)[0]:
                    C.append((d[j], j))
                    R.append((d[j], j))
                    if len(R) > ef:
                        R.remove(max(R))
    return [j for _, j in sorted(R)[:k]]


def test_tie_bridge_needs_the_ties_kept():
    """the case discriminates: the bounded set that keeps ties at worst.dist finds row 10 through row 6, the one that drops them does not"""
    c = H.tie_bridge()
    lists0 = {0: list(range(1, 10)), 6: [10]}
    assert beam_model(c.data[:, 0], lists0, 3, 3) == [10, 8, 7] == c.rows.tolist()
    assert beam_model(c.data[:, 0], lists0, 3, 3, drop_ties=True) == [8, 7, 4]


@pytest.mark.parametrize("case", H.designed_cases(), ids=lambda c: c.name)
def test_ref_designed_cases(ref, case):
    """rows, distance bits and the distances scored, each written out by hand in tests/hnsw_common.py"""
    sc = []
    (rows, d), = H.ref_search(ref, case.data, O.L2, case.g, case.query, case.k, case.ef, scored=sc)
    assert rows.tolist() == case.rows.tolist(), (case.name, rows, case.rows)
    assert np.array_equal(d.view(np.uint32), case.dists.view(np.uint32)), (case.name, d, case.dists)
    assert sc == [case.scored], (case.name, sc, case.scored)


def test_ref_nan_query_ties_everything(ref):
    """a NaN query: every distance is +inf at once (ip: reported as -inf), so the walk is the all-ties walk whatever the rows"""
    data = np.random.default_rng(3).standard_normal((600, 8)).astype(f32)
    q = np.full((1, 8), np.nan, f32)
    for metric, far in ((O.IP, -np.inf), (O.L2, np.inf), (O.COS, np.inf)):
        for k, ef in H.ALL_TIES:
            sc = []
            (rows, d), = H.ref_search(ref, data, metric, H.path_graph(600), q, k, ef, scored=sc)
            assert rows.tolist() == list(range(k)) and (d == far).all() and sc == [ef + 1], (metric, k, ef, rows, d, sc)


# ---- the build's resource report ------------------------------------------------------------------------------------------------------
def test_search_kernel_keeps_its_registers():
    """k_hnsw_search in csrc/resource_usage.txt, read the way tests/test_text_modes.py reads it: no scratch, no spilled register, three waves
    per SIMD or more — what the beam shared through csrc/graph.h (graph_beam, forced inline, its state in registers) has to keep."""
    import re
    from pathlib import Path

    import lynsedb_amd

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    assert rep.exists(), "the build writes csrc/resource_usage.txt"
    blocks = re.findall(r"Function Name: (\S+)(.*?)LDS Size", rep.read_text(), flags=re.S)
    mine = [(n, {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", body)})
            for n, body in blocks if "k_hnsw_search" in n]
    assert mine, "k_hnsw_search is not in the report"
    for name, f in mine:
        assert f["ScratchSize [bytes/lane]"] == 0 and f["SGPRs Spill"] == 0 and f["VGPRs Spill"] == 0, (name, f)
        assert f["Occupancy [waves/SIMD]"] >= 3, (name, f)
