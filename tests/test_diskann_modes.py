"""DISKANN-{L2,COS} on the CPU: mode and option parsing, the random draws of rules 1-4 (lynse_hip_vamana_draws against the restatement
and a Python big-integer model), and the restatement the GPU tests compare against (tests/diskann_ref/diskann_ref.c) checked on its own:
the starts, the reference's own prune case, a 6-node build against a Python transliteration in exact integers, and searches with
their answers written out by hand.  No GPU."""
import numpy as np
import pytest

import diskann_common as D
from lynsedb_amd import _lib
from lynsedb_amd.core import DISKANN_DEFAULTS, DISKANN_SEED, diskann_build_options, diskann_mode_of, hnsw_mode_of

f32 = np.float32
L2, COS, PAD = D.L2, D.COS, D.PAD


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return D.build_ref(tmp_path_factory.mktemp("diskann_ref"), oracle)


# ---- modes and options ------------------------------------------------------------------------------------------------------------
def test_modes():
    for mode, metric in (("DISKANN-L2", _lib.METRIC_L2), ("DISKANN-COS", _lib.METRIC_COSINE), ("DISKANN-COSINE", _lib.METRIC_COSINE),
                         ("diskann-l2", _lib.METRIC_L2), ("DiskAnn-Cosine", _lib.METRIC_COSINE)):
        assert diskann_mode_of(mode) == metric
        assert hnsw_mode_of(mode) is None
    for mode in ("DISKANN-IP", "DISKANN-L2-PQ8", "DISKANN-IP-PQ8", "DISKANN-COS-PQ", "DISKANN-L2-SQ8", "DISKANN-COS-SQ8", "DISKANN", "DISKANN-HAMMING",
                 "HNSW-L2", "FLAT-L2", "IVF-L2"):
        assert diskann_mode_of(mode) is None


def test_build_options():
    assert DISKANN_DEFAULTS == {"r": 16, "l": 64, "alpha": 1.2} and DISKANN_SEED == 42
    assert diskann_build_options(None) == {"r": 16, "l": 64, "alpha": float(f32(1.2)), "max_degree": 16}
    assert diskann_build_options({"r": 4, "l": 8, "alpha": 1.0, "max_degree": 9}) == {"r": 4, "l": 8, "alpha": 1.0, "max_degree": 9}
    assert diskann_build_options({"r": 5})["max_degree"] == 5
    # keys of the other index families are ignored, None means the default
    assert diskann_build_options({"n_clusters": 9, "nprobe": 3, "m": 4, "ef_search": 7, "r": None})["r"] == 16
    for name in ("r", "l", "max_degree", "m", "n_clusters", "nprobe"):
        with pytest.raises(ValueError, match=f"Invalid argument: {name} must be greater than 0"):
            diskann_build_options({name: 0})
    for bad in (0.99, float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="Invalid argument: alpha must be a finite value >= 1.0"):
            diskann_build_options({"alpha": bad})
    # validate()'s order: the positive checks come before alpha
    with pytest.raises(ValueError, match="r must be greater than 0"):
        diskann_build_options({"alpha": 0.5, "r": 0})
    with pytest.raises(ValueError, match="unknown index build parameter 'beam'; supported keys: n_clusters, n_centroids, m, ef_construction"):
        diskann_build_options({"beam": 10})


# ---- rules 1-4 --------------------------------------------------------------------------------------------------------------------
def entry_on_position_0_seed(n, r):
    """a seed whose shuffle C already starts with ... any fixed node: position 0 of C is where the entry swap is the identity; the
    draws do not know the entry, so the case is a seed with order[0] == cands[0] (the entry when every sum ties)"""
    for seed in range(10_000):
        _, cands, order, _ = D.draws_py(seed, n, r)
        if order[0] == cands[0]:
            return seed
    raise AssertionError("no such seed")


@pytest.mark.parametrize("seed,n,r", [(42, 0, 4), (42, 1, 4), (42, 2, 4), (42, 5, 2), (42, 5, 16), (7, 5, 4), (42, 40, 16), (0, 100, 64), (42, 700, 4),
                                      (None, 9, 3)])
def test_draws_against_python_and_the_restatement(ref, seed, n, r):
    if seed is None:
        seed = entry_on_position_0_seed(n, r)
    exp = D.draws_py(seed, n, r)
    for name, fn in (("library", _lib.lib.lynse_hip_vamana_draws), ("restatement", ref[0].dr_draws)):
        got = D.draws_of(fn, seed, n, r)
        for what, g, e in zip(("refs", "cands", "order", "adj0"), got, exp):
            assert np.array_equal(g, e), (name, what, g, e)
    refs, cands, order, adj0 = exp
    assert refs.size == min(32, n) and cands.size == min(64, n) and sorted(order.tolist()) == list(range(n))
    for i in range(n):
        row = adj0[i][adj0[i] != PAD].tolist()
        assert len(row) == min(r, max(n - 1, 0)) == len(set(row)) and i not in row and (adj0[i, len(row):] == PAD).all()


def test_draws_refusals():
    import ctypes as C

    z = np.zeros(64, np.uint32)
    p = z.ctypes.data_as(C.c_void_p)
    assert _lib.lib.lynse_hip_vamana_draws(42, 3, 0, p, p, p, p) == _lib.ERR_UNSUPPORTED
    assert _lib.lib.lynse_hip_vamana_draws(42, 3, 65, p, p, p, p) == _lib.ERR_UNSUPPORTED
    assert _lib.lib.lynse_hip_vamana_draws(42, 3, 4, None, p, p, p) == _lib.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("n,entry,anchors,exp", [(1, 0, 8, [0]), (5, 2, 8, [2, 0, 1, 3, 4]), (5, 0, 8, [0, 1, 2, 3, 4]), (8, 7, 8, [7, 0, 1, 2, 3, 4, 5, 6]),
                                                 (9, 4, 8, [4, 0, 1, 2, 3, 5, 6, 7]), (9, 8, 8, [8, 0, 1, 2, 3, 4, 5, 6, 7]),
                                                 (600, 75, 8, [75, 0, 150, 225, 300, 375, 450, 525]), (600, 7, 8, [7, 0, 75, 150, 225, 300, 375, 450, 525]),
                                                 (100, 50, 32, None)])
def test_starts(ref, n, entry, anchors, exp):
    got = D.ref_starts(ref, n, entry, anchors)
    assert got == D.starts_py(n, entry, anchors)
    if exp is not None:
        assert got == exp
    assert len(got) == len(set(got)) <= 33


# ---- rule 6 -----------------------------------------------------------------------------------------------------------------------
def test_prune_the_references_own_case(ref):
    """diskann_robust_prune_uses_alpha (diskann.rs:2234) as data: p at the origin, a close, b almost behind a, c far and orthogonal"""
    data = np.array([[0, 0], [1, 0], [1.1, 0.05], [0, 2]], f32)
    d_pb = f32(f32(1.1) * f32(1.1)) + f32(f32(0.05) * f32(0.05))
    assert D.ref_prune(ref, data, L2, 0, [1.0, d_pb, 2.0], [1, 2, 3], 2, 1.2) == [1, 3]
    # alpha = 1 is the plain rule: b is still occluded, c still survives (5 > 2)
    assert D.ref_prune(ref, data, L2, 0, [1.0, d_pb, 2.0], [1, 2, 3], 2, 1.0) == [1, 3]
    # p itself and a node named twice are dropped; ties are ordered by node
    assert D.ref_prune(ref, data, L2, 0, [0.0, 2.0, 1.0, 1.0, 2.0], [0, 3, 1, 1, 3], 4, 1.2) == [1, 3]
    data = np.array([[0], [2], [-2], [3]], f32)
    assert D.ref_prune(ref, data, L2, 0, [4.0, 4.0, 9.0], [2, 1, 3], 3, 1.0) == [1, 2]   # 1 before 2 at 4; 3: d(1, 3) = 1 is not > 9
    assert D.ref_prune(ref, data, L2, 0, [4.0, 4.0, 9.0], [2, 1, 3], 1, 1.0) == [1]
    # alpha keeps what the plain rule cuts: d(1, 3) = 1, 9.5 * 1 > 9
    assert D.ref_prune(ref, data, L2, 0, [4.0, 4.0, 9.0], [2, 1, 3], 3, 9.5) == [1, 2, 3]


# ---- rule 8 -----------------------------------------------------------------------------------------------------------------------
def test_search_answers_written_out_by_hand(ref):
    data, g, n = D.fan_graph()
    sc = []
    (rows, d), = D.ref_search(ref, data, L2, g, np.zeros((1, 1), f32), 1, D.query_ef(g, n, 1, 0), scored=sc)
    assert rows.tolist() == [1] and d.tolist() == [0.25] and sc == [74]
    # ef below the number of starts: n = 600 on the line, x_i = i + 1, query 0, ef = 1: R keeps the nearest start (row 0) and the walk
    # stops at once when 0 names nothing; the other 8 starts were scored
    x = (np.arange(600, dtype=f32) + 1).reshape(-1, 1)
    g = D.made_graph(600, 1, {}, entry=301)
    sc = []
    (rows, d), = D.ref_search(ref, x, L2, g, np.zeros((1, 1), f32), 1, 1, scored=sc)
    assert rows.tolist() == [0] and d.tolist() == [1.0] and sc == [9]
    # a path from the far end: the entry 4 and the anchors 0 .. 3 of n = 5 are all the rows: everything is a start
    g = D.made_graph(5, 2, {i: [j for j in (i - 1, i + 1) if 0 <= j < 5] for i in range(5)}, entry=4)
    sc = []
    (rows, d), = D.ref_search(ref, x[:5], L2, g, np.zeros((1, 1), f32), 3, 5, scored=sc)
    assert rows.tolist() == [0, 1, 2] and d.tolist() == [1.0, 4.0, 9.0] and sc == [5]
    # a component the starts do not reach stays unseen: the count is below k
    g = D.made_graph(20, 2, {0: [1], 1: [0]}, entry=0)
    (rows, d), = D.ref_search(ref, x[:20], L2, g, np.zeros((1, 1), f32), 15, 20)
    assert rows.tolist() == [0, 1, 2, 5, 7, 10, 12, 15, 17]   # the starts 0, 2, 5, ... and 1


# ---- rules 5-7 --------------------------------------------------------------------------------------------------------------------
def build_py(x, r, l, alpha, seed, max_batches=0):
    """Rules 2-7 transliterated for 1-D integer-valued rows under L2 (every distance an exact small integer, so Python floats and f32
    agree), fewer rows than a batch and than the anchors: every search starts from all rows, so its result is the best L_b rows."""
    n = len(x)
    assert n <= 8
    d = lambda a, b: float((x[a] - x[b]) ** 2)
    refs, cands, order, adj0 = D.draws_py(seed, n, r)
    best, entry = float("inf"), int(cands[0])
    for c in cands:
        s = sum(d(int(c), int(j)) for j in refs)
        if s < best:
            best, entry = s, int(c)
    order = order.tolist()
    pos = order.index(entry)
    order[0], order[pos] = order[pos], order[0]
    G = [[int(v) for v in row if v != PAD] for row in adj0]
    lb = max(min(max(l, r), 128), r)

    def prune(p, cand, a):
        pool = sorted({v: (dv, v) for dv, v in cand if v != p}.values())
        out = []
        while pool and len(out) < r:
            b = pool[0][1]
            out.append(b)
            pool = [(dv, v) for dv, v in pool if v != b and a * d(b, v) > dv]
        return out

    batches = 0
    for a in ([1.0, alpha] if alpha > 1.0 + 2.0 ** -23 else [1.0]):
        fwd = []
        for p in order:   # one batch
            beam = sorted((d(p, v), v) for v in range(n))[:lb]
            fwd.append((p, prune(p, beam + [(d(p, v), v) for v in G[p]], a)))
        for p, lst in fwd:
            G[p] = list(lst)
        touched = []
        for p, lst in fwd:
            for dst in lst:
                if p not in G[dst]:
                    G[dst].append(p)
                if dst not in touched:
                    touched.append(dst)
        for dst in touched:
            if len(G[dst]) > r:
                G[dst] = prune(dst, [(d(dst, v), v) for v in G[dst]], a)
        batches += 1
        if batches == max_batches:
            break
    adj = np.full((n, r), PAD, np.uint32)
    for i, row in enumerate(G):
        adj[i, :len(row)] = row
    return entry, adj


@pytest.mark.parametrize("x,r,l,alpha,seed,mb", [([0, 1, 3, 6, 10, 15], 2, 2, 1.2, 42, 0), ([0, 1, 3, 6, 10, 15], 2, 2, 1.2, 42, 1), ([0, 1, 3, 6, 10, 15], 2, 4, 1.0, 7, 0),
                                                 ([5, 5, 0, 9, 9, 2], 3, 3, 2.0, 3, 0), ([0, 4], 4, 4, 1.2, 42, 0), ([3], 2, 2, 1.2, 42, 0),
                                                 ([0, 1, 2, 3, 4, 5, 6, 7], 1, 1, 1.5, 1, 0)])
def test_small_builds_against_the_python_transliteration(ref, x, r, l, alpha, seed, mb):
    data = np.asarray(x, f32).reshape(-1, 1)
    g = D.ref_build(ref, data, L2, r, l, alpha, seed, mb)
    entry, adj = build_py(x, r, l, alpha, seed, mb)
    assert g.entry == entry
    assert np.array_equal(g.adj, adj), (g.adj, adj)


def test_restatement_build_invariants(ref):
    """the restatement over three batches and two passes: lists hold distinct nodes other than their own, at most r, pads at the end;
    a stopped build differs from the finished one; the hub case sees the long commit list it was made for"""
    data, _ = D.clustered(3, 700, 8, 8, 0.15, 1)
    g = D.ref_build(ref, data, L2, 4, 8, 1.2)
    for i, row in enumerate(g.adj):
        nb = row[row != PAD].tolist()
        assert len(nb) == len(set(nb)) and i not in nb and (row[len(nb):] == PAD).all()
    graphs = [D.ref_build(ref, data, L2, 4, 8, 1.2, max_batches=mb).adj for mb in (1, 3, 4, 6)]
    assert np.array_equal(graphs[3], g.adj)
    assert all(not np.array_equal(graphs[i], graphs[i + 1]) for i in range(3))
    hub = D.ref_build(ref, D.hub_data(), L2, 4, 8, 1.2)
    assert hub.longest > 4 + 200, hub.longest


# ---- the build's resource report ------------------------------------------------------------------------------------------------------
def test_search_kernel_keeps_its_registers():
    """k_vamana_search in csrc/resource_usage.txt, read the way tests/test_text_modes.py reads it: no scratch, no spilled register, three waves
    per SIMD or more — what the beam shared through csrc/graph.h (graph_beam, forced inline, its state in registers) has to keep."""
    import re
    from pathlib import Path

    import lynsedb_amd

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    assert rep.exists(), "the build writes csrc/resource_usage.txt"
    blocks = re.findall(r"Function Name: (\S+)(.*?)LDS Size", rep.read_text(), flags=re.S)
    mine = [(n, {k: int(v) for k, v in re.findall(r"(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", body)})
            for n, body in blocks if "k_vamana_search" in n]
    assert mine, "k_vamana_search is not in the report"
    for name, f in mine:
        assert f["ScratchSize [bytes/lane]"] == 0 and f["SGPRs Spill"] == 0 and f["VGPRs Spill"] == 0, (name, f)
        assert f["Occupancy [waves/SIMD]"] >= 3, (name, f)
