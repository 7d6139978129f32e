"""GPU parity tests for DISKANN-{L2,COS} (DiskANNIndex, src/index/diskann.rs, in memory and at full precision) through the C ABI and the
Collection, against the restatement of the DiskANN rule block of include/lynse_hip.h (tests/diskann_ref/diskann_ref.c: the draws, the
batched Vamana build and the search in plain C, every distance computed afresh by the oracle's lo_compute_distance, unbounded heaps, a
sequential commit).  The entry, the adjacency with its order, result ids, f32 distance bits, counts and the distances scored are
compared exactly; there are no tolerances."""
import numpy as np
import pytest

import diskann_common as D
import oracle as O
from diskann_common import assert_same_graph, check, load, make_data, sweep

pytestmark = pytest.mark.gpu
L2, COS, PAD = D.L2, D.COS, D.PAD
f32 = np.float32
LDS_MAX = 160 * 1024


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return D.build_ref(tmp_path_factory.mktemp("diskann_ref"), oracle)


def flat(L, data):
    idx = L.FlatIndex(None, data.shape[1], device=0)
    idx.write(np.ascontiguousarray(data, f32))
    return idx


# -------------------------------------------------------------------- search over loaded graphs ----
COMBOS = [(1, 0, 5), (10, 0, 300), (10, 200, 5), (3, 64, 1), (64, 0, 2)]   # (k, ef_query, nq)


@pytest.mark.parametrize("r,kind", [(1, "gauss"), (4, "gauss"), (16, "dup"), (64, "gauss"), (4, "nonfinite"), (16, "nonfinite"), (64, "dup")])
def test_search_random_graphs(L, ref, r, kind):
    rng = np.random.default_rng(1000 + r)
    data, queries = make_data(kind, rng, 600, 16, 37)
    idx = flat(L, data)
    g = D.random_graph(rng, 600, r, l=int(rng.integers(1, 40)))
    for metric in (L2, COS):
        sweep(idx, ref, data, g, metric, queries, COMBOS)


def test_search_ef_below_the_starts(L, ref):
    """k = 1, l = 1, n = 600: the smallest beam a query can have, ef = 10 k = 10 against 9 starts.  A beam below the number of starts
    is the build's alone (r = l = 1: L_b = 1 against 33 starts, test_builds[300-5-1-1-1.2-gauss])."""
    rng = np.random.default_rng(2)
    data, queries = make_data("gauss", rng, 600, 16, 9)
    idx = flat(L, data)
    sweep(idx, ref, data, D.random_graph(rng, 600, 4, l=1), L2, queries, [(1, 0, 9), (1, 1, 1)])


@pytest.mark.parametrize("n", [1, 2, 5, 8, 9, 33])
def test_search_few_rows(L, ref, n):
    """fewer rows than anchors: every row is a start"""
    rng = np.random.default_rng(n)
    data, queries = make_data("gauss", rng, n, 16, 7)
    idx = flat(L, data)
    for entry in {0, n - 1, n // 2}:
        g = D.random_graph(rng, n, 4, fill=0.5)
        g.entry = entry
        for metric in (L2, COS):
            sweep(idx, ref, data, g, metric, queries, [(1, 0, 7), (n, 0, 3), (n + 3, n + 5, 1)])


def test_search_entry_equal_to_an_anchor(L, ref):
    rng = np.random.default_rng(4)
    data, queries = make_data("gauss", rng, 600, 16, 11)
    idx = flat(L, data)
    for entry in (0, 75, 525, 76, 599):   # anchors of n = 600: 0, 75, ..., 525
        g = D.random_graph(rng, 600, 4)
        g.entry = entry
        sweep(idx, ref, data, g, L2, queries, [(10, 0, 11)])


def test_search_designed_graphs(L, ref):
    """the fan of 64 at worst.dist behind a full R with its answer written out (tests/test_diskann_modes.py holds the restatement to
    it); a disconnected graph: the count is below k; pads inside a list and a neighbour named twice: the stored form drops both"""
    data, g, n = D.fan_graph()
    idx = flat(L, data)
    load(idx, g, L2)
    idx.profile_enable(True)
    idx.diskann_stage_times(reset=True)
    rows, dists, counts = idx.search_diskann_batch_arrays(np.zeros((1, 1), f32), 1, L2)
    t = idx.diskann_stage_times(reset=True)
    idx.profile_enable(False)
    assert (int(counts[0]), rows[0].tolist(), dists[0].tolist(), t["scored"]) == (1, [1], [0.25], 74)
    sweep(idx, ref, data, g, L2, np.array([[0.0], [0.3], [-7.0], [6.9]], f32), [(1, 0, 4), (7, 0, 4), (7, 74, 4)])
    x = (np.arange(20, dtype=f32) + 1).reshape(-1, 1)
    g = D.made_graph(20, 2, {0: [1], 1: [0]}, entry=0)
    idx = flat(L, x)
    load(idx, g, L2)
    rows, dists, counts = idx.search_diskann_batch_arrays(np.zeros((1, 1), f32), 15, L2)
    assert int(counts[0]) == 9 and rows[0, :9].tolist() == [0, 1, 2, 5, 7, 10, 12, 15, 17]
    sweep(idx, ref, x, g, L2, np.zeros((1, 1), f32), [(15, 0, 1)])
    g = D.made_graph(20, 4, {i: [PAD, (i + 1) % 20, (i + 1) % 20, (i + 2) % 20] for i in range(20)}, entry=3)
    load(idx, g, L2)
    adj = idx.diskann_params()["adj"]
    assert np.array_equal(adj[:, 0], (np.arange(20) + 1) % 20) and np.array_equal(adj[:, 1], (np.arange(20) + 2) % 20) and (adj[:, 2:] == PAD).all()
    sweep(idx, ref, x, g, L2, np.zeros((1, 1), f32), [(5, 0, 1)])


def test_search_ties_through_compactions(L, ref):
    """integer rows in two dimensions: most distances tie, lists of 64 and ef = 10: C passes its 2 ef + 41 slots with ties at worst.dist
    among its entries, so the compaction's `<=` (graph_beam, csrc/graph.h: `if (Cn + 8 > c_cap)` -> graph_compact with `(kx >> 32) <= wd`)
    and the (dist, node) order of every pop and eviction decide the answer"""
    rng = np.random.default_rng(6)
    data = rng.integers(-6, 7, (600, 2)).astype(f32)
    queries = rng.integers(-6, 7, (20, 2)).astype(f32)
    idx = flat(L, data)
    for seed in range(3):
        g = D.random_graph(np.random.default_rng(seed), 600, 64, fill=1.0)
        sweep(idx, ref, data, g, L2, queries, [(1, 0, 20), (1, 12, 20), (3, 0, 20)])


@pytest.mark.parametrize("n", [31, 32, 33, 64, 65, 97])
def test_search_visited_words(L, ref, n):
    """node ids across the 32-bit words of the bitmap: a complete graph on n rows, lists of 64 where they fit"""
    rng = np.random.default_rng(n)
    data, queries = make_data("gauss", rng, n, 8, 5)
    idx = flat(L, data)
    r = 64
    g = D.made_graph(n, r, {i: [int(v) for v in rng.permutation(n)[:r]] for i in range(n)}, entry=n - 1)
    sweep(idx, ref, data, g, L2, queries, [(n, 0, 5), (1, 0, 5)])


def test_graph_covers_the_first_rows_only_and_leaves_hnsw_alone(L, ref):
    """rule 9"""
    import hnsw_common as H

    rng = np.random.default_rng(5)
    data, queries = make_data("gauss", rng, 300, 16, 9)
    idx = flat(L, data)
    hg = H.random_graph(rng, 300, 4)
    H.load(idx, hg, L2)
    g = D.random_graph(rng, 200, 4)
    load(idx, g, L2)
    exp = D.ref_search(ref, data[:200], L2, g, queries, 10, D.query_ef(g, 200, 10, 0))
    check(idx.search_diskann_batch_arrays(queries, 10, L2), exp, "first rows")
    idx.write(rng.standard_normal((50, 16)).astype(f32))
    check(idx.search_diskann_batch_arrays(queries, 10, L2), exp, "after an append")
    p = idx.diskann_params(arrays=False)
    assert (p["n"], p["r"], p["l"], p["entry"], p["metric"], p["alpha"]) == (200, 4, 4, g.entry, L2, 0.0)
    assert idx.hnsw_params(arrays=False)["m"] == 4   # a separate state
    idx.drop_diskann()
    assert idx.diskann_params()["r"] == 0 and idx.diskann_params()["n"] == 0 and idx.hnsw_params(arrays=False)["m"] == 4
    with pytest.raises(ValueError, match="no DiskANN index"):
        idx.search_diskann_batch_arrays(queries, 10, L2)
    load(idx, g, L2)
    idx.drop_hnsw()
    check(idx.search_diskann_batch_arrays(queries, 10, L2), exp, "after the HNSW graph went")


# ------------------------------------------------------------------------------------------ build ----
def build_and_compare(L, ref, data, metric, r, l, alpha, what, seed=42, max_batches=0, queries=None):
    idx = flat(L, data)
    g = D.ref_build(ref, data, metric, r, l, alpha, seed, max_batches)
    idx.build_diskann(metric, r, l, alpha, None, seed, max_batches)
    p = idx.diskann_params()
    assert_same_graph(p, g, what)
    assert p["l"] == max(l, r) and p["alpha"] == float(f32(alpha)) and p["metric"] == metric
    if queries is not None:
        n = data.shape[0]
        for k, efq in [(10, 0), (1, 200)]:
            check(idx.search_diskann_batch_arrays(queries, k, metric, efq), D.ref_search(ref, data, metric, g, queries, k, D.query_ef(g, n, k, efq)), what)
    return idx, g


@pytest.mark.parametrize("max_batches", [0, 1, 3, 4])
def test_build_three_batches_two_passes(L, ref, max_batches):
    """700 x 8, r 4, l 8, alpha 1.2: three batches, the last one short, two passes; stopped after 1, 3 (the end of pass 1) and 4"""
    rng = np.random.default_rng(70)
    data, queries = make_data("gauss", rng, 700, 8, 13)
    for metric in (L2, COS):
        build_and_compare(L, ref, data, metric, 4, 8, 1.2, (D.NAME[metric], max_batches), max_batches=max_batches, queries=queries)


@pytest.mark.parametrize("n,dim,r,l,alpha,kind", [(300, 16, 16, 64, 1.2, "gauss"), (300, 16, 16, 64, 1.0, "gauss"), (5, 8, 16, 64, 1.2, "gauss"),
                                                  (1, 8, 4, 8, 1.2, "gauss"), (2, 8, 4, 8, 1.2, "gauss"), (300, 16, 64, 64, 1.2, "gauss"),
                                                  (300, 16, 4, 4096, 1.2, "gauss"), (300, 16, 16, 2, 1.2, "gauss"), (300, 8, 4, 8, 1.2, "dup"),
                                                  (300, 8, 8, 16, 2.0, "dup"), (300, 5, 1, 1, 1.2, "gauss"), (300, 16, 4, 8, 1.2, "nonfinite"),
                                                  (257, 3, 2, 4, 1.5, "gauss"), (256, 3, 2, 4, 1.5, "gauss")])
def test_builds(L, ref, n, dim, r, l, alpha, kind):
    """the defaults; alpha = 1 (one pass); r >= n (the degree is n - 1); n = 1 and 2; r = l = 64; l = 4096 (the build beam is capped at
    128); l < r; duplicate rows (ties by (d, node) in the prune); r = l = 1 (L_b = 1 against 33 starts); non-finite rows; a batch of
    exactly 256 and one of 256 + 1"""
    rng = np.random.default_rng(n + dim + r + l)
    data, queries = make_data(kind, rng, n, dim, 9)
    for metric in (L2, COS):
        build_and_compare(L, ref, data, metric, r, l, alpha, (D.NAME[metric], n, dim, r, l, alpha, kind), queries=queries)


def test_build_hub(L, ref):
    """520 x 32, row 0 at the origin and the others unit vectors, r = 4: row 0 is every batch member's nearest row, receives some 250
    reverse edges in one commit and goes through the r + 256 prune.  The restatement saw a list longer than r + 200."""
    data = D.hub_data()
    idx, g = build_and_compare(L, ref, data, L2, 4, 8, 1.2, "hub", queries=data[1:6])
    assert g.longest > 4 + 200, g.longest


def test_build_seed_and_stage_times(L, ref):
    rng = np.random.default_rng(8)
    data, _ = make_data("gauss", rng, 300, 8, 1)
    idx, g7 = build_and_compare(L, ref, data, L2, 4, 8, 1.2, "seed 7", seed=7)
    t = idx.diskann_stage_times()
    assert t["build_us"] > 0 and t["build_search_us"] == 0   # a plain build waits once, at its end
    idx.profile_enable(True)
    idx.build_diskann(L2, 4, 8, 1.2, None, 42)
    idx.profile_enable(False)
    t = idx.diskann_stage_times()
    assert min(t["build_search_us"], t["build_prune_us"], t["build_commit_us"]) > 0
    g42 = D.ref_build(ref, data, L2, 4, 8, 1.2, 42)
    assert_same_graph(idx.diskann_params(), g42, "seed 42, timed")
    assert not np.array_equal(g7.adj, g42.adj)


# ----------------------------------------------------------------------------------------- limits ----
def test_search_in_two_chunks(L):
    """graph_search (csrc/graph_host.inc): qc = min(nq, 256 MiB / (4 vis_words), ...).  n = 2^22 rows give vis_words = 131,072 (512 KiB of
    visited bits per query) and qc = 512, so 513 queries go as chunks of 512 and 1: the second uploads `queries + q0 * D` and copies
    back to `out_rows + q0 * k`, `out_dists + q0 * k` and `out_counts + q0`.  Every list is a pad (r = l = 1, entry 1): a query sees its 9
    starts — row 1 and rows a n / 8 — and answers the 3 nearest by (distance, row); integer coordinates, so every L2 distance is exact
    in f32."""
    n, nq, k = 1 << 22, 513, 3
    assert (256 << 20) // (4 * ((n + 31) // 32)) == nq - 1
    rng = np.random.default_rng(22)
    data = rng.integers(-8, 9, (n, 2)).astype(f32)
    queries = np.stack([np.arange(nq) % 32 - 16, np.arange(nq) // 32 - 8], axis=1).astype(f32)
    assert np.unique(queries, axis=0).shape[0] == nq
    starts = np.array(D.starts_py(n, 1, D.QUERY_ANCHORS))
    assert starts.tolist() == [1] + [a * n // 8 for a in range(8)]
    idx = flat(L, data)
    load(idx, D.Graph(1, 1, np.full((n, 1), PAD, np.uint32), 1), L2)
    idx.profile_enable(True)
    idx.diskann_stage_times(reset=True)
    rows, dists, counts = idx.search_diskann_batch_arrays(queries, k, L2)
    t = idx.diskann_stage_times(reset=True)
    idx.profile_enable(False)
    d = ((queries[:, None, :] - data[starts][None, :, :]) ** 2).sum(axis=2, dtype=f32)   # [nq][9]
    order = np.stack([np.lexsort((starts, d[qi]))[:k] for qi in range(nq)])
    assert counts.tolist() == [k] * nq, np.nonzero(counts != k)[0][:5]
    assert np.array_equal(rows, starts[order].astype(np.uint64)), np.nonzero((rows != starts[order]).any(axis=1))[0][:5]
    assert np.array_equal(dists.view(np.uint32), np.take_along_axis(d, order, axis=1).view(np.uint32))
    assert (t["searches"], t["scored"]) == (1, 9 * nq), t


def test_largest_beam(L, ref):
    """lynse_hip_flat_search_diskann_f32: GraphSearchLds::bytes(ef, vamana_c_cap(ef), D) (csrc/graph.h) = 24 ef + 584 + 4 D bytes of LDS.  D = 16: ef = 6,790 (k = 679) fits, ef = 6,800 (k = 680) is the
    first that does not: refused, and the next search still answers."""
    assert 24 * 6790 + 584 + 64 <= LDS_MAX < 24 * 6800 + 584 + 64
    rng = np.random.default_rng(9)
    data, queries = make_data("gauss", rng, 7000, 16, 2)
    idx = flat(L, data)
    g = D.random_graph(rng, 7000, 4, fill=1.0)
    sweep(idx, ref, data, g, L2, queries, [(679, 0, 2)])
    with pytest.raises(NotImplementedError, match="do not fit in LDS"):
        idx.search_diskann_batch_arrays(queries, 680, L2)
    with pytest.raises(NotImplementedError, match="between 1 and 4096"):
        idx.search_diskann_batch_arrays(queries, 1, L2, 4097)
    sweep(idx, ref, data, g, L2, queries, [(10, 4096, 2)])


def test_widest_rows(L, ref):
    """the build: the prune holds two arrays of r + 256 keys and two rows, 16 (r + 256) + 8 D bytes: r = 1, D = 19,966 fits, 19,967 is
    refused.  Load and search: 24 ef + 584 + 4 D with ef >= 1: D = 40,808 fits (one row: ef = 1), 40,809 is refused."""
    assert 16 * 257 + 8 * 19966 <= LDS_MAX < 16 * 257 + 8 * 19967 and 24 + 584 + 4 * 40808 <= LDS_MAX < 24 + 584 + 4 * 40809
    rng = np.random.default_rng(10)
    data = rng.standard_normal((5, 19967)).astype(f32)
    build_and_compare(L, ref, np.ascontiguousarray(data[:, :19966]), COS, 1, 1, 1.2, "D = 19,966", queries=np.ascontiguousarray(data[:2, :19966]))
    wide = flat(L, data)
    with pytest.raises(NotImplementedError, match="does not fit in LDS"):
        wide.build_diskann(COS, 1, 1, 1.2)
    row = rng.standard_normal((1, 40809)).astype(f32)
    g = D.made_graph(1, 1, {}, entry=0)
    idx = flat(L, np.ascontiguousarray(row[:, :40808]))
    sweep(idx, ref, np.ascontiguousarray(row[:, :40808]), g, L2, np.ascontiguousarray(row[:, :40808]) + f32(1), [(1, 0, 1)])
    with pytest.raises(NotImplementedError, match="does not fit in LDS"):
        load(flat(L, row), g, L2)
    check(idx.search_diskann_batch_arrays(np.ascontiguousarray(row[:, :40808]), 1, L2), [(np.zeros(1, np.uint64), np.zeros(1, f32))], "after the refusal")


# ------------------------------------------------------------------------------------------ C ABI ----
def test_cabi_refusals(L):
    rng = np.random.default_rng(9)
    data = rng.standard_normal((100, 16)).astype(f32)
    q = data[:3]
    g = D.random_graph(rng, 100, 4)
    idx = flat(L, data)
    unsupported, invalid = NotImplementedError, ValueError
    for metric in ("ip", "hamming", "jaccard", "l1", "chebyshev"):
        with pytest.raises(unsupported):
            idx.build_diskann(metric)
        with pytest.raises(unsupported):
            idx.load_diskann(metric, 4, 8, g.adj, 0)
    for kw in ({"r": 0}, {"r": 65}, {"l": 0}, {"l": 4097}, {"alpha": 0.5}, {"alpha": float("inf")}, {"alpha": float("nan")}):
        with pytest.raises(unsupported):
            idx.build_diskann(L2, **kw)
    with pytest.raises(invalid, match="no DiskANN index"):
        idx.search_diskann_batch_arrays(q, 3, L2)
    load(idx, g, L2)
    with pytest.raises(invalid, match="another metric"):
        idx.search_diskann_batch_arrays(q, 3, COS)
    with pytest.raises(unsupported):
        idx.search_diskann_batch_arrays(q, 3, "ip")
    assert idx.search_diskann_batch_arrays(q, 0, L2)[2].tolist() == [0, 0, 0]
    bad = g.adj.copy(); bad[3, 0] = 100
    with pytest.raises(invalid, match="beyond the rows"):
        idx.load_diskann(L2, 4, 8, bad, 0)
    with pytest.raises(invalid, match="entry"):
        idx.load_diskann(L2, 4, 8, g.adj, 100)
    with pytest.raises(invalid, match="more rows"):
        idx.load_diskann(L2, 4, 8, np.zeros((101, 4), np.uint32), 0)
    h16 = L.FlatIndex(None, 16, device=0, dtype="f16")
    h16.write(data)
    packed = L.FlatIndex(None, 64, device=0)
    packed.write_packed(rng.integers(0, 1 << 62, (100, 1), dtype=np.uint64))
    mapped = flat(L, data)
    mapped.set_row_map(2, 1)
    for h in (h16, packed, mapped):
        with pytest.raises(unsupported):
            h.build_diskann(L2)
    for h in (h16, mapped):
        with pytest.raises(unsupported):
            load(h, g, L2)


# ------------------------------------------------------------------------------------- Collection ----
def coll(L, data, mode, params=None, ids=None):
    c = L.Collection("c", data.shape[1], device=0)
    c.add_items(data, np.arange(data.shape[0]) + 1000 if ids is None else ids)
    c.commit()
    c.build_index(mode, params)
    return c


def test_collection_recall_case(L, ref, oracle):
    """4096 x 32 in 32 clusters with the defaults: equal to the restatement, which measured recall@10 = 1.000 on this data on the CPU
    (scripts/diskann_ref_recall.py; HNSW reads 0.960 on it), so the reference's own gate of 0.90
    (benchmarks/gate_index_modes.py:259-273) is asserted here.  On the 20,000-row cut of the 1000-cluster set the restatement read
    0.93, below the 0.95 that would let a gate be asserted: equality alone covers it."""
    data, queries, g, res = D.recall_case(ref)
    c = coll(L, data, "DISKANN-L2", ids=np.arange(4096))
    assert_same_graph(c._flat.diskann_params(), g, "recall case")
    hit = 0
    for qi, r in enumerate(c.batch_search(queries, 10)):
        assert r.index_mode() == "DISKANN-L2"
        assert np.array_equal(np.asarray(r.ids()), res[qi][0].astype(np.int64))
        assert np.array_equal(np.asarray(r.distances(), f32).view(np.uint32), res[qi][1].view(np.uint32))
        e_ids, _ = oracle.canonical_topk(queries[qi], data, 10, L2, O.IPFORM_SINGLE)
        hit += len(set(int(x) for x in r.ids()) & set(int(x) for x in e_ids))
    print(f"recall@10 on the GPU = {hit / 1000:.4f}")
    assert hit / 1000 >= 0.90


@pytest.mark.parametrize("mode,metric", [("DISKANN-L2", L2), ("diskann-cos", COS), ("DISKANN-COSINE", COS)])
def test_collection_search_paths(L, ref, oracle, mode, metric):
    rng = np.random.default_rng(11 + metric)
    data, queries = make_data("gauss", rng, 700, 24, 12)
    opts = {"r": 4, "l": 8, "alpha": 1.2, "nprobe": 5, "m": 3}   # (nprobe, m: other families' keys, ignored)
    c = coll(L, data, mode, opts)
    g = D.ref_build(ref, data, metric, 4, 8, 1.2)
    assert_same_graph(c._flat.diskann_params(), g, mode)

    def expect(q, k, ef, gg=g, dd=data):
        return D.ref_search(ref, dd, metric, gg, q, k, D.query_ef(gg, dd.shape[0], k, ef))

    def same(results, exp, off=1000):
        for r, (e_rows, e_d) in zip(results, exp):
            assert r.index_mode() == mode.upper()
            assert np.array_equal(np.asarray(r.ids()), e_rows.astype(np.int64) + off)
            assert np.array_equal(np.asarray(r.distances(), f32).view(np.uint32), e_d.view(np.uint32))

    same(c.batch_search(queries, 10), expect(queries, 10, 0))
    same([c.search(queries[0], 5)], expect(queries[:1], 5, 0))
    same(c.batch_search(queries, 10, nprobe=300), expect(queries, 10, 300))   # nprobe > 0 is ef_query
    prof = c.search_profile(queries[0], 10)
    assert prof["profile"]["index_path"] == "ann_index" and prof["items"]["index"] == mode.upper()
    assert prof["profile"]["device"]["diskann"]["scored"] > 0
    # tombstones: k' = k + tombstones through the graph, then the filter
    dead = [int(x) + 1000 for x in expect(queries[:1], 3, 0)[0][0][:2]]
    c.delete_items(dead)
    for r, (e_rows, e_d) in zip(c.batch_search(queries, 10), expect(queries, 12, 0)):
        keep = ~np.isin(e_rows + 1000, dead)
        assert np.array_equal(np.asarray(r.ids()), (e_rows[keep] + 1000).astype(np.int64)[:10])
    c.restore_items(dead)
    # a subset takes the exact filtered scan
    subset = np.arange(0, 700, 3)
    for qi, r in enumerate(c.batch_search(queries, 7, subset=subset)):
        e_ids, e_d = oracle.canonical_topk(queries[qi], data[subset], 7, metric, O.IPFORM_SINGLE)
        assert np.array_equal(np.asarray(r.ids()), subset[e_ids.astype(np.int64)] + 1000)
        assert np.array_equal(np.asarray(r.distances(), f32).view(np.uint32), e_d.view(np.uint32))
    # rows added and flushed: the graph is rebuilt at the next search and finds them
    extra = (queries[:3] + f32(1e-3)).astype(f32)
    c.add_items(extra, [5000, 5001, 5002])
    c.commit()
    data2 = np.concatenate([data, extra])
    g2 = D.ref_build(ref, data2, metric, 4, 8, 1.2)
    res = c.batch_search(queries[:3], 10)
    assert_same_graph(c._flat.diskann_params(), g2, "rebuilt")
    ids = np.concatenate([np.arange(700) + 1000, [5000, 5001, 5002]])
    for qi, r in enumerate(res):
        e_rows, e_d = expect(queries[qi:qi + 1], 10, 0, g2, data2)[0]
        assert np.array_equal(np.asarray(r.ids()), ids[e_rows.astype(np.int64)])


def test_collection_replacement_and_refusals(L):
    rng = np.random.default_rng(3)
    data = rng.standard_normal((300, 16)).astype(f32)
    c = coll(L, data, "FLAT-L2-PQ4")
    assert c._flat.pq_params(arrays=False)["M"] == 4
    c.build_index("DISKANN-L2", {"r": 4})
    assert c._flat.pq_params(arrays=False)["M"] == 0 and c._flat.diskann_params(arrays=False)["r"] == 4
    assert c.search(data[5], 3).index_mode() == "DISKANN-L2"
    c.build_index("FLAT-L2-RABITQ")
    assert c._flat.diskann_params(arrays=False)["r"] == 0 and c._flat.rabitq_params(arrays=False)["padded_dim"] == 16
    c.build_index("DISKANN-COS")
    p = c._flat.diskann_params(arrays=False)
    assert c._flat.rabitq_params(arrays=False)["padded_dim"] == 0 and (p["metric"], p["r"], p["l"]) == (COS, 16, 64) and p["alpha"] == float(f32(1.2))
    c.build_index("HNSW-L2", {"m": 4})
    assert c._flat.diskann_params(arrays=False)["r"] == 0 and c._flat.hnsw_params(arrays=False)["m"] == 4
    c.build_index("DISKANN-L2")
    assert c._flat.hnsw_params(arrays=False)["m"] == 0 and c._flat.diskann_params(arrays=False)["r"] == 16
    c.build_index("FLAT-L2")
    assert c._flat.diskann_params(arrays=False)["r"] == 0 and c.search(data[5], 3).index_mode() == "FLAT-L2"
    for mode in ("DISKANN-IP", "DISKANN-L2-PQ8", "DISKANN-IP-PQ8", "DISKANN-L2-SQ8", "DISKANN-COS-SQ8"):
        with pytest.raises(NotImplementedError):
            c.build_index(mode)
    with pytest.raises(ValueError, match="r must be greater than 0"):
        c.build_index("DISKANN-L2", {"r": 0})
    with pytest.raises(ValueError, match="alpha must be a finite value >= 1.0"):
        c.build_index("DISKANN-L2", {"alpha": 0.9})
    with pytest.raises(ValueError, match="unknown index build parameter 'ef'"):
        c.build_index("DISKANN-L2", {"ef": 3})
    for bad in ({"r": 65}, {"l": 4097}):
        with pytest.raises(NotImplementedError):
            c.build_index("DISKANN-L2", bad)
    empty = L.Collection("e", 16, device=0)
    with pytest.raises(ValueError, match="Empty database"):
        empty.build_index("DISKANN-L2")
