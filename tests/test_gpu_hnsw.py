"""GPU parity tests for HNSW-{IP,L2,COS} (HNSWIndex, src/index/hnsw.rs) through the C ABI and the Collection, against the restatement of
the HNSW rule block of include/lynse_hip.h (tests/hnsw_ref/hnsw_ref.c: levels, the bulk build and the search in plain C, every distance
computed afresh by the oracle's lo_compute_distance, unbounded heaps).  Levels, adjacency, entry point, result ids and f32 distance
bits are compared exactly; there are no tolerances."""
import numpy as np
import pytest

import hnsw_common as H
import oracle as O
from hnsw_common import assert_same_graph, check, combos_for, load, make_data, sweep

pytestmark = pytest.mark.gpu
IP, L2, COS = O.IP, O.L2, O.COS
NAME = {IP: "ip", L2: "l2", COS: "cosine"}
f32 = np.float32
PAD = H.PAD


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return H.build_ref(tmp_path_factory.mktemp("hnsw_ref"), oracle)


# -------------------------------------------------------------------- search over loaded graphs ----
@pytest.mark.parametrize("n,dim,m,kind", [(1, 3, 2, "gauss"), (2, 8, 4, "int"), (65, 20, 2, "dup"), (65, 128, 16, "gauss"), (65, 3, 4, "nonfinite"),
                                          (600, 8, 4, "gauss"), (600, 20, 16, "dup"), (600, 128, 2, "int"), (600, 771, 4, "gauss"),
                                          (600, 20, 4, "nonfinite"), (600, 3, 16, "int")])
def test_search_random_graphs(L, ref, n, dim, m, kind):
    rng = np.random.default_rng(n * 1000 + dim * 7 + m)
    data, queries = make_data(kind, rng, n, dim, 37)
    idx = L.FlatIndex(None, dim, device=0)
    idx.write(data)
    g = H.random_graph(rng, n, m)
    if n == 600 and m == 4:
        assert 3 <= int(g.levels.max()) + 1   # several levels: the descent is exercised
    for metric in (IP, L2, COS):
        sweep(idx, ref, data, g, metric, queries, combos_for(n))


def special_graphs(n, m):
    cap = 2 * m
    out = {"path": H.flat_graph(n, m, {i: [j for j in (i - 1, i + 1) if 0 <= j < n] for i in range(n)}),
           "star": H.flat_graph(n, m, {**{i: [0] for i in range(1, n)}, 0: list(range(1, min(n, cap + 1)))}),
           # node 1 has an empty list; the entry's component is {0, 1, 2}: counts < k
           "small_component": H.flat_graph(n, m, {0: [1, 2], 1: [], 2: [0]})}
    # pads inside a list and a neighbour named twice: the stored form drops both
    g = H.flat_graph(n, m, {i: [(i + 1) % n] for i in range(n)})
    g.adj0[:, 2] = g.adj0[:, 0]
    g.adj0[:, 0] = PAD
    g.adj0[:, 3] = g.adj0[:, 2]
    out["pads_and_repeats"] = g
    return out


@pytest.mark.parametrize("n,dim", [(65, 8), (600, 20)])
def test_search_special_graphs(L, ref, n, dim):
    rng = np.random.default_rng(n + dim)
    data, queries = make_data("gauss", rng, n, dim, 11)
    idx = L.FlatIndex(None, dim, device=0)
    idx.write(data)
    for name, g in special_graphs(n, 2).items():
        for metric in (IP, L2, COS):
            sweep(idx, ref, data, g, metric, queries, [(10, 10, 5), (10, 0, 11), (n + 3, n + 5, 2), (1, 1, 300)])
    # the path graph walks every node when ef covers them all
    g = special_graphs(n, 2)["path"]
    load(idx, g, L2)
    rows, dists, counts = idx.search_hnsw_batch_arrays(queries[:1], n, L2, n)
    assert int(counts[0]) == n and sorted(rows[0].tolist()) == list(range(n))
    p = idx.hnsw_params()
    assert (p["m"], p["n"], p["entry"], p["top_level"], p["n_upper"], p["metric"]) == (2, n, 0, 0, 0, L2)
    # the exported lists are the stored form
    g = special_graphs(n, 2)["pads_and_repeats"]
    load(idx, g, L2)
    a0 = idx.hnsw_params()["adj0"]
    assert np.array_equal(a0[:, 0], (np.arange(n) + 1) % n) and (a0[:, 1:] == PAD).all()


def test_graph_covers_the_first_rows_only(L, ref):
    """rule 6: rows appended after a load stay outside the graph"""
    rng = np.random.default_rng(5)
    data, queries = make_data("gauss", rng, 300, 16, 9)
    idx = L.FlatIndex(None, 16, device=0)
    idx.write(data)
    g = H.random_graph(rng, 200, 4)
    load(idx, g, L2)
    exp = H.ref_search(ref, data[:200], L2, g, queries, 10, 50)
    check(idx.search_hnsw_batch_arrays(queries, 10, L2), exp, 10, L2, "first rows")
    idx.write(rng.standard_normal((50, 16)).astype(f32))
    check(idx.search_hnsw_batch_arrays(queries, 10, L2), exp, 10, L2, "after an append")
    assert idx.hnsw_params(arrays=False)["n"] == 200
    idx.drop_hnsw()
    assert idx.hnsw_params()["m"] == 0 and idx.hnsw_params()["n"] == 0
    with pytest.raises(ValueError, match="no HNSW index"):
        idx.search_hnsw_batch_arrays(queries, 10, L2)


# ------------------------------------------------------------------------------------------ build ----
@pytest.mark.parametrize("n,dim,m,efc,kind", [(1, 8, 2, 8, "gauss"), (17, 24, 4, 128, "gauss"), (17, 8, 16, 8, "dup"), (600, 24, 4, 8, "gauss"),
                                              (600, 100, 16, 128, "gauss"), (600, 8, 2, 128, "dup"), (600, 24, 2, 8, "int"),
                                              (1500, 24, 16, 8, "dup"), (1500, 100, 4, 128, "gauss")])
def test_build_equals_the_restatement(L, ref, n, dim, m, efc, kind):
    rng = np.random.default_rng(n + dim + m + efc)
    data, queries = make_data(kind, rng, n, dim, 23)
    idx = L.FlatIndex(None, dim, device=0)
    idx.write(data)
    for metric in (IP, L2, COS):
        seed = 42 + metric
        levels = H.ref_levels(ref, seed, m, None, n)
        g = H.ref_build(ref, data, metric, m, efc, levels)
        idx.build_hnsw(metric, m, efc, 50, None, seed)
        p = idx.hnsw_params()
        assert (p["metric"], p["m"], p["ef_search"], p["n"]) == (metric, m, 50, n)
        assert_same_graph(p, g, (NAME[metric], n, dim, m, efc, kind))
        combos = [(10, 0, 23), (1, 1, 5), (n + 3, n + 5, 2)]
        first = [idx.search_hnsw_batch_arrays(queries[np.arange(nq) % 23], k, metric, efq) for k, efq, nq in combos]
        for (k, efq, nq), got in zip(combos, first):
            check(got, H.ref_search(ref, data, metric, g, queries[np.arange(nq) % 23], k, max(efq or 50, k)), k, metric, "built")
        # build -> export -> load -> search: the same results
        idx.load_hnsw(metric, p["m"], p["ef_search"], p["levels"], p["adj0"], p["upper_node"], p["upper_level"], p["upper_adj"], p["entry"])
        assert_same_graph(idx.hnsw_params(), g, "reloaded")
        for (k, efq, nq), got in zip(combos, first):
            again = idx.search_hnsw_batch_arrays(queries[np.arange(nq) % 23], k, metric, efq)
            assert all(np.array_equal(a.view(np.uint32) if a.dtype == f32 else a, b.view(np.uint32) if b.dtype == f32 else b) for a, b in zip(again, got))


def test_build_with_a_level_cap_and_nan_rows(L, ref):
    """NaN rows: every distance to and from them is +inf from the moment it is computed.  (Rows with infinite elements are left out of
    the build tests: as queries of the exact search, which is where the candidate lists come from, their order is not pinned.)"""
    rng = np.random.default_rng(77)
    data, queries = make_data("gauss", rng, 400, 12, 9)
    data[rng.integers(0, 400, 50), rng.integers(0, 12, 50)] = np.nan
    queries[2, 3] = np.nan
    idx = L.FlatIndex(None, 12, device=0)
    idx.write(data)
    for metric, cap in ((L2, 1), (IP, 0), (COS, None)):
        levels = H.ref_levels(ref, 7, 3, cap, 400)
        g = H.ref_build(ref, data, metric, 3, 16, levels)
        idx.build_hnsw(metric, 3, 16, 20, cap, 7)
        assert_same_graph(idx.hnsw_params(), g, (NAME[metric], cap))
        check(idx.search_hnsw_batch_arrays(queries, 10, metric), H.ref_search(ref, data, metric, g, queries, 10, 20), 10, metric, "nan build")


# ------------------------------------------------------------------------------------- Collection ----
def coll(L, data, mode, params=None, ids=None):
    c = L.Collection("c", data.shape[1], device=0)
    c.add_items(data, np.arange(data.shape[0]) + 1000 if ids is None else ids)
    c.commit()
    c.build_index(mode, params)
    return c


def test_collection_recall_case(L, ref, oracle):
    """the recall case of tests/test_hnsw_modes.py on the GPU: equal to the restatement, hence at its recall (>= 0.90)"""
    data, queries, g, res, _ = H.recall_case(ref)
    c = coll(L, data, "HNSW-L2", ids=np.arange(4096))
    assert_same_graph(c._flat.hnsw_params(), g, "recall case")
    out = c.batch_search(queries, 10)
    hit = 0
    for qi, r in enumerate(out):
        assert r.index_mode() == "HNSW-L2"
        assert np.array_equal(np.asarray(r.ids()), res[qi][0].astype(np.int64))
        assert np.array_equal(np.asarray(r.distances(), f32).view(np.uint32), res[qi][1].view(np.uint32))
        e_ids, _ = oracle.canonical_topk(queries[qi], data, 10, L2, O.IPFORM_SINGLE)
        hit += len(set(int(x) for x in r.ids()) & set(int(x) for x in e_ids))
    print(f"recall@10 on the GPU = {hit / 1000:.4f}")
    assert hit / 1000 >= 0.90


@pytest.mark.parametrize("mode,metric", [("HNSW-IP", IP), ("hnsw-l2", L2), ("HNSW-COS", COS), ("HNSW-COSINE", COS)])
def test_collection_search_paths(L, ref, oracle, mode, metric):
    rng = np.random.default_rng(11 + metric)
    data, queries = make_data("gauss", rng, 700, 24, 12)
    opts = {"m": 4, "ef_construction": 32, "ef_search": 20, "nprobe": 5}   # (nprobe: another family's key, ignored)
    c = coll(L, data, mode, opts)
    g = H.ref_build(ref, data, metric, 4, 32, H.ref_levels(ref, 42, 4, None, 700))
    assert_same_graph(c._flat.hnsw_params(), g, mode)

    def expect(q, k, ef):
        return H.ref_search(ref, data, metric, g, q, k, max(ef, k))

    def same(results, exp, off=1000):
        for r, (e_rows, e_d) in zip(results, exp):
            assert r.index_mode() == mode.upper()
            assert np.array_equal(np.asarray(r.ids()), e_rows.astype(np.int64) + off)
            assert np.array_equal(np.asarray(r.distances(), f32).view(np.uint32), e_d.view(np.uint32))

    same(c.batch_search(queries, 10), expect(queries, 10, 20))
    same([c.search(queries[0], 5)], expect(queries[:1], 5, 20))
    same(c.batch_search(queries, 10, nprobe=64), expect(queries, 10, 64))   # nprobe > 0 is the query-time ef
    prof = c.search_profile(queries[0], 10)
    assert prof["profile"]["index_path"] == "ann_index" and prof["items"]["index"] == mode.upper()
    assert prof["profile"]["device"]["hnsw"]["scored"] > 0
    # tombstones: k' = k + tombstones through the graph, then the filter
    dead = [int(x) + 1000 for x in expect(queries[:1], 3, 20)[0][0][:2]]
    c.delete_items(dead)
    exp = expect(queries, 12, 20)
    for r, (e_rows, e_d) in zip(c.batch_search(queries, 10), exp):
        keep = ~np.isin(e_rows + 1000, dead)
        assert np.array_equal(np.asarray(r.ids()), (e_rows[keep] + 1000).astype(np.int64)[:10])
    c.restore_items(dead)
    # a subset takes the exact filtered scan
    subset = np.arange(0, 700, 3)
    for qi, r in enumerate(c.batch_search(queries, 7, subset=subset)):
        e_ids, e_d = oracle.canonical_topk(queries[qi], data[subset], 7, metric, O.IPFORM_SINGLE)
        assert np.array_equal(np.asarray(r.ids()), subset[e_ids.astype(np.int64)] + 1000)
        assert np.array_equal(np.asarray(r.distances(), f32).view(np.uint32), e_d.view(np.uint32))
    # rows added and flushed: the graph is rebuilt and finds them
    extra = (queries[:3] + f32(1e-3)).astype(f32)
    c.add_items(extra, [5000, 5001, 5002])
    c.commit()
    data2 = np.concatenate([data, extra])
    g2 = H.ref_build(ref, data2, metric, 4, 32, H.ref_levels(ref, 42, 4, None, 703))
    res = c.batch_search(queries[:3], 10)
    assert_same_graph(c._flat.hnsw_params(), g2, "rebuilt")
    ids = np.concatenate([np.arange(700) + 1000, [5000, 5001, 5002]])
    for qi, r in enumerate(res):
        e_rows, e_d = H.ref_search(ref, data2, metric, g2, queries[qi:qi + 1], 10, 20)[0]
        assert np.array_equal(np.asarray(r.ids()), ids[e_rows.astype(np.int64)])
        if metric != IP:
            assert 5000 + qi in [int(x) for x in r.ids()]


def test_collection_replacement_and_refusals(L):
    rng = np.random.default_rng(3)
    data = rng.standard_normal((300, 16)).astype(f32)
    c = coll(L, data, "FLAT-L2-PQ4")
    assert c._flat.pq_params(arrays=False)["M"] == 4
    c.build_index("HNSW-L2", {"m": 4})
    assert c._flat.pq_params(arrays=False)["M"] == 0 and c._flat.hnsw_params(arrays=False)["m"] == 4
    assert c.search(data[5], 3).index_mode() == "HNSW-L2"
    c.build_index("FLAT-L2-RABITQ")
    assert c._flat.hnsw_params(arrays=False)["m"] == 0 and c._flat.rabitq_params(arrays=False)["padded_dim"] == 16
    c.build_index("HNSW-IP")
    assert c._flat.rabitq_params(arrays=False)["padded_dim"] == 0 and c._flat.hnsw_params(arrays=False)["metric"] == IP
    c.build_index("FLAT-IP")
    assert c._flat.hnsw_params(arrays=False)["m"] == 0
    for mode in ("HNSW-IP-SQ8", "HNSW-L2-SQ8", "DISKANN-IP", "HNSW-CORRELATION"):
        with pytest.raises(NotImplementedError):
            c.build_index(mode)
    with pytest.raises(ValueError, match="m must be greater than 0"):
        c.build_index("HNSW-L2", {"m": 0})
    with pytest.raises(ValueError, match="unknown index build parameter 'ef'"):
        c.build_index("HNSW-L2", {"ef": 3})
    for bad in ({"m": 1}, {"m": 33}, {"ef_construction": 4097}, {"ef_search": 4097}):
        with pytest.raises(NotImplementedError):
            c.build_index("HNSW-L2", bad)
    empty = L.Collection("e", 16, device=0)
    with pytest.raises(ValueError, match="Empty database"):
        empty.build_index("HNSW-L2")


# ------------------------------------------------------------------------------------------ C ABI ----
def test_cabi_refusals(L):
    rng = np.random.default_rng(9)
    data = rng.standard_normal((100, 16)).astype(f32)
    q = data[:3]
    g = H.random_graph(rng, 100, 4)
    idx = L.FlatIndex(None, 16, device=0)
    idx.write(data)
    unsupported, invalid = NotImplementedError, ValueError
    for metric in ("hamming", "jaccard", "dice", "tanimoto", "l1", "chebyshev", "canberra", "bray_curtis"):
        with pytest.raises(unsupported):
            idx.build_hnsw(metric)
    for kw in ({"m": 1}, {"m": 33}, {"ef_construction": 0}, {"ef_construction": 4097}, {"ef_search": 0}, {"ef_search": 4097}):
        with pytest.raises(unsupported):
            idx.build_hnsw(L2, **kw)
    with pytest.raises(invalid, match="no HNSW index"):
        idx.search_hnsw_batch_arrays(q, 3, L2)
    load(idx, g, L2)
    with pytest.raises(invalid, match="another metric"):
        idx.search_hnsw_batch_arrays(q, 3, IP)
    with pytest.raises(unsupported):
        idx.search_hnsw_batch_arrays(q, 3, "hamming")
    with pytest.raises(unsupported):
        idx.search_hnsw_batch_arrays(q, 3, L2, 4097)
    rows, dists, counts = idx.search_hnsw_batch_arrays(q, 0, L2)
    assert counts.tolist() == [0, 0, 0]
    # load validation
    def bad(**kw):
        a = {"levels": g.levels.copy(), "adj0": g.adj0.copy(), "upper_node": g.upper_node.copy(), "upper_level": g.upper_level.copy(),
             "upper_adj": g.upper_adj.copy(), "entry": g.entry}
        a.update(kw)
        return a

    cases = []
    a0 = g.adj0.copy(); a0[3, 0] = 100
    cases.append(bad(adj0=a0))                                   # a neighbour >= n
    lo = int(np.nonzero(g.levels == 0)[0][0])
    ua = g.upper_adj.copy(); ua[0, 0] = lo
    cases.append(bad(upper_adj=ua))                              # a level-0 node in an upper list
    cases.append(bad(entry=lo))                                  # the entry is not on the top level
    cases.append(bad(entry=100))
    cases.append(bad(upper_node=g.upper_node[::-1].copy()))      # not ascending
    lv = g.levels.copy(); lv[lo] = 1
    cases.append(bad(levels=lv))                                 # the upper lists do not match the levels
    for a in cases:
        with pytest.raises(invalid):
            idx.load_hnsw(L2, 4, 50, a["levels"], a["adj0"], a["upper_node"], a["upper_level"], a["upper_adj"], a["entry"])
    with pytest.raises(unsupported):
        idx.load_hnsw(L2, 33, 50, g.levels, np.zeros((100, 66), np.uint32), g.upper_node, g.upper_level, np.zeros((g.upper_node.size, 33), np.uint32), g.entry)
    big = H.random_graph(rng, 101, 4)
    with pytest.raises(invalid, match="more rows"):
        load(idx, big, L2)

    # handles the graph is not defined for
    h16 = L.FlatIndex(None, 16, device=0, dtype="f16")
    h16.write(data)
    packed = L.FlatIndex(None, 64, device=0)
    packed.write_packed(rng.integers(0, 1 << 62, (100, 1), dtype=np.uint64))
    mapped = L.FlatIndex(None, 16, device=0)
    mapped.write(data)
    mapped.set_row_map(2, 1)
    for h in (h16, packed, mapped):
        with pytest.raises(unsupported):
            h.build_hnsw(L2)
    for h in (h16, mapped):
        with pytest.raises(unsupported):
            load(h, g, L2)



def test_refused_while_tickets_are_outstanding(L):
    """the HNSW entries hold the handle's lock exclusively: with a batch in flight (a shard large enough that submit pipelines it) they
    are refused, and answer again after the wait"""
    import torch

    rng = np.random.default_rng(10)
    data = rng.standard_normal((30_000, 32)).astype(f32)
    q = data[:8] + f32(0.01)
    idx = L.FlatIndex(None, 32, device=0)
    idx.write(data)
    idx.finalize()
    load(idx, H.random_graph(rng, 100, 4), L2)
    idx.search_batch_arrays(q, 3, "l2")
    idx.prepare("l2", 8)
    dq = torch.from_numpy(q).cuda()
    d_rows, d_d, d_c = torch.zeros((8, 3), dtype=torch.int64).cuda(), torch.zeros((8, 3)).cuda(), torch.zeros(8, dtype=torch.int32).cuda()
    t = idx.search_submit(dq, 3, L2, d_rows, d_d, d_c)
    try:
        with pytest.raises(NotImplementedError, match="in flight"):
            idx.search_hnsw_batch_arrays(q, 3, L2)
        with pytest.raises(NotImplementedError, match="in flight"):
            idx.build_hnsw(L2)
    finally:
        t.wait()
    assert all(1 <= c <= 3 for c in idx.search_hnsw_batch_arrays(q, 3, L2)[2].tolist())
