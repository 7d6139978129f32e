"""GPU tests of the incremental HNSW insert (rule 7 of the HNSW block of include/lynse_hip.h): build over the first rows, append,
extend — and the exported graph equals the restatement's build over all rows (tests/hnsw_ref/hnsw_ref.c), array for array, stored
order included.  There are no tolerances.  Unless a test says otherwise (new rows) * ef_construction < (old rows), so mode 0 takes the
incremental path, and the stats say so."""
import numpy as np
import pytest

import hnsw_common as H
import oracle as O
from hnsw_common import assert_same_graph, check, levels_py, make_data
from hnsw_extend_common import extend_steps, same_as_fresh_build

pytestmark = pytest.mark.gpu
IP, L2, COS = O.IP, O.L2, O.COS
NAME = H.NAME
f32 = np.float32


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle):
    return H.build_ref(tmp_path_factory.mktemp("hnsw_ref_extend"), oracle)


def searches_equal(idx, ref, data, g, metric, queries, ef_search=50):
    n = data.shape[0]
    for k, efq, nq in [(10, 0, queries.shape[0]), (1, 1, 5), (n + 3, n + 5, 2)]:
        q = queries[np.arange(nq) % queries.shape[0]]
        check(idx.search_hnsw_batch_arrays(q, k, metric, efq), H.ref_search(ref, data, metric, g, q, k, max(efq or ef_search, k)), k, metric,
              (NAME[metric], n, k, efq))


# 1
@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_basic(L, ref, metric):
    rng = np.random.default_rng(100 + metric)
    data, queries = make_data("gauss", rng, 2037, 24, 23)
    idx, g, stats = extend_steps(L, ref, data, [2000, 2037], metric, 4, 16, seed=42 + metric, what="basic")
    st = stats[0]
    assert st["new_items"] >= 37 and 1 <= st["researched"] < 2000 and st["dirty_lists"] >= 37 and st["total_us"] > 0.0
    same_as_fresh_build(L, idx, data, metric, 4, 16, seed=42 + metric)
    searches_equal(idx, ref, data, g, metric, queries)
    H.scored_sweep(idx, ref, data, g, metric, queries, [(10, 0, 23), (5, 64, 7)])


# 2
def test_top_level_moves(L, ref):
    lv = levels_py(42, 4, None, 3000)
    i_star = int(np.nonzero(lv == lv.max())[0][0])
    assert lv[:i_star].max() < lv.max() and 21 * 16 < i_star
    n0, n1 = i_star, i_star + 21
    rng = np.random.default_rng(2)
    data, queries = make_data("gauss", rng, n1, 16, 11)
    idx = L.FlatIndex(None, 16, device=0)
    idx.write(data[:n0])
    idx.build_hnsw(L2, 4, 16, 50, None, 42)
    before = idx.hnsw_params(arrays=False)
    idx.write(data[n0:])
    idx.extend_hnsw()
    after = idx.hnsw_params()
    assert idx.hnsw_extend_stats()["path"] == 0
    assert after["entry"] == i_star != before["entry"] and after["top_level"] == int(lv.max()) > before["top_level"]
    g = H.ref_build(ref, data, L2, 4, 16, lv[:n1])
    assert_same_graph(after, g, "top level moves")
    searches_equal(idx, ref, data, g, L2, queries)


# 3
@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_many_levels(L, ref, metric):
    rng = np.random.default_rng(30 + metric)
    data, queries = make_data("gauss", rng, 650, 16, 11)
    lv = levels_py(7, 2, None, 650)
    assert int(lv[:600].max()) >= 4 and int((lv[600:] >= 1).sum()) >= 10
    idx, g, stats = extend_steps(L, ref, data, [600, 650], metric, 2, 8, seed=7, what="many levels")
    assert stats[0]["reselected"] > 0 and stats[0]["new_items"] == 50 + int(lv[600:].sum())
    searches_equal(idx, ref, data, g, metric, queries)


# 4
@pytest.mark.parametrize("sizes", [[1, 5, 25], [10, 15]])
def test_short_lists(L, ref, sizes):
    rng = np.random.default_rng(sizes[0])
    data, queries = make_data("gauss", rng, sizes[-1], 12, 7)
    for metric in (IP, L2, COS):
        idx, g, _ = extend_steps(L, ref, data, sizes, metric, 4, 16, mode=1, what="short lists")
        searches_equal(idx, ref, data, g, metric, queries)


# 5
@pytest.mark.parametrize("kind", ["int", "dup", "copies"])
def test_ties(L, ref, kind):
    rng = np.random.default_rng(len(kind))
    data, queries = make_data("dup" if kind == "copies" else kind, rng, 1530, 8, 11)
    if kind == "copies":   # every appended row duplicates an existing one
        data[1500:] = data[rng.integers(0, 1500, 30)]
    for metric in (IP, L2, COS):
        idx, g, _ = extend_steps(L, ref, data, [1500, 1530], metric, 4, 8, what=("ties", kind))
        searches_equal(idx, ref, data, g, metric, queries)


# 6
@pytest.mark.parametrize("where", ["old", "new", "both"])
def test_nan_rows(L, ref, where):
    rng = np.random.default_rng(60 + len(where))
    data, queries = make_data("gauss", rng, 410, 12, 9)
    if where in ("old", "both"):
        data[rng.integers(0, 400, 40), rng.integers(0, 12, 40)] = np.nan
    if where in ("new", "both"):
        data[[401, 405, 409], [0, 5, 11]] = np.nan
    for metric in (IP, L2, COS):
        idx, g, _ = extend_steps(L, ref, data, [400, 410], metric, 3, 16, seed=7, ef_search=20, what=("nan", where))
        check(idx.search_hnsw_batch_arrays(queries, 10, metric), H.ref_search(ref, data, metric, g, queries, 10, 20), 10, metric, "nan extend")


# 7
@pytest.mark.parametrize("n0,dim,add", [(1500, 2048, 45), (1000, 7, 20), (1000, 33, 20)])
def test_scan_tiles_and_odd_widths(L, ref, n0, dim, add):
    """D 2048: 160 KiB / (4 D) = 20 new rows per tile, 45 new rows in three tiles; D 7 and 33: the tails of the single-row form"""
    rng = np.random.default_rng(dim)
    data, queries = make_data("gauss", rng, n0 + add, dim, 5)
    for metric in (IP, L2, COS):
        idx, g, _ = extend_steps(L, ref, data, [n0, n0 + add], metric, 4, 8, what=("width", dim))
        check(idx.search_hnsw_batch_arrays(queries, 10, metric), H.ref_search(ref, data, metric, g, queries, 10, 50), 10, metric, "width")


# 8
def test_repeated_extends(L, ref):
    rng = np.random.default_rng(8)
    data, queries = make_data("gauss", rng, 1272, 24, 11)
    idx, g, _ = extend_steps(L, ref, data, [1200, 1201, 1208, 1272], L2, 4, 16, what="repeated")
    before = idx.hnsw_params()
    idx.extend_hnsw()
    st = idx.hnsw_extend_stats()
    assert st["path"] == 2 and (st["rows_before"], st["rows_after"], st["new_items"], st["researched"]) == (1272, 1272, 0, 0)
    after = idx.hnsw_params()
    assert all(np.array_equal(before[key], after[key]) for key in before)
    searches_equal(idx, ref, data, g, L2, queries)


# 9
@pytest.mark.parametrize("kind", ["gauss", "dup"])
def test_staged_plan(L, ref, kind):
    """as tests/test_gpu_hnsw_limits.py sizes it: 600 rows over a plan of cap 256, ask = 64 = cap / 4 the largest accepted"""
    rng = np.random.default_rng(90 + len(kind))
    data, queries = make_data(kind, rng, 600, 24, 11)
    for metric in (IP, L2, COS):
        idx, g, _ = extend_steps(L, ref, data, [595, 600], metric, 2, 63, mode=1, plan=(256, 2, 256), what=("staged", kind))
        searches_equal(idx, ref, data, g, metric, queries)
    # ef_construction 64 over the same plan: refused by extend as by build, the old graph untouched
    idx = L.FlatIndex(None, 24, device=0)
    idx.write(data[:595])
    idx.build_hnsw(L2, 2, 64, 50, None, 42)
    idx.set_plan(256, 2, 256)
    g = H.ref_build(ref, data[:595], L2, 2, 64, levels_py(42, 2, None, 595))
    assert_same_graph(idx.hnsw_params(), g, "before the refused extend")
    idx.write(data[595:])
    for mode in (0, 1):
        with pytest.raises(NotImplementedError, match="a quarter of the scan's candidate capacity"):
            idx.extend_hnsw(mode)
    assert idx.hnsw_params(arrays=False)["n"] == 595
    assert_same_graph(idx.hnsw_params(), g, "after the refused extend")
    searches_equal(idx, ref, data[:595], g, L2, queries)


# 10
def test_work_is_local(L, ref):
    rng = np.random.default_rng(10)
    n0, dim = 2000, 16
    cluster = np.arange(n0 + 10) % 8
    cluster[n0:] = 3
    centres = np.zeros((8, dim), f32)
    centres[:, 0] = 100.0 * np.arange(8)
    data = (centres[cluster] + rng.standard_normal((n0 + 10, dim))).astype(f32)
    idx, g, stats = extend_steps(L, ref, data, [n0, n0 + 10], L2, 4, 16, what="local")
    lv = levels_py(42, 4, None, n0)
    # level 0: only the 250 rows of cluster 3 can see a new row within their 17 nearest; above, every old member may
    assert 1 <= stats[0]["researched"] <= 250 + int(lv.sum()), stats[0]
    queries = data[rng.integers(0, n0, 9)] + f32(0.1)
    searches_equal(idx, ref, data, g, L2, queries)


# 11
def test_auto_fallback(L, ref):
    rng = np.random.default_rng(11)
    data, queries = make_data("gauss", rng, 500, 16, 7)
    idx, g, stats = extend_steps(L, ref, data, [400, 500], L2, 4, 16, path=1, what="fallback")
    assert stats[0]["researched"] == 0
    searches_equal(idx, ref, data, g, L2, queries)
    # one row fewer than the rule asks for: incremental
    extend_steps(L, ref, data, [400, 424], L2, 4, 16, path=0, what="below the rule")
    extend_steps(L, ref, data, [400, 425], L2, 4, 16, path=1, what="at the rule")


# 12
def test_refusals(L, ref):
    import torch

    rng = np.random.default_rng(12)
    data, queries = make_data("gauss", rng, 320, 16, 5)
    idx = L.FlatIndex(None, 16, device=0)
    idx.write(data[:300])
    with pytest.raises(ValueError, match="no HNSW index"):
        idx.extend_hnsw()
    H.load(idx, H.random_graph(rng, 200, 4), L2)
    with pytest.raises(NotImplementedError, match="loaded graph"):
        idx.extend_hnsw()
    assert idx.hnsw_params(arrays=False)["n"] == 200
    idx.build_hnsw(L2, 4, 16, 50, None, 42)
    idx.write(data[300:])
    with pytest.raises(ValueError, match="mode"):
        idx.extend_hnsw(7)
    assert idx.hnsw_params(arrays=False)["n"] == 300
    idx.extend_hnsw(1)
    g = H.ref_build(ref, data, L2, 4, 16, levels_py(42, 4, None, 320))
    assert_same_graph(idx.hnsw_params(), g, "after the refusals")
    # a mutation drops the graph, and extend says so
    idx.update_rows([3], data[:1])
    assert idx.hnsw_params(arrays=False)["m"] == 0
    with pytest.raises(ValueError, match="no HNSW index"):
        idx.extend_hnsw()
    # a ticket outstanding: as the build
    big = L.FlatIndex(None, 32, device=0)
    rows = rng.standard_normal((30_000, 32)).astype(f32)
    big.write(rows[:29_990])
    big.finalize()
    big.build_hnsw(L2, 4, 8, 50, None, 42)
    big.write(rows[29_990:])
    big.finalize()
    q = rows[:8] + f32(0.01)
    big.search_batch_arrays(q, 3, "l2")
    big.prepare("l2", 8)
    dq = torch.from_numpy(q).cuda()
    d_rows, d_d, d_c = torch.zeros((8, 3), dtype=torch.int64).cuda(), torch.zeros((8, 3)).cuda(), torch.zeros(8, dtype=torch.int32).cuda()
    t = big.search_submit(dq, 3, L2, d_rows, d_d, d_c)
    try:
        with pytest.raises(NotImplementedError, match="in flight"):
            big.extend_hnsw()
    finally:
        t.wait()
    assert big.hnsw_params(arrays=False)["n"] == 29_990
    big.extend_hnsw()
    assert big.hnsw_params(arrays=False)["n"] == 30_000 and big.hnsw_extend_stats()["path"] == 0


# 13
def test_collection_and_named_field(L, ref):
    rng = np.random.default_rng(13)
    n0, add, dim = 1200, 30, 24
    data, queries = make_data("gauss", rng, n0 + add, dim, 9)
    ids = (np.arange(n0 + add) + 1000).tolist()
    fields = [{"g": int(i % 100)} for i in range(n0 + add)]
    opts = {"m": 4, "ef_construction": 16, "ef_search": 20}
    fdata, fq = np.roll(data, 1, axis=1).copy(), np.roll(queries, 1, axis=1).copy()   # the field's vectors: another set, row for row

    def coll(first):
        c = L.Collection("c", dim, device=0)
        c.add_items(data[:first], ids[:first], fields=fields[:first])
        c.commit()
        c.build_index("HNSW-L2", opts)
        c.create_vector_field("v", dim, "l2")
        c.add_named_vectors("v", fdata[:first], ids[:first])
        c.build_vector_field_index("v", "HNSW-L2", opts)
        return c

    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(np.asarray(x.ids()), np.asarray(y.ids()))
            assert np.array_equal(np.asarray(x.distances(), f32).view(np.uint32), np.asarray(y.distances(), f32).view(np.uint32))

    whole, grown = coll(n0 + add), coll(n0)
    grown.add_items(data[n0:], ids[n0:], fields=fields[n0:])
    grown.commit()
    same(grown.batch_search(queries, 10), whole.batch_search(queries, 10))
    st = grown._flat.hnsw_extend_stats()
    assert st["path"] == 0 and (st["rows_before"], st["rows_after"]) == (n0, n0 + add)
    g = H.ref_build(ref, data, L2, 4, 16, levels_py(42, 4, None, n0 + add))
    assert_same_graph(grown._flat.hnsw_params(), g, "collection")
    assert grown.batch_search(queries[:1], 5)[0].index_mode() == "HNSW-L2"
    grown.add_named_vectors("v", fdata[n0:], ids[n0:])
    same(grown.batch_search_vector_field("v", fq, 10), whole.batch_search_vector_field("v", fq, 10))
    f = grown._vfields["v"]
    st = f.flat.hnsw_extend_stats()
    assert st["path"] == 0 and f.hnsw_rows == n0 + add == st["rows_after"]
    for key, val in whole._vfields["v"].flat.hnsw_params().items():
        assert np.array_equal(f.flat.hnsw_params()[key], val), key
    # tombstones and where= take the exact filtered scan: unchanged by how the graph came to be
    same(grown.batch_search(queries, 10, where="g < 60"), whole.batch_search(queries, 10, where="g < 60"))
    same(grown.batch_search_vector_field("v", fq, 10, where="g < 60"), whole.batch_search_vector_field("v", fq, 10, where="g < 60"))
    for c in (grown, whole):
        c.delete_items(ids[5:40] + ids[n0 + 2:n0 + 9])
    same(grown.batch_search(queries, 10), whole.batch_search(queries, 10))
    same(grown.batch_search_vector_field("v", fq, 10), whole.batch_search_vector_field("v", fq, 10))
