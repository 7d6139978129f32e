"""GPU parity tests for the approximate flat search (`search(approx=True, eps=...)`; THE APPROXIMATE FLAT SEARCH block of
include/lynse_hip.h) through FlatIndex.search_approx and the Collection, against the restatement of the four paths
(tests/approx_ref/approx_ref.c, checked on its own in tests/test_approx_modes.py).  Parity is exact: ids equal and f32 distance bits
equal; there are no tolerances.  The sizes are the smallest that reach each path: big = dim > 16 and n > 65,536."""
import numpy as np
import pytest

from approx_common import BRAY, CANB, CHEB, COS, IP, L1, L2, NAME, build_ref, same_answer

pytestmark = pytest.mark.gpu
f32 = np.float32
ADDITIVE = [L1, CHEB, CANB, BRAY]
BIG_N = 65537


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("approx_ref"))


def index_of(L, data):
    idx = L.FlatIndex(None, data.shape[1], device=0)
    idx.write(np.ascontiguousarray(data, f32))
    return idx


def check(idx, ref, q, data, k, metric, eps, want_path=None):
    """one approximate search against the restatement -> (the restatement's answer, what the library says ran)"""
    rows, dists, info = idx.search_approx(q, k, NAME[metric], eps)
    ans = ref.search(q, data, k, metric, eps)
    same_answer(rows, dists, ans)
    assert {x: info[x] for x in ans.info} == ans.info, (info, ans.info)
    if want_path is not None:
        assert info["path"] == want_path
    return ans, info


def norm_cache_data():
    """flat_mmap.rs:6325-6343: 96 x 32, row 5 zero, the query is row 17"""
    i, j = np.arange(96)[:, None], np.arange(32)[None, :]
    data = (((i * 131 + j * 17 + (i * j * 7) % 19) % 997).astype(f32) / f32(997.0) - f32(0.5) + i.astype(f32) * f32(1e-5)).astype(f32)
    data[5] = 0.0
    return data, data[17].copy()


@pytest.fixture(scope="module")
def big43():
    rng = np.random.default_rng(43)
    return (rng.random((BIG_N, 43), dtype=f32) - f32(0.3)).astype(f32)


@pytest.fixture(scope="module")
def big43_idx(L, big43):
    return index_of(L, big43)


# ---- path 1: l2 and cosine, the norm-cached full scan -------------------------------------------------------------------------------
def test_path1_reference_data(L, ref):
    data, q = norm_cache_data()
    idx = index_of(L, data)
    for metric in (L2, COS):
        for k in (1, 5, 50):
            ans, _ = check(idx, ref, q, data, k, metric, 1e-8, want_path=1)
        assert ans.rows[0] == 17
    exact = idx.search_batch_arrays(q[None], 5, "l2")
    assert np.array_equal(exact[0][0], idx.search_approx(q, 5, "l2", 1e-8)[0])   # (:6352-6357: the ids of the exact search)
    # a query equal to a row under l2: the expansion may go below zero and clamps to 0.0, never negative
    rows, dists, _ = idx.search_approx(q, 3, "l2", 1e-4)
    assert rows[0] == 17 and dists[0] >= 0.0 and np.all(dists >= 0.0)
    # cosine: the zero row scores 1.0, a zero query answers rows 0 .. k - 1 at 1.0
    ans = ref.search(q, data, 96, COS, 1e-4)
    rows, dists, _ = idx.search_approx(q, 96, "cosine", 1e-4)
    same_answer(rows, dists, ans)
    assert dists[rows.tolist().index(5)] == 1.0
    rows, dists, info = idx.search_approx(np.zeros(32, f32), 7, "cosine", 1e-4)
    assert rows.tolist() == list(range(7)) and dists.tolist() == [1.0] * 7 and info["path"] == 1
    same_answer(rows, dists, ref.search(np.zeros(32, f32), data, 7, COS, 1e-4))


@pytest.mark.parametrize("shape", [(4095, 40), (4096, 40), (4097, 40), (5000, 43)])
def test_path1_at_the_ip_form_threshold(L, ref, shape):
    """the dot product takes the single-row form below 4,096 rows and the batch-of-8 form from there on; 43: a tail of three"""
    rng = np.random.default_rng(shape[0])
    data = (rng.random(shape, dtype=f32) - f32(0.4)).astype(f32)
    data[11] = 0.0
    q = (rng.random(shape[1], dtype=f32) - f32(0.4)).astype(f32)
    idx = index_of(L, data)
    for metric in (L2, COS):
        for k in (1, 5, 50):
            check(idx, ref, q, data, k, metric, 1e-4, want_path=1)
    check(idx, ref, data[3], data, 5, L2, 1e-4, want_path=1)   # a query equal to a row


# ---- path 2: every row exactly -----------------------------------------------------------------------------------------------------
def test_path2_ip_is_the_single_row_form(L, ref):
    rng = np.random.default_rng(2)
    data = rng.standard_normal((4096, 128)).astype(f32)
    idx = index_of(L, data)
    differs = 0
    for s in range(4):
        q = rng.standard_normal(128).astype(f32)
        ans, _ = check(idx, ref, q, data, 10, IP, 1e-4, want_path=2)
        e_rows, e_dists, _ = idx.search_batch_arrays(q[None], 10, "ip")   # the exact search: the batch-of-8 form from 4,096 rows on
        differs += int(np.any(e_dists[0].view(np.uint32) != ans.dists.view(np.uint32)))
    assert differs > 0   # the two forms differ in the last ulp somewhere: the approximate path really scores in the single-row form


@pytest.mark.parametrize("metric", ADDITIVE)
def test_path2_additive(L, ref, metric):
    rng = np.random.default_rng(metric)
    data = (rng.random((3000, 43), dtype=f32) + f32(0.01)).astype(f32)
    q = (rng.random(43, dtype=f32) + f32(0.01)).astype(f32)
    idx = index_of(L, data)
    for k in (1, 10):
        check(idx, ref, q, data, k, metric, 1e-4, want_path=2)


def test_path2_at_the_size_edges(L, ref, big43):
    """n = 65,536 at dim 43 and n = 65,537 at dim 16 are still path 2"""
    data = big43[:65536]
    idx = index_of(L, data)
    for metric in (IP, L1):
        check(idx, ref, big43[65536], data, 10, metric, 1e-4, want_path=2)
    rng = np.random.default_rng(16)
    d16 = (rng.random((BIG_N, 16), dtype=f32) - f32(0.5)).astype(f32)
    idx = index_of(L, d16)
    for metric in (IP, BRAY):
        check(idx, ref, d16[9] + f32(0.25), d16, 10, metric, 1e-4, want_path=2)


# ---- path 3: ip, big ---------------------------------------------------------------------------------------------------------------
def queries_of(rng, d):
    pos = rng.random(d, dtype=f32)
    pos[3] = 0.0
    mixed = (rng.random(d, dtype=f32) - f32(0.5)).astype(f32)
    return {"sum_desc": pos, "sum_asc": -pos, "hybrid": mixed}


def test_path3_at_43(L, ref, big43, big43_idx):
    rng = np.random.default_rng(343)
    for case, q in queries_of(rng, 43).items():
        for k in (1, 10):
            for eps in (1e-6, 1e-4, 1e-2, 1.0):
                ans, info = check(big43_idx, ref, q, big43, k, IP, eps, want_path=3)
                assert info["ip_case"] == case and info["sample_dims"] == (0 if case != "hybrid" else 32)
                assert info["fell_back"] == (case == "hybrid" and info["pool"] >= BIG_N)   # (k = 10 at eps 1e-6: the pool would be every row)


def test_path3_at_70000_by_32(L, ref):
    """flat_mmap.rs:6222-6260 and, at dim 32, the hybrid case falling back to the exact search (every dimension would be sampled)"""
    n, d = 70000, 32
    rng = np.random.default_rng(70)
    data = (rng.random((n, d), dtype=f32) * f32(0.01)).astype(f32)
    data[12345] = 1.0
    data[54321] = -2.0
    idx = index_of(L, data)
    for k in (1, 10):
        for eps in (1e-6, 1e-4, 1e-2, 1.0):
            ans, info = check(idx, ref, np.ones(d, f32), data, k, IP, eps, want_path=3)
            assert ans.rows[0] == 12345 and ans.dists[0] == 32.0 and info["ip_case"] == "sum_desc"
            ans, info = check(idx, ref, -np.ones(d, f32), data, k, IP, eps, want_path=3)
            assert ans.rows[0] == 54321 and ans.dists[0] == 64.0 and info["ip_case"] == "sum_asc"
            mixed = np.ones(d, f32)
            mixed[1] = -0.5
            ans, info = check(idx, ref, mixed, data, k, IP, eps, want_path=3)
            assert info["ip_case"] == "hybrid" and info["fell_back"]


# ---- path 4: the additive metrics, big ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ADDITIVE)
def test_path4(L, ref, big43, big43_idx, metric):
    rng = np.random.default_rng(400 + metric)
    q = (rng.random(43, dtype=f32) - f32(0.3)).astype(f32)
    for eps in (1e-4, 1e-2):
        for k in (1, 10):
            ans, info = check(big43_idx, ref, q, big43, k, metric, eps, want_path=4)
            assert not info["fell_back"] and info["sample_dims"] == 32 and info["pool"] == ans.pool.size


# ---- the planted pool boundary -----------------------------------------------------------------------------------------------------
def outside_blocks(ref, d, sample):
    out = np.ones(d, bool)
    for s, ln in ref.blocks(d, sample):
        out[s:s + ln] = False
    return out


def planted_case(ref, kind, rank_of_pool):
    """Small-integer data (every sum exact in any order).  The row at coarse rank pool - 1 + rank_of_pool becomes the exact best without
    its coarse score changing -> data, query, metric, the planted row"""
    rng = np.random.default_rng({"sum": 1, "hybrid": 2, "l1": 3}[kind])
    n, d, eps = BIG_N, 43, 1e-4
    out = outside_blocks(ref, d, 32)
    if kind == "sum":
        metric = IP
        data = rng.integers(0, 4, (n, d)).astype(f32)
        q = np.ones(d, f32)
        q[0] = 100.0
    elif kind == "hybrid":
        metric = IP
        data = rng.integers(-2, 3, (n, d)).astype(f32)
        q = rng.integers(1, 3, d).astype(f32) * np.where(np.arange(d) % 2 == 0, 1.0, -1.0).astype(f32)
    else:
        metric = L1
        data = rng.integers(0, 4, (n, d)).astype(f32)
        data[:, out] += 100.0   # every row is far from the query outside the blocks
        q = rng.integers(0, 4, d).astype(f32)
        q[out] = 0.0
    base = ref.search(q, data, 1, metric, eps)
    pool = base.info["pool"]
    key = -base.coarse if (kind != "l1") else base.coarse
    order = np.lexsort((np.arange(n), key))
    assert np.array_equal(order[:pool].astype(np.uint32), base.pool)   # the pool is the canonical cut of the coarse scores
    row = int(order[pool - 1 + rank_of_pool])
    if kind == "sum":     # the weight moves to dimension 0, the sum stays
        delta = 20.0 - data[row, 0]
        data[row, 0] = 20.0
        data[row, 1:1 + int(delta)] -= 1.0
    elif kind == "hybrid":   # the whole new signal lies outside the sampled blocks
        data[row, out] = 50.0 * np.sign(q[out])
    else:
        data[row, out] = q[out]
    return data, q, metric, row, pool


@pytest.mark.parametrize("kind", ["sum", "hybrid", "l1"])
def test_planted_row_at_the_pool_boundary(L, ref, kind):
    for rank_of_pool, found in ((0, True), (1, False)):
        data, q, metric, row, pool = planted_case(ref, kind, rank_of_pool)
        d64 = data.astype(np.float64)
        exact = (d64 @ q) if metric == IP else np.abs(d64 - q).sum(1)
        assert int(np.argmax(exact) if metric == IP else np.argmin(exact)) == row   # the truly best row
        idx = index_of(L, data)
        ans, info = check(idx, ref, q, data, 1, metric, 1e-4)
        assert info["pool"] == pool and not info["fell_back"]
        assert (row in ans.pool) == found and (int(ans.rows[0]) == row) == found, (kind, rank_of_pool)
        e_rows, _, _ = idx.search_batch_arrays(q[None], 1, NAME[metric])
        assert int(e_rows[0, 0]) == row   # the exact search finds it either way


@pytest.mark.parametrize("kind", ["hybrid", "l1"])
def test_signal_outside_the_blocks_is_not_seen(L, ref, kind):
    """the best row's whole signal lies in dimensions outside the three blocks: the coarse pass reads nothing of it"""
    rng = np.random.default_rng(9)
    n, d = BIG_N, 43
    out = outside_blocks(ref, d, 32)
    if kind == "hybrid":
        metric = IP
        data = rng.integers(-2, 3, (n, d)).astype(f32)
        q = rng.integers(1, 3, d).astype(f32) * np.where(np.arange(d) % 2 == 0, 1.0, -1.0).astype(f32)
        data[40000] = 0.0
        data[40000, out] = 50.0 * np.sign(q[out])
    else:
        metric = L1
        data = rng.integers(0, 4, (n, d)).astype(f32)
        data[:, out] += 100.0
        q = rng.integers(0, 4, d).astype(f32)
        q[out] = 0.0
        data[40000] = q + 3.0   # the worst a row can be inside the blocks ...
        data[40000, out] = 0.0  # ... and exactly the query outside them
    idx = index_of(L, data)
    ans, info = check(idx, ref, q, data, 1, metric, 1e-4)
    e_rows, _, _ = idx.search_batch_arrays(q[None], 1, NAME[metric])
    assert int(e_rows[0, 0]) == 40000 and 40000 not in ans.pool and int(ans.rows[0]) != 40000


# ---- invalidation ------------------------------------------------------------------------------------------------------------------
def test_derived_copies_follow_every_mutation(L, ref):
    """flat_mmap.rs:6262-6272 through the Collection: after add_items + commit, upsert_items, update_items and compact the next
    approximate search is the restatement's on the final rows (row sums, norms and the sum order are built again)"""
    n, d = 70000, 32
    rows = np.zeros((n, d), f32)
    rows[12345] = 1.0
    c = L.Collection("approx-mut", d)
    c.add_items(rows, list(range(n)))
    c.commit()
    q = np.ones(d, f32)

    def agree(want_id, want_dist):
        for mode in ("FLAT-IP", "FLAT-L2"):
            c.build_index(mode, None)
            metric = IP if mode == "FLAT-IP" else L2
            res = c.search(q, 1, approx=True, eps=1e-4)
            ans = ref.search(q, rows, 1, metric, 1e-4)
            assert res.ids().tolist() == [int(ids[ans.rows[0]])]
            assert np.array_equal(res.distances().view(np.uint32), ref.round(ans.dists, 1e-4).view(np.uint32))
            if metric == IP:
                assert res.ids().tolist() == [want_id] and res.distances().tolist() == [want_dist]

    ids = np.arange(n)
    agree(12345, 32.0)
    c.add_items(np.full((1, d), 2.0, f32), [n])
    c.commit()
    rows, ids = np.concatenate([rows, np.full((1, d), 2.0, f32)]), np.arange(n + 1)
    agree(n, 64.0)
    c.upsert_items(np.full((1, d), 3.0, f32), [777])
    rows[777] = 3.0
    agree(777, 96.0)
    c.update_items(np.full((1, d), 4.0, f32), [888])
    rows[888] = 4.0
    agree(888, 128.0)
    c.delete_items([888, 5])
    assert c.compact() == 2
    keep = ~np.isin(ids, [888, 5])
    rows, ids = rows[keep], ids[keep]
    agree(777, 96.0)


# ---- the Collection ----------------------------------------------------------------------------------------------------------------
def collection(L, data, mode, name="approx"):
    c = L.Collection(name, data.shape[1])
    c.add_items(data, list(range(data.shape[0])))
    c.commit()
    if mode:
        c.build_index(mode, None)
    return c


def test_fails_without_the_feature_rounding(L):
    rng = np.random.default_rng(5)
    data = rng.standard_normal((500, 24)).astype(f32)
    c = collection(L, data, None)
    res = c.search(rng.standard_normal(24).astype(f32), 3, approx=True, eps=0.5)
    d = res.distances().astype(np.float64)
    assert np.all(d / 0.5 == np.round(d / 0.5)), d   # multiples of 0.5
    plain = c.search(data[0], 3)
    assert not np.all(plain.distances() / 0.5 == np.round(plain.distances() / 0.5))   # (the exact answer is not)


def test_collection_merges_raw_and_rounds_last(L, ref):
    # approx_search.rs:296-323 through Collection.search: ranked on 0.6 / 0.9, reported as 1.0
    c = collection(L, np.array([[0.6], [0.9]], f32), None)
    res = c.search([1.0], 1, approx=True, eps=1.0)
    assert res.ids().tolist() == [1] and res.distances().tolist() == [1.0]
    # pending rows merge on raw scores: pending 1.4 and 0.6 against flushed 0.9 and 0.6
    c.add_items(np.array([[0.6], [1.4]], f32), [2, 3])
    res = c.search([1.0], 2, approx=True, eps=1.0)
    assert res.ids().tolist() == [3, 1] and res.distances().tolist() == [1.0, 1.0]
    # rounding before the merge would change the winner: flushed 1.2 (row 0) and pending 1.4 (row 1) both round to 1.0 and the tie
    # would go to row 0; merged raw, 1.4 wins and is then reported as 1.0
    c2 = collection(L, np.array([[1.2]], f32), None)
    c2.add_items(np.array([[1.4]], f32), [1])
    res = c2.search([1.0], 1, approx=True, eps=1.0)
    assert res.ids().tolist() == [1] and res.distances().tolist() == [1.0]
    # tombstones are filtered on raw scores, then the rest is rounded
    c.delete_items([3])
    res = c.search([1.0], 2, approx=True, eps=1.0)
    assert res.ids().tolist() == [1, 0] and res.distances().tolist() == [1.0, 1.0]


def test_flag_is_ignored_where_the_reference_ignores_it(L):
    rng = np.random.default_rng(6)
    data = rng.standard_normal((3000, 32)).astype(f32)
    q = rng.standard_normal(32).astype(f32)

    def same(c, **kw):
        a, b = c.search(q, 5, approx=True, eps=0.5, **kw), c.search(q, 5, approx=False, **kw)
        assert a.ids().tolist() == b.ids().tolist()
        assert np.array_equal(a.distances().view(np.uint32), b.distances().view(np.uint32))

    flat = collection(L, data, "FLAT-L2")
    same(flat, subset=np.arange(0, 3000, 3))
    for mode in ("IVF-L2", "HNSW-L2", "FLAT-L2-PQ8"):
        same(collection(L, data, mode, name=mode.lower()))
    c = L.Collection("with-fields", 32)
    c.add_items(data, list(range(3000)), [{"g": int(i % 4)} for i in range(3000)])
    c.commit()
    same(c, where="g < 2")
    ham = collection(L, (data > 0).astype(f32), "FLAT-HAMMING-BINARY", name="ham")
    same(ham)


def test_flat_sq8_takes_path_1(L, ref):
    rng = np.random.default_rng(8)
    data = rng.standard_normal((2000, 40)).astype(f32)
    q = rng.standard_normal(40).astype(f32)
    c = collection(L, data, "FLAT-L2-SQ8")
    prof = c.search_profile(q, 5, approx=True, eps=1e-2)
    assert prof["profile"]["device"]["approx"]["path"] == 1
    ans = ref.search(q, data, 5, L2, 1e-2)
    assert prof["items"]["ids"] == ans.rows.tolist()
    assert np.array_equal(np.asarray(prof["items"]["scores"], f32).view(np.uint32), ref.round(ans.dists, 1e-2).view(np.uint32))
    assert "approx" not in c.search_profile(q, 5)["profile"]["device"]


def test_search_vector_field_approx(L, ref):
    rng = np.random.default_rng(10)
    base = rng.standard_normal((300, 8)).astype(f32)
    c = collection(L, base, None)
    fdata = (rng.random((300, 43), dtype=f32) + f32(0.01)).astype(f32)
    c.create_vector_field("aux", 43, "l1")
    c.add_named_vectors("aux", fdata, list(range(300)))
    q = (rng.random(43, dtype=f32) + f32(0.01)).astype(f32)
    res = c.search_vector_field("aux", q, 4, approx=True, eps=0.25)
    ans = ref.search(q, fdata, 4, L1, 0.25)
    assert res.ids().tolist() == ans.rows.tolist()
    assert np.array_equal(res.distances().view(np.uint32), ref.round(ans.dists, 0.25).view(np.uint32))
    exact = c.search_vector_field("aux", q, 4)
    assert exact.ids().tolist() == ans.rows.tolist() and not np.array_equal(exact.distances(), res.distances())


def test_refusals(L):
    idx = L.FlatIndex(None, 16, device=0)
    idx.write(np.zeros((10, 16), f32))
    with pytest.raises(NotImplementedError):
        idx.search_approx(np.zeros(16, f32), 3, "hamming", 1e-4)
    rows, dists, info = idx.search_approx(np.zeros(16, f32), 0, "ip", 1e-4)
    assert rows.size == 0 and info["path"] == 0
    rows, dists, info = idx.search_approx(np.ones(16, f32), 50, "l2", None)
    assert rows.tolist() == list(range(10)) and info["eps"] == pytest.approx(1e-4)
