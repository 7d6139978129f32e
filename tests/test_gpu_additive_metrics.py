"""GPU parity tests for the additive metrics (ids 7-10: Manhattan, Chebyshev, Canberra, Bray-Curtis; include/lynse_hip.h) through the
C ABI, FlatIndex and the Collection, against a restatement of the four forms (tests/additive_ref/additive_ref.c: plain C, eight explicit
lanes; checked on its own in tests/test_additive_metric_modes.py).  A NaN distance is compared as +inf, the order is (distance, row);
result ids and f32 distance bits are compared exactly, there are no tolerances."""
import ctypes as C

import numpy as np
import pytest

from additive_common import BRAY, CANB, CHEB, L1, NAME, build_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
_vp = C.c_void_p
METRICS = [L1, CHEB, CANB, BRAY]
UNSUPPORTED = 9   # LYNSE_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("additive_ref"))


def topk(d, k, live=None):
    """the canonical best min(k, live rows) of one query's distances -> (rows, distances)"""
    rows = np.arange(d.size) if live is None else np.nonzero(live)[0]
    order = rows[np.lexsort((rows, d[rows]))][:k]
    return order.astype(np.uint64), d[order]


def check_batch(got, dmat, k, live=None, what=None):
    rows, dists, counts = got
    for qi in range(dmat.shape[0]):
        e_r, e_d = topk(dmat[qi], k, live)
        c = int(counts[qi])
        assert c == e_r.size, (what, qi, c, e_r.size)
        assert np.array_equal(rows[qi, :c], e_r), (what, qi, rows[qi, :c][:12], e_r[:12])
        assert np.array_equal(dists[qi, :c].view(np.uint32), e_d.view(np.uint32)), (what, qi, dists[qi, :c][:12], e_d[:12])


def make(rng, n, dim, kind):
    return (rng.standard_normal((n, dim)) if kind == 0 else rng.random((n, dim)) + 0.01).astype(f32)


def index_of(L, data, **kw):
    idx = L.FlatIndex(None, data.shape[1], device=0, **kw)
    idx.write(data)
    return idx


# ---- single pairs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", METRICS)
def test_single_pairs_are_bit_equal(L, ref, m):
    rng = np.random.default_rng(m)
    for D in [1, 3, 7, 8, 9, 15, 16, 17, 24, 100, 128, 771, 1536]:
        for kind in range(2):
            a, b = make(rng, 1, D, kind)[0], make(rng, 1, D, kind)[0]
            g = np.float32(L.py_compute_distance(a, b, NAME[m]))
            assert g.view(np.uint32) == ref.dist(m, a, b).view(np.uint32), (m, D, kind, g, ref.dist(m, a, b))
    for mm, a, b, exp in [(L1, [1, 2, 3], [3, 0, 4], 5.0), (L1, [1, 2], [4, 0], 5.0), (CHEB, [1, 2, 3], [4, 0, 3], 3.0),
                          (CANB, [1, 0, 3], [2, 0, 1], 5 / 6), (BRAY, [1, 2], [2, 4], 1 / 3)]:
        if mm == m:
            assert abs(L.py_compute_distance(np.array(a, f32), np.array(b, f32), NAME[m]) - exp) < 1e-5
    ids, d = L.py_top_k_search(np.array([1, 2, 3], f32), np.array([[3, 0, 4], [1, 2, 3], [0, 0, 0]], f32), NAME[m], 2)
    assert list(ids) == [1, 0] and d[0] == 0.0 and d[1].view(np.uint32) == ref.dist(m, [1, 2, 3], [3, 0, 4]).view(np.uint32)


def special_pairs():
    nan, inf = np.nan, np.inf
    out = []
    for D in (8, 3, 11, 19):
        spots = sorted({0, D - 1, min(D - 1, 8), D // 2})
        for s in spots:
            for va, vb in [(nan, 0.0), (0.0, nan), (inf, 1.0), (-inf, 1.0), (inf, inf), (inf, -inf), (0.0, 0.0), (2.5, -2.5), (nan, nan)]:
                a = np.linspace(0.5, 2.0, D).astype(f32)
                b = np.linspace(1.0, 0.25, D).astype(f32)
                a[s], b[s] = va, vb
                out.append((a, b))
        out.append((np.zeros(D, f32), np.zeros(D, f32)))                       # 0 / 0 everywhere; Bray-Curtis 0 at a zero denominator
        a = np.linspace(0.5, 2.0, D).astype(f32)
        out.append((a, -a))                                                   # a = -b: Bray-Curtis +inf at a zero denominator
        out.append((np.full(D, nan, f32), np.zeros(D, f32)))                  # every step NaN
    return out


@pytest.mark.parametrize("m", METRICS)
def test_special_values(L, ref, m):
    nan, inf = np.nan, np.inf

    def gpu(a, b):
        return np.float32(L.py_compute_distance(np.asarray(a, f32), np.asarray(b, f32), NAME[m]))

    for a, b in special_pairs():
        e = ref.dist(m, a, b)
        e = np.float32(inf) if np.isnan(e) else e   # a NaN distance is reported as +inf
        g = gpu(a, b)
        assert g.view(np.uint32) == e.view(np.uint32), (m, a, b, g, e)
    z = np.zeros(16, f32)
    if m == CHEB:
        a = z.copy(); a[0] = nan; a[8] = 2
        assert gpu(a, z) == 2.0                    # a NaN in an early step is erased by the lane's next step
        a = z.copy(); a[1] = 3; a[8] = nan
        assert gpu(a, z) == 3.0                    # a NaN in a lane's last step is dropped at the reduction
        assert gpu([nan, 1, nan], [0, 0, 0]) == 1.0 and gpu(np.full(19, nan, f32), np.zeros(19, f32)) == 0.0   # never NaN (nor +inf from one)
    if m == CANB:
        a = np.ones(8, f32); b = np.ones(8, f32); a[2] = nan
        assert gpu(a, b) == 0.0                    # a NaN denominator adds +0 in the body ...
        assert gpu(a[:3], b[:3]) == inf            # ... and NaN in the tail (reported as +inf)
        a = np.ones(11, f32); b = np.ones(11, f32); a[2] = nan
        assert gpu(a, b) == 0.0
        a[2] = 1; a[9] = nan
        assert gpu(a, b) == inf
    if m == BRAY:
        a = np.arange(1, 12, dtype=f32)
        assert gpu(a, -a) == inf and gpu(np.zeros(11, f32), np.zeros(11, f32)) == 0.0 and gpu(a, a) == 0.0


# ---- search parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 3, 8, 9, 100, 128, 771])
@pytest.mark.parametrize("m", METRICS)
def test_search_parity(L, ref, m, D):
    rng = np.random.default_rng(100 * m + D)
    for n in (1003, 3000):                              # the last row tile is partial
        data = make(rng, n, D, 1 if m == BRAY else n % 2)
        queries = make(rng, 256, D, 1 if m == BRAY else n % 2)
        queries[5] = data[77]
        dmat = ref.dists(m, queries, data)
        idx = index_of(L, data)
        for nq in (1, 3, 17, 256):                      # a partial query tile, a partial block of 8 queries
            for k in (1, 10, 100):
                check_batch(idx.search_batch_arrays(queries[:nq], k, NAME[m]), dmat[:nq], k, what=(m, D, n, nq, k))
        ids, d = idx.search(queries[5], 3, NAME[m])
        assert ids[0] == 77 and d[0] == 0.0
        res = idx.batch_search(queries[:4], 7, NAME[m])
        for qi, (ids, d) in enumerate(res):
            e_r, e_d = topk(dmat[qi], 7)
            assert np.array_equal(ids, e_r.astype(np.uint32)) and np.array_equal(d.view(np.uint32), e_d.view(np.uint32))


@pytest.mark.parametrize("m", METRICS)
def test_ties_go_by_row_and_k_cuts_through_a_tie_class(L, ref, m):
    rng = np.random.default_rng(7)
    data = rng.integers(0, 3, size=(700, 8)).astype(f32)
    queries = rng.integers(0, 3, size=(9, 8)).astype(f32)
    dmat = ref.dists(m, queries, data)
    if m == CHEB:
        assert set(np.unique(dmat)) <= {0.0, 1.0, 2.0}
    idx = index_of(L, data)
    for k in (1, 5, 37, 200, 699, 700):
        check_batch(idx.search_batch_arrays(queries, k, NAME[m]), dmat, k, what=(m, k))
    if m == CHEB:   # the cut falls inside a class of equal distances
        d0 = np.sort(dmat[0])
        assert d0[36] == d0[37]


@pytest.mark.parametrize("m", METRICS)
def test_edge_sizes(L, ref, m):
    rng = np.random.default_rng(3)
    dim = 12
    queries = make(rng, 3, dim, 1)
    for n in (1, 31, 33):
        data = make(rng, n, dim, 1)
        dmat = ref.dists(m, queries, data)
        idx = index_of(L, data)
        for k in (n, n + 5, 1):
            check_batch(idx.search_batch_arrays(queries, k, NAME[m]), dmat, k, what=(m, n, k))
        rows, dists, counts = idx.search_batch_arrays(queries, 0, NAME[m])
        assert counts.tolist() == [0, 0, 0]
    empty = L.FlatIndex(None, dim, device=0)
    rows, dists, counts = empty.search_batch_arrays(queries, 5, NAME[m])
    assert counts.tolist() == [0, 0, 0]
    assert len(empty.search(queries[0], 5, NAME[m])[0]) == 0


@pytest.mark.parametrize("m", METRICS)
def test_filters(L, ref, m):
    rng = np.random.default_rng(11)
    n, dim, nq = 2500, 20, 5
    data, queries = make(rng, n, dim, 1), make(rng, nq, dim, 1)
    dmat = ref.dists(m, queries, data)
    idx = index_of(L, data)
    sub = np.unique(rng.integers(0, n, 600)).astype(np.uint64)
    live = np.isin(np.arange(n), sub)
    # an id list (duplicates once, ids >= len skipped) and the same rows as a BitSet
    listed = np.concatenate([sub[::-1], sub[:50], np.array([n, n + 7, 1 << 40], np.uint64)])
    for k in (1, 10, 300):
        check_batch(idx.search_filtered_batch_arrays(queries, k, NAME[m], listed), dmat, k, live, what=(m, "list", k))
        check_batch(idx.search_filtered_bitset_batch_arrays(queries, k, NAME[m], L.BitSet.from_rows(sub, n).words), dmat, k, live, what=(m, "bits", k))
    # a subset smaller than k
    few = np.array([2400, 3, 64, 63], np.uint64)
    check_batch(idx.search_filtered_batch_arrays(queries, 10, NAME[m], few), dmat, 10, np.isin(np.arange(n), few), what=(m, "few"))
    # an empty subset
    rows, dists, counts = idx.search_filtered_batch_arrays(queries, 10, NAME[m], np.zeros(0, np.uint64))
    assert counts.tolist() == [0] * nq
    rows, dists, counts = idx.search_filtered_bitset_batch_arrays(queries, 10, NAME[m], np.zeros((n + 63) // 64, np.uint64))
    assert counts.tolist() == [0] * nq
    # rows beyond the bitset's words are out; bits at or beyond len are ignored
    words = L.BitSet.from_rows(sub, n).words
    short = words[:10].copy()
    check_batch(idx.search_filtered_bitset_batch_arrays(queries, 50, NAME[m], short), dmat, 50, live & (np.arange(n) < 640), what=(m, "short"))
    longer = np.concatenate([words, np.full(3, ~np.uint64(0), np.uint64)])
    longer[(n - 1) // 64] |= ~np.uint64(0) << np.uint64(n % 64)
    check_batch(idx.search_filtered_bitset_batch_arrays(queries, 700, NAME[m], longer), dmat, 700, live, what=(m, "long"))
    # the single-query form
    ids, d = idx.search_filtered(queries[1], 10, NAME[m], sub)
    e_r, e_d = topk(dmat[1], 10, live)
    assert np.array_equal(ids, e_r.astype(np.uint32)) and np.array_equal(d.view(np.uint32), e_d.view(np.uint32))


def test_query_chunks_of_223_and_7(L, ref):
    """n = 600,000: the score matrix of 230 queries is past 512 MiB, the batch goes as 223 + 7 (ScoreCut::chunk)"""
    rng = np.random.default_rng(13)
    n, dim, nq, k = 600_000, 16, 230, 10
    data = rng.random((n, dim), dtype=f32)
    queries = rng.random((nq, dim), dtype=f32)
    idx = index_of(L, data)
    got = idx.search_batch_arrays(queries, k, "l1")
    dmat = ref.dists(L1, queries, data)
    part = np.argpartition(dmat, 64, axis=1)[:, :64]   # (the canonical top 10 lie among the 64 smallest ... unless 55 rows tie: checked)
    rows, dists, counts = got
    for qi in range(nq):
        cand = np.sort(part[qi])
        assert np.sum(dmat[qi] <= dmat[qi, cand].max()) >= k
        order = cand[np.lexsort((cand, dmat[qi, cand]))][:k]
        assert int(counts[qi]) == k and np.array_equal(rows[qi], order.astype(np.uint64)), qi
        assert np.array_equal(dists[qi].view(np.uint32), dmat[qi, order].view(np.uint32)), qi


@pytest.mark.parametrize("m", [L1, CANB])
def test_more_than_16384_keys_are_sorted_on_the_host(L, ref, m):
    rng = np.random.default_rng(17)
    n, dim, k = 21_000, 8, 20_000
    data, queries = make(rng, n, dim, 1), make(rng, 2, dim, 1)
    data[500:520] = data[100]     # ties
    idx = index_of(L, data)
    check_batch(idx.search_batch_arrays(queries, k, NAME[m]), ref.dists(m, queries, data), k, what=(m, "host sort"))
    check_batch(idx.search_batch_arrays(queries, n + 1, NAME[m]), ref.dists(m, queries, data), n, what=(m, "host sort, all"))


@pytest.mark.parametrize("m", METRICS)
def test_wide_rows_and_the_lds_refusal(L, ref, m):
    rng = np.random.default_rng(19)
    dim = 5000
    data, queries = make(rng, 100, dim, 1), make(rng, 3, dim, 1)
    idx = index_of(L, data)
    check_batch(idx.search_batch_arrays(queries, 10, NAME[m]), ref.dists(m, queries, data), 10, what=(m, dim))
    wide = L.FlatIndex(None, 24_000, device=0)
    wide.write(np.ones((2, 24_000), f32))
    with pytest.raises(NotImplementedError, match="do not fit in LDS"):
        wide.search_batch_arrays(np.ones((1, 24_000), f32), 1, NAME[m])


@pytest.mark.parametrize("dim", [8, 11])
@pytest.mark.parametrize("m", METRICS)
def test_non_finite_rows_and_queries_follow_the_pinned_order(L, ref, m, dim):
    rng = np.random.default_rng(23)
    n = 300
    data = make(rng, n, dim, 1)
    nan, inf = np.nan, np.inf
    data[3, 0] = nan; data[10, dim - 1] = nan; data[20, 1] = inf; data[21, 2] = -inf; data[22] = inf; data[40, dim // 2] = nan
    data[50] = 0.0
    queries = make(rng, 6, dim, 1)
    queries[1, 0] = inf
    queries[2, dim - 1] = nan
    queries[3] = nan
    queries[4] = 0.0
    dmat = ref.dists(m, queries, data)
    idx = index_of(L, data)
    for k in (5, 290, n):
        check_batch(idx.search_batch_arrays(queries, k, NAME[m]), dmat, k, what=(m, dim, k))
    if m in (L1, BRAY):   # a NaN query: every distance NaN -> rows 0 .. k-1 at +inf
        rows, dists, counts = idx.search_batch_arrays(queries[3:4], 7, NAME[m])
        assert rows[0].tolist() == list(range(7)) and np.all(np.isposinf(dists[0]))


# ---- range search -----------------------------------------------------------------------------------------------------------------
def check_range(got, dmat_raw, thr, cap, live=None):
    rows, dists, counts, passed = got
    for qi in range(dmat_raw.shape[0]):
        d = dmat_raw[qi]
        ok = d <= thr[qi]                               # a NaN distance never passes
        if live is not None:
            ok &= live
        pr = np.nonzero(ok)[0]
        order = pr[np.lexsort((pr, d[pr]))][:cap]
        assert int(passed[qi]) == pr.size and int(counts[qi]) == order.size, (qi, passed[qi], pr.size)
        assert np.array_equal(rows[qi, :order.size], order.astype(np.uint64)), qi
        assert np.array_equal(dists[qi, :order.size].view(np.uint32), d[order].view(np.uint32)), qi
        assert np.all(rows[qi, order.size:] == ~np.uint64(0)) and np.all(np.isposinf(dists[qi, order.size:]))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("m", METRICS)
def test_range_search(L, ref, m, dtype):
    rng = np.random.default_rng(29)
    n, dim, nq = 1500, 27, 6
    data, queries = make(rng, n, dim, 1), make(rng, nq, dim, 1)
    if dtype == "f16":
        data = data.astype(np.float16).astype(f32)      # the shard scores its exactly decoded rows
    data[7, 3] = np.nan
    idx = index_of(L, data, dtype=dtype)
    raw = np.empty((nq, n), f32)
    for qi in range(nq):
        for r in range(n):
            raw[qi, r] = ref.dist(m, queries[qi], data[r])
    thr = np.array([np.sort(raw[qi][~np.isnan(raw[qi])])[[0, 40, 400, 1400, 5, 900][qi]] for qi in range(nq)], f32)
    thr[4] = np.inf
    for cap in (10, 2000):
        check_range(idx.search_range_batch_arrays(queries, thr, cap, NAME[m]), raw, thr, cap)
    live = np.arange(n) % 3 != 0
    words = L.BitSet.from_rows(np.nonzero(live)[0], n).words
    check_range(idx.search_range_batch_arrays(queries, thr, 25, NAME[m], words), raw, thr, 25, live)
    if dtype == "f16":   # top-k under the additive metrics on an F16 shard: refused
        with pytest.raises(NotImplementedError):
            idx.search_batch_arrays(queries, 5, NAME[m])


# ---- the Collection ---------------------------------------------------------------------------------------------------------------
MODES = {"FLAT-L1": L1, "FLAT-MANHATTAN": L1, "FLAT-CITYBLOCK": L1, "FLAT-CHEBYSHEV": CHEB, "FLAT-CHEBYCHEV": CHEB, "FLAT-LINF": CHEB,
         "FLAT-CANBERRA": CANB, "FLAT-BRAY-CURTIS": BRAY, "FLAT-BRAYCURTIS": BRAY, "flat-manhattan": L1, "Flat-Bray-Curtis": BRAY}


def test_collection_reference_case_under_every_mode_name(L, ref):
    """the reference's API test (tests/standard_tests/test_search.py:176-212): 32 x 16 from default_rng(20260620).random + 0.01, row 7
    finds itself at ~0"""
    data = (np.random.default_rng(20260620).random((32, 16)) + 0.01).astype(f32)
    for mode, m in MODES.items():
        c = L.Collection("domain", 16, device=0)
        c.add_items(data, list(range(32)))
        c.commit()
        c.build_index(mode)
        res = c.search(data[7], k=3)
        assert res.ids()[0] == 7 and abs(float(res.distances()[0])) < 1e-6
        assert res.index_mode() == mode.upper()
        e_r, e_d = topk(ref.dists(m, data[7:8], data)[0], 3)
        assert np.array_equal(res.ids(), e_r.astype(np.int64)) and np.array_equal(res.distances().view(np.uint32), e_d.view(np.uint32))


@pytest.mark.parametrize("mode", ["FLAT-L1", "FLAT-LINF", "FLAT-CANBERRA", "FLAT-BRAY-CURTIS"])
def test_collection_glue(L, ref, mode):
    m = MODES[mode]
    rng = np.random.default_rng(31)
    n, dim, k = 900, 24, 10
    data = make(rng, n, dim, 1)
    ids = (rng.permutation(n) * 5 + 100).astype(np.int64)
    queries = make(rng, 4, dim, 1)
    c = L.Collection("glue", dim, device=0)
    c.add_items(data[:700], ids[:700].tolist())
    c.commit()
    c.build_index(mode)
    assert c._ivf is None and not c._pq and not c._rabitq
    dmat = ref.dists(m, queries, data)

    def expect(qi, k, live):
        e_r, e_d = topk(dmat[qi], k, live)
        return ids[e_r.astype(np.int64)], e_d

    def same(res, exp):
        assert np.array_equal(res.ids(), exp[0]), (res.ids(), exp[0])
        assert np.array_equal(res.distances().view(np.uint32), exp[1].view(np.uint32))

    first = np.arange(n) < 700
    for qi, res in enumerate(c.batch_search(queries, k)):
        same(res, expect(qi, k, first))
    # pending rows are merged in
    c.add_items(data[700:], ids[700:].tolist())
    assert c.pending_len() == 200
    for qi, res in enumerate(c.batch_search(queries, k)):
        same(res, expect(qi, k, None))
    c.commit()
    same(c.search(queries[0], k), expect(0, k, None))
    # subset= as rows and as a BitSet
    sub = np.arange(0, n, 4)
    live = np.isin(np.arange(n), sub)
    same(c.search(queries[1], k, subset=sub), expect(1, k, live))
    same(c.search(queries[1], k, subset=L.BitSet.from_rows(sub, n)), expect(1, k, live))
    # tombstones
    best = [int(x) for x in c.search(queries[2], 5).ids()]
    c.delete_items(best)
    alive = ~np.isin(ids, best)
    same(c.search(queries[2], k), expect(2, k, alive))
    same(c.search(queries[2], k, subset=sub), expect(2, k, alive & live))
    # search_range
    thr = float(np.sort(dmat[3])[60])
    r_ids, r_d = c.search_range(queries[3], thr, max_results=40)
    pr = np.nonzero((dmat[3] <= thr) & alive)[0]
    order = pr[np.lexsort((pr, dmat[3][pr]))][:40]
    assert r_ids == [int(x) for x in ids[order]] and np.array_equal(np.asarray(r_d, f32).view(np.uint32), dmat[3][order].view(np.uint32))
    c.restore_items(best)
    # search_profile
    prof = c.search_profile(queries[0], k)
    assert prof["profile"]["index_path"] == "flat_mmap" and prof["items"]["ids"] == [int(x) for x in expect(0, k, None)[0]]
    assert prof["items"]["index"] == mode
    prof = c.search_profile(queries[0], k, subset=sub)
    assert prof["profile"]["index_path"] == "flat_mmap_filtered" and prof["items"]["ids"] == [int(x) for x in expect(0, k, live)[0]]


def test_collection_mode_sequence_leaves_no_auxiliary_index(L, ref):
    rng = np.random.default_rng(37)
    data = make(rng, 600, 32, 1)
    c = L.Collection("seq", 32, device=0)
    c.add_items(data, list(range(600)))
    c.commit()
    c.build_index("FLAT-L1")
    c.build_index("FLAT-L2-PQ8")
    assert c._pq
    c.build_index("FLAT-CANBERRA")
    assert not c._pq and not c._rabitq and c._ivf is None
    assert c._flat.pq_params(arrays=False)["M"] == 0
    res = c.search(data[9], 5)
    e_r, e_d = topk(ref.dists(CANB, data[9:10], data)[0], 5)
    assert np.array_equal(res.ids(), e_r.astype(np.int64)) and np.array_equal(res.distances().view(np.uint32), e_d.view(np.uint32))
    for mode in ("FLAT-L1-SQ8", "FLAT-L1-PQ8", "FLAT-CANBERRA-BINARY", "IVF-L1", "SPANN-CHEBYSHEV", "ivf-manhattan"):
        with pytest.raises(ValueError, match="Invalid argument: Unknown index type: "):
            c.build_index(mode)
    assert c.search(data[9], 5).index_mode() == "FLAT-CANBERRA"


# ---- refusals of the C ABI --------------------------------------------------------------------------------------------------------
def test_c_abi_refusals(L):
    import torch

    lib = L._lib.lib
    rng = np.random.default_rng(41)
    n, dim, nq, k = 300, 16, 2, 3
    data, queries = make(rng, n, dim, 1), make(rng, nq, dim, 1)
    idx = index_of(L, data)
    rows, dists, counts = np.zeros((nq, k), np.uint64), np.zeros((nq, k), f32), np.zeros(nq, np.uint32)
    p = lambda a: a.ctypes.data_as(_vp)

    def refused(rc):
        assert rc == UNSUPPORTED, (rc, L._lib.last_error())
        assert "Unknown metric" not in L._lib.last_error()

    refused(lib.lynse_hip_flat_search_sq8_f32(idx.handle, p(queries), nq, k, L1, p(rows), p(dists), p(counts)))
    refused(lib.lynse_hip_flat_search_pq_f32(idx.handle, p(queries), nq, k, L1, 32, p(rows), p(dists), p(counts)))
    refused(lib.lynse_hip_flat_search_rabitq_f32(idx.handle, p(queries), nq, k, L1, 200, p(rows), p(dists), p(counts)))
    refused(lib.lynse_hip_flat_prepare(idx.handle, L1, 16))
    refused(lib.lynse_hip_flat_search_packed_u64(idx.handle, p(np.zeros((nq, 1), np.uint64)), nq, k, L1, p(rows), p(dists), p(counts)))
    out = _vp()
    refused(lib.lynse_hip_ivf_build(p(data), n, dim, 4, 3, L1, 0, 0, C.byref(out)))
    ivf = L.IvfFlatIndex.build(None, data, dim, 4, 3, "l2")
    with pytest.raises(NotImplementedError):
        ivf.search(queries[0], k, 2, "manhattan")
    dev = torch.device("cuda", 0)
    dq = torch.as_tensor(queries, device=dev)
    d_rows = torch.zeros((nq, k), dtype=torch.int64, device=dev)
    d_dists = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    d_counts = torch.zeros(nq, dtype=torch.int32, device=dev)
    with pytest.raises(NotImplementedError):
        idx.search_device(dq, k, L1, d_rows, d_dists, d_counts)
    with pytest.raises(NotImplementedError):
        idx.search_submit(dq, k, L1, d_rows, d_dists, d_counts)
    refused(lib.lynse_hip_flat_search_sharded_f32_device(idx.handle, None, _vp(dq.data_ptr()), nq, k, L1, _vp(d_rows.data_ptr()),
                                                         _vp(d_dists.data_ptr()), _vp(d_counts.data_ptr())))
    with pytest.raises(NotImplementedError):
        idx.coarse_scores(queries, L1)
    for bad in (11, -1):
        assert lib.lynse_hip_flat_search_f32(idx.handle, p(queries), nq, k, bad, p(rows), p(dists), p(counts)) == 3   # LYNSE_ERR_UNKNOWN_METRIC
    # an F16 shard (top-k only), a packed-only handle, a row-mapped handle
    h16 = index_of(L, data, dtype="f16")
    refused(lib.lynse_hip_flat_search_f32(h16.handle, p(queries), nq, k, L1, p(rows), p(dists), p(counts)))
    packed = L.FlatIndex(None, 64, device=0)
    packed.write_packed(np.arange(10, dtype=np.uint64).reshape(10, 1))
    q64 = np.zeros((nq, 64), f32)
    refused(lib.lynse_hip_flat_search_f32(packed.handle, p(q64), nq, k, L1, p(rows), p(dists), p(counts)))
    idx.set_row_map(2, 1)
    refused(lib.lynse_hip_flat_search_f32(idx.handle, p(queries), nq, k, L1, p(rows), p(dists), p(counts)))
    idx.set_row_map(1, 0)
    assert lib.lynse_hip_flat_search_f32(idx.handle, p(queries), nq, k, L1, p(rows), p(dists), p(counts)) == 0
    # a call while a ticket is outstanding is refused (the search borrows per-handle scratch under the exclusive lock)
    big = index_of(L, rng.random((70_000, 32), dtype=f32))
    q40 = rng.random((40, 32), dtype=f32)
    dq = torch.as_tensor(q40, device=dev)
    outs = [(torch.zeros((40, k), dtype=torch.int64, device=dev), torch.zeros((40, k), dtype=torch.float32, device=dev),
             torch.zeros(40, dtype=torch.int32, device=dev)) for _ in range(2)]
    big.search_device(dq, k, "l2", *outs[0])     # (builds the derived data: the next batch of this shape is pipelined)
    rows, dists, counts = np.zeros((40, k), np.uint64), np.zeros((40, k), f32), np.zeros(40, np.uint32)
    t = big.search_submit(dq, k, "l2", *outs[1])
    rc = lib.lynse_hip_flat_search_f32(big.handle, p(q40), 40, k, L1, p(rows), p(dists), p(counts))
    msg = L._lib.last_error()
    t.wait()
    assert rc == 1 and "outstanding tickets" in msg, (rc, msg)   # LYNSE_ERR_INVALID_ARGUMENT, as every exclusive entry answers
    assert lib.lynse_hip_flat_search_f32(big.handle, p(q40), 40, k, L1, p(rows), p(dists), p(counts)) == 0 and counts.tolist() == [k] * 40
