"""GPU parity tests for SPANN-{IP,L2,COS}[-SQ8] (SPANNIndex, src/index/spann.rs) through the C ABI against a composition of the
existing oracle.

Expected values: oracle.kmeans_train for the centroids, oracle.all_distances (single-row kernels) of every row against the
centroids, the posting rule restated in Python (lynsedb_amd.core.spann_posting_rule) for the lists; for a search, the probed lists
of oracle.ivf_search, the DISTINCT rows of those lists (intersected with the subset; fewer than k -> all subset rows), scored with
oracle.all_distances and put in the canonical (distance, row) order.  SQ8 composes the quantizer restatement of test_gpu_ivf_sq8."""
import numpy as np
import pytest

import oracle as O
from conftest import oracle_for_every_query
from lynsedb_amd.core import spann_posting_rule
from test_gpu_ivf_sq8 import canonical, clustered, sq_codec, sq_fit

pytestmark = pytest.mark.gpu
IP, L2, COS = O.IP, O.L2, O.COS
NAME = {IP: "ip", L2: "l2", COS: "cosine"}
f32 = np.float32


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


# ------------------------------------------------------------------------------------- restatement ----
def ranks_of(oracle, row, cen, metric):
    d = oracle.all_distances(row, cen, metric, ip_form=O.IPFORM_SINGLE)
    with np.errstate(all="ignore"):
        return (-d if metric == IP else d).astype(f32)


def row_lists(oracle, rows, cen, metric, R):
    return [spann_posting_rule(ranks_of(oracle, r, cen, metric), R) for r in rows]


def csr_of(lists, nlist):
    """list-major CSR (rows ascending inside a list) of per-row lists"""
    members = [[] for _ in range(nlist)]
    for r, ls in enumerate(lists):
        for c in ls:
            members[c].append(r)
    off = np.zeros(nlist + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in members])
    rows = np.array([r for m in members for r in m], np.uint32)
    return off, rows


def expected_search(oracle, q, data, cen, off, rows, nprobe, k, metric, subset=None, scored=None, sq=None):
    """SPANNIndex::search of one query: (ids, dists) of the canonical top k (plain), or the SQ8 pool + exact rescore."""
    n = data.shape[0]
    qd = sq_codec(q[None, :], *sq)[0] if sq else q
    rowsrc = scored if scored is not None else data
    if k == 0:
        return np.zeros(0, np.uint64), np.zeros(0, f32)
    nl = cen.shape[0]
    np_eff = min(max(nprobe, 1), nl)
    _, _, probed = oracle.ivf_search(qd, rowsrc, cen, off, rows, np_eff, 1, metric)
    allowed = np.ones(n, bool) if subset is None else np.isin(np.arange(n), np.asarray(subset, np.int64))
    cand = np.unique(np.concatenate([rows[int(off[c]):int(off[c + 1])] for c in probed] + [np.zeros(0, np.uint32)]).astype(np.int64))
    cand = cand[allowed[cand]]
    if cand.size < k:
        cand = np.nonzero(allowed)[0]
    if cand.size == 0:
        return np.zeros(0, np.uint64), np.zeros(0, f32)
    d = oracle.all_distances(qd, rowsrc[cand], metric, ip_form=O.IPFORM_SINGLE)
    ids, dd = canonical(cand.astype(np.uint64), d, metric)
    if sq is None:
        return ids[:k], dd[:k]
    pool = min(max(10 * k, k), cand.size)
    p_ids = ids[:pool]
    ex = oracle.all_distances(q, data[p_ids.astype(np.int64)], metric, ip_form=O.IPFORM_SINGLE)
    ids, dd = canonical(p_ids, ex, metric)
    c = min(k, pool)
    return ids[:c], dd[:c]


def check_search(oracle, got, queries, data, cen, off, rows, nprobe, k, metric, subset=None, scored=None, sq=None, what=""):
    g_rows, g_d, g_c = got
    want = oracle_for_every_query(lambda qi: expected_search(oracle, queries[qi], data, cen, off, rows, nprobe, k, metric, subset, scored, sq),
                                  queries.shape[0])
    for qi, (e_ids, e_d) in enumerate(want):
        c = int(g_c[qi])
        assert c == len(e_ids), (what, qi, c, len(e_ids))
        assert np.array_equal(g_rows[qi, :c].astype(np.uint64), e_ids), (what, qi, g_rows[qi, :c], e_ids)
        assert np.array_equal(g_d[qi, :c].view(np.uint32), e_d.view(np.uint32)), (what, qi, g_d[qi, :c], e_d)


def assert_postings(idx, want_off, want_rows, what=""):
    off, rows = idx.postings()
    assert np.array_equal(off, want_off), (what, off, want_off)
    assert np.array_equal(rows, want_rows), what


# --------------------------------------------------------------------------------------- postings ----
@pytest.mark.parametrize("metric", [IP, L2, COS])
@pytest.mark.parametrize("R", [0, 1, 2, 4])
def test_build_postings_bit_equal(L, oracle, metric, R):
    _, data = clustered(30 + metric, 2500, 20, ncent=10, noise=0.6)
    data[7] = data[8]                      # duplicate rows
    data[100] = data[101] = data[102]
    nlist = 24
    idx = L.SpannIndex.build(data, 20, nlist, 20, NAME[metric], replica_count=R)
    cen, asg = oracle.kmeans_train(data, nlist, 20, metric)
    assert idx.n_partitions == cen.shape[0] and len(idx) == data.shape[0] and idx.replica_count == R
    if R == 0:
        want = [[int(a)] for a in asg]
    else:
        want = row_lists(oracle, data, cen, metric, R)
    off, rows = csr_of(want, cen.shape[0])
    assert_postings(idx, off, rows, (metric, R))
    if R > 0:
        assert rows.size > data.shape[0]     # boundary replicas exist on this data


@pytest.mark.parametrize("metric", [IP, L2, COS])
@pytest.mark.parametrize("R", [0, 1, 2, 4])
def test_insert_postings_of_non_finite_and_extreme_rows(L, oracle, metric, R):
    """Rows with NaN / +-inf elements, huge magnitudes (an overflowing inner product) and duplicates follow the sequential rule."""
    rng, data = clustered(40 + metric, 600, 12, ncent=6, noise=0.5)
    nlist = 10
    idx = L.SpannIndex.build(data, 12, nlist, 20, NAME[metric], replica_count=R)
    cen, asg = oracle.kmeans_train(data, nlist, 20, metric)
    new = rng.standard_normal((12, 12)).astype(f32)
    new[0, 3] = np.nan
    new[1, :] = np.nan
    new[2, 5] = np.inf
    new[3, 5] = -np.inf
    new[4, :] = np.inf
    new[5, 0], new[5, 1] = np.inf, -np.inf
    new[6, :] = f32(3e38)                 # inner products overflow
    new[7, ::2], new[7, 1::2] = f32(3e38), f32(-3e38)
    new[8] = 0.0                          # zero row (cosine: the 1e-30 floor)
    new[9] = data[3]                      # duplicates of indexed rows
    new[10] = new[9]
    new[11] = cen[2]                      # a row on a centroid
    idx.insert(new)
    allrows = np.concatenate([data, new])
    off0, rows0 = idx.postings()
    # the old rows keep their lists (R = 0: the k-means assignments), the new ones follow the rule
    old = [[int(a)] for a in asg] if R == 0 else row_lists(oracle, data, cen, metric, R)
    want = old + row_lists(oracle, new, cen, metric, R)
    off, rows = csr_of(want, cen.shape[0])
    assert np.array_equal(off0, off), metric
    assert np.array_equal(rows0, rows), metric
    assert len(idx) == allrows.shape[0]


@pytest.mark.parametrize("metric,R", [(L2, 1), (IP, 2)])
def test_build_over_more_than_65536_rows(L, oracle, metric, R):
    """70,000 rows: the top-keep FLAT search runs in two batches (65,536 + 4,464, the second with row0 > 0) and k_spann_flag
    strides its grid (8,192 blocks x 4 rows per pass).  Postings bit-equal to the rule; queries at rows of the second batch."""
    rng, data = clustered(200 + R, 70_000, 16, ncent=12, noise=0.6)
    nlist = 16
    idx = L.SpannIndex.build(data, 16, nlist, 5, NAME[metric], replica_count=R)
    cen, _ = oracle.kmeans_train(data, nlist, 5, metric)
    off, rows = csr_of(row_lists(oracle, data, cen, metric, R), cen.shape[0])
    assert_postings(idx, off, rows, (metric, R))
    at = 65_536 + rng.integers(0, 70_000 - 65_536, 8)
    queries = (data[at] + 0.01).astype(f32)
    got = idx.search_batch_arrays(queries, 10, 4)
    check_search(oracle, got, queries, data, cen, off, rows, 4, 10, metric, what=(metric, R))
    assert (got[0][:, :10] >= 65_536).any()
    if metric == L2:
        assert np.array_equal(got[0][:, 0], at.astype(np.uint64))


def test_insert_of_more_than_65536_rows(L, oracle):
    """An insert of 66,000 rows: two top-keep batches and a strided k_spann_flag grid over the new rows, whose NaN, +inf and 3e38
    rows sit before and past 32,768 and 65,536 (k_spann_slow for rows of both batches)."""
    rng, data = clustered(210, 2000, 12, ncent=6, noise=0.5)
    nlist, metric, R = 10, COS, 1
    idx = L.SpannIndex.build(data, 12, nlist, 20, NAME[metric], replica_count=R)
    cen, _ = oracle.kmeans_train(data, nlist, 20, metric)
    new = (np.repeat(data, 33, axis=0) + 0.3 * rng.standard_normal((66_000, 12))).astype(f32)
    for at in (100, 40_000, 65_800):
        new[at, 3] = np.nan
        new[at + 1, :] = np.inf
        new[at + 2, :] = f32(3e38)
    idx.insert(new)
    want = row_lists(oracle, data, cen, metric, R) + row_lists(oracle, new, cen, metric, R)
    assert_postings(idx, *csr_of(want, cen.shape[0]), "insert of 66,000 rows")
    assert len(idx) == 68_000


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_slow_rule_over_16384_centroids(L, oracle, metric):
    """k_spann_slow at nlist = 16,384 (the IVF limit): 64 KiB of ranks plus the keep slots in LDS.  Loaded over lists of the nearest
    centroid (float64), then an insert of rows with NaN, +-inf and 3e38 elements beside ordinary ones, compared with row_lists."""
    rng = np.random.default_rng(220 + metric)
    nlist, dim, R = 16_384, 8, 2
    cen = rng.standard_normal((nlist, dim)).astype(f32)
    data = rng.standard_normal((20_000, dim)).astype(f32)
    c64 = cen.astype(np.float64)
    near = np.argmin(np.sum(c64 ** 2, 1)[None] - 2 * data.astype(np.float64) @ c64.T, axis=1)
    old = [[int(c)] for c in near]
    off, rows = csr_of(old, nlist)
    idx = L.SpannIndex.load(data, cen, off, rows, R, NAME[metric])
    new = rng.standard_normal((10, dim)).astype(f32)
    new[0, 3] = np.nan
    new[1, :] = np.nan
    new[2, 5] = np.inf
    new[3, 5] = -np.inf
    new[4, :] = np.inf
    new[5, 0], new[5, 1] = np.inf, -np.inf
    new[6, :] = f32(3e38)                 # inner products overflow
    new[7, ::2], new[7, 1::2] = f32(3e38), f32(-3e38)
    idx.insert(new)
    want = old + row_lists(oracle, new, cen, metric, R)
    assert_postings(idx, *csr_of(want, nlist), metric)


@pytest.mark.parametrize("metric,sq8", [(IP, False), (L2, False), (COS, False), (L2, True)])
def test_build_at_768(L, oracle, metric, sq8):
    """D = 768: the posting rule's top-keep is the FLAT search of the rows against the centroid store at embedding width;
    postings and a search checked (SQ8: on the decoded rows, with the exact rerank)."""
    rng, data = clustered(230 + metric + 10 * sq8, 3000, 768, ncent=10, noise=0.6)
    nlist, R = 16, 2
    idx = L.SpannIndex.build(data, 768, nlist, 10, NAME[metric], replica_count=R, sq8=sq8)
    sq = sq_fit(data) if sq8 else None
    route = sq_codec(data, *sq) if sq8 else data
    cen, _ = oracle.kmeans_train(route, nlist, 10, metric)
    off, rows = csr_of(row_lists(oracle, route, cen, metric, R), cen.shape[0])
    assert_postings(idx, off, rows, (metric, sq8))
    assert rows.size > data.shape[0]
    queries = (data[rng.integers(0, data.shape[0], 12)] + 0.05 * rng.standard_normal((12, 768))).astype(f32)
    got = idx.search_batch_arrays(queries, 10, 4)
    check_search(oracle, got, queries, data, cen, off, rows, 4, 10, metric, scored=route if sq8 else None, sq=sq, what=(metric, sq8))


# ----------------------------------------------------------------------------------------- search ----
def loaded(L, oracle, data, nlist, metric, R):
    """an index over given lists: k-means of the oracle, lists by the rule (the build path is checked above)"""
    cen, _ = oracle.kmeans_train(data, nlist, 6, metric)
    off, rows = csr_of(row_lists(oracle, data, cen, metric, R), cen.shape[0])
    idx = L.SpannIndex.load(data, cen, off, rows, R, NAME[metric])
    return idx, cen, off, rows


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_search_sweep(L, oracle, metric):
    rng, data = clustered(50 + metric, 3000, 16, ncent=12, noise=0.5)
    idx, cen, off, rows = loaded(L, oracle, data, 32, metric, 2)
    for nq in (1, 7, 256, 300):
        queries = (data[rng.integers(0, data.shape[0], nq)] + 0.2 * rng.standard_normal((nq, 16))).astype(f32)
        for k in (1, 10, 100, 2000):
            for nprobe in (1, 8, 32):
                if nq >= 256 and k == 2000 and nprobe != 8:
                    continue
                got = idx.search_batch_arrays(queries, k, nprobe)
                check_search(oracle, got, queries, data, cen, off, rows, nprobe, k, metric, what=(metric, nq, k, nprobe))


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_search_large_store_runs_the_staged_and_int8_plans(L, oracle, metric):
    """65,536 rows x 256 (87K postings): few queries take the staged plan on the f16 shadow (never the fused few-query plan, which
    a SPANN store does not use), 33..256 queries start on the certified int8 pass (profile last_plan bit 6)."""
    rng = np.random.default_rng(60 + metric)
    n, dim, nlist = 65536, 256, 64
    centers = rng.standard_normal((24, dim)).astype(f32)
    data = (centers[rng.integers(0, 24, n)] + 0.4 * rng.standard_normal((n, dim))).astype(f32)
    cen = data[rng.choice(n, nlist, replace=False)].copy()
    # any lists load: primary = nearest by float64 distance, plus the second nearest for every third row
    c2 = (data.astype(np.float64) @ cen.T.astype(np.float64))
    order = np.argsort(-c2 if metric == IP else (np.sum(cen.astype(np.float64) ** 2, 1)[None] - 2 * c2), axis=1)[:, :2]
    lists = [[int(o[0])] + ([int(o[1])] if r % 3 == 0 else []) for r, o in enumerate(order)]
    off, rows = csr_of(lists, nlist)
    idx = L.SpannIndex.load(data, cen, off, rows, 1, NAME[metric])
    plans = {}
    idx.profile_enable(True)
    for nq, k, nprobe in ((1, 10, 8), (7, 100, 8), (64, 10, 8), (256, 10, 4), (256, 100, 8)):
        queries = (data[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, dim))).astype(f32)
        idx.profile_get(reset=True)
        got = idx.search_batch_arrays(queries, k, nprobe)
        plans[nq] = int(idx.profile_get(reset=True)["last_plan"])
        check_search(oracle, got, queries, data, cen, off, rows, nprobe, k, metric, what=(metric, nq, k, nprobe))
    idx.profile_enable(False)
    for nq, plan in plans.items():
        assert not plan & 32, (nq, plan)                       # bit 5: the fused few-query search
        assert bool(plan & 64) == (nq >= 33), (nq, plan)       # bit 6: started on the certified int8 pass


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_fewer_than_k_distinct_candidates_fall_back_to_all_rows(L, oracle, metric):
    rng, data = clustered(70 + metric, 800, 8, ncent=8, noise=0.2)
    idx, cen, off, rows = loaded(L, oracle, data, 40, metric, 1)
    queries = (data[rng.integers(0, 800, 9)] + 0.1 * rng.standard_normal((9, 8))).astype(f32)
    sizes = np.diff(off.astype(np.int64))
    k = int(sizes.max()) + 5        # one probed list never holds k distinct rows
    got = idx.search_batch_arrays(queries, k, 1)
    assert (got[2] == k).all()
    check_search(oracle, got, queries, data, cen, off, rows, 1, k, metric, what="fallback")
    subset = rng.choice(800, 60, replace=False)
    for kk in (5, 30, 100):
        got = idx.search_filtered_batch_arrays(queries, kk, 2, subset)
        check_search(oracle, got, queries, data, cen, off, rows, 2, kk, metric, subset=subset, what=("subset", kk))
    got = idx.search_filtered_batch_arrays(queries, 5, 2, np.array([5000, 6000]))
    assert (got[2] == 0).all()


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_sq8_search_pools(L, oracle, metric):
    rng, data = clustered(80 + metric, 4000, 16, ncent=10, noise=0.5)
    mn, sc = sq_fit(data)
    dec = sq_codec(data, mn, sc)
    cen, _ = oracle.kmeans_train(dec, 24, 6, metric)
    off, rows = csr_of(row_lists(oracle, dec, cen, metric, 2), cen.shape[0])
    idx = L.SpannIndex.load(data, cen, off, rows, 2, NAME[metric], mins=mn, scales=sc)
    assert idx.is_sq8
    g_mn, g_sc = idx.sq8_params()
    assert np.array_equal(g_mn.view(np.uint32), mn.view(np.uint32))
    # pools up to 17,000 / all rows: host-selected; 300 queries: query chunks of 256 + 44
    for nq, k, nprobe in ((1, 10, 4), (7, 1, 1), (40, 100, 8), (3, 1700, 4), (2, 3000, 24), (300, 10, 4)):
        queries = (data[rng.integers(0, 4000, nq)] + 0.2 * rng.standard_normal((nq, 16))).astype(f32)
        got = idx.search_batch_arrays(queries, k, nprobe)
        check_search(oracle, got, queries, data, cen, off, rows, nprobe, k, metric, scored=dec, sq=(mn, sc), what=(metric, nq, k, nprobe))
    subset = rng.choice(4000, 300, replace=False)
    queries = data[:5]
    got = idx.search_filtered_batch_arrays(queries, 20, 2, subset)
    check_search(oracle, got, queries, data, cen, off, rows, 2, 20, metric, subset=subset, scored=dec, sq=(mn, sc), what="sq8 subset")


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_sq8_build_postings_use_the_decoded_rows(L, oracle, metric):
    _, data = clustered(90 + metric, 1500, 12, ncent=8, noise=0.6)
    idx = L.SpannIndex.build(data, 12, 16, 20, NAME[metric], replica_count=1, sq8=True)
    mn, sc = sq_fit(data)
    dec = sq_codec(data, mn, sc)
    cen, _ = oracle.kmeans_train(dec, 16, 20, metric)
    off, rows = csr_of(row_lists(oracle, dec, cen, metric, 1), cen.shape[0])
    assert_postings(idx, off, rows, metric)


@pytest.mark.parametrize("sq8", [False, True])
@pytest.mark.parametrize("R", [0, 2])
def test_insert_then_delete_rebuilds_the_postings(L, oracle, sq8, R):
    metric = L2
    rng, data = clustered(100 + R, 1200, 10, ncent=8, noise=0.5)
    idx = L.SpannIndex.build(data, 10, 12, 20, NAME[metric], replica_count=R, sq8=sq8)
    mn, sc = sq_fit(data) if sq8 else (None, None)
    route = (lambda x: sq_codec(x, mn, sc)) if sq8 else (lambda x: x)
    cen, asg = oracle.kmeans_train(route(data), 12, 20, metric)
    new = (data[:50] + 0.3 * rng.standard_normal((50, 10))).astype(f32)
    idx.insert(new)
    allrows = np.concatenate([data, new])
    base = [[int(a)] for a in asg] if R == 0 else row_lists(oracle, route(data), cen, metric, R)
    want = base + row_lists(oracle, route(new), cen, metric, R)
    assert_postings(idx, *csr_of(want, cen.shape[0]), "insert")
    gone = np.array([0, 5, 17, 1100, 1210, 99999])
    idx.delete(gone)
    keep = np.setdiff1d(np.arange(allrows.shape[0]), gone)
    kept = allrows[keep]
    want = row_lists(oracle, route(kept), cen, metric, R)
    off, rows = csr_of(want, cen.shape[0])
    assert_postings(idx, off, rows, "delete")
    assert len(idx) == kept.shape[0]
    queries = kept[:6]
    got = idx.search_batch_arrays(queries, 10, 3)
    if sq8:
        check_search(oracle, got, queries, kept, cen, off, rows, 3, 10, metric, scored=route(kept), sq=(mn, sc), what="after delete")
    else:
        check_search(oracle, got, queries, kept, cen, off, rows, 3, 10, metric, what="after delete")


def test_refused_entry_points(L):
    import ctypes as C

    from lynsedb_amd import _lib
    from lynsedb_amd.core import IvfFlatIndex

    data = np.random.default_rng(3).standard_normal((300, 8)).astype(f32)
    idx = L.SpannIndex.build(data, 8, 6, 10, "l2", replica_count=1)
    view = IvfFlatIndex(idx._h, 8)
    try:
        with pytest.raises(_lib.LynseUnsupportedError):
            view.search_metric_batch_arrays(data[:2], 5, 2, "ip")
        with pytest.raises(_lib.LynseUnsupportedError):
            view.assign(data[:2])
        with pytest.raises(_lib.LynseUnsupportedError):
            view.export()
        with pytest.raises(_lib.LynseUnsupportedError):
            _lib.check(_lib.lib.lynse_hip_ivf_set_row_map(idx._h, 2, 0))
        for routing in (0, 1, 2):
            with pytest.raises(_lib.LynseUnsupportedError):
                _lib.check(_lib.lib.lynse_hip_ivf_set_routing(idx._h, routing))
        with pytest.raises(_lib.LynseUnsupportedError):
            _lib.check(_lib.lib.lynse_hip_ivf_set_fused_search(idx._h, 1))
        import torch
        dq = torch.zeros((1, 8), dtype=torch.float32, device="cuda")
        dr = torch.zeros((1, 5), dtype=torch.int64, device="cuda")
        dd = torch.zeros((1, 5), dtype=torch.float32, device="cuda")
        dc = torch.zeros(1, dtype=torch.int32, device="cuda")
        with pytest.raises(_lib.LynseUnsupportedError):
            _lib.check(_lib.lib.lynse_hip_ivf_search_f32_device(idx._h, C.c_void_p(dq.data_ptr()), 1, 5, 2, C.c_void_p(dr.data_ptr()),
                                                                C.c_void_p(dd.data_ptr()), C.c_void_p(dc.data_ptr())))
        t = C.c_void_p()
        with pytest.raises(_lib.LynseUnsupportedError):
            _lib.check(_lib.lib.lynse_hip_ivf_search_submit_f32_device(idx._h, None, C.c_void_p(dq.data_ptr()), 1, 5, 2, C.c_void_p(dr.data_ptr()),
                                                                       C.c_void_p(dd.data_ptr()), C.c_void_p(dc.data_ptr()), C.byref(t)))
    finally:
        view._h = None
    for m in ("hamming", "jaccard"):
        with pytest.raises(_lib.LynseUnsupportedError):
            L.SpannIndex.build(data, 8, 6, 10, m)
    flat = IvfFlatIndex.build(None, data, 8, 4, 5, "ip", l2_partitions=False)
    with pytest.raises(ValueError):
        _lib.check(_lib.lib.lynse_hip_spann_postings(flat._h, None, None, None))


@pytest.mark.parametrize("sq8", [False, True])
@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_short_results_are_padded(L, oracle, metric, sq8):
    """Results shorter than k (k above the rows, a subset smaller than k, a subset outside the index) end in row ~0 and the worst
    distance of the metric, as every search of the C ABI does (include/lynse_hip.h conventions)."""
    rng, data = clustered(120 + metric, 300, 8, ncent=4, noise=0.4)
    idx = L.SpannIndex.build(data, 8, 6, 10, NAME[metric], replica_count=2, sq8=sq8)
    worst = np.float32(-np.inf if metric == IP else np.inf)
    queries = data[:5]
    cases = [(idx.search_batch_arrays(queries, 400, 2), 300),
             (idx.search_filtered_batch_arrays(queries, 10, 1, np.array([3, 77, 150])), 3),
             (idx.search_filtered_batch_arrays(queries, 10, 1, np.array([1000, 2000])), 0)]
    for (r, d, c), want in cases:
        assert (c == want).all(), (c, want)
        assert (r[:, want:] == np.uint64(~np.uint64(0))).all()
        assert (d[:, want:] == worst).all()
        assert np.isfinite(d[:, :want]).all()
        assert all(len(set(row[:want].tolist())) == want for row in r)   # distinct rows


def test_load_refuses_lists_the_search_cannot_serve(L):
    rng = np.random.default_rng(5)
    data = rng.standard_normal((6, 4)).astype(f32)
    cen = data[:2].copy()
    ok_off, ok_rows = np.array([0, 4, 8], np.uint64), np.array([0, 1, 2, 3, 2, 3, 4, 5], np.uint32)
    L.SpannIndex.load(data, cen, ok_off, ok_rows, 1, "l2")
    with pytest.raises(ValueError):   # row 0 in no list
        L.SpannIndex.load(data, cen, np.array([0, 3, 7], np.uint64), np.array([1, 2, 3, 2, 3, 4, 5], np.uint32), 1, "l2")
    with pytest.raises(ValueError):   # row 2 in two lists with replica_count 0
        L.SpannIndex.load(data, cen, ok_off, ok_rows, 0, "l2")
    with pytest.raises(ValueError):   # row 0 twice in list 0
        L.SpannIndex.load(data, cen, np.array([0, 5, 9], np.uint64), np.array([0, 0, 1, 2, 3, 2, 3, 4, 5], np.uint32), 1, "l2")


def test_k_zero_and_empty_results(L):
    data = np.random.default_rng(4).standard_normal((200, 6)).astype(f32)
    idx = L.SpannIndex.build(data, 6, 5, 10, "ip", replica_count=1)
    _, _, c = idx.search_batch_arrays(data[:3], 0, 2)
    assert (c == 0).all()
    idx.delete(np.arange(200))
    assert len(idx) == 0
    from lynsedb_amd import _lib

    with pytest.raises(_lib.LynseHipError):   # LYNSE_ERR_INDEX_NOT_BUILT
        idx.search_batch_arrays(data[:1], 3, 2)


# ------------------------------------------------------------------------- the reference's own cases ----
def test_reference_unit_cases(L):
    """spann.rs:595-667"""
    data = np.array([[0, 0], [1, 0], [0, 1], [5, 5], [5.2, 5], [5, 5.2]], f32)
    ids = np.array([10, 11, 12, 13, 14, 15])
    idx = L.SpannIndex.build(data, 2, 2, 20, "l2", replica_count=1)
    r, d, c = idx.search_batch_arrays(np.array([[5.1, 5.0]], f32), 2, 2)
    assert int(c[0]) == 2 and ids[int(r[0, 0])] in (13, 14) and d[0, 0] <= d[0, 1]
    data2 = np.array([[0, 0], [1, 0], [5, 5], [5.1, 5]], f32)
    idx2 = L.SpannIndex.build(data2, 2, 2, 20, "l2", replica_count=1)
    r, _, c = idx2.search_filtered_batch_arrays(np.array([[5.1, 5.0]], f32), 2, 1, np.array([0, 1]))
    assert int(c[0]) == 2 and all(int(x) <= 1 for x in r[0, :2])
    data3 = np.array([[0, 0], [0.2, 0], [0, 0.2], [5, 5], [5.2, 5], [5, 5.2]], f32)
    idx3 = L.SpannIndex.build(data3, 2, 2, 20, "l2", replica_count=1, sq8=True)
    r, d, c = idx3.search_batch_arrays(np.array([[5.1, 5.0]], f32), 2, 2)
    assert int(c[0]) == 2 and np.isfinite(d[0, :2]).all()


@pytest.mark.parametrize("mode", ["SPANN-IP", "SPANN-L2", "SPANN-COS", "SPANN-COSINE", "SPANN-IP-SQ8", "SPANN-L2-SQ8", "SPANN-COS-SQ8",
                                  "SPANN-COSINE-SQ8"])
def test_collection_modes(L, oracle, mode):
    from lynsedb_amd.core import spann_mode_of

    metric, sq8 = spann_mode_of(mode)
    rng, data = clustered(110, 900, 8, ncent=6, noise=0.4)
    c = L.Collection("c", 8)
    c.add_items(data[:800], list(range(1000, 1800)))
    c.commit()
    c.build_index(mode, {"n_clusters": 8, "nprobe": 3, "replica_count": 2})
    assert "SPANN" in c._index_mode and c._ivf.replica_count == 2 and c._ivf.is_sq8 == sq8
    c.add_items(data[800:], list(range(1800, 1900)))   # committed after the build: inserted lazily
    c.commit()
    res = c.search(data[850], k=5)
    assert len(res) == 5
    if metric != IP:   # (under IP the best row need not be the query itself)
        assert int(res.ids()[0]) == 1850
    assert len(c._ivf) == 900
    # the index's own answer, composed
    idx = c._ivf
    off, rows = idx.postings()
    route = data if not sq8 else sq_codec(data, *idx.sq8_params())
    cen, _ = oracle.kmeans_train(route[:800], 8, 20, metric)
    got = idx.search_batch_arrays(data[[3, 850]], 7, 3)
    check_search(oracle, got, data[[3, 850]], data, cen, off, rows, 3, 7, metric, scored=route if sq8 else None,
                 sq=idx.sq8_params() if sq8 else None, what=mode)
    res = c.search(data[3], k=4, subset=np.array([0, 1, 2, 3, 4]))
    assert set(int(x) for x in res.ids()) <= {1000, 1001, 1002, 1003, 1004}
    c.delete_items([1003])
    assert 1003 not in [int(x) for x in c.search(data[3], k=4).ids()]
    prof = c.search_profile(data[3], k=4)
    assert prof["profile"]["index_path"] == "ann_index"
    if sq8:
        assert prof["profile"]["rerank_us"] > 0
    c.add_items(data[:2], [5000, 5001])               # pending rows merge into the results
    top = c.search(data[0], k=1).ids()
    assert len(top) == 1 and (metric == IP or int(top[0]) in (1000, 5000))


def test_collection_refusals(L):
    c = L.Collection("c", 4)
    with pytest.raises(ValueError, match="^Empty database$"):
        c.build_index("SPANN-IP")
    c.add_items(np.ones((3, 4), f32), [1, 2, 3])
    with pytest.raises(ValueError, match="Unknown index type"):
        c.build_index("SPANN-HAMMING")
    with pytest.raises(ValueError, match="^Invalid argument: replica_count must be greater than 0$"):
        c.build_index("SPANN-L2", {"replica_count": 0})
