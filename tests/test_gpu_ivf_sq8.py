"""GPU parity tests for IVF-{IP,L2,COS}-SQ8: IVFIndex with QuantizerType::Scalar (src/index/ivf.rs:132-337, ScalarQuantizer
quantizer/mod.rs:110-250) through the C ABI against a composition of the existing oracle.

Expected values: the quantizer restated in numpy (f32 arithmetic, rules in include/lynse_hip.h), oracle.kmeans_train on the
decoded rows, oracle.ivf_search / ivf_search_filtered of the decoded query over the decoded rows with k = pool, then
oracle.compute_distance(query, row) on the ORIGINAL query and rows per pool entry and the canonical (distance, row) order."""
import numpy as np
import pytest

import oracle as O
from conftest import oracle_for_every_query

pytestmark = pytest.mark.gpu
IP, L2, COS = O.IP, O.L2, O.COS
NAME = {IP: "ip", L2: "l2", COS: "cosine"}
f32 = np.float32
FMAX = np.finfo(f32).max


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


# ------------------------------------------------------------------------------------- restatement ----
def sq_fit(data):
    """ScalarQuantizer::fit: min from f32::MAX / max from f32::MIN with strict comparisons (NaN never wins)."""
    col_lo = np.where(np.isnan(data), np.inf, data).min(axis=0)
    col_hi = np.where(np.isnan(data), -np.inf, data).max(axis=0)
    mn = np.minimum(col_lo, FMAX).astype(f32)
    mx = np.maximum(col_hi, -FMAX).astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        rng = (mx - mn).astype(f32)
        sc = np.where(rng == 0, f32(1.0), (rng / f32(255.0)).astype(f32)).astype(f32)
    return mn, sc


def sq_codec(x, mn, sc):
    """decode(encode(x)): ((v - min) / scale).clamp(0, 255) as u8 (NaN -> 0), then fl(fl(code * scale) + min)."""
    with np.errstate(all="ignore"):
        t = ((np.asarray(x, f32) - mn).astype(f32) / sc).astype(f32)
        t = np.where(np.isnan(t), f32(0), t)
        code = np.trunc(np.clip(t, 0, 255)).astype(np.uint8)
        return ((code.astype(f32) * sc).astype(f32) + mn).astype(f32)


def canonical(ids, dists, metric):
    dists = (np.asarray(dists, f32) + f32(0)).astype(f32)
    ids = np.asarray(ids, np.uint64)
    key = -dists.astype(np.float64) if metric == IP else dists.astype(np.float64)
    order = np.lexsort((ids, key))
    return ids[order], dists[order]


def expected(oracle, q, data, dec, cen, off, rows, nprobe, k, metric, mn, sc, subset=None):
    qd = sq_codec(q[None, :], mn, sc)[0]
    pool = min(max(10 * k, k), data.shape[0])
    if subset is None:
        p_ids, _, _ = oracle.ivf_search(qd, dec, cen, off, rows, nprobe, pool, metric)
    else:
        p_ids, _ = oracle.ivf_search_filtered(qd, dec, cen, off, rows, nprobe, pool, metric, subset)
    ex = np.array([oracle.compute_distance(q, data[int(r)], metric) for r in p_ids], f32)
    ids, d = canonical(p_ids, ex, metric)
    c = min(k, len(ids))
    return ids[:c], d[:c]


def check(oracle, got, queries, data, dec, cen, asg, nprobe, k, metric, mn, sc, subset=None, what=""):
    off, rows = oracle.lists_from_assignments(asg, cen.shape[0])
    g_rows, g_d, g_c = got
    want = oracle_for_every_query(lambda qi: expected(oracle, queries[qi], data, dec, cen, off, rows, nprobe, k, metric, mn, sc, subset),
                                  queries.shape[0])
    for qi, (e_ids, e_d) in enumerate(want):
        c = int(g_c[qi])
        assert c == len(e_ids), (what, qi, c, len(e_ids))
        assert np.array_equal(g_rows[qi, :c].astype(np.uint64), e_ids), (what, qi, g_rows[qi, :c], e_ids)
        assert np.array_equal(g_d[qi, :c].view(np.uint32), e_d.view(np.uint32)), (what, qi, g_d[qi, :c], e_d)


def clustered(seed, n, dim, ncent=12, noise=0.3):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((ncent, dim)).astype(f32)
    data = (centers[rng.integers(0, ncent, n)] + noise * rng.standard_normal((n, dim))).astype(f32)
    return rng, data


def loaded(L, oracle, data, nlist, metric, iters=8):
    """An SQ8 index with the oracle's k-means on the decoded rows, loaded through load_sq8 (k-means out of the comparison)."""
    mn, sc = sq_fit(data)
    dec = sq_codec(data, mn, sc)
    cen, asg = oracle.kmeans_train(dec, nlist, iters, metric)
    idx = L.IvfFlatIndex.load_sq8(data, cen, asg, mn, sc, NAME[metric])
    return idx, mn, sc, dec, cen, asg


# -------------------------------------------------------------------------------------- quantizer ----
def _sq8_params_case(L, seed, dim, const, nan, neg, inf):
    rng = np.random.default_rng(seed)
    n = 1500
    data = rng.standard_normal((n, dim)).astype(f32)
    data[:, const] = 2.5                                # constant dimension: scale 1.0
    data[::7, nan] = np.nan                             # NaN elements among finite ones never win min / max
    data[:, neg] = -np.abs(data[:, neg]) - 3.0          # negative-only values
    data[11, inf] = np.inf                              # +inf is a max like any other value
    for metric in (IP, L2, COS):
        idx = L.IvfFlatIndex.build(None, data, dim, 8, 5, NAME[metric], quantizer="sq8")
        mn, sc = idx.sq8_params()
        e_mn, e_sc = sq_fit(data)
        assert np.array_equal(mn.view(np.uint32), e_mn.view(np.uint32)), (mn, e_mn)
        assert np.array_equal(sc.view(np.uint32), e_sc.view(np.uint32)), (sc, e_sc)
        assert sc[const] == 1.0


def test_sq8_params_bit_equal_to_the_restatement(L):
    _sq8_params_case(L, 1, 24, 3, 5, 9, 12)


@pytest.mark.parametrize("dim,cols", [(300, (259, 261, 265, 268)), (768, (259, 517, 265, 524))])
def test_sq8_params_past_the_first_column_block(L, dim, cols):
    """k_ivfsq_minmax / k_ivfsq_fit cover 256 columns per blockIdx.x: D = 300 and 768 take two and three column blocks, with the
    constant, NaN-laced, negative-only and +inf columns in the second (and third) one."""
    _sq8_params_case(L, dim, dim, *cols)


def test_sq8_is_refused_for_binary_metrics_and_non_sq8_handles(L):
    data = np.random.default_rng(2).standard_normal((100, 8)).astype(f32)
    with pytest.raises(ValueError):   # LYNSE_ERR_INVALID_ARGUMENT
        L.IvfFlatIndex.build(None, data, 8, 4, 5, "hamming", quantizer="sq8")
    flat = L.IvfFlatIndex.build(None, data, 8, 4, 5, "ip", l2_partitions=False)
    with pytest.raises(ValueError):
        flat.sq8_params()


# --------------------------------------------------------------------------------------- training ----
AT_768 = [pytest.param(IP, 24, id="0"), pytest.param(L2, 24, id="1"), pytest.param(COS, 24, id="2"),
          pytest.param(IP, 768, id="768-0"), pytest.param(L2, 768, id="768-1"), pytest.param(COS, 768, id="768-2")]


@pytest.mark.parametrize("metric,dim", AT_768)
def test_sq8_build_trains_on_the_decoded_rows(L, oracle, metric, dim):
    """D = 768: the device quantiser over three column blocks, k-means on the decoded rows at embedding width."""
    _, data = clustered(10 + metric + (0 if dim == 24 else dim), 3000, dim)
    idx = L.IvfFlatIndex.build(None, data, dim, 16, 20, NAME[metric], quantizer="sq8")
    mn, sc = idx.sq8_params()
    dec = sq_codec(data, mn, sc)
    e_cen, e_asg = oracle.kmeans_train(dec, 16, 20, metric)
    cen, asg, _, _ = idx.export()
    assert np.array_equal(cen.view(np.uint32), e_cen.view(np.uint32))
    assert np.array_equal(asg, e_asg)
    queries = (data[:20] + 0.05).astype(f32)
    check(oracle, idx.search_batch_arrays(queries, 10, 4), queries, data, dec, e_cen, e_asg, 4, 10, metric, mn, sc, what="built")


# ----------------------------------------------------------------------------------------- search ----
@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_sq8_search_sweep(L, oracle, metric):
    rng, data = clustered(20 + metric, 6000, 40)
    nlist = 32
    idx, mn, sc, dec, cen, asg = loaded(L, oracle, data, nlist, metric)
    allq = (data[rng.integers(0, data.shape[0], 256)] + 0.1 * rng.standard_normal((256, 40))).astype(f32)
    for nq in (1, 8, 40, 256):
        queries = allq[:nq]
        for k in (1, 10, 100):
            for nprobe in (1, 8, nlist):
                check(oracle, idx.search_batch_arrays(queries, k, nprobe), queries, data, dec, cen, asg, nprobe, k, metric, mn, sc,
                      what=(nq, k, nprobe))
    # nq = 600: query chunks of 256 / 256 / 88, each with its own codec, pool stage and rerank
    more = (data[rng.integers(0, data.shape[0], 344)] + 0.1 * rng.standard_normal((344, 40))).astype(f32)
    queries = np.concatenate([allq, more])
    check(oracle, idx.search_batch_arrays(queries, 10, 8), queries, data, dec, cen, asg, 8, 10, metric, mn, sc, what="nq=600")


def test_sq8_pool_stage_plans(L, oracle):
    """The pool stage is the IVF-Flat search over the decoded slab: one query takes the fused few-query path, a handful the
    staged path, and 33-256 IP queries over >= 64K rows of whole 128-column slabs start on the certified int8 pass."""
    rng, data = clustered(31, 70_000, 128, ncent=24)
    idx, mn, sc, dec, cen, asg = loaded(L, oracle, data, 64, IP, iters=4)
    queries = (data[rng.integers(0, data.shape[0], 64)] + 0.05 * rng.standard_normal((64, 128))).astype(f32)
    idx.profile_enable(True)
    for nq, k, nprobe, bit in ((1, 1, 8, 32), (8, 10, 8, None), (64, 10, 8, 64)):
        idx.profile_get(reset=True)
        got = idx.search_batch_arrays(queries[:nq], k, nprobe)
        plan = int(idx.profile_get(reset=True)["last_plan"])
        if bit is None:
            assert plan & (32 | 64) == 0, plan
        else:
            assert plan & bit, (nq, plan)
        check(oracle, got, queries[:nq], data, dec, cen, asg, nprobe, k, IP, mn, sc, what=("plan", nq))
    idx.profile_enable(False)


def test_sq8_pool_stage_int8_plan_at_768(L, oracle):
    """The certified int8 pass at embedding width: 64 IP queries over 66,000 rows of six whole 128-column slabs (D = 768).  Any
    lists load: each decoded row goes to its best of 64 sampled decoded rows by a float64 inner product (no k-means restatement
    at this size)."""
    rng, data = clustered(33, 66_000, 768, ncent=24)
    mn, sc = sq_fit(data)
    dec = sq_codec(data, mn, sc)
    cen = dec[rng.choice(data.shape[0], 64, replace=False)].copy()
    asg = np.argmax(dec.astype(np.float64) @ cen.T.astype(np.float64), axis=1).astype(np.uint32)
    idx = L.IvfFlatIndex.load_sq8(data, cen, asg, mn, sc, "ip")
    queries = (data[rng.integers(0, data.shape[0], 64)] + 0.05 * rng.standard_normal((64, 768))).astype(f32)
    idx.profile_enable(True)
    idx.profile_get(reset=True)
    got = idx.search_batch_arrays(queries, 10, 8)
    plan = int(idx.profile_get(reset=True)["last_plan"])
    idx.profile_enable(False)
    assert plan & 64, plan
    check(oracle, got, queries, data, dec, cen, asg, 8, 10, IP, mn, sc, what="int8 plan at 768")


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_sq8_rerank_lds_boundary_at_768(L, oracle, metric):
    """D = 768, 16,400 rows, every list probed.  k = 1,638: a pool of 16,380 keys, sorted in LDS beside the 3 KiB query.
    k = 1,639: a pool of 16,390 > 16,384, scored on the device and selected on the host."""
    rng, data = clustered(170 + metric, 16_400, 768, ncent=8)
    idx, mn, sc, dec, cen, asg = loaded(L, oracle, data, 8, metric, iters=2)
    q = (data[rng.integers(0, data.shape[0], 2)] + 0.05 * rng.standard_normal((2, 768))).astype(f32)
    for k, pool in ((1638, 16_380), (1639, 16_390)):
        assert min(10 * k, data.shape[0]) == pool and (pool <= 16_384) == (k == 1638)
        got = idx.search_batch_arrays(q, k, 8)
        assert (got[2] == k).all()
        check(oracle, got, q, data, dec, cen, asg, 8, k, metric, mn, sc, what=("rerank", k))


@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_sq8_pool_edges(L, oracle, metric):
    # pool > candidates: short lists, nprobe 1
    rng, data = clustered(40 + metric, 2000, 16)
    idx, mn, sc, dec, cen, asg = loaded(L, oracle, data, 64, metric)
    q = (data[:6] + 0.02).astype(f32)
    check(oracle, idx.search_batch_arrays(q, 10, 1), q, data, dec, cen, asg, 1, 10, metric, mn, sc, what="short lists")
    # every probed list empty -> the whole corpus: an extra centroid that owns no row, placed where the DECODED query ranks it first
    qd = sq_codec(q[:1], mn, sc)[0]
    extra = qd if metric == L2 else (1000.0 * qd).astype(f32)
    cen2 = np.concatenate([cen, extra[None, :]]).astype(f32)
    idx2 = L.IvfFlatIndex.load_sq8(data, cen2, asg, mn, sc, NAME[metric])
    check(oracle, idx2.search_batch_arrays(q[:1], 5, 1), q[:1], data, dec, cen2, asg, 1, 5, metric, mn, sc, what="empty probes")
    # k = 10,000 on a small index: the pool is the whole corpus, every row comes back
    got = idx.search_batch_arrays(q[:2], 10_000, 64)
    assert int(got[2][0]) == data.shape[0]
    check(oracle, got, q[:2], data, dec, cen, asg, 64, 10_000, metric, mn, sc, what="k=10000")


@pytest.mark.parametrize("metric", [IP, L2])
def test_sq8_large_pools(L, oracle, metric):
    rng, data = clustered(50 + metric, 25_000, 16)
    idx, mn, sc, dec, cen, asg = loaded(L, oracle, data, 16, metric, iters=4)
    q = (data[rng.integers(0, data.shape[0], 3)] + 0.05).astype(f32)
    # k = 500: pool 5,000 > 4,096 -> the pool stage takes the large-k path, the rerank still selects in LDS
    check(oracle, idx.search_batch_arrays(q, 500, 6), q, data, dec, cen, asg, 6, 500, metric, mn, sc, what="k=500")
    # k = 2,000: pool 20,000 > 16,384 -> scored on the device, selected on the host
    check(oracle, idx.search_batch_arrays(q[:2], 2000, 16), q[:2], data, dec, cen, asg, 16, 2000, metric, mn, sc, what="k=2000")


# --------------------------------------------------------------------------------------- filtered ----
@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_sq8_filtered(L, oracle, metric):
    rng, data = clustered(60 + metric, 5000, 32)
    idx, mn, sc, dec, cen, asg = loaded(L, oracle, data, 24, metric)
    q = (data[rng.integers(0, 5000, 12)] + 0.05 * rng.standard_normal((12, 32))).astype(f32)
    subset = np.sort(rng.choice(5000, 1500, replace=False)).astype(np.uint64)
    for k, nprobe in ((10, 3), (40, 24)):
        got = idx.search_filtered_batch_arrays(q, k, nprobe, subset)
        check(oracle, got, q, data, dec, cen, asg, nprobe, k, metric, mn, sc, subset=subset, what=("subset", k, nprobe))
    # a subset disjoint from the probed lists: the rows of one list the query does not probe -> answered from the subset
    off, rows = oracle.lists_from_assignments(asg, cen.shape[0])
    probed = set(int(c) for c in oracle.ivf_search(sq_codec(q[:1], mn, sc)[0], dec, cen, off, rows, 1, 5, metric)[2])
    other = next(c for c in range(cen.shape[0]) if c not in probed and off[c + 1] > off[c])
    sub2 = np.sort(rows[int(off[other]):int(off[other + 1])]).astype(np.uint64)
    got = idx.search_filtered_batch_arrays(q[:1], 5, 1, sub2)
    check(oracle, got, q[:1], data, dec, cen, asg, 1, 5, metric, mn, sc, subset=sub2, what="disjoint subset")


# ------------------------------------------------------------------------------------ insert / delete ----
@pytest.mark.parametrize("metric,dim", AT_768)
def test_sq8_insert_clamps_and_delete_reassigns(L, oracle, metric, dim):
    rng, data = clustered(70 + metric + (0 if dim == 24 else dim), 4000, dim)
    idx, mn, sc, dec, cen, asg = loaded(L, oracle, data, 16, metric)
    new = (3.0 * rng.standard_normal((300, dim))).astype(f32)         # partly outside the fitted range: the codes clamp
    idx.insert(new)
    mn2, sc2 = idx.sq8_params()
    assert np.array_equal(mn2.view(np.uint32), mn.view(np.uint32)) and np.array_equal(sc2.view(np.uint32), sc.view(np.uint32))
    all_rows = np.concatenate([data, new]).astype(f32)
    all_dec = sq_codec(all_rows, mn, sc)
    asg_all = np.concatenate([asg, oracle.kmeans_assign(all_dec[4000:], cen, metric)]).astype(np.uint32)
    _, g_asg, _, _ = idx.export()
    assert np.array_equal(g_asg, asg_all)
    q = (all_rows[rng.integers(0, 4300, 10)] + 0.05).astype(f32)
    check(oracle, idx.search_batch_arrays(q, 10, 4), q, all_rows, all_dec, cen, asg_all, 4, 10, metric, mn, sc, what="insert")
    gone = np.sort(rng.choice(4300, 700, replace=False))
    idx.delete(gone)
    keep = np.setdiff1d(np.arange(4300), gone)
    left, left_dec = all_rows[keep], all_dec[keep]
    asg_left = oracle.kmeans_assign(left_dec, cen, metric)
    assert len(idx) == keep.size
    check(oracle, idx.search_batch_arrays(q, 10, 4), q, left, left_dec, cen, asg_left, 4, 10, metric, mn, sc, what="delete")


# -------------------------------------------------------------------------------------- refusals ----
def test_sq8_refused_entry_points(L):
    import ctypes as C

    import torch

    _, data = clustered(80, 2000, 16)
    idx = L.IvfFlatIndex.build(None, data, 16, 8, 5, "l2", quantizer="sq8")
    with pytest.raises(L._lib.LynseUnsupportedError):
        idx.search_metric_batch_arrays(data[:2], 5, 2, "l2")
    dev = torch.device("cuda", 0)
    dq = torch.as_tensor(data[:2], device=dev)
    r = torch.zeros((2, 5), dtype=torch.int64, device=dev)
    d = torch.zeros((2, 5), dtype=torch.float32, device=dev)
    c = torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(L._lib.LynseUnsupportedError):
        idx.search_submit(dq, 5, 2, r, d, c)
    with pytest.raises(L._lib.LynseUnsupportedError):
        L._lib.check(L._lib.lib.lynse_hip_ivf_set_row_map(idx._h, C.c_uint64(2), C.c_uint64(1)))
    # the device-resident search of an SQ8 index is the blocking one with device buffers
    idx.search_device(dq, 5, 2, r, d, c)
    g = idx.search_batch_arrays(data[:2], 5, 2)
    assert np.array_equal(r.cpu().numpy().astype(np.uint64), g[0]) and np.array_equal(d.cpu().numpy(), g[1])
    assert np.array_equal(c.cpu().numpy().astype(np.uint32), g[2])


# ------------------------------------------------------------------------------------- Collection ----
def compose(L, rows_committed, ids, pending, pending_ids, tomb, q, k, metric, nlist, nprobe):
    """What Collection.search answers for an IVF-*-SQ8 index: the SQ8 index over the committed rows (k + |tombstones|), the
    pending rows merged by exact distance, tombstoned ids dropped."""
    from lynsedb_amd.core import py_top_k_search
    from lynsedb_amd.shard_node import filter_tombstoned_limit, merge_row_results

    idx = L.IvfFlatIndex.build(None, rows_committed, rows_committed.shape[1], nlist, 20, NAME[metric], quantizer="sq8")
    sk = k + len(tomb)
    g_rows, g_d, g_c = idx.search_batch_arrays(q[None, :], sk, nprobe)
    r, d = g_rows[0, :int(g_c[0])], g_d[0, :int(g_c[0])]
    p_i, p_d = py_top_k_search(q, pending, NAME[metric], sk)
    r, d = merge_row_results(r, d, (np.asarray(p_i, np.int64) + rows_committed.shape[0]).astype(np.uint64), p_d, sk, metric)
    all_ids = np.concatenate([ids, pending_ids]).astype(np.uint64)
    return filter_tombstoned_limit(all_ids[np.asarray(r, np.int64)], d, np.asarray(sorted(tomb), np.uint64), k)


@pytest.mark.parametrize("mode,metric", [("IVF-IP-SQ8", IP), ("IVF-L2-SQ8", L2), ("IVF-COS-SQ8", COS), ("IVF-COSINE-SQ8", COS)])
def test_collection_ivf_sq8_modes(L, mode, metric):
    rng, data = clustered(90, 3000, 16)
    ids = np.arange(1000, 4000)
    col = L.Collection("c", 16)
    col.add_items(data, ids.tolist())
    col.commit()
    col.build_index(mode, {"n_clusters": 12, "nprobe": 3})
    pending = (data[:40] + 0.01).astype(f32)
    col.add_items(pending, list(range(9000, 9040)))
    tomb = {1000 + 5, 1000 + 77, 9003}
    col.delete_items(sorted(tomb))
    q = (data[5] + 0.02).astype(f32)
    res = col.search(q, 10)
    assert res.index_mode() == mode
    e_ids, e_d = compose(L, data, ids, pending, np.arange(9000, 9040), tomb, q, 10, metric, 12, 3)
    assert np.array_equal(np.asarray(res.ids(), np.int64), np.asarray(e_ids, np.int64))
    assert np.array_equal(np.asarray(res.distances(), f32).view(np.uint32), np.asarray(e_d, f32).view(np.uint32))
    prof = col.search_profile(q, 10)["profile"]
    assert prof["index_path"] == "ann_index" and prof["device"]["rescored_candidates"] > 0


def test_collection_cos_aliases_agree_and_pq_refused(L):
    _, data = clustered(91, 2000, 16)
    out = []
    for mode in ("IVF-COS-SQ8", "IVF-COSINE-SQ8"):
        col = L.Collection("c", 16)
        col.add_items(data, list(range(2000)))
        col.commit()
        col.build_index(mode, {"n_clusters": 8, "nprobe": 2})
        res = col.search((data[3] + 0.1).astype(f32), 10)
        out.append((np.asarray(res.ids()), np.asarray(res.distances(), f32)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
    col = L.Collection("c", 16)
    col.add_items(data, list(range(2000)))
    col.commit()
    with pytest.raises(NotImplementedError):
        col.build_index("IVF-IP-PQ")


# ------------------------------------------------------------------------------------- odd widths ----
@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_sq8_odd_dimension(L, oracle, metric):
    """D = 37: the exact_score tail (D % 8), the LDS query staging, the codec and the raw-row gather on a width that is no
    multiple of 4 or 8 — search, insert and delete."""
    rng, data = clustered(100 + metric, 3000, 37)
    idx, mn, sc, dec, cen, asg = loaded(L, oracle, data, 16, metric)
    q = (data[rng.integers(0, 3000, 40)] + 0.05 * rng.standard_normal((40, 37))).astype(f32)
    for nq, k, nprobe in ((1, 10, 3), (40, 10, 3), (40, 100, 16)):
        check(oracle, idx.search_batch_arrays(q[:nq], k, nprobe), q[:nq], data, dec, cen, asg, nprobe, k, metric, mn, sc,
              what=("odd", nq, k, nprobe))
    new = (2.0 * rng.standard_normal((50, 37))).astype(f32)
    idx.insert(new)
    all_rows = np.concatenate([data, new]).astype(f32)
    all_dec = sq_codec(all_rows, mn, sc)
    asg_all = np.concatenate([asg, oracle.kmeans_assign(all_dec[3000:], cen, metric)]).astype(np.uint32)
    gone = np.sort(rng.choice(3050, 400, replace=False))
    idx.delete(gone)
    keep = np.setdiff1d(np.arange(3050), gone)
    asg_left = oracle.kmeans_assign(all_dec[keep], cen, metric)
    check(oracle, idx.search_batch_arrays(q, 10, 4), q, all_rows[keep], all_dec[keep], cen, asg_left, 4, 10, metric, mn, sc,
          what="odd delete")


# ----------------------------------------------------------------------------------------- assign ----
@pytest.mark.parametrize("metric", [IP, L2, COS])
def test_sq8_assign_routes_the_decoded_rows(L, oracle, metric):
    """lynse_hip_ivf_assign_f32 on an SQ8 index = kmeans::assign_metric of decode(encode(rows)) under the fitted quantizer (rows
    partly outside its range clamp)."""
    rng, data = clustered(110 + metric, 2500, 29)
    idx, mn, sc, dec, cen, asg = loaded(L, oracle, data, 12, metric)
    rows = np.concatenate([data[:200], (3.0 * rng.standard_normal((100, 29))).astype(f32)]).astype(f32)
    got = idx.assign(rows)
    assert np.array_equal(got, oracle.kmeans_assign(sq_codec(rows, mn, sc), cen, metric))


# ------------------------------------------------------------------------- device outputs, host select ----
def test_sq8_device_search_with_host_selected_pool(L, oracle):
    """search_device at k = 2,000 (pool 20,000 > 16,384): the rerank scores on the device, the host selects and uploads into the
    caller's device buffers — the same as the host-output search and the oracle composition."""
    import torch

    rng, data = clustered(120, 25_000, 16)
    idx, mn, sc, dec, cen, asg = loaded(L, oracle, data, 16, L2, iters=4)
    q = (data[rng.integers(0, data.shape[0], 2)] + 0.05).astype(f32)
    k = 2000
    dev = torch.device("cuda", 0)
    r = torch.zeros((2, k), dtype=torch.int64, device=dev)
    d = torch.zeros((2, k), dtype=torch.float32, device=dev)
    c = torch.zeros(2, dtype=torch.int32, device=dev)
    idx.search_device(torch.as_tensor(q, device=dev), k, 16, r, d, c)
    got = (r.cpu().numpy().view(np.uint64), d.cpu().numpy(), c.cpu().numpy().astype(np.uint32))
    check(oracle, got, q, data, dec, cen, asg, 16, k, L2, mn, sc, what="device k=2000")
    # 600 device-resident queries: query chunks of 256 / 256 / 88 read from and written to each chunk's offset in the device buffers
    q = (data[rng.integers(0, data.shape[0], 600)] + 0.05 * rng.standard_normal((600, 16))).astype(f32)
    r = torch.zeros((600, 10), dtype=torch.int64, device=dev)
    d = torch.zeros((600, 10), dtype=torch.float32, device=dev)
    c = torch.zeros(600, dtype=torch.int32, device=dev)
    idx.search_device(torch.as_tensor(q, device=dev), 10, 4, r, d, c)
    got = (r.cpu().numpy().view(np.uint64), d.cpu().numpy(), c.cpu().numpy().astype(np.uint32))
    check(oracle, got, q, data, dec, cen, asg, 4, 10, L2, mn, sc, what="device nq=600")


def test_sq8_sharded_search_is_refused(L):
    import ctypes as C

    import torch

    from lynsedb_amd.sharded import NativeComm

    _, data = clustered(130, 1000, 16)
    idx = L.IvfFlatIndex.build(None, data, 16, 8, 5, "ip", quantizer="sq8")
    comm = NativeComm(None, 0, 1, 0)
    dev = torch.device("cuda", 0)
    dq = torch.as_tensor(data[:2], device=dev)
    r = torch.zeros((2, 5), dtype=torch.int64, device=dev)
    d = torch.zeros((2, 5), dtype=torch.float32, device=dev)
    c = torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(L._lib.LynseUnsupportedError):
        L._lib.check(L._lib.lib.lynse_hip_ivf_search_sharded_f32_device(idx._h, comm._c, C.c_void_p(dq.data_ptr()), 2, 5, 2,
                                                                          C.c_void_p(r.data_ptr()), C.c_void_p(d.data_ptr()),
                                                                          C.c_void_p(c.data_ptr())))


# ----------------------------------------------------------------------------------- stage timings ----
def test_sq8_stage_times_and_search_profile(L):
    _, data = clustered(140, 4000, 32)
    idx = L.IvfFlatIndex.build(None, data, 32, 16, 5, "ip", quantizer="sq8")
    idx.profile_enable(True)
    idx.sq8_stage_times(reset=True)
    idx.search_batch_arrays(data[:8], 10, 4)
    idx.search_batch_arrays(data[:1], 10, 4)
    t = idx.sq8_stage_times(reset=True)
    assert t["searches"] == 2 and t["pool_us"] > 0 and t["rerank_us"] > 0, t
    idx.profile_enable(False)
    idx.search_batch_arrays(data[:1], 10, 4)
    assert idx.sq8_stage_times(reset=True)["searches"] == 0   # (profiling off: nothing recorded)
    col = L.Collection("c", 32)
    col.add_items(data, list(range(4000)))
    col.commit()
    col.build_index("IVF-IP-SQ8", {"n_clusters": 16, "nprobe": 4})
    assert col.search_profile(data[3], 10)["profile"]["rerank_us"] > 0


# ------------------------------------------------------------------- Collection: rows committed after the build ----
@pytest.mark.parametrize("mode,metric", [("IVF-L2-SQ8", L2), ("IVF-COS-SQ8", COS)])
def test_collection_sq8_lazy_insert_of_committed_rows(L, mode, metric):
    """Rows committed after build_index reach the index through IVFIndex::insert (encoded with the fitted quantizer) on the next
    search: the results equal an SQ8 index built over the first rows with the later ones inserted."""
    rng, data = clustered(150, 3000, 16)
    later = (data[:300] + 0.5 * rng.standard_normal((300, 16))).astype(f32)
    col = L.Collection("c", 16)
    col.add_items(data, list(range(3000)))
    col.commit()
    col.build_index(mode, {"n_clusters": 12, "nprobe": 3})
    col.add_items(later, list(range(3000, 3300)))
    col.commit()
    q = (later[7] + 0.01).astype(f32)
    res = col.search(q, 10)
    ref = L.IvfFlatIndex.build(None, data, 16, 12, 20, NAME[metric], quantizer="sq8")
    ref.insert(later)
    g_rows, g_d, g_c = ref.search_batch_arrays(q[None, :], 10, 3)
    c = int(g_c[0])
    assert np.array_equal(np.asarray(res.ids(), np.int64), g_rows[0, :c].astype(np.int64))
    assert np.array_equal(np.asarray(res.distances(), f32).view(np.uint32), g_d[0, :c].view(np.uint32))
