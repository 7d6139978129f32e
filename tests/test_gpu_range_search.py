"""GPU parity tests for range search (Collection::search_range, src/engine.rs:6410-6483) through the C ABI and the Collection.  The
expected answer is built in numpy from the oracle: all_distances(..., IPFORM_SINGLE) on the f32 rows (on the round_f16-decoded rows
for an F16 shard), packed_distance for the binary metrics, then the pass test, a lexsort by (distance in metric order, row) and the
cut at max_results.  Row ids, counts, `passed` and f32 distance bits are compared with array_equal; there are no tolerances.  The wide-row
tests walk every branch of range_plan (a restatement of it next to them asserts which one a width takes) and add L1 and Canberra against the
additive restatement (tests/additive_ref/additive_ref.c)."""
import numpy as np
import pytest

import oracle as O
from additive_common import CANB, L1, build_ref
from conftest import oracle_for_every_query

pytestmark = pytest.mark.gpu
IP, L2, COS = O.IP, O.L2, O.COS
NAME = {IP: "ip", L2: "l2", COS: "cosine", O.HAMMING: "hamming", O.JACCARD: "jaccard", O.DICE: "dice", L1: "l1", CANB: "canberra"}
f32 = np.float32
NO_ROW = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    assert L_._lib.device_count() >= 1
    return L_


# ------------------------------------------------------------------------------------- expectation ----
def all_dists(oracle, queries, rows, metric):
    """D[q, r] = compute_distance_f32(query q, row r): the single-row kernels at every n"""
    return np.stack(oracle_for_every_query(lambda i: oracle.all_distances(queries[i], rows, metric, O.IPFORM_SINGLE), queries.shape[0]))


def expect_one(d, thr, cap, asc, live=None, order=None):
    """rows, distances and the passer count of one query from its distances to every row (order: canonical_order(d, asc), if at hand)"""
    with np.errstate(invalid="ignore"):
        ok = (d <= f32(thr)) if asc else (d >= f32(thr))   # a NaN on either side compares false
    if live is not None:
        ok = ok & live
    if order is None:
        order = canonical_order(d, asc)
    rows = order[ok[order]][:cap]
    return rows.astype(np.uint64), d[rows], int(ok.sum())


def canonical_order(d, asc):
    """every row by (distance in metric order, row); -0 == +0; where a NaN lands does not matter (it never passes)"""
    key = d + f32(0.0)
    return np.lexsort((np.arange(d.size), key if asc else -key))


class Case:
    """the oracle's distances of a batch against every row, with each query's canonical order computed once"""

    def __init__(self, queries, D, metric):
        self.queries, self.D, self.metric, self.asc = queries, D, metric, metric != IP
        self.order = [canonical_order(D[q], self.asc) for q in range(D.shape[0])]


def check(got, case, thr, cap, live=None):
    rows, dists, counts, passed = got
    D, asc = case.D, case.asc
    nq = D.shape[0]
    assert rows.shape == (nq, cap) and dists.shape == (nq, cap) and counts.shape == (nq,) and passed.shape == (nq,)
    worst = f32(np.inf) if asc else f32(-np.inf)
    for q in range(nq):
        e_rows, e_d, e_passed = expect_one(D[q], thr[q], cap, asc, live, case.order[q])
        c = int(counts[q])
        assert int(passed[q]) == e_passed, (q, thr[q])
        assert c == min(e_passed, cap), (q, thr[q])
        assert np.array_equal(rows[q, :c], e_rows), (q, thr[q])
        assert np.array_equal(dists[q, :c].view(np.uint32), e_d.view(np.uint32)), (q, thr[q])
        assert not np.isnan(dists[q, :c]).any()
        assert (rows[q, c:] == NO_ROW).all() and (dists[q, c:] == worst).all()


def thresholds_of(case):
    """the threshold sets of the sweep, one value per query each, from the oracle's distances (finite data)"""
    D, asc = case.D, case.asc
    nq, n = D.shape
    fail = f32(-np.inf) if asc else f32(np.inf)        # the side on which a threshold passes less
    s = np.stack([D[q][case.order[q]] for q in range(nq)])   # best first
    best, some = s[:, 0], s[:, min(2, n - 1)]
    out = {
        "below_best": np.nextafter(best, fail),         # 0 rows
        "equal": some.copy(),                           # that row is in ...
        "next_after": np.nextafter(some, fail),         # ... and one ulp towards the failing side it is out
        "median": s[:, n // 2].copy(),
        "inf_all": np.full(nq, -fail, f32),
        "1e6_all": np.full(nq, 1e6 if asc else -1e6, f32),
        "inf_none": np.full(nq, fail, f32),
        "1e6_none": np.full(nq, -1e6 if asc else 1e6, f32),
    }
    return {k: v.astype(f32) for k, v in out.items()}, some


def sweep(idx, case, caps, live=None, words=None):
    nq, n = case.D.shape
    thr, some = thresholds_of(case)
    for cap in caps:
        got = {k: idx.search_range_batch_arrays(case.queries, t, cap, NAME[case.metric], words) for k, t in thr.items()}
        for k, t in thr.items():
            check(got[k], case, t, cap, live)
        if live is None:
            assert (got["below_best"][2] == 0).all() and (got["below_best"][3] == 0).all()
            assert (got["inf_all"][3] == n).all() and (got["1e6_all"][3] == n).all()
            assert (got["inf_none"][3] == 0).all() and (got["1e6_none"][3] == 0).all()
            # the row whose distance IS the threshold: counted in, and out one ulp further (its equals leave with it)
            n_eq = (case.D == some[:, None]).sum(axis=1)
            assert np.array_equal(got["equal"][3].astype(np.int64) - got["next_after"][3].astype(np.int64), n_eq) and (n_eq >= 1).all()


def make_case(oracle, rng, n, dim, nq, metric, rows_of=lambda d: d):
    data = rng.standard_normal((n, dim)).astype(f32)
    queries = rng.standard_normal((nq, dim)).astype(f32)
    return data, Case(queries, all_dists(oracle, queries, rows_of(data), metric), metric)


# every dim, every n and every nq of the sweep, each metric with each of them; 4097 rows: IPFORM_AUTO would switch form at 4096,
# 257 queries cross the 256-query chunk, 768 columns fill the LDS tiles differently from the narrow rows
SHAPES = [  # (dim, n, nq)
    (1, 1, 1), (1, 65, 33), (7, 63, 3), (7, 4097, 257), (8, 65, 257), (8, 20000, 3), (16, 1, 33), (16, 4097, 1), (17, 63, 257),
    (17, 20000, 33), (100, 65, 1), (100, 4097, 257), (100, 20000, 3), (768, 63, 33), (768, 4097, 3), (768, 20000, 1),
]


@pytest.mark.parametrize("metric", [IP, L2, COS], ids=lambda m: NAME[m])
@pytest.mark.parametrize("dim,n,nq", SHAPES)
def test_shape_sweep(L, oracle, dim, n, nq, metric):
    rng = np.random.default_rng(1000 * dim + n + nq)
    data, case = make_case(oracle, rng, n, dim, nq, metric)
    idx = L.FlatIndex(None, dim, device=0)
    idx.write(data)
    sweep(idx, case, caps=[n + 5, 7] if n > 7 else [n + 5, 1])


@pytest.mark.parametrize("metric", [IP, L2, COS], ids=lambda m: NAME[m])
def test_cap_with_ties_at_the_cut(L, oracle, metric):
    rng = np.random.default_rng(5)
    base = rng.standard_normal((300, 16)).astype(f32)
    data = np.tile(base, (4, 1))                     # row r, r + 300, r + 600, r + 900 are equal
    queries = rng.standard_normal((3, 16)).astype(f32)
    case = Case(queries, all_dists(oracle, queries, data, metric), metric)
    D, n, asc = case.D, data.shape[0], case.asc
    idx = L.FlatIndex(None, 16, device=0)
    idx.write(data)
    thr = np.full(3, np.inf if asc else -np.inf, f32)
    for cap in (4 * 10 + 2, 4 * 123 + 1, 4 * 200 + 3):   # the cut falls inside a group of four equal distances
        got = idx.search_range_batch_arrays(queries, thr, cap, NAME[metric])
        check(got, case, thr, cap)
        assert (got[3] == n).all() and (got[2] == cap).all()
        for q in range(3):   # the group at the cut is really tied, and its lowest rows were kept
            last = got[1][q, cap - 1]
            tied = np.nonzero(D[q] == last)[0]
            assert tied.size >= 4
            kept = np.intersect1d(got[0][q].astype(np.int64), tied)
            assert 0 < kept.size < tied.size and np.array_equal(kept, tied[: kept.size])


def test_large_cap_beyond_the_device_sort(L, oracle):
    rng = np.random.default_rng(6)
    n, dim, cap = 40000, 8, 20000
    for metric in (IP, L2):
        data, case = make_case(oracle, rng, n, dim, 2, metric)
        asc = case.asc
        idx = L.FlatIndex(None, dim, device=0)
        idx.write(data)
        s = np.stack([case.D[q][case.order[q]] for q in range(2)])   # best first
        for thr in (np.full(2, np.inf if asc else -np.inf, f32), s[:, 17000].astype(f32), s[:, 25000].astype(f32)):
            got = idx.search_range_batch_arrays(case.queries, thr, cap, NAME[metric])
            check(got, case, thr, cap)
        assert (got[2] == cap).all() and (got[3] > cap).all()


def test_non_finite_rows_queries_and_thresholds(L, oracle):
    rng = np.random.default_rng(77)
    dim = 20
    data = rng.standard_normal((2500, dim)).astype(f32)
    data[3] = np.nan
    data[50, 7] = np.nan
    data[90, 0] = np.inf
    data[91, 19] = -np.inf
    data[92, 3], data[92, 4] = np.inf, -np.inf
    data[93] = np.inf
    data[94] = 3e38
    queries = rng.standard_normal((6, dim)).astype(f32)
    queries[1] = np.nan
    queries[2, 5] = np.nan
    queries[3, 0] = np.inf
    queries[4] = -np.inf
    queries[5] = 3e38
    idx = L.FlatIndex(None, dim, device=0)
    idx.write(data)
    for metric in (IP, L2, COS):
        case = Case(queries, all_dists(oracle, queries, data, metric), metric)
        D = case.D
        assert np.isnan(D).any() and (metric == COS or np.isinf(D).any())
        finite_mid = np.array([np.median(r[np.isfinite(r)]) if np.isfinite(r).any() else 0.0 for r in D], f32)
        for cap in (3000, 40):
            for thr in (np.full(6, np.nan, f32), np.full(6, np.inf, f32), np.full(6, -np.inf, f32), np.zeros(6, f32), finite_mid,
                        np.full(6, 3.4e38, f32), np.full(6, -3.4e38, f32)):
                got = idx.search_range_batch_arrays(queries, thr, cap, NAME[metric])
                check(got, case, thr, cap)
                if np.isnan(thr).all():
                    assert (got[2] == 0).all() and (got[3] == 0).all()   # a NaN threshold returns nothing


@pytest.mark.parametrize("dim,n", [(17, 4097), (100, 300), (768, 65)])
def test_f16_shard_scores_its_decoded_rows_with_the_f32_kernels(L, oracle, dim, n):
    rng = np.random.default_rng(dim)
    for metric in (IP, L2, COS):
        data, case = make_case(oracle, rng, n, dim, 5, metric, rows_of=oracle.round_f16)
        idx = L.FlatIndex(None, dim, device=0, dtype="f16")
        idx.write(data)
        sweep(idx, case, caps=[n, 9])


# ------------------------------------------------------------------------------------- wide rows ----
RANGE_MAX_Q, RANGE_MAX_ROWS, LDS_78K, LDS_MAX = 16, 128, 78 * 1024, 160 * 1024


def range_plan(D, qc):
    """range_plan of csrc/range_host.inc restated: (TQ, R, budget, LDS bytes) of k_range_scan for rows of D floats and chunks of qc
    queries, None where a query and a row do not fit"""
    st = (D + 7) // 8 * 8 + 8
    row_b, q_b = st * 4, D * 4
    size = lambda tq, r: (tq * D + 3) // 4 * 16 + r * row_b + tq * 8
    tq = max(1, min(RANGE_MAX_Q, qc, (24 * 1024) // q_b))
    budget = LDS_78K
    if size(tq, 8) > budget:
        budget = LDS_MAX
    if size(tq, 1) > budget:
        tq = 1
    if size(tq, 1) > budget:
        return None
    r = min(RANGE_MAX_ROWS, (budget - size(tq, 0)) // row_b)
    return tq, r, budget, size(tq, r)


# dim -> the (TQ, R, budget) its chunks of 5 queries and of 1 query are meant to hit: fewer than 8 queries at 8 rows under 78 KiB, the
# whole LDS at 3 / 2 / 1 queries, R down to 1, and the widest row that fits (163,816 of the 163,840 bytes)
WIDE_PLANS = {
    769: ((5, 20, LDS_78K), (1, 24, LDS_78K)),
    1536: ((4, 8, LDS_78K), (1, 11, LDS_78K)),
    2048: ((3, 16, LDS_MAX), (1, 8, LDS_78K)),
    2049: ((2, 17, LDS_MAX), (1, 8, LDS_78K)),
    3073: ((1, 12, LDS_MAX), (1, 12, LDS_MAX)),
    6145: ((1, 5, LDS_MAX), (1, 5, LDS_MAX)),
    20000: ((1, 1, LDS_MAX), (1, 1, LDS_MAX)),
    20472: ((1, 1, LDS_MAX), (1, 1, LDS_MAX)),
}
WIDE_ADDITIVE, WIDE_F16 = (2048, 6145, 20472), (1536, 3073, 20472)


@pytest.fixture(scope="module")
def additive_ref(tmp_path_factory):
    return build_ref(tmp_path_factory.mktemp("additive_ref"))


def wide_sweep(L, oracle, additive_ref, dim, dtype="f32"):
    """n = 70 rows (no multiple of 32, nor of any R but 5 and 1: the last tile is partial; at R = 5, dim 6145, 73 rows as well) against
    5 queries and against 1: the plan depends on the chunk's query count"""
    ns = [70]
    for nq, want in zip((5, 1), WIDE_PLANS[dim]):
        plan = range_plan(dim, nq)
        print(f"\ndim {dim}, {nq} queries: TQ {plan[0]}, R {plan[1]}, budget {plan[2]}, LDS bytes {plan[3]}")
        assert plan[:3] == want and plan[3] <= plan[2], (dim, nq, plan)
        if plan[1] > 1 and 70 % plan[1] == 0 and 73 not in ns:
            ns.append(73)
        assert any(n % plan[1] for n in ns) or plan[1] == 1
    assert 70 % 32 and range_plan(20472, 1)[3] == 163816 and range_plan(20473, 1) is None and range_plan(20473, 5) is None
    rng = np.random.default_rng(dim)
    for n in ns:
        data = rng.standard_normal((n, dim)).astype(f32)
        queries = rng.standard_normal((5, dim)).astype(f32)
        rows = oracle.round_f16(data) if dtype == "f16" else data
        idx = L.FlatIndex(None, dim, device=0, dtype=dtype)
        idx.write(data)
        cases = [Case(queries, all_dists(oracle, queries, rows, m), m) for m in (IP, L2, COS)]
        if dim in WIDE_ADDITIVE:
            cases += [Case(queries, additive_ref.raw_dists(m, queries, rows), m) for m in (L1, CANB)]
        for case in cases:
            assert np.isfinite(case.D).all()
            sweep(idx, case, caps=[n + 5, 7])
            sweep(idx, Case(case.queries[:1], case.D[:1], case.metric), caps=[n + 5, 7])


@pytest.mark.parametrize("dim", sorted(WIDE_PLANS))
def test_wide_rows_take_every_plan(L, oracle, additive_ref, dim):
    wide_sweep(L, oracle, additive_ref, dim)


@pytest.mark.parametrize("dim", WIDE_F16)
def test_wide_rows_take_every_plan_on_an_f16_shard(L, oracle, additive_ref, dim):
    wide_sweep(L, oracle, additive_ref, dim, dtype="f16")


def test_widest_row_and_the_refusal(L, oracle, additive_ref):
    """one float more than the widest row: refused on the host before any launch; the handle next to it still answers"""
    rng = np.random.default_rng(20473)
    too_wide = L.FlatIndex(None, 20473, device=0)
    too_wide.write(rng.standard_normal((3, 20473)).astype(f32))
    widest = L.FlatIndex(None, 20472, device=0)
    data = rng.standard_normal((70, 20472)).astype(f32)
    widest.write(data)
    queries = rng.standard_normal((2, 20472)).astype(f32)
    case = Case(queries, all_dists(oracle, queries, data, L2), L2)
    for nq in (2, 1):
        for name in ("ip", "l2", "cosine", "l1", "canberra"):
            with pytest.raises(L._lib.LynseUnsupportedError, match="do not fit in LDS"):
                too_wide.search_range_batch_arrays(np.ones((nq, 20473), f32), np.zeros(nq, f32), 5, name)
        sweep(widest, case, caps=[75, 7])


def packed_dists(oracle, qw, words, metric):
    return np.array([[oracle.packed_distance(qw[i], words[r], metric) for r in range(words.shape[0])] for i in range(qw.shape[0])], f32)


@pytest.mark.parametrize("packed_only", [True, False], ids=["packed_only", "f32_rows"])
def test_binary_metrics_at_130_bits(L, oracle, packed_only):
    rng = np.random.default_rng(130)
    dim, n, nq = 130, 700, 4                          # three words, the last with two live bits
    data = (rng.random((n, dim)) < 0.4).astype(f32)
    data[5] = 0.0                                      # an empty row: jaccard / dice against an empty query is 0 / 0
    queries = (rng.random((nq, dim)) < 0.4).astype(f32)
    queries[3] = 0.0
    if not packed_only:                               # values that are not 0 / 1: the bit is (x > 0.5)
        data = (data * rng.uniform(0.51, 3.0, data.shape) + (1 - data) * rng.uniform(-2.0, 0.5, data.shape)).astype(f32)
        queries[0] = np.where(queries[0] > 0.5, 0.75, 0.25)
    words, qw = oracle.pack_binary(data), oracle.pack_binary(queries)
    idx = L.FlatIndex(None, dim, device=0)
    if packed_only:
        idx.write_packed(words)
    else:
        idx.write(data)
    for metric in (O.HAMMING, O.JACCARD, O.DICE):
        sweep(idx, Case(queries, packed_dists(oracle, qw, words, metric), metric), caps=[n + 1, 13])
    if packed_only:
        with pytest.raises(L._lib.LynseUnsupportedError):
            idx.search_range_batch_arrays(queries, np.zeros(nq, f32), 5, "l2")


def test_row_mask(L, oracle):
    rng = np.random.default_rng(9)
    n, dim, nq = 1000, 24, 5
    data, case_l2 = make_case(oracle, rng, n, dim, nq, L2)
    queries = case_l2.queries
    idx = L.FlatIndex(None, dim, device=0)
    idx.write(data)
    nw = (n + 63) // 64
    every_other = np.zeros(n, bool)
    every_other[::2] = True
    masks = {
        "every_other": (L.BitSet.from_rows(np.nonzero(every_other)[0], n).words, every_other),
        "all_zero": (np.zeros(nw, np.uint64), np.zeros(n, bool)),
        "no_words": (np.zeros(0, np.uint64), np.zeros(n, bool)),
        "bits_beyond_len": (np.full(nw + 3, 0xFFFFFFFFFFFFFFFF, np.uint64), np.ones(n, bool)),
        "short": (np.full(5, 0xFFFFFFFFFFFFFFFF, np.uint64), np.arange(n) < 320),   # rows the words do not cover are out
    }
    for case in (case_l2, Case(queries, all_dists(oracle, queries, data, IP), IP)):
        for name, (words, live) in masks.items():
            sweep(idx, case, caps=[n, 11], live=live, words=words)
    # the binary scan applies the same mask
    bdata = (rng.random((n, 130)) < 0.5).astype(f32)
    bq = (rng.random((2, 130)) < 0.5).astype(f32)
    bidx = L.FlatIndex(None, 130, device=0)
    bidx.write(bdata)
    bcase = Case(bq, packed_dists(oracle, oracle.pack_binary(bq), oracle.pack_binary(bdata), O.HAMMING), O.HAMMING)
    sweep(bidx, bcase, caps=[n, 11], live=every_other, words=masks["every_other"][0])


def test_row_sharded_handle_is_refused(L):
    idx = L.FlatIndex(None, 8, device=0)
    idx.write(np.ones((10, 8), f32))
    idx.set_row_map(2, 1)
    with pytest.raises(L._lib.LynseUnsupportedError):
        idx.search_range_batch_arrays(np.ones((1, 8), f32), [0.0], 5, "ip")
    idx.set_row_map(1, 0)
    assert int(idx.search_range_batch_arrays(np.ones((1, 8), f32), [0.0], 5, "ip")[2][0]) == 5


# ------------------------------------------------------------------------------------- Collection ----
def expect_collection(oracle, q, data, ids, metric, thr, cap, dead=()):
    d = oracle.all_distances(q, data, metric, O.IPFORM_SINGLE)
    live = ~np.isin(ids, np.asarray(list(dead), np.int64))
    rows, dd, _ = expect_one(d, thr, cap, metric != IP, live)
    return [int(x) for x in ids[rows.astype(np.int64)]], dd


def same(got, exp):
    ids, dists = got
    assert isinstance(ids, list) and isinstance(dists, list)
    assert all(type(x) is int for x in ids) and all(type(x) is float for x in dists)
    assert ids == exp[0]
    assert np.array_equal(np.asarray(dists, f32).view(np.uint32), exp[1].view(np.uint32))


def test_collection_ids_tombstones_pending_and_subset(L, oracle):
    rng = np.random.default_rng(21)
    n, dim = 500, 12
    data = rng.standard_normal((n, dim)).astype(f32)
    ids = (rng.permutation(n) * 7 + 1000).astype(np.int64)        # a non-identity id map
    q = rng.standard_normal(dim).astype(f32)
    c = L.Collection("range", dim, device=0)
    c.add_items(data[:400], ids[:400].tolist())
    assert c.search_range(q, -1e6, 50) == ([], [])                # nothing flushed yet: pending rows are not searched
    c.commit()
    c.add_items(data[400:], ids[400:].tolist())
    d_ip = oracle.all_distances(q, data, IP, O.IPFORM_SINGLE)
    thr = float(np.sort(d_ip[:400])[200])
    same(c.search_range(q, thr), expect_collection(oracle, q, data[:400], ids[:400], IP, thr, 1000))   # rows 400.. still pending
    c.commit()
    same(c.search_range(q, thr), expect_collection(oracle, q, data, ids, IP, thr, 1000))
    same(c.search_range(q, thr, max_results=17), expect_collection(oracle, q, data, ids, IP, thr, 17))
    # tombstones leave before the cap: delete the ten best, the cap refills from the rows behind them
    best = c.search_range(q, thr, max_results=10)[0]
    c.delete_items(best)
    after = c.search_range(q, thr, max_results=10)
    same(after, expect_collection(oracle, q, data, ids, IP, thr, 10, dead=best))
    assert len(after[0]) == 10 and not set(after[0]) & set(best)
    # subset= intersects with the tombstones
    sub_rows = np.arange(0, n, 3)
    exp_sub = expect_one(d_ip, thr, 1000, False, np.isin(np.arange(n), sub_rows) & ~np.isin(ids, best))
    same(c.search_range(q, thr, subset=sub_rows), ([int(x) for x in ids[exp_sub[0].astype(np.int64)]], exp_sub[1]))
    same(c.search_range(q, thr, subset=L.BitSet.from_rows(sub_rows, n)), ([int(x) for x in ids[exp_sub[0].astype(np.int64)]], exp_sub[1]))
    c.restore_items(best)
    same(c.search_range(q, thr, max_results=10), expect_collection(oracle, q, data, ids, IP, thr, 10))
    with pytest.raises(RuntimeError, match="Dimension mismatch"):
        c.search_range(q[:-1], thr)
    assert c.search_range(q[:-1], thr, max_results=0) == ([], [])   # the early return comes first (engine.rs:6416-6426)


@pytest.mark.parametrize("mode,metric,params", [("FLAT-IP", IP, None), ("IVF-L2", L2, {"n_clusters": 8, "nprobe": 2}),
                                                ("FLAT-COS-PQ", COS, None), ("FLAT-L2-RABITQ", L2, None)])
def test_collection_ignores_the_built_index(L, oracle, mode, metric, params):
    rng = np.random.default_rng(33)
    n, dim = 600, 16
    data = rng.standard_normal((n, dim)).astype(f32)
    ids = np.arange(n, dtype=np.int64)[::-1].copy()
    q = rng.standard_normal(dim).astype(f32)
    c = L.Collection("range_modes", dim, device=0)
    c.add_items(data, ids.tolist())
    c.build_index(mode, params)
    d = oracle.all_distances(q, data, metric, O.IPFORM_SINGLE)
    for thr in (float(np.median(d)), float(d[17])):
        for cap in (1000, 25):
            same(c.search_range(q, thr, cap), expect_collection(oracle, q, data, ids, metric, thr, cap))


def test_reference_standard_cases(L):
    """tests/standard_tests/test_search.py:594-621, :736-743 of the reference on its fixture's recipe (DIM 8, N 20, seeds 42 and 0)"""
    DIM, N = 8, 20
    np.random.seed(42)
    vectors = [np.random.rand(DIM).astype(f32) for _ in range(N)]
    np.random.seed(0)
    query_vec = np.random.rand(DIM).astype(f32)
    c = L.Collection("populated", DIM, device=0)
    c.add_items(np.stack(vectors), list(range(N)))
    c.commit()
    ids, dists = c.search_range(query_vec, threshold=10.0)
    assert ids == [] and dists == []                                   # ip scores of vectors in [0, 1)^8 stay below 8
    ids, _ = c.search_range(query_vec, threshold=-1e6)
    assert sorted(ids) == list(range(N))                               # every row
    assert c.search_range(query_vec, threshold=1e6) == ([], [])
    assert len(c.search_range(query_vec, threshold=1e6, max_results=3)[0]) <= 3
    assert len(c.search_range(query_vec, threshold=-1e6, max_results=3)[0]) == 3
    assert c.search_range(query_vec, threshold=-1e6, max_results=0) == ([], [])
    del_id = ids[0]
    c.delete_items([del_id])
    after = c.search_range(query_vec, threshold=-1e6)[0]
    assert del_id not in after and len(after) == N - 1
    c.delete_items([3, 4])
    after = c.search_range(query_vec, threshold=-1e6)[0]
    assert 3 not in after and 4 not in after
