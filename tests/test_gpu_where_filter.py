"""Field filters on the device (`where=`): the BitSet words and the count of k_field_filter against the per-row model of
tests/fields_common.py, searches with `where=` against the same searches with `subset=` set to the model's rows, the device-words entry
of the filtered scan against the host-words entry, and the alignment of the field columns with the rows through every row path."""
import os

import numpy as np
import pytest

import fields_common as F

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 127, 129, 4_113, 300_017]     # tail words and the zero padding beyond n; the last is more than one grid pass


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L

    return L


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def words_of(mask):
    """BitSet words of a bool array: bit r of word r // 64, LSB first, zero beyond the end"""
    pad = np.zeros((mask.size + 63) // 64 * 64, np.uint8)
    pad[:mask.size] = mask
    return np.packbits(pad, bitorder="little").view(np.uint64) if pad.size else np.zeros(0, np.uint64)


# ---- the kernel's words against the model -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filter_case(L):
    """300,017 rows drawn from the pool (the first rows are the whole pool, shuffled), the model's answer per pool row and expression,
    and every expression compiled once against the table's dictionaries."""
    from lynsedb_amd import fields as W

    rng = np.random.default_rng(2525)
    P = len(F.POOL)
    pick = np.concatenate([rng.permutation(P), rng.integers(0, P, SIZES[-1] - P)])
    pool = W.FieldTable()
    pool.append([r or {} for r in F.POOL], P)
    table = pool.take(pick)
    cases = []
    for name, expr, cond in F.expressions():
        pred = W.parse_where(expr)
        by_pool = np.array([F.model_match(cond, r) for r in F.POOL], dtype=bool)   # the decision is the model's, row by row
        cases.append((name, pred, by_pool, table.device_program(pred)))
    return W.FieldFilter(), table, pick, cases


@pytest.mark.parametrize("n", SIZES)
def test_filter_words_and_count_match_the_model(filter_case, n):
    ff, table, pick, cases = filter_case
    ff.upload(table, list(table.cols), n)
    for name, pred, by_pool, (leaves, aux) in cases:
        want = by_pool[pick[:n]]
        count = ff.run(n, pred.any, leaves, aux)
        got = ff.words()
        assert got.size == (n + 63) // 64, (name, n)
        assert count == int(np.count_nonzero(want)), (name, n, count)
        assert np.array_equal(got, words_of(want)), (name, n, np.nonzero(got != words_of(want))[0][:4])
    ptr, nw = ff.words_device()
    assert nw == (n + 63) // 64 and bool(ptr.value) == (n > 0)


def test_filter_refuses_what_it_cannot_bound(L, filter_case):
    """the checks the kernel relies on: a column of another length, key lists and tables outside aux, unsorted keys, unknown kinds"""
    from lynsedb_amd import fields as W
    from lynsedb_amd._lib import FieldLeaf

    ff = W.FieldFilter()
    ff.set_column(0, np.full(100, W.TAG_INT, np.uint8), np.arange(100, dtype=np.uint64))
    one = lambda *a: (FieldLeaf * 1)(FieldLeaf(*a))   # noqa: E731
    assert ff.run(100, False, one(W.LEAF_EQ, 0, 0, 0, W.TAG_INT, 0, 7, 0, 0), np.zeros(0, np.uint64)) == 1
    assert ff.run(100, False, one(W.LEAF_EQ, 5, 0, 0, W.TAG_INT, 0, 7, 0, 0), np.zeros(0, np.uint64)) == 0       # a column never set: nobody carries it
    good = np.array([0, 0, 0, 0, 3, 3, 3, 3, 3, 5, 6, 7], np.uint64)                                              # three Int keys
    assert ff.run(100, False, one(W.LEAF_KEYSET, 0, 0, 0, 0, 0, 0, 0, 3), good) == 3
    for leaf, aux, n in ((one(W.LEAF_EQ, 0, 0, 0, W.TAG_INT, 0, 7, 0, 0), np.zeros(0, np.uint64), 99),             # the column holds 100 rows
                         (one(W.LEAF_KEYSET, 0, 0, 0, 0, 0, 0, 1, 3), good, 100),                                 # the list runs past aux
                         (one(W.LEAF_KEYSET, 0, 0, 0, 0, 0, 0, 0, 4), good, 100),                                 # starts do not end at aux_len
                         (one(W.LEAF_KEYSET, 0, 0, 0, 0, 0, 0, 0, 3), np.array([0, 0, 0, 0, 3, 3, 3, 3, 3, 6, 5, 7], np.uint64), 100),   # unsorted
                         (one(W.LEAF_STRTABLE, 0, 0, 0, 0, 0, 0, 0, 65), np.zeros(1, np.uint64), 100),            # a table of 65 codes needs 2 words
                         (one(9, 0, 0, 0, 0, 0, 0, 0, 0), np.zeros(0, np.uint64), 100),
                         (one(W.LEAF_NUM_RANGE, 0, 4, 0, 0, 0, 0, 0, 0), np.zeros(0, np.uint64), 100)):
        with pytest.raises(Exception):
            ff.run(n, False, leaf, aux)
    with pytest.raises(Exception):   # an array row whose payload does not index arr_ptr
        ff.set_column(1, np.full(4, W.TAG_ARRAY, np.uint8), np.arange(4, dtype=np.uint64), np.array([0, 1, 2], np.uint64), np.full(2, W.TAG_INT, np.uint8), np.zeros(2, np.uint64))
    with pytest.raises(Exception):
        ff.set_column(1, np.full(4, 8, np.uint8), np.zeros(4, np.uint64))


# ---- searches: where= against subset= of the model's rows ---------------------------------------------------------------------
N_FLUSHED, N_PENDING, DIM = 2_500, 37, 24


def search_rows(i):
    """the fields of row i of the search collections: g = i % 100 drives the selectivity, the rest exercises the other leaf kinds"""
    return {"g": i % 100, "lang": ("en", "de", "fr")[i % 3], "body": "alpha beta" if i % 4 else "alpha gamma delta", "tags": ["x", i % 5], "w": i / 8.0}


WHERE_CASES = [                                            # (name, where string, model structure)
    ("empty",) + F.rng("g", "<", "0"),
    ("1 %",) + F.rng("g", "<", "1"),
    ("60 %",) + F.rng("g", "<", "60"),
    ("full",) + F.rng("g", ">=", "0"),
    ("and",) + F.all_of(F.rng("g", ">=", "10"), F.eq("lang", "'en'"), F.contains("tags", "3")),
    ("in",) + F.in_("g", ["3", "5", "98", "400"]),
    ("or",) + F.any_of(F.eq("g", "7"), F.eq("lang", "'fr'")),
]


def make_collection(L, mode, seed):
    rng = np.random.default_rng(seed)
    n = N_FLUSHED + N_PENDING
    data = (rng.random((n, DIM)) < 0.5).astype(np.float32) if "HAMMING" in mode else rng.standard_normal((n, DIM)).astype(np.float32)
    rows = [search_rows(i) for i in range(n)]
    c = L.Collection("w", DIM)
    c.add_items(data[:N_FLUSHED], list(range(1000, 1000 + N_FLUSHED)), fields=rows[:N_FLUSHED])
    c.build_index(mode, {"n_clusters": 16} if mode.startswith("IVF") else None)
    c.add_items(data[N_FLUSHED:], list(range(1000 + N_FLUSHED, 1000 + n)), fields=rows[N_FLUSHED:])     # these stay pending
    assert c.pending_len() == N_PENDING
    q = (rng.random((5, DIM)) < 0.5).astype(np.float32) if "HAMMING" in mode else rng.standard_normal((5, DIM)).astype(np.float32)
    return c, rows, q


def model_rows(rows, cond):
    return np.array([i for i, r in enumerate(rows) if F.model_match(cond, r)], dtype=np.uint64)


def assert_same_results(got, want, what):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert len(a) == len(b), what
        assert np.array_equal(a.ids(), b.ids()), (what, a.ids(), b.ids())
        assert np.array_equal(bits(a.distances()), bits(b.distances())), what


def with_strategy(strategy, call):
    """the call under LYNSE_HIP_FILTER_STRATEGY (read per call): "direct" = gathered rows, "masked" = the masked scan, None = the cost model"""
    old = os.environ.pop("LYNSE_HIP_FILTER_STRATEGY", None)
    if strategy is not None:
        os.environ["LYNSE_HIP_FILTER_STRATEGY"] = "1" if strategy == "direct" else "2"
    try:
        return call()
    finally:
        os.environ.pop("LYNSE_HIP_FILTER_STRATEGY", None)
        if old is not None:
            os.environ["LYNSE_HIP_FILTER_STRATEGY"] = old


@pytest.mark.parametrize("mode", ["FLAT-IP", "FLAT-L2", "FLAT-COS", "FLAT-HAMMING", "FLAT-L1"])
def test_search_where_equals_search_subset(L, mode):
    """ids, distance bits and counts, at 1 % and 60 % (either side of the gathered / masked switch: at this size the cost model always masks,
    so both strategies are also forced, as the other filter tests do), with an empty and a full match; pending rows included.  And the
    device-words entry of the exact filtered scan against the host-words entry called directly."""
    c, rows, q = make_collection(L, mode, 7)
    metric = c._metric
    for name, expr, cond in WHERE_CASES:
        sub = model_rows(rows, cond)
        assert c.query_fields(expr) == [1000 + int(r) for r in sub], (mode, name)
        for strategy in (None, "direct", "masked"):
            for k in (1, 10):
                got = with_strategy(strategy, lambda: c.batch_search(q, k, where=expr))
                want = with_strategy(strategy, lambda: c.batch_search(q, k, subset=sub))
                assert_same_results(got, want, (mode, name, strategy, k))
                assert all(len(r) == min(k, sub.size) for r in got), (mode, name, strategy, k)
            one = with_strategy(strategy, lambda: c.search(q[0], 10, where=expr))
            assert np.array_equal(one.ids(), got[0].ids())
            # the two C entries on the very same words
            rw = c._resolve_where(expr)
            if rw.count:
                d_words, n_words = c._field_filter.words_device()
                dev = with_strategy(strategy, lambda: c._flat.search_filtered_bitset_device_batch_arrays(q, 10, metric, d_words, n_words, rw.count))
                host = with_strategy(strategy, lambda: c._flat.search_filtered_bitset_batch_arrays(q, 10, metric, c._field_filter.words()))
                assert np.array_equal(dev[2], host[2]), (mode, name, strategy)
                for i, cnt in enumerate(dev[2].tolist()):
                    assert np.array_equal(dev[0][i, :cnt], host[0][i, :cnt]) and np.array_equal(bits(dev[1][i, :cnt]), bits(host[1][i, :cnt])), (mode, name, strategy, i)


def test_device_words_entry_on_each_side_of_the_strategy_switch(L):
    """The cost model's own choice: 200,000 x 1,024 rows written on the device and 4 queries — a 0.1 % filter is cheaper gathered (fewer
    rows scanned than the shard holds), a 50 % filter masked.  The count the filter reads back feeds the choice as the count of host words
    does: the two entries scan the same rows and return the same bits."""
    import torch

    from lynsedb_amd import fields as W

    n, dim = 200_000, 1_024
    gen = torch.Generator(device="cuda").manual_seed(3)
    idx = L.FlatIndex(None, dim)
    idx.write_device(torch.rand((n, dim), generator=gen, device="cuda", dtype=torch.float32))
    q = torch.rand((4, dim), generator=gen, device="cuda", dtype=torch.float32).cpu().numpy()
    ff = W.FieldFilter()
    ff.set_column(0, np.full(n, W.TAG_INT, np.uint8), (np.arange(n) % 1000).astype(np.uint64))
    from lynsedb_amd._lib import FieldLeaf

    idx.profile_enable(True)
    for lit, gathered in ((1, True), (500, False)):
        leaf = (FieldLeaf * 1)(FieldLeaf(W.LEAF_NUM_RANGE, 0, W.OP_LT, 0, 0, 0, W.normalize_f64_bits(float(lit)), 0, 0))
        count = ff.run(n, False, leaf, np.zeros(0, np.uint64))
        assert count == n // 1000 * lit
        d_words, n_words = ff.words_device()
        for metric in ("ip", "l2"):
            idx.profile_get(reset=True)
            dev = idx.search_filtered_bitset_device_batch_arrays(q, 10, metric, d_words, n_words, count)
            p_dev = idx.profile_get(reset=True)
            host = idx.search_filtered_bitset_batch_arrays(q, 10, metric, ff.words())
            p_host = idx.profile_get(reset=True)
            assert (0 < p_dev["scan_rows"] < n) == gathered and p_dev["scan_rows"] == p_host["scan_rows"], (lit, metric, p_dev, p_host)
            assert np.array_equal(dev[0], host[0]) and np.array_equal(bits(dev[1]), bits(host[1])) and np.array_equal(dev[2], host[2]), (lit, metric)
            assert (dev[0] % 1000 < lit).all() and (dev[2] == 10).all()
    idx.profile_enable(False)


@pytest.mark.parametrize("mode", ["IVF-IP", "HNSW-L2"])
def test_index_modes_take_the_filter(L, mode):
    """an IVF index gets the words read back as the subset it accepts; under a graph index a filtered search is the exact filtered scan"""
    c, rows, q = make_collection(L, mode, 11)
    for name, expr, cond in WHERE_CASES:
        sub = model_rows(rows, cond)
        assert_same_results(c.batch_search(q, 10, where=expr), c.batch_search(q, 10, subset=sub), (mode, name))
        assert_same_results(c.batch_search(q, 10, nprobe=4, where=expr), c.batch_search(q, 10, nprobe=4, subset=sub), (mode, name, "nprobe"))


def test_range_sparse_text_and_hybrid_take_the_filter(L):
    c, rows, q = make_collection(L, "FLAT-L2", 13)
    n = len(rows)
    ids = list(range(1000, 1000 + n))
    c.add_sparse_vectors([{i % 50: 1.0 + (i % 7), (i * 7) % 50: 0.5} for i in range(n)], ids)
    for name, expr, cond in WHERE_CASES:
        sub = model_rows(rows, cond)
        assert c.search_range(q[0], 40.0, 500, subset=c.where_subset(expr)) == c.search_range(q[0], 40.0, 500, subset=sub), name   # (its signature is pinned)
        assert np.array_equal(c.where_subset(expr).to_vec(), sub), name
        a, b = c.search_sparse({3: 1.0, 11: 2.0}, 20, where=expr), c.search_sparse({3: 1.0, 11: 2.0}, 20, subset=sub)
        assert np.array_equal(a.ids(), b.ids()) and np.array_equal(bits(a.distances()), bits(b.distances())), name
        assert_same_results(c.batch_search_sparse([{3: 1.0}, {4: 1.0, 5: 1.0}], 7, where=expr), c.batch_search_sparse([{3: 1.0}, {4: 1.0, 5: 1.0}], 7, subset=sub), name)
        a, b = c.text_search("gamma alpha", None, 15, where=expr), c.text_search("gamma alpha", None, 15, subset=sub)
        assert np.array_equal(a.ids(), b.ids()) and np.array_equal(bits(a.distances()), bits(b.distances())), name
        assert_same_results(c.batch_text_search(["delta", "beta en"], ["body"], 9, where=expr), c.batch_text_search(["delta", "beta en"], ["body"], 9, subset=sub), name)
        a, b = c.hybrid_search(q[0], "gamma", 10, where=expr), c.hybrid_search(q[0], "gamma", 10, subset=sub)
        assert np.array_equal(a.ids(), b.ids()) and np.array_equal(bits(a.distances()), bits(b.distances())), name
    # the text index reads the same `fields` dicts as before: an unfiltered text search is what it was
    assert len(c.text_search("alpha", None, 5)) == 5


def test_where_surface_errors(L):
    c, rows, q = make_collection(L, "FLAT-IP", 17)
    sub = np.arange(10, dtype=np.uint64)
    for call in (lambda: c.search(q[0], 5, where="g < 5", subset=sub), lambda: c.batch_search(q, 5, where="g < 5", subset=sub),
                 lambda: c.search_profile(q[0], 5, where="g < 5", subset=sub),
                 lambda: c.search_sparse({1: 1.0}, 5, where="g < 5", subset=sub), lambda: c.text_search("alpha", None, 5, where="g < 5", subset=sub),
                 lambda: c.hybrid_search(q[0], "alpha", 5, where="g < 5", subset=sub)):
        with pytest.raises(ValueError, match="not both"):
            call()
    for expr in ("g != 5", "g LIKE '5%'", "(g = 5)", "g IN (1) AND lang = 'en'"):
        with pytest.raises(NotImplementedError, match="ApexBase SQL"):
            c.search(q[0], 5, where=expr)
        with pytest.raises(NotImplementedError, match="ApexBase SQL"):
            c.query_fields(expr)
    with pytest.raises(NotImplementedError):      # where_expr= keeps the answer it has
        c.search(q[0], 5, where_expr="g < 5")


def test_search_profile_reports_the_filter(L):
    c, rows, q = make_collection(L, "FLAT-IP", 19)
    expr, cond = F.all_of(F.rng("g", "<", "30"), F.eq("lang", "'de'"))
    sub = model_rows(rows, cond)
    out = c.search_profile(q[0], 10, where=expr)
    p = out["profile"]
    assert p["filter_expression"] == expr and p["filter_matches"] == sub.size == p["scanned_vectors"]
    assert p["index_path"] == "flat_mmap_filtered" and p["filter_us"] > 0 and p["result_count"] == 10
    assert out["items"]["ids"] == [int(i) for i in c.search(q[0], 10, subset=sub).ids()]
    assert c.search_profile(q[0], 10)["profile"]["filter_expression"] is None


# ---- alignment: the columns follow the rows through every row path ------------------------------------------------------------
def test_columns_stay_aligned_through_every_row_path(L):
    rng = np.random.default_rng(23)
    dim = 8
    c = L.Collection("a", dim)
    state = {}          # id -> fields dict or None (a row added without fields), for the ids that have a row
    dead = set()
    exprs = [F.rng("g", "<", "40"), F.eq("lang", "'en'"), F.contains("tags", "'x'"), F.all_of(F.rng("g", ">=", "10"), F.eq("lang", "'de'")),
             F.in_("g", ["1", "2", "3", "77"]), F.any_of(F.eq("g", "5"), F.eq("lang", "'fr'")), F.eq("extra", "true"), F.rng("w", ">", "'a'")]

    def vec(m):
        return rng.standard_normal((m, dim)).astype(np.float32)

    def check(what):
        for expr, cond in exprs:
            want = sorted(i for i, f in state.items() if i not in dead and F.model_match(cond, f))
            assert c.query_fields(expr) == want, (what, expr)

    ids = list(range(300))
    c.add_items(vec(300), ids, fields=[search_rows(i) for i in ids])
    state.update({i: search_rows(i) for i in ids})
    check("pending only")                                       # nothing flushed yet: the host evaluator alone
    c.add_items(vec(50), list(range(300, 350)))                 # without fields: every field missing
    state.update({i: None for i in range(300, 350)})
    check("add without fields")
    c.commit()
    assert c.pending_len() == 0
    check("flush")
    c.add_items(vec(20), list(range(350, 370)), fields=[{"g": 1, "extra": True, "w": "text"} for _ in range(20)])
    state.update({i: {"g": 1, "extra": True, "w": "text"} for i in range(350, 370)})
    check("flushed and pending")
    c.upsert_items(vec(3), [5, 6, 1000], fields=[{"g": 77, "lang": "en"}, {}, {"g": 2, "tags": ["x", "x"]}])     # two rows rewritten, one new
    state.update({5: {"g": 77, "lang": "en"}, 6: {}, 1000: {"g": 2, "tags": ["x", "x"]}})
    check("upsert with fields")
    c.upsert_items(vec(2), [7, 1001])                           # without fields: the old row keeps its fields, the new one has none
    state[1001] = None
    check("upsert without fields")
    c.update_items(vec(1), [8], fields=[{"lang": "fr", "extra": True}])
    state[8] = {"lang": "fr", "extra": True}
    check("update")
    c.delete_items([0, 5, 320, 355, 1000])
    dead.update([0, 5, 320, 355, 1000])
    check("tombstones")
    assert c.compact() == 5
    for i in dead:
        del state[i]
    dead.clear()
    check("compact")
    c.add_items(vec(4), [2000, 2001, 2002, 2003], fields=[{"g": 3}, {"lang": "en"}, {}, {"tags": ["x"]}])
    state.update({2000: {"g": 3}, 2001: {"lang": "en"}, 2002: {}, 2003: {"tags": ["x"]}})
    check("pending after compact")
    got = c.search(vec(1)[0], 400, where="g < 40")
    assert sorted(int(i) for i in got.ids()) == c.query_fields("g < 40")
