"""Multi-vector (MaxSim) search on the GPU against a dozen lines of numpy: an f64 product, the max over a record's tokens, then the f32
sum of rule 4 (include/lynse_hip.h, MULTI-VECTOR SEARCH).  Integer-valued inputs make every partial sum exact, so there the answer
must match bit for bit, ties by record row included."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    return L_


def ref_scores(q, sets, products=False):
    """-> (scores f32 as reported: NaN as -inf, -0 as +0; which records have tokens[; sum_i max_j sum_k |q_ik p_jk|, sum_i |m_i|])"""
    lens = np.array([len(p) for p in sets])
    has, scores = lens > 0, np.full(len(sets), -np.inf, f32)
    if not has.any():
        return (scores, has, None, None) if products else (scores, has)
    P = np.concatenate([np.asarray(p, f32).reshape(len(p), -1) for p, h in zip(sets, has) if h]).astype(np.float64)
    starts = np.concatenate([[0], np.cumsum(lens[has])[:-1]])
    with np.errstate(invalid="ignore", over="ignore"):
        s = (np.asarray(q, np.float64) @ P.T).astype(f32)                        # rule 2
        m = np.maximum.reduceat(np.where(np.isnan(s), -np.inf, s), starts, axis=1)   # rule 3
        acc = m[0].copy()
        for i in range(1, len(m)):                                              # rule 4: ((m_0 + m_1) + m_2) + ...
            acc = (acc + m[i]).astype(f32)
    scores[has] = np.where(np.isnan(acc), -np.inf, acc) + f32(0.0)
    if not products:
        return scores, has
    mag = np.maximum.reduceat(np.abs(np.asarray(q, np.float64)) @ np.abs(P).T, starts, axis=1).sum(axis=0)
    return scores, has, mag, np.abs(m.astype(np.float64)).sum(axis=0)


def expect(scores, has, k, keep=None):
    rows = np.nonzero(has if keep is None else has & keep)[0]
    o = rows[np.lexsort((rows, -scores[rows].astype(np.float64)))][:k]
    return o, scores[o]


def coll_of(L, sets, fields=None):
    """record row r has user id 3 r + 7 and the token set sets[r]"""
    n = len(sets)
    c = L.Collection("mv", 4, device=0)
    c.add_items(np.ones((n, 4), f32), [3 * r + 7 for r in range(n)], fields=fields)
    c.commit()
    c.add_multi_vectors([3 * r + 7 for r in range(n)], sets)
    return c


def same(res, rows, scores):
    assert res.index_mode() == "MULTIVEC-MAXSIM-IP"
    assert [int(x) for x in res.ids()] == [3 * int(r) + 7 for r in rows]
    assert np.array_equal(res.distances().view(u32), np.asarray(scores, f32).view(u32)), (res.distances(), scores)


def int_sets(rng, lens, dim):
    return [rng.integers(-3, 4, (int(t), dim)).astype(f32) for t in lens]


# boundary corpora: a record boundary exactly on a 32-token block boundary (32 | 32), one token before it (31 | 33) and after (33 | 31)
CORPORA = {
    "one": [33], "two": [0, 100], "on_block": [32, 32, 1, 31, 32], "before": [31, 33, 0, 32], "after": [33, 31, 100, 1],
    "mixed300": None,   # 300 records drawn from {0, 1, 31, 32, 33, 100}
    "ranges": None,     # > 3 wave ranges of ~2,048 tokens, one record of 2,500 tokens (longer than a range) in the middle
}


def corpus(name, rng):
    if name == "mixed300":
        return rng.choice([0, 1, 31, 32, 33, 100], 300)
    if name == "ranges":
        return np.concatenate([rng.choice([0, 1, 31, 32, 33, 100], 120), [2500], rng.choice([1, 31, 32, 33, 100], 60)])
    return CORPORA[name]


@pytest.mark.parametrize("name,dim", [("one", 1), ("two", 2), ("on_block", 7), ("before", 128), ("after", 130), ("mixed300", 7), ("mixed300", 128),
                                      ("ranges", 2), ("ranges", 130)])
def test_exact_on_integer_data(L, name, dim):
    rng = np.random.default_rng(len(name) * 1000 + dim)
    sets = int_sets(rng, corpus(name, rng), dim)
    c = coll_of(L, sets)
    if name == "ranges":
        assert c.search_profile(None, 1, query_tokens=np.ones((1, dim), f32))["profile"]["device"]["multivec"]["ranges"] >= 4
    for tq in (1, 31, 32, 33, 64, 65):
        q = rng.integers(-3, 4, (tq, dim)).astype(f32)
        scores, has = ref_scores(q, sets)
        for k in (1, 10, len(sets) + 5):
            same(c.search_multi_vector(q, k), *expect(scores, has, k))


def test_planted_record_comes_first(L):
    """A planted best match at every token of a record — so at every column lane of a block — for each record position: row 0 (32
    tokens: columns 0 .. 31 of the first block), the last row, the last and the first record of a wave range, and a record of 70
    tokens that spans blocks (every column of the carry and of the end-of-record write).  One store per planted token."""
    rng = np.random.default_rng(5)
    lens = np.concatenate([[32], rng.choice([31, 32, 33, 100], 80), [40, 70], rng.choice([1, 31, 33], 40), [33]])
    base = [rng.integers(-1, 2, (int(t), 16)).astype(f32) for t in lens]
    first_of_range = int(np.searchsorted(np.cumsum(lens), 2048, side="right"))   # the ranges close at 2,048 tokens: this record opens the second
    q = rng.integers(-1, 2, (33, 16)).astype(f32)
    q[:, 3] = 0
    q[0] = 0
    q[0, 3] = 1   # only query token 0 reads column 3
    scores0, has = ref_scores(q, base)
    for r in (0, len(lens) - 1, first_of_range - 1, first_of_range, 82):   # (82: the 70 tokens)
        for j in range(int(lens[r])):
            sets = list(base)
            sets[r] = base[r].copy()
            sets[r][j, 3] = 1000.0   # query token 0 gains ~1000 on this record alone
            scores = scores0.copy()
            scores[r] = ref_scores(q, [sets[r]])[0][0]
            rows, sc = expect(scores, has, 3)
            assert rows[0] == r and sc[0] > 900
            idx = L.MultiVectorIndex(16, device=0)
            idx.append(sets)
            got_rows, got_sc, cnt = idx.search_batch_arrays([q], 3)
            assert cnt[0] == 3 and np.array_equal(got_rows[0], rows) and np.array_equal(got_sc[0].view(u32), sc.view(u32)), (r, j)


def test_real_valued_data_within_the_summation_bound(L):
    rng = np.random.default_rng(11)
    dim, tq, k, u = 128, 32, 10, 2.0 ** -24
    sets = [rng.standard_normal((int(t), dim)).astype(f32) for t in rng.choice([1, 31, 32, 33, 100], 300)]
    c = coll_of(L, sets)
    gamma = lambda n: n * u / (1 - n * u)   # noqa: E731
    qualified, queries = 0, [rng.standard_normal((tq, dim)).astype(f32) for _ in range(20)]
    for q, res in zip(queries, c.batch_search_multi_vector(queries, k)):
        scores, has, mag, msum = ref_scores(q, sets, products=True)
        exact = np.full(len(sets), -np.inf)
        exact[has] = np.maximum.reduceat(q.astype(np.float64) @ np.concatenate(sets).astype(np.float64).T,
                                         np.concatenate([[0], np.cumsum([len(p) for p in sets])[:-1]]), axis=1).sum(axis=0)
        B = np.full(len(sets), np.inf)
        B[has] = gamma(dim) * mag + gamma(tq) * msum
        got_rows = (res.ids() - 7) // 3
        assert len(res) == k and np.all(np.abs(res.distances().astype(np.float64) - exact[got_rows]) <= B[got_rows])
        order = np.argsort(-exact, kind="stable")
        if exact[order[k - 1]] - exact[order[k]] > 2 * B.max():
            qualified += 1
            assert sorted(got_rows) == sorted(order[:k])
    assert qualified >= 0.9 * len(queries)   # (a property of the reference and the seed alone)


def test_masks_equal_the_reference_over_the_survivors(L):
    rng = np.random.default_rng(3)
    lens = np.concatenate([rng.choice([0, 1, 31, 32, 33, 100], 200), [2500], rng.choice([1, 33], 30)])
    sets, n = int_sets(rng, lens, 7), len(lens)
    c = coll_of(L, sets, fields=[{"g": int(r % 5)} for r in range(n)])
    q = rng.integers(-3, 4, (33, 7)).astype(f32)
    scores, has = ref_scores(q, sets)
    rows = np.arange(n)
    second_range = (np.cumsum(lens) > 2048) & (np.cumsum(lens) <= 4096)   # every record of one wave range, and more
    sub = rows[rng.random(n) < 0.5]
    same(c.search_multi_vector(q, 20, subset=sub), *expect(scores, has, 20, np.isin(rows, sub)))
    same(c.search_multi_vector(q, n, subset=L.BitSet.from_rows(rows[~second_range], n)), *expect(scores, has, n, ~second_range))
    same(c.search_multi_vector(q, 20, where="g >= 2"), *expect(scores, has, 20, rows % 5 >= 2))
    dead = expect(scores, has, 6)[0]
    c.delete_items([3 * int(r) + 7 for r in dead])
    same(c.search_multi_vector(q, 20), *expect(scores, has, 20, ~np.isin(rows, dead)))
    same(c.search_multi_vector(q, 20, subset=sub), *expect(scores, has, 20, np.isin(rows, sub) & ~np.isin(rows, dead)))
    same(c.search_multi_vector(q, 20, where="g >= 2"), *expect(scores, has, 20, (rows % 5 >= 2) & ~np.isin(rows, dead)))
    assert len(c.search_multi_vector(q, 5, subset=np.zeros(0, np.uint64))) == 0
    assert len(c.search_multi_vector(q, 5, subset=rows[~has])) == 0   # only records without tokens survive
    # compaction of token sets is out of scope, but the ids it removes from the collection must stay gone, filter or no filter
    assert c.compact() == len(dead)
    gone = [3 * int(r) + 7 for r in dead]
    for kw in ({}, {"where": "g >= 0"}):
        res = c.search_multi_vector(q, n, **kw)
        same(res, *expect(scores, has, n, ~np.isin(rows, dead)))
        assert not set(gone) & set(int(x) for x in res.ids())
    same(c.search_multi_vector(q, 20, where="g >= 2"), *expect(scores, has, 20, (rows % 5 >= 2) & ~np.isin(rows, dead)))


def test_batch_equals_singles(L):
    rng = np.random.default_rng(4)
    sets = int_sets(rng, rng.choice([0, 1, 31, 32, 33, 100], 150), 9)
    c = coll_of(L, sets)
    queries = [rng.integers(-3, 4, (tq, 9)).astype(f32) for tq in (1, 65, 32, 7, 129)]
    batch = c.batch_search_multi_vector(queries, 12)
    for q, b in zip(queries, batch):
        one = c.search_multi_vector(q, 12)
        same(b, *expect(*ref_scores(q, sets), 12))
        assert np.array_equal(one.ids(), b.ids()) and np.array_equal(one.distances().view(u32), b.distances().view(u32))


def test_nan_and_inf_tokens(L):
    """written out by hand, dim 2, query tokens (1, 0) and (0, 1):
    row 0: tokens (1, 2)              -> 1 + 2 = 3
    row 1: tokens (NaN, 5), (4, 1)    -> max(NaN, 4) + max(NaN, 1): the NaN products are skipped: 5
    row 2: token (NaN, NaN)           -> -inf + -inf = -inf
    row 3: token (inf, 0)             -> inf + NaN -> m = (inf, -inf): inf + -inf = NaN, reported -inf, ties with row 2 by row
    row 4: tokens (inf, 1), (0, 7)    -> max(inf, 0) + max(NaN, 7) = inf
    row 5: token (-inf, 1)            -> -inf + (NaN skipped: -inf) = -inf"""
    nan, inf = float("nan"), float("inf")
    sets = [np.array(t, f32) for t in ([[1, 2]], [[nan, 5], [4, 1]], [[nan, nan]], [[inf, 0]], [[inf, 1], [0, 7]], [[-inf, 1]])]
    q = np.array([[1, 0], [0, 1]], f32)
    c = coll_of(L, sets)
    same(c.search_multi_vector(q, 10), [4, 1, 0, 2, 3, 5], [inf, 5.0, 3.0, -inf, -inf, -inf])
    same(c.search_multi_vector(q, 10), *expect(*ref_scores(q, sets), 10))
