"""Multi-vector (MaxSim) search over an f16 token store against numpy (include/lynse_hip.h, F16 TOKEN STORAGE): both sides rounded
to binary16 with subnormals flushed (rule 1'), an f64 product cast to f32, the max over a record's tokens, the f32 sum of rule 4.
Integer-valued inputs are exact in f16 and make every partial sum exact, so there the answer must match bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32, u32, f16 = np.float32, np.uint32, np.float16


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    return L_


def h16(x):
    """rule 1': nearest-even to binary16, a subnormal result to a zero of its sign; returned as f64"""
    with np.errstate(over="ignore"):
        b = np.asarray(x).astype(f16).view(np.uint16)
    return np.where(b & 0x7C00, b, b & 0x8000).astype(np.uint16).view(f16).astype(np.float64)


def ref_scores(q, sets, products=False):
    """-> (scores f32 as reported: NaN as -inf, -0 as +0; which records have tokens[; the f64 scores, sum_i max_j sum_k |q_ik p_jk|, sum_i |m_i|])"""
    lens = np.array([len(p) for p in sets])
    has, scores = lens > 0, np.full(len(sets), -np.inf, f32)
    P = h16(np.concatenate([np.asarray(p).reshape(len(p), -1) for p, h in zip(sets, has) if h]))
    Q = h16(q)
    starts = np.concatenate([[0], np.cumsum(lens[has])[:-1]])
    with np.errstate(invalid="ignore", over="ignore"):
        s64 = Q @ P.T
        s = s64.astype(f32)                                                        # rule 2'
        m = np.maximum.reduceat(np.where(np.isnan(s), -np.inf, s), starts, axis=1)   # rule 3
        acc = m[0].copy()
        for i in range(1, len(m)):                                              # rule 4: ((m_0 + m_1) + m_2) + ...
            acc = (acc + m[i]).astype(f32)
    scores[has] = np.where(np.isnan(acc), -np.inf, acc) + f32(0.0)
    if not products:
        return scores, has
    exact, mag, msum = (np.full(len(sets), -np.inf), np.full(len(sets), np.inf), np.full(len(sets), np.inf))
    exact[has] = np.maximum.reduceat(s64, starts, axis=1).sum(axis=0)
    mag[has] = np.maximum.reduceat(np.abs(Q) @ np.abs(P).T, starts, axis=1).sum(axis=0)
    msum[has] = np.abs(m.astype(np.float64)).sum(axis=0)
    return scores, has, exact, mag, msum


def expect(scores, has, k, keep=None):
    rows = np.nonzero(has if keep is None else has & keep)[0]
    o = rows[np.lexsort((rows, -scores[rows].astype(np.float64)))][:k]
    return o, scores[o]


def coll_of(L, sets, fields=None):
    """record row r has user id 3 r + 7 and the token set sets[r], in an f16 store"""
    n = len(sets)
    c = L.Collection("mvh", 4, device=0)
    c.add_items(np.ones((n, 4), f32), [3 * r + 7 for r in range(n)], fields=fields)
    c.commit()
    c.add_multi_vectors([3 * r + 7 for r in range(n)], sets, dtype="f16")
    return c


def same(res, rows, scores):
    assert res.index_mode() == "MULTIVEC-MAXSIM-IP-F16"
    assert [int(x) for x in res.ids()] == [3 * int(r) + 7 for r in rows]
    assert np.array_equal(res.distances().view(u32), np.asarray(scores, f32).view(u32)), (res.distances(), scores)


def int_sets(rng, lens, dim):
    return [rng.integers(-3, 4, (int(t), dim)).astype(f32) for t in lens]


# a record boundary exactly on a 32-token block boundary (32 | 32), one token before it (31 | 33) and after (33 | 31)
CORPORA = {"one": [33], "two": [0, 100], "on_block": [32, 32, 1, 31, 32], "before": [31, 33, 0, 32], "after": [33, 31, 100, 1]}


def corpus(name, rng):
    if name == "mixed300":
        return rng.choice([0, 1, 31, 32, 33, 100], 300)
    if name == "ranges":   # > 3 wave ranges of ~2,048 tokens, one record of 2,500 tokens (longer than a range) in the middle
        return np.concatenate([rng.choice([0, 1, 31, 32, 33, 100], 120), [2500], rng.choice([1, 31, 32, 33, 100], 60)])
    return CORPORA[name]


@pytest.mark.parametrize("name,dim", [("one", 1), ("two", 2), ("on_block", 7), ("before", 128), ("after", 130), ("mixed300", 17), ("ranges", 130),
                                      ("ranges", 520)])
def test_exact_on_integer_data(L, name, dim):
    rng = np.random.default_rng(len(name) * 1000 + dim)
    sets = int_sets(rng, corpus(name, rng), dim)
    c = coll_of(L, sets)
    assert c.multi_vector_dtype() == "f16"
    if name == "ranges":
        assert c.search_profile(None, 1, query_tokens=np.ones((1, dim), f32))["profile"]["device"]["multivec"]["ranges"] >= 4
    for tq in (1, 31, 32, 33, 64, 65):
        q = rng.integers(-3, 4, (tq, dim)).astype(f32)
        scores, has = ref_scores(q, sets)
        for k in (1, 10, len(sets) + 5):
            same(c.search_multi_vector(q, k), *expect(scores, has, k))


# rule 1': ties to even (2049 -> 2048, 2051 -> 2052), the overflow edge (65519 -> 65504, 65520 -> inf), the least normal kept, values
# below it flushed with their sign (-0 is reported +0), NaN -> a record that scores -inf
RULE1 = np.array([2049, 2051, 65519, 65520, 2.0 ** -14, 0.99 * 2.0 ** -14, 2.0 ** -15, -(2.0 ** -15), np.nan], f32)


@pytest.mark.parametrize("how", ["tokens_f32", "tokens_f16", "query"])
def test_rule_1_through_the_scores(L, how):
    one = np.ones((1, 1), f32)
    with np.errstate(over="ignore"):
        given = RULE1.astype(f16) if how == "tokens_f16" else RULE1   # (raw halves: 2^-15 arrives as a subnormal and must be flushed)
    want = h16(given).astype(f32)
    want = np.where(np.isnan(want), -np.inf, want).astype(f32) + f32(0.0)
    assert list(want[:5]) == [2048, 2052, 65504, np.inf, 2.0 ** -14] and list(want[5:]) == [0, 0, 0, -np.inf]
    idx = L.MultiVectorIndex(1, device=0, dtype="f16")
    if how == "query":
        idx.append([one])
        rows, scores, counts = idx.search_batch_arrays([v.reshape(1, 1) for v in RULE1], 1)
        assert list(counts) == [1] * len(RULE1) and not rows.any()
        assert np.array_equal(scores[:, 0].view(u32), want.view(u32)), (scores[:, 0], want)
    else:
        idx.append([v.reshape(1, 1) for v in given])
        rows, scores, counts = idx.search_batch_arrays([one], len(given))
        o = np.lexsort((np.arange(len(want)), -want.astype(np.float64)))
        assert counts[0] == len(given) and np.array_equal(rows[0], o)
        assert np.array_equal(scores[0].view(u32), want[o].view(u32)), (scores[0], want[o])


def test_append_f16_needs_an_f16_handle(L):
    import ctypes as C

    idx = L.MultiVectorIndex(4, device=0)
    assert idx.dtype == "f32"
    tokens, counts = np.ones((2, 4), f16), np.array([2], np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L._lib.lib.lynse_hip_multivec_append_f16(idx._h, p(tokens), p(counts), 1) == 1 and "f16 handle only" in L._lib.last_error()
    assert idx.counts() == {"records": 0, "tokens": 0, "ranges": 0}


def test_planted_record_comes_first(L):
    """A planted best match at every token of a record — so at every column lane of a block — for row 0 (32 tokens), the last row,
    the last and the first record of a wave range, and a record of 70 tokens that spans blocks.  One store per planted token."""
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
            idx = L.MultiVectorIndex(16, device=0, dtype="f16")
            idx.append(sets)
            got_rows, got_sc, cnt = idx.search_batch_arrays([q], 3)
            assert cnt[0] == 3 and np.array_equal(got_rows[0], rows) and np.array_equal(got_sc[0].view(u32), sc.view(u32)), (r, j)


def test_real_valued_data_within_the_summation_bound(L):
    """B = 2 (gamma(dim) mag + gamma(Tq) msum), u = 2^-24: the products are exact, and each f32 add of the instruction is allowed a
    whole ulp (truncation) instead of half, since its internal rounding is not documented here — hence the factor 2."""
    rng = np.random.default_rng(11)
    dim, tq, k, u = 128, 32, 10, 2.0 ** -24
    sets = [rng.standard_normal((int(t), dim)).astype(f32) for t in rng.choice([1, 31, 32, 33, 100], 300)]
    c = coll_of(L, sets)
    gamma = lambda n: n * u / (1 - n * u)   # noqa: E731
    qualified, queries = 0, [rng.standard_normal((tq, dim)).astype(f32) for _ in range(20)]
    for q, res in zip(queries, c.batch_search_multi_vector(queries, k)):
        _, has, exact, mag, msum = ref_scores(q, sets, products=True)
        B = 2 * (gamma(dim) * mag + gamma(tq) * msum)
        got_rows = (res.ids() - 7) // 3
        err = np.abs(res.distances().astype(np.float64) - exact[got_rows])
        print("max error / bound", float((err / B[got_rows]).max()))
        assert len(res) == k and np.all(err <= B[got_rows])
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
    alive = ~np.isin(rows, dead)
    same(c.search_multi_vector(q, 20), *expect(scores, has, 20, alive))
    same(c.search_multi_vector(q, 20, subset=sub), *expect(scores, has, 20, np.isin(rows, sub) & alive))
    assert len(c.search_multi_vector(q, 5, subset=rows[~has])) == 0   # only records without tokens survive
    assert c.compact() == len(dead)   # the ids it removes from the collection stay gone, filter or no filter
    for kw in ({}, {"where": "g >= 0"}):
        same(c.search_multi_vector(q, n, **kw), *expect(scores, has, n, alive))
    same(c.search_multi_vector(q, 20, where="g >= 2"), *expect(scores, has, 20, (rows % 5 >= 2) & alive))


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
