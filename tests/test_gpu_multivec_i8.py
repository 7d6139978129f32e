"""Multi-vector (MaxSim) search over an int8 token store against a numpy restatement of include/lynse_hip.h, INT8 TOKEN STORAGE, rules
1" - 4": every step is exact or one f32 rounding, so ids, order and score BITS must agree on arbitrary (Gaussian) data."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    return L_


def quant(x):
    """rule 1": -> (codes int64, scales f32)"""
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        amax = np.fmax.reduce(np.abs(x), axis=1, initial=f32(0))   # fmax skips a NaN
        ok = (amax > 0) & np.isfinite(amax)
        one = np.where(ok, amax, f32(1))
        inv, s = np.where(ok, f32(127) / one, f32(0)), np.where(ok, one / f32(127), f32(0))
        r = np.rint(x * inv[:, None])
    return np.where(np.isnan(r), 0, np.clip(r, -127, 127)).astype(np.int64), s.astype(f32)


def ref_scores(q, sets):
    """-> (scores f32 as reported, which records have tokens)"""
    lens = np.array([len(p) for p in sets])
    has, scores = lens > 0, np.full(len(sets), -np.inf, f32)
    (cp, sp), (cq, sq) = quant(np.concatenate([np.asarray(p, f32).reshape(len(p), -1) for p in sets if len(p)])), quant(q)
    v = (cq @ cp.T).astype(f32) * sp[None, :]                                                       # rule 2"
    m = sq[:, None] * np.maximum.reduceat(v, np.concatenate([[0], np.cumsum(lens[has])[:-1]]), axis=1)   # rule 3"
    T = np.zeros((-(-len(q) // 32) * 32, m.shape[1]), f32)
    T[:len(q)] = m
    T = T.reshape(-1, 32, m.shape[1])
    for _ in range(5):                                                                              # rule 4": the pairwise tree
        T = T[:, 0::2] + T[:, 1::2]
    acc = T[0, 0]
    for t in range(1, len(T)):
        acc = acc + T[t, 0]
    scores[has] = acc + f32(0.0)
    return scores, has


def expect(scores, has, k, keep=None):
    rows = np.nonzero(has if keep is None else has & keep)[0]
    o = rows[np.lexsort((rows, -scores[rows].astype(np.float64)))][:k]
    return o, scores[o]


def coll_of(L, sets, fields=None):
    """record row r has user id 3 r + 7 and the token set sets[r], in an int8 store"""
    ids = [3 * r + 7 for r in range(len(sets))]
    c = L.Collection("mvi", 4, device=0)
    c.add_items(np.ones((len(sets), 4), f32), ids, fields=fields)
    c.commit()
    c.add_multi_vectors(ids, sets, dtype="i8")
    return c


def same(res, rows, scores):
    assert res.index_mode() == "MULTIVEC-MAXSIM-IP-I8"
    assert [int(x) for x in res.ids()] == [3 * int(r) + 7 for r in rows]
    assert np.array_equal(res.distances().view(u32), np.asarray(scores, f32).view(u32)), (res.distances(), scores)


# record lengths around the 4-row hand-over and the block of 32, empty records, 40 one-token records (every row of a block ends one),
# and > 3 wave ranges with one record of 2,500 tokens (longer than a range)
EDGES = [3, 4, 5, 0, 8, 9, 31, 32, 33, 0, 1, 2, 7, 64, 30, 1, 1, 35]
CORPORA = {"edges": EDGES, "ones": [1] * 40 + [5, 0] + [1] * 30, "ranges": EDGES * 6 + [2500] + EDGES * 5 + [1200, 900, 40]}
CASES = [("edges", 1, ()), ("ones", 31, ()), ("edges", 32, ()), ("edges", 33, ()), ("ranges", 130, ()), ("edges", 520, (256,)), ("edges", 1024, (128,))]


@pytest.mark.parametrize("name,dim,more_tq", CASES)
def test_bits_equal_the_rules_on_gaussian_data(L, name, dim, more_tq):
    rng = np.random.default_rng(1000 * len(name) + dim)
    sets = [rng.standard_normal((t, dim)).astype(f32) for t in CORPORA[name]]
    c = coll_of(L, sets)
    assert c.multi_vector_dtype() == "i8"
    if name == "ranges":
        assert c.search_profile(None, 1, query_tokens=np.ones((1, dim), f32))["profile"]["device"]["multivec"]["ranges"] >= 4
    queries = [rng.standard_normal((tq, dim)).astype(f32) for tq in (1, 31, 32, 33, 64, 65) + more_tq]
    refs = [ref_scores(q, sets) for q in queries]
    for q, ref in zip(queries, refs):
        for k in (1, 10, len(sets) + 5):
            same(c.search_multi_vector(q, k), *expect(*ref, k))
    for res, ref in zip(c.batch_search_multi_vector(queries, 10), refs):   # one batch, differing token counts
        same(res, *expect(*ref, 10))


def test_largest_dot_product_is_exact(L):
    """dim 1024, +-1 with equal signs: d = 127^2 * 1024, the edge of rule 2" """
    rng = np.random.default_rng(2)
    sign = np.where(rng.random(1024) < 0.5, -1, 1).astype(f32)
    sets = [np.where(rng.random((3, 1024)) < 0.5, -1, 1).astype(f32), np.stack([sign, -sign]), sign[None, :]]
    scores, has = ref_scores(sign[None, :], sets)
    assert scores[1] == scores[2] == f32(127 * 127 * 1024) * f32(1 / 127) * f32(1 / 127)
    same(coll_of(L, sets).search_multi_vector(sign[None, :], 3), *expect(scores, has, 3))


# rule 1": a zero row, a NaN element, an inf element, ties of rintf (amax 127: inv = 1), and a subnormal amax whose inv overflows, so
# the products are +-inf and clamp (0 * inf = NaN codes as 0)
RULE1 = np.array([[0, 0, 0, 0], [1, np.nan, -2, 0.5], [1, np.inf, 2, 3], [127, 0.5, 1.5, -2.5], [1e-39, -1e-39, 0, 5e-40]], f32)


@pytest.mark.parametrize("how", ["tokens", "query"])
def test_rule_1_through_the_scores(L, how):
    rng = np.random.default_rng(3)
    codes, scales = quant(RULE1)
    assert [list(r) for r in codes] == [[0] * 4, [64, 0, -127, 32], [0] * 4, [127, 0, 2, -2], [127, -127, 0, 127]] and scales[0] == scales[2] == 0
    plain = rng.standard_normal((6, 4)).astype(f32)
    if how == "tokens":
        sets, queries = [r[None, :] for r in RULE1] + [RULE1, plain], [plain, plain[:1]]
    else:
        sets, queries = [plain[:2], plain[2:]], [r[None, :] for r in RULE1] + [RULE1]
    c = coll_of(L, sets)
    for q in queries:
        same(c.search_multi_vector(q, len(sets)), *expect(*ref_scores(q, sets), len(sets)))


def test_masks_never_return_masked_or_empty_records(L):
    rng = np.random.default_rng(4)
    lens = CORPORA["ranges"]
    sets, n = [rng.standard_normal((t, 7)).astype(f32) for t in lens], len(lens)
    c = coll_of(L, sets, fields=[{"g": int(r % 5)} for r in range(n)])
    q = rng.standard_normal((33, 7)).astype(f32)
    scores, has = ref_scores(q, sets)
    rows = np.arange(n)
    sub = rows[rng.random(n) < 0.5]
    same(c.search_multi_vector(q, n, subset=sub), *expect(scores, has, n, np.isin(rows, sub)))
    same(c.search_multi_vector(q, 20, where="g >= 2"), *expect(scores, has, 20, rows % 5 >= 2))
    dead = expect(scores, has, 6)[0]
    c.delete_items([3 * int(r) + 7 for r in dead])
    alive = ~np.isin(rows, dead)
    same(c.search_multi_vector(q, n), *expect(scores, has, n, alive))
    same(c.search_multi_vector(q, 20, subset=sub), *expect(scores, has, 20, np.isin(rows, sub) & alive))
    same(c.search_multi_vector(q, 20, where="g >= 2"), *expect(scores, has, 20, alive & (rows % 5 >= 2)))
    assert len(c.search_multi_vector(q, 5, subset=rows[~has])) == 0   # only records without tokens survive


def test_within_the_quantisers_worst_case_of_f64(L):
    """|q_ik - sq_i cq_ik| <= sq_i / 2 and likewise for p, so |q_i . p_j - sq_i s_j d_ij| <= B_ij = (sq_i / 2) |p_j|_1 + (s_j / 2) |q_i|_1
    + dim sq_i s_j / 4; a max moves by at most the largest B_ij of its record, the score by their sum over i; 1e-5 relative for the f32 steps."""
    rng = np.random.default_rng(5)
    dim, tq = 128, 32
    sets = [rng.standard_normal((t, dim)).astype(f32) for t in rng.choice([1, 5, 31, 33, 64], 80)]
    q = rng.standard_normal((tq, dim)).astype(f32)
    res = coll_of(L, sets).search_multi_vector(q, len(sets))
    assert len(res) == len(sets)
    sq = quant(q)[1].astype(np.float64)
    for rid, got in zip(res.ids(), res.distances()):
        p = sets[(int(rid) - 7) // 3].astype(np.float64)
        s = quant(p)[1].astype(np.float64)
        B = np.outer(sq / 2, np.abs(p).sum(1)) + np.outer(np.abs(q).sum(1, dtype=np.float64), s / 2) + dim * np.outer(sq, s) / 4
        exact = (q.astype(np.float64) @ p.T).max(1).sum()
        assert abs(float(got) - exact) <= B.max(1).sum() + 1e-5 * (np.abs(q).astype(np.float64) @ np.abs(p).T).max(1).sum()
