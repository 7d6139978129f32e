"""Multi-vector (MaxSim) search over an MXFP4 token store against numpy's restatement of include/lynse_hip.h, MXFP4 TOKEN STORAGE: rules
1''' / 1'''' dequantise, rule 2''' is their f64 product cast to f32, then the record max and the pairwise tree of rule 4'''.  On lossless
data (tokens on the E2M1 grid times a block's power of two, small integer queries) every partial sum is exact: score BITS must agree."""
import numpy as np
import pytest

import lynsedb_amd as L

pytestmark = pytest.mark.gpu
f32, u32 = np.float32, np.uint32
E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6])


def mx_blocks(x, shift):
    """-> (p * 2^-E as f64 [rows][blocks][32], 2^E): blocks over the zero-padded row, NaN skipped by amax and coded 0, a block whose
    amax is 0 or +inf all zero under a unit scale"""
    x = np.asarray(x, f32)
    x = np.pad(x, ((0, 0), (0, -x.shape[1] % 32))).reshape(len(x), -1, 32).astype(np.float64)
    with np.errstate(all="ignore"):
        amax = np.fmax.reduce(np.abs(x), axis=2, initial=0.0)
        ok = (amax > 0) & np.isfinite(amax)
        E = np.where(ok, np.clip(np.frexp(np.where(ok, amax, 1.0))[1] - 1 - shift, -127, 127), 0)   # floor(log2 amax) = frexp's exponent - 1
        v = np.where(ok[..., None], x * 2.0 ** -E[..., None], 0.0)
    return np.where(np.isnan(v), 0.0, v), 2.0 ** E[..., None]


def deq_tokens(x):
    """rule 1''': the nearest E2M1 value, a tie to the code whose low bit is 0, saturating at 6"""
    v, scale = mx_blocks(x, 2)
    d = np.abs(np.abs(v)[..., None] - E2M1)
    lo, hi = d.argmin(-1), 7 - d[..., ::-1].argmin(-1)   # the first and the last of the nearest codes: they differ on a tie
    return (np.sign(v) * E2M1[np.where(lo % 2 == 0, lo, hi)] * scale).reshape(len(v), -1)


def deq_query(x):
    """rule 1'''': nearest even at E4M3's 4 significant bits, whole steps of 2^-9 below 2^-6, saturating at 448"""
    v, scale = mx_blocks(x, 8)
    m, e = np.frexp(np.abs(v))
    r = np.where(np.abs(v) < 2.0 ** -6, np.rint(np.abs(v) * 512) / 512, np.ldexp(np.rint(m * 16) / 16, e))
    return (np.sign(v) * np.minimum(r, 448.0) * scale).reshape(len(v), -1)


def ref_scores(q, sets):
    """-> (scores f32 as reported, which records have tokens, f64 scores of the dequantised operands, sum_i max_j sum_k |q p|, sum_i |m_i|)"""
    lens = np.array([len(p) for p in sets])
    has, out = lens > 0, [np.full(len(sets), -np.inf, t) for t in (f32, np.float64, np.float64, np.float64)]
    P, Q = deq_tokens(np.concatenate([np.asarray(p, f32).reshape(len(p), -1) for p in sets if len(p)])), deq_query(q)
    starts = np.concatenate([[0], np.cumsum(lens[has])[:-1]])
    m = np.maximum.reduceat((Q @ P.T).astype(f32), starts, axis=1)   # rules 2''' and 3'''
    T = np.zeros((-(-len(Q) // 32) * 32, m.shape[1]), f32)
    T[:len(Q)] = m
    T = T.reshape(-1, 32, m.shape[1])
    for _ in range(5):                                               # rule 4''': the pairwise tree, then the tiles in order
        T = T[:, 0::2] + T[:, 1::2]
    acc = T[0, 0]
    for t in range(1, len(T)):
        acc = acc + T[t, 0]
    out[0][has], out[1][has] = acc + f32(0.0), np.maximum.reduceat(Q @ P.T, starts, axis=1).sum(0)
    out[2][has], out[3][has] = np.maximum.reduceat(np.abs(Q) @ np.abs(P).T, starts, axis=1).sum(0), np.abs(m.astype(np.float64)).sum(0)
    return (out[0], has, *out[1:])


def expect(ref, k, keep=None):
    rows = np.nonzero(ref[1] if keep is None else ref[1] & keep)[0]
    o = rows[np.lexsort((rows, -ref[0][rows].astype(np.float64)))][:k]
    return o, ref[0][o]


def coll_of(sets, fields=None):
    """record row r has user id 3 r + 7 and the token set sets[r], in an MXFP4 store"""
    ids = [3 * r + 7 for r in range(len(sets))]
    c = L.Collection("mvx", 4, device=0)
    c.add_items(np.ones((len(sets), 4), f32), ids, fields=fields)
    c.commit()
    c.add_multi_vectors(ids, sets, dtype="mxfp4")
    return c


def same(res, rows, scores):
    assert res.index_mode() == "MULTIVEC-MAXSIM-IP-MXFP4" and [int(x) for x in res.ids()] == [3 * int(r) + 7 for r in rows]
    assert np.array_equal(res.distances().view(u32), np.asarray(scores, f32).view(u32)), (res.distances(), scores)


def lossless_sets(rng, lens, dim):
    """tokens on the signed E2M1 grid times 2^e per block, e in {-1, 0, 1}; one block in ten is zero, every other holds a 4 or a 6 (E = e)"""
    out, nb = [], -(-dim // 32)
    for t in map(int, lens):
        x = rng.choice(E2M1, (t, nb * 32)) * rng.choice([-1.0, 1.0], (t, nb * 32))
        for b in range(nb):
            x[np.arange(t), 32 * b + rng.integers(0, min(32, dim - 32 * b), t)] = rng.choice([4.0, 6.0, -4.0, -6.0], t)
        x = x.reshape(t, nb, 32) * (2.0 ** rng.integers(-1, 2, (t, nb, 1))) * (rng.random((t, nb, 1)) >= 0.1)
        out.append(x.reshape(t, nb * 32)[:, :dim].astype(f32))
    return out


# §29's corpora: a record boundary on a 32-token block boundary, one token before and after it; > 3 wave ranges around a 2,500-token record
MIX = [0, 1, 31, 32, 33, 100]
CORPORA = {"one": [33], "two": [0, 100], "on_block": [32, 32, 1, 31, 32], "before": [31, 33, 0, 32], "after": [33, 31, 100, 1],
           "mixed300": lambda rng: rng.choice(MIX, 300), "ranges": lambda rng: np.concatenate([rng.choice(MIX, 120), [2500], rng.choice(MIX[1:], 60)])}


# dims: a partial block, exactly one, half a k-step and one column more, a whole k-step, a half-step tail, more than one chunk, many
@pytest.mark.parametrize("name,dim", [("one", 1), ("two", 31), ("on_block", 32), ("before", 33), ("after", 64), ("mixed300", 96), ("ranges", 130),
                                      ("ranges", 520)])
def test_score_bits_on_lossless_data(name, dim):
    rng = np.random.default_rng(len(name) * 1000 + dim)
    lens = CORPORA[name](rng) if callable(CORPORA[name]) else CORPORA[name]
    sets = lossless_sets(rng, lens, dim)
    c = coll_of(sets)
    assert c.multi_vector_dtype() == "mxfp4"
    if name == "ranges":
        assert c.search_profile(None, 1, query_tokens=np.ones((1, dim), f32))["profile"]["device"]["multivec"]["ranges"] >= 4
    for tq in (1, 31, 32, 33, 64, 65, 128, 129):   # (the plan serves 129 tokens up to dim 576)
        q = rng.integers(-3, 4, (tq, dim)).astype(f32)
        ref = ref_scores(q, sets)
        for k in (1, 10, len(sets) + 5):
            same(c.search_multi_vector(q, k), *expect(ref, k))


def around(ties):
    return np.array([[np.nextafter(f32(t), f32(0)), t, np.nextafter(f32(t), f32(1e9))] for t in ties], f32).reshape(-1)


@pytest.mark.parametrize("how", ["tokens", "query"])
def test_rule_1_through_the_scores(how):
    """A pilot in column 0 fixes E = 0 (4.0 in a token, 256 in a query), the probe sits in column 1, which alone is read on the other
    side (there an exact 1.0): every tie with its two neighbours, saturation, a subnormal, NaN, a zero block and one whose amax is +inf."""
    if how == "tokens":
        probes = np.concatenate([around([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]), f32([6.0, 7.9, -0.25, -1.25, -5.5, np.nan])])
        want = deq_tokens(np.stack([np.full(len(probes), 4.0, f32), probes], 1))[:, 1]
        assert list(want[1:21:3]) == [0, 1, 1, 2, 2, 4, 4] and list(want[:3]) == [0, 0, 0.5] and list(want[21:]) == [6, 6, 0, -1, -6, 0]
        sets = [np.array([[4.0, p]], f32) for p in probes] + [np.zeros((1, 2), f32), np.array([[np.inf, 1.0]], f32), np.full((1, 2), np.nan, f32)]
        queries = [np.array([[0, 1]], f32)]
    else:
        probes = np.concatenate([around([17.0, 19.0, 464.0, 2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9]), f32([448.0, 449.0, 500.0, 2.0 ** -9, 2.0 ** -6, -19.0, np.nan])])
        want = deq_query(np.stack([np.full(len(probes), 256.0, f32), probes], 1))[:, 1]
        assert list(want[1:19:3]) == [16, 20, 448, 0, 2.0 ** -8, 2.0 ** -8] and list(want[18:]) == [448, 448, 448, 2.0 ** -9, 2.0 ** -6, -20, 0]
        sets = [np.array([[0, 1.0]], f32), np.array([[0, -1.0]], f32)]
        queries = [np.array([[256.0, p]], f32) for p in probes] + [np.zeros((1, 2), f32), np.array([[np.inf, 1.0]], f32)]
    ref0 = [ref_scores(q, sets)[0][0] for q in queries] if how == "query" else ref_scores(queries[0], sets)[0]   # record 0 / query 0: the probes
    assert np.array_equal(np.array(ref0[:len(want)]), want.astype(f32) + f32(0)) and not np.any(ref0[len(want):])
    for q, res in zip(queries, coll_of(sets).batch_search_multi_vector(queries, len(sets))):
        same(res, *expect(ref_scores(q, sets), len(sets)))


def test_real_valued_data_within_the_summation_bound():
    """Against the f64 score of the DEQUANTISED operands: B = 2 (gamma(dim) mag + gamma(Tq) msum), u = 2^-24 — the products are exact,
    gamma over the adds of rules 2''' and 4''', and each add of the instruction is allowed a whole ulp instead of half (its internal
    rounding is not documented): the factor 2.  Measured on the MI355X: max error / bound = 0.019."""
    rng = np.random.default_rng(11)
    dim, tq, k, u = 128, 32, 10, 2.0 ** -24
    sets = [rng.standard_normal((int(t), dim)).astype(f32) for t in rng.choice(MIX[1:], 300)]
    gamma = lambda n: n * u / (1 - n * u)   # noqa: E731
    queries = [rng.standard_normal((tq, dim)).astype(f32) for _ in range(20)]
    for q, res in zip(queries, coll_of(sets).batch_search_multi_vector(queries, k)):
        _, _, exact, mag, msum = ref_scores(q, sets)
        B, got = 2 * (gamma(dim) * mag + gamma(tq) * msum), (res.ids() - 7) // 3
        err = np.abs(res.distances().astype(np.float64) - exact[got])
        print("max error / bound", float((err / B[got]).max()))
        assert len(res) == k and np.all(err <= B[got]) and np.all(exact[got] >= np.sort(exact)[-k] - 2 * B.max())


def test_masks_batch_and_rerank_equal_the_reference():
    rng = np.random.default_rng(3)
    lens = np.concatenate([rng.choice(MIX, 200), [2500], rng.choice([1, 33], 30)])
    sets, n = lossless_sets(rng, lens, 40), len(lens)
    c = coll_of(sets, fields=[{"g": int(r % 5)} for r in range(n)])
    queries = [rng.integers(-3, 4, (tq, 40)).astype(f32) for tq in (33, 1, 65, 7, 129)]
    refs, rows = [ref_scores(q, sets) for q in queries], np.arange(n)
    lists = [np.sort(rng.choice(n, m, replace=False)) for m in (1, 40, n, 3, 70)]
    reranked = c.batch_rerank_multi_vector(queries, [[3 * int(r) + 7 for r in cand] for cand in lists], 12)   # (the masked-scan route)
    for q, ref, b, cand, rr in zip(queries, refs, c.batch_search_multi_vector(queries, 12), lists, reranked):
        one = c.search_multi_vector(q, 12)
        same(b, *expect(ref, 12))
        assert np.array_equal(one.ids(), b.ids()) and np.array_equal(one.distances().view(u32), b.distances().view(u32))
        same(rr, *expect(ref, 12, np.isin(rows, cand)))
    q, ref, has = queries[0], refs[0], refs[0][1]
    second_range = (np.cumsum(lens) > 2048) & (np.cumsum(lens) <= 4096)   # every record of one wave range, and more
    sub = rows[rng.random(n) < 0.5]
    same(c.search_multi_vector(q, 20, subset=sub), *expect(ref, 20, np.isin(rows, sub)))
    same(c.search_multi_vector(q, n, subset=rows[:9]), *expect(ref, n, rows < 9))   # few tokens live: still the masked scan
    same(c.search_multi_vector(q, n, subset=L.BitSet.from_rows(rows[~second_range], n)), *expect(ref, n, ~second_range))
    same(c.search_multi_vector(q, 20, where="g >= 2"), *expect(ref, 20, rows % 5 >= 2))
    dead = expect(ref, 6)[0]
    c.delete_items([3 * int(r) + 7 for r in dead])
    alive = ~np.isin(rows, dead)
    same(c.search_multi_vector(q, 20, subset=sub), *expect(ref, 20, np.isin(rows, sub) & alive))
    assert len(c.search_multi_vector(q, 5, subset=rows[~has])) == 0   # only records without tokens survive
    assert c.compact() == len(dead)   # the ids it removes from the collection stay gone, filter or no filter
    for kw in ({}, {"where": "g >= 0"}):
        same(c.search_multi_vector(q, n, **kw), *expect(ref, n, alive))


def test_planted_record_comes_first_and_append_f16_is_refused():
    """A planted best token at every row of a block, for the first record (32 tokens), the last, the last and the first record of a
    wave range, and a record of 70 tokens that spans blocks; dim 64, so both lane halves carry data.  One store per planted token."""
    rng = np.random.default_rng(5)
    lens = np.concatenate([[32], rng.choice([31, 32, 33, 100], 80), [40, 70], rng.choice([1, 31, 33], 40), [33]])
    base = [rng.integers(-1, 2, (int(t), 64)).astype(f32) for t in lens]
    first_of_range = int(np.searchsorted(np.cumsum(lens), 2048, side="right"))   # the ranges close at 2,048 tokens: this record opens the second
    q = rng.integers(-1, 2, (33, 64)).astype(f32)
    q[:, 35], q[0] = 0, 0
    q[0, 35] = 1   # only query token 0 reads column 35 (the second block: the upper lane half)
    ref0 = ref_scores(q, base)
    for r in (0, len(lens) - 1, first_of_range - 1, first_of_range, 82):   # (82: the 70 tokens)
        for j in range(int(lens[r])):
            sets, scores = list(base), ref0[0].copy()
            sets[r] = base[r].copy()
            sets[r][j, 35] = 768.0   # 6 * 2^7: query token 0 gains 768 on this record alone (the +-1 of its block round to 0)
            scores[r] = ref_scores(q, [sets[r]])[0][0]
            rows, sc = expect((scores, ref0[1]), 3)
            idx = L.MultiVectorIndex(64, device=0, dtype="fp4")
            idx.append(sets)
            got_rows, got_sc, cnt = idx.search_batch_arrays([q], 3)
            assert rows[0] == r and sc[0] > 700 and cnt[0] == 3 and np.array_equal(got_rows[0], rows) and np.array_equal(got_sc[0].view(u32), sc.view(u32)), (r, j)
    halves, counts = np.ones((2, 64), np.float16), np.array([2], np.uint64)
    assert L._lib.lib.lynse_hip_multivec_append_f16(idx._h, halves.ctypes.data, counts.ctypes.data, 1) == 1 and "f16 handle only" in L._lib.last_error()
    assert idx.dtype == "mxfp4" and idx.counts()["records"] == len(lens)
