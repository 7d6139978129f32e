"""MaxSim over per-query candidate lists (k_maxsim_cand_h16 / _i8) against numpy restatements of the stores' rules over the candidates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32, u32, f16 = np.float32, np.uint32, np.float16
MODE = {"f32": "MULTIVEC-MAXSIM-IP", "f16": "MULTIVEC-MAXSIM-IP-F16", "i8": "MULTIVEC-MAXSIM-IP-I8"}


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    return L_


def h16(x):
    """rule 1': nearest-even to binary16, a subnormal result to a zero of its sign; as f64"""
    b = np.asarray(x).astype(f16).view(np.uint16)
    return np.where(b & 0x7C00, b, b & 0x8000).astype(np.uint16).view(f16).astype(np.float64)


def quant(x):
    """rule 1": -> (codes int64, scales f32) of rows with a finite, positive amax"""
    amax = np.abs(np.asarray(x, f32)).max(axis=1)
    return np.clip(np.rint(x * (f32(127) / amax)[:, None]), -127, 127).astype(np.int64), (amax / f32(127)).astype(f32)


def ref_scores(q, sets, dtype):
    """-> (scores f32 per record, -inf for a record without tokens; the f64 scores and the magnitudes of the summation bound for f16)"""
    lens = np.array([len(p) for p in sets])
    has, scores = lens > 0, np.full(len(sets), -np.inf, f32)
    starts = np.concatenate([[0], np.cumsum(lens[has])[:-1]])
    P = np.concatenate([p for p in sets if len(p)])
    if dtype == "i8":   # rules 2" - 4": one multiply by each scale, the pairwise tree within a tile of 32, the tiles in order
        (cp, sp), (cq, sq) = quant(P), quant(q)
        m = sq[:, None] * np.maximum.reduceat((cq @ cp.T).astype(f32) * sp[None, :], starts, axis=1)
        T = np.zeros((-(-len(q) // 32) * 32, m.shape[1]), f32)
        T[:len(q)] = m
        T = T.reshape(-1, 32, m.shape[1])
        for _ in range(5):
            T = T[:, 0::2] + T[:, 1::2]
        acc = T[0, 0]
        for t in range(1, len(T)):
            acc = acc + T[t, 0]
        scores[has] = acc + f32(0.0)
        return scores, None, None
    Q, P = h16(q), h16(P)   # rules 2' - 4: an f64 product cast to f32, the max, ((m_0 + m_1) + m_2) + ... in f32
    m = np.maximum.reduceat((Q @ P.T).astype(f32), starts, axis=1)
    acc = m[0].copy()
    for i in range(1, len(m)):
        acc = (acc + m[i]).astype(f32)
    scores[has] = acc + f32(0.0)
    exact, bound = np.full(len(sets), -np.inf), np.full(len(sets), np.inf)
    gamma = lambda n: n * 2.0 ** -24 / (1 - n * 2.0 ** -24)   # noqa: E731  (the bound of test_real_valued_data_within_the_summation_bound)
    exact[has] = np.maximum.reduceat(Q @ P.T, starts, axis=1).sum(axis=0)
    bound[has] = 2 * (gamma(q.shape[1]) * np.maximum.reduceat(np.abs(Q) @ np.abs(P).T, starts, axis=1).sum(axis=0) + gamma(len(q)) * np.abs(m.astype(np.float64)).sum(axis=0))
    return scores, exact, bound


def coll_of(L, sets, dtype):
    """record row r has user id 3 r + 7 and the token set sets[r]"""
    ids = [3 * r + 7 for r in range(len(sets))]
    c = L.Collection("mvr", 4, device=0)
    c.add_items(np.ones((len(sets), 4), f32), ids)
    c.commit()
    c.add_multi_vectors(ids, sets, dtype=dtype)
    return c


def expect(scores, rows, k):
    rows = np.unique(np.array([r for r in rows if scores[r] > -np.inf], dtype=np.int64))
    return rows[np.lexsort((rows, -scores[rows].astype(np.float64)))][:k]


ids_of = lambda rows: [3 * int(r) + 7 for r in rows]   # noqa: E731


# every block shape of a record (0, 1, 31, 32, 33, 100 tokens and 79 blocks), token-less records at both kinds of neighbours
LENS = [33, 0, 1, 31, 32, 100, 2500, 0, 70, 33, 1, 32, 100, 31]
# one candidate; one workgroup of 4; 5; every record; record 0 + the last + token-less ones + a row twice; nothing that scores; nothing
LISTS = [[6], [0, 2, 5, 13], [0, 2, 3, 6, 13], list(range(14)), [13, 0, 1, 7, 0, 4], [1, 7], []]
CASES = [("f16", "int", d) for d in (1, 7, 128, 130)] + [("i8", "gauss", d) for d in (1, 7, 128, 130, 520)] + [("f16", "gauss", 128), ("f32", "int", 7)]


@pytest.mark.parametrize("dtype,data,dim", CASES)
def test_rerank_equals_the_reference_over_the_candidates(L, dtype, data, dim):
    rng = np.random.default_rng(dim + len(dtype))
    draw = (lambda *s: rng.standard_normal(s).astype(f32)) if data == "gauss" else (lambda *s: rng.integers(-3, 4, s).astype(f32))
    sets = [draw(t, dim) for t in LENS]
    c = coll_of(L, sets, dtype)
    queries = [draw(tq, dim) for tq in (1, 32, 33, 65)]
    refs = [ref_scores(q, sets, "f16" if dtype == "f32" else dtype) for q in queries]   # (integer data: an f32 store sums exactly too)
    full = [c.search_multi_vector(q, len(LENS)) for q in queries] if dtype == "i8" else None

    def check(res, qi, rows, k):
        scores, exact, bound = refs[qi]
        assert res.index_mode() == MODE[dtype]
        if data == "gauss" and dtype == "f16":   # the order inside an MFMA is the hardware's: the summation bound, not bits
            got = (res.ids() - 7) // 3
            err = np.abs(res.distances().astype(np.float64) - exact[got])
            scored = expect(scores, rows, len(LENS))
            assert len(got) == min(k, len(scored)) and set(got) <= set(scored) and np.all(err <= bound[got])
            return
        want = expect(scores, rows, k)
        assert [int(x) for x in res.ids()] == ids_of(want), (qi, rows, k)
        assert np.array_equal(res.distances().view(u32), scores[want].view(u32)), (res.distances(), scores[want])
        if full is not None:   # the scan's bits for the same records
            at = {int(i): s for i, s in zip(full[qi].ids(), full[qi].distances().view(u32))}
            assert [at[int(i)] for i in res.ids()] == list(res.distances().view(u32))

    for qi, q in enumerate(queries):
        for rows in LISTS:
            for k in (None, 2):
                check(c.rerank_multi_vector(q, ids_of(rows), k), qi, rows, len(LENS) if k is None else k)
    # one batch: every query its own list and its own token count
    for qi, res in enumerate(c.batch_rerank_multi_vector(queries, [ids_of(LISTS[(qi + 1) % 5]) for qi in range(4)])):
        check(res, qi, LISTS[(qi + 1) % 5], len(LENS))


@pytest.mark.parametrize("dtype", ["f16", "i8"])
def test_planted_token_wins_at_every_row_of_a_block(L, dtype):
    """One store holds, for every row j of a 33- and a 70-token record, a copy with the best token planted at j, next to decoys; query j
    reranks [decoys, copy j]: every lane, register and block position wins once.  > 256 queries: one workgroup each, its waves stride."""
    rng = np.random.default_rng(7)
    draw = (lambda *s: rng.standard_normal(s).astype(f32)) if dtype == "i8" else (lambda *s: rng.integers(-1, 2, s).astype(f32))
    decoys = [draw(t, 16) for t in (40, 33, 1, 100, 70, 31, 32)]
    bases = [draw(33, 16), draw(70, 16)]
    q = draw(33, 16)
    sets, lists = list(decoys), []
    for b in bases:
        for j in range(len(b)):
            p = b.copy()
            p[j] = 100 * q[0]   # query token 0 gains 100 |q_0|^2 on this record alone
            lists.append(list(range(len(decoys))) + [len(sets)])
            sets.append(p)
    c = coll_of(L, sets, dtype)
    scores = ref_scores(q, sets, dtype)[0]
    out = c.batch_rerank_multi_vector([q] * (3 * len(lists)), [ids_of(rows) for rows in lists] * 3, 3)
    assert len(out) > 256
    for res, rows in zip(out, lists * 3):
        want = expect(scores, rows, 3)
        assert want[0] == rows[-1] and [int(x) for x in res.ids()] == ids_of(want), rows[-1]
        assert np.array_equal(res.distances().view(u32), scores[want].view(u32))


@pytest.mark.parametrize("dtype", ["i8", "f16"])
def test_a_small_subset_runs_the_candidate_kernel_with_the_scans_bits(L, dtype):
    """Gaussian data: a filtered search of three rows is routed and returns the unfiltered scan's bits (f16: the reason it is routed)"""
    rng = np.random.default_rng(9)
    sets = [rng.standard_normal((t, 24)).astype(f32) for t in [1, 31, 33, 0, 32, 100] * 60]
    c, q = coll_of(L, sets, dtype), rng.standard_normal((33, 24)).astype(f32)
    full = c.search_multi_vector(q, len(sets))
    # 260 queries, every record listed: one workgroup a query, 75 items a wave (more than the 64 whose extents the lanes hold at once)
    for res in c.batch_rerank_multi_vector([q] * 260, [ids_of(range(len(sets)))] * 260)[::37]:
        assert np.array_equal(res.ids(), full.ids()) and np.array_equal(res.distances().view(u32), full.distances().view(u32))
    at = {int(i): s for i, s in zip(full.ids(), full.distances().view(u32))}
    prof = c.search_profile(None, 5, query_tokens=q, subset=[0, 1, 2])
    assert prof["profile"]["index_path"] == "multivec_candidates" and prof["profile"]["device"]["multivec"]["scan_rows"] == 65
    res = c.search_multi_vector(q, 5, subset=[0, 1, 2])
    assert sorted(int(i) for i in res.ids()) == [7, 10, 13] and [at[int(i)] for i in res.ids()] == list(res.distances().view(u32))
    assert list(res.distances()) == sorted(res.distances(), reverse=True)
    assert c.search_profile(None, 5, query_tokens=q, subset=np.arange(180))["profile"]["index_path"] == "multivec_scan"   # half the store


def test_rows_past_the_store_are_refused(L):
    idx, one = L.MultiVectorIndex(8, device=0, dtype="i8"), np.ones((1, 8), f32)
    idx.append([np.ones((2, 8), f32), one])
    with pytest.raises(ValueError, match="is not a record"):
        idx.rerank_batch_arrays([one], [[0, 2]], 1)
    rows, scores, counts = idx.rerank_batch_arrays([one, one], [[], [1]], 4)
    assert list(counts) == [0, 1] and rows[1, 0] == 1
