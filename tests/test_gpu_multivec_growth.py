"""A multi-vector store built by several appends answers as the same records appended at once: the second append regrows the token
block (its capacity is the first call's total, 97 rows; the held rows are copied on the device into a block of 194) and the third lands
in the spare rows of the grown block (169 + 5 <= 194).  Every other multi-vector test builds its store in one append."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32, u32, f16 = np.float32, np.uint32, np.float16

DIM = 40                                   # ld = 64: the padding columns exist
LENS = [33, 0, 1, 31, 32, 70, 0, 2, 5]
SPLIT = [(0, 5), (5, 8), (8, 9)]
KS = (1, 4, 20)


@pytest.fixture(scope="module")
def L():
    import lynsedb_amd as L_

    return L_


@pytest.fixture(scope="module")
def queries():
    rng = np.random.default_rng(41)
    return [rng.standard_normal((t, DIM)).astype(f32) for t in (1, 33, 65)]


@pytest.fixture(scope="module", params=["f32", "f16", "i8"])
def pair(request, L):
    """-> (dtype, the store of one append, the store of three)"""
    dtype = request.param
    rng = np.random.default_rng(40)
    sets = [rng.standard_normal((t, DIM)).astype(f32) for t in LENS]
    if dtype == "f16":   # the middle append goes up as raw halves (append_f16); the single append stores the same halves from f32
        a, b = SPLIT[1]
        sets[a:b] = [s.astype(f16) for s in sets[a:b]]
    once, grown = L.MultiVectorIndex(DIM, device=0, dtype=dtype), L.MultiVectorIndex(DIM, device=0, dtype=dtype)
    once.append(sets)
    for a, b in SPLIT:
        grown.append(sets[a:b])
    return dtype, once, grown


def same(x, y):
    (r1, s1, c1), (r2, s2, c2) = x, y
    assert np.array_equal(c1, c2)
    assert np.array_equal(r1, r2)
    assert np.array_equal(s1.view(u32), s2.view(u32))


def test_counts_agree(pair):
    _, once, grown = pair
    assert once.counts() == grown.counts()
    assert once.counts()["records"] == len(LENS) and once.counts()["tokens"] == sum(LENS)


@pytest.mark.parametrize("masked", [False, True])
def test_search_agrees(L, pair, queries, masked):
    _, once, grown = pair
    words = L.BitSet.from_rows(np.array([0, 3, 5, 8], np.uint64), len(LENS)).words if masked else None
    live = 4 if masked else sum(1 for t in LENS if t)
    for k in KS:
        x, y = once.search_batch_arrays(queries, k, words), grown.search_batch_arrays(queries, k, words)
        same(x, y)
        assert np.all(x[2] == min(k, live))


def test_rerank_agrees(pair, queries):
    dtype, once, grown = pair
    if dtype == "f32":
        return   # an f32 store has no candidate kernel: its rerank is the masked scan above
    lists = [[0, 5, 8], [1, 2]]   # record 1 has no tokens
    for qs in (queries[:2], queries[1:]):
        for k in KS:
            x, y = once.rerank_batch_arrays(qs, lists, k), grown.rerank_batch_arrays(qs, lists, k)
            same(x, y)
            assert list(x[2]) == [min(k, 3), 1]
